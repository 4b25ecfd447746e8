/*
 * qr_gather.hpp - gather fans (include/qrhip.h qr_gather_rays_async / qr_gather_views_async / qr_gather_hits_async): from every
 * surface point a fan of K SHADED rays along a direction table shared by all points, answered as one weighted sum of the
 * renderer's colours per point.  Final gather, one-bounce diffuse irradiance, lightmap and probe baking, sky light weighted by
 * visibility, glossy pre-integration.  The partner of the occlusion fans (qr_fan.hpp): what a host would otherwise compose from
 * hit records, N x K qr_ray rows, qr_shade_rays_async and a reduction.
 *
 * One kernel template, the fan kernel's three sources of the surface point (SRC = QR_FAN_SRC_RAYS / _VIEW / _HITS), its element
 * set-up, first walk and surface_point, its wave-uniform loop over k with scalar loads of dirs[k], its dot product and traced
 * rule, and its ballot that skips a direction no lane traces: all unchanged in arithmetic.  Inside the loop the wave runs the
 * renderer's machine on the fan rays (render_wave RAYS = 10, qr_kernel.hpp): lane i's ray is (pos, eps, +-d, reach), handed over
 * in registers, a lane that does not trace the direction is a lane past n.  Its colour comes back in a register and is folded
 * into the lane's sum: wgt = weight (* |dot| or dot with QR_GATHER_COSINE), acc.rgb = acc.rgb + col.rgb * wgt (one fp32 multiply,
 * then one fp32 add, never fused), acc.w = acc.w + wgt, cnt += 1.  An untraced direction does nothing.
 *
 * What must survive a render_wave call -- position, normal, the four accumulators and the count: 11 words per lane -- waits in
 * LDS (2816 B per wave), as the running sum does in qr_views_mean_kernel, whose comment records what registers live across the
 * recursion cost in spills.  Everything else is computed again after the call, each time through an opaque copy of the lane
 * index: dirs[k] (a scalar load), the dot product (the same operations on the same words: the same bits), the element's index.
 * Which lanes have a surface point and which are inside the launch are two ballots (wave-uniform: scalar registers).
 *
 * `coherent` of the first walk and of the fan rounds' first round: the fan kernel's rule (a view, or caller rays under
 * QR_TRACE_COHERENT; in the fan without QR_FAN_FLIP only).  The walk instances are chosen as qr_shade_rays_kernel (caller rays,
 * caller records: the per-lane walks) and qr_render_views_kernel (views: the scene's) choose theirs.  Results depend on neither.
 */
#ifndef QR_GATHER_HPP
#define QR_GATHER_HPP

#include <float.h>

/* cosine != 0: QR_GATHER_COSINE; resume != 0: QR_GATHER_RESUME; the rest as FanP */
struct GatherP
{
    const qr_gather_dir *dirs;
    int32_t k;
    uint32_t flip, cosine, resume;
    float eps, reach;           /* reach: already FLT_MAX for +inf */
    f32x4 *gather;
    int32_t *count;
};

/* this lane's element of the launch, through opaque copies of its inputs (not address registers kept alive through the fan) */
template <int SRC>
__device__ __forceinline__ size_t gather_element(const ViewsP &vp)
{
    if constexpr (SRC == QR_FAN_SRC_VIEW)
    {
        const u32 ord = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x | (blockIdx.y << 14)));
        const int view = __builtin_amdgcn_readfirstlane((int)blockIdx.z);
        int x, y, k;
        const bool in = pixel_of_view(ord, 0, vp, x, y, k);
        return ((size_t)view * (size_t)vp.height + (size_t)(in ? y : 0)) * (size_t)vp.width + (size_t)(in ? x : 0);
    }
    else
    {
        int lane = (int)threadIdx.x;
        asm volatile("" : "+v"(lane));
        return (size_t)((int64_t)blockIdx.x * QR_BLOCK + (int64_t)lane);
    }
}

template <int SRC, bool DIVK, bool COHERENT, int WAVES>
__global__ __launch_bounds__(QR_BLOCK, WAVES)
void qr_gather_kernel(LaunchP lp, const f32x4 *__restrict__ src, int32_t n, ViewsP vp, GatherP gp)
{
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const BaseP B = (BaseP)lp.B;
    const QR_CONST f32x4 *dirs = (const QR_CONST f32x4 *)gp.dirs;
#pragma clang diagnostic pop
    const FrmP fr = c_frm(B);
    /* pos xyz, nrm xyz, acc rgbw, cnt (its bits): [word][lane] */
    __shared__ float lds_g[11][64];
    lm_t in_mask, has_mask;                     /* lanes inside the launch; lanes with a surface point */
    {
        bool active;
        size_t rec;                             /* this lane's element */
        V3 pos = {0.0f, 0.0f, 0.0f}, nrm = {0.0f, 0.0f, 0.0f};
        bool has = false;                       /* a surface point: id >= 0 */

        if constexpr (SRC == QR_FAN_SRC_HITS)
        {
            const int64_t i = (int64_t)blockIdx.x * QR_BLOCK + (int64_t)threadIdx.x;
            active = i < (int64_t)n;
            const int64_t q = active ? i : 0;       /* n > 0: lanes past the end read record 0 and trace nothing */
            const f32x4 a = src[3 * q], b = src[3 * q + 1];
            pos = {a.x, a.y, a.z};
            nrm = {b.x, b.y, b.z};
            has = active && __float_as_int(b.w) >= 0;
            rec = (size_t)q;
        }
        else
        {
            Ray r;
            if constexpr (SRC == QR_FAN_SRC_VIEW)
            {
                /* qr_hit_kernel's VIEW branch: one lane per pixel of an 8x8 footprint, sample 0's offsets at the frame's FSAA */
                const u32 ord = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x | (blockIdx.y << 14)));
                const int view = __builtin_amdgcn_readfirstlane((int)blockIdx.z);
                int x, y, k;
                active = pixel_of_view(ord, 0, vp, x, y, k);
                float ha, va;
                sample_offsets(fr, lp.B, fr->fr.fsaa, x, k, ha, va);
                float hs = (float)x + ha; hs = hs + 0.0f;
                float vs = (float)y + va; vs = vs + 0.0f;
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
                const QR_CONST qr_view *vw = (const QR_CONST qr_view *)vp.views + view;
#pragma clang diagnostic pop
                view_ray(vw, hs, vs, r);
                rec = ((size_t)view * (size_t)vp.height + (size_t)(active ? y : 0)) * (size_t)vp.width + (size_t)(active ? x : 0);
            }
            else
            {
                const int64_t i = (int64_t)blockIdx.x * QR_BLOCK + (int64_t)threadIdx.x;
                active = i < (int64_t)n;
                const int64_t q = active ? i : 0;   /* n > 0: lanes past the end read ray 0 and do not walk */
                const f32x4 a = src[2 * q], b = src[2 * q + 1];
                r.org = {a.x, a.y, a.z}; r.tmin = a.w;
                r.dir = {b.x, b.y, b.z};
                r.tmax = b.w > FLT_MAX ? FLT_MAX : b.w;
                r.osrf = 0; r.oflg = 0;
                r.ploc = {0.0f, 0.0f, 0.0f};
                rec = (size_t)q;
            }
            r.list = active ? fr->off_query : 0u;

            Hit h;
            bool occ0 = false;
            traverse<false, DIVK, true>(B, active, SRC == QR_FAN_SRC_VIEW || COHERENT, r, h, occ0
#ifdef QR_STATS
                                        , lp.stats
#endif
                                        );
            has = active && h.srf != 0;
            if (has)
            {
                V3 tex; u32 mo;
                surface_point(lp.B, fr->off_shade, r, h, pos, nrm, tex, mo);
            }
        }

        /* the start: zeros, or with QR_GATHER_RESUME the element's row and count (an element without a surface point reads none) */
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        int cnt = 0;
        if (gp.resume != 0u && has)
        {
            acc = gp.gather[rec];
            cnt = gp.count[rec];
        }
        const int lane = (int)(threadIdx.x & 63u);
        lds_g[0][lane] = pos.x; lds_g[1][lane] = pos.y; lds_g[2][lane] = pos.z;
        lds_g[3][lane] = nrm.x; lds_g[4][lane] = nrm.y; lds_g[5][lane] = nrm.z;
        lds_g[6][lane] = acc.x; lds_g[7][lane] = acc.y; lds_g[8][lane] = acc.z; lds_g[9][lane] = acc.w;
        lds_g[10][lane] = __int_as_float(cnt);
        in_mask = LM(active);
        has_mask = LM(has);
    }

    /* direction k for this lane, from LDS and the table: the fan kernel's dot product, traced rule and direction */
    auto fan_dir = [&](const f32x4 d4, const int lane_s, V3 &dir, float &dot) -> bool {
        const bool has = ((has_mask >> lane_s) & 1ull) != 0ull;
        const float nx = lds_g[3][lane_s], ny = lds_g[4][lane_s], nz = lds_g[5][lane_s];
        float x1 = nx * d4.x, x2 = ny * d4.y, x3 = nz * d4.z;
        x1 = x1 + x2;
        dot = x1 + x3;
        if (gp.flip != 0u)
        {
            const bool neg = dot < 0.0f;            /* a NaN dot is not flipped */
            dir.x = neg ? -d4.x : d4.x; dir.y = neg ? -d4.y : d4.y; dir.z = neg ? -d4.z : d4.z;
            return has;
        }
        dir = {d4.x, d4.y, d4.z};
        return has && 0.0f < dot;                   /* LT_amb: a NaN dot is closed */
    };

    /* the fan: every lane of the wave stays in the loop (the walks are wave-wide), lanes without a surface point trace nothing */
    const bool coherent = (SRC == QR_FAN_SRC_VIEW || COHERENT) && gp.flip == 0u;
#pragma nounroll
    for (int k = 0; k < gp.k; k++)
    {
        V3 col = {0.0f, 0.0f, 0.0f};
        {
            const f32x4 d4 = dirs[k];               /* wave-uniform: one scalar load */
            int lane_s = (int)(threadIdx.x & 63u);
            asm volatile("" : "+v"(lane_s));
            Ray f;
            float dot;
            const bool traced = fan_dir(d4, lane_s, f.dir, dot);
            if (LM(traced) == 0) continue;          /* a floor under a direction that points down */
            f.org = {lds_g[0][lane_s], lds_g[1][lane_s], lds_g[2][lane_s]};
            f.tmin = gp.eps; f.tmax = gp.reach;
            f.list = 0u; f.osrf = 0; f.oflg = 0;
            f.ploc = {0.0f, 0.0f, 0.0f};
            render_wave<false, DIVK, false, 10>(lp, 0u, 0u, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &col, nullptr,
                                                nullptr, traced, 0u, &f, coherent);
        }
        /* the fold: nothing of the direction was kept through the recursion */
        const f32x4 d4 = dirs[k];
        int lane_s = (int)(threadIdx.x & 63u);
        asm volatile("" : "+v"(lane_s));
        V3 dir;
        float dot;
        if (fan_dir(d4, lane_s, dir, dot))
        {
            float wgt = d4.w;
            if (gp.cosine != 0u)
            {
                const float c = (gp.flip != 0u && dot < 0.0f) ? -dot : dot;
                wgt = wgt * c;
            }
            const float pr = col.x * wgt, pg = col.y * wgt, pb = col.z * wgt;
            lds_g[6][lane_s] = lds_g[6][lane_s] + pr;
            lds_g[7][lane_s] = lds_g[7][lane_s] + pg;
            lds_g[8][lane_s] = lds_g[8][lane_s] + pb;
            lds_g[9][lane_s] = lds_g[9][lane_s] + wgt;
            lds_g[10][lane_s] = __int_as_float(__float_as_int(lds_g[10][lane_s]) + 1);
        }
    }

    int lane_e = (int)(threadIdx.x & 63u);
    asm volatile("" : "+v"(lane_e));
    if (((in_mask >> lane_e) & 1ull) != 0ull)
    {
        const size_t rec = gather_element<SRC>(vp);
        const bool has = ((has_mask >> lane_e) & 1ull) != 0ull;
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        int cnt = -1;
        if (has)
        {
            acc = {lds_g[6][lane_e], lds_g[7][lane_e], lds_g[8][lane_e], lds_g[9][lane_e]};
            cnt = __float_as_int(lds_g[10][lane_e]);
        }
        gp.gather[rec] = acc;                       /* one 16-byte store per lane */
        gp.count[rec] = cnt;
    }
}

#endif /* QR_GATHER_HPP */
