/*
 * qr_gather.hpp - gather fans (include/qrhip.h qr_gather_rays_async / qr_gather_views_async / qr_gather_hits_async): from every
 * surface point a fan of K SHADED rays along a direction table shared by all points, answered as one weighted sum of the
 * renderer's colours per point.  Final gather, one-bounce diffuse irradiance, lightmap and probe baking, sky light weighted by
 * visibility, glossy pre-integration.  The partner of the occlusion fans (qr_fan.hpp): what a host would otherwise compose from
 * hit records, N x K qr_ray rows, qr_shade_rays_async and a reduction.
 *
 * One kernel template on the fans' three sources of the surface point (SRC = QR_FAN_SRC_RAYS / _VIEW / _HITS; fan_element,
 * qr_fan.hpp), a wave-uniform loop over k with scalar loads of dirs[k], the fans' dot product and traced rule (fan_dir), and
 * the ballot that skips a direction no lane traces.  Inside the loop the wave runs the
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

/* the fold of one traced direction into the lane's parked sums (words 6..10 of column l): wgt = w, times cz (mirrored with it
 * under `flip`) with QR_GATHER_COSINE; acc.rgb = acc.rgb + col.rgb * wgt, one fp32 multiply, then one fp32 add; acc.w = acc.w + wgt;
 * cnt += 1.  cz: the cosine between the direction and the normal, as the kernel has it */
__device__ __forceinline__ void gather_fold(float (*g)[64], const int l, const V3 col, const float w, const float cz, const GatherP &gp)
{
    float wgt = w;
    if (gp.cosine != 0u)
    {
        const float c = (gp.flip != 0u && cz < 0.0f) ? -cz : cz;
        wgt = wgt * c;
    }
    const float pr = col.x * wgt, pg = col.y * wgt, pb = col.z * wgt;
    g[6][l] = g[6][l] + pr;
    g[7][l] = g[7][l] + pg;
    g[8][l] = g[8][l] + pb;
    g[9][l] = g[9][l] + wgt;
    g[10][l] = __int_as_float(__float_as_int(g[10][l]) + 1);
}

/* the end of a gather kernel: every lane inside the launch stores its row (one 16-byte store) and its count; zeros and -1
 * without a surface point */
template <int SRC>
__device__ __forceinline__ void gather_store(float (*g)[64], const lm_t in_mask, const lm_t has_mask, const ViewsP &vp, const GatherP &gp)
{
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
            acc = {g[6][lane_e], g[7][lane_e], g[8][lane_e], g[9][lane_e]};
            cnt = __float_as_int(g[10][lane_e]);
        }
        gp.gather[rec] = acc;
        gp.count[rec] = cnt;
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
    /* pos xyz, nrm xyz, acc rgbw, cnt (its bits): [word][lane] */
    __shared__ float lds_g[11][64];
    lm_t in_mask, has_mask;                     /* lanes inside the launch; lanes with a surface point */
    {
        size_t rec;                             /* this lane's element */
        V3 pos, nrm;
        bool has = false;
        const bool active = fan_element<SRC, DIVK, COHERENT>(B, lp.B, src, n, vp, rec, pos, nrm, has, lp.stats);

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
            const V3 nrm = {lds_g[3][lane_s], lds_g[4][lane_s], lds_g[5][lane_s]};
            const bool traced = fan_dir(d4, nrm, ((has_mask >> lane_s) & 1ull) != 0ull, gp.flip, f.dir, dot);
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
        const V3 nrm = {lds_g[3][lane_s], lds_g[4][lane_s], lds_g[5][lane_s]};
        V3 dir;
        float dot;
        if (fan_dir(d4, nrm, ((has_mask >> lane_s) & 1ull) != 0ull, gp.flip, dir, dot)) gather_fold(lds_g, lane_s, col, d4.w, dot, gp);
    }
    gather_store<SRC>(lds_g, in_mask, has_mask, vp, gp);
}

#endif /* QR_GATHER_HPP */
