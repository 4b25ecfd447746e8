/*
 * qr_fan_framed.hpp - framed fans (include/qrhip.h qr_fan_*_framed_async / qr_gather_*_framed_async): the occlusion fans
 * (qr_fan.hpp) and the gather fans (qr_gather.hpp) with the direction table given in every surface point's OWN frame -- local +z
 * is the element's normal -- and, if wanted, turned about the normal by a caller-supplied spin (c, sn) per element.  A
 * cosine-distributed hemisphere about the normal, no direction wasted below the surface, a per-pixel rotation of the kernel.
 *
 * The frame, once per element (fan_frame): the branchless orthonormal basis of Duff et al. 2017 in a fixed operation order,
 *   s = nz < 0 ? -1 : 1;  a = -1 / (s + nz);  b = (nx * ny) * a;
 *   t = (1 + ((s * nx) * nx) * a,  s * b,  -(s * nx));   bt = (b,  s + (ny * ny) * a,  -ny);
 *   u = t * c + bt * sn;   v = bt * c - t * sn            (per component: two products, then one add or subtract)
 * all fp32, the division IEEE, nothing fused; no spin is (1, 0) through the same operations.  The frame is VALID iff every word
 * of n, u and v has |w| <= FLT_MAX; an element with an invalid frame traces nothing.
 *
 * Per direction (x, y, z, w) of the table (wave-uniform: scalar loads, as in the unframed kernels): dot = z, the table's own
 * cosine; the mirror under `flip` ((-x, -y, -z) where z < 0) and the rule without it (0 < z) are wave-uniform too, so a row that
 * points below the surface is skipped by the whole wave; d = (u * x' + v * y') + n * z' per component, three products and two
 * adds in that order: 9 multiplies and 6 adds per lane.  Elements (fan_element), the fold and the final store
 * (gather_fold, gather_store) are the unframed kernels' own functions (qr_fan.hpp, qr_gather.hpp).
 *
 * Two kernel templates with symbols of their own (the unframed kernels' assembly stays as it was), five instances each, chosen
 * as the unframed calls choose theirs.  The fan kernel keeps u and v in six more registers across the loop and has no LDS of its
 * own.  The gather kernel parks the spin beside the eleven words qr_gather_kernel parks (13 words per lane, 3328 B per wave) and
 * computes the frame again from the parked normal and spin before every traced direction -- the same operations on the same
 * words: the same bits as a parked u, v, for one division and two dozen operations next to a shaded ray, and 1024 B of LDS per
 * wave less, which keeps the eleventh workgroup on a compute unit.  The fold after render_wave needs nothing of the
 * frame: the traced rule is a ballot bit and z, the weight is w and z.
 *
 * `coherent` of the fan rounds: the unframed rule and no spin (spun neighbours do not share a direction).  Results do not
 * depend on it.
 */
#ifndef QR_FAN_FRAMED_HPP
#define QR_FAN_FRAMED_HPP

#include <float.h>

/* the element's frame from its normal and spin; returns whether it is valid */
__device__ __forceinline__ bool fan_frame(const V3 n, const float c, const float sn, V3 &u, V3 &v)
{
    const float s = n.z < 0.0f ? -1.0f : 1.0f;         /* -0.0 and NaN give +1 */
    const float a = -1.0f / (s + n.z);
    const float b = (n.x * n.y) * a;
    const float sx = s * n.x;
    const V3 t = {1.0f + (sx * n.x) * a, s * b, -sx};
    const V3 bt = {b, s + (n.y * n.y) * a, -n.y};
    float p, q;
    p = t.x * c; q = bt.x * sn; u.x = p + q;
    p = t.y * c; q = bt.y * sn; u.y = p + q;
    p = t.z * c; q = bt.z * sn; u.z = p + q;
    p = bt.x * c; q = t.x * sn; v.x = p - q;
    p = bt.y * c; q = t.y * sn; v.y = p - q;
    p = bt.z * c; q = t.z * sn; v.z = p - q;
    /* a NaN fails every comparison */
    return __builtin_fabsf(n.x) <= FLT_MAX && __builtin_fabsf(n.y) <= FLT_MAX && __builtin_fabsf(n.z) <= FLT_MAX
        && __builtin_fabsf(u.x) <= FLT_MAX && __builtin_fabsf(u.y) <= FLT_MAX && __builtin_fabsf(u.z) <= FLT_MAX
        && __builtin_fabsf(v.x) <= FLT_MAX && __builtin_fabsf(v.y) <= FLT_MAX && __builtin_fabsf(v.z) <= FLT_MAX;
}

/* row k of the table as the wave traces it: mirrored where z < 0 under `flip`; returns the rule without the element's part
 * (flip, or 0 < z: a NaN z is closed without flip and traced unmirrored with it).  Wave-uniform. */
__device__ __forceinline__ bool framed_row(const f32x4 d4, const uint32_t flip, V3 &l)
{
    if (flip != 0u)
    {
        const bool neg = d4.z < 0.0f;
        l.x = neg ? -d4.x : d4.x; l.y = neg ? -d4.y : d4.y; l.z = neg ? -d4.z : d4.z;
        return true;
    }
    l = {d4.x, d4.y, d4.z};
    return 0.0f < d4.z;
}

/* d = (u * x' + v * y') + n * z' */
__device__ __forceinline__ V3 framed_dir(const V3 u, const V3 v, const V3 n, const V3 l)
{
    V3 d;
    float p, q, r;
    p = u.x * l.x; q = v.x * l.y; r = n.x * l.z; p = p + q; d.x = p + r;
    p = u.y * l.x; q = v.y * l.y; r = n.y * l.z; p = p + q; d.y = p + r;
    p = u.z * l.x; q = v.z * l.y; r = n.z * l.z; p = p + q; d.z = p + r;
    return d;
}

/* ---- the occlusion fan with the frame; spin: float [elements][2] or null ---- */

template <int SRC, bool DIVK, bool COHERENT>
__global__ __launch_bounds__(QR_BLOCK, DIVK && SRC != QR_FAN_SRC_HITS ? QR_DIVK_WAVES : QR_MIN_WAVES_PER_SIMD)
void qr_fan_framed_kernel(const char *__restrict__ blob, const f32x4 *__restrict__ src, int32_t n, ViewsP vp, FanP fp,
                          const float2 *__restrict__ spin, unsigned long long *__restrict__ stats)
{
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const BaseP B = (BaseP)blob;
    const QR_CONST f32x4 *dirs = (const QR_CONST f32x4 *)fp.dirs;
#pragma clang diagnostic pop
    size_t rec;                                 /* this lane's element */
    V3 pos, nrm;
    bool has = false;
    const bool active = fan_element<SRC, DIVK, COHERENT>(B, blob, src, n, vp, rec, pos, nrm, has, stats);

    /* the frame: rec is inside the launch for every lane (element 0 for the lanes past it) */
    float c = 1.0f, sn = 0.0f;
    if (spin != nullptr)
    {
        const float2 s2 = spin[rec];
        c = s2.x; sn = s2.y;
    }
    V3 u, v;
    const bool framed = fan_frame(nrm, c, sn, u, v) && has;     /* a surface point with a valid frame */

    /* the fan: every lane of the wave stays in the loop (the walks are wave-wide), lanes without a frame trace nothing */
    const bool coherent = (SRC == QR_FAN_SRC_VIEW || COHERENT) && fp.flip == 0u && spin == nullptr;
    const u32 qlist = c_frm(B)->off_query;
    int count = 0;
    u32 word = 0;
    for (int k = 0; k < fp.k; k++)
    {
        const f32x4 d4 = dirs[k];                   /* wave-uniform: one scalar load */
        V3 l;
        const bool traced = framed_row(d4, fp.flip, l) && framed;
        bool open = false;
        if (LM(traced) != 0)
        {
            Ray f;
            f.dir = framed_dir(u, v, nrm, l);
            f.org = pos; f.tmin = fp.eps; f.tmax = fp.reach;
            f.list = traced ? qlist : 0u;
            f.osrf = 0; f.oflg = 0;
            f.ploc = {0.0f, 0.0f, 0.0f};
            Hit fh;
            bool occ = false;
            traverse<true, DIVK, true>(B, traced, coherent, f, fh, occ, stats);
            open = traced && !occ;
        }
        /* the end of direction k: kept as text in both fan kernels (as a function it cost the view instances time) */
        count += open ? 1 : 0;
        word |= (open ? 1u : 0u) << (k & 31);
        if ((k & 31) == 31 || k == fp.k - 1)
        {
            if (fp.mask != nullptr && active) fp.mask[(size_t)(k >> 5) * (size_t)fp.elems + rec] = word;
            word = 0;
        }
    }
    if (active) fp.open[rec] = has ? count : -1;
}

/* ---- the gather fan with the frame ---- */

template <int SRC, bool DIVK, bool COHERENT, int WAVES>
__global__ __launch_bounds__(QR_BLOCK, WAVES)
void qr_gather_framed_kernel(LaunchP lp, const f32x4 *__restrict__ src, int32_t n, ViewsP vp, GatherP gp,
                             const float2 *__restrict__ spin)
{
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const BaseP B = (BaseP)lp.B;
    const QR_CONST f32x4 *dirs = (const QR_CONST f32x4 *)gp.dirs;
#pragma clang diagnostic pop
    /* pos xyz, nrm xyz, acc rgbw, cnt (its bits), spin c sn: [word][lane] */
    __shared__ float lds_g[13][64];
    lm_t in_mask, has_mask, frm_mask;           /* lanes inside the launch; with a surface point; with a valid frame as well */
    {
        size_t rec;                             /* this lane's element */
        V3 pos, nrm;
        bool has = false;
        const bool active = fan_element<SRC, DIVK, COHERENT>(B, lp.B, src, n, vp, rec, pos, nrm, has, lp.stats);

        /* the frame's validity is decided here, once; u and v are computed again where a direction is traced */
        float c = 1.0f, sn = 0.0f;
        if (spin != nullptr)
        {
            const float2 s2 = spin[rec];            /* inside the launch for every lane */
            c = s2.x; sn = s2.y;
        }
        V3 u, v;
        const bool framed = fan_frame(nrm, c, sn, u, v) && has;

        /* the start: zeros, or with QR_GATHER_RESUME the element's row and count (an element that traces nothing reads none) */
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        int cnt = 0;
        if (gp.resume != 0u && framed)
        {
            acc = gp.gather[rec];
            cnt = gp.count[rec];
        }
        const int lane = (int)(threadIdx.x & 63u);
        lds_g[0][lane] = pos.x; lds_g[1][lane] = pos.y; lds_g[2][lane] = pos.z;
        lds_g[3][lane] = nrm.x; lds_g[4][lane] = nrm.y; lds_g[5][lane] = nrm.z;
        lds_g[6][lane] = acc.x; lds_g[7][lane] = acc.y; lds_g[8][lane] = acc.z; lds_g[9][lane] = acc.w;
        lds_g[10][lane] = __int_as_float(cnt);
        lds_g[11][lane] = c; lds_g[12][lane] = sn;
        in_mask = LM(active);
        has_mask = LM(has);
        frm_mask = LM(framed);
    }

    /* the fan: every lane of the wave stays in the loop (the walks are wave-wide), lanes without a frame trace nothing */
    const bool coherent = (SRC == QR_FAN_SRC_VIEW || COHERENT) && gp.flip == 0u && spin == nullptr;
#pragma nounroll
    for (int k = 0; k < gp.k; k++)
    {
        V3 col = {0.0f, 0.0f, 0.0f};
        {
            const f32x4 d4 = dirs[k];               /* wave-uniform: one scalar load */
            int lane_s = (int)(threadIdx.x & 63u);
            asm volatile("" : "+v"(lane_s));
            V3 l;
            const bool traced = framed_row(d4, gp.flip, l) && ((frm_mask >> lane_s) & 1ull) != 0ull;
            if (LM(traced) == 0) continue;          /* a row below the surface, or a wave without frames */
            const V3 nrm = {lds_g[3][lane_s], lds_g[4][lane_s], lds_g[5][lane_s]};
            V3 u, v;
            (void)fan_frame(nrm, lds_g[11][lane_s], lds_g[12][lane_s], u, v);
            Ray f;
            f.dir = framed_dir(u, v, nrm, l);
            f.org = {lds_g[0][lane_s], lds_g[1][lane_s], lds_g[2][lane_s]};
            f.tmin = gp.eps; f.tmax = gp.reach;
            f.list = 0u; f.osrf = 0; f.oflg = 0;
            f.ploc = {0.0f, 0.0f, 0.0f};
            render_wave<false, DIVK, false, 10>(lp, 0u, 0u, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &col, nullptr,
                                                nullptr, traced, 0u, &f, coherent);
        }
        /* the fold: nothing of the direction or the frame was kept through the recursion, and nothing of the frame is needed */
        const f32x4 d4 = dirs[k];
        int lane_s = (int)(threadIdx.x & 63u);
        asm volatile("" : "+v"(lane_s));
        if (((frm_mask >> lane_s) & 1ull) != 0ull) gather_fold(lds_g, lane_s, col, d4.w, d4.z, gp);
    }
    gather_store<SRC>(lds_g, in_mask, has_mask, vp, gp);
}

#endif /* QR_FAN_FRAMED_HPP */
