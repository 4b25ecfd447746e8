/*
 * qr_fan.hpp - occlusion fans (include/qrhip.h qr_fan_rays_async / qr_fan_views_async / qr_fan_hits_async): from every surface
 * point a fan of K visibility rays along a direction table shared by all points, answered as the number of open directions per
 * point and, if wanted, one bit per direction.  Ambient occlusion, sky and sun visibility, openness of lightmap texels and probes.
 *
 * One kernel template, three sources of the surface point (pos, nrm, id): fan_element below, which the framed fan and the
 * gather kernels call for all three and this kernel for caller rays and records (its view branch keeps the text):
 *   SRC = QR_FAN_SRC_RAYS   the first hit of the caller's qr_ray i, the hit record's (qr_hitrec.hpp): lane i of workgroup g is
 *                           ray g * 64 + i, traverse<false, DIVK, true>, then surface_point.
 *   SRC = QR_FAN_SRC_VIEW   the first hit of a pixel of a caller-supplied camera, the hit record's again: the grid is
 *                           (footprint columns, footprint rows, views), a footprint is 8x8 pixels, sample 0's ray under FSAA.
 *   SRC = QR_FAN_SRC_HITS   the caller's qr_hit record i: pos, nrm and id are read (two of its three 16-byte pieces), no first walk.
 * The hit stays in registers: no record and no ray ever reaches memory.
 *
 * The fan loop is wave-uniform over k.  dirs[k] is read with scalar loads through the constant address space (the table is the
 * same for every lane, as a qr_view record is for a view launch).  Per lane: dot = (nrm.x * d.x + nrm.y * d.y) + nrm.z * d.z (three
 * products, two adds, never fused); without `flip` the direction is traced iff 0 < dot (the renderer's rule for lights, LT_amb);
 * with `flip` every direction is traced, as -d where dot < 0.  A ballot of the traced lanes skips the walk when it is empty (a
 * floor under a direction that points down).  The walk is traverse<true, DIVK, true> on DevHeader::off_query with the ballot as
 * `active`: the occlusion query's walk (qr_query.hpp), the ray (pos, eps, +-d, reach), no originating surface.  A count register
 * and a mask register collect the answers; the mask word is stored after every 32nd direction and after the last, into plane
 * k >> 5 of `mask` (uint32 [planes][elements]: a wave of caller rays or records stores 256 contiguous bytes).
 *
 * `coherent` of the fan walks (packet walks allowed on long hierarchies): the rays of one direction leave neighbouring points in
 * the same direction where the points are neighbours and nothing is flipped -- a view, or caller rays under QR_TRACE_COHERENT,
 * without `flip`: the situation of the shadow rays of primary hits, which the renderer walks as packets.  With `flip` neighbours on
 * a curved surface part into d and -d, and caller rays or records vouch for nothing: those walk per lane on long hierarchies.
 * Results do not depend on it.  No LDS of its own (the hand-over pool of the per-lane walks is traverse's).
 */
#ifndef QR_FAN_HPP
#define QR_FAN_HPP

#include <float.h>

#define QR_FAN_SRC_RAYS 0
#define QR_FAN_SRC_VIEW 1
#define QR_FAN_SRC_HITS 2

/* src: the qr_ray array (RAYS) or the qr_hit array (HITS); n: their element count; elems: elements of the launch (the stride of
 * a mask plane); flip != 0: QR_FAN_FLIP; mask may be null */
struct FanP
{
    const qr_fan_dir *dirs;
    int32_t k;
    uint32_t flip;
    float eps, reach;           /* reach: already FLT_MAX for +inf */
    int32_t *open;
    uint32_t *mask;
    uint64_t elems;
};

/* This lane's element of a fan launch and its surface point: rec, pos, nrm, and has (a surface point: id >= 0); returns whether
 * the lane is inside the launch.  RAYS and VIEW: launch_ray (qr_hitrec.hpp), the first walk -- traverse<false, DIVK, true> on
 * DevHeader::off_query, coherent for a view or where the caller vouches for it -- and surface_point for the lanes that hit.
 * HITS: two of record i's three 16-byte pieces, no walk; n > 0: a lane past the end reads record 0 and traces nothing. */
template <int SRC, bool DIVK, bool COHERENT>
__device__ __forceinline__ bool fan_element(BaseP B, const char *G, const f32x4 *__restrict__ src, int32_t n, const ViewsP &vp,
                                            size_t &rec, V3 &pos, V3 &nrm, bool &has, WalkStats stats)
{
    bool active;
    pos = {0.0f, 0.0f, 0.0f}; nrm = {0.0f, 0.0f, 0.0f};
    if constexpr (SRC == QR_FAN_SRC_HITS)
    {
        const int64_t i = (int64_t)blockIdx.x * QR_BLOCK + (int64_t)threadIdx.x;
        active = i < (int64_t)n;
        const int64_t q = active ? i : 0;
        const f32x4 a = src[3 * q], b = src[3 * q + 1];
        pos = {a.x, a.y, a.z};
        nrm = {b.x, b.y, b.z};
        has = active && __float_as_int(b.w) >= 0;
        rec = (size_t)q;
    }
    else
    {
        const FrmP fr = c_frm(B);
        Ray r;
        active = launch_ray<SRC == QR_FAN_SRC_VIEW>(fr, G, src, n, vp, r, rec);
        r.list = active ? fr->off_query : 0u;

        Hit h;
        bool occ0 = false;
        traverse<false, DIVK, true>(B, active, SRC == QR_FAN_SRC_VIEW || COHERENT, r, h, occ0, stats);
        has = active && h.srf != 0;
        if (has)
        {
            V3 tex; u32 mo;
            surface_point(G, fr->off_shade, r, h, pos, nrm, tex, mo);
        }
    }
    return active;
}

/* direction d4 of the table as an element with normal n traces it: dot = (n.x * d.x + n.y * d.y) + n.z * d.z; with `flip` the
 * direction is mirrored where dot < 0 (a NaN dot is not) and every element with a surface point traces it; without, it is traced
 * iff 0 < dot (LT_amb: a NaN dot is closed) */
__device__ __forceinline__ bool fan_dir(const f32x4 d4, const V3 n, const bool has, const uint32_t flip, V3 &dir, float &dot)
{
    float x1 = n.x * d4.x, x2 = n.y * d4.y, x3 = n.z * d4.z;
    x1 = x1 + x2;
    dot = x1 + x3;
    if (flip != 0u)
    {
        const bool neg = dot < 0.0f;
        dir.x = neg ? -d4.x : d4.x; dir.y = neg ? -d4.y : d4.y; dir.z = neg ? -d4.z : d4.z;
        return has;
    }
    dir = {d4.x, d4.y, d4.z};
    return has && 0.0f < dot;
}

template <int SRC, bool DIVK, bool COHERENT>
__global__ __launch_bounds__(QR_BLOCK, DIVK && SRC != QR_FAN_SRC_HITS ? QR_DIVK_WAVES : QR_MIN_WAVES_PER_SIMD)
void qr_fan_kernel(const char *__restrict__ blob, const f32x4 *__restrict__ src, int32_t n, ViewsP vp, FanP fp,
                   unsigned long long *__restrict__ stats)
{
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const BaseP B = (BaseP)blob;
    const QR_CONST f32x4 *dirs = (const QR_CONST f32x4 *)fp.dirs;
#pragma clang diagnostic pop
    const FrmP fr = c_frm(B);
    bool active;
    size_t rec;                                 /* this lane's element */
    V3 pos = {0.0f, 0.0f, 0.0f}, nrm = {0.0f, 0.0f, 0.0f};
    bool has = false;                           /* a surface point: id >= 0 */
    if constexpr (SRC == QR_FAN_SRC_VIEW)
    {
        /* fan_element's view branch -- launch_ray<true>, the first walk, surface_point -- kept here as text (DESIGN.md 4s:
         * through the functions the view instances' assembly changed and one of them measured slower) */
        Ray r;
        {
            const u32 ord = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x | (blockIdx.y << 14)));
            const int view = __builtin_amdgcn_readfirstlane((int)blockIdx.z);
            int x, y, k;
            active = pixel_of_view(ord, 0, vp, x, y, k);
            float ha, va;
            sample_offsets(fr, blob, fr->fr.fsaa, x, k, ha, va);
            float hs = (float)x + ha; hs = hs + 0.0f;
            float vs = (float)y + va; vs = vs + 0.0f;
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
            const QR_CONST qr_view *vw = (const QR_CONST qr_view *)vp.views + view;
#pragma clang diagnostic pop
            view_ray(vw, hs, vs, r);
            rec = ((size_t)view * (size_t)vp.height + (size_t)(active ? y : 0)) * (size_t)vp.width + (size_t)(active ? x : 0);
        }
        r.list = active ? fr->off_query : 0u;

        Hit h;
        bool occ0 = false;
        traverse<false, DIVK, true>(B, active, SRC == QR_FAN_SRC_VIEW || COHERENT, r, h, occ0, stats);
        has = active && h.srf != 0;
        if (has)
        {
            V3 tex; u32 mo;
            surface_point(blob, fr->off_shade, r, h, pos, nrm, tex, mo);
        }
    }
    else active = fan_element<SRC, DIVK, COHERENT>(B, blob, src, n, vp, rec, pos, nrm, has, stats);

    /* the fan: every lane of the wave stays in the loop (the walks are wave-wide), lanes without a surface point trace nothing */
    const bool coherent = (SRC == QR_FAN_SRC_VIEW || COHERENT) && fp.flip == 0u;
    const u32 qlist = fr->off_query;
    int count = 0;
    u32 word = 0;
    for (int k = 0; k < fp.k; k++)
    {
        const f32x4 d4 = dirs[k];                   /* wave-uniform: one scalar load */
        Ray f;
        float dot;
        const bool traced = fan_dir(d4, nrm, has, fp.flip, f.dir, dot);
        bool open = false;
        if (LM(traced) != 0)
        {
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

#endif /* QR_FAN_HPP */
