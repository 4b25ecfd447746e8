/*
 * qr_query.hpp - ray queries (include/qrhip.h qr_trace_rays_async / qr_occluded_async): closest hit or occlusion of
 * caller-supplied rays against the snapshot's global list, compiled into the image by QR_UPLOAD_RAY_QUERIES
 * (DevHeader::off_query).
 *
 * One lane per ray, 64 rays per wave (one wave per workgroup, QR_BLOCK).  Every lane reads its 32-byte qr_ray with two
 * 16-byte loads (consecutive lanes, consecutive rays: the wave reads 2 KB in one pass) and walks the query list through
 * the renderer's own `traverse` (qr_walk.hpp) -- packet walk, per-lane walk, hand-over pool and uniform grid are chosen
 * there exactly as for the renderer's rays, nothing is forked.  All lanes share one list head, so a wave takes the packet
 * walk unless the list is a long hierarchy and the caller does not vouch for coherence (QR_TRACE_COHERENT).  Results are
 * stored per lane, coalesced: float t and int32 id, or one byte of occlusion.
 *
 * A query ray has no originating surface: osrf = 0 (0 is never a DSurf offset, QR_OFF_SRF = 256) and oflg = 0, so the
 * walk's self-exclusion of secondary rays never applies; callers step off a surface with tmin.
 */
#ifndef QR_QUERY_HPP
#define QR_QUERY_HPP

#include <float.h>

/* the caller's qr_ray q, everything but the list: two 16-byte loads (consecutive lanes, consecutive rays).  No originating
 * surface.  +inf is taken as FLT_MAX (what the engine's cameras use): the walk scales the depth bound (w.tbuf * 1.000001,
 * w.tbuf * dd), and with +inf a zero factor would give NaN.  (render_wave keeps its own copy: its assembly is what bench.py times.) */
__device__ __forceinline__ void caller_ray(const f32x4 *__restrict__ rays, const int64_t q, Ray &r)
{
    const f32x4 a = rays[2 * q], b = rays[2 * q + 1];
    r.org = {a.x, a.y, a.z}; r.tmin = a.w;
    r.dir = {b.x, b.y, b.z};
    r.tmax = b.w > FLT_MAX ? FLT_MAX : b.w;
    r.osrf = 0; r.oflg = 0;
    r.ploc = {0.0f, 0.0f, 0.0f};
}

template <bool SHADOW, bool COHERENT>
__global__ __launch_bounds__(QR_BLOCK, SHADOW ? QR_MIN_WAVES_PER_SIMD : QR_DIVK_WAVES)
void qr_trace_kernel(const char *__restrict__ blob, const f32x4 *__restrict__ rays, int32_t n,
                     float *__restrict__ t_out, int32_t *__restrict__ id_out, uint8_t *__restrict__ occ_out,
                     unsigned long long *__restrict__ stats)
{
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const BaseP B = (BaseP)blob;
#pragma clang diagnostic pop
    const int64_t i = (int64_t)blockIdx.x * QR_BLOCK + (int64_t)threadIdx.x;
    const bool active = i < (int64_t)n;
    Ray r;
    {
        /* caller_ray's text, kept here (through the function this kernel's ray address took another form) */
        const int64_t k = active ? i : 0;           /* n > 0: lanes past the end read ray 0 and do not walk */
        const f32x4 a = rays[2 * k], b = rays[2 * k + 1];
        r.org = {a.x, a.y, a.z}; r.tmin = a.w;
        r.dir = {b.x, b.y, b.z};
        r.tmax = b.w > FLT_MAX ? FLT_MAX : b.w;
        r.list = active ? c_frm(B)->off_query : 0u;
        r.osrf = 0; r.oflg = 0;
        r.ploc = {0.0f, 0.0f, 0.0f};
    }
    Hit h;
    bool occ = false;
    traverse<SHADOW, true, true>(B, active, COHERENT, r, h, occ, stats);
    if (!active) return;
    if constexpr (SHADOW) occ_out[i] = occ ? 1 : 0;
    else
    {
        /* the encoding of render_wave's hit ids (qr_kernel.hpp): surface index << 1 | side, -1 = none */
        const int hsi = (int)((h.srf - QR_OFF_SRF) >> 7);           /* DSurf records are 128 B */
        t_out[i] = h.t;
        id_out[i] = h.srf != 0 ? ((hsi << 1) | h.side) : -1;
    }
}

#endif /* QR_QUERY_HPP */
