/*
 * qr_layers.hpp - hit layers (include/qrhip.h qr_layer_rays_async / qr_layer_views_async): the first K hits along caller-supplied
 * rays or the pixels of caller-supplied cameras, in order, in one launch -- picking through glass, thickness and entry / exit
 * pairs, order-independent transparency, layered depth images, "how many surfaces lie between A and B".
 *
 * Layer 0 is the closest hit of the ray (org, tmin, dir, tmax) as qr_trace_kernel finds it; layer j + 1 is the closest hit of
 * (org, t_j, dir, tmax), t_j being layer j's t bit for bit: a hit counts when tmin < t < tmax and a query ray has no
 * self-exclusion, so "the next hit" is the same ray with tmin = t.  What a host would otherwise loop over qr_trace_rays_async,
 * reading the rays again for every layer and rewriting tmin in between; here the ray, the count and the alive flag stay in
 * registers and only the answers leave.
 *
 * One kernel template, two ray sources (launch_ray, qr_hitrec.hpp):
 *   VIEW = false  the caller's qr_ray array: lane i of workgroup g is ray g * 64 + i.
 *   VIEW = true   the grid is (footprint columns, footprint rows, views), a footprint is 8x8 pixels, one lane per pixel, sample
 *                 0's ray under FSAA.
 * Then a wave-uniform loop over the layers.  Per layer: the ballot of the lanes that are still alive; when it is empty the walk
 * loop is left (traverse is never called without an active lane, as the fan kernel never calls it: its LM(traced) != 0).
 * Otherwise traverse<false, DIVK, true> on DevHeader::off_query with the ballot's lanes as `active` (r.list = 0 for the others),
 * then -- a wave-uniform branch on the pointer -- surface_point for the lanes that hit, then the stores of the layer's plane
 * entries, then r.tmin = h.t.  A lane dies on its first miss; traverse gives h.t = r.tmax and h.srf = 0 to every lane that did not
 * walk or did not hit, so dead lanes store the miss values of their plane entry with the same instructions.  After the walk loop
 * the remaining planes are filled with miss values by stores alone: all k planes are always written in full.
 *
 * Planes are [k][elements] (element = ray index, or (view, y, x) of a view launch), indexed with size_t: the lanes of a wave of
 * caller rays store 256 contiguous bytes of t, of id, and 3 KB of records per layer.  No LDS or scratch of its own (the
 * hand-over pool of the per-lane walks is traverse's).
 *
 * `coherent` of the later layers: the rays of layer j + 1 are the rays of layer j with another tmin -- the same origins and
 * directions, so neighbours stay neighbours and what the caller (QR_TRACE_COHERENT) or the camera vouches for holds for every
 * layer.  Results do not depend on it.
 */
#ifndef QR_LAYERS_HPP
#define QR_LAYERS_HPP

#include <float.h>

/* k: layers, 1..QR_LAYER_MAX; count is required, t, id and hits may be null; elems: elements of the launch (the stride of a
 * plane); off_mat: byte offset of the image's material table, as for qr_hit_kernel */
struct LayerP
{
    int32_t k;
    u32 off_mat;
    int32_t *count;
    float *t;
    int32_t *id;
    f32x4 *hits;
    uint64_t elems;
};

template <bool VIEW, bool DIVK, bool COHERENT>
__global__ __launch_bounds__(QR_BLOCK, DIVK ? QR_DIVK_WAVES : QR_MIN_WAVES_PER_SIMD)
void qr_layer_kernel(const char *__restrict__ blob, const f32x4 *__restrict__ rays, int32_t n, ViewsP vp, LayerP lp,
                     unsigned long long *__restrict__ stats)
{
    static_assert(sizeof(qr_material) == 128, "material index = (byte offset - off_mat) >> 7");
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const BaseP B = (BaseP)blob;
#pragma clang diagnostic pop
    const FrmP fr = c_frm(B);
    size_t rec;                                 /* this lane's element */
    Ray r;
    const bool active = launch_ray<VIEW>(fr, blob, rays, n, vp, r, rec);

    /* the layers: every lane of the wave stays in the loop (the walks are wave-wide), a lane that has missed walks no more */
    const u32 qlist = fr->off_query;
    const size_t elems = (size_t)lp.elems;
    bool alive = active;
    int count = 0;
    int j = 0;
    for (; j < lp.k; j++)
    {
        if (LM(alive) == 0) break;
        r.list = alive ? qlist : 0u;
        Hit h;
        bool occ = false;
        traverse<false, DIVK, true>(B, alive, VIEW || COHERENT, r, h, occ, stats);
        /* a lane that did not walk or did not hit holds traverse's defaults: h.t = r.tmax, h.srf = 0 */
        const bool hit = alive && h.srf != 0;
        const size_t e = (size_t)j * elems + rec;
        const int id = hit ? (((int)((h.srf - QR_OFF_SRF) >> 7) << 1) | h.side) : -1;        /* the encoding of qr_trace_kernel */
        if (lp.hits != nullptr)
        {
            V3 pos = {0.0f, 0.0f, 0.0f}, nrm = {0.0f, 0.0f, 0.0f}, tex = {0.0f, 0.0f, 0.0f};
            int mat = -1;
            if (hit)
            {
                u32 mo;
                surface_point(blob, fr->off_shade, r, h, pos, nrm, tex, mo);
                mat = (int)((mo - lp.off_mat) >> 7);
            }
            if (active)
            {
                f32x4 *__restrict__ o = lp.hits + 3 * e;
                o[0] = f32x4{pos.x, pos.y, pos.z, h.t};
                o[1] = f32x4{nrm.x, nrm.y, nrm.z, __int_as_float(id)};
                o[2] = f32x4{tex.x, tex.y, tex.z, __int_as_float(mat)};
            }
        }
        if (active)
        {
            if (lp.t != nullptr) lp.t[e] = h.t;
            if (lp.id != nullptr) lp.id[e] = id;
        }
        count += hit ? 1 : 0;
        if (hit) r.tmin = h.t;                      /* the next layer's ray: the same ray from this hit's t on, no epsilon */
        alive = hit;
    }

    /* no lane of the wave is alive (or the layers are done): the planes that are left get the miss values, without a walk */
    if (!active) return;
    for (; j < lp.k; j++)
    {
        const size_t e = (size_t)j * elems + rec;
        if (lp.t != nullptr) lp.t[e] = r.tmax;
        if (lp.id != nullptr) lp.id[e] = -1;
        if (lp.hits != nullptr)
        {
            f32x4 *__restrict__ o = lp.hits + 3 * e;
            o[0] = f32x4{0.0f, 0.0f, 0.0f, r.tmax};
            o[1] = f32x4{0.0f, 0.0f, 0.0f, __int_as_float(-1)};
            o[2] = f32x4{0.0f, 0.0f, 0.0f, __int_as_float(-1)};
        }
    }
    lp.count[rec] = count;
}

#endif /* QR_LAYERS_HPP */
