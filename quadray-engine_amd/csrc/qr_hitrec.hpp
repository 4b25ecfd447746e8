/*
 * qr_hitrec.hpp - hit records (include/qrhip.h qr_hit_rays_async / qr_hit_views_async): for caller-supplied rays or the pixels
 * of caller-supplied cameras, the closest hit qr_trace_rays_async finds and the surface point the renderer would shade there --
 * hit point, world normal, texture colour, material -- 48 bytes per ray.  Nothing is lit and no secondary ray is traced.
 *
 * One kernel template, two ray sources (launch_ray below, shared with the layer, fan and gather kernels; DESIGN.md 4s lists it
 * and the kernels that keep its text, this one's ray branch among them):
 *   VIEW = false  the caller's qr_ray array (caller_ray, qr_query.hpp): lane i of workgroup g is ray g * 64 + i.  Per-lane walks
 *                 on long lists unless the caller vouches for coherence (QR_TRACE_COHERENT).
 *   VIEW = true   the grid is (footprint columns, footprint rows, views) as for qr_render_views_kernel, but a footprint is always
 *                 8x8 pixels, one lane per PIXEL: only sample 0 of a pixel is recorded (as ids and depth of a view render are), so
 *                 with FSAA the other samples' lanes would idle.  pixel_of_view (qr_kernel.hpp, at fsaa 0) gives the pixel;
 *                 sample_offsets and view_ray below give the ray with the arithmetic of render_wave's VIEW branch for sample 0.
 *                 (render_wave computes its ray inline.  Calling these two functions from it instead left the arithmetic alone
 *                 but renumbered registers in nine existing kernels, so it keeps its text and they restate it here.)  The first
 *                 round of a view render is coherent, so is this walk; DIVK is chosen as qr_render_views_async chooses it.
 * Then `traverse<false, DIVK, true>` on DevHeader::off_query, the surface-point block, and three 16-byte stores per lane
 * (consecutive lanes, consecutive records: a wave of caller rays writes 3 KB in one piece).
 *
 * The surface-point block (surface_point below) restates the first block of shade() (qr_shade.hpp, "if (act)" up to the gamma
 * square of the texture colour) operation for operation; shade() itself is untouched (DESIGN.md "Hit records").  Material and
 * texel reads are divergent per-lane vector loads, as there.
 */
#ifndef QR_HITREC_HPP
#define QR_HITREC_HPP

#include <float.h>

/* FSAA sub-sample offsets of pixel column x, sample k (engine.cpp:3480-3550; render_wave's, qr_kernel.hpp); G: the image
 * through the global address space */
__device__ __forceinline__ void sample_offsets(FrmP fr, const char *G, int fsaa, int x, int k, float &ha, float &va)
{
    int ai = 0;
    if (fsaa == 1) ai = (x & 1) * 2 + k;
    if (fsaa == 2) ai = k;
    if (fsaa == 0) { ha = fr->fr.hor_a[0]; va = fr->fr.ver_a[0]; }       /* wave-uniform: scalar loads */
    else
    {
        const qr_frame *gf = (const qr_frame *)G;
        ha = gf->hor_a[ai]; va = gf->ver_a[ai];
    }
}

/* the primary ray of a view at sample position (hs, vs): tracer.cpp:1287-1322 on the view record, in the operation order of
 * render_wave's VIEW branch; everything but the list.  No originating surface; t_max +inf is taken as FLT_MAX */
__device__ __forceinline__ void view_ray(const QR_CONST qr_view *vw, float hs, float vs, Ray &ray)
{
    float x1 = vw->hor[0] * hs, x2 = vw->hor[1] * hs, x3 = vw->hor[2] * hs;
    float x4 = vw->ver[0] * vs, x5 = vw->ver[1] * vs, x6 = vw->ver[2] * vs;
    x1 = x1 + x4; x2 = x2 + x5; x3 = x3 + x6;
    ray.dir.x = x1 + vw->dir[0];
    ray.dir.y = x2 + vw->dir[1];
    ray.dir.z = x3 + vw->dir[2];
    ray.org.x = vw->org[0]; ray.org.y = vw->org[1]; ray.org.z = vw->org[2];
    ray.tmin = vw->t_min;
    const float vt = vw->t_max;
    ray.tmax = vt > FLT_MAX ? FLT_MAX : vt;
    ray.osrf = 0; ray.oflg = 0;
    ray.ploc = {0, 0, 0};
}

/* This lane's element of a launch and its ray, everything but the list; returns whether the lane is inside the launch.
 *   VIEW = false  lane i of workgroup g is ray g * 64 + i of the caller's array (caller_ray, qr_query.hpp); rec = i.  n > 0: a
 *                 lane past the end reads ray 0, keeps rec = 0, and neither walks nor stores.
 *   VIEW = true   one lane per pixel of an 8x8 footprint (pixel_of_view at fsaa 0: k = 0), sample 0's offsets at the frame's FSAA;
 *                 rec = (view, y, x).  A lane outside the frame keeps pixel (0, 0) of its view and stores nothing.
 * (render_wave keeps its own copy of the view ray's arithmetic: its assembly is what bench.py times.) */
template <bool VIEW>
__device__ __forceinline__ bool launch_ray(FrmP fr, const char *G, const f32x4 *__restrict__ rays, int32_t n, const ViewsP &vp,
                                           Ray &r, size_t &rec)
{
    bool active;
    if constexpr (VIEW)
    {
        const u32 ord = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x | (blockIdx.y << 14)));
        const int view = __builtin_amdgcn_readfirstlane((int)blockIdx.z);
        int x, y, k;
        active = pixel_of_view(ord, 0, vp, x, y, k);
        float ha, va;
        sample_offsets(fr, G, fr->fr.fsaa, x, k, ha, va);
        float hs = (float)x + ha; hs = hs + 0.0f;       /* the zero jitter of a frame that is not path-traced */
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
        const int64_t q = active ? i : 0;
        caller_ray(rays, q, r);
        rec = (size_t)q;
    }
    return active;
}

/* hit point, world normal as shading uses it, texture colour and the byte offset of the hit side's material, for a lane WITH a hit */
__device__ __forceinline__ void surface_point(const char *__restrict__ G, u32 off_shade, const Ray &r, const Hit &h,
                                              V3 &hit, V3 &nrm, V3 &tex, u32 &mo)
{
    const u32 hsrf = h.srf;
    const int side = h.side;
    const DShade *__restrict__ sd = (const DShade *)(G + (off_shade + ((hsrf - QR_OFF_SRF) >> 2)));   /* 32 B per 128 B */
    const DSurf *__restrict__ s = (const DSurf *)(G + hsrf);

    const float t = h.t;
    float x0, x1, x2, x3, x4, x5, x6;
    x4 = r.dir.x * t; hit.x = x4 + r.org.x;
    x5 = r.dir.y * t; hit.y = x5 + r.org.y;
    x6 = r.dir.z * t; hit.z = x6 + r.org.z;

    const int props = side | (side ? s->props1 : s->props0);
    mo = sd->mat[side];
    const u32 fl = s->flags;
    const u32 tside = side ? QR_SMASK : 0u;
    const int has_trm = (int)DF_TRM(fl);
    const int nkind = (int)DF_NKIND(fl);
    float tu = 0.0f, tv = 0.0f;
    V3 ln = {0, 0, 0};                          /* normal in surface space */

    if (nkind == 1)
    {
        /* PL_mat 4139-4193 */
        if (props & QR_PROP_TEXTURE)
        {
            tu = fxor(vget(h.loc, (int)DF_MAP(fl, 0)), DF_SGN(fl, 0));
            tv = fxor(vget(h.loc, (int)DF_MAP(fl, 1)), DF_SGN(fl, 1));
        }
        x6 = fxor(1.0f, tside);
        vset(ln, (int)DF_MAP(fl, 2), fxor(x6, DF_SGN(fl, 2)));
    }
    else
    {
        /* QD_mat 4845-4905 / TP_mat 4280-4336 */
        x4 = h.loc.x * s->sci[0]; x5 = h.loc.y * s->sci[1]; x6 = h.loc.z * s->sci[2];
        if (nkind == 2)
        {
            x4 = x4 - s->scj[0]; x5 = x5 - s->scj[1]; x6 = x6 - s->scj[2];
        }
        x1 = x4 * x4; x2 = x5 * x5; x3 = x6 * x6;
        x1 = x1 + x2; x1 = x1 + x3;
        x0 = rsq(x1);
        x0 = fxor(x0, tside);
        ln.x = x4 * x0; ln.y = x5 * x0; ln.z = x6 * x0;
    }
    nrm = ln;
    if (has_trm != 0)
    {
        /* MT_nrm 2184-2263: transposed trnode matrix */
        const DSurf *__restrict__ tr = (const DSurf *)(G + s->trn);
        const int ttrm = (int)DF_TRM(tr->flags);
        x1 = ln.x; x2 = ln.y; x3 = ln.z;
        x4 = tr->tci[0] * x1;
        x5 = tr->tcj[1] * x2;
        x6 = tr->tck[2] * x3;
        if (ttrm != 1)
        {
            x4 = x4 + tr->tcj[0] * x2;
            x4 = x4 + tr->tck[0] * x3;
            x5 = x5 + tr->tci[1] * x1;
            x5 = x5 + tr->tck[1] * x3;
            x6 = x6 + tr->tci[2] * x1;
            x6 = x6 + tr->tcj[2] * x2;
        }
        if (ttrm != 2)
        {
            x1 = x4 * x4; x2 = x5 * x5; x3 = x6 * x6;
            x1 = x1 + x2; x1 = x1 + x3;
            x0 = rsq(x1);
            x4 = x4 * x0; x5 = x5 * x0; x6 = x6 * x0;
        }
        nrm.x = x4; nrm.y = x5; nrm.z = x6;
    }

    /* MT_tex 2293-2327, PAINT_FRAG / PAINT_COLX 653-673 */
    const qr_material *__restrict__ mt = (const qr_material *)(G + mo);
    u32 toff = 0;
    if (props & QR_PROP_TEXTURE)
    {
        x4 = mt->t_map[0] ? tv : tu;
        x5 = mt->t_map[1] ? tv : tu;
        x4 = x4 - mt->xoffs; x5 = x5 - mt->yoffs;
        x4 = x4 * mt->xscal; x5 = x5 * mt->yscal;
        const int32_t iu = cvt_floor(x4) & (int32_t)mt->xmask;
        const int32_t iv = cvt_floor(x5) & (int32_t)mt->ymask;
        toff = (u32)iu + ((u32)iv << (mt->yshft & 31));
    }
    const u32 texel = *(const u32 *)(G + ((u32)mt->tex + toff * 4u));
    const u32 cmask = mt->cmask;
    const float clampv = mt->clamp;
    tex.x = (float)(int32_t)((texel >> 16) & cmask) / clampv;
    tex.y = (float)(int32_t)((texel >> 8) & cmask) / clampv;
    tex.z = (float)(int32_t)(texel & cmask) / clampv;
    if (props & QR_PROP_GAMMA) { tex.x = tex.x * tex.x; tex.y = tex.y * tex.y; tex.z = tex.z * tex.z; }
}

/* off_mat: byte offset of the image's material table (qr_material records, 128 B each): DShade::mat -> snapshot material index */
template <bool VIEW, bool DIVK, bool COHERENT>
__global__ __launch_bounds__(QR_BLOCK, DIVK ? QR_DIVK_WAVES : QR_MIN_WAVES_PER_SIMD)
void qr_hit_kernel(const char *__restrict__ blob, const f32x4 *__restrict__ rays, int32_t n, ViewsP vp, u32 off_mat,
                   f32x4 *__restrict__ out, unsigned long long *__restrict__ stats)
{
    static_assert(sizeof(qr_material) == 128, "material index = (byte offset - off_mat) >> 7");
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const BaseP B = (BaseP)blob;
#pragma clang diagnostic pop
    const FrmP fr = c_frm(B);
    bool active;
    size_t rec;                                 /* this lane's record in `out` */
    Ray r;
    if constexpr (VIEW) active = launch_ray<true>(fr, blob, rays, n, vp, r, rec);
    else
    {
        /* launch_ray<false>'s text, kept here (through the function this kernel's ray address took another form) */
        const int64_t i = (int64_t)blockIdx.x * QR_BLOCK + (int64_t)threadIdx.x;
        active = i < (int64_t)n;
        const int64_t q = active ? i : 0;           /* n > 0: lanes past the end read ray 0 and do not walk */
        const f32x4 a = rays[2 * q], b = rays[2 * q + 1];
        r.org = {a.x, a.y, a.z}; r.tmin = a.w;
        r.dir = {b.x, b.y, b.z};
        r.tmax = b.w > FLT_MAX ? FLT_MAX : b.w;
        r.osrf = 0; r.oflg = 0;
        r.ploc = {0.0f, 0.0f, 0.0f};
        rec = (size_t)q;
    }
    r.list = active ? fr->off_query : 0u;

    Hit h;
    bool occ = false;
    traverse<false, DIVK, true>(B, active, VIEW || COHERENT, r, h, occ, stats);
    if (!active) return;

    V3 hit = {0.0f, 0.0f, 0.0f}, nrm = {0.0f, 0.0f, 0.0f}, tex = {0.0f, 0.0f, 0.0f};
    int id = -1, mat = -1;
    if (h.srf != 0)
    {
        u32 mo;
        surface_point(blob, fr->off_shade, r, h, hit, nrm, tex, mo);
        id = ((int)((h.srf - QR_OFF_SRF) >> 7) << 1) | h.side;          /* the encoding of qr_trace_kernel */
        mat = (int)((mo - off_mat) >> 7);
    }
    f32x4 *__restrict__ o = out + 3 * rec;
    o[0] = f32x4{hit.x, hit.y, hit.z, h.t};
    o[1] = f32x4{nrm.x, nrm.y, nrm.z, __int_as_float(id)};
    o[2] = f32x4{tex.x, tex.y, tex.z, __int_as_float(mat)};
}

#endif /* QR_HITREC_HPP */
