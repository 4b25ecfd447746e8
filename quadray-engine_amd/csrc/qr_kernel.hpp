/*
 * qr_kernel.hpp - device code of the gfx950 rendering backend.
 *
 * What it computes: the reference's per-pixel pipeline `render0`
 * (core/tracer/tracer.cpp:1081-5405): primary rays, object-list traversal with
 * trnode transform caching and bounding-volume arrays, plane / quadric /
 * two-plane solvers, depth + axis + custom (CSG) clipping, Phong lighting with
 * hard shadows, refraction + Fresnel, reflection + metal/plain Fresnel,
 * FSAA reduce, gamma, 0x00RRGGBB packing.
 *
 * How it is organised for CDNA4 (this is not the reference's structure):
 *   - one lane = one ray (sample); a 64-lane wavefront = one 8x8 pixel block
 *     (4x4 / 8x4 pixels under 4x / 2x FSAA) and is its own workgroup; waves take
 *     entries of a host-computed schedule (footprints that can recurse first and
 *     with issue priority, the tile-list head in the entry, empty tiles leave at once).
 *   - COMPILED LISTS: the upload pass (qr_compile.cpp, qr_program.h) turns every list of the
 *     snapshot into a contiguous program of 32-byte cells whose opcode says what the walk does
 *     there (solver, which diff / ray it reads, cull, shadow class); the whole scene is one
 *     blob addressed by byte offsets from one base register.
 *   - WAVE-PACKET TRAVERSAL: lanes of a wave that walk the same list walk it
 *     together; the cell offset is wave-uniform, so cells and surface records are
 *     fetched with SCALAR loads (constant address space) into SGPRs and only per-ray
 *     quantities live in VGPRs.  Lanes with different lists (secondary rays leaving
 *     different surfaces) are served group by group (__ballot / readfirstlane) - the
 *     wave-level analogue of the reference's CHECK_MASK NONE/FULL packet early-outs
 *     (rtbase.h:1209).
 *   - per cell, a conservative bounding-sphere test (ours) lets the wave skip
 *     elements no ray can meet; bounding-volume arrays are skipped per ray and,
 *     when no ray of the group enters one, jumped over by the whole wave.
 *   - DEFERRED SHADING: the reference shades every hit that passes the depth
 *     test while it walks a list (overdraw); shading has no effect on the walk
 *     and fully overwrites the lane's colour, so walking first (keeping the
 *     depth-test sequence) and shading only the final hit is bit-identical and
 *     costs one shading (and one set of shadow rays) per ray
 *     (checked on the CPU by tests/test_oracle.py::test_deferred_shading_*).
 *   - recursion (context stack, tracer.h:426-665) becomes a per-lane explicit
 *     stack of 16-dword frames evaluated in the reference's order
 *     (refraction child, then reflection child), so colour arithmetic keeps the
 *     reference's association.
 *
 * Numeric contract: IEEE fp32, no contraction (-ffp-contract=off), correctly
 * rounded / and sqrt (hipcc default), compare predicates and integer
 * conversions as in oracle/qr_oracle.c's header.
 */
#ifndef QR_KERNEL_HPP
#define QR_KERNEL_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>
#include "qr_scene.h"
#include "qr_program.h"

#ifndef QR_BLOCK
#define QR_BLOCK 64                /* one wave per workgroup: a wave slot is refilled the moment its wave ends (+8 % Mrays/s over 256) */
#endif
#ifndef QR_MAX_DEPTH
#define QR_MAX_DEPTH 10           /* RT_STACK_DEPTH, tracer.h:46 */
#endif
/* timing experiments (QR_DBG environment variable) exist only in -DQR_KNOBS builds */
#ifdef QR_KNOBS
#define QR_KNOB(bit) ((cx.dbg & (bit)) != 0)
#else
#define QR_KNOB(bit) false
#endif
#define QR_PER_LANE_TILE 0xFFFFFFFEu /* schedule entry: the footprint straddles tiles, look the list up per pixel (QR_SCHED_PER_LANE) */
#ifndef QR_RETURN_LOOP
#define QR_RETURN_LOOP 1     /* the instance with the per-lane walks: a lane unwinds all finished levels in one round (0: one level per round,
                              * as the packet instance does: there it costs demo1 1 % of its isolated launch, A/B in profiles/r04_return_loop_ab.txt) */
#endif
#ifndef QR_DYN_PRIO
#define QR_DYN_PRIO 1        /* issue priority follows the recursion round a wave is in (0: fixed by the footprint's class) */
#endif
#define QR_WT_SLOTS 14       /* QR_WAVETIME builds: u64 slots per wave */
#ifndef QR_MIN_WAVES_PER_SIMD
#define QR_MIN_WAVES_PER_SIMD 4   /* __launch_bounds__ 2nd argument: waves per SIMD */
#endif
#ifndef QR_DIVK_WAVES
#define QR_DIVK_WAVES 3           /* the instance with the per-lane walks: 168 VGPRs, none spilled.  (With walk_pool alone 4 waves and 70
                                   * spilled registers were 8 % faster; with the grid walk's state it is 93 spilled and 1 % slower.) */
#endif

typedef uint32_t u32;
#define QR_SMASK 0x80000000u

/* -DQR_PROF builds: wave-level event counters in a device global, printed by qr_render_count (where does a frame's instruction
 * budget go: tools/gpu_prof.py) */
#ifdef QR_PROF
__device__ unsigned long long qr_prof[80];
#define QR_PROF_HIT(i) do { if (__ffsll((long long)__ballot(true)) - 1 == (int)(threadIdx.x & 63u)) atomicAdd(&qr_prof[i], 1ull); } while (0)
#define QR_PROF_ADD(i, n) do { if (__ffsll((long long)__ballot(true)) - 1 == (int)(threadIdx.x & 63u)) atomicAdd(&qr_prof[i], (unsigned long long)(n)); } while (0)
/* algorithmic fp32 operations the kernel executes, with the weights of SURVEY.md 8(d) as oracle/qr_oracle.c applies them (FL()):
 * n operations for every lane that is active here / for every lane of `mask` */
#define QR_FLOPS(n) QR_PROF_ADD(48, (unsigned long long)(n) * (unsigned long long)__popcll(__ballot(true)))
#define QR_FLOPS_M(n, cnt) QR_PROF_ADD(48, (unsigned long long)(n) * (unsigned long long)(cnt))
/* beside them, the arithmetic of this implementation's own culls (no step of SURVEY 8(d): never part of a roofline numerator):
 * walk set-up 9 (+ 6 with box cells), sphere test 20, box slab test 22 */
#define QR_CULL_FLOPS(n) QR_PROF_ADD(49, (unsigned long long)(n) * (unsigned long long)__popcll(__ballot(true)))
#else
#define QR_PROF_HIT(i) do { } while (0)
#define QR_PROF_ADD(i, n) do { } while (0)
#define QR_FLOPS(n) do { } while (0)
#define QR_FLOPS_M(n, cnt) do { } while (0)
#define QR_CULL_FLOPS(n) do { } while (0)
#endif

/* The diagnostic builds enter the walks, shade() and render_wave through these hooks alone: QR_ST(...) holds statements
 * and declarations of the -DQR_STATS build, QR_PF(...) of -DQR_PROF, QR_WT(...) of -DQR_WAVETIME (tools/gpu_wavetime.py), QR_GD(...)
 * of the guarded statistics build (-DQR_STATS -DQR_GUARD); each expands to nothing in every other build, the product's among them.
 * WalkStats is the counter block as the walks take it, always: the pointer itself in the statistics build, and an empty object made
 * from that pointer -- no register, no argument -- elsewhere (Ctx::stats and LaunchP::stats stay pointers). */
#ifdef QR_STATS
typedef unsigned long long *WalkStats;
#define QR_ST(...) __VA_ARGS__
#else
struct WalkStats { __device__ __forceinline__ WalkStats(unsigned long long *) {} };
#define QR_ST(...)
#endif
#ifdef QR_PROF
#define QR_PF(...) __VA_ARGS__
#else
#define QR_PF(...)
#endif
#ifdef QR_WAVETIME
#define QR_WT(...) __VA_ARGS__
#else
#define QR_WT(...)
#endif
#if defined(QR_STATS) && defined(QR_GUARD)
#define QR_GD(...) __VA_ARGS__
#else
#define QR_GD(...)
#endif

/* what a launch needs besides the scene image: kernel arguments */
struct LaunchP
{
    const char *B;                      /* the compiled scene (qr_program.h), device memory                    */
    const uint32_t *order;              /* wave schedule, 8 B per wave: {bx | by << 14 | heaviness << 30, list offset} */
    int32_t n_blocks;
    int32_t depth;
    int32_t row_begin, row_end;         /* rows rendered by this launch                                        */
    int32_t index, thnum;               /* reference row interleave                                            */
    int32_t group_first, group_stride;  /* 8-row groups: first + k*stride                                      */
    unsigned long long *stats;          /* QR_STATS / QR_WAVETIME builds only                                  */
    int32_t dbg;                        /* timing experiments only (QR_DBG)                                    */
};

/* ------------------------------------------------------------------------ */
/* lane primitives (same definitions as the oracle)                          */
/* ------------------------------------------------------------------------ */

__device__ __forceinline__ u32   f2u(float f) { return __float_as_uint(f); }
__device__ __forceinline__ float u2f(u32 u)   { return __uint_as_float(u); }

__device__ __forceinline__ bool ceq(float a, float b) { return a == b; }
__device__ __forceinline__ bool cne(float a, float b) { return !(a == b); }
__device__ __forceinline__ bool clt(float a, float b) { return a < b; }
__device__ __forceinline__ bool cle(float a, float b) { return a <= b; }
__device__ __forceinline__ bool cgt(float a, float b) { return !(a <= b); }
__device__ __forceinline__ bool cge(float a, float b) { return !(a < b); }

__device__ __forceinline__ float fxor(float a, u32 m) { return u2f(f2u(a) ^ m); }
__device__ __forceinline__ float fabs_bits(float a)   { return u2f(f2u(a) & 0x7FFFFFFFu); }
__device__ __forceinline__ float rsq(float x) { return 1.0f / __builtin_sqrtf(x); }

__device__ __forceinline__ int32_t cvt_floor(float x)
{
    float f = __builtin_floorf(x);
    return (f >= -2147483648.0f && f < 2147483648.0f) ? (int32_t)f : (int32_t)0x80000000u;
}
__device__ __forceinline__ int32_t cvt_near(float x)
{
    float f = __builtin_rintf(x);
    return (f >= -2147483648.0f && f < 2147483648.0f) ? (int32_t)f : (int32_t)0x80000000u;
}

struct V3 { float x, y, z; };

__device__ __forceinline__ float vget(const V3 &v, int i) { return i == 0 ? v.x : i == 1 ? v.y : v.z; }
__device__ __forceinline__ void  vset(V3 &v, int i, float f)
{
    v.x = i == 0 ? f : v.x; v.y = i == 1 ? f : v.y; v.z = i == 2 ? f : v.z;
}

#define FLAG_SIDE 1
#define FLAG_PASS_THRU 2

/*
 * Wave-uniform records are read through the CONSTANT address space: with a
 * uniform (readfirstlane-derived) offset the backend then selects s_load_dword*
 * into SGPRs instead of 64 identical vector loads.  The image is never written
 * while a launch is in flight.
 */
#define QR_CONST __attribute__((address_space(4)))
typedef const QR_CONST char *BaseP;
typedef const QR_CONST DevHeader *FrmP;
typedef u32 u32x2 __attribute__((ext_vector_type(2)));
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef u32 u32x8 __attribute__((ext_vector_type(8)));

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
__device__ __forceinline__ FrmP c_frm(BaseP B) { return (FrmP)B; }
#pragma clang diagnostic pop

/* per-wave context: the blob through both address spaces (uniform -> scalar loads, per-lane -> vector loads) */
struct Ctx
{
    BaseP B;
    const char *G;
    u32 off_shade;
    unsigned long long *stats;
    int dbg;
};

/* ------------------------------------------------------------------------ */
/* per-lane traversal state                                                  */
/* ------------------------------------------------------------------------ */

struct Ray
{
    V3 org, dir;            /* ctx_ORG, ctx_RAY_X..Z                          */
    float tmin, tmax;       /* ctx_T_MIN, initial ctx_T_BUF                   */
    u32 list;               /* byte offset of the list program, 0 = none      */
    u32 osrf;               /* ctx_PARAM(OBJ): byte offset of the originating surface's DSurf, 0 = none */
    int oflg;               /* ctx_PARAM(FLG) & 3: side | pass-thru           */
    V3 ploc;                /* parent's local hit (parent ctx_NRM_I..K)       */
};

struct Hit
{
    float t;                /* final ctx_T_BUF                                */
    u32 srf;                /* byte offset of the hit surface's DSurf, 0 = none */
    int side;
    V3 loc;                 /* local (possibly conic-adjusted) hit, ctx_NEW   */
};

#include "qr_walk.hpp"
#include "qr_shade.hpp"
#include "qr_pt_eager.hpp"

/* ------------------------------------------------------------------------ */
/* the kernel                                                                */
/* ------------------------------------------------------------------------ */

__device__ __forceinline__ float clamp1(float x) { return x < 1.0f ? x : 1.0f; }

/*
 * Path-tracer mode (RT_FEAT_PT; the third kernel instance only).  What the engine keeps per frame buffer
 * (engine.cpp:2875-2893): one LCG state and three colour planes per pixel sample; pts_o = 1 / frames so far,
 * pts_u = 1 - pts_o (tracer.cpp:1112-1136).
 */
struct PtParams { u32 *seeds; float *acc_r, *acc_g, *acc_b; float pts_o, pts_u; int eager, pad; };

/*
 * Ray shading (qr_shade_rays_async; RAYS != 0 instances only): the wave's 64 primary rays come from the caller's qr_ray
 * array instead of the camera, and its colours leave linear, before the frame's output step.  RAYS = 1: caller rays; 2: caller
 * rays that the caller vouches are neighbours (QR_TRACE_COHERENT), so that the first round may take packet walks.
 */
struct RaysP { const f32x4 *rays; int32_t n; int32_t pad; float *rgb; };

/*
 * View rendering (qr_render_views_async; the RAYS = 3 instance): a wave is one footprint of one caller-supplied camera (qr_view,
 * the camera part of the frame record) at the launch's frame size.  Its rays are the frame's primary rays computed from the view
 * record instead of the snapshot's, they walk the camera-independent ray-query list as caller rays do (CALLER: a view's t_min
 * and origin are the caller's), and their colours leave through the frame's output step into frames[view][y][x].
 */
struct ViewsP { const qr_view *views; int32_t width, height; float *depth; };

/*
 * Path-traced views (qr_pt_views_async; the RAYS = 5 instance, PT = true): the accumulation of PtParams for every view of a view
 * launch, in memory the caller owns.  state: per view four planes of width * height * samples-per-pixel 32-bit words -- the LCG
 * states, then the running means of r, g, b -- slot (y * width + x) * samples-per-pixel + k (include/qrhip.h).  done: samples the
 * state holds; samples: how many this launch adds; mean: optional float [view][y][x][3], the pixel's linear colour after the FSAA
 * reduce.
 */
struct PtViewsP { u32 *state; int32_t done, samples; float *mean; };

/*
 * Path-traced rays (qr_pt_rays_async; the RAYS = 6 instance, PT = true): caller rays as in RaysP, and per ray an optional spread
 * (qr_ray_spread, two 16-byte words: du xyz, pad, dv xyz, pad; nullptr: none) along which every sample's direction is jittered.
 * rgb: optional float [n][3], the running means after the launch.  The accumulation itself (state, done, samples) is the
 * kernel's own argument: qr_pt_rays_kernel.
 */
struct PtRaysP { const f32x4 *rays; const f32x4 *spread; int32_t n; int32_t pad; float *rgb; };

/* one wave = one schedule entry: footprint `ord`, its tile-list program, rendered into `frame` */
/*
 * The pixel sample a lane stands for and whether this launch owns it, from the schedule word.  Computed where it is needed --
 * at the start of a wave, in the empty-tile exit, at the final store -- each time through opaque copies of its inputs: as
 * common subexpressions the coordinates were four registers live across the whole recursion, and the 128-register kernel
 * instance spilled them (2 KB of scratch traffic per wave: two thirds of the HBM bytes of the deep-recursion frames).
 */
__device__ __forceinline__ bool pixel_of(u32 ord, int fsaa, const LaunchP &lp, FrmP fr, int &x, int &y, int &k)
{
    asm volatile("" : "+s"(ord));
    int lane = (int)(threadIdx.x & 63u);
    asm volatile("" : "+v"(lane));
    const int fw = fsaa == 2 ? 4 : 8, fh = fsaa == 0 ? 8 : 4;
    const int pix = lane >> fsaa;               /* pixel index inside the wave */
    k = lane & ((1 << fsaa) - 1);               /* sample index inside the pixel */
    const int px = fsaa == 2 ? (pix & 3) : (pix & 7), py = fsaa == 2 ? (pix >> 2) : (pix >> 3);
    x = (int)(ord & 0x3FFFu) * fw + px;
    y = (int)((ord >> 14) & 0x3FFFu) * fh + py;
    const int group = y >> 3;
    bool inside = x < fr->fr.frm_w && y < fr->fr.frm_h && y >= lp.row_begin && y < lp.row_end;
    if (group < lp.group_first) inside = false;
    if (lp.group_stride != 1 && (group - lp.group_first) % lp.group_stride != 0) inside = false;
    if (inside && lp.thnum > 1) inside = (y % lp.thnum) == lp.index;
    return inside;
}

/* ... and of a view launch (RAYS = 3): the footprint word holds the workgroup's x | y << 14, the frame is the launch's */
__device__ __forceinline__ bool pixel_of_view(u32 ord, int fsaa, const ViewsP &vp, int &x, int &y, int &k)
{
    asm volatile("" : "+s"(ord));
    int lane = (int)(threadIdx.x & 63u);
    asm volatile("" : "+v"(lane));
    const int fw = fsaa == 2 ? 4 : 8, fh = fsaa == 0 ? 8 : 4;
    const int pix = lane >> fsaa;
    k = lane & ((1 << fsaa) - 1);
    const int px = fsaa == 2 ? (pix & 3) : (pix & 7), py = fsaa == 2 ? (pix >> 2) : (pix >> 3);
    x = (int)(ord & 0x3FFFu) * fw + px;
    y = (int)((ord >> 14) & 0x3FFFu) * fh + py;
    return x < vp.width && y < vp.height;
}

/*
 * RAYS (ray shading, see RaysP) changes where the wave's rays come from (the caller's array: gw is the workgroup, lane i of it
 * ray gw * 64 + i), which lanes are inside (i < n), drops the empty-tile exit and the issue-priority schedule, and stores the
 * linear colour and the first hit's id per ray instead of the frame's output step.  The recursion between them is one piece.
 * RAYS = 3 (view rendering, see ViewsP): the frame's own ray arithmetic and output step on the view gw of the launch, footprint
 * `ord`, the walk and the missing tile schedule of the caller-ray instances; the first hit's t leaves right after the first walk.
 * RAYS = 4 (view accumulation, qr_views_mean_kernel): RAYS = 3 up to and including the FSAA reduce; the reduced linear colour is
 * handed back in `mean_out` (sample 0's lane holds the pixel's) and nothing is stored.  The caller runs it once per view: everything
 * a wave sets up -- rays, recursion stack, mode, counters -- is set up here, on every call, and nothing is read from an earlier one.
 * RAYS = 5 (path-traced views, qr_pt_views_kernel; PT = true): ONE path-tracer sample of the view's footprint.  The view's ray
 * set-up and first walk (RAYS = 3) around the path tracer's jitter, shading and bounces; the sample's generator state comes in and
 * goes out through `rng_io`, its colour leaves in `mean_out` before the running mean, and nothing is read from or written to
 * global memory for it: the caller keeps the state between samples.  Always the deferred order (no eager machine).
 * RAYS = 6 (path-traced rays, qr_pt_rays_kernel; PT = true): ONE path-tracer sample of the wave's 64 caller rays (PtRaysP; gw is
 * the workgroup, lane i of it ray gw * 64 + i).  The ray -- and its spread, when there is one -- is read again on every call and not
 * kept across the recursion; with a spread the sample first draws two numbers and moves the direction along du and dv by the
 * tent filter's values.  Rays are never taken as neighbours (the first round is RAYS = 1's), there is no empty-tile exit, no
 * priority schedule, no id and no depth; state and colour travel as for RAYS = 5 (`rng_io`, `mean_out`), and a lane past n draws
 * nothing.
 * RAYS = 7 (adaptive path-traced rays, qr_pt_adapt_kernel; PT = true): RAYS = 6 with one difference: a lane is inside only when
 * its ray also takes this sample (`take`, the stop rule of include/qrhip.h evaluated by the caller's loop).  A lane that does not
 * is a lane past n: it draws nothing, walks nothing and stays out of every ballot.
 * RAYS = 8 (indexed adaptive path-traced rays, qr_pt_list_kernel; PT = true): RAYS = 7 with the lane's ray index supplied by the
 * caller (`ray_i`, an entry of its list) instead of gw * 64 + lane.  `take` is all that makes a lane inside: the caller has folded
 * "this list position is served and its entry is below n" into it.  The index is used for the ray's and the spread's rows and
 * nothing else, before the first walk: it is not live through the recursion.
 * RAYS = 9 (adaptive path-traced views, qr_pt_adapt_views_kernel; PT = true): RAYS = 5 with one difference: a lane is inside only
 * when its slot also takes this sample (`take`, as for RAYS = 7).  A lane that does not is a lane past the frame's edge: it draws
 * nothing, walks nothing and stays out of every ballot.  The first round stays RAYS = 5's (`coherent`): the slots that take are a
 * subset of one footprint's primary rays, and the flag only chooses among walks that solve the same surfaces in the same order
 * with the same arithmetic (traverse) -- nothing in that round reads a neighbour lane's ray or needs one alive, which the partial
 * footprints at a frame's right and bottom edges already rest on.
 * RAYS = 10 (gather fans, qr_gather_kernel in qr_gather.hpp): RAYS = 1's machine on ONE ray per lane that the caller supplies in
 * registers (`ray_in`: origin, direction, tmin, tmax already taken as FLT_MAX for +inf; the list is set here).  A lane is inside
 * only when it has such a ray (`take`); a lane that has none is a lane past n, as for RAYS = 7.  The first round is `coherent`
 * where the caller says so (`coh_in`: the fan kernel's rule).  The linear colour comes back in `mean_out`; no id, no depth, no
 * store, and nothing is read from global memory for the ray.
 */
template <bool COUNT, bool DIVK, bool PT = false, int RAYS = 0>
__device__ __forceinline__ void render_wave(const LaunchP &lp, const u32 ord, const u32 sched_head, const int gw,
                                            uint32_t *__restrict__ frame, int32_t *__restrict__ ids,
                                            unsigned long long *__restrict__ counters, const PtParams *ptp = nullptr,
                                            const RaysP *rp = nullptr, const ViewsP *vp = nullptr, V3 *mean_out = nullptr,
                                            u32 *rng_io = nullptr, const PtRaysP *pr = nullptr, const bool take = true,
                                            const u32 ray_i = 0u, const Ray *ray_in = nullptr, const bool coh_in = false)
{
    constexpr bool CALLER_RAYS = RAYS == 1 || RAYS == 2, VIEW = RAYS == 3 || RAYS == 4 || RAYS == 5 || RAYS == 9, MEAN = RAYS == 4;
    constexpr bool PTV = RAYS == 5 || RAYS == 9, PTVA = RAYS == 9, PTR = RAYS == 6 || RAYS == 7 || RAYS == 8, PTA = RAYS == 7, PTL = RAYS == 8;
    constexpr bool GATHER = RAYS == 10;
    static_assert(!PTV || PT, "the path-traced view instance is a path-tracer instance");
    static_assert(!PTR || PT, "the path-traced ray instance is a path-tracer instance");
    static_assert(!GATHER || !PT, "the gather instance is a ray-tracer instance");
    (void)mean_out; (void)rng_io; (void)pr; (void)take; (void)ray_i; (void)ray_in; (void)coh_in;
    QR_WT(const unsigned long long wt_start = __builtin_amdgcn_s_memrealtime();)
    QR_WT(const unsigned long long wt_clk0 = __builtin_amdgcn_s_memtime();)      /* shader cycles: with the 100 MHz stamps, the clock the wave ran at */
    QR_WT(qr_wt_groups[0] = 0; qr_wt_groups[1] = 0; qr_wt_shadow = 0; qr_wt_cells[0] = qr_wt_cells[1] = qr_wt_cells[2] = qr_wt_cells[3] = 0;)
    QR_WT(unsigned long long wt_mid = 0, wt_trav = 0, wt_shade = 0, wt_t0 = 0; u32 wt_push = 0;)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    Ctx cx;
    cx.B = (BaseP)lp.B; cx.G = lp.B; cx.stats = lp.stats; cx.dbg = lp.dbg;
#pragma clang diagnostic pop
    const BaseP B = cx.B;
    const FrmP fr = c_frm(B);
    cx.off_shade = fr->off_shade;
    const int fsaa = fr->fr.fsaa;
    const int ns = 1 << fsaa;
    const int lane = threadIdx.x & 63;
    const int pix = lane >> fsaa;               /* pixel index inside the wave */
    const int k = lane & (ns - 1);              /* sample index inside the pixel */

    /* wave footprint: 8x8 pixels (no AA), 8x4 (2x), 4x4 (4x).  Every WAVE takes one entry of
     * the host-computed schedule (footprints that can spawn deep recursion first, so that their
     * long waves overlap the bulk instead of forming a tail); consecutive entries are
     * neighbouring footprints, so waves running side by side still share tile lists in the scalar cache. */
    const int fw = fsaa == 2 ? 4 : 8, fh = fsaa == 0 ? 8 : 4;
    (void)gw;
    /* footprints that can recurse get issue priority: the frame ends with the slowest of them, and while
     * the bulk is in flight they would otherwise share their SIMD's issue slots evenly */
#if QR_DYN_PRIO
    /* ... and among them the ones that actually do: every traversal round a wave starts raises its priority (2 waves of demo
     * scene 1 at 1080p run 7 rounds, 20 run 6, 12 000 one -- but 3 900 footprints CAN recurse and fill the first generation) */
    if constexpr (!RAYS) if (ord >> 30) __builtin_amdgcn_s_setprio(1);
    int prio_round = 0;
#else
    if constexpr (!RAYS) if (ord >> 30) { if ((ord >> 30) >= 2) __builtin_amdgcn_s_setprio(3); else __builtin_amdgcn_s_setprio(2); }
#endif
    const int px = fsaa == 2 ? (pix & 3) : (pix & 7), py = fsaa == 2 ? (pix >> 2) : (pix >> 3);
    const int x = (int)(ord & 0x3FFFu) * fw + px;
    const int y = (int)((ord >> 14) & 0x3FFFu) * fh + py;
    const int group = y >> 3;
    const int frm_w = VIEW ? vp->width : fr->fr.frm_w;

    bool inside;
    if constexpr (PTVA) inside = x < frm_w && y < vp->height && take;
    else if constexpr (VIEW) inside = x < frm_w && y < vp->height;      /* the grid is the frame's footprints: every wave holds a pixel */
    else if constexpr (CALLER_RAYS) inside = (u32)gw * 64u + (u32)lane < (u32)rp->n;      /* n > 0: every wave holds a ray */
    else if constexpr (PTA) inside = (u32)gw * 64u + (u32)lane < (u32)pr->n && take;
    else if constexpr (PTL) inside = take;
    else if constexpr (PTR) inside = (u32)gw * 64u + (u32)lane < (u32)pr->n;
    else if constexpr (GATHER) inside = take;
    else
    {
        inside = x < frm_w && y < fr->fr.frm_h && y >= lp.row_begin && y < lp.row_end;
        if (group < lp.group_first) inside = false;
        if (lp.group_stride != 1 && (group - lp.group_first) % lp.group_stride != 0) inside = false;
        if (inside && lp.thnum > 1) inside = (y % lp.thnum) == lp.index;
        if (!any_lane(inside)) return;             /* whole wave outside this launch's rows */
    }
    if (!RAYS && sched_head < 256u)
    {
        /* empty tiles: no ray of these footprints meets anything; the reference's pipeline ends with colour 0 for such a
         * packet (clamp, sqrt and cvt of 0 are 0), so store it and leave.  The head is the number of footprints of the
         * run along the row (qr_compile.cpp; 0: one) */
        const u32 run = sched_head == 0 ? 1u : sched_head;
        unsigned long long n = 0;
        for (u32 i = 0; i < run; i++)
        {
            int x0, y0, k0;
            const bool in0 = pixel_of(ord + i, fsaa, lp, fr, x0, y0, k0);
            if (in0 && k0 == 0)
            {
                frame[(size_t)y0 * frm_w + x0] = 0u;
                if (ids != nullptr) ids[(size_t)y0 * frm_w + x0] = -1;
            }
            if (COUNT && in0) n++;
        }
        if (COUNT)
        {
            for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off);
            if (lane == 0 && n != 0) atomicAdd(&counters[0], n);
        }
        return;
    }

    Counters cnt = {0, 0, 0, 0};
    const float t_inf = fr->fr.t_max;

    u32 rng = 0;                                /* PT: this sample's LCG state */
    Ray ray;
    if constexpr (GATHER)
    {
        /* the caller's ray, from its registers: a caller ray's fields (no originating surface), the ray-query list */
        ray.org = ray_in->org; ray.tmin = ray_in->tmin;
        ray.dir = ray_in->dir; ray.tmax = ray_in->tmax;
        ray.list = inside ? fr->off_query : 0u;
        ray.osrf = 0; ray.oflg = 0;
        ray.ploc = {0, 0, 0};
    }
    else if constexpr (PTR)
    {
        /* the caller's ray as below, then the sample's jitter along the ray's spread: two draws, horizontal first, through the
         * tent filter of the frame's samples (tracer.cpp:1218-1285) without the FSAA halving -- caller rays have none; every
         * step one fp32 operation (-ffp-contract=off).  Lanes past the end read ray 0 and spread 0, draw nothing and do not walk */
        const u32 i = inside ? (PTL ? ray_i : (u32)gw * 64u + (u32)lane) : 0u;
        const f32x4 a = pr->rays[2 * (size_t)i], b = pr->rays[2 * (size_t)i + 1];
        ray.org = {a.x, a.y, a.z}; ray.tmin = a.w;
        ray.dir = {b.x, b.y, b.z};
        ray.tmax = b.w > FLT_MAX ? FLT_MAX : b.w;
        ray.list = inside ? fr->off_query : 0u;
        ray.osrf = 0; ray.oflg = 0;
        ray.ploc = {0, 0, 0};
        if (inside) rng = *rng_io;              /* the caller's: column i of the state's plane 0 */
        if (pr->spread != nullptr)
        {
            const f32x4 du = pr->spread[2 * (size_t)i], dv = pr->spread[2 * (size_t)i + 1];
            if (inside)
            {
                float u = pt_random(rng); u = u + u;
                float hr = u < 1.0f ? __builtin_sqrtf(u) - 1.0f : 1.0f - __builtin_sqrtf(2.0f - u);
                float v = pt_random(rng); v = v + v;
                float vr = v < 1.0f ? __builtin_sqrtf(v) - 1.0f : 1.0f - __builtin_sqrtf(2.0f - v);
                hr = hr * 0.5f; vr = vr * 0.5f;
                float x1 = du.x * hr, x2 = du.y * hr, x3 = du.z * hr;
                float x4 = dv.x * vr, x5 = dv.y * vr, x6 = dv.z * vr;
                x1 = x1 + x4; x2 = x2 + x5; x3 = x3 + x6;
                ray.dir.x = ray.dir.x + x1;
                ray.dir.y = ray.dir.y + x2;
                ray.dir.z = ray.dir.z + x3;
            }
        }
    }
    else if constexpr (CALLER_RAYS)
    {
        /* the caller's ray, as qr_trace_kernel reads it (qr_query.hpp): two 16-byte loads; lanes past the end read ray 0 and
         * do not walk.  No originating surface; tmax +inf is taken as FLT_MAX */
        const u32 i = inside ? (u32)gw * 64u + (u32)lane : 0u;
        const f32x4 a = rp->rays[2 * (size_t)i], b = rp->rays[2 * (size_t)i + 1];
        ray.org = {a.x, a.y, a.z}; ray.tmin = a.w;
        ray.dir = {b.x, b.y, b.z};
        ray.tmax = b.w > FLT_MAX ? FLT_MAX : b.w;
        ray.list = inside ? fr->off_query : 0u;
        ray.osrf = 0; ray.oflg = 0;
        ray.ploc = {0, 0, 0};
    }
    else
    /* primary ray, tracer.cpp:1287-1322; sample offsets engine.cpp:3480-3550 */
    {
        int ai = 0;
        if (fsaa == 1) ai = (x & 1) * 2 + k;
        if (fsaa == 2) ai = k;
        float ha, va;
        if (fsaa == 0) { ha = fr->fr.hor_a[0]; va = fr->fr.ver_a[0]; }       /* wave-uniform: scalar loads */
        else
        {
            const qr_frame *gf = (const qr_frame *)cx.G;
            ha = gf->hor_a[ai]; va = gf->ver_a[ai];
        }
        float hr = 0.0f, vr = 0.0f;
        if constexpr (PT)
        {
            /* tent-filter jitter of the sample position, tracer.cpp:1218-1285 */
            bool jitter;
            if constexpr (PTV) jitter = inside; else jitter = inside && ptp->eager != 3;
            if (jitter)
            {
                if constexpr (PTV) rng = *rng_io;       /* the caller's: slot (y * width + x) * ns + k of the view's state */
                else
                rng = ptp->seeds[((size_t)y * fr->fr.frm_row + x) * ns + k];     /* the engine's slot: row stride frm_row (tracer.cpp:1168-1176) */
                float a = pt_random(rng); a = a + a;
                hr = a < 1.0f ? __builtin_sqrtf(a) - 1.0f : 1.0f - __builtin_sqrtf(2.0f - a);
                float b = pt_random(rng); b = b + b;
                vr = b < 1.0f ? __builtin_sqrtf(b) - 1.0f : 1.0f - __builtin_sqrtf(2.0f - b);
                hr = hr * 0.5f; vr = vr * 0.5f;
                if (fsaa != 0) { hr = hr * 0.5f; vr = vr * 0.5f; }
            }
        }
        float hs = (float)x + ha; hs = hs + hr;
        float vs = (float)y + va; vs = vs + vr;
        if constexpr (VIEW)
        {
            /* the same operations on the view record: wave-uniform, scalar loads (64 bytes), nothing of it kept in VGPRs.
             * The first hit walks the ray-query list; t_max +inf is taken as FLT_MAX, as for caller rays */
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
            const QR_CONST qr_view *vw = (const QR_CONST qr_view *)vp->views + gw;
#pragma clang diagnostic pop
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
            ray.list = inside ? fr->off_query : 0u;
        }
        else
        {
        float x1 = fr->fr.hor[0] * hs, x2 = fr->fr.hor[1] * hs, x3 = fr->fr.hor[2] * hs;
        float x4 = fr->fr.ver[0] * vs, x5 = fr->fr.ver[1] * vs, x6 = fr->fr.ver[2] * vs;
        x1 = x1 + x4; x2 = x2 + x5; x3 = x3 + x6;
        ray.dir.x = x1 + fr->fr.dir[0];
        ray.dir.y = x2 + fr->fr.dir[1];
        ray.dir.z = x3 + fr->fr.dir[2];
        ray.org.x = fr->fr.org[0]; ray.org.y = fr->fr.org[1]; ray.org.z = fr->fr.org[2];
        ray.tmin = fr->fr.t_min; ray.tmax = t_inf;
        ray.osrf = 0; ray.oflg = 0;
        ray.ploc = {0, 0, 0};
        ray.list = 0;
        if (sched_head != QR_PER_LANE_TILE)
        {
            if (inside) ray.list = sched_head;
        }
        else if (inside)
        {
            const int tile = (y / fr->fr.tile_h) * fr->fr.tls_row + (x / fr->fr.tile_w);
            ray.list = *(const u32 *)(cx.G + (fr->off_tiles + (u32)tile * 4u));
        }
        }
    }

    /* recursion frames: levels 0..LDSL-1 in LDS ([level][quarter][lane]: a quarter of all lanes is contiguous,
     * 16-byte accesses at a 16-byte lane stride), deeper levels in scratch */
    /* Ray tracer: a frame's first two quarters (colour so far, factors: all a node with ONE child ever reads back) live in LDS
     * for the four shallowest levels and in scratch below; the other two (the second child's origin, direction and local hit:
     * only written by a node with BOTH children) in scratch.  8 KB of LDS per wave as before, but of the frames demo scene 2
     * pushes at 3840x2160 with 4x FSAA -- 18 M with one child, 9 M with two, a third of them deeper than level 1 -- most never
     * touch scratch now.  Path tracer (six quarters: its bounce): one whole level in LDS. */
    constexpr int LDSL = PT ? 1 : 0;
    constexpr int NLDS = PT ? 0 : QR_LDS_NARROW_LEVELS;
    constexpr int FQ = PT ? 6 : 4;              /* quarters per frame: the path tracer also keeps its bounce (q4, q5) */
    __shared__ f32x4 lds_frames[LDSL > 0 ? LDSL : 1][FQ][PT ? 64 : 1];
    __shared__ f32x4 lds_narrow[NLDS > 0 ? NLDS : 1][2][PT ? 1 : 64];
    f32x4 deep[PT ? QR_MAX_DEPTH - LDSL : 1][FQ];
    f32x4 deep_narrow[PT ? 1 : QR_MAX_DEPTH - NLDS][2];
    f32x4 deep_wide[PT ? 1 : QR_MAX_DEPTH][2];
    auto frame_put = [&](int level, int quarter, f32x4 v) {
        if constexpr (PT) { if (level < LDSL) lds_frames[level][quarter][lane] = v; else deep[level - LDSL][quarter] = v; }
        else if (quarter >= 2) deep_wide[level][quarter - 2] = v;
        else if (level < NLDS) lds_narrow[level][quarter][lane] = v;
        else deep_narrow[level - NLDS][quarter] = v;
    };
    auto frame_get = [&](int level, int quarter) -> f32x4 {
        if constexpr (PT) return level < LDSL ? lds_frames[level][quarter][lane] : deep[level - LDSL][quarter];
        else if (quarter >= 2) return deep_wide[level][quarter - 2];
        else return level < NLDS ? lds_narrow[level][quarter][lane] : deep_narrow[level - NLDS][quarter];
    };
    Outer ou;
    ou.sp = 0;
    ou.mode = inside ? 0 : 2;                   /* 0 trace, 1 return, 2 done */
    ou.ret = {0, 0, 0};
    ou.hit_id = -1;
    /* the primary hit id is only wanted by id renders and only when the wave ends: it waits in LDS, not in a register that
     * every frame's waves would carry through the whole recursion */
    __shared__ int lds_hit_id[64];
    if (ids != nullptr) lds_hit_id[lane] = -1;
    int &sp = ou.sp, &mode = ou.mode;
    V3 &ret = ou.ret;
    const int depth = lp.depth;

    if (COUNT && inside) cnt.primary++;
    QR_FLOPS_M(16, __popcll(__ballot(inside)));             /* primary ray */

    bool eager_done = false;
    if constexpr (PT && !PTV && !PTR)
    {
        if (ptp->eager)
        {
            ret = pt_eager(cx, ray, inside, depth, t_inf, rng, ptp->eager == 3);
            eager_done = true;
        }
    }

    while (!eager_done && any_lane(mode != 2))
    {
        const bool tr = mode == 0;
        bool ret_once = true;
#ifdef QR_STATS
        {
            const unsigned long long n_tr = (unsigned long long)__popcll(__ballot(tr)), n_on = (unsigned long long)__popcll(__ballot(mode != 2));
            if (__ffsll((long long)__ballot(true)) - 1 == lane) { atomicAdd(&cx.stats[28], 1ull); atomicAdd(&cx.stats[29], n_tr); atomicAdd(&cx.stats[30], n_on); }
        }
#endif
        if (any_lane(tr))
        {
            Hit h; bool occ;
            QR_WT(wt_t0 = __builtin_amdgcn_s_memrealtime();)
#if QR_DYN_PRIO
            if constexpr (!RAYS)
                if (prio_round < 3) { prio_round++; if (prio_round == 2) __builtin_amdgcn_s_setprio(2); else if (prio_round == 3) __builtin_amdgcn_s_setprio(3); }
#endif
            /* coherent: every ray of this round is a primary ray (neighbouring pixels; caller rays only when vouched for) */
            const bool coherent = (GATHER ? coh_in : (RAYS != 1 && RAYS != 6 && RAYS != 7 && RAYS != 8)) && !any_lane(tr && sp != 0);
            traverse<false, DIVK, RAYS != 0>(B, tr, coherent, ray, h, occ, cx.stats);
            QR_WT(if (wt_mid == 0) wt_mid = __builtin_amdgcn_s_memrealtime();)
            QR_WT(wt_push++;)
            QR_WT(wt_trav += __builtin_amdgcn_s_memrealtime() - wt_t0;)
            QR_WT(wt_t0 = __builtin_amdgcn_s_memrealtime();)
            if constexpr (VIEW && !PTV)
            {
                /* the first hit's t (the view's t_max where there is none), sample 0's: stored here, in the only round whose
                 * tracing lanes are at level 0, so that nothing waits in a register through the recursion for it */
                if (vp->depth != nullptr)
                {
                    int x_d, y_d, k_d;
                    const bool in_d = pixel_of_view(ord, fsaa, *vp, x_d, y_d, k_d) && k_d == 0;
                    if (in_d && tr && sp == 0)
                        vp->depth[((size_t)gw * (size_t)vp->height + (size_t)y_d) * (size_t)frm_w + (size_t)x_d] = h.t;
                }
            }
            const bool got = tr && h.srf != 0 && !QR_KNOB(4);
            if (tr && !got) { ret = {0, 0, 0}; mode = 1; }
            const int hsi = (int)((h.srf - QR_OFF_SRF) >> 7);          /* surface index: DSurf records are 128 B */
            if (ids != nullptr)
            {
                int lane_h = (int)(threadIdx.x & 63u);
                asm volatile("" : "+v"(lane_h));
                if (got && sp == 0) lds_hit_id[lane_h] = (hsi << 1) | h.side;
            }

            Shaded o;
            shade<COUNT, DIVK, PT>(cx, got, coherent, ray, h, o, cnt, &rng, depth - sp);
            QR_WT(wt_shade += __builtin_amdgcn_s_memrealtime() - wt_t0;)

            if (got)
            {
                const bool can_spawn = (depth - sp) != 0;
                /* PT: one more flag in front of the surface index: the node has a diffuse bounce to follow LAST (the
                 * node's colour is linear in its children: rfl c_rfl + trn c_trn + x0 (bounce l_dff tex + emission)).
                 * Children and colour association: DESIGN.md 4 "Path-tracer instance", order of draws, items 4 and 5,
                 * which the oracle's kernel order (qro_render_pt) restates */
                const bool has_pt = PT && o.want_pt && can_spawn;
                const int meta = PT ? ((hsi << 5) | (has_pt ? 16 : 0) | (h.side << 3) | (o.want_rf ? 4 : 0))
                                    : ((hsi << 4) | (h.side << 3) | (o.want_rf ? 4 : 0));
                if constexpr (PT)
                {
                    if (has_pt)
                    {
                        frame_put(sp, 4, f32x4{o.ptw.x * o.x0, o.ptw.y * o.x0, o.ptw.z * o.x0, 0.0f});
                        frame_put(sp, 5, f32x4{o.pdir.x, o.pdir.y, o.pdir.z, 0.0f});
                    }
                }
#ifdef QR_PROF
                {
                    /* frames pushed, by level (lanes): wide = both children, narrow = one */
                    const bool wide = o.want_tr && can_spawn && (o.want_rf || has_pt), narrow = can_spawn && !wide && (o.want_tr || o.want_rf);
                    for (int lv = 0; lv < 8; lv++)
                    {
                        const unsigned long long nw = __popcll(__ballot(wide && (sp < 7 ? sp : 7) == lv)), nn = __popcll(__ballot(narrow && (sp < 7 ? sp : 7) == lv));
                        if (nw) QR_PROF_ADD(32 + lv, nw);
                        if (nn) QR_PROF_ADD(40 + lv, nn);
                    }
                }
#endif
                if (o.want_tr && can_spawn)
                {
                    frame_put(sp, 0, f32x4{o.col.x, o.col.y, o.col.z, __int_as_float(meta | 1)});
                    frame_put(sp, 1, f32x4{o.c_trn, o.c_rfl, o.x0, o.hit.x});
                    if (o.want_rf || has_pt)
                    {
                        /* only a node that also has a reflection child needs its direction and local hit later */
                        frame_put(sp, 2, f32x4{o.rdir.x, o.rdir.y, o.rdir.z, o.hit.y});
                        frame_put(sp, 3, f32x4{o.loc.x, o.loc.y, o.loc.z, o.hit.z});
                    }
                    sp++;
                    ray.org = o.hit; ray.dir = o.tdir; ray.tmin = 0.0f; ray.tmax = t_inf;
                    ray.list = o.lst_tr; ray.osrf = h.srf; ray.oflg = h.side | FLAG_PASS_THRU;
                    ray.ploc = o.loc;
                    mode = 0;
                    if (COUNT) cnt.refract++;
                }
                else
                {
                    /* TR_mix with a zero child colour, 3560-3598 */
                    V3 c;
                    c.x = 0.0f + o.col.x * o.x0;
                    c.y = 0.0f + o.col.y * o.x0;
                    c.z = 0.0f + o.col.z * o.x0;
                    if (o.want_rf && can_spawn)
                    {
                        /* a reflection-only frame is read back for its colour and factor alone */
                        frame_put(sp, 0, f32x4{c.x, c.y, c.z, __int_as_float(meta | 2)});
                        frame_put(sp, 1, f32x4{o.c_trn, o.c_rfl, o.x0, o.hit.x});
                        if (has_pt)
                        {
                            frame_put(sp, 2, f32x4{0.0f, 0.0f, 0.0f, o.hit.y});
                            frame_put(sp, 3, f32x4{o.loc.x, o.loc.y, o.loc.z, o.hit.z});
                        }
                        sp++;
                        ray.org = o.hit; ray.dir = o.rdir; ray.tmin = 0.0f; ray.tmax = t_inf;
                        ray.list = o.lst_rf; ray.osrf = h.srf; ray.oflg = h.side;
                        ray.ploc = o.loc;
                        mode = 0;
                        if (COUNT) cnt.reflect++;
                    }
                    else
                    {
                        if (o.want_rf) { c.x = 0.0f + c.x; c.y = 0.0f + c.y; c.z = 0.0f + c.z; }
                        if (has_pt)
                        {
                            /* no other child: the bounce at once */
                            frame_put(sp, 0, f32x4{c.x, c.y, c.z, __int_as_float(meta | 3)});
                            sp++;
                            ray.org = o.hit; ray.dir = o.pdir; ray.tmin = 0.0f; ray.tmax = t_inf;
                            ray.list = o.lst_pt; ray.osrf = h.srf; ray.oflg = h.side;
                            ray.ploc = o.loc;
                            mode = 0;
                        }
                        else
                        {
                        ret = c;
                        mode = 1;
                        }
                    }
                }
            }
        }

        /* returns.  DIVK instance: a lane unwinds until its sample is finished or has its next ray (one level per round before
         * round 4) -- a lane's state machine does not depend on its neighbours, and every unfinished lane then traces in every
         * round: fewer, fuller rounds (config 5: +1.3 %).  The packet instance keeps one level per round */
        while ((QR_RETURN_LOOP && DIVK) ? mode == 1 : (mode == 1 && ret_once))
        {
            ret_once = false;
            if (sp == 0)
            {
                mode = 2;
            }
            else
            {
                const f32x4 q0 = frame_get(sp - 1, 0), q1 = frame_get(sp - 1, 1);
                const int fmeta = __float_as_int(q0.w);
                const int phase = fmeta & 3;
                constexpr int MS = PT ? 5 : 4;              /* surface index sits above the flags */
                /* PT: the node's other children are done, `c` is its colour without the bounce: follow the bounce now */
                auto bounce = [&](V3 c) {
                    const f32x4 q2 = frame_get(sp - 1, 2), q3 = frame_get(sp - 1, 3), q5 = frame_get(sp - 1, 5);
                    frame_put(sp - 1, 0, f32x4{c.x, c.y, c.z, __int_as_float(fmeta | 3)});
                    const int psi = fmeta >> MS, pside = (fmeta >> 3) & 1;
                    ray.org = {q1.w, q2.w, q3.w};
                    ray.dir = {q5.x, q5.y, q5.z};
                    ray.tmin = 0.0f; ray.tmax = t_inf;
                    ray.list = ((const DShade *)(cx.G + (cx.off_shade + (u32)psi * (u32)sizeof(DShade))))->lst[pside];
                    ray.osrf = QR_OFF_SRF + ((u32)psi << 7); ray.oflg = pside;
                    ray.ploc = {q3.x, q3.y, q3.z};
                    mode = 0;
                };
                if (PT && phase == 3)
                {
                    /* PT_ret 2598-2620: the bounce's colour times l_dff tex (times x0, see above) */
                    const f32x4 q4 = frame_get(sp - 1, 4);
                    ret.x = q0.x + ret.x * q4.x;
                    ret.y = q0.y + ret.y * q4.y;
                    ret.z = q0.z + ret.z * q4.z;
                    sp--;
                }
                else if (phase == 1)
                {
                    /* TR_ret + TR_mix 3534-3598 */
                    V3 c;
                    c.x = ret.x * q1.x + q0.x * q1.z;
                    c.y = ret.y * q1.x + q0.y * q1.z;
                    c.z = ret.z * q1.x + q0.z * q1.z;
                    if (fmeta & 4)
                    {
                        /* reflection child of the same node (depth budget is
                         * the same as for the refraction child) */
                        const f32x4 q2 = frame_get(sp - 1, 2), q3 = frame_get(sp - 1, 3);
                        frame_put(sp - 1, 0, f32x4{c.x, c.y, c.z, __int_as_float((fmeta & ~3) | 2)});
                        const int psi = fmeta >> MS, pside = (fmeta >> 3) & 1;
                        ray.org = {q1.w, q2.w, q3.w};
                        ray.dir = {q2.x, q2.y, q2.z};
                        ray.tmin = 0.0f; ray.tmax = t_inf;
                        ray.list = ((const DShade *)(cx.G + (cx.off_shade + (u32)psi * (u32)sizeof(DShade))))->lst[pside];
                        ray.osrf = QR_OFF_SRF + ((u32)psi << 7); ray.oflg = pside;
                        ray.ploc = {q3.x, q3.y, q3.z};
                        mode = 0;
                        if (COUNT) cnt.reflect++;
                    }
                    else if (PT && (fmeta & 16)) bounce(c);
                    else
                    {
                        ret = c;
                        sp--;
                    }
                }
                else
                {
                    /* RF_ret + RF_mix 3868-3908 */
                    V3 c;
                    c.x = ret.x * q1.y + q0.x;
                    c.y = ret.y * q1.y + q0.y;
                    c.z = ret.z * q1.y + q0.z;
                    if (PT && (fmeta & 16)) bounce(c);
                    else
                    {
                        ret = c;
                        sp--;
                    }
                }
            }
        }
    }

#ifdef QR_WAVETIME
    if (!COUNT && !RAYS && __ffsll((long long)__ballot(true)) - 1 == lane)
    {
        unsigned long long *o = counters + 64 + (size_t)gw * QR_WT_SLOTS;
        o[0] = wt_start; o[1] = wt_mid; o[2] = __builtin_amdgcn_s_memrealtime();
        o[12] = wt_clk0; o[13] = __builtin_amdgcn_s_memtime();
        o[4] = ord; o[5] = qr_wt_groups[0]; o[6] = qr_wt_groups[1]; o[7] = wt_push; o[8] = wt_trav; o[9] = wt_shade; o[10] = qr_wt_shadow;
        o[11] = (unsigned long long)qr_wt_cells[0] | ((unsigned long long)qr_wt_cells[1] << 16) | ((unsigned long long)qr_wt_cells[2] << 32) | ((unsigned long long)qr_wt_cells[3] << 48);
        o[3] = (unsigned long long)__builtin_amdgcn_s_getreg(4 | (31 << 11))
             | ((unsigned long long)(__builtin_amdgcn_s_getreg(20 | (3 << 11)) & 15) << 32)
             | ((unsigned long long)wt_push << 40);
    }
#endif
    if constexpr (PTV || PTR)
    {
        /* the sample's colour and the generator's state go back to the caller's loop: the running mean is taken there */
        *mean_out = ret;
        *rng_io = rng;
        return;
    }
    if constexpr (GATHER)
    {
        /* the ray's linear colour goes back to the caller's loop: the weighted sum is taken there */
        *mean_out = ret;
        return;
    }
    if constexpr (PT && !PTV && !PTR)
    {
        /* 5176-5219: running mean of the samples in the colour planes; the frame shows the mean so far */
        if (inside)
        {
            const size_t si = ((size_t)y * fr->fr.frm_row + x) * ns + k;
            ptp->seeds[si] = rng;
            const float ar = ret.x * ptp->pts_o + ptp->acc_r[si] * ptp->pts_u;
            const float ag = ret.y * ptp->pts_o + ptp->acc_g[si] * ptp->pts_u;
            const float ab = ret.z * ptp->pts_o + ptp->acc_b[si] * ptp->pts_u;
            ptp->acc_r[si] = ar; ptp->acc_g[si] = ag; ptp->acc_b[si] = ab;
            ret = {ar, ag, ab};
        }
    }
    if constexpr (CALLER_RAYS)
    {
        /* the linear colour (12 bytes per lane) and the first hit's id: no clamp, reduce, gamma or pack */
        if (inside)
        {
            const size_t i = (size_t)gw * 64u + (size_t)lane;
            rp->rgb[3 * i] = ret.x; rp->rgb[3 * i + 1] = ret.y; rp->rgb[3 * i + 2] = ret.z;
            if (ids != nullptr) ids[i] = lds_hit_id[lane];
        }
        return;
    }
    QR_FLOPS_M(6 + 2 * fsaa, __popcll(__ballot(inside)));
    /* XX_end 5161-5343: clamp, FSAA reduce, gamma, pack */
    float cr = clamp1(ret.x), cg = clamp1(ret.y), cb = clamp1(ret.z);
    if (fsaa >= 1)
    {
        cr = cr * 0.5f; cg = cg * 0.5f; cb = cb * 0.5f;
        cr = cr + __shfl_down(cr, 1); cg = cg + __shfl_down(cg, 1); cb = cb + __shfl_down(cb, 1);
    }
    if (fsaa >= 2)
    {
        cr = cr * 0.5f; cg = cg * 0.5f; cb = cb * 0.5f;
        cr = cr + __shfl_down(cr, 2); cg = cg + __shfl_down(cg, 2); cb = cb + __shfl_down(cb, 2);
    }
    if constexpr (MEAN)
    {
        *mean_out = {cr, cg, cb};
        return;
    }
    /* pixel coordinates and row ownership once more (pixel_of) */
    int x_e, y_e, k_e;
    bool inside_e;
    if constexpr (VIEW)
    {
        inside_e = pixel_of_view(ord, fsaa, *vp, x_e, y_e, k_e) && k_e == 0;
        const size_t view_px = (size_t)gw * (size_t)vp->height * (size_t)frm_w;       /* frames[view], ids[view] */
        frame += view_px;
        if (ids != nullptr) ids += view_px;
    }
    else inside_e = pixel_of(ord, fsaa, lp, fr, x_e, y_e, k_e) && k_e == 0;
    if (inside_e)
    {
        if (fr->fr.ctx_flags & QR_PROP_GAMMA)
        {
            asm volatile("" ::: "memory");      /* keep the branch: three IEEE square roots are not worth speculating */
            cr = __builtin_sqrtf(cr); cg = __builtin_sqrtf(cg); cb = __builtin_sqrtf(cb);
        }
        const float cl = fr->fr.clamp; const u32 cmask = fr->fr.cmask;
        cr = cr * cl; cg = cg * cl; cb = cb * cl;
        const u32 p = (((u32)cvt_near(cr) & cmask) << 16) |
                      (((u32)cvt_near(cg) & cmask) << 8) |
                       ((u32)cvt_near(cb) & cmask);
        frame[(size_t)y_e * frm_w + x_e] = p;
        if (ids != nullptr)
        {
            int lane_e = (int)(threadIdx.x & 63u);
            asm volatile("" : "+v"(lane_e));        /* not the address register of the wave's first instructions, kept alive */
            ids[(size_t)y_e * frm_w + x_e] = lds_hit_id[lane_e];
        }
    }

    if (COUNT)
    {
        /* one atomic per wave and counter */
        unsigned long long v[4] = { cnt.primary, cnt.shadow, cnt.reflect, cnt.refract };
        for (int i = 0; i < 4; i++)
        {
            unsigned long long s = v[i];
            for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
            if (lane == 0 && s != 0) atomicAdd(&counters[i], s);
        }
    }
}

/* single-scene launch */
template <bool COUNT, int WAVES, bool DIVK>
__global__ __launch_bounds__(QR_BLOCK, WAVES)
void qr_render_kernel(LaunchP lp, uint32_t *__restrict__ frame, int32_t *__restrict__ ids,
                      unsigned long long *__restrict__ counters)
{
    const int gw = __builtin_amdgcn_readfirstlane((int)blockIdx.x * (QR_BLOCK / 64) + (int)(threadIdx.x >> 6));
    if (gw >= lp.n_blocks) return;
    /* schedule entry {footprint coordinates, tile-list offset or QR_PER_LANE_TILE}: one scalar load */
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const u32x2 sched = ((const QR_CONST u32x2 *)lp.order)[gw];
#pragma clang diagnostic pop
    render_wave<COUNT, DIVK>(lp, sched.x, sched.y, gw, frame, ids, counters);
}

/* path-tracer launch: one sample per pixel sample and call, accumulated in the planes of `pt` */
__global__ __launch_bounds__(QR_BLOCK, 3)
void qr_render_pt_kernel(LaunchP lp, PtParams pt, uint32_t *__restrict__ frame, unsigned long long *__restrict__ counters)
{
    const int gw = __builtin_amdgcn_readfirstlane((int)blockIdx.x * (QR_BLOCK / 64) + (int)(threadIdx.x >> 6));
    if (gw >= lp.n_blocks) return;
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const u32x2 sched = ((const QR_CONST u32x2 *)lp.order)[gw];
#pragma clang diagnostic pop
    render_wave<false, false, true>(lp, sched.x, sched.y, gw, frame, nullptr, counters, &pt);
}

/*
 * Ray shading (qr_shade_rays_async): one lane per caller ray, 64 per wave, one wave per workgroup; the per-lane walk instance
 * of the renderer's machine (caller rays may be incoherent, and only it knows shadow grids).  COHERENT: QR_TRACE_COHERENT.
 */
template <bool COHERENT>
__global__ __launch_bounds__(QR_BLOCK, QR_DIVK_WAVES)
void qr_shade_rays_kernel(LaunchP lp, RaysP rp, int32_t *__restrict__ ids)
{
    const int gw = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
    render_wave<false, true, false, COHERENT ? 2 : 1>(lp, 0u, 0u, gw, nullptr, ids, nullptr, nullptr, &rp);
}

/*
 * View rendering (qr_render_views_async): the grid is (footprint columns, footprint rows, views), one wave per workgroup.  The
 * first round is the frame's: neighbouring pixels of one camera, packet walks.  Two instances, chosen as render() chooses its
 * own: the per-lane walks for scenes with long hierarchies or grids (the ray-query list of a large scene is long), the packet
 * walks alone for the others -- demo scene 1 at 1080p: 0.194 ms against 0.258 ms at depth 10, 0.143 against 0.188 at depth 0
 * (profiles/r07_render_views.txt).
 */
template <bool DIVK, int WAVES>
__global__ __launch_bounds__(QR_BLOCK, WAVES)
void qr_render_views_kernel(LaunchP lp, ViewsP vp, uint32_t *__restrict__ frames, int32_t *__restrict__ ids)
{
    const u32 ord = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x | (blockIdx.y << 14)));
    const int view = __builtin_amdgcn_readfirstlane((int)blockIdx.z);
    render_wave<false, DIVK, false, 3>(lp, ord, 0u, view, frames, ids, nullptr, nullptr, nullptr, &vp);
}

/*
 * The pieces the kernels below are composed of.  Their operation order is the interface: rays.py states it in
 * numpy and the tests compare bit for bit.  render_wave keeps its own copy of the output step: its assembly is what bench.py times.
 */

/* XX_end 5161-5343, first half: clamp and FSAA reduce, by EVERY lane of the wave (the reduce needs all samples of a pixel; sample
 * 0's lane ends with the pixel's colour).  cn: an integer per sample that takes the same reduce, unscaled */
__device__ __forceinline__ void fsaa_reduce(const int fsaa, float &cr, float &cg, float &cb, int *cn = nullptr)
{
    cr = clamp1(cr); cg = clamp1(cg); cb = clamp1(cb);
    if (fsaa >= 1)
    {
        cr = cr * 0.5f; cg = cg * 0.5f; cb = cb * 0.5f;
        cr = cr + __shfl_down(cr, 1); cg = cg + __shfl_down(cg, 1); cb = cb + __shfl_down(cb, 1);
        if (cn != nullptr) *cn = *cn + __shfl_down(*cn, 1);
    }
    if (fsaa >= 2)
    {
        cr = cr * 0.5f; cg = cg * 0.5f; cb = cb * 0.5f;
        cr = cr + __shfl_down(cr, 2); cg = cg + __shfl_down(cg, 2); cb = cb + __shfl_down(cb, 2);
        if (cn != nullptr) *cn = *cn + __shfl_down(*cn, 2);
    }
}

/* ... second half: gamma, scale, round, mask, pack */
__device__ __forceinline__ u32 pack_pixel(FrmP fr, float cr, float cg, float cb)
{
    if (fr->fr.ctx_flags & QR_PROP_GAMMA)
    {
        asm volatile("" ::: "memory");      /* keep the branch: three IEEE square roots are not worth speculating */
        cr = __builtin_sqrtf(cr); cg = __builtin_sqrtf(cg); cb = __builtin_sqrtf(cb);
    }
    const float cl = fr->fr.clamp; const u32 cmask = fr->fr.cmask;
    cr = cr * cl; cg = cg * cl; cb = cb * cl;
    return (((u32)cvt_near(cr) & cmask) << 16) | (((u32)cvt_near(cg) & cmask) << 8) | ((u32)cvt_near(cb) & cmask);
}

/* 5176-5219: the running mean after sample `number` (1-based, counted from the state's reset) of a lane whose means wait in
 * column l of `acc`: weights 1.0f / (float)number and 1.0f - that, IEEE division, the bits of the host's (qr_device.hip
 * launch<>).  The generator's state is parked beside it; the means only when another sample follows (`more`) */
__device__ __forceinline__ V3 pt_mean_fold(u32 *rng_col, float (*acc)[64], const int l, const u32 rng, const V3 c, const int number,
                                           const bool more)
{
    const float pts_o = 1.0f / (float)number, pts_u = 1.0f - pts_o;
    V3 m;
    m.x = c.x * pts_o + acc[0][l] * pts_u;
    m.y = c.y * pts_o + acc[1][l] * pts_u;
    m.z = c.z * pts_o + acc[2][l] * pts_u;
    rng_col[l] = rng;
    if (more) { acc[0][l] = m.x; acc[1][l] = m.y; acc[2][l] = m.z; }
    return m;
}

/*
 * The adaptive state (include/qrhip.h): eight planes of 32-bit words -- the LCG state, the running means of r, g, b, the count m,
 * Welford's M2 of r, g, b -- a column per ray or per slot.  A wave keeps 64 columns in LDS (`st`, [word][lane], 2 KB); a lane finds
 * its column in memory as state[p * stride + col].  The ray, list and view kernels differ only in stride and col.
 */

/* the stop rule on values: the only statement of the expression of include/qrhip.h.  Vector compares whose lane masks are
 * combined as scalars: no branch */
__device__ __forceinline__ bool pt_adapt_rule(const u32 m, const float m2r, const float m2g, const float m2b, const u32 min_samples,
                                              const u32 max_samples, const float tol2)
{
    float lim = (float)m * (float)(m - 1u);
    lim = lim * tol2;
    const bool conv = m2r <= lim && m2g <= lim && m2b <= lim;
    return m < max_samples && (m < min_samples || m < 2u || !conv);
}

/* ... on column l of the wave's state */
__device__ __forceinline__ bool pt_adapt_take(const u32 (*st)[64], const int l, const int min_samples, const int max_samples, const float tol2)
{
    return pt_adapt_rule(st[4][l], u2f(st[5][l]), u2f(st[6][l]), u2f(st[7][l]), (u32)min_samples, (u32)max_samples, tol2);
}

/* the wave's state from memory.  A lane outside the launch holds m = max_samples: the rule never lets it take */
__device__ __forceinline__ void pt_adapt_load(u32 (*st)[64], const int l, const u32 *state, const size_t stride, const size_t col,
                                              const bool inside, const int max_samples)
{
    u32 w[QR_PT_ADAPT_STATE_WORDS] = {0u, 0u, 0u, 0u, (u32)max_samples, 0u, 0u, 0u};
    if (inside)
    {
#pragma unroll
        for (int p = 0; p < QR_PT_ADAPT_STATE_WORDS; p++) w[p] = state[(size_t)p * stride + col];
    }
#pragma unroll
    for (int p = 0; p < QR_PT_ADAPT_STATE_WORDS; p++) st[p][l] = w[p];
}

/* one sample of colour c into column l: Welford's update, one fp32 operation per step, the division IEEE */
__device__ __forceinline__ void pt_adapt_fold(u32 (*st)[64], const int l, const u32 rng, const V3 c)
{
    const u32 m = st[4][l] + 1u;
    const float o = 1.0f / (float)m, u = 1.0f - o;
    st[4][l] = m;
    st[0][l] = rng;
    const float col[3] = {c.x, c.y, c.z};
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
    {
        const float mean = u2f(st[1 + ch][l]);
        const float d1 = col[ch] - mean;
        const float a = col[ch] * o, b = mean * u;
        const float mn = a + b;
        const float d2 = col[ch] - mn;
        const float p = d1 * d2;
        st[1 + ch][l] = f2u(mn);
        st[5 + ch][l] = f2u(u2f(st[5 + ch][l]) + p);
    }
}

/* column l back to memory, by a lane inside the launch: a column that took a sample holds more than it came with, so the count in
 * memory says which columns to write (no flag is carried through the samples) */
__device__ __forceinline__ void pt_adapt_store(const u32 (*st)[64], const int l, u32 *state, const size_t stride, const size_t col)
{
    if (st[4][l] != state[4 * stride + col])
    {
#pragma unroll
        for (int p = 0; p < QR_PT_ADAPT_STATE_WORDS; p++) state[(size_t)p * stride + col] = st[p][l];
    }
}

/* `open` (may be null): ONE vector atomic add per wave, from its first lane, of the number of lanes the rule on the final state
 * still lets take, and none when that number is 0 */
__device__ __forceinline__ void pt_adapt_open(u32 *open, const u32 (*st)[64], const int l, const int min_samples, const int max_samples,
                                              const float tol2)
{
    if (open != nullptr)
    {
        const unsigned long long still = __ballot(pt_adapt_take(st, l, min_samples, max_samples, tol2));
        if (still != 0ull && l == 0) atomicAdd(open, (u32)__popcll(still));
    }
}

/*
 * View accumulation (qr_render_views_mean_async): the grid is the footprints of ONE frame, one wave per workgroup; the wave renders
 * its footprint from every view of the launch in array order (a wave-uniform loop: the view record comes through scalar loads,
 * as in a view launch) and keeps the running sum of the reduced linear colours -- one fp32 add per channel and view, in order,
 * never fused (-ffp-contract=off) -- for the lanes that hold sample 0 (in LDS between views, see below).  The sum is stored once,
 * after the loop, with the optional packed pixel (the rest of the output step on sum * scale): 12 to 16 bytes of global traffic per pixel
 * however many views there are.  QR_MEAN_RESUME: the sum starts from sum[p] instead of the first view's colour.  One wave per
 * footprint whatever n_views is: a small frame does not fill the machine (include/qrhip.h).  Instances as the view launch's.
 */
template <bool DIVK, int WAVES>
__global__ __launch_bounds__(QR_BLOCK, WAVES)
void qr_views_mean_kernel(LaunchP lp, ViewsP vp, int n_views, float *__restrict__ sum, uint32_t *__restrict__ frame,
                          float scale, u32 resume)
{
    const u32 ord = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x | (blockIdx.y << 14)));
    /* the running sum waits in LDS while a view is rendered (768 B per wave): live in registers across render_wave it cost the
     * per-lane instance 13 more spilled registers (26: over its budget) and the packet instance 7 */
    __shared__ float lds_sum[3][64];
    const int lane = (int)(threadIdx.x & 63u);
    if (resume)
    {
        const int fsaa_r = c_frm((BaseP)lp.B)->fr.fsaa;
        int x_r, y_r, k_r;
        if (pixel_of_view(ord, fsaa_r, vp, x_r, y_r, k_r) && k_r == 0)
        {
            const float *p = sum + 3 * ((size_t)y_r * (size_t)vp.width + (size_t)x_r);
            lds_sum[0][lane] = p[0]; lds_sum[1][lane] = p[1]; lds_sum[2][lane] = p[2];
        }
    }
    V3 s = {0.0f, 0.0f, 0.0f};
#pragma nounroll
    for (int v = 0; v < n_views; v++)
    {
        V3 c;
        render_wave<false, DIVK, false, 4>(lp, ord, 0u, __builtin_amdgcn_readfirstlane(v), nullptr, nullptr, nullptr, nullptr,
                                           nullptr, &vp, &c);
        int lane_s = (int)(threadIdx.x & 63u);
        asm volatile("" : "+v"(lane_s));            /* not an address register kept alive through the view */
        if (v == 0 && !resume) s = c;
        else
        {
            s.x = lds_sum[0][lane_s] + c.x; s.y = lds_sum[1][lane_s] + c.y; s.z = lds_sum[2][lane_s] + c.z;
        }
        if (v + 1 < n_views) { lds_sum[0][lane_s] = s.x; lds_sum[1][lane_s] = s.y; lds_sum[2][lane_s] = s.z; }
    }
    const FrmP fr = c_frm((BaseP)lp.B);
    int x_e, y_e, k_e;
    if (pixel_of_view(ord, fr->fr.fsaa, vp, x_e, y_e, k_e) && k_e == 0)
    {
        const size_t px = (size_t)y_e * (size_t)vp.width + (size_t)x_e;
        sum[3 * px] = s.x; sum[3 * px + 1] = s.y; sum[3 * px + 2] = s.z;
        if (frame != nullptr)
        {
            /* the rest of the output step on the scaled sum */
            frame[px] = pack_pixel(fr, s.x * scale, s.y * scale, s.z * scale);
        }
    }
}

/*
 * Path-traced views (qr_pt_views_async): the grid is (footprint columns, footprint rows, views), one wave per workgroup, as in a
 * view launch; the wave adds pv.samples samples to its footprint in a wave-uniform loop.  What the engine keeps per pixel sample
 * (PtParams: one LCG state, three running means) is read from the caller's state once, waits in LDS while a sample is traced
 * (1 KB per wave: nothing of it is live in registers through the recursion but the generator's state, which the path tracer
 * carries anyway), and is written back once, after the last sample; then the frame's output step (fsaa_reduce, pack_pixel) runs
 * once on the means.  The running mean is pt_mean_fold's; its weights are wave-uniform.  The path-tracer instance's walks and
 * launch bound.
 */
__global__ __launch_bounds__(QR_BLOCK, 3)
void qr_pt_views_kernel(LaunchP lp, ViewsP vp, PtViewsP pv, uint32_t *__restrict__ frames)
{
    const u32 ord = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x | (blockIdx.y << 14)));
    const int view = __builtin_amdgcn_readfirstlane((int)blockIdx.z);
    __shared__ u32 lds_rng[64];
    __shared__ float lds_acc[3][64];
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const FrmP fr = c_frm((BaseP)lp.B);
#pragma clang diagnostic pop
    const int fsaa = fr->fr.fsaa;
    const size_t slots = (size_t)vp.width * (size_t)vp.height << fsaa;      /* of one view, of one plane */
    u32 *const st = pv.state + (size_t)view * 4u * slots;
    const int lane = (int)(threadIdx.x & 63u);
    {
        int x_r, y_r, k_r;
        if (pixel_of_view(ord, fsaa, vp, x_r, y_r, k_r))
        {
            const size_t si = (((size_t)y_r * (size_t)vp.width + (size_t)x_r) << fsaa) + (size_t)k_r;
            lds_rng[lane] = st[si];
            lds_acc[0][lane] = u2f(st[slots + si]); lds_acc[1][lane] = u2f(st[2 * slots + si]); lds_acc[2][lane] = u2f(st[3 * slots + si]);
        }
    }
    V3 m = {0.0f, 0.0f, 0.0f};
#pragma nounroll
    for (int s = 0; s < pv.samples; s++)
    {
        int lane_s = (int)(threadIdx.x & 63u);
        asm volatile("" : "+v"(lane_s));            /* not an address register kept alive through the sample */
        u32 rng = lds_rng[lane_s];
        V3 c;
        render_wave<false, false, true, 5>(lp, ord, 0u, view, nullptr, nullptr, nullptr, nullptr, nullptr, &vp, &c, &rng);
        asm volatile("" : "+v"(lane_s));
        /* lanes outside the frame carry zeros and a state nobody reads */
        m = pt_mean_fold(lds_rng, lds_acc, lane_s, rng, c, pv.done + s + 1, s + 1 < pv.samples);
    }
    int x_e, y_e, k_e;
    const bool inside_e = pixel_of_view(ord, fsaa, vp, x_e, y_e, k_e);
    if (inside_e)
    {
        const size_t si = (((size_t)y_e * (size_t)vp.width + (size_t)x_e) << fsaa) + (size_t)k_e;
        st[si] = lds_rng[lane];
        st[slots + si] = f2u(m.x); st[2 * slots + si] = f2u(m.y); st[3 * slots + si] = f2u(m.z);
    }
    /* the frame's output step on the means */
    float cr = m.x, cg = m.y, cb = m.z;
    fsaa_reduce(fsaa, cr, cg, cb);
    if (inside_e && k_e == 0)
    {
        const size_t px = ((size_t)view * (size_t)vp.height + (size_t)y_e) * (size_t)vp.width + (size_t)x_e;
        if (pv.mean != nullptr) { pv.mean[3 * px] = cr; pv.mean[3 * px + 1] = cg; pv.mean[3 * px + 2] = cb; }
        frames[px] = pack_pixel(fr, cr, cg, cb);
    }
}

/*
 * Path-traced rays (qr_pt_rays_async): one lane per caller ray, 64 per wave, one wave per workgroup, as in ray shading; the wave
 * adds `samples` samples to its rays in a wave-uniform loop.  state: four planes of n 32-bit words --
 * the LCG states, then the running means of r, g, b -- ray i is column i (include/qrhip.h).  It is read once before the first
 * sample, waits in LDS while a sample is traced (1 KB per wave: nothing of it is live in registers through the recursion but the
 * generator's state, which the path tracer carries anyway) and is written once after the last, with the optional rgb; the ray
 * and its spread are read again by every sample.  The running mean of sample number done + s + 1 is pt_mean_fold's.
 * A lane past n reads and writes nothing.  The path-tracer instance's walks (packet walks only) and launch bound.
 */
__global__ __launch_bounds__(QR_BLOCK, 3)
void qr_pt_rays_kernel(LaunchP lp, PtRaysP pr, u32 *__restrict__ state, int done, int samples)
{
    const int gw = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
    __shared__ u32 lds_rng[64];
    __shared__ float lds_acc[3][64];
    const size_t n = (size_t)(u32)pr.n;
    const int lane = (int)(threadIdx.x & 63u);
    {
        const size_t i = (size_t)(u32)gw * 64u + (size_t)lane;
        if (i < n)
        {
            lds_rng[lane] = state[i];
            lds_acc[0][lane] = u2f(state[n + i]); lds_acc[1][lane] = u2f(state[2 * n + i]); lds_acc[2][lane] = u2f(state[3 * n + i]);
        }
    }
    V3 m = {0.0f, 0.0f, 0.0f};
#pragma nounroll
    for (int s = 0; s < samples; s++)
    {
        int lane_s = (int)(threadIdx.x & 63u);
        asm volatile("" : "+v"(lane_s));            /* not an address register kept alive through the sample */
        u32 rng = lds_rng[lane_s];
        V3 c;
        render_wave<false, false, true, 6>(lp, 0u, 0u, gw, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &c, &rng, &pr);
        asm volatile("" : "+v"(lane_s));
        /* lanes past n carry zeros and a state nobody reads */
        m = pt_mean_fold(lds_rng, lds_acc, lane_s, rng, c, done + s + 1, s + 1 < samples);
    }
    int lane_e = (int)(threadIdx.x & 63u);
    asm volatile("" : "+v"(lane_e));
    const size_t i_e = (size_t)(u32)gw * 64u + (size_t)lane_e;
    if (i_e < n)
    {
        state[i_e] = lds_rng[lane_e];
        state[n + i_e] = f2u(m.x); state[2 * n + i_e] = f2u(m.y); state[3 * n + i_e] = f2u(m.z);
        if (pr.rgb != nullptr) { pr.rgb[3 * i_e] = m.x; pr.rgb[3 * i_e + 1] = m.y; pr.rgb[3 * i_e + 2] = m.z; }
    }
}

/*
 * Adaptive path-traced rays (qr_pt_adapt_rays_async): qr_pt_rays_kernel with a sample count and a noise estimate per ray and a
 * stop rule evaluated on chip.  state: eight planes of n 32-bit words -- the LCG states, the running means of r, g, b, the count
 * m of samples the ray holds, Welford's M2 (sum of squared deviations) of r, g, b -- ray i is column i (include/qrhip.h).  All
 * eight words are read once (pt_adapt_load) and wait in LDS (2 KB per wave); nothing of them is live in registers through a
 * sample but the generator's state.  Before every candidate sample each lane evaluates the rule on its own column (pt_adapt_take):
 *     take = m < max && (m < min || m < 2 || !(M2r <= lim && M2g <= lim && M2b <= lim)),  lim = ((float)m * (float)(m - 1)) * tol2
 * (per-lane data, so vector compares; only the ballot is scalar).  A lane that does not take a candidate takes none later in the
 * launch -- its column did not change -- and is out of the sample like a lane past n (render_wave RAYS = 7); the wave leaves the
 * loop when no lane is left, so a wave runs as long as its slowest ray.  The update is Welford's (pt_adapt_fold).  The state is
 * written back once, by the lanes that took a sample (pt_adapt_store); rgb by every lane below n; `open` gets ONE vector atomic
 * add per wave (pt_adapt_open).
 */
__global__ __launch_bounds__(QR_BLOCK, 3)
void qr_pt_adapt_kernel(LaunchP lp, PtRaysP pr, u32 *__restrict__ state, int samples, int min_samples, int max_samples, float tol2,
                        u32 *__restrict__ open)
{
    const int gw = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
    __shared__ u32 lds_st[QR_PT_ADAPT_STATE_WORDS][64];
    const size_t n = (size_t)(u32)pr.n;
    const int lane = (int)(threadIdx.x & 63u);
    const size_t i = (size_t)(u32)gw * 64u + (size_t)lane;
    pt_adapt_load(lds_st, lane, state, n, i, i < n, max_samples);
#pragma nounroll
    for (int s = 0; s < samples; s++)
    {
        int lane_s = (int)(threadIdx.x & 63u);
        asm volatile("" : "+v"(lane_s));            /* not an address register kept alive through the sample */
        const bool take = pt_adapt_take(lds_st, lane_s, min_samples, max_samples, tol2);
        if (!any_lane(take)) break;
        u32 rng = lds_st[0][lane_s];
        V3 c;
        render_wave<false, false, true, 7>(lp, 0u, 0u, gw, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &c, &rng, &pr, take);
        asm volatile("" : "+v"(lane_s));
        if (take) pt_adapt_fold(lds_st, lane_s, rng, c);
    }
    int lane_e = (int)(threadIdx.x & 63u);
    asm volatile("" : "+v"(lane_e));
    const size_t i_e = (size_t)(u32)gw * 64u + (size_t)lane_e;
    if (i_e < n)
    {
        pt_adapt_store(lds_st, lane_e, state, n, i_e);
        if (pr.rgb != nullptr)
        {
            pr.rgb[3 * i_e] = u2f(lds_st[1][lane_e]); pr.rgb[3 * i_e + 1] = u2f(lds_st[2][lane_e]); pr.rgb[3 * i_e + 2] = u2f(lds_st[3][lane_e]);
        }
    }
    pt_adapt_open(open, lds_st, lane_e, min_samples, max_samples, tol2);
}

/*
 * Adaptive path-traced views (qr_pt_adapt_views_async): the grid of a view launch -- (footprint columns, footprint rows, views),
 * one wave per workgroup -- around the adaptive sample loop.  state: per view eight planes of width * height *
 * samples-per-pixel 32-bit words, the adaptive state's planes, slot (y * width + x) * samples-per-pixel + k: one view's block is
 * an adaptive ray state of `slots` columns.  All eight words wait in LDS (2 KB per wave); nothing of them is live in registers
 * through a sample but the generator's state.  The rule is evaluated PER SLOT, per
 * pixel sample and not per pixel, at the top of the wave-uniform loop; a lane outside the frame holds m = max_samples and never
 * takes; a lane that does not take is out of the sample like a lane past the frame's edge (render_wave RAYS = 9); the wave leaves
 * when no lane is left, so it runs as long as its slowest slot.  Rule, update, write-back and `open` are the adaptive state's
 * functions (pt_adapt_take, _fold, _store, _open) on stride `slots` and column `si`.  After the write-back EVERY lane runs the
 * frame's output step on the means read back from LDS (the FSAA reduce needs all lanes of a pixel, taken or not); the counts
 * are reduced the same way in integers.
 */
struct PtAdaptViewsP { u32 *state; int32_t samples, min_samples, max_samples; float tol2; float *mean; int32_t *counts; u32 *open; };

__global__ __launch_bounds__(QR_BLOCK, 3)
void qr_pt_adapt_views_kernel(LaunchP lp, ViewsP vp, PtAdaptViewsP pa, uint32_t *__restrict__ frames)
{
    const u32 ord = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x | (blockIdx.y << 14)));
    const int view = __builtin_amdgcn_readfirstlane((int)blockIdx.z);
    __shared__ u32 lds_st[QR_PT_ADAPT_STATE_WORDS][64];
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const FrmP fr = c_frm((BaseP)lp.B);
#pragma clang diagnostic pop
    const int fsaa = fr->fr.fsaa;
    const size_t slots = (size_t)vp.width * (size_t)vp.height << fsaa;      /* of one view, of one plane */
    u32 *const st = pa.state + (size_t)view * (size_t)QR_PT_ADAPT_STATE_WORDS * slots;
    const int max_samples = pa.max_samples, min_samples = pa.min_samples;
    const float tol2 = pa.tol2;
    {
        int x_r, y_r, k_r;
        const bool inside_r = pixel_of_view(ord, fsaa, vp, x_r, y_r, k_r);
        /* pixel_of_view always writes x, y and k, so si is a number for a lane outside the frame too; only `inside_r` lanes read */
        const size_t si = (((size_t)y_r * (size_t)vp.width + (size_t)x_r) << fsaa) + (size_t)k_r;
        pt_adapt_load(lds_st, (int)(threadIdx.x & 63u), st, slots, si, inside_r, max_samples);
    }
#pragma nounroll
    for (int s = 0; s < pa.samples; s++)
    {
        int lane_s = (int)(threadIdx.x & 63u);
        asm volatile("" : "+v"(lane_s));            /* not an address register kept alive through the sample */
        const bool take = pt_adapt_take(lds_st, lane_s, min_samples, max_samples, tol2);
        if (!any_lane(take)) break;
        u32 rng = lds_st[0][lane_s];
        V3 c;
        render_wave<false, false, true, 9>(lp, ord, 0u, view, nullptr, nullptr, nullptr, nullptr, nullptr, &vp, &c, &rng, nullptr, take);
        asm volatile("" : "+v"(lane_s));
        if (take) pt_adapt_fold(lds_st, lane_s, rng, c);
    }
    int lane_e = (int)(threadIdx.x & 63u);
    asm volatile("" : "+v"(lane_e));
    int x_e, y_e, k_e;
    const bool inside_e = pixel_of_view(ord, fsaa, vp, x_e, y_e, k_e);
    if (inside_e)
    {
        const size_t si = (((size_t)y_e * (size_t)vp.width + (size_t)x_e) << fsaa) + (size_t)k_e;
        pt_adapt_store(lds_st, lane_e, st, slots, si);
    }
    /* the frame's output step on the means, by every lane: lanes outside the frame carry zeros.  The counts take the same
     * reduce in integers */
    float cr = u2f(lds_st[1][lane_e]), cg = u2f(lds_st[2][lane_e]), cb = u2f(lds_st[3][lane_e]);
    int cn = inside_e ? (int)lds_st[4][lane_e] : 0;
    fsaa_reduce(fsaa, cr, cg, cb, &cn);
    if (inside_e && k_e == 0)
    {
        const size_t px = ((size_t)view * (size_t)vp.height + (size_t)y_e) * (size_t)vp.width + (size_t)x_e;
        if (pa.mean != nullptr) { pa.mean[3 * px] = cr; pa.mean[3 * px + 1] = cg; pa.mean[3 * px + 2] = cb; }
        if (pa.counts != nullptr) pa.counts[px] = cn;
        frames[px] = pack_pixel(fr, cr, cg, cb);
    }
    pt_adapt_open(pa.open, lds_st, lane_e, min_samples, max_samples, tol2);
}

/*
 * Indexed adaptive path-traced rays (qr_pt_adapt_list_rays_async): adaptive path-traced rays with the wave's 64 rays taken from a
 * list of ray indices instead of from 64 consecutive columns, so that the rays a stop rule has left open -- scattered among rays that have
 * stopped -- fill whole waves (the list: qr_openlist.hpp, or any list of distinct indices the caller makes).  Wave w serves list
 * positions 64 w .. 64 w + 63 below min(cap, *count); *count is one scalar load, and a wave at or past it leaves before it touches
 * anything else.  Lane l reads its entry i once; the ray's and the spread's rows, the eight state words and the rgb row are all
 * addressed by i.  An entry >= n, and a position past the end, is a lane outside: it holds the sentinel index and m = max_samples,
 * so the rule never lets it take, and reads and writes nothing.  The index waits in LDS beside the state (2 KB + 256 B per wave)
 * and is read again at the top of every sample, as lane_s is made again: it is not a register live through the recursion.
 * Everything else is the adaptive state's functions on stride n and column i: the rule at the top of the wave-uniform sample
 * loop, any_lane(take) the exit, Welford's update, a column written back only when its count changed, rgb for the listed rays
 * only, `open` one vector atomic add per wave.  A ray's result depends on nothing but its own column, ray and spread, so the
 * state after the call is bit for bit the state qr_pt_adapt_kernel leaves on the listed columns.
 */
__global__ __launch_bounds__(QR_BLOCK, 3)
void qr_pt_list_kernel(LaunchP lp, PtRaysP pr, u32 *__restrict__ state, const u32 *__restrict__ index, const u32 *__restrict__ count,
                       u32 cap, int samples, int min_samples, int max_samples, float tol2, u32 *__restrict__ open)
{
    const int gw = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
    const u32 cnt = *count;                                 /* wave-uniform address: a scalar load */
    const u32 lim = cnt < cap ? cnt : cap;
    if ((u32)gw * 64u >= lim) return;
    __shared__ u32 lds_st[QR_PT_ADAPT_STATE_WORDS][64];
    __shared__ u32 lds_ix[64];
    const u32 n = (u32)pr.n;
    constexpr u32 NONE = 0xFFFFFFFFu;                       /* n <= INT32_MAX: never a ray */
    const int lane = (int)(threadIdx.x & 63u);
    {
        const u32 p = (u32)gw * 64u + (u32)lane;
        u32 ix = NONE;
        if (p < lim) { ix = index[p]; if (ix >= n) ix = NONE; }
        lds_ix[lane] = ix;
        pt_adapt_load(lds_st, lane, state, n, ix, ix != NONE, max_samples);
    }
#pragma nounroll
    for (int s = 0; s < samples; s++)
    {
        int lane_s = (int)(threadIdx.x & 63u);
        asm volatile("" : "+v"(lane_s));            /* not an address register kept alive through the sample */
        const bool take = pt_adapt_take(lds_st, lane_s, min_samples, max_samples, tol2);
        if (!any_lane(take)) break;
        u32 rng = lds_st[0][lane_s];
        const u32 ri = lds_ix[lane_s];              /* dead after the ray's rows are read */
        V3 c;
        render_wave<false, false, true, 8>(lp, 0u, 0u, gw, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &c, &rng, &pr, take, ri);
        asm volatile("" : "+v"(lane_s));
        if (take) pt_adapt_fold(lds_st, lane_s, rng, c);
    }
    int lane_e = (int)(threadIdx.x & 63u);
    asm volatile("" : "+v"(lane_e));
    const u32 i_e = lds_ix[lane_e];
    if (i_e < n)
    {
        pt_adapt_store(lds_st, lane_e, state, n, i_e);
        if (pr.rgb != nullptr)
        {
            const size_t o3 = 3 * (size_t)i_e;
            pr.rgb[o3] = u2f(lds_st[1][lane_e]); pr.rgb[o3 + 1] = u2f(lds_st[2][lane_e]); pr.rgb[o3 + 2] = u2f(lds_st[3][lane_e]);
        }
    }
    pt_adapt_open(open, lds_st, lane_e, min_samples, max_samples, tol2);
}

/*
 * Multi-target launch (qr_render_multi_async): ONE grid renders row ranges of several frames -- of the
 * same or of different scenes -- so that the N blocks a GPU owns in a sharded step share one launch: a
 * frame cut into N small launches pays N ramps, drains and tails (0.23 ms for 8 blocks of demo1 at
 * 1080p against 0.09 ms for the whole frame).  Schedule entries are 16 bytes {footprint, tile-list
 * offset, target index, 0}, heavy footprints of all targets first.  Everything a target needs travels
 * in the kernel arguments (nothing of a scene's launch state is cached on the device).
 */
#define QR_MAX_TARGETS 16
struct DevTarget { uint32_t *frame; const char *B; int32_t row_begin, row_end; int32_t depth, pad; };
struct DevTargets { DevTarget t[QR_MAX_TARGETS]; };

template <int WAVES, bool DIVK>
__global__ __launch_bounds__(QR_BLOCK, WAVES)
void qr_render_multi_kernel(DevTargets tg, const uint32_t *__restrict__ order16, int n_blocks,
                            unsigned long long *__restrict__ counters)
{
    const int gw = __builtin_amdgcn_readfirstlane((int)blockIdx.x * (QR_BLOCK / 64) + (int)(threadIdx.x >> 6));
    if (gw >= n_blocks) return;
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const u32x4 sched = ((const QR_CONST u32x4 *)order16)[gw];
#pragma clang diagnostic pop
    const DevTarget t = tg.t[sched.z & (QR_MAX_TARGETS - 1)];
    LaunchP lp;
    lp.B = t.B; lp.order = nullptr; lp.n_blocks = n_blocks; lp.depth = t.depth;
    lp.row_begin = t.row_begin; lp.row_end = t.row_end;
    lp.index = 0; lp.thnum = 1;
    lp.group_first = t.row_begin / 8; lp.group_stride = 1;
#ifdef QR_STATS
    lp.stats = counters + 4;            /* instrumented builds count into the first scene's counter block */
#else
    lp.stats = nullptr;
#endif
    lp.dbg = 0;
    render_wave<false, DIVK>(lp, sched.x, sched.y, gw, t.frame, nullptr, counters);
}

#endif /* QR_KERNEL_HPP */
