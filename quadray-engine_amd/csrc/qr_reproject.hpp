/*
 * Temporal reprojection (include/qrhip.h qr_reproject_views_async, qr_reproject_moving_async): every pixel of this frame's hit
 * records is projected into the previous frame's camera, the previous history is fetched there through four bilinear taps held to the same surface by the
 * previous records, and this frame's colour is blended in.  The arithmetic is the header's, operation for operation; rays.py
 * reproject_pass states it in numpy.
 *
 * One lane per pixel, workgroups of QR_REPROJ_TW x QR_REPROJ_TH pixels, blockIdx.z the view: a wave is two rows of 32 pixels,
 * and under a camera that moved a little its taps land in a compact patch of the previous frame and share cache lines.  The
 * previous view record is wave-uniform and read through the constant address space (scalar loads), and so are A, B, C and det
 * derived from it.  The taps go in rounds: the nrm / id quads of all four first, then pos and the two history quads of all four at
 * once -- of the tap itself only where id and normal pass --, then the sums in tap order.  No LDS: where a tap lands depends on
 * the data.  History and hit records move as 16-byte quads; every store of this file is a vector store.
 *
 * All calls run one pixel, qr_reproject_pixel.hpp: the static kernels qr_reproject_kernel<CH> include it without the move step,
 * qr_reproj_moving_kernel<CH> with it, qr_reproj_clamp_kernel<CH, MOVING> with the clamp step (and the move step or not).
 *
 * The clamp kernels (qr_reproject_clamped_async) are the only ones with LDS: a pixel's box is made of this frame's colours in a
 * (2r + 1) x (2r + 1) neighbourhood, r <= QR_CLAMP_MAX_RADIUS, which -- unlike the taps -- is known before the data.  The
 * (32 + 2R) x (8 + 2R) neighbourhood of the tile is staged ONCE as separate planes, as qr_upsample.hpp does it: the colour as read
 * (demodulated at staging by the entry's own albedo) and validity (inside this view's frame and id >= 0, from the record's id
 * quad); an entry outside the frame is invalid and loads nothing, so a halo never takes the next row's or the next view's pixels
 * of the flat frame for neighbours, and entries further than r from the tile are not staged at all.  Every lane stages and
 * reaches the one barrier, the lanes past the frame's edge included: the pixel's early return comes after it.  Then the box, a
 * direct evaluation in the header's order (a row's partials i = -r..r, then the rows folded j = -r..r), then the pixel.
 * Banking: a plane row is 38 consecutive dwords; a half wave is one row of 32 pixels and reads, for one (i, j), the 32 consecutive
 * dwords (ty + R + j) * 38 + R + i + 0..31 of one plane.  ds_read_b32 takes the two 32-lane halves in turn and banks by dword
 * address mod 32: 32 consecutive dwords are 32 different banks, whatever the row's start, so the layout is conflict-free without
 * padding (the staging writes, 256 consecutive entries of a plane, likewise).  (CH + 1) planes x 38 x 14 entries x 4 B =
 * 8 512 B (three channels) / 10 640 B (four).  A separable form (a row pass into planes of its own, then a column pass) gives the
 * same bits by the header's order; it is not built.
 */
#pragma once

#define QR_REPROJ_TW 32
#define QR_REPROJ_TH 8
#define QR_REPROJ_BLOCK (QR_REPROJ_TW * QR_REPROJ_TH)

struct ReprojP
{
    const float *colour_in; const f32x4 *hits; const float *var_in;
    const qr_view *views_prev; const f32x4 *hits_prev; const f32x4 *hist_in;   /* all three or none */
    f32x4 *hist_out; float *colour_out; float *var_out; float *coords_out;
    int32_t width, height;
    u32 flags;
    float off_x, off_y, normal_min, plane_max, min_weight, alpha_min, alpha_mom_min, max_len, var_min_len, unknown, alb_floor;
};

/* the clamp block of qr_reproject_clamped_async as the kernels take it */
struct ReprojClampArgs
{
    float *moved_out;                                       /* or null */
    u32 flags;                                              /* QR_CLAMP_*: checked by the host */
    int32_t radius;                                         /* 1..QR_CLAMP_MAX_RADIUS */
    float gamma, short_len;
};

#define QR_CLAMP_LW (QR_REPROJ_TW + 2 * QR_CLAMP_MAX_RADIUS)            /* the tile and its widest halo */
#define QR_CLAMP_LH (QR_REPROJ_TH + 2 * QR_CLAMP_MAX_RADIUS)
#define QR_CLAMP_LN (QR_CLAMP_LW * QR_CLAMP_LH)

/* what the kernels without the clamp step name in the statements that CLAMP = false discards */
#define QR_REPROJ_NO_CLAMP \
    constexpr bool CLAMP = false; \
    const ReprojClampArgs cl = {nullptr, 0u, 0, 0.0f, 0.0f}; \
    const float (*const l_col)[QR_CLAMP_LN] = nullptr; \
    const int32_t *const l_ok = nullptr;

/* The box of lane tid's pixel from the staged planes, the header's clamp step operation for operation: per channel lo and hi from
 * the valid entries within r of the pixel, a row's partials first (i ascending), then the rows' partials folded (j ascending).
 * An invalid entry adds nothing: the sums start at +0.0 and cannot become -0.0, so skipping it and adding +0.0 are the same bits. */
template <int CH>
__device__ __forceinline__ void qr_clamp_box(const float (*l_col)[QR_CLAMP_LN], const int32_t *l_ok, int tid, int r, u32 flags,
                                             float gamma, float *lo, float *hi)
{
    const int e0 = (tid / QR_REPROJ_TW + QR_CLAMP_MAX_RADIUS) * QR_CLAMP_LW + (tid % QR_REPROJ_TW + QR_CLAMP_MAX_RADIUS);
    if (flags & QR_CLAMP_VARIANCE)
    {
        int n = 0;
        float t1[CH], t2[CH];
#pragma unroll
        for (int k = 0; k < CH; k++) { t1[k] = 0.0f; t2[k] = 0.0f; }
        for (int j = -r; j <= r; j++)
        {
            int rn = 0;
            float r1[CH], r2[CH];
#pragma unroll
            for (int k = 0; k < CH; k++) { r1[k] = 0.0f; r2[k] = 0.0f; }
            for (int i = -r; i <= r; i++)
            {
                const int e = e0 + j * QR_CLAMP_LW + i;
                const bool ok = l_ok[e] != 0;
                rn += ok ? 1 : 0;
#pragma unroll
                for (int k = 0; k < CH; k++)
                {
                    const float v = l_col[k][e];
                    r1[k] = ok ? r1[k] + v : r1[k];
                    r2[k] = ok ? r2[k] + v * v : r2[k];
                }
            }
            n += rn;
#pragma unroll
            for (int k = 0; k < CH; k++) { t1[k] = t1[k] + r1[k]; t2[k] = t2[k] + r2[k]; }
        }
        const float nf = (float)n;                          /* n >= 1: the pixel itself keeps history, so it is a hit */
#pragma unroll
        for (int k = 0; k < CH; k++)
        {
            const float mu = t1[k] / nf;
            float v = t2[k] / nf - mu * mu;
            v = 0.0f < v ? v : 0.0f;
            const float w = gamma * __builtin_sqrtf(v);
            lo[k] = mu - w; hi[k] = mu + w;
        }
    }
    else
    {
        const float inf = u2f(0x7F800000u);
#pragma unroll
        for (int k = 0; k < CH; k++) { lo[k] = inf; hi[k] = -inf; }
        for (int j = -r; j <= r; j++)
        {
            float rl[CH], rh[CH];
#pragma unroll
            for (int k = 0; k < CH; k++) { rl[k] = inf; rh[k] = -inf; }
            for (int i = -r; i <= r; i++)
            {
                const int e = e0 + j * QR_CLAMP_LW + i;
                const bool ok = l_ok[e] != 0;
#pragma unroll
                for (int k = 0; k < CH; k++)
                {
                    const float v = l_col[k][e];
                    rl[k] = ok && v < rl[k] ? v : rl[k];
                    rh[k] = ok && rh[k] < v ? v : rh[k];
                }
            }
#pragma unroll
            for (int k = 0; k < CH; k++)
            {
                lo[k] = rl[k] < lo[k] ? rl[k] : lo[k];
                hi[k] = hi[k] < rh[k] ? rh[k] : hi[k];
            }
        }
    }
}

template <int CH>
__global__ __launch_bounds__(QR_REPROJ_BLOCK)
void qr_reproject_kernel(const ReprojP p)
{
    constexpr bool MOVING = false;
    const f32x4 *const motion = nullptr;                    /* named in the step that MOVING = false discards */
    const u32 n_motion = 0u;
    QR_REPROJ_NO_CLAMP
#include "qr_reproject_pixel.hpp"
}

/* qr_reproject_moving_async with a table: the same pixel with the move step */
struct ReprojMovingP
{
    ReprojP r;
    const f32x4 *motion;                                    /* n_motion rows of three quads */
    u32 n_motion;                                           /* >= 1 */
};

template <int CH>
__global__ __launch_bounds__(QR_REPROJ_BLOCK)
void qr_reproj_moving_kernel(const ReprojMovingP mp)
{
    constexpr bool MOVING = true;
    const ReprojP &p = mp.r;
    const f32x4 *const motion = mp.motion;
    const u32 n_motion = mp.n_motion;
    QR_REPROJ_NO_CLAMP
#include "qr_reproject_pixel.hpp"
}

/* qr_reproject_clamped_async with a block: the same pixel with the clamp step, with a table (MOVING) or without */
struct ReprojClampP
{
    ReprojMovingP m;                                        /* without a table: motion null, n_motion 0, never read */
    ReprojClampArgs cl;
};

template <int CH, bool MOVING>
__global__ __launch_bounds__(QR_REPROJ_BLOCK)
void qr_reproj_clamp_kernel(const ReprojClampP cp)
{
    __shared__ float l_col[CH][QR_CLAMP_LN];
    __shared__ int32_t l_ok[QR_CLAMP_LN];

    constexpr bool CLAMP = true;
    const ReprojP &p = cp.m.r;
    const f32x4 *const motion = cp.m.motion;
    const u32 n_motion = cp.m.n_motion;
    const ReprojClampArgs &cl = cp.cl;
    {
        /* stage: every lane, the ones past the frame's edge included */
        constexpr int R = QR_CLAMP_MAX_RADIUS;
        const int r = cl.radius;
        const int tx0 = (int)blockIdx.x * QR_REPROJ_TW, ty0 = (int)blockIdx.y * QR_REPROJ_TH;
        const size_t view_px0 = (size_t)__builtin_amdgcn_readfirstlane((int)blockIdx.z) * (size_t)p.width * (size_t)p.height;
        for (int e = (int)threadIdx.x; e < QR_CLAMP_LN; e += QR_REPROJ_BLOCK)
        {
            const int lx = e % QR_CLAMP_LW, ly = e / QR_CLAMP_LW;
            if (lx < R - r || lx >= QR_REPROJ_TW + R + r || ly < R - r || ly >= QR_REPROJ_TH + R + r) continue;     /* never read */
            const int qx = tx0 - R + lx, qy = ty0 - R + ly;
            int32_t ok = 0;
            float c[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (qx >= 0 && qx < p.width && qy >= 0 && qy < p.height)
            {
                const size_t q = view_px0 + (size_t)qy * (size_t)p.width + (size_t)qx;
                const f32x4 *h = p.hits + q * 3;
                if ((int32_t)f2u(h[1].w) >= 0)
                {
                    ok = 1;
#pragma unroll
                    for (int k = 0; k < CH; k++) c[k] = p.colour_in[q * CH + k];
                    if (p.flags & QR_REPROJ_DEMODULATE) qr_albedo_divide(c, h[2], p.alb_floor);
                }
            }
#pragma unroll
            for (int k = 0; k < CH; k++) l_col[k][e] = c[k];
            l_ok[e] = ok;
        }
    }
    __syncthreads();
#include "qr_reproject_pixel.hpp"
}
