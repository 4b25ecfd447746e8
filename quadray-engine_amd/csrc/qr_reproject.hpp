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
 * Both calls run one pixel, qr_reproject_pixel.hpp: the static kernels qr_reproject_kernel<CH> include it without the move step,
 * qr_reproj_moving_kernel<CH> with it.
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

template <int CH>
__global__ __launch_bounds__(QR_REPROJ_BLOCK)
void qr_reproject_kernel(const ReprojP p)
{
    constexpr bool MOVING = false;
    const f32x4 *const motion = nullptr;                    /* named in the step that MOVING = false discards */
    const u32 n_motion = 0u;
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
#include "qr_reproject_pixel.hpp"
}
