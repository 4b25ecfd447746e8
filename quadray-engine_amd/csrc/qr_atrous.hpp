/*
 * The guided a-trous filter (include/qrhip.h qr_atrous_views_async): one edge-avoiding 5x5 pass over view frames, the taps `step`
 * pixels apart, stopped by the qr_hit records of the pixels (normal, plane distance) and by the luminance against the
 * accumulator's variance.  The arithmetic is the header's, operation for operation; rays.py atrous_pass states it in numpy.
 *
 * Tiles are taken in the DECIMATED lattice.  The pixels of one phase (x mod step, y mod step) only ever read each other, so
 * they form a dense 5x5 problem of ceil(W / step) x ceil(H / step) entries: a workgroup takes QR_ATROUS_TW x QR_ATROUS_TH
 * entries of one phase, stages them with a halo of 2 entries per side -- whatever the step -- in LDS, and after one barrier
 * every lane reads its 25 taps from there.  Staged per entry, once: the colour as read (demodulated), its luminance, the
 * variance, nrm, pos and id; an entry outside the frame is staged with id = -1 and is then skipped like any miss.  The planes are
 * separate arrays (structure of arrays): a row of 32 lanes reads 32 consecutive dwords of one plane, which no bank sees twice.
 * 36 x 12 entries x 13 planes = 22 464 B with four channels: seven workgroups per CU.
 *
 * qr_pt_adapt_var_kernel (qr_pt_adapt_views_variance_async) is the per-pixel variance of an adaptive view state, one lane per
 * pixel.  Every store of this file is a vector store.
 */
#pragma once

#define QR_ATROUS_TW 32                 /* lattice entries per tile row: one half wave */
#define QR_ATROUS_TH 8
#define QR_ATROUS_LW (QR_ATROUS_TW + 4) /* with the halo */
#define QR_ATROUS_LH (QR_ATROUS_TH + 4)
#define QR_ATROUS_LN (QR_ATROUS_LW * QR_ATROUS_LH)
#define QR_ATROUS_BLOCK (QR_ATROUS_TW * QR_ATROUS_TH)

struct AtrousP
{
    const float *colour_in; const float *var_in; const f32x4 *hits;
    float *colour_out; float *var_out;
    int32_t width, height, step, normal_sq;
    int32_t tiles_x, tiles_y;           /* tiles per phase */
    u32 flags;
    float sigma_z, sigma_l2, eps_l, alb_floor;
};

/* max(alb, floor) as the header writes it: a NaN albedo gives the floor */
__device__ __forceinline__ float qr_atrous_alb(float alb, float floor) { return alb > floor ? alb : floor; }

/* the first three channels of c divided by the albedo ha of a record, each floored: this file, qr_upsample.hpp and
 * qr_reproject_pixel.hpp.  The multiply, the normal stop and the plane stop stay written out in the two kernels that have them:
 * as functions they moved qr_atrous_kernel's register allocation. */
__device__ __forceinline__ void qr_albedo_divide(float *c, const f32x4 ha, float floor)
{
    c[0] = c[0] / qr_atrous_alb(ha.x, floor);
    c[1] = c[1] / qr_atrous_alb(ha.y, floor);
    c[2] = c[2] / qr_atrous_alb(ha.z, floor);
}

template <int CH>
__global__ __launch_bounds__(QR_ATROUS_BLOCK)
void qr_atrous_kernel(const AtrousP p)
{
    __shared__ float l_col[CH][QR_ATROUS_LN];
    __shared__ float l_lum[QR_ATROUS_LN], l_var[QR_ATROUS_LN];
    __shared__ float l_nrm[3][QR_ATROUS_LN], l_pos[3][QR_ATROUS_LN];
    __shared__ int32_t l_id[QR_ATROUS_LN];

    const int tid = (int)threadIdx.x;
    const int W = p.width, H = p.height, s = p.step;
    const u32 flags = p.flags;
    const bool has_var = p.var_in != nullptr;
    /* the block's phase and its tile in that phase's lattice */
    const int phx = (int)blockIdx.x / p.tiles_x, i0 = ((int)blockIdx.x % p.tiles_x) * QR_ATROUS_TW;
    const int phy = (int)blockIdx.y / p.tiles_y, j0 = ((int)blockIdx.y % p.tiles_y) * QR_ATROUS_TH;
    const size_t view_px = (size_t)blockIdx.z * (size_t)W * (size_t)H;

    for (int e = tid; e < QR_ATROUS_LN; e += QR_ATROUS_BLOCK)
    {
        const int lx = e % QR_ATROUS_LW, ly = e / QR_ATROUS_LW;
        const int x = phx + (i0 + lx - 2) * s, y = phy + (j0 + ly - 2) * s;
        int32_t id = -1;
        if (x >= 0 && x < W && y >= 0 && y < H)
        {
            const size_t px = view_px + (size_t)y * (size_t)W + (size_t)x;
            const f32x4 *h = p.hits + px * 3;
            const f32x4 hn = h[1];
            id = (int32_t)f2u(hn.w);
            float c[CH];
#pragma unroll
            for (int k = 0; k < CH; k++) c[k] = p.colour_in[px * CH + k];
            if ((flags & QR_ATROUS_DEMODULATE) && id >= 0)
                qr_albedo_divide(c, h[2], p.alb_floor);
#pragma unroll
            for (int k = 0; k < CH; k++) l_col[k][e] = c[k];
            l_lum[e] = (c[0] * 0.2126f + c[1] * 0.7152f) + c[2] * 0.0722f;
            l_var[e] = has_var ? p.var_in[px] : 1.0f;
            l_nrm[0][e] = hn.x; l_nrm[1][e] = hn.y; l_nrm[2][e] = hn.z;
            if (flags & QR_ATROUS_PLANE)
            {
                const f32x4 hp = h[0];
                l_pos[0][e] = hp.x; l_pos[1][e] = hp.y; l_pos[2][e] = hp.z;
            }
        }
        l_id[e] = id;
    }
    __syncthreads();

    const int tx = tid % QR_ATROUS_TW, ty = tid / QR_ATROUS_TW;
    const int x = phx + (i0 + tx) * s, y = phy + (j0 + ty) * s;
    if (x >= W || y >= H) return;                           /* past the frame's edge: nothing after this point synchronises */
    const size_t px = view_px + (size_t)y * (size_t)W + (size_t)x;
    const int ec = (ty + 2) * QR_ATROUS_LW + (tx + 2);
    const int32_t id_p = l_id[ec];
    float out[CH], var_o = l_var[ec];
#pragma unroll
    for (int k = 0; k < CH; k++) out[k] = l_col[k][ec];
    if (id_p >= 0)
    {
        const float lum_p = l_lum[ec], v_p = var_o;
        const float npx = l_nrm[0][ec], npy = l_nrm[1][ec], npz = l_nrm[2][ec];
        float ppx = 0.0f, ppy = 0.0f, ppz = 0.0f;
        if (flags & QR_ATROUS_PLANE) { ppx = l_pos[0][ec]; ppy = l_pos[1][ec]; ppz = l_pos[2][ec]; }
        const float den = p.sigma_l2 * v_p + p.eps_l;
        float sum_c[CH], sum_w = 0.0f, sum_v = 0.0f;
#pragma unroll
        for (int k = 0; k < CH; k++) sum_c[k] = 0.0f;
        constexpr float Hk[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
#pragma unroll
        for (int dy = -2; dy <= 2; dy++)
        {
#pragma unroll
            for (int dx = -2; dx <= 2; dx++)
            {
                const int e = ec + dy * QR_ATROUS_LW + dx;
                float w = Hk[dy + 2] * Hk[dx + 2];
                bool take = true;
                if (dx != 0 || dy != 0)
                {
                    take = l_id[e] >= 0;
                    if (flags & QR_ATROUS_NORMAL)
                    {
                        float d = (npx * l_nrm[0][e] + npy * l_nrm[1][e]) + npz * l_nrm[2][e];
                        d = 0.0f < d ? d : 0.0f;
                        for (int k = 0; k < p.normal_sq; k++) d = d * d;
                        w = w * d;
                    }
                    if (flags & QR_ATROUS_PLANE)
                    {
                        const float ex = l_pos[0][e] - ppx, ey = l_pos[1][e] - ppy, ez = l_pos[2][e] - ppz;
                        const float d = (npx * ex + npy * ey) + npz * ez;
                        const float t = fabsf(d) / p.sigma_z;
                        w = w * (1.0f / (1.0f + t * t));
                    }
                    if (flags & QR_ATROUS_LUMA)
                    {
                        const float dl = lum_p - l_lum[e];
                        w = w * (1.0f / (1.0f + (dl * dl) / den));
                    }
                    take = take && 0.0f < w;
                }
                if (take)
                {
#pragma unroll
                    for (int k = 0; k < CH; k++) sum_c[k] = sum_c[k] + l_col[k][e] * w;
                    sum_w = sum_w + w;
                    sum_v = sum_v + l_var[e] * (w * w);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < CH; k++) out[k] = sum_c[k] / sum_w;
        var_o = sum_v / (sum_w * sum_w);
        if (flags & QR_ATROUS_MODULATE)
        {
            const f32x4 ha = p.hits[px * 3 + 2];
            out[0] = out[0] * qr_atrous_alb(ha.x, p.alb_floor);
            out[1] = out[1] * qr_atrous_alb(ha.y, p.alb_floor);
            out[2] = out[2] * qr_atrous_alb(ha.z, p.alb_floor);
        }
    }
#pragma unroll
    for (int k = 0; k < CH; k++) p.colour_out[px * CH + k] = out[k];
    if (has_var) p.var_out[px] = var_o;
}

/* per pixel, the channel-mean variance of the FSAA-reduced mean of an adaptive view state (include/qrhip.h
 * qr_pt_adapt_views_variance_async; rays.py pt_adapt_view_variance): one lane per pixel, blockIdx.y the view */
__global__ __launch_bounds__(256)
void qr_pt_adapt_var_kernel(const u32 *__restrict__ state, u32 pixels, int fsaa, float unknown, float *__restrict__ var)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= pixels) return;
    const int spp = 1 << fsaa;
    const size_t slots = (size_t)pixels << fsaa;
    const u32 *st = state + (size_t)blockIdx.y * QR_PT_ADAPT_STATE_WORDS * slots;
    float sum = 0.0f;
    for (int k = 0; k < spp; k++)
    {
        const size_t c = (i << fsaa) + (size_t)k;
        const u32 m = st[4 * slots + c];
        float v = unknown;
        if (2u <= m)
        {
            float sq = (u2f(st[5 * slots + c]) + u2f(st[6 * slots + c])) + u2f(st[7 * slots + c]);
            sq = 0.0f < sq ? sq : 0.0f;
            v = sq / (((float)m * (float)(m - 1u)) * 3.0f);
        }
        sum = k == 0 ? v : sum + v;
    }
    var[(size_t)blockIdx.y * pixels + i] = sum * (1.0f / (float)(spp * spp));
}
