/*
 * Guided upsampling (include/qrhip.h qr_upsample_views_async): light computed on a coarse lattice -- every factor-th pixel of
 * the frame from a phase on -- is brought to the full frame through the four lattice points around each pixel, each weighted by
 * its bilinear weight and by how well its guide, the FULL frame's qr_hit record at the lattice point, agrees with the pixel's own
 * record.  The arithmetic is the header's, operation for operation; rays.py upsample_pass states it in numpy.
 *
 * One lane per full pixel, workgroups of QR_UPS_TW x QR_UPS_TH pixels, blockIdx.z the view.  The lattice entries a tile can touch
 * are columns floor((x0 - px) / s) .. floor((x0 + 31 - px) / s) + 1 and the rows likewise: at most (ceil(32 / s) + 2) x
 * (ceil(8 / s) + 2), 34 x 10 at s = 1.  They are staged ONCE in LDS as separate planes -- the colour as read (demodulated at
 * staging), the variance, the guide's nrm, pos and id --, so that the stride-s reads of 48-byte records happen once per entry and
 * not once per tap of every lane; an entry outside the coarse frame is staged as a miss with zeros and never looked at (a lane
 * tells inside from outside by the entry's coordinates).  After one barrier a lane reads its four taps from there.  A half wave
 * is one row of 32 pixels: its lanes read entries (x - px) / s of one plane row, runs of equal addresses (broadcast) over at
 * most 17 consecutive dwords at s >= 2 and 32 consecutive dwords at s = 1: no bank is asked for two addresses.
 * (8 + CH) planes x 340 entries x 4 B = 14 960 B (three channels) / 16 320 B (four).  Every store of this file is a vector store.
 */
#pragma once

#define QR_UPS_TW 32                    /* full pixels per tile row: one half wave */
#define QR_UPS_TH 8
#define QR_UPS_BLOCK (QR_UPS_TW * QR_UPS_TH)
#define QR_UPS_LW (QR_UPS_TW + 2)       /* lattice entries a tile can touch at factor 1 */
#define QR_UPS_LH (QR_UPS_TH + 2)
#define QR_UPS_LN (QR_UPS_LW * QR_UPS_LH)

struct UpsampleP
{
    const float *colour_lo; const float *var_lo; const f32x4 *hits;
    float *colour_out; float *var_out; float *weight_out;
    int32_t width, height, wl, hl;      /* the full and the coarse frame */
    int32_t factor, phase_x, phase_y, normal_sq;
    u32 flags;
    float sigma_z, alb_floor;
};

template <int CH>
__global__ __launch_bounds__(QR_UPS_BLOCK)
void qr_upsample_kernel(const UpsampleP p)
{
    __shared__ float l_col[CH][QR_UPS_LN];
    __shared__ float l_var[QR_UPS_LN];
    __shared__ float l_nrm[3][QR_UPS_LN], l_pos[3][QR_UPS_LN];
    __shared__ int32_t l_id[QR_UPS_LN];

    const int tid = (int)threadIdx.x;
    const int W = p.width, H = p.height, Wl = p.wl, Hl = p.hl, s = p.factor, phx = p.phase_x, phy = p.phase_y;
    const u32 flags = p.flags;
    const bool has_var = p.var_lo != nullptr;
    const int view = __builtin_amdgcn_readfirstlane((int)blockIdx.z);
    const size_t view_px = (size_t)view * (size_t)W * (size_t)H;
    const size_t view_lo = (size_t)view * (size_t)Wl * (size_t)Hl;
    /* floor((a - phase) / s) for a >= 0: phase < s, so a - phase + s is not negative */
    const int tx0 = (int)blockIdx.x * QR_UPS_TW, ty0 = (int)blockIdx.y * QR_UPS_TH;
    const int cx0 = (int)((unsigned)(tx0 - phx + s) / (unsigned)s) - 1, cy0 = (int)((unsigned)(ty0 - phy + s) / (unsigned)s) - 1;
    const int lw = (int)((unsigned)(tx0 + QR_UPS_TW - 1 - phx + s) / (unsigned)s) - cx0 + 1;        /* entries in use: <= QR_UPS_LW */
    const int lh = (int)((unsigned)(ty0 + QR_UPS_TH - 1 - phy + s) / (unsigned)s) - cy0 + 1;        /* <= QR_UPS_LH */

    for (int e = tid; e < QR_UPS_LN; e += QR_UPS_BLOCK)
    {
        const int lx = e % QR_UPS_LW, ly = e / QR_UPS_LW;
        if (lx >= lw || ly >= lh) continue;
        const int qx = cx0 + lx, qy = cy0 + ly;
        int32_t id = -1;
        float c[CH], var = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f, gx = 0.0f, gy = 0.0f, gz = 0.0f;
#pragma unroll
        for (int k = 0; k < CH; k++) c[k] = 0.0f;
        if (qx >= 0 && qx < Wl && qy >= 0 && qy < Hl)
        {
            /* the guide: the full record at the lattice point, inside the frame by the coarse frame's size */
            const size_t gp = view_px + (size_t)(s * qy + phy) * (size_t)W + (size_t)(s * qx + phx);
            const size_t lo = view_lo + (size_t)qy * (size_t)Wl + (size_t)qx;
            const f32x4 *h = p.hits + gp * 3;
            const f32x4 hn = h[1];
            id = (int32_t)f2u(hn.w);
            nx = hn.x; ny = hn.y; nz = hn.z;
#pragma unroll
            for (int k = 0; k < CH; k++) c[k] = p.colour_lo[lo * CH + k];
            if ((flags & QR_UPSAMPLE_DEMODULATE) && id >= 0)
                qr_albedo_divide(c, h[2], p.alb_floor);
            if (has_var) var = p.var_lo[lo];
            if (flags & QR_UPSAMPLE_PLANE)
            {
                const f32x4 hp = h[0];
                gx = hp.x; gy = hp.y; gz = hp.z;
            }
        }
#pragma unroll
        for (int k = 0; k < CH; k++) l_col[k][e] = c[k];
        l_var[e] = var;
        l_nrm[0][e] = nx; l_nrm[1][e] = ny; l_nrm[2][e] = nz;
        l_pos[0][e] = gx; l_pos[1][e] = gy; l_pos[2][e] = gz;
        l_id[e] = id;
    }
    __syncthreads();

    const int x = tx0 + tid % QR_UPS_TW, y = ty0 + tid / QR_UPS_TW;
    if (x >= W || y >= H) return;                           /* past the frame's edge: nothing after this point synchronises */
    const size_t px = view_px + (size_t)y * (size_t)W + (size_t)x;

    /* position: X0 is -1 left of the first coarse column */
    const int X0 = (int)((unsigned)(x - phx + s) / (unsigned)s) - 1, Y0 = (int)((unsigned)(y - phy + s) / (unsigned)s) - 1;
    const int rx = (x - phx) - X0 * s, ry = (y - phy) - Y0 * s;
    const float wx = (float)rx / (float)s, wy = (float)ry / (float)s;
    const int e00 = (Y0 - cy0) * QR_UPS_LW + (X0 - cx0);

    const f32x4 *h = p.hits + px * 3;
    const f32x4 hn = h[1];
    const int32_t id_p = (int32_t)f2u(hn.w);
    f32x4 hp;
    hp.x = 0.0f; hp.y = 0.0f; hp.z = 0.0f; hp.w = 0.0f;
    if ((flags & QR_UPSAMPLE_PLANE) && id_p >= 0) hp = h[0];

    /* the four taps: entry, bilinear weight, guide weight; a tap that is not eligible has g = 0 and is never taken */
    int et[4];
    float b[4], g[4];
#pragma unroll
    for (int t = 0; t < 4; t++)
    {
        const int i = t & 1, j = t >> 1;
        const int qx = X0 + i, qy = Y0 + j;
        const int e = e00 + j * QR_UPS_LW + i;
        et[t] = e;
        b[t] = (i ? wx : 1.0f - wx) * (j ? wy : 1.0f - wy);
        const bool inside = qx >= 0 && qx < Wl && qy >= 0 && qy < Hl;
        const int32_t id_g = l_id[e];
        float gw = 0.0f;
        if (id_p < 0)
        {
            if (inside && id_g < 0) gw = 1.0f;
        }
        else if (inside && id_g >= 0 && (!(flags & QR_UPSAMPLE_SAME_ID) || id_g == id_p))
        {
            gw = 1.0f;
            if (flags & QR_UPSAMPLE_NORMAL)
            {
                float d = (hn.x * l_nrm[0][e] + hn.y * l_nrm[1][e]) + hn.z * l_nrm[2][e];
                d = 0.0f < d ? d : 0.0f;
                for (int k = 0; k < p.normal_sq; k++) d = d * d;
                gw = gw * d;
            }
            if (flags & QR_UPSAMPLE_PLANE)
            {
                const float ex = l_pos[0][e] - hp.x, ey = l_pos[1][e] - hp.y, ez = l_pos[2][e] - hp.z;
                const float d = (hn.x * ex + hn.y * ey) + hn.z * ez;
                const float tt = fabsf(d) / p.sigma_z;
                gw = gw * (1.0f / (1.0f + tt * tt));
            }
            gw = 0.0f < gw ? gw : 0.0f;                     /* a NaN closes the tap */
        }
        g[t] = gw;
    }

    float out[CH], var_o = 0.0f, weight = 0.0f;
    float sc[CH], sw = 0.0f, sv = 0.0f;
#pragma unroll
    for (int k = 0; k < CH; k++) sc[k] = 0.0f;
    /* stage 1: w = b * g */
#pragma unroll
    for (int t = 0; t < 4; t++)
    {
        const float w = b[t] * g[t];
        if (0.0f < w)
        {
#pragma unroll
            for (int k = 0; k < CH; k++) sc[k] = sc[k] + l_col[k][et[t]] * w;
            sw = sw + w;
            sv = sv + l_var[et[t]] * (w * w);
        }
    }
    weight = sw;
    if (!(0.0f < sw))
    {
        /* stage 2: the open taps all have bilinear weight 0: w = g */
#pragma unroll
        for (int t = 0; t < 4; t++)
        {
            const float w = g[t];
            if (0.0f < w)
            {
#pragma unroll
                for (int k = 0; k < CH; k++) sc[k] = sc[k] + l_col[k][et[t]] * w;
                sw = sw + w;
                sv = sv + l_var[et[t]] * (w * w);
            }
        }
        weight = 0.0f;
    }
    if (0.0f < sw)
    {
#pragma unroll
        for (int k = 0; k < CH; k++) out[k] = sc[k] / sw;
        var_o = sv / (sw * sw);
    }
    else
    {
        /* stage 3: the nearest coarse pixel, clamped into the coarse frame: one of the four entries */
        int qx = X0 + (2 * rx >= s ? 1 : 0), qy = Y0 + (2 * ry >= s ? 1 : 0);
        qx = qx < 0 ? 0 : (qx > Wl - 1 ? Wl - 1 : qx);
        qy = qy < 0 ? 0 : (qy > Hl - 1 ? Hl - 1 : qy);
        const int e = (qy - cy0) * QR_UPS_LW + (qx - cx0);
#pragma unroll
        for (int k = 0; k < CH; k++) out[k] = l_col[k][e];
        var_o = l_var[e];
        weight = -1.0f;
    }
    if ((flags & QR_UPSAMPLE_MODULATE) && id_p >= 0)
    {
        const f32x4 ha = h[2];
        out[0] = out[0] * qr_atrous_alb(ha.x, p.alb_floor);
        out[1] = out[1] * qr_atrous_alb(ha.y, p.alb_floor);
        out[2] = out[2] * qr_atrous_alb(ha.z, p.alb_floor);
    }
    if constexpr (CH == 4)
    {
        /* one 16-byte store where the caller's pointer allows it (uniform) */
        if (((uintptr_t)p.colour_out & 15u) == 0u)
        {
            f32x4 o;
            o.x = out[0]; o.y = out[1]; o.z = out[2]; o.w = out[3];
            *reinterpret_cast<f32x4 *>(p.colour_out + px * 4) = o;
        }
        else
        {
#pragma unroll
            for (int k = 0; k < 4; k++) p.colour_out[px * 4 + k] = out[k];
        }
    }
    else
    {
#pragma unroll
        for (int k = 0; k < CH; k++) p.colour_out[px * CH + k] = out[k];
    }
    if (has_var) p.var_out[px] = var_o;
    if (p.weight_out != nullptr) p.weight_out[px] = weight;
}
