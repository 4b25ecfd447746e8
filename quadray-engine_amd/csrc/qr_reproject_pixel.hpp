/*
 * The pixel of temporal reprojection, written once: the statements of one lane, included into the body of each kernel of
 * qr_reproject.hpp (no include guard: this is program text, not declarations).  In scope where it is included: CH (3 or 4),
 * the constant MOVING, the parameters `p` (ReprojP) and, with MOVING, the table `motion` of `n_motion` >= 1 rows of three quads.
 *
 * Why text and not a `template <int CH, bool MOVING>` device function: the function, inlined, gives the static kernels another
 * register allocation (821 -> 820 instructions, 82 / 74 -> 78 / 78 VGPRs) although nothing of the move step is left in them;
 * included, their code is the same instruction for instruction as without the move step (tools/kernel_asm_diff.py).
 *
 * MOVING: the move step of qr_reproject_moving_async -- the record's surface s = id_p >> 1 names a row of the motion table, three
 * 16-byte loads asked for before the previous camera is read, and the projection and the tap tests see the moved point and
 * normal.  The bound test s < n_motion guards the address: a lane beyond the table loads row 0 (a table has at least one) and
 * ignores it; a miss loads nothing.  Neighbouring lanes mostly share a surface, so a wave's row loads fall into one or a few
 * cache lines.
 *
 * CLAMP: the clamp step of qr_reproject_clamped_async between the taps and the blend.  In scope with it: the block `cl`
 * (ReprojClampArgs) and the planes l_col, l_ok that qr_reproj_clamp_kernel staged and synchronised on BEFORE this text, so that the
 * early return below comes after the kernel's one barrier.  The kernels without the step name the three as constants that the
 * discarded statements never read.
 */
    const int tid = (int)threadIdx.x;
    const int W = p.width, H = p.height;
    const int x = (int)blockIdx.x * QR_REPROJ_TW + tid % QR_REPROJ_TW, y = (int)blockIdx.y * QR_REPROJ_TH + tid / QR_REPROJ_TW;
    if (x >= W || y >= H) return;                           /* past the frame's edge: nothing after this point synchronises (CLAMP: the staging and its barrier lie before this text) */
    const int view = __builtin_amdgcn_readfirstlane((int)blockIdx.z);
    const size_t view_px = (size_t)view * (size_t)W * (size_t)H;
    const size_t px = view_px + (size_t)y * (size_t)W + (size_t)x;

    /* read: the record, the colour (demodulated), its luminance, the fresh rule's variance */
    const f32x4 *h = p.hits + px * 3;
    f32x4 hp = h[0], hn = h[1];                             /* MOVING: pos and nrm become the moved ones below */
    const int32_t id_p = (int32_t)f2u(hn.w);
    float c[4];
#pragma unroll
    for (int k = 0; k < CH; k++) c[k] = p.colour_in[px * CH + k];
    if constexpr (CH == 3) c[3] = 0.0f;
    if ((p.flags & QR_REPROJ_DEMODULATE) && id_p >= 0) qr_albedo_divide(c, h[2], p.alb_floor);
    const float l = (c[0] * 0.2126f + c[1] * 0.7152f) + c[2] * 0.0722f;
    const float l2 = l * l;
    const float v_fresh = p.var_in != nullptr ? p.var_in[px] : p.unknown;

    const float qnan = u2f(0x7FC00000u);
    float m1 = l, m2 = l2, len = 1.0f, var = v_fresh, cx = qnan, cy = qnan;
    [[maybe_unused]] float moved = -1.0f;                   /* CLAMP: -1 where the entry is fresh, by any rule */

    if (p.views_prev != nullptr && id_p >= 0)
    {
        bool listed = true;
        if constexpr (MOVING)
        {
            /* move: where the point was and how its normal stood in the previous frame (not renormalised).  The row is asked
             * for first; the scalar loads of the camera below do not wait for it */
            const u32 s = (u32)id_p >> 1;
            listed = s < n_motion;
            const f32x4 *row = motion + (size_t)(listed ? s : 0u) * 3;
            const f32x4 r0 = row[0], r1 = row[1], r2 = row[2];
            const f32x4 cp = hp, cn = hn;
            hp.x = ((r0.x * cp.x + r0.y * cp.y) + r0.z * cp.z) + r0.w;
            hp.y = ((r1.x * cp.x + r1.y * cp.y) + r1.z * cp.z) + r1.w;
            hp.z = ((r2.x * cp.x + r2.y * cp.y) + r2.z * cp.z) + r2.w;
            hn.x = (r0.x * cn.x + r0.y * cn.y) + r0.z * cn.z;
            hn.y = (r1.x * cn.x + r1.y * cn.y) + r1.z * cn.z;
            hn.z = (r2.x * cn.x + r2.y * cn.y) + r2.z * cn.z;
        }
        /* project: wave-uniform up to det */
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
        const QR_CONST qr_view *vw = (const QR_CONST qr_view *)p.views_prev + view;
#pragma clang diagnostic pop
        const float ox = vw->org[0], oy = vw->org[1], oz = vw->org[2];
        const float dx = vw->dir[0], dy = vw->dir[1], dz = vw->dir[2];
        const float hx = vw->hor[0], hy = vw->hor[1], hz = vw->hor[2];
        const float vx = vw->ver[0], vy = vw->ver[1], vz = vw->ver[2];
        const float Ax = hy * vz - hz * vy, Ay = hz * vx - hx * vz, Az = hx * vy - hy * vx;
        const float Bx = vy * dz - vz * dy, By = vz * dx - vx * dz, Bz = vx * dy - vy * dx;
        const float Cx = dy * hz - dz * hy, Cy = dz * hx - dx * hz, Cz = dx * hy - dy * hx;
        const float det = (dx * Ax + dy * Ay) + dz * Az;
        const float ex = hp.x - ox, ey = hp.y - oy, ez = hp.z - oz;
        const float den = (ex * Ax + ey * Ay) + ez * Az;
        const float nu = (ex * Bx + ey * By) + ez * Bz;
        const float nv = (ex * Cx + ey * Cy) + ez * Cz;
        const float fx = nu / den - p.off_x, fy = nv / den - p.off_y;
        const bool front = listed && ((0.0f < den && 0.0f < det) || (den < 0.0f && det < 0.0f));
        if (front)
        {
            cx = fx; cy = fy;
            if (-1.0f < fx && fx < (float)W && -1.0f < fy && fy < (float)H)
            {
                const float x0 = floorf(fx), y0 = floorf(fy);
                const float wx = fx - x0, wy = fy - y0;
                const int ix = (int)x0, iy = (int)y0;       /* -1 .. W - 1, -1 .. H - 1 */
                /* The four taps in three rounds, so that a lane waits for memory twice and not twelve times: all four nrm / id
                 * quads are asked for before the first is looked at, then pos and history of the taps that passed, then the sums
                 * in tap order.  (One tap after the other -- quad, test, quad, test -- took 0.116 ms at 1080p, 3.2x a first
                 * frame's launch: every wave sat through a chain of dependent loads; profiles/r26_reproject.txt.) */
                size_t q[4];
                float b[4];
                bool open[4];
                f32x4 qn[4], qp[4], g0[4], g1[4];
#pragma unroll
                for (int t = 0; t < 4; t++)
                {
                    const int i = t & 1, j = t >> 1;
                    const int qx = ix + i, qy = iy + j;
                    b[t] = (i ? wx : 1.0f - wx) * (j ? wy : 1.0f - wy);
                    open[t] = qx >= 0 && qx < W && qy >= 0 && qy < H && 0.0f < b[t];
                    q[t] = open[t] ? view_px + (size_t)qy * (size_t)W + (size_t)qx : px;      /* closed: the pixel's own index, unused */
                }
#pragma unroll
                for (int t = 0; t < 4; t++) qn[t] = p.hits_prev[q[t] * 3 + 1];
#pragma unroll
                for (int t = 0; t < 4; t++)
                    open[t] = open[t] && (int32_t)f2u(qn[t].w) == id_p
                              && p.normal_min < (hn.x * qn[t].x + hn.y * qn[t].y) + hn.z * qn[t].z;
                /* no branch around these twelve loads: a tap that failed id or normal asks for the pixel's own index instead,
                 * lines its neighbours' taps bring in anyway, and what it gets is never looked at.  (With the loads under
                 * `if (open[t])` the compiler waited for each tap's quads before it issued the next tap's.) */
#pragma unroll
                for (int t = 0; t < 4; t++)
                {
                    const size_t qt = open[t] ? q[t] : px;
                    qp[t] = p.hits_prev[qt * 3];
                    g0[t] = p.hist_in[qt * 2]; g1[t] = p.hist_in[qt * 2 + 1];
                }
                float sw = 0.0f, sc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, s1 = 0.0f, s2 = 0.0f, sl = 0.0f;
#pragma unroll
                for (int t = 0; t < 4; t++)
                {
                    const float ddx = qp[t].x - hp.x, ddy = qp[t].y - hp.y, ddz = qp[t].z - hp.z;
                    if (open[t] && fabsf((hn.x * ddx + hn.y * ddy) + hn.z * ddz) <= p.plane_max && 1.0f <= g1[t].z)
                    {
                        sw = sw + b[t];
                        sc[0] = sc[0] + g0[t].x * b[t]; sc[1] = sc[1] + g0[t].y * b[t]; sc[2] = sc[2] + g0[t].z * b[t];
                        if constexpr (CH == 4) sc[3] = sc[3] + g0[t].w * b[t];
                        s1 = s1 + g1[t].x * b[t]; s2 = s2 + g1[t].y * b[t]; sl = sl + g1[t].z * b[t];
                    }
                }
                if (p.min_weight < sw)
                {
                    float h2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if constexpr (CLAMP)
                    {
                        /* clamp: the fetched colour held to the box of this frame's colours around the pixel, out of LDS */
                        float lo[CH], hi[CH];
                        qr_clamp_box<CH>(l_col, l_ok, tid, cl.radius, cl.flags, cl.gamma, lo, hi);
                        moved = 0.0f;
#pragma unroll
                        for (int k = 0; k < CH; k++)
                        {
                            const float hc = sc[k] / sw;
                            const float h1 = hc < lo[k] ? lo[k] : hc;
                            h2[k] = hi[k] < h1 ? hi[k] : h1;
                            const float d = fabsf(h2[k] - hc);
                            moved = d > moved ? d : moved;
                        }
                    }
                    len = sl / sw + 1.0f;
                    len = len < p.max_len ? len : p.max_len;
                    if constexpr (CLAMP)
                    {
                        if ((cl.flags & QR_CLAMP_SHORTEN) && 0.0f < moved) len = len < cl.short_len ? len : cl.short_len;
                    }
                    const float a = 1.0f / len;
                    const float ac = a > p.alpha_min ? a : p.alpha_min, am = a > p.alpha_mom_min ? a : p.alpha_mom_min;
#pragma unroll
                    for (int k = 0; k < CH; k++)
                    {
                        if constexpr (CLAMP) c[k] = h2[k] * (1.0f - ac) + c[k] * ac;
                        else c[k] = (sc[k] / sw) * (1.0f - ac) + c[k] * ac;
                    }
                    m1 = (s1 / sw) * (1.0f - am) + l * am;
                    m2 = (s2 / sw) * (1.0f - am) + l2 * am;
                    if (p.var_min_len <= len)
                    {
                        const float v = m2 - m1 * m1;
                        var = 0.0f < v ? v : 0.0f;
                    }
                }
            }
        }
    }

    f32x4 o0, o1;
    o0.x = c[0]; o0.y = c[1]; o0.z = c[2]; o0.w = c[3];
    o1.x = m1; o1.y = m2; o1.z = len; o1.w = 0.0f;
    p.hist_out[px * 2] = o0; p.hist_out[px * 2 + 1] = o1;
    if (p.colour_out != nullptr)
    {
#pragma unroll
        for (int k = 0; k < CH; k++) p.colour_out[px * CH + k] = c[k];
    }
    if (p.var_out != nullptr) p.var_out[px] = var;
    if (p.coords_out != nullptr) { p.coords_out[px * 2] = cx; p.coords_out[px * 2 + 1] = cy; }
    if constexpr (CLAMP)
    {
        if (cl.moved_out != nullptr) cl.moved_out[px] = moved;
    }
