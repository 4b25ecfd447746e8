/*
 * ptrays_oracle.c - TEST INFRASTRUCTURE: path-traced caller rays (include/qrhip.h qr_pt_rays_async) read out of the oracle.
 *
 * oracle/qr_oracle.c has the path tracer in the kernel's order of draws (tracer_t.pt = 2, deferred) behind its own camera
 * (sample() / pixel()).  This translation unit includes the oracle's source (its functions are static), sets the context up
 * from a caller's ray exactly as tests/hitrec_oracle.c and qro_trace_rays do, and runs the contract of qr_pt_rays_async
 * around trace_list: the generator state from the caller's state, the optional spread jitter (the tent filter of sample(),
 * without the FSAA halving, on the ray's direction), the walk, the running mean, the state back.  Every draw is the
 * oracle's pt_random, every bounce the oracle's shade().
 *
 * state: uint32 [4][n] -- plane 0 the LCG states, planes 1..3 the float32 running means of r, g, b; ray i is column i.
 * spread: NULL or float [n][8] = du xyz, pad, dv xyz, pad.  done: samples the state holds; samples: how many to add.
 * depth < 0: the snapshot's.  rgb (optional) float [n][3]: the running means after the call.  stats (optional) uint64 [6]:
 * the oracle's path-tracer counters (qr_oracle.py PT_STATS) summed over all rays and samples.
 *
 * Built with the oracle's own flags (oracle/Makefile): -O2 -std=c99 -fPIC -shared -ffp-contract=off -fno-fast-math -fopenmp
 */
#include "../oracle/qr_oracle.c"

int qrp_pt_rays(const void *blob, uint64_t size, const float *rays, const float *spread, int64_t n, uint32_t *state,
                int done, int samples, int depth, int threads, float *rgb, uint64_t *stats)
{
    scene_t S;
    int rc = qr_scene_view_init(&S.v, blob, size);
    int64_t i;
    uint64_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0;
    if (rc != 0) return rc;
    if (n < 0 || done < 0 || samples < 1) return -1;
    S.depth = depth >= 0 ? depth : S.v.frame->depth;
    (void)threads;
#ifdef _OPENMP
    if (threads > 0) omp_set_num_threads(threads);
#endif
#pragma omp parallel for schedule(dynamic, 64) reduction(+:s0,s1,s2,s3,s4,s5)
    for (i = 0; i < n; i++)
    {
        const float *q = rays + 8 * i;
        tracer_t T;
        float mean[3];
        int s, ch;
        memset(&T, 0, sizeof(T));
        T.s = &S; T.depth = S.depth; T.top = S.depth; T.deferred = 1; T.pt = 2;
        T.rng = state[i];
        for (ch = 0; ch < 3; ch++) mean[ch] = u2f(state[(size_t)(ch + 1) * (size_t)n + (size_t)i]);
        for (s = 0; s < samples; s++)
        {
            ctx_t c;
            const float o = 1.0f / (float)(done + s + 1), u = 1.0f - o;
            memset(&c, 0, sizeof(c));
            c.t_buf = q[7] > FLT_MAX ? FLT_MAX : q[7];
            c.t_min = q[3];
            c.org[0] = q[0]; c.org[1] = q[1]; c.org[2] = q[2];
            c.ray[0] = q[4]; c.ray[1] = q[5]; c.ray[2] = q[6];
            c.wmask = 0xFFFFFFFFu;
            c.param_tag = 0;
            c.param_flg = S.v.frame->ctx_flags;
            c.param_obj = QR_NULL;
            c.local_obj = QR_NULL;
            c.pend_si = QR_NULL;
            c.hit_id = -1;
            if (spread != NULL)
            {
                /* the tent filter of sample(), two numbers, horizontal first; no FSAA halving: caller rays have none */
                const float *sp = spread + 8 * i;
                float hv[2];
                int j;
                for (j = 0; j < 2; j++)
                {
                    float w = pt_random(&T, j == 0 ? PT_DRAW_JITTER_H : PT_DRAW_JITTER_V), a, b;
                    w = w + w;
                    a = sqrtf(w); a = a - 1.0f;
                    b = 2.0f - w; b = sqrtf(b); b = 1.0f - b;
                    a = fsel(clt(w, 1.0f), a, b);
                    a = a * 0.5f;
                    hv[j] = a;
                }
                for (ch = 0; ch < 3; ch++)
                {
                    float a = sp[ch] * hv[0], b = sp[4 + ch] * hv[1];
                    a = a + b;
                    c.ray[ch] = c.ray[ch] + a;
                }
            }
            trace_list(&T, &c, NULL, S.v.frame->clist);
            for (ch = 0; ch < 3; ch++)
            {
                float a = c.col[ch] * o, b = mean[ch] * u;
                mean[ch] = a + b;
            }
        }
        state[i] = T.rng;
        for (ch = 0; ch < 3; ch++) state[(size_t)(ch + 1) * (size_t)n + (size_t)i] = f2u(mean[ch]);
        if (rgb != NULL) { rgb[3 * i + 0] = mean[0]; rgb[3 * i + 1] = mean[1]; rgb[3 * i + 2] = mean[2]; }
        s0 += T.st[0]; s1 += T.st[1]; s2 += T.st[2]; s3 += T.st[3]; s4 += T.st[4]; s5 += T.st[5];
    }
    if (stats != NULL) { stats[0] = s0; stats[1] = s1; stats[2] = s2; stats[3] = s3; stats[4] = s4; stats[5] = s5; }
    return 0;
}
