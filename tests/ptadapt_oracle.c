/*
 * ptadapt_oracle.c - TEST INFRASTRUCTURE: the raw path-tracer samples of caller rays (include/qrhip.h qr_pt_adapt_rays_async)
 * read out of the oracle.
 *
 * The truth of tests/test_pt_adaptive.py is rays.py pt_adapt_fold over what this file gives: for every ray the colour of each
 * of `samples` CONSECUTIVE samples from the ray's generator word, and the generator word after each.  There is no mean, no count
 * and no rule in here.  Like tests/ptrays_oracle.c this translation unit includes the oracle's source (its functions are
 * static), sets the context up from a caller's ray as tests/hitrec_oracle.c and qro_trace_rays do, and runs one sample of
 * qr_pt_rays_async (steps 1 to 3 of its header text) around trace_list: the optional spread jitter (the tent filter of
 * sample(), without the FSAA halving, on the ray's direction), then the walk.  Every draw is the oracle's pt_random, every
 * bounce the oracle's shade().
 *
 * rng_in: uint32 [n].  spread: NULL or float [n][8] = du xyz, pad, dv xyz, pad.  depth < 0: the snapshot's.
 * cols: float [n][samples][3].  rngs: uint32 [n][samples].
 *
 * Built with the oracle's own flags (oracle/Makefile): -O2 -std=c99 -fPIC -shared -ffp-contract=off -fno-fast-math -fopenmp
 */
#include "../oracle/qr_oracle.c"

int qrp_pt_samples(const void *blob, uint64_t size, const float *rays, const float *spread, int64_t n, const uint32_t *rng_in,
                   int samples, int depth, int threads, float *cols, uint32_t *rngs)
{
    scene_t S;
    int rc = qr_scene_view_init(&S.v, blob, size);
    int64_t i;
    if (rc != 0) return rc;
    if (n < 0 || samples < 1) return -1;
    S.depth = depth >= 0 ? depth : S.v.frame->depth;
    (void)threads;
#ifdef _OPENMP
    if (threads > 0) omp_set_num_threads(threads);
#endif
#pragma omp parallel for schedule(dynamic, 64)
    for (i = 0; i < n; i++)
    {
        const float *q = rays + 8 * i;
        tracer_t T;
        int s, ch;
        memset(&T, 0, sizeof(T));
        T.s = &S; T.depth = S.depth; T.top = S.depth; T.deferred = 1; T.pt = 2;
        T.rng = rng_in[i];
        for (s = 0; s < samples; s++)
        {
            ctx_t c;
            const size_t k = (size_t)i * (size_t)samples + (size_t)s;
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
            for (ch = 0; ch < 3; ch++) cols[3 * k + (size_t)ch] = c.col[ch];
            rngs[k] = T.rng;
        }
    }
    return 0;
}
