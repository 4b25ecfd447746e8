/*
 * ptaview_oracle.c - TEST INFRASTRUCTURE: the raw path-tracer samples of a view's pixel samples (include/qrhip.h
 * qr_pt_adapt_views_async) read out of the oracle.
 *
 * The truth of tests/test_pt_adaptive_views.py is rays.py pt_adapt_fold over what this file gives: for a snapshot rewritten to
 * ONE view and frame size (tests/test_render_views.py _view_snapshot) and a generator word per slot, the colour of each of
 * `samples` CONSECUTIVE samples of every slot, and the generator word after each.  There is no mean, no count and no rule in
 * here.  Like tests/ptadapt_oracle.c this translation unit includes the oracle's source (its functions are static); a sample is
 * the oracle's own sample() -- the tent-filter jitter with the FSAA halving, the frame's ray arithmetic, the walk, every draw
 * the oracle's pt_random, every bounce the oracle's shade() -- in the fast kernel's order (T.pt = 2, T.deferred = 1) with T.rng
 * preset from the caller's word.
 *
 * slot = (y * frm_w + x) * samples_per_pixel + k;  slots = frm_w * frm_h * samples_per_pixel.
 * rng_in: uint32 [slots].  depth < 0: the snapshot's.  cols: float [slots][samples][3].  rngs: uint32 [slots][samples].
 *
 * Built with the oracle's own flags (oracle/Makefile): -O2 -std=c99 -fPIC -shared -ffp-contract=off -fno-fast-math -fopenmp
 */
#include "../oracle/qr_oracle.c"

int qrv_pt_samples(const void *blob, uint64_t size, const uint32_t *rng_in, int64_t slots, int samples, int depth, int threads,
                   float *cols, uint32_t *rngs)
{
    scene_t S;
    int rc = qr_scene_view_init(&S.v, blob, size);
    int w, h, ns;
    int64_t i;
    if (rc != 0) return rc;
    w = S.v.frame->frm_w; h = S.v.frame->frm_h; ns = 1 << S.v.frame->fsaa;
    if (samples < 1 || slots != (int64_t)w * (int64_t)h * (int64_t)ns) return -1;
    S.depth = depth >= 0 ? depth : S.v.frame->depth;
    (void)threads;
#ifdef _OPENMP
    if (threads > 0) omp_set_num_threads(threads);
#endif
#pragma omp parallel for schedule(dynamic, 64)
    for (i = 0; i < slots; i++)
    {
        const int k = (int)(i % ns), x = (int)((i / ns) % w), y = (int)((i / ns) / w);
        tracer_t T;
        int s, ch;
        memset(&T, 0, sizeof(T));
        T.s = &S; T.depth = S.depth; T.top = S.depth; T.deferred = 1; T.pt = 2;
        T.rng = rng_in[i];
        for (s = 0; s < samples; s++)
        {
            const size_t o = (size_t)i * (size_t)samples + (size_t)s;
            float col[3];
            int id;
            sample(&T, x, y, k, col, &id);
            for (ch = 0; ch < 3; ch++) cols[3 * o + (size_t)ch] = col[ch];
            rngs[o] = T.rng;
        }
    }
    return 0;
}
