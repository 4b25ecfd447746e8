/*
 * hitrec_oracle.c - TEST INFRASTRUCTURE: hit records (include/qrhip.h qr_hit) read out of the oracle.
 *
 * oracle/qr_oracle.c in deferred mode shades the closest hit of a walk once, and after that its context holds the hit
 * point, the world normal and the texture colour the renderer lights with.  This translation unit includes the oracle's
 * source (its functions are static), runs the loop of qro_trace_rays mode 0 and writes those fields out.  No arithmetic
 * of its own.  The oracle computes a normal only for sides whose props carry QR_PROP_NORMAL, the kernel for every hit:
 * the snapshot is copied and the prop set on every side before the walk (the walk itself never reads it: t and ids stay
 * those of qro_trace_rays on the untouched snapshot, tests/test_hit_records.py checks that on every ray).
 *
 * Built with the oracle's own flags (oracle/Makefile): -O2 -std=c99 -fPIC -shared -ffp-contract=off -fno-fast-math -fopenmp
 */
#include "../oracle/qr_oracle.c"

typedef struct hitrec_t
{
    float pos[3]; float t;
    float nrm[3]; int32_t id;
    float alb[3]; int32_t mat;
} hitrec_t;                     /* qr_hit, 48 bytes */

int qrh_hit_rays(const void *blob, uint64_t size, const float *rays, int64_t n, int threads, hitrec_t *out)
{
    scene_t S;
    void *copy = malloc(size ? size : 1);
    int rc;
    int64_t i;
    uint32_t k;
    if (copy == NULL || n < 0) { free(copy); return -1; }
    memcpy(copy, blob, size);
    rc = qr_scene_view_init(&S.v, copy, size);
    if (rc != 0) { free(copy); return rc; }
    for (k = 0; k < S.v.hdr->n_srf; k++)
    {
        qr_surface *s = (qr_surface *)((char *)copy + S.v.hdr->off_srf) + k;
        s->props[0] |= QR_PROP_NORMAL; s->props[1] |= QR_PROP_NORMAL;
    }
    S.depth = 0;
    (void)threads;
#ifdef _OPENMP
    if (threads > 0) omp_set_num_threads(threads);
#endif
#pragma omp parallel for schedule(dynamic, 64)
    for (i = 0; i < n; i++)
    {
        const float *q = rays + 8 * i;
        hitrec_t *o = out + i;
        tracer_t T;
        ctx_t c;
        memset(&T, 0, sizeof(T));       /* path-tracer mode off (T.pt) */
        T.s = &S; T.depth = 0; T.deferred = 1;
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
        trace_list(&T, &c, NULL, S.v.frame->clist);
        memset(o, 0, sizeof(*o));       /* nine +0.0f */
        o->t = c.t_buf;
        o->id = c.hit_id;
        o->mat = -1;
        if (c.hit_id >= 0)
        {
            o->pos[0] = c.hit[0]; o->pos[1] = c.hit[1]; o->pos[2] = c.hit[2];
            o->nrm[0] = c.nrm[0]; o->nrm[1] = c.nrm[1]; o->nrm[2] = c.nrm[2];
            o->alb[0] = c.tex[0]; o->alb[1] = c.tex[1]; o->alb[2] = c.tex[2];
            o->mat = S.v.srf[c.hit_id >> 1].mat[c.hit_id & 1];
        }
    }
    free(copy);
    return 0;
}
