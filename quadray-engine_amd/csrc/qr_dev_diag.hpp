/*
 * qr_dev_diag.hpp - read-outs of the diagnostic builds: the QR_PROF and QR_STATS counters behind qr_render_count, the
 * QR_WAVETIME stamps behind qr_render_timed.  In the product build every function here does nothing.  Host code; included by
 * qr_device.hip.
 */
static int diag_print_counters(qr_device_scene *s)
{
    static const char *const kind[3] = { "shadow", "primary", "secondary" };
    (void)s; (void)kind;
#ifdef QR_PROF
    unsigned long long pf[80];
    HIP_TRY(hipMemcpyFromSymbol(pf, HIP_SYMBOL(qr_prof), sizeof(pf)));
    static const char *nm[48] = { "candidates through clip()", "clipper programs run", "clipper cells", "  fast plane cells", "  trnode / trsame cells",
        "  generic plane tests", "  quadric tests", "", "solve: plane cells", "solve: quadric cells", "solve: two-plane cells", "solve in shadow walks", "solve in nearest-hit walks",
        "solve with own / cached transform", "solve with conic fix", "", "cells loaded by packet walks", "  culled by their sphere", "shadow packet walks", "nearest-hit packet walks",
        "trnode cells", "bounding-volume cells", "", "", "shade() calls", "light rounds", "solves without any accepted hit", "  of them planes", "  of them without a candidate root", "box cull tests" };
    for (int i = 0; i < 30; i++) if (nm[i][0]) fprintf(stderr, "QR_PROF %-36s %llu\n", nm[i], pf[i]);
    fprintf(stderr, "QR_PROF algorithmic fp32 operations executed (SURVEY 8(d) weights, per lane) %llu\n", pf[48]);
    fprintf(stderr, "QR_PROF fp32 operations of the implementation's own culls (sphere / box tests, walk set-up) %llu\n", pf[49]);
    fprintf(stderr, "QR_PROF frames pushed by level 0..7+ (lanes), both children:");
    for (int i = 0; i < 8; i++) fprintf(stderr, " %llu", pf[32 + i]);
    fprintf(stderr, "\nQR_PROF frames pushed by level 0..7+ (lanes), one child:    ");
    for (int i = 0; i < 8; i++) fprintf(stderr, " %llu", pf[40 + i]);
    fprintf(stderr, "\n");
    fprintf(stderr, "QR_PROF trnode cells reached %llu, ranges that end without a member handed out %llu\n", pf[62], pf[63]);
    /* own-surface cells and cells that cast no shadow in the packet walks' solves (profiles/r25_own_surface_roots.txt) */
    for (int k = 0; k < 3; k++)
    {
        const unsigned long long *a = pf + 50 + 4 * k;
        fprintf(stderr, "QR_PROF solves of %s packet walks: own-surface cells plane %llu quadric %llu two-plane %llu, cells that cast no shadow %llu\n",
                kind[k], a[0], a[1], a[2], a[3]);
    }
    /* packet shadow pyramid (qr_shade.hpp): the level of the node a wave's vote chose, and the votes that ended on an empty node */
    fprintf(stderr, "QR_PROF pyramid votes by level 0..7:");
    for (int i = 0; i < 8; i++) fprintf(stderr, " %llu", pf[64 + i]);
    fprintf(stderr, ", on an empty node (no walk) %llu\n", pf[72]);
    unsigned long long z[80] = {0};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(qr_prof), z, sizeof(z)));
#endif
#ifdef QR_STATS
    unsigned long long st[60];
    HIP_TRY(hipMemcpy(st, s->d_counters + 4, sizeof(st), hipMemcpyDeviceToHost));
    /* arrays with a cull sphere in the packet walks (walk_list, profiles/r22_array_cull.txt) */
    for (int k = 0; k < 3; k++)
    {
        const unsigned long long *a = st + 32 + 9 * k;
        fprintf(stderr, "QR_STATS arrays %s: handed out %llu jumped in the run %llu jumped past waiting rays %llu jumped onto END %llu "
                        "left all inside %llu split %llu rays ruled out %llu with occluded rays %llu with waiting rays %llu\n",
                kind[k], a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]);
    }
    if (st[27]) fprintf(stderr, "QR_GUARD %llu bad cell offsets; first: tag %llu offset 0x%llx context 0x%llx\n", st[27], st[24], st[25], st[26]);
    fprintf(stderr, "QR_STATS per-lane walks %llu: steps %llu (%.1f per walk, %.1f lanes stepping), solve rounds %llu (%.1f lanes solving)\n",
            st[16], st[17], st[16] ? (double)st[17] / st[16] : 0.0, st[17] ? (double)st[18] / st[17] : 0.0,
            st[19], st[19] ? (double)st[20] / st[19] : 0.0);
    fprintf(stderr, "QR_STATS per-lane SHADOW walks %llu: steps %llu (%.1f per walk, %.1f lanes stepping, %.1f lanes at start), solve rounds %llu; non-shadow lanes at start %.1f\n",
            st[9], st[10], st[9] ? (double)st[10] / st[9] : 0.0, st[10] ? (double)st[11] / st[10] : 0.0,
            st[9] ? (double)st[15] / st[9] : 0.0, st[22], st[16] ? (double)st[21] / st[16] : 0.0);
    fprintf(stderr, "QR_STATS ranges handed over %llu\n", st[23]);
    fprintf(stderr, "QR_STATS outer rounds %llu: %.1f lanes tracing, %.1f lanes not finished\n", st[28], st[28] ? (double)st[29] / st[28] : 0.0, st[28] ? (double)st[30] / st[28] : 0.0);
    for (int k = 0; k < 3; k++)
        fprintf(stderr, "QR_STATS %s: walks %llu elem-iterations %llu (%.1f per walk, %.0f%% culled) active lanes per iteration %.1f\n", kind[k],
                st[3 * k], st[3 * k + 1], st[3 * k] ? (double)st[3 * k + 1] / st[3 * k] : 0.0,
                st[3 * k + 1] ? 100.0 * st[12 + k] / st[3 * k + 1] : 0.0,
                st[3 * k + 1] ? (double)st[3 * k + 2] / st[3 * k + 1] : 0.0);
#endif
    return QR_OK;
}

/* QR_WAVETIME builds: the stamps of a scene's waves, QR_WT_SLOTS words per schedule entry behind the counter head -- per wave
 * of the last launch {start, first traverse done, end} in 100 MHz ticks, {hw_id | xcc << 32 | walks << 40} */
static int diag_wavetime_clear(qr_device_scene *s, hipStream_t st)
{
    (void)s; (void)st;
#ifdef QR_WAVETIME
    HIP_TRY(hipMemsetAsync(s->d_counters + QR_COUNTER_HEAD, 0, (size_t)s->lp.n_blocks * QR_WT_SLOTS * sizeof(unsigned long long), st));
#endif
    return QR_OK;
}

#ifdef QR_WAVETIME
/* tools/gpu_timeline.py: the stamps the waves of this scene's LAST launch wrote; not part of include/qrhip.h -- the product
 * library does not export it */
extern "C" int qr_wavetime_read(qr_device_scene *s, unsigned long long *out, uint64_t n_words, int clear)
{
    if (s == nullptr || out == nullptr) return qr_fail(QR_ERR_ARG, "bad argument");
    const uint64_t have = (uint64_t)s->lp.n_blocks * QR_WT_SLOTS;
    if (n_words > have) n_words = have;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpy(out, s->d_counters + QR_COUNTER_HEAD, n_words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (clear) HIP_TRY(hipMemset(s->d_counters + QR_COUNTER_HEAD, 0, have * sizeof(unsigned long long)));
    return (int)QR_WT_SLOTS;
}
#endif

/* QR_WAVETIME_OUT=path: the stamps of the last launch, written to that file */
static int diag_wavetime_dump(qr_device_scene *s)
{
    (void)s;
#ifdef QR_WAVETIME
    if (const char *path = getenv("QR_WAVETIME_OUT"))
    {
        std::vector<unsigned long long> w((size_t)s->lp.n_blocks * QR_WT_SLOTS);
        const int rc = qr_wavetime_read(s, w.data(), w.size(), 0);
        if (rc < 0) return rc;
        FILE *f = fopen(path, "wb");
        if (f) { fwrite(w.data(), sizeof(unsigned long long), w.size(), f); fclose(f); }
    }
#endif
    return QR_OK;
}
