/*
 * qr_dev_upload.hpp - a snapshot becomes a program (the host half, shared with qr_render0) and the program a scene on a
 * device.  Host code; included by qr_device.hip after qr_dev_launch.hpp.
 */
static int pick_device(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return qr_fail(QR_ERR_DEVICE, "no HIP device available (the gfx950 backend has no CPU fallback)");
    if (device < 0 || device >= ndev) return qr_fail(QR_ERR_ARG, "device ordinal out of range");
    HIP_TRY(hipSetDevice(device));
    return QR_OK;
}

#include "qr_bounds.hpp"
#include "qr_binning.hpp"

static int view_of(const void *blob, uint64_t size, qr_scene_view &v)
{
    const int rc = qr_scene_view_init(&v, blob, size);
    if (rc != 0) return qr_fail(QR_ERR_ARG, "malformed snapshot (qr_scene_view_init " + std::to_string(rc) + ")");
    return QR_OK;
}

/* the vectors of the host passes: working copies of the list cells and tile heads (the tile lists, and with them the cell
 * array and the tile geometry of the frame record, are replaced when the binning pass runs) */
struct HostPass { std::vector<BSphere> bsph; std::vector<qr_elem> E; std::vector<int32_t> T; };

/* Host half of an upload: validate, bound, (re-bin on `device`), compile -> prog.  verbose 1: the bounding-sphere count,
 * 2: the time of every phase as well; want_blocks / finalize / query_flags: qr_program_build's. */
static int build_program(const qr_scene_view &v, int device, bool rebin, HostPass &hp, QrProgram &prog, int verbose,
                         int want_blocks, bool finalize, uint32_t query_flags)
{
    double ph_t = verbose >= 2 ? now_ms() : 0.0;
    auto phase = [&](const char *name) { if (verbose >= 2) { const double t = now_ms(); fprintf(stderr, "upload phase %-12s %.3f ms\n", name, t - ph_t); ph_t = t; } };
    std::string err;
    int rc = qr_snapshot_validate(v, err);
    if (rc != QR_OK) return qr_fail(rc, err);
    phase("validate");
    qr_bound_spheres(v, hp.bsph);
    if (verbose)
    {
        int nreal = 0, nfin = 0;
        for (uint32_t i = 0; i < v.hdr->n_srf; i++)
        {
            const qr_surface &q = v.srf[i];
            if (q.srf_t[3] < 0 || q.srf_t[3] >= QR_TAG_SURFACE_MAX) continue;
            nreal++; if (hp.bsph[i].r < 1e30f) nfin++;
        }
        fprintf(stderr, "bounding spheres: %d of %d real surfaces bounded\n", nfin, nreal);
    }
    phase("bounds");
    if (rebin) hp.E.reserve((size_t)v.hdr->n_elm + (size_t)v.hdr->n_elm / 2 + 65536);      /* room for the tile cells */
    hp.E.assign(v.elm, v.elm + v.hdr->n_elm);
    hp.T.assign(v.tiles, v.tiles + v.hdr->n_tiles);
    qr_frame frm = *v.frame;
    /* QR_REBIN=1: the per-tile lists are rebuilt on the GPU from the camera list instead of taken from the engine (the
     * engine may then run without its own tiling, RT_OPTS_TILING).  The frame is the engine's UNTILED picture: on most
     * scenes that is also its tiled one, but where its screen tiling drops a surface from a tile that the surface does
     * cover the two differ, so this is not the drop-in-exact mode */
    if (rebin)
    {
        QR_TRY(pick_device(device));
        QR_TRY(rebin_tiles(v, hp.bsph, frm, hp.E, hp.T));
        phase("rebin");
    }
    rc = qr_program_build(v, hp.E, hp.T, frm, hp.bsph, prog, err, want_blocks, finalize, query_flags);
    if (rc != QR_OK) return qr_fail(rc, err);
    phase("compile");
    return QR_OK;
}

extern "C" int qr_scene_upload(const void *blob, uint64_t size, int device, qr_device_scene **out) { return qr_scene_upload_ex(blob, size, device, 0u, out); }

extern "C" int qr_scene_upload_ex(const void *blob, uint64_t size, int device, uint32_t flags, qr_device_scene **out)
{
    if (blob == nullptr || out == nullptr) return qr_fail(QR_ERR_ARG, "null argument");
    if (getenv("QR_REBIN") && atoi(getenv("QR_REBIN")) != 0) flags |= QR_UPLOAD_REBIN_TILES;
    const char *qv = getenv("QR_VERBOSE");
    qr_scene_view v;
    QR_TRY(view_of(blob, size, v));
    QrProgram prog; HostPass hp;
    QR_TRY(build_program(v, device, (flags & QR_UPLOAD_REBIN_TILES) != 0, hp, prog, qv ? (atoi(qv) >= 2 ? 2 : 1) : 0, 0, true,
                         flags & QR_UPLOAD_RAY_QUERIES));
    QR_TRY(pick_device(device));
    const size_t total = prog.blob.size();

    /* staging buffer in page-locked memory, kept per thread: a pageable host-to-device copy above ~1 MB
     * takes 13-23 ms on this stack (the runtime pins the source on the fly), a pinned one 0.1 ms */
    static thread_local StageBuf stage;
    HIP_TRY(stage.ensure(total, total / 2));
    memcpy(stage.p, prog.blob.data(), total);

    /* every failure exit below destroys what the scene holds so far */
    struct Guard { qr_device_scene *s; ~Guard() { (void)qr_scene_destroy(s); } } g = { new qr_device_scene() };
    qr_device_scene *s = g.s;                       /* value-initialised: plain members are zero */
    static std::atomic<uint64_t> next_serial{1};
    s->serial = next_serial.fetch_add(1, std::memory_order_relaxed);
    s->device = device; s->hdr = *v.hdr;
    const double tm0 = now_ms();
    HIP_TRY(hipMalloc(&s->d_blob, total));
    const double tm1 = now_ms();
    const hipError_t image_hipMemcpy = hipMemcpy(s->d_blob, stage.p, total, hipMemcpyHostToDevice);
    if (qv) fprintf(stderr, "upload: device bytes %zu, hipMalloc %.3f ms, hipMemcpy %.3f ms\n", total, tm1 - tm0, now_ms() - tm1);
    HIP_TRY(image_hipMemcpy);
    HIP_TRY(hipMalloc((void **)&s->d_counters, counter_bytes(prog.n_sched)));
    s->blob_bytes = total;

    s->fr = prog.frm;
    s->lp = launchp_of(prog.frm);
    s->lp.B = (const char *)s->d_blob;
    s->lp.order = (const uint32_t *)((const char *)s->d_blob + prog.off_order);
    s->lp.n_blocks = (int32_t)prog.n_sched;
    s->lp.stats = s->d_counters + 4;
    s->lp.dbg = getenv("QR_DBG") ? atoi(getenv("QR_DBG")) : 0;
    s->h_order.swap(prog.order);
    s->n_cells = hp.E.size();
    s->off_query = prog.off_query; s->off_mat = prog.off_mat;
    s->divk = pick_divk(env_tristate("QR_DIV"), prog);          /* read per upload: tests set QR_DIV between scenes */
    s->n_groups = (prog.frm.frm_h + 7) / 8;
    g.s = nullptr;
    *out = s;
    return QR_OK;
}

extern "C" int qr_scene_destroy(qr_device_scene *s)
{
    if (s == nullptr) return QR_OK;
    (void)hipSetDevice(s->device);
    multi_forget(s);
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    for (auto &kv : s->sub) kv.second.release();
    (void)hipFree(s->d_counters); (void)hipFree(s->d_blob); (void)hipFree(s->d_seeds); (void)hipFree(s->d_acc);
    delete s;
    return QR_OK;
}
