/*
 * qr_dropin.hpp - qr_render0, the reference entry point.  Host code; included by qr_device.hip last.
 *
 * One call = flatten + compile + upload + launch + copy back; nothing of the
 * caller's memory is retained (the engine releases its pools every frame, engine.cpp:3317-3323).
 *
 * What IS kept, per calling thread, is our own: per entry of QR_DEVICES (one entry without it) a device arena for the
 * scene image and the frame (no hipMalloc / hipFree per call) and streams; page-locked staging buffers and the vectors
 * of the host passes.  The frame is rendered in horizontal blocks (the schedule is grouped by block), QR_DROPIN_BLOCKS of
 * them on one device, a run of blocks per device on several: block k is copied back over PCIe on its device's copy
 * stream while block k + 1 renders, and the host moves finished blocks into the caller's frame (non-temporal stores)
 * while the next copy is in flight -- or, when the caller has registered its frame (qr_frame_register), the copy engines
 * write the blocks straight into it.  When the flattened scene is byte-identical to the one this thread uploaded last (a
 * paused animation), validation, compilation and upload are skipped.
 */
#ifndef QR_DROPIN_BLOCKS
#define QR_DROPIN_BLOCKS 4
#ifndef QR_DROPIN_STREAMS
#define QR_DROPIN_STREAMS 3     /* measured through the engine, demo1 / demo1 + swarm, ms per frame: 1: 0.83 / 14.1, 2: 0.75 / 12.3, 3: 0.76 / 11.3, 4: 0.83 / 12.1 */
#endif
#endif

/* The caller's rt_SIMD_INFOX, read through its ABI description: pointer-sized fields and the lane-broadcast sample counters. */
struct SInf
{
    uint8_t *inf; size_t ps, Q, P;
    SInf(const void *s_inf, const qr_abi_desc *abi) : inf((uint8_t *)(uintptr_t)s_inf), ps(abi->pointer_bits / 8), Q(abi->quads), P(abi->pointer_bits / 32) {}
    /* pointer-sized field `slot` behind the Q * 0x100 bytes of vector fields (tracer.h:163-211); sign: a signed number */
    uint64_t field(int slot, bool sign = false) const
    {
        const uint8_t *at = inf + Q * 0x100 + (size_t)slot * ps;
        uint64_t p = 0; uint32_t a;
        if (ps == 8) memcpy(&p, at, 8); else { memcpy(&a, at, 4); p = sign ? (uint64_t)(int64_t)(int32_t)a : a; }
        return p;
    }
    /* inf_PTS_C / _O / _U (k = 0, 1, 2): sample count + 1 and the weights of the running mean, lanes() floats each
     * (tracer.h:251-257); the count is the one field of s_inf render0 writes */
    float *pts(int k) const { return (float *)(inf + Q * (0x130 + 0x10 * (size_t)k) + 0x100 * P); }
    size_t lanes() const { return Q * 4; }
};

/* what one entry of the device list holds on its device */
struct DropSlot
{
    int device = -1;
    DevBuf blob, frame, counters;
    DevBuf pt;                                  /* path-tracer mode: device copies of the engine's seed plane and three colour planes */
    hipStream_t sk = nullptr, sc = nullptr;
    hipStream_t sx[QR_DROPIN_BLOCKS] = {};     /* one launch stream per row block (sx[0] == sk): a block's tail overlaps the next block's bulk */
    hipEvent_t ev_up = nullptr;                 /* uploads of this call are on the device */
    hipEvent_t ev_k[QR_DROPIN_BLOCKS] = {}, ev_c[QR_DROPIN_BLOCKS] = {};
    bool resident = false;              /* the thread's current program is the image in `blob` */
};

struct DropIn
{
    DropSlot slot[QR_MAX_DEVICES];
    int n_slots = 0;
    PinBuf h_stage, h_frame;            /* every device uploads from h_stage */
    std::vector<uint8_t> blob, last_blob;
    HostPass hp;
    QrProgram prog;
    bool compiled = false;              /* prog is the program of last_blob ... */
    int compiled_blocks = 0;            /* ... with its schedule grouped for this many row blocks */
    void evict() { for (DropSlot &s : slot) s.resident = false; }      /* no image can be trusted to be on its device */
    int fail(int rc) { evict(); return rc; }
};
static thread_local DropIn g_drop;

/* everything a slot holds on its device, made current here; false: that device cannot be reached, the slot is left as it is */
static bool slot_release(DropSlot &c)
{
    if (c.device < 0) { c = DropSlot(); return true; }
    if (hipSetDevice(c.device) != hipSuccess) return false;
    (void)hipDeviceSynchronize();
    for (int k = 1; k < QR_DROPIN_BLOCKS; k++) if (c.sx[k]) (void)hipStreamDestroy(c.sx[k]);
    if (c.sk) (void)hipStreamDestroy(c.sk);
    if (c.sc) (void)hipStreamDestroy(c.sc);
    if (c.ev_up) (void)hipEventDestroy(c.ev_up);
    for (int k = 0; k < QR_DROPIN_BLOCKS; k++) { if (c.ev_k[k]) (void)hipEventDestroy(c.ev_k[k]); if (c.ev_c[k]) (void)hipEventDestroy(c.ev_c[k]); }
    c.blob.release(); c.frame.release(); c.counters.release(); c.pt.release();
    c = DropSlot();
    return true;
}

/* streams, events: created together; on any failure nothing is kept (the slot's device stays -1, the next call starts over) */
static int slot_create(DropSlot &c)
{
    HIP_TRY(hipStreamCreateWithFlags(&c.sk, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&c.sc, hipStreamNonBlocking));
    c.sx[0] = c.sk;
    for (int k = 1; k < QR_DROPIN_BLOCKS; k++) HIP_TRY(hipStreamCreateWithFlags(&c.sx[k], hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&c.ev_up, hipEventDisableTiming));
    for (int k = 0; k < QR_DROPIN_BLOCKS; k++) { HIP_TRY(hipEventCreateWithFlags(&c.ev_k[k], hipEventDisableTiming)); HIP_TRY(hipEventCreateWithFlags(&c.ev_c[k], hipEventDisableTiming)); }
    return QR_OK;
}

static int slot_prepare(DropSlot &c, int dev, size_t image_bytes, size_t frame_bytes, size_t n_sched)
{
    if (c.device != dev)
    {
        /* first call of this thread, or another device: what the previous device held is released there first;
         * c.device is only set once every stream and event exists, so a failure leaves no half-built state behind */
        (void)slot_release(c); c.device = -1;
        QR_TRY(pick_device(dev));
        const int rc = slot_create(c);
        if (rc != QR_OK) { c.device = dev; (void)slot_release(c); return rc; }
        c.device = dev;
    }
    else HIP_TRY(hipSetDevice(dev));
    HIP_TRY(counters_ensure(c.counters, n_sched));
    bool grew = false;
    const hipError_t image_alloc = c.blob.ensure(image_bytes, image_slack(image_bytes), &grew);
    if (grew) c.resident = false;
    HIP_TRY(image_alloc);
    HIP_TRY(c.frame.ensure(frame_bytes));
    return QR_OK;
}

/* the thread's page-locked staging buffers (some device is current) */
static int dropin_host_buffers(DropIn &c, size_t image_bytes, size_t frame_bytes)
{
    bool grew = false;
    const hipError_t image_alloc = c.h_stage.ensure(image_bytes, image_slack(image_bytes), &grew);
    if (grew) c.evict();                        /* the image every upload reads is gone */
    HIP_TRY(image_alloc);
    HIP_TRY(c.h_frame.ensure(frame_bytes));
    return QR_OK;
}

/*
 * Path-tracer mode through the drop-in entry point.  The engine keeps one LCG state per pixel sample (inf_PSEED) and three
 * colour planes with the running mean (inf_PTR_R/G/B, engine.cpp:2875-2893), all frm_row << fsaa words per row, and a
 * sample counter in every thread's rt_SIMD_INFOX which render0 itself advances (tracer.cpp:1112-1136).  A call owns rows
 * index, index + thnum, ...: those rows of the four planes travel to the device before the launches and back after them.
 */
struct DropInPt
{
    uint8_t *host[4] = { nullptr, nullptr, nullptr, nullptr };     /* seeds, r, g, b on the host */
    size_t row_bytes = 0, plane_words = 0;
    int first = 0, step = 1, rows = 0;
};

static int dropin_pt_begin(DropSlot &c, const SInf &si, const LaunchP &lp, const qr_frame &fr, DropInPt &io, PtParams &pt)
{
    static const int slot[4] = { 3, 16, 17, 18 };       /* inf_PSEED, inf_PTR_R, inf_PTR_G, inf_PTR_B (tracer.h:163, 205-211) */
    for (int k = 0; k < 4; k++)
    {
        io.host[k] = (uint8_t *)(uintptr_t)si.field(slot[k]);
        if (io.host[k] == nullptr) return qr_fail(QR_ERR_ARG, "path-tracer mode without seed / colour planes in s_inf");
    }
    const float cnt = si.pts(0)[0] + 1.0f, o = 1.0f / cnt, u = 1.0f - o;
    for (size_t l = 0; l < si.lanes(); l++) { si.pts(0)[l] = cnt; si.pts(1)[l] = o; si.pts(2)[l] = u; }

    const size_t ns = (size_t)1 << fr.fsaa;
    io.row_bytes = (size_t)fr.frm_row * ns * 4;
    io.plane_words = (size_t)fr.frm_row * fr.frm_h * ns;
    io.step = lp.thnum;
    io.first = lp.index;
    io.rows = fr.frm_h > io.first ? (fr.frm_h - io.first + io.step - 1) / io.step : 0;
    HIP_TRY(c.pt.ensure(4 * io.plane_words * 4));
    uint32_t *const d_pt = c.pt.as<uint32_t>();
    for (int k = 0; k < 4 && io.rows > 0; k++)
        HIP_TRY(hipMemcpy2DAsync((uint8_t *)(d_pt + (size_t)k * io.plane_words) + (size_t)io.first * io.row_bytes, io.step * io.row_bytes,
                                 io.host[k] + (size_t)io.first * io.row_bytes, io.step * io.row_bytes,
                                 io.row_bytes, (size_t)io.rows, hipMemcpyHostToDevice, c.sk));
    pt.seeds = d_pt;
    pt.acc_r = (float *)(d_pt + io.plane_words); pt.acc_g = (float *)(d_pt + 2 * io.plane_words); pt.acc_b = (float *)(d_pt + 3 * io.plane_words);
    pt.pts_o = o; pt.pts_u = u;
    pt.eager = 1;               /* the reference's shading order: its random streams, its frames */
    pt.pad = 0;
    return QR_OK;
}

static hipError_t dropin_pt_end(DropSlot &c, const DropInPt &io)
{
    hipError_t e = hipSuccess;
    for (int k = 0; k < 4 && io.rows > 0 && e == hipSuccess; k++)
        e = hipMemcpy2DAsync(io.host[k] + (size_t)io.first * io.row_bytes, io.step * io.row_bytes,
                             (const uint8_t *)(c.pt.as<uint32_t>() + (size_t)k * io.plane_words) + (size_t)io.first * io.row_bytes, io.step * io.row_bytes,
                             io.row_bytes, (size_t)io.rows, hipMemcpyDeviceToHost, c.sk);
    if (e == hipSuccess) e = hipStreamSynchronize(c.sk);
    return e;
}

extern "C" int qr_render0(const void *s_inf, const qr_abi_desc *abi)
{
    const bool verbose = getenv("QR_VERBOSE") != nullptr;
    const double t0 = now_ms();
    DropIn &c = g_drop;
    std::string err;
    int rc = qr_flatten_impl(s_inf, abi, c.blob, err);
    if (rc != QR_OK) return qr_fail(rc, err);
    const double t1 = now_ms();

    /* frame pointer and stride: inf_FRAME / inf_FRM_ROW, tracer.h:186-190 */
    const SInf si(s_inf, abi);
    uint32_t *frame_host = (uint32_t *)(uintptr_t)si.field(11);
    const int row_pixels = (int)(int64_t)si.field(10, true);
    if (frame_host == nullptr) return qr_fail(QR_ERR_ARG, "s_inf->frame is NULL");

    /* the devices of this call, and with them the number of row blocks of the schedule: QR_DROPIN_BLOCKS on one device,
     * a run of blocks (at least one) for each of several.  A path-traced frame stays on the first device: its sample planes
     * live there */
    std::vector<int> devs;
    QR_TRY(device_list(devs));
    qr_scene_view v;
    QR_TRY(view_of(c.blob.data(), c.blob.size(), v));
    if (v.frame->pt_on) devs.resize(1);
    const int n_dev = (int)devs.size();
    const int want_blocks = n_dev * (n_dev >= QR_DROPIN_BLOCKS ? 1 : QR_DROPIN_BLOCKS / n_dev);

    /* host passes (skipped when nothing changed since this thread's last call) */
    const bool same = c.compiled && c.compiled_blocks == want_blocks && c.blob.size() == c.last_blob.size()
                   && memcmp(c.blob.data(), c.last_blob.data(), c.blob.size()) == 0;
    if (!same)
    {
        c.compiled = false;
        c.evict();
        static const bool rebin = env_tristate("QR_REBIN") == 1;
        /* no packet shadow pyramids in an image that is compiled for ONE frame: building them costs more host time than the
         * frame's kernel gets back (profiles/r30_packet_shadow_pyramid.txt); QR_DROPIN_PGRID=1 builds them all the same */
        static const bool pgrid = env_tristate("QR_DROPIN_PGRID") == 1;
        QR_TRY(build_program(v, devs[0], rebin, c.hp, c.prog, 0, want_blocks, false, pgrid ? 0u : QR_BUILD_NO_PGRID));
        /* the finished image is verified offset by offset (qr_program_verify) on EVERY frame that was compiled: the layout
         * depends on list contents (programs shared by content, clear runs, box cells), so equal totals do not mean an equal
         * structure, and the product kernel checks no offset it loads.  The walk costs ~0.05 ms at 1080p since heads equal to
         * the one just checked are skipped (tools/host_compile_time.py).  QR_VERIFY=0 switches it off (timing experiments) */
        static const bool verify_on = env_tristate("QR_VERIFY") != 0;
        if (verify_on && (rc = qr_program_verify(c.prog, err)) != QR_OK) return qr_fail(rc, err);
    }
    const double t2 = now_ms();
    const qr_frame &fr = c.prog.frm;
    const int w = fr.frm_w, h = fr.frm_h;
    const size_t frame_bytes = (size_t)w * h * 4;
    const int K = (int)c.prog.block_first.size() - 1;          /* fewer than asked for on a frame of few tile rows */
    const int bps = (K + n_dev - 1) / n_dev;                   /* blocks per slot: block k belongs to slot k / bps */
    if (K < 1 || bps > QR_DROPIN_BLOCKS) return qr_fail(QR_ERR_ARG, "schedule blocks do not match the device list");
    /* slots in use: entry j of the list; slots beyond the list release what they hold */
    for (int j = 0; j < n_dev; j++) QR_TRY(slot_prepare(c.slot[j], devs[(size_t)j], c.prog.blob.size(), frame_bytes, c.prog.n_sched));
    for (int j = n_dev; j < c.n_slots; j++) { (void)slot_release(c.slot[j]); c.slot[j] = DropSlot(); }
    c.n_slots = n_dev;
    HostDst dst(frame_host, row_pixels, w, h);
    QR_TRY(dropin_host_buffers(c, c.prog.blob.size(), dst.pinned ? 0 : frame_bytes));
    dst.stage = c.h_frame.as<uint32_t>();
    if (!same)
    {
        memcpy(c.h_stage.p, c.prog.blob.data(), c.prog.blob.size());
        c.last_blob.swap(c.blob);
        c.compiled = true; c.compiled_blocks = want_blocks;
    }
    hipError_t e = hipSuccess;
    for (int j = 0; j < n_dev && e == hipSuccess; j++)
    {
        DropSlot &sl = c.slot[j];
        e = hipSetDevice(sl.device);
        if (e == hipSuccess && !sl.resident)
        {
            e = hipMemcpyAsync(sl.blob.p, c.h_stage.p, c.prog.blob.size(), hipMemcpyHostToDevice, sl.sk);
            sl.resident = e == hipSuccess;
        }
        if (e == hipSuccess) e = hipEventRecord(sl.ev_up, sl.sk);
    }
    if (e != hipSuccess) return c.fail(qr_fail(QR_ERR_DEVICE, std::string("qr_render0 upload: ") + hipGetErrorString(e)));
    const double t3 = now_ms();

    LaunchP lp = launchp_of(fr);
    DropInPt ptio; PtParams pt = {};
    if (fr.pt_on)
    {
        HIP_TRY(hipSetDevice(c.slot[0].device));
        QR_TRY(dropin_pt_begin(c.slot[0], si, lp, fr, ptio, pt));
        /* the seed and colour planes travel on the slot's first stream AFTER the image: the launch streams of the later row
         * blocks wait on ev_up, so it is recorded again behind those copies (round 4: recorded only behind the image, a block
         * on sx[1] / sx[2] could start before its seeds had arrived -- one wrong frame in ~20 runs with four engine threads) */
        HIP_TRY(hipEventRecord(c.slot[0].ev_up, c.slot[0].sk));
    }
    else
    {
        /* FF_ini, tracer.cpp:1128-1132: every ray-traced frame zeroes the sample count in s_inf; rt_Scene::set_pton relies on
         * it to restart the accumulation after it has reset the seed and colour planes (engine.cpp:3729-3745) */
        for (size_t l = 0; l < si.lanes(); l++) si.pts(0)[l] = 0.0f;
    }

    /* kernel instance as for uploaded scenes, QR_DIV read once per process */
    static const int force_div = env_tristate("QR_DIV");
    const Instance inst = { pick_divk(force_div, c.prog) };
    /* QR_DROPIN_STREAMS=n: a slot's blocks on n streams in turn (1: one after the other) */
    static const int n_streams = []() { const char *v = getenv("QR_DROPIN_STREAMS"); const int n = v ? atoi(v) : QR_DROPIN_STREAMS;
                                        return n < 1 ? 1 : (n > QR_DROPIN_BLOCKS ? QR_DROPIN_BLOCKS : n); }();
    for (int k = 0; k < K && e == hipSuccess; k++)
    {
        DropSlot &sl = c.slot[k / bps];
        const int kk = k % bps;
        if ((e = hipSetDevice(sl.device)) != hipSuccess) break;
        hipStream_t sk = sl.sx[kk % n_streams];
        if (sk != sl.sk) e = hipStreamWaitEvent(sk, sl.ev_up, 0);
        if (e != hipSuccess) break;
        const uint32_t e0 = c.prog.block_first[k], e1 = c.prog.block_first[k + 1];
        unsigned long long *const counters = sl.counters.as<unsigned long long>();
        lp.B = (const char *)sl.blob.p;
        lp.stats = counters + 4;
        lp.order = (const uint32_t *)((const char *)sl.blob.p + c.prog.off_order) + 2 * (size_t)e0;
        lp.n_blocks = (int32_t)(e1 - e0);
        lp.row_begin = (int32_t)c.prog.block_row[k]; lp.row_end = (int32_t)c.prog.block_row[k + 1];
        e = launch_lp<false>(inst, lp, sl.frame.as<uint32_t>(), nullptr, counters, sk, fr.pt_on ? &pt : nullptr);
        if (e == hipSuccess) e = hipEventRecord(sl.ev_k[kk], sk);
        /* copy block k back as soon as it is rendered, on the slot's copy stream: into the caller's registered frame, or
         * into the staging frame */
        if (e == hipSuccess) e = hipStreamWaitEvent(sl.sc, sl.ev_k[kk], 0);
        if (e == hipSuccess) e = band_send(dst, sl.frame.as<uint32_t>(), lp.row_begin, lp.row_end, lp.index, lp.thnum, sl.sc);
        if (e == hipSuccess) e = hipEventRecord(sl.ev_c[kk], sl.sc);
    }
    if (fr.pt_on && e == hipSuccess)
    {
        DropSlot &sl = c.slot[0];
        for (int k = 0; k < K && e == hipSuccess; k++) e = hipStreamWaitEvent(sl.sk, sl.ev_k[k % bps], 0);   /* the planes go back when every block is done */
        if (e == hipSuccess) e = dropin_pt_end(sl, ptio);    /* the planes with this frame's sample go back to the engine */
    }
    const double t4 = now_ms();
    /* the host moves finished blocks into the caller's frame: only the rows this call owns (index / thnum),
     * honouring a negative stride (bottom-up frames, engine.cpp:2814-2850); a registered frame only waits for its copies */
    for (int k = 0; k < K && e == hipSuccess; k++)
    {
        e = hipEventSynchronize(c.slot[k / bps].ev_c[k % bps]);
        if (e == hipSuccess) band_land(dst, (int)c.prog.block_row[k], (int)c.prog.block_row[k + 1], lp.index, lp.thnum);
    }
    if (e != hipSuccess) return c.fail(qr_fail(QR_ERR_DEVICE, std::string("qr_render0: ") + hipGetErrorString(e)));
    if (verbose)
        fprintf(stderr, "qr_render0: flatten %.3f ms (%zu bytes), validate+compile %.3f ms%s, stage+upload %.3f ms (%zu bytes), launches %.3f ms, wait+copy-back %.3f ms%s, %d device slot%s\n",
                t1 - t0, c.last_blob.size(), t2 - t1, same ? " (unchanged scene: skipped)" : "", t3 - t2, c.prog.blob.size(), t4 - t3, now_ms() - t4,
                dst.pinned ? " (registered frame: direct)" : "", n_dev, n_dev == 1 ? "" : "s");
    return QR_OK;
}
