/*
 * qr_dev_host.hpp - frames in host memory: the device list, registered frames, the copy-back of rendered rows, and
 * qr_render_host with its QR_DEVICES replicas.  Host code; included by qr_device.hip.
 */

/* per-thread device frame + pinned staging buffer, kept between calls: the drop-in path renders a frame
 * per call, and hipMalloc/hipFree plus a pageable 8 MB copy cost more than the kernel itself */
#define QR_COPY_CHUNKS 4
#define QR_MAX_DEVICES 8

/* copy into the caller's frame with non-temporal stores: the frame is written once and not read by us, so
 * read-for-ownership traffic and cache pollution of a plain memcpy are avoided (8 MB per frame) */
static void copy_streaming(void *dst, const void *src, size_t n)
{
#if defined(__SSE2__)
    uint8_t *d = (uint8_t *)dst; const uint8_t *s = (const uint8_t *)src;
    const size_t head = (16 - ((uintptr_t)d & 15)) & 15;
    if (n < 4096 || head >= n) { memcpy(dst, src, n); return; }
    memcpy(d, s, head); d += head; s += head; n -= head;
    const size_t blocks = n / 64;
    for (size_t i = 0; i < blocks; i++)
    {
        const __m128i a = _mm_loadu_si128((const __m128i *)(s + 0)), b = _mm_loadu_si128((const __m128i *)(s + 16));
        const __m128i c = _mm_loadu_si128((const __m128i *)(s + 32)), e = _mm_loadu_si128((const __m128i *)(s + 48));
        _mm_stream_si128((__m128i *)(d + 0), a); _mm_stream_si128((__m128i *)(d + 16), b);
        _mm_stream_si128((__m128i *)(d + 32), c); _mm_stream_si128((__m128i *)(d + 48), e);
        s += 64; d += 64;
    }
    _mm_sfence();
    memcpy(d, s, n - blocks * 64);
#else
    memcpy(dst, src, n);
#endif
}

/*
 * QR_DEVICES=0,1,...: the frame of a host-frame call (qr_render0, qr_render_host) is cut into blocks of rows, one run of
 * blocks per entry of the list; every entry renders its rows on its device and copies them into the host frame itself
 * (tracer.cpp:1144-1145 / engine.cpp:3465-3478: the engine's threads own rows index, index + thnum, ... of one frame and write
 * them in place -- here a device owns a band).  The same ordinal may be listed more than once (separate buffers and
 * streams on that device: how a one-GPU box tests the path).  Without QR_DEVICES: the one device of QR_DEVICE (default 0).
 */
static int device_list(std::vector<int> &v)
{
    v.clear();
    if (const char *e = getenv("QR_DEVICES"))
    {
        const char *p = e;
        while (*p)
        {
            while (*p == ',' || *p == ' ') p++;
            if (!*p) break;
            char *end = nullptr;
            const long d = strtol(p, &end, 10);
            if (end == p) return qr_fail(QR_ERR_ARG, std::string("QR_DEVICES: not a list of device ordinals: ") + e);
            /* without any device the call fails as QR_ERR_DEVICE further down (pick_device): no CPU fallback */
            if (d < 0 || (qr_device_count() > 0 && d >= qr_device_count())) return qr_fail(QR_ERR_ARG, std::string("QR_DEVICES: ordinal out of range in ") + e);
            if (v.size() >= QR_MAX_DEVICES) return qr_fail(QR_ERR_ARG, std::string("QR_DEVICES: more than ") + std::to_string(QR_MAX_DEVICES) + " entries");
            v.push_back((int)d);
            p = end;
        }
    }
    if (v.empty()) { int d = 0; if (const char *e = getenv("QR_DEVICE")) d = atoi(e); v.push_back(d); }
    return QR_OK;
}

/*
 * Caller frames registered for direct copies (qr_frame_register): rendered rows go from device memory straight into
 * such a frame by DMA -- no page-locked staging frame, no host copy.  The registration is the CALLER's statement that the
 * range stays mapped until qr_frame_unregister: the library never pins a pointer it merely saw in a call (the engine may
 * free its frame between two calls, engine.cpp:3317-3323 / 2814-2850).
 *
 * Tried and dropped for the drop-in path: page-locking the engine's frame in place for a direct DMA
 * copy-back saves 0.35 ms per 1080p frame on demo1 but makes demo2 ten times slower (host accesses to the
 * engine's heap next to the frame and later copies slow down once the range is registered).
 */
struct PinnedRange { uintptr_t base; size_t bytes; };
static std::vector<PinnedRange> g_pins;
static std::mutex g_pins_lock;

extern "C" int qr_frame_register(void *frame, uint64_t bytes)
{
    if (frame == nullptr || bytes == 0) return qr_fail(QR_ERR_ARG, "null frame");
    std::vector<int> dl;
    QR_TRY(device_list(dl));
    QR_TRY(pick_device(dl[0]));
    std::lock_guard<std::mutex> lk(g_pins_lock);
    for (const PinnedRange &r : g_pins)
        if (r.base == (uintptr_t)frame) return r.bytes == bytes ? QR_OK : qr_fail(QR_ERR_ARG, "frame is registered with another size");
    HIP_TRY(hipHostRegister(frame, (size_t)bytes, hipHostRegisterPortable));
    g_pins.push_back({ (uintptr_t)frame, (size_t)bytes });
    return QR_OK;
}

extern "C" int qr_frame_unregister(void *frame)
{
    std::lock_guard<std::mutex> lk(g_pins_lock);
    for (size_t i = 0; i < g_pins.size(); i++)
        if (g_pins[i].base == (uintptr_t)frame)
        {
            g_pins.erase(g_pins.begin() + (ptrdiff_t)i);
            HIP_TRY(hipHostUnregister(frame));
            return QR_OK;
        }
    return qr_fail(QR_ERR_ARG, "frame was not registered");
}

static bool frame_is_pinned(const void *p, size_t bytes)
{
    std::lock_guard<std::mutex> lk(g_pins_lock);
    for (const PinnedRange &r : g_pins)
        if ((uintptr_t)p >= r.base && (uintptr_t)p + bytes <= r.base + r.bytes) return true;
    return false;
}

/* rows [y0, y1) of a device frame (compact, w pixels a row) that belong to index / thnum, into a registered host frame */
static hipError_t copy_rows_direct(uint32_t *frame_host, int row_pixels, const uint32_t *d_frame, int w, int y0, int y1,
                                   int index, int thnum, hipStream_t st)
{
    if (thnum <= 1)
    {
        if (y1 <= y0) return hipSuccess;
        if (row_pixels == w) return hipMemcpyAsync(frame_host + (size_t)y0 * w, d_frame + (size_t)y0 * w, (size_t)(y1 - y0) * w * 4, hipMemcpyDeviceToHost, st);
        return hipMemcpy2DAsync(frame_host + (size_t)y0 * row_pixels, (size_t)row_pixels * 4, d_frame + (size_t)y0 * w, (size_t)w * 4,
                                (size_t)w * 4, (size_t)(y1 - y0), hipMemcpyDeviceToHost, st);
    }
    const int first = y0 + ((index - y0 % thnum) % thnum + thnum) % thnum;
    if (first >= y1) return hipSuccess;
    const int rows = (y1 - first + thnum - 1) / thnum;
    return hipMemcpy2DAsync(frame_host + (size_t)first * row_pixels, (size_t)thnum * row_pixels * 4, d_frame + (size_t)first * w, (size_t)thnum * w * 4,
                            (size_t)w * 4, (size_t)rows, hipMemcpyDeviceToHost, st);
}

/* rows [y0, y1) of a compact staging frame that belong to index / thnum, into the caller's frame (any stride, also negative:
 * bottom-up frames, engine.cpp:2814-2850) */
static void copy_rows_host(uint32_t *frame_host, int row_pixels, const uint32_t *h_frame, int w, int y0, int y1, int index, int thnum)
{
    if (thnum <= 1 && row_pixels == w) { copy_streaming(frame_host + (size_t)y0 * w, h_frame + (size_t)y0 * w, (size_t)(y1 - y0) * w * 4); return; }
    for (int y = y0; y < y1; y++)
    {
        if (thnum > 1 && (y % thnum) != index) continue;
        memcpy(frame_host + (ptrdiff_t)y * row_pixels, h_frame + (size_t)y * w, (size_t)w * 4);
    }
}

/* Where a call's pixels go: the caller's frame of w x h pixels, directly when it lies in a registered range (`pinned`; a
 * frame with a negative or short stride is not addressable as one range), else through the page-locked staging frame. */
struct HostDst
{
    uint32_t *frame; int row_pixels, w; bool pinned; uint32_t *stage = nullptr;
    HostDst(uint32_t *frame_host, int row_pixels_, int w_, int h) : frame(frame_host), row_pixels(row_pixels_), w(w_)
    {
        const size_t span = row_pixels < w || h <= 0 ? 0 : ((size_t)(h - 1) * (size_t)row_pixels + (size_t)w) * 4;
        pinned = span != 0 && frame_is_pinned(frame_host, span);
    }
};

/* a band's copy-back: rows [y0, y1) of a device frame that belong to index / thnum set out on `st` ... */
static hipError_t band_send(const HostDst &d, const uint32_t *d_frame, int y0, int y1, int index, int thnum, hipStream_t st)
{
    if (d.pinned) return copy_rows_direct(d.frame, d.row_pixels, d_frame, d.w, y0, y1, index, thnum, st);
    if (y1 <= y0) return hipSuccess;
    return hipMemcpyAsync(d.stage + (size_t)y0 * d.w, d_frame + (size_t)y0 * d.w, (size_t)(y1 - y0) * d.w * 4, hipMemcpyDeviceToHost, st);
}
/* ... and, once that copy has finished, reach the caller's frame (a registered frame already has them) */
static void band_land(const HostDst &d, int y0, int y1, int index, int thnum)
{
    if (!d.pinned) copy_rows_host(d.frame, d.row_pixels, d.stage, d.w, y0, y1, index, thnum);
}

/* ---- qr_render_host: uploaded scene -> host frame ---- */

/* what one entry of QR_DEVICES holds for an uploaded scene (several entries only) */
struct HostReplica
{
    int device = -1;
    void *d_blob = nullptr; bool own_blob = false;
    unsigned long long *d_counters = nullptr;
    void *d_frame = nullptr;
    SchedBuf sched; int y0 = 0, y1 = 0;         /* the band of rows and the schedule entries that own them */
    hipStream_t st = nullptr; hipEvent_t ev = nullptr;
};

struct HostPathCache
{
    int device = -1;
    DevBuf d_frame; PinBuf h_frame;
    hipEvent_t ev[QR_COPY_CHUNKS] = {};
    /* QR_DEVICES with several entries: replicas of the scene this thread rendered last */
    uint64_t rep_serial = 0;      /* qr_device_scene::serial the replicas were built for (0: none) */
    std::vector<int> rep_devices;
    std::vector<HostReplica> rep;
    /* no destructor: the HIP runtime may already be shut down when thread-locals are destroyed at exit, so all of it leaks */
};
static thread_local HostPathCache g_hpc;

static void replicas_release(HostPathCache &c)
{
    for (HostReplica &r : c.rep)
    {
        if (r.device < 0 || hipSetDevice(r.device) != hipSuccess) continue;
        (void)hipDeviceSynchronize();
        if (r.own_blob) (void)hipFree(r.d_blob);
        (void)hipFree(r.d_counters); (void)hipFree(r.d_frame); r.sched.release();
        if (r.st) (void)hipStreamDestroy(r.st);
        if (r.ev) (void)hipEventDestroy(r.ev);
    }
    c.rep.clear(); c.rep_serial = 0; c.rep_devices.clear();
}

/* (re)build the replicas of `s` for the device list: image copies (peer copy from the scene's device), the schedule entries
 * of every band, a frame buffer, a stream */
static int replicas_prepare(HostPathCache &c, qr_device_scene *s, const std::vector<int> &devs)
{
    /* keyed on the upload's serial: the address of a destroyed scene and of its image are reused by the next upload of the
     * same size (an animation re-uploads every frame), and replicas of the old image must not render for the new one */
    if (c.rep_serial == s->serial && c.rep_devices == devs) return QR_OK;
    replicas_release(c);
    const int n = (int)devs.size(), H = s->fr.frm_h, W = s->fr.frm_w;
    c.rep.resize((size_t)n);
    for (int j = 0; j < n; j++)
    {
        HostReplica &r = c.rep[(size_t)j];
        int rc = pick_device(devs[(size_t)j]);
        if (rc != QR_OK) { replicas_release(c); return rc; }
        r.device = devs[(size_t)j];
        /* bands of whole 8-row groups */
        const int groups = (H + 7) / 8;
        r.y0 = (int)((long long)groups * j / n) * 8; r.y1 = j == n - 1 ? H : (int)((long long)groups * (j + 1) / n) * 8;
        if (r.y1 > H) r.y1 = H;
        const std::vector<uint32_t> keep = sched_subset(s, sel_band(r.y0, r.y1));
        hipError_t e = hipSuccess;
        if (r.device == s->device) r.d_blob = s->d_blob;
        else
        {
            e = hipMalloc(&r.d_blob, s->blob_bytes);
            if (e == hipSuccess) { r.own_blob = true; e = hipMemcpyPeer(r.d_blob, r.device, s->d_blob, s->device, s->blob_bytes); }
        }
        const size_t cb = counter_bytes(keep.size() / 2);
        if (e == hipSuccess) e = hipMalloc((void **)&r.d_counters, cb);
        if (e == hipSuccess) e = hipMemset(r.d_counters, 0, cb);
        if (e == hipSuccess) e = hipMalloc(&r.d_frame, (size_t)W * H * 4);
        if (e == hipSuccess) e = r.sched.upload(keep, 2);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&r.st, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&r.ev, hipEventDisableTiming);
        if (e != hipSuccess) { replicas_release(c); return qr_fail(QR_ERR_DEVICE, std::string("QR_DEVICES replica: ") + hipGetErrorString(e)); }
    }
    c.rep_serial = s->serial; c.rep_devices = devs;
    return QR_OK;
}

extern "C" int qr_render_host(qr_device_scene *s, uint32_t *frame_host, int row_pixels)
{
    if (s == nullptr || frame_host == nullptr) return qr_fail(QR_ERR_ARG, "null argument");
    const int w = s->fr.frm_w, h = s->fr.frm_h;
    const size_t bytes = (size_t)w * h * 4;
    QR_TRY(pt_rows_ok(s));
    HIP_TRY(hipSetDevice(s->device));
    HostPathCache &c = g_hpc;
    const bool whole = is_whole_frame(s->lp, h);
    HostDst dst(frame_host, row_pixels, w, h);
    if (!dst.pinned) HIP_TRY(c.h_frame.ensure(bytes));
    uint32_t *const h_frame = c.h_frame.as<uint32_t>();
    dst.stage = h_frame;

    /* ---- several devices: one band of rows each ---- */
    std::vector<int> devs;
    if (getenv("QR_DEVICES")) QR_TRY(device_list(devs));
    if (devs.size() > 1 && whole && !s->pt_on)
    {
        QR_TRY(replicas_prepare(c, s, devs));
        hipError_t e = hipSuccess;
        for (HostReplica &r : c.rep)
        {
            if (e != hipSuccess || (e = hipSetDevice(r.device)) != hipSuccess) break;
            LaunchP lp = s->lp;
            lp.B = (const char *)r.d_blob; lp.order = r.sched.d; lp.n_blocks = r.sched.n;
            lp.row_begin = r.y0; lp.row_end = r.y1; lp.stats = r.d_counters + 4;
            e = launch_lp<false>({ s->divk }, lp, (uint32_t *)r.d_frame, nullptr, r.d_counters, r.st);
            if (e != hipSuccess) break;
            e = band_send(dst, (const uint32_t *)r.d_frame, r.y0, r.y1, 0, 1, r.st);
            if (e == hipSuccess) e = hipEventRecord(r.ev, r.st);
        }
        for (HostReplica &r : c.rep)
            if (e == hipSuccess && (e = hipEventSynchronize(r.ev)) == hipSuccess) band_land(dst, r.y0, r.y1, 0, 1);
        (void)hipSetDevice(s->device);
        if (e != hipSuccess) return qr_fail(QR_ERR_DEVICE, std::string("render (QR_DEVICES): ") + hipGetErrorString(e));
        return QR_OK;
    }

    if (c.device != s->device)
    {
        if (c.d_frame.p) { (void)hipSetDevice(c.device); c.d_frame.release(); (void)hipSetDevice(s->device); }
        c.device = s->device;
    }
    HIP_TRY(c.d_frame.ensure(bytes));
    const uint32_t *const d_frame = c.d_frame.as<uint32_t>();
    hipError_t e = launch<false>(s, c.d_frame.p, nullptr, nullptr);
    if (e == hipSuccess && dst.pinned)
    {
        /* registered frame: the rows this call owns by DMA, straight into it */
        if (s->lp.group_stride == 1)
            e = band_send(dst, d_frame, s->lp.row_begin, s->lp.row_end, s->lp.index, s->lp.thnum, nullptr);
        else
            for (int g = s->lp.group_first; g * 8 < h && e == hipSuccess; g += s->lp.group_stride)
                e = band_send(dst, d_frame, g * 8, g * 8 + 8 < h ? g * 8 + 8 : h, s->lp.index, s->lp.thnum, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) return qr_fail(QR_ERR_DEVICE, std::string("render: ") + hipGetErrorString(e));
        return QR_OK;
    }
    if (e == hipSuccess && whole && row_pixels == w && h >= 64)
    {
        /* compact whole frame: the copy back runs in QR_COPY_CHUNKS row bands, the DMA of band k+1 under
         * the host memcpy of band k into the caller's frame */
        if (c.ev[0] == nullptr) for (int k = 0; k < QR_COPY_CHUNKS; k++) if (hipEventCreateWithFlags(&c.ev[k], hipEventDisableTiming) != hipSuccess) c.ev[k] = nullptr;
        bool ok = true;
        for (int k = 0; k < QR_COPY_CHUNKS; k++) ok = ok && c.ev[k] != nullptr;
        if (ok)
        {
            int y0[QR_COPY_CHUNKS + 1];
            for (int k = 0; k <= QR_COPY_CHUNKS; k++) y0[k] = (int)((long long)h * k / QR_COPY_CHUNKS);
            for (int k = 0; k < QR_COPY_CHUNKS && e == hipSuccess; k++)
            {
                e = band_send(dst, d_frame, y0[k], y0[k + 1], 0, 1, nullptr);
                if (e == hipSuccess) e = hipEventRecord(c.ev[k], nullptr);
            }
            for (int k = 0; k < QR_COPY_CHUNKS && e == hipSuccess; k++)
            {
                e = hipEventSynchronize(c.ev[k]);
                if (e == hipSuccess) band_land(dst, y0[k], y0[k + 1], 0, 1);
            }
            if (e != hipSuccess) return qr_fail(QR_ERR_DEVICE, std::string("render: ") + hipGetErrorString(e));
            return QR_OK;
        }
    }
    if (e == hipSuccess) e = hipMemcpy(h_frame, d_frame, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return qr_fail(QR_ERR_DEVICE, std::string("render: ") + hipGetErrorString(e));
    /* copy only the rows this call owns, honouring a negative stride (bottom-up
     * frames, engine.cpp:2814-2850) */
    if (whole && row_pixels == w) { memcpy(frame_host, h_frame, bytes); return QR_OK; }
    for (int y = s->lp.row_begin; y < s->lp.row_end; y++)
        if (sel_holds(sel_of(s->lp), y, 1, h)) memcpy(frame_host + (ptrdiff_t)y * row_pixels, h_frame + (size_t)y * w, (size_t)w * 4);
    return QR_OK;
}
