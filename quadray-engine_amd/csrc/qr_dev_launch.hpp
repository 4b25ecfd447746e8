/*
 * qr_dev_launch.hpp - which rows a launch renders, which schedule entries own them, which kernel instance runs them: the
 * frame launch of an uploaded scene, of its QR_DEVICES replicas, of qr_render0, and the multi-target launch.  Host code;
 * included by qr_device.hip after qr_device_scene.
 */

/* ---- row selection ---- */
/* the rows of a frame a launch renders: rows [row_begin, row_end) of the 8-row groups group_first, + group_stride, ... that
 * belong to index / thnum (qr_scene_set_rows, qr_scene_set_tile_rows); LaunchP carries the same six fields to the kernel */
struct RowSel { int32_t row_begin, row_end, group_first, group_stride, index, thnum; };

static RowSel sel_of(const LaunchP &lp) { return { lp.row_begin, lp.row_end, lp.group_first, lp.group_stride, lp.index, lp.thnum }; }
static RowSel sel_band(int y0, int y1) { return { y0, y1, 0, 1, 0, 1 }; }

static bool is_whole_frame(const LaunchP &lp, int H)
{
    return lp.row_begin == 0 && lp.row_end == H && lp.group_first == 0 && lp.group_stride == 1 && lp.thnum <= 1;
}

/* a schedule entry's first word: footprint column (bits 0-13) and row (14-27), heaviness (30-31) */
struct SchedWord { int bx, by, heavy; };
static SchedWord sched_decode(uint32_t w) { return { (int)(w & 0x3FFFu), (int)((w >> 14) & 0x3FFFu), (int)(w >> 30) }; }
/* rows of a footprint: 8 x 8 pixels, 8 x 4 of four samples each with anti-aliasing */
static int footprint_rows(int fsaa) { return fsaa == 0 ? 8 : 4; }

/* does the footprint whose first row is y0 hold a row of the selection?  An empty range holds none. */
static bool sel_holds(const RowSel &r, int y0, int fh, int H)
{
    for (int y = y0; y < y0 + fh && y < H; y++)
    {
        const int g = y >> 3;
        if (y >= r.row_begin && y < r.row_end && g >= r.group_first && (g - r.group_first) % r.group_stride == 0
            && (r.thnum <= 1 || (y % r.thnum) == r.index)) return true;
    }
    return false;
}

/* the entries of the scene's whole-frame schedule that own a selected row, in schedule order: emit(word0, word1) */
template <class F>
static void sched_select(const qr_device_scene *s, const RowSel &r, F emit)
{
    const int fh = footprint_rows(s->fr.fsaa), H = s->fr.frm_h;
    for (size_t i = 0; i + 1 < s->h_order.size(); i += 2)
        if (sel_holds(r, sched_decode(s->h_order[i]).by * fh, fh, H)) emit(s->h_order[i], s->h_order[i + 1]);
}

static std::vector<uint32_t> sched_subset(const qr_device_scene *s, const RowSel &r)
{
    std::vector<uint32_t> keep;
    sched_select(s, r, [&](uint32_t a, uint32_t b) { keep.push_back(a); keep.push_back(b); });
    return keep;
}

/* a cache of schedule subsets is full: a subset may still be in use by queued launches, so wait before recycling the buffers */
template <class M>
static void sched_cache_trim(M &cache, size_t limit)
{
    if (cache.size() < limit) return;
    (void)hipDeviceSynchronize();
    for (auto &kv : cache) kv.second.release();
    cache.clear();
}

/* ---- kernel instance and launch ---- */
static int env_tristate(const char *name) { const char *v = getenv(name); return v ? (atoi(v) != 0 ? 1 : 0) : -1; }

/* the kernel instance with the per-lane walk: when some list is a long hierarchy, or QR_DIV=0 / 1 (`forced`, -1 unset) says
 * so (experiments, tests); only that instance knows shadow grids */
static bool pick_divk(int forced, const QrProgram &prog) { return (forced >= 0 ? forced != 0 : prog.has_long_lists) || prog.has_grids; }

/* register budget variant of the plain instance (waves per SIMD); QR_WAVES is a tuning knob for experiments */
static int plain_waves()
{
    static const int waves = []() { const char *e = getenv("QR_WAVES"); int w = e ? atoi(e) : QR_MIN_WAVES_PER_SIMD;
                                    return (w == 3 || w == 4 || w == 5) ? w : QR_MIN_WAVES_PER_SIMD; }();
    return waves;
}
struct Instance { bool divk; int waves = QR_MIN_WAVES_PER_SIMD; };

static dim3 wave_grid(int32_t n_waves) { return dim3((unsigned)((n_waves + (QR_BLOCK / 64) - 1) / (QR_BLOCK / 64)), 1, 1); }

/* launch parameters a frame record asks for: the whole frame, the caller's index / thnum */
static LaunchP launchp_of(const qr_frame &frm)
{
    LaunchP lp = {};
    lp.depth = frm.depth > QR_MAX_DEPTH ? QR_MAX_DEPTH : frm.depth;
    lp.row_begin = 0; lp.row_end = frm.frm_h;
    lp.index = frm.index; lp.thnum = frm.thnum > 0 ? frm.thnum : 1;
    lp.group_first = 0; lp.group_stride = 1;
    return lp;
}

/* THE frame launch: lp.n_blocks waves of the schedule lp.order, with the path-tracer kernel when `pt` is given */
template <bool COUNT>
static hipError_t launch_lp(Instance k, const LaunchP &lp, uint32_t *f, int32_t *ids, unsigned long long *counters, hipStream_t st,
                            const PtParams *pt = nullptr)
{
    if (lp.n_blocks <= 0) return hipSuccess;
    const dim3 grid = wave_grid(lp.n_blocks), block(QR_BLOCK);
    (void)k.waves;
    if (pt) hipLaunchKernelGGL(qr_render_pt_kernel, grid, block, 0, st, lp, *pt, f, counters);
    else if (k.divk) hipLaunchKernelGGL((qr_render_kernel<COUNT, QR_DIVK_WAVES, true>), grid, block, 0, st, lp, f, ids, counters);
#ifdef QR_WAVE_VARIANTS
    else if (!COUNT && k.waves == 3) hipLaunchKernelGGL((qr_render_kernel<false, 3, false>), grid, block, 0, st, lp, f, ids, counters);
    else if (!COUNT && k.waves == 5) hipLaunchKernelGGL((qr_render_kernel<false, 5, false>), grid, block, 0, st, lp, f, ids, counters);
#endif
    else hipLaunchKernelGGL((qr_render_kernel<COUNT, 4, false>), grid, block, 0, st, lp, f, ids, counters);
    return hipGetLastError();
}

/* an uploaded scene's launch with its current row selection: a launch restricted by qr_scene_set_rows / _set_tile_rows only
 * starts the waves that own pixels */
template <bool COUNT>
static hipError_t launch(qr_device_scene *s, void *frame_dev, int32_t *ids_dev, hipStream_t st)
{
    if (s->n_groups == 0) return hipSuccess;
    LaunchP lp = s->lp;
    if (!is_whole_frame(lp, s->fr.frm_h))
    {
        const RowSel r = sel_of(lp);
        const std::array<int32_t, 6> key = { r.row_begin, r.row_end, r.group_first, r.group_stride, r.index, r.thnum };
        auto it = s->sub.find(key);
        if (it == s->sub.end())
        {
            /* first launch with this selection */
            const std::vector<uint32_t> keep = sched_subset(s, r);
            sched_cache_trim(s->sub, 256);
            SchedBuf sb;
            const hipError_t e = sb.upload(keep, 2);
            if (e != hipSuccess) return e;
            it = s->sub.emplace(key, sb).first;
        }
        lp.order = it->second.d;
        lp.n_blocks = it->second.n;
    }
    if (lp.n_blocks <= 0) return hipSuccess;
    if (!s->pt_on) return launch_lp<COUNT>({ s->divk, plain_waves() }, lp, (uint32_t *)frame_dev, ids_dev, s->d_counters, st);
    /* one more sample of every pixel sample: weights of the running mean, tracer.cpp:1112-1136 */
    if (COUNT || ids_dev != nullptr) return hipErrorInvalidValue;
    s->pt_frames++;
    PtParams pt;
    const size_t n = (size_t)s->fr.frm_row * s->fr.frm_h * ((size_t)1 << s->fr.fsaa);
    pt.seeds = s->d_seeds; pt.acc_r = s->d_acc; pt.acc_g = s->d_acc + n; pt.acc_b = s->d_acc + 2 * n;
    pt.pts_o = 1.0f / (float)s->pt_frames; pt.pts_u = 1.0f - pt.pts_o;
    pt.eager = s->pt_eager; pt.pad = 0;
    return launch_lp<false>({ s->divk }, lp, (uint32_t *)frame_dev, nullptr, s->d_counters, st, &pt);
}

/* A path-traced frame is ONE more sample of every pixel sample: the sample count (and with it the weights of the running
 * mean, tracer.cpp:1112-1136) advances once per launch, so a frame cut into several row-range launches would weigh its
 * later ranges wrongly.  Such launches are refused; the drop-in entry point, where the engine itself cuts a frame into
 * index / thnum slices, takes the count from the caller's s_inf instead (dropin_pt_begin). */
static int pt_rows_ok(const qr_device_scene *s)
{
    if (s->pt_on && !is_whole_frame(s->lp, s->fr.frm_h))
        return qr_fail(QR_ERR_UNSUP, "path-tracer mode renders whole frames only: reset qr_scene_set_rows / qr_scene_set_tile_rows to the full frame");
    return QR_OK;
}

/* ---- the multi-target launch ---- */
/* combined schedules of multi-target launches, keyed by (scene, row range) per target; only the schedule is
 * cached -- recursion depth and frame pointers travel in the kernel arguments of every launch.  qr_scene_destroy drops the
 * entries of its scene (multi_forget): a later scene may get the same address */
static std::map<std::vector<int64_t>, SchedBuf> g_multi;
static std::mutex g_multi_lock;

static void multi_forget(const qr_device_scene *s)
{
    std::lock_guard<std::mutex> lk(g_multi_lock);
    for (auto it = g_multi.begin(); it != g_multi.end(); )
    {
        bool uses = false;
        for (size_t i = 0; i < it->first.size(); i += 3) if (it->first[i] == (int64_t)(intptr_t)s) uses = true;
        if (uses) { it->second.release(); it = g_multi.erase(it); }
        else ++it;
    }
}

extern "C" int qr_render_multi_async(int n, qr_device_scene *const *scenes, void *const *frames_dev,
                                     const int *row_begin, const int *row_end, void *stream)
{
    if (n <= 0 || scenes == nullptr || frames_dev == nullptr || row_begin == nullptr || row_end == nullptr)
        return qr_fail(QR_ERR_ARG, "bad argument");
    bool direct = n <= QR_MAX_TARGETS;
    for (int i = 0; i < n; i++)
    {
        if (scenes[i] == nullptr || frames_dev[i] == nullptr) return qr_fail(QR_ERR_ARG, "null scene or frame");
        if (scenes[i]->pt_on) return qr_fail(QR_ERR_UNSUP, "a scene in path-tracer mode cannot be part of a multi-target launch");
        if (scenes[i]->device != scenes[0]->device) return qr_fail(QR_ERR_ARG, "scenes live on different devices");
        if (row_begin[i] < 0 || row_end[i] > scenes[i]->fr.frm_h || row_begin[i] > row_end[i]) return qr_fail(QR_ERR_ARG, "bad row range");
    }
#ifdef QR_WAVETIME
    direct = false;
#endif
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(scenes[0]->device));
    if (!direct)
    {
        /* no combined kernel for this set: one launch per target */
        for (int i = 0; i < n; i++)
        {
            qr_device_scene *s = scenes[i];
            const LaunchP keep = s->lp; const int32_t keep_groups = s->n_groups;
            int rc = qr_scene_set_rows(s, row_begin[i], row_end[i], 0, 1);
            if (rc == QR_OK) { hipError_t e = launch<false>(s, frames_dev[i], nullptr, st); if (e != hipSuccess) rc = qr_fail(QR_ERR_DEVICE, hipGetErrorString(e)); }
            s->lp = keep; s->n_groups = keep_groups;
            QR_TRY(rc);
        }
        return QR_OK;
    }
    std::vector<int64_t> key;
    for (int i = 0; i < n; i++) { key.push_back((int64_t)(intptr_t)scenes[i]); key.push_back(row_begin[i]); key.push_back(row_end[i]); }
    SchedBuf ms;
    {
        std::lock_guard<std::mutex> lk(g_multi_lock);
        auto it = g_multi.find(key);
        if (it == g_multi.end())
        {
            std::vector<uint32_t> ent[4];                    /* by heaviness, heaviest first; entries of 4 words */
            for (int i = 0; i < n; i++)
                sched_select(scenes[i], sel_band(row_begin[i], row_end[i]), [&](uint32_t a, uint32_t b) {
                    std::vector<uint32_t> &v = ent[3 - sched_decode(a).heavy];
                    v.push_back(a); v.push_back(b); v.push_back((uint32_t)i); v.push_back(0u); });
            std::vector<uint32_t> all;
            for (int h = 0; h < 4; h++) all.insert(all.end(), ent[h].begin(), ent[h].end());
            sched_cache_trim(g_multi, 64);
            SchedBuf m;
            HIP_TRY(m.upload(all, 4));
            it = g_multi.emplace(key, m).first;
        }
        ms = it->second;
    }
    if (ms.n == 0) return QR_OK;
    DevTargets tg;
    memset(&tg, 0, sizeof(tg));
    bool divk = false;
    for (int i = 0; i < n; i++)
    {
        tg.t[i].frame = (uint32_t *)frames_dev[i];
        tg.t[i].B = scenes[i]->lp.B;
        tg.t[i].row_begin = row_begin[i]; tg.t[i].row_end = row_end[i];
        tg.t[i].depth = scenes[i]->lp.depth;
        divk = divk || scenes[i]->divk;
    }
    const dim3 grid = wave_grid(ms.n), block(QR_BLOCK);
    if (divk) hipLaunchKernelGGL((qr_render_multi_kernel<QR_DIVK_WAVES, true>), grid, block, 0, st, tg, (const uint32_t *)ms.d, ms.n, scenes[0]->d_counters);
    else      hipLaunchKernelGGL((qr_render_multi_kernel<QR_MIN_WAVES_PER_SIMD, false>), grid, block, 0, st, tg, (const uint32_t *)ms.d, ms.n, scenes[0]->d_counters);
    HIP_TRY(hipGetLastError());
    return QR_OK;
}
