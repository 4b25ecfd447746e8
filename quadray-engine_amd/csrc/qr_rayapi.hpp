/*
 * qr_rayapi.hpp - host glue of the ray API (include/qrhip.h): ray queries, shading, views, path-traced rays and views,
 * the a-trous filter, temporal reprojection, open lists, hit records, fans, gather fans and hit layers.  Included by qr_device.hip (one
 * translation unit) after qr_device_scene, HIP_TRY, QR_TRY, need_scene and pt_seed_plane.
 *
 * Every check, grid and kernel choice is stated once, below; an entry point composes these in the order of its own
 * refusals and adds only what is its own.  That order is part of the interface (tests/test_api_refusals.py).
 */

/* ---- checks: each refusal and its message ---- */

/* what: "ray" or "record", as in "ray count must be 0..INT32_MAX" */
static int count_arg(int64_t n, const char *what)
{
    if (n < 0 || n > (int64_t)INT32_MAX) return qr_fail(QR_ERR_ARG, std::string(what) + " count must be 0..INT32_MAX");
    return QR_OK;
}

static int flags_arg(uint32_t flags, uint32_t allowed, const char *msg)
{
    if (flags & ~allowed) return qr_fail(QR_ERR_ARG, msg);
    return QR_OK;
}

static int view_size_args(int n_views, int width, int height)
{
    if (n_views < 0 || n_views > QR_VIEW_MAX_VIEWS) return qr_fail(QR_ERR_ARG, "view count must be 0.." + std::to_string(QR_VIEW_MAX_VIEWS));
    if (width < 1 || height < 1 || width > QR_VIEW_MAX_DIM || height > QR_VIEW_MAX_DIM)
        return qr_fail(QR_ERR_ARG, "view frame size must be 1.." + std::to_string(QR_VIEW_MAX_DIM) + " in each dimension");
    return QR_OK;
}

/* the footprints of one wave (the frame's FSAA) that cover a width x height frame */
struct Footprints { int64_t cols, rows; };
static Footprints footprints(const qr_device_scene *s, int width, int height)
{
    const int fsaa = s->fr.fsaa;
    const int fw = fsaa == 2 ? 4 : 8, fh = fsaa == 0 ? 8 : 4;
    return { (width + fw - 1) / fw, (height + fh - 1) / fh };
}

/* views x footprints fit one grid.  Every launch over views holds to it, the one-lane-per-pixel ones too (so that a size
 * one of them takes is taken by all), except qr_render_views_mean_async: its grid is the footprints of ONE frame whatever
 * n_views is, at most 4096 x 4096 workgroups (QR_VIEW_MAX_DIM), so it takes view counts this limit refuses. */
static int view_grid_arg(const qr_device_scene *s, int n_views, int width, int height)
{
    const Footprints f = footprints(s, width, height);
    if ((int64_t)n_views * f.cols * f.rows > (int64_t)QR_VIEW_MAX_WAVES)
        return qr_fail(QR_ERR_ARG, "views x footprints exceed one grid (QR_VIEW_MAX_WAVES)");
    return QR_OK;
}

static int need_query_list(const qr_device_scene *s)
{
    if (s->off_query == 0) return qr_fail(QR_ERR_UNSUP, "scene was uploaded without QR_UPLOAD_RAY_QUERIES: it holds no ray-query list");
    return QR_OK;
}

/* why: what the scene's path-tracer state cannot give this call */
static int no_pt_mode(const qr_device_scene *s, const char *why)
{
    if (s->pt_on) return qr_fail(QR_ERR_UNSUP, std::string("scene is in path-tracer mode: ") + why);
    return QR_OK;
}

static int samples_arg(int samples, int most)
{
    if (samples < 1 || samples > most) return qr_fail(QR_ERR_ARG, "samples must be 1.." + std::to_string(most));
    return QR_OK;
}

static int done_arg(int done, int samples)
{
    if (done < 0 || (int64_t)done + (int64_t)samples >= ((int64_t)1 << 24))
        return qr_fail(QR_ERR_ARG, "done must be 0 or more and done + samples below 2^24 (the sample number is exact in fp32)");
    return QR_OK;
}

/* the adaptive stop rule's parameters */
static int rule_args(int min_samples, int max_samples, float tol2)
{
    if (min_samples < 0 || max_samples < 1 || min_samples > max_samples || max_samples >= (1 << 24))
        return qr_fail(QR_ERR_ARG, "min_samples and max_samples must be 0 <= min_samples <= max_samples, 1 <= max_samples < 2^24 (the count is exact in fp32)");
    if (!(tol2 >= 0.0f) || tol2 > FLT_MAX) return qr_fail(QR_ERR_ARG, "tol2 must be a finite number, 0 or more");
    return QR_OK;
}

/* pointers: every one of `ps` is there / aligned (a null pointer is aligned: the optional ones go in as they are) */
static int need_ptrs(std::initializer_list<const void *> ps)
{
    for (const void *p : ps) if (p == nullptr) return qr_fail(QR_ERR_ARG, "null argument");
    return QR_OK;
}

static int aligned_ptrs(std::initializer_list<const void *> ps, unsigned align, const char *msg)
{
    uintptr_t bits = 0;
    for (const void *p : ps) bits |= (uintptr_t)p;
    if ((bits & (align - 1u)) != 0) return qr_fail(QR_ERR_ARG, msg);
    return QR_OK;
}

/* the 16-byte pointers of a call, then its 4-byte ones, each list with its own message */
static int aligned_16_and_4(std::initializer_list<const void *> wide, const char *wide_msg,
                            std::initializer_list<const void *> words, const char *words_msg)
{
    QR_TRY(aligned_ptrs(wide, 16, wide_msg));
    return aligned_ptrs(words, 4, words_msg);
}

/* the image filters' parameter blocks (a-trous, upsampling, reprojection): msg names the block */
static int need_params(const void *p, const char *msg)
{
    if (p == nullptr) return qr_fail(QR_ERR_ARG, msg);
    return QR_OK;
}

static int channels_arg(int channels)
{
    if (channels != 3 && channels != 4) return qr_fail(QR_ERR_ARG, "channels must be 3 or 4");
    return QR_OK;
}

static int normal_sq_arg(int normal_sq)
{
    if (normal_sq < 0 || normal_sq > 7) return qr_fail(QR_ERR_ARG, "normal_sq must be 0..7");
    return QR_OK;
}

/* two optional arguments that go together */
static int both_or_neither(bool a, bool b, const char *msg)
{
    if (a != b) return qr_fail(QR_ERR_ARG, msg);
    return QR_OK;
}

static int put_bytes(uint64_t *bytes_out, uint64_t bytes)
{
    if (bytes_out == nullptr) return qr_fail(QR_ERR_ARG, "null argument");
    *bytes_out = bytes;
    return QR_OK;
}

/* ---- grids and parameter blocks ---- */

static dim3 ray_grid(int64_t n) { return dim3((unsigned)((n + QR_BLOCK - 1) / QR_BLOCK)); }

/* one lane per pixel: 8x8 footprints at every FSAA (never more workgroups than view_grid_arg allows) */
static dim3 pixel_grid(int width, int height, int n_views)
{
    return dim3((unsigned)((width + 7) / 8), (unsigned)((height + 7) / 8), (unsigned)n_views);
}

/* one wave per footprint of every view */
static dim3 footprint_grid(const qr_device_scene *s, int width, int height, int n_views)
{
    const Footprints f = footprints(s, width, height);
    return dim3((unsigned)f.cols, (unsigned)f.rows, (unsigned)n_views);
}

/* one lane per pixel in tw x th pixel tiles, blockIdx.z the view: 32 x 8 tiles give grid.x <= 512, grid.y <= 2048 at QR_VIEW_MAX_DIM */
static dim3 tile_grid(int width, int height, int n_views, int tw, int th)
{
    return dim3((unsigned)((width + tw - 1) / tw), (unsigned)((height + th - 1) / th), (unsigned)n_views);
}

static ViewsP views_params(const qr_view *views, int width, int height, float *depth = nullptr)
{
    ViewsP vp;
    vp.views = views; vp.width = width; vp.height = height; vp.depth = depth;
    return vp;
}

static PtRaysP pt_rays_params(const qr_ray *rays, const qr_ray_spread *spread, int64_t n, float *rgb)
{
    PtRaysP pr;
    pr.rays = (const f32x4 *)rays; pr.spread = (const f32x4 *)spread; pr.n = (int32_t)n; pr.pad = 0; pr.rgb = rgb;
    return pr;
}

static int launched()
{
    HIP_TRY(hipGetLastError());
    return QR_OK;
}

/* ---- kernel choice: a run-time flag as a compile-time constant, so that a launch is written once ---- */

/* f(std::true_type) or f(std::false_type): decltype(c)::value goes among the kernel's template arguments */
template <class F> static void pick(bool flag, F &&f)
{
    if (flag) f(std::true_type{}); else f(std::false_type{});
}

/* f(std::integral_constant<int, 3>) or <int, 4>: the channels of a filtered frame, checked by channels_arg */
template <class F> static void pick_channels(int channels, F &&f)
{
    pick(channels == 3, [&](auto three) { f(std::integral_constant<int, decltype(three)::value ? 3 : 4>{}); });
}

/* The instance of a launch over views, chosen as the frame launch chooses its own: per-lane walks only where some list
 * is a long hierarchy or carries a grid, and with them that instance's register budget -- the two move together. */
template <bool DIVK> struct Walk
{
    static constexpr bool divk = DIVK;
    static constexpr int waves = DIVK ? QR_DIVK_WAVES : QR_MIN_WAVES_PER_SIMD;
};
template <class F> static void pick_walk(const qr_device_scene *s, F &&f)
{
    if (s->divk) f(Walk<true>{}); else f(Walk<false>{});
}

/* ---- ray queries (qr_query.hpp) ---- */

static int query_args(const qr_device_scene *s, const qr_ray *rays, int64_t n, const void *out0, const void *out1, uint32_t flags)
{
    QR_TRY(need_scene(s));
    QR_TRY(count_arg(n, "ray"));
    QR_TRY(flags_arg(flags, QR_TRACE_COHERENT, "unknown query flags"));
    QR_TRY(need_query_list(s));
    if (n == 0) return QR_OK;
    QR_TRY(need_ptrs({rays, out0, out1}));
    return aligned_ptrs({rays}, 16, "rays must be 16-byte aligned");
}

extern "C" int qr_trace_rays_async(qr_device_scene *s, const qr_ray *rays_dev, int64_t n,
                                   float *t_out_dev, int32_t *id_out_dev, uint32_t flags, void *stream)
{
    QR_TRY(query_args(s, rays_dev, n, t_out_dev, id_out_dev, flags));
    if (n == 0) return QR_OK;
    HIP_TRY(hipSetDevice(s->device));
    pick(flags & QR_TRACE_COHERENT, [&](auto coherent) {
        hipLaunchKernelGGL((qr_trace_kernel<false, decltype(coherent)::value>), ray_grid(n), dim3(QR_BLOCK), 0, (hipStream_t)stream,
                           (const char *)s->d_blob, (const f32x4 *)rays_dev, (int32_t)n, t_out_dev, id_out_dev, (uint8_t *)nullptr,
                           s->lp.stats);
    });
    return launched();
}

extern "C" int qr_occluded_async(qr_device_scene *s, const qr_ray *rays_dev, int64_t n,
                                 uint8_t *occ_out_dev, uint32_t flags, void *stream)
{
    QR_TRY(query_args(s, rays_dev, n, occ_out_dev, occ_out_dev, flags));
    if (n == 0) return QR_OK;
    HIP_TRY(hipSetDevice(s->device));
    pick(flags & QR_TRACE_COHERENT, [&](auto coherent) {
        hipLaunchKernelGGL((qr_trace_kernel<true, decltype(coherent)::value>), ray_grid(n), dim3(QR_BLOCK), 0, (hipStream_t)stream,
                           (const char *)s->d_blob, (const f32x4 *)rays_dev, (int32_t)n, (float *)nullptr, (int32_t *)nullptr,
                           occ_out_dev, s->lp.stats);
    });
    return launched();
}

/* ray shading (qr_kernel.hpp qr_shade_rays_kernel): the renderer's colour for caller rays, at the scene's current depth */
extern "C" int qr_shade_rays_async(qr_device_scene *s, const qr_ray *rays_dev, int64_t n,
                                   float *rgb_out_dev, int32_t *id_out_dev, uint32_t flags, void *stream)
{
    QR_TRY(query_args(s, rays_dev, n, rgb_out_dev, rgb_out_dev, flags));
    QR_TRY(no_pt_mode(s, "caller rays carry no sample seeds"));
    if (n == 0) return QR_OK;
    HIP_TRY(hipSetDevice(s->device));
    RaysP rp;
    rp.rays = (const f32x4 *)rays_dev; rp.n = (int32_t)n; rp.pad = 0; rp.rgb = rgb_out_dev;
    pick(flags & QR_TRACE_COHERENT, [&](auto coherent) {
        hipLaunchKernelGGL((qr_shade_rays_kernel<decltype(coherent)::value>), ray_grid(n), dim3(QR_BLOCK), 0, (hipStream_t)stream,
                           s->lp, rp, id_out_dev);
    });
    return launched();
}

/* ---- views (qr_kernel.hpp qr_render_views_kernel, qr_views_mean_kernel): frames from caller cameras, at the scene's depth ---- */

static const char *const VIEWS_NO_PT = "its seeds and colour planes belong to the snapshot's frame";

extern "C" int qr_render_views_async(qr_device_scene *s, const qr_view *views_dev, int n_views, int width, int height,
                                     uint32_t *frames_dev, int32_t *ids_dev, float *depth_dev, uint32_t flags, void *stream)
{
    QR_TRY(need_scene(s));
    QR_TRY(view_size_args(n_views, width, height));
    QR_TRY(flags_arg(flags, 0u, "unknown view flags"));
    QR_TRY(need_query_list(s));
    QR_TRY(no_pt_mode(s, VIEWS_NO_PT));
    QR_TRY(view_grid_arg(s, n_views, width, height));
    if (n_views == 0) return QR_OK;
    QR_TRY(need_ptrs({views_dev, frames_dev}));
    QR_TRY(aligned_ptrs({views_dev}, 16, "views must be 16-byte aligned"));
    QR_TRY(aligned_ptrs({frames_dev, ids_dev, depth_dev}, 4, "frames, ids and depth must be 4-byte aligned"));
    HIP_TRY(hipSetDevice(s->device));
    const ViewsP vp = views_params(views_dev, width, height, depth_dev);
    pick_walk(s, [&](auto w) {
        hipLaunchKernelGGL((qr_render_views_kernel<decltype(w)::divk, decltype(w)::waves>), footprint_grid(s, width, height, n_views),
                           dim3(QR_BLOCK), 0, (hipStream_t)stream, s->lp, vp, frames_dev, ids_dev);
    });
    return launched();
}

/* the sum and the mean frame of many views of one frame, in one launch */
extern "C" int qr_render_views_mean_async(qr_device_scene *s, const qr_view *views_dev, int n_views, int width, int height,
                                          float *sum_dev, uint32_t *frame_dev, float scale, uint32_t flags, void *stream)
{
    QR_TRY(need_scene(s));
    QR_TRY(view_size_args(n_views, width, height));
    QR_TRY(flags_arg(flags, QR_MEAN_RESUME, "unknown view accumulation flags"));
    if (frame_dev != nullptr && !(std::isfinite(scale) && scale > 0.0f))
        return qr_fail(QR_ERR_ARG, "scale must be finite and greater than 0 when a frame is wanted");
    QR_TRY(need_query_list(s));
    QR_TRY(no_pt_mode(s, VIEWS_NO_PT));
    if (n_views == 0) return QR_OK;
    QR_TRY(need_ptrs({views_dev, sum_dev}));
    QR_TRY(aligned_ptrs({views_dev}, 16, "views must be 16-byte aligned"));
    QR_TRY(aligned_ptrs({sum_dev, frame_dev}, 4, "sum and frame must be 4-byte aligned"));
    HIP_TRY(hipSetDevice(s->device));
    const ViewsP vp = views_params(views_dev, width, height);
    const uint32_t resume = flags & QR_MEAN_RESUME;
    if (frame_dev == nullptr) scale = 1.0f;
    pick_walk(s, [&](auto w) {      /* the footprints of the ONE frame: no view_grid_arg above */
        hipLaunchKernelGGL((qr_views_mean_kernel<decltype(w)::divk, decltype(w)::waves>), footprint_grid(s, width, height, 1),
                           dim3(QR_BLOCK), 0, (hipStream_t)stream, s->lp, vp, n_views, sum_dev, frame_dev, scale, resume);
    });
    return launched();
}

/* ---- path-traced views (qr_kernel.hpp qr_pt_views_kernel): progressive frames from caller cameras, state in the caller's memory ---- */

/* the checks every entry point of the feature shares: sizes and the view launch's limits; *slots: words of one plane of one view */
static int pt_views_dims(const qr_device_scene *s, int n_views, int width, int height, uint64_t *slots)
{
    QR_TRY(need_scene(s));
    QR_TRY(view_size_args(n_views, width, height));
    QR_TRY(view_grid_arg(s, n_views, width, height));
    *slots = ((uint64_t)width * (uint64_t)height) << s->fr.fsaa;
    if ((uint64_t)n_views * *slots > ((uint64_t)1 << 30))
        return qr_fail(QR_ERR_ARG, "more than 2^30 pixel samples of path-tracer state in one launch");
    return QR_OK;
}

/* the seed plane of qr_scene_set_pt in plane 0 of every view, the other words - 1 planes 0: synchronous, as qr_scene_set_pt is */
static int pt_views_state_reset(const qr_device_scene *s, int n_views, uint64_t slots, void *state_dev, int words)
{
    if (n_views == 0) return QR_OK;
    QR_TRY(need_ptrs({state_dev}));
    QR_TRY(aligned_ptrs({state_dev}, 4, "state must be 4-byte aligned"));
    HIP_TRY(hipSetDevice(s->device));
    const std::vector<uint32_t> seeds = pt_seed_plane(slots);
    HIP_TRY(hipDeviceSynchronize());
    uint32_t *st = (uint32_t *)state_dev;
    for (int v = 0; v < n_views; v++, st += words * slots)
    {
        HIP_TRY(hipMemcpy(st, seeds.data(), slots * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(st + slots, 0, (words - 1) * slots * sizeof(uint32_t)));
    }
    HIP_TRY(hipDeviceSynchronize());
    return QR_OK;
}

extern "C" int qr_pt_views_state_bytes(qr_device_scene *s, int n_views, int width, int height, uint64_t *bytes_out)
{
    uint64_t slots = 0;
    QR_TRY(pt_views_dims(s, n_views, width, height, &slots));
    return put_bytes(bytes_out, (uint64_t)n_views * QR_PT_VIEWS_STATE_WORDS * slots * sizeof(uint32_t));
}

extern "C" int qr_pt_views_reset(qr_device_scene *s, int n_views, int width, int height, void *state_dev)
{
    uint64_t slots = 0;
    QR_TRY(pt_views_dims(s, n_views, width, height, &slots));
    return pt_views_state_reset(s, n_views, slots, state_dev, QR_PT_VIEWS_STATE_WORDS);
}

extern "C" int qr_pt_views_async(qr_device_scene *s, const qr_view *views_dev, int n_views, int width, int height,
                                 void *state_dev, int done, int samples, uint32_t *frames_dev, float *mean_dev,
                                 uint32_t flags, void *stream)
{
    uint64_t slots = 0;
    QR_TRY(pt_views_dims(s, n_views, width, height, &slots));
    QR_TRY(flags_arg(flags, 0u, "unknown path-traced view flags"));
    QR_TRY(samples_arg(samples, QR_PT_VIEWS_MAX_SAMPLES));
    QR_TRY(done_arg(done, samples));
    QR_TRY(need_query_list(s));
    if (n_views == 0) return QR_OK;
    QR_TRY(need_ptrs({views_dev, state_dev, frames_dev}));
    QR_TRY(aligned_ptrs({views_dev}, 16, "views must be 16-byte aligned"));
    QR_TRY(aligned_ptrs({state_dev, frames_dev, mean_dev}, 4, "state, frames and mean must be 4-byte aligned"));
    HIP_TRY(hipSetDevice(s->device));
    const ViewsP vp = views_params(views_dev, width, height);
    PtViewsP pv;
    pv.state = (uint32_t *)state_dev; pv.done = done; pv.samples = samples; pv.mean = mean_dev;
    /* one instance, as the scene's own path tracer has one: the packet walks (shade<..., PT> exists for them alone) */
    hipLaunchKernelGGL(qr_pt_views_kernel, footprint_grid(s, width, height, n_views), dim3(QR_BLOCK), 0, (hipStream_t)stream,
                       s->lp, vp, pv, frames_dev);
    return launched();
}

/* ---- path-traced rays (qr_kernel.hpp qr_pt_rays_kernel): progressive samples for caller rays, state in the caller's memory ---- */

/* the checks every entry point of the feature shares */
static int pt_rays_dims(const qr_device_scene *s, int64_t n)
{
    QR_TRY(need_scene(s));
    return count_arg(n, "ray");
}

extern "C" int qr_pt_rays_state_bytes(qr_device_scene *s, int64_t n, uint64_t *bytes_out)
{
    QR_TRY(pt_rays_dims(s, n));
    return put_bytes(bytes_out, (uint64_t)n * QR_PT_RAYS_STATE_WORDS * sizeof(uint32_t));
}

/* the seeds of slots 0 .. n - 1 of qr_scene_set_pt's plane, running means 0: synchronous */
extern "C" int qr_pt_rays_reset(qr_device_scene *s, int64_t n, void *state_dev)
{
    QR_TRY(pt_rays_dims(s, n));
    if (n == 0) return QR_OK;
    QR_TRY(need_ptrs({state_dev}));
    QR_TRY(aligned_ptrs({state_dev}, 4, "state must be 4-byte aligned"));
    HIP_TRY(hipSetDevice(s->device));
    const std::vector<uint32_t> seeds = pt_seed_plane((size_t)n);
    HIP_TRY(hipDeviceSynchronize());
    uint32_t *st = (uint32_t *)state_dev;
    HIP_TRY(hipMemcpy(st, seeds.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(st + n, 0, 3 * (size_t)n * sizeof(uint32_t)));
    HIP_TRY(hipDeviceSynchronize());
    return QR_OK;
}

/* ... and once there are rays: what the launches over path-traced rays ask of rays and spread */
static int pt_rays_ptrs(std::initializer_list<const void *> needed, const qr_ray *rays, const qr_ray_spread *spread)
{
    QR_TRY(need_ptrs(needed));
    return aligned_ptrs({rays, spread}, 16, "rays and spread must be 16-byte aligned");
}

extern "C" int qr_pt_rays_async(qr_device_scene *s, const qr_ray *rays_dev, const qr_ray_spread *spread_dev, int64_t n,
                                void *state_dev, int done, int samples, float *rgb_dev, uint32_t flags, void *stream)
{
    QR_TRY(pt_rays_dims(s, n));
    QR_TRY(flags_arg(flags, 0u, "unknown path-traced ray flags"));
    QR_TRY(samples_arg(samples, QR_PT_RAYS_MAX_SAMPLES));
    QR_TRY(done_arg(done, samples));
    QR_TRY(need_query_list(s));
    if (n == 0) return QR_OK;
    QR_TRY(pt_rays_ptrs({rays_dev, state_dev}, rays_dev, spread_dev));
    QR_TRY(aligned_ptrs({state_dev, rgb_dev}, 4, "state and rgb must be 4-byte aligned"));
    HIP_TRY(hipSetDevice(s->device));
    const PtRaysP pr = pt_rays_params(rays_dev, spread_dev, n, rgb_dev);
    /* one instance, as the scene's own path tracer has one: the packet walks (shade<..., PT> exists for them alone); rays are
     * never taken as neighbours */
    hipLaunchKernelGGL(qr_pt_rays_kernel, ray_grid(n), dim3(QR_BLOCK), 0, (hipStream_t)stream, s->lp, pr, (uint32_t *)state_dev,
                       done, samples);
    return launched();
}

/* ---- adaptive path-traced rays (qr_kernel.hpp qr_pt_adapt_kernel): per-ray counts, Welford's M2 and a stop rule on chip ---- */

extern "C" int qr_pt_adapt_state_bytes(qr_device_scene *s, int64_t n, uint64_t *bytes_out)
{
    QR_TRY(pt_rays_dims(s, n));
    return put_bytes(bytes_out, (uint64_t)n * QR_PT_ADAPT_STATE_WORDS * sizeof(uint32_t));
}

/* plane 0 as qr_pt_rays_reset writes it, every other plane 0: synchronous */
extern "C" int qr_pt_adapt_reset(qr_device_scene *s, int64_t n, void *state_dev)
{
    QR_TRY(qr_pt_rays_reset(s, n, state_dev));
    if (n == 0) return QR_OK;
    HIP_TRY(hipMemset((uint32_t *)state_dev + QR_PT_RAYS_STATE_WORDS * (size_t)n, 0,
                      (QR_PT_ADAPT_STATE_WORDS - QR_PT_RAYS_STATE_WORDS) * (size_t)n * sizeof(uint32_t)));
    HIP_TRY(hipDeviceSynchronize());
    return QR_OK;
}

/* the checks the adaptive launches share, in the order their refusals are documented: scene and count, flags, samples (the open
 * list has none: it passes 1), the rule's parameters, the ray-query list */
static int pt_adapt_args(const qr_device_scene *s, int64_t n, int samples, int min_samples, int max_samples, float tol2, uint32_t flags)
{
    QR_TRY(pt_rays_dims(s, n));
    QR_TRY(flags_arg(flags, 0u, "unknown adaptive path-traced ray flags"));
    QR_TRY(samples_arg(samples, QR_PT_ADAPT_MAX_SAMPLES));
    QR_TRY(rule_args(min_samples, max_samples, tol2));
    return need_query_list(s);
}

extern "C" int qr_pt_adapt_rays_async(qr_device_scene *s, const qr_ray *rays_dev, const qr_ray_spread *spread_dev, int64_t n,
                                      void *state_dev, int samples, int min_samples, int max_samples, float tol2,
                                      float *rgb_dev, uint32_t *open_dev, uint32_t flags, void *stream)
{
    QR_TRY(pt_adapt_args(s, n, samples, min_samples, max_samples, tol2, flags));
    if (n == 0) return QR_OK;
    QR_TRY(pt_rays_ptrs({rays_dev, state_dev}, rays_dev, spread_dev));
    QR_TRY(aligned_ptrs({state_dev, rgb_dev, open_dev}, 4, "state, rgb and open must be 4-byte aligned"));
    HIP_TRY(hipSetDevice(s->device));
    const PtRaysP pr = pt_rays_params(rays_dev, spread_dev, n, rgb_dev);
    hipLaunchKernelGGL(qr_pt_adapt_kernel, ray_grid(n), dim3(QR_BLOCK), 0, (hipStream_t)stream, s->lp, pr, (uint32_t *)state_dev,
                       samples, min_samples, max_samples, tol2, open_dev);
    return launched();
}

/* ---- adaptive path-traced views (qr_kernel.hpp qr_pt_adapt_views_kernel): qr_pt_views_async with the adaptive rays' state per slot ---- */

/* the checks every entry point of the feature shares: pt_views_dims, and the state's bytes held to what qr_pt_views_async allows */
static int pt_adapt_views_dims(const qr_device_scene *s, int n_views, int width, int height, uint64_t *slots)
{
    QR_TRY(pt_views_dims(s, n_views, width, height, slots));
    if ((uint64_t)n_views * *slots > ((uint64_t)1 << 29))
        return qr_fail(QR_ERR_ARG, "more than 2^29 pixel samples of adaptive path-tracer state in one launch");
    return QR_OK;
}

extern "C" int qr_pt_adapt_views_state_bytes(qr_device_scene *s, int n_views, int width, int height, uint64_t *bytes_out)
{
    uint64_t slots = 0;
    QR_TRY(pt_adapt_views_dims(s, n_views, width, height, &slots));
    return put_bytes(bytes_out, (uint64_t)n_views * QR_PT_ADAPT_STATE_WORDS * slots * sizeof(uint32_t));
}

extern "C" int qr_pt_adapt_views_reset(qr_device_scene *s, int n_views, int width, int height, void *state_dev)
{
    uint64_t slots = 0;
    QR_TRY(pt_adapt_views_dims(s, n_views, width, height, &slots));
    return pt_views_state_reset(s, n_views, slots, state_dev, QR_PT_ADAPT_STATE_WORDS);
}

extern "C" int qr_pt_adapt_views_async(qr_device_scene *s, const qr_view *views_dev, int n_views, int width, int height,
                                       void *state_dev, int samples, int min_samples, int max_samples, float tol2,
                                       uint32_t *frames_dev, float *mean_dev, int32_t *counts_dev, uint32_t *open_dev,
                                       uint32_t flags, void *stream)
{
    uint64_t slots = 0;
    QR_TRY(pt_adapt_views_dims(s, n_views, width, height, &slots));
    QR_TRY(flags_arg(flags, 0u, "unknown adaptive path-traced view flags"));
    QR_TRY(samples_arg(samples, QR_PT_ADAPT_VIEWS_MAX_SAMPLES));
    QR_TRY(rule_args(min_samples, max_samples, tol2));
    QR_TRY(need_query_list(s));
    if (n_views == 0) return QR_OK;
    QR_TRY(need_ptrs({views_dev, state_dev, frames_dev}));
    QR_TRY(aligned_ptrs({views_dev}, 16, "views must be 16-byte aligned"));
    QR_TRY(aligned_ptrs({state_dev, frames_dev, mean_dev, counts_dev, open_dev}, 4, "state, frames, mean, counts and open must be 4-byte aligned"));
    HIP_TRY(hipSetDevice(s->device));
    const ViewsP vp = views_params(views_dev, width, height);
    PtAdaptViewsP pa;
    pa.state = (uint32_t *)state_dev; pa.samples = samples; pa.min_samples = min_samples; pa.max_samples = max_samples; pa.tol2 = tol2;
    pa.mean = mean_dev; pa.counts = counts_dev; pa.open = open_dev;
    hipLaunchKernelGGL(qr_pt_adapt_views_kernel, footprint_grid(s, width, height, n_views), dim3(QR_BLOCK), 0, (hipStream_t)stream,
                       s->lp, vp, pa, frames_dev);
    return launched();
}

/* the per-pixel variance of an adaptive view state (qr_atrous.hpp qr_pt_adapt_var_kernel): the state is only read */
extern "C" int qr_pt_adapt_views_variance_async(qr_device_scene *s, const int32_t *state, int n_views, int width, int height,
                                                float unknown, float *var_dev, uint32_t flags, void *stream)
{
    uint64_t slots = 0;
    QR_TRY(pt_adapt_views_dims(s, n_views, width, height, &slots));
    QR_TRY(flags_arg(flags, 0u, "unknown adaptive view variance flags"));
    if (n_views == 0) return QR_OK;
    QR_TRY(need_ptrs({state, var_dev}));
    QR_TRY(aligned_ptrs({state, var_dev}, 4, "state and var must be 4-byte aligned"));
    HIP_TRY(hipSetDevice(s->device));
    const uint32_t pixels = (uint32_t)width * (uint32_t)height;
    const dim3 grid((pixels + 255u) / 256u, (unsigned)n_views), block(256);
    hipLaunchKernelGGL(qr_pt_adapt_var_kernel, grid, block, 0, (hipStream_t)stream, (const uint32_t *)state, pixels, s->fr.fsaa,
                       unknown, var_dev);
    return launched();
}

/* ---- guided a-trous filter (qr_atrous.hpp): one edge-avoiding pass over view frames, tiles in the decimated lattice ---- */

extern "C" int qr_atrous_views_async(qr_device_scene *s, const float *colour_in, const float *var_in, const qr_hit *hits,
                                     int n_views, int width, int height, const qr_atrous_params *p,
                                     float *colour_out, float *var_out, void *stream)
{
    QR_TRY(need_scene(s));
    QR_TRY(need_params(p, "null filter parameters"));
    QR_TRY(view_size_args(n_views, width, height));
    if (p->step < 1 || p->step > QR_ATROUS_MAX_STEP) return qr_fail(QR_ERR_ARG, "step must be 1.." + std::to_string(QR_ATROUS_MAX_STEP));
    QR_TRY(channels_arg(p->channels));
    QR_TRY(normal_sq_arg(p->normal_sq));
    QR_TRY(flags_arg(p->flags, QR_ATROUS_NORMAL | QR_ATROUS_PLANE | QR_ATROUS_LUMA | QR_ATROUS_DEMODULATE | QR_ATROUS_MODULATE,
                     "unknown filter flags"));
    if (!(p->sigma_z > 0.0f) || !(p->sigma_l2 > 0.0f) || !(p->eps_l > 0.0f) || !(p->alb_floor > 0.0f))
        return qr_fail(QR_ERR_ARG, "sigma_z, sigma_l2, eps_l and alb_floor must be above 0");
    QR_TRY(both_or_neither(var_in != nullptr, var_out != nullptr, "var_in and var_out go together: both or neither"));
    if (n_views == 0) return QR_OK;
    QR_TRY(need_ptrs({colour_in, colour_out, hits}));
    QR_TRY(aligned_16_and_4({hits}, "hits must be 16-byte aligned",
                            {colour_in, colour_out, var_in, var_out}, "colour and variance must be 4-byte aligned"));
    if (colour_in == colour_out || (var_in != nullptr && var_in == var_out))
        return qr_fail(QR_ERR_ARG, "a pass reads neighbours: it cannot run in place");
    HIP_TRY(hipSetDevice(s->device));
    AtrousP ap;
    ap.colour_in = colour_in; ap.var_in = var_in; ap.hits = (const f32x4 *)hits; ap.colour_out = colour_out; ap.var_out = var_out;
    ap.width = width; ap.height = height; ap.step = p->step; ap.normal_sq = p->normal_sq; ap.flags = p->flags;
    ap.sigma_z = p->sigma_z; ap.sigma_l2 = p->sigma_l2; ap.eps_l = p->eps_l; ap.alb_floor = p->alb_floor;
    /* phases per axis (no more than there are pixels), and tiles over the longest phase: entry i of phase f is pixel f + i * step */
    const int phx = std::min(p->step, width), phy = std::min(p->step, height);
    ap.tiles_x = ((width + p->step - 1) / p->step + QR_ATROUS_TW - 1) / QR_ATROUS_TW;
    ap.tiles_y = ((height + p->step - 1) / p->step + QR_ATROUS_TH - 1) / QR_ATROUS_TH;
    /* grid.y = phy * tiles_y <= height / 8 + 2 * step: far below 65535 at QR_VIEW_MAX_DIM */
    const dim3 grid((unsigned)(phx * ap.tiles_x), (unsigned)(phy * ap.tiles_y), (unsigned)n_views), block(QR_ATROUS_BLOCK);
    pick_channels(p->channels, [&](auto ch) {
        hipLaunchKernelGGL(qr_atrous_kernel<decltype(ch)::value>, grid, block, 0, (hipStream_t)stream, ap);
    });
    return launched();
}

/* ---- guided upsampling (qr_upsample.hpp): one lane per full pixel, 32 x 8 pixel tiles, blockIdx.z the view ---- */

extern "C" int qr_upsample_views_async(qr_device_scene *s, const float *colour_lo, const float *var_lo, const qr_hit *hits,
                                       int n_views, int width, int height, const qr_upsample_params *p,
                                       float *colour_out, float *var_out, float *weight_out, void *stream)
{
    QR_TRY(need_scene(s));
    QR_TRY(need_params(p, "null upsampling parameters"));
    QR_TRY(view_size_args(n_views, width, height));
    if (p->factor < 1 || p->factor > QR_UPSAMPLE_MAX_FACTOR)
        return qr_fail(QR_ERR_ARG, "factor must be 1.." + std::to_string(QR_UPSAMPLE_MAX_FACTOR));
    if (p->phase_x < 0 || p->phase_x >= p->factor || p->phase_y < 0 || p->phase_y >= p->factor)
        return qr_fail(QR_ERR_ARG, "phase_x and phase_y must be 0..factor - 1");
    if (p->phase_x >= width || p->phase_y >= height) return qr_fail(QR_ERR_ARG, "the phase lies beyond the frame: the coarse frame is empty");
    QR_TRY(channels_arg(p->channels));
    QR_TRY(normal_sq_arg(p->normal_sq));
    QR_TRY(flags_arg(p->flags, QR_UPSAMPLE_NORMAL | QR_UPSAMPLE_PLANE | QR_UPSAMPLE_SAME_ID | QR_UPSAMPLE_DEMODULATE | QR_UPSAMPLE_MODULATE,
                     "unknown upsampling flags"));
    if (!(p->sigma_z > 0.0f) || !(p->alb_floor > 0.0f)) return qr_fail(QR_ERR_ARG, "sigma_z and alb_floor must be above 0");
    QR_TRY(both_or_neither(var_lo != nullptr, var_out != nullptr, "var_lo and var_out go together: both or neither"));
    if (n_views == 0) return QR_OK;
    QR_TRY(need_ptrs({colour_lo, colour_out, hits}));
    QR_TRY(aligned_16_and_4({hits}, "hits must be 16-byte aligned",
                            {colour_lo, var_lo, colour_out, var_out, weight_out}, "colour, variance and weight must be 4-byte aligned"));
    for (const void *o : {(const void *)colour_out, (const void *)var_out, (const void *)weight_out})
        for (const void *i : {(const void *)colour_lo, (const void *)var_lo, (const void *)hits})
            if (o != nullptr && o == i) return qr_fail(QR_ERR_ARG, "a pixel reads its neighbours' lattice points: an output cannot be an input");
    HIP_TRY(hipSetDevice(s->device));
    UpsampleP up;
    up.colour_lo = colour_lo; up.var_lo = var_lo; up.hits = (const f32x4 *)hits;
    up.colour_out = colour_out; up.var_out = var_out; up.weight_out = weight_out;
    up.width = width; up.height = height;
    up.wl = (width - p->phase_x + p->factor - 1) / p->factor; up.hl = (height - p->phase_y + p->factor - 1) / p->factor;
    up.factor = p->factor; up.phase_x = p->phase_x; up.phase_y = p->phase_y; up.normal_sq = p->normal_sq; up.flags = p->flags;
    up.sigma_z = p->sigma_z; up.alb_floor = p->alb_floor;
    const dim3 grid = tile_grid(width, height, n_views, QR_UPS_TW, QR_UPS_TH), block(QR_UPS_BLOCK);
    pick_channels(p->channels, [&](auto ch) {
        hipLaunchKernelGGL(qr_upsample_kernel<decltype(ch)::value>, grid, block, 0, (hipStream_t)stream, up);
    });
    return launched();
}

/* ---- temporal reprojection (qr_reproject.hpp): one lane per pixel, 32 x 8 pixel tiles, blockIdx.z the view ---- */

/* the three entry points: every check of the static contract, then the table's, then the clamp block's, then the launch of
 * the static kernel (no table), of the moving one, or -- with a block -- of the clamp kernel with or without a table */
static int reproject_launch(qr_device_scene *s, const float *colour_in, const qr_hit *hits, const float *var_in,
                            const qr_view *views_prev, const qr_hit *hits_prev, const float *hist_in,
                            const qr_motion *motion_dev, int n_motion,
                            int n_views, int width, int height, const qr_reproject_params *p, const qr_clamp_params *clamp,
                            float *hist_out, float *colour_out, float *var_out, float *coords_out, float *moved_out, void *stream)
{
    QR_TRY(need_scene(s));
    QR_TRY(need_params(p, "null reprojection parameters"));
    QR_TRY(view_size_args(n_views, width, height));
    QR_TRY(channels_arg(p->channels));
    QR_TRY(flags_arg(p->flags, QR_REPROJ_DEMODULATE, "unknown reprojection flags"));
    if (p->reserved[0] != 0u || p->reserved[1] != 0u || p->reserved[2] != 0u)
        return qr_fail(QR_ERR_ARG, "the reserved words of the reprojection parameters must be 0");
    if (!(std::fabs(p->off_x) <= FLT_MAX) || !(std::fabs(p->off_y) <= FLT_MAX)) return qr_fail(QR_ERR_ARG, "off_x and off_y must be finite");
    if (p->normal_min != p->normal_min) return qr_fail(QR_ERR_ARG, "normal_min must not be NaN");
    if (!(p->plane_max > 0.0f) || !(p->alb_floor > 0.0f)) return qr_fail(QR_ERR_ARG, "plane_max and alb_floor must be above 0");
    if (!(p->min_weight >= 0.0f)) return qr_fail(QR_ERR_ARG, "min_weight must be 0 or more");
    if (!(p->alpha_min >= 0.0f && p->alpha_min <= 1.0f) || !(p->alpha_mom_min >= 0.0f && p->alpha_mom_min <= 1.0f))
        return qr_fail(QR_ERR_ARG, "alpha_min and alpha_mom_min must be 0..1");
    if (!(p->max_len >= 1.0f) || !(p->var_min_len >= 1.0f)) return qr_fail(QR_ERR_ARG, "max_len and var_min_len must be 1 or more");
    const int n_prev = (views_prev != nullptr) + (hits_prev != nullptr) + (hist_in != nullptr);
    if (n_prev != 0 && n_prev != 3)
        return qr_fail(QR_ERR_ARG, "views_prev, hits_prev and hist_in go together: all three or none (the first frame)");
    if (n_motion < 0 || n_motion > (1 << 30)) return qr_fail(QR_ERR_ARG, "n_motion must be 0..2^30");
    QR_TRY(both_or_neither(motion_dev != nullptr, n_motion > 0,
                           "motion_dev and n_motion go together: a table of n_motion >= 1 rows, or NULL and 0"));
    QR_TRY(aligned_ptrs({motion_dev}, 16, "the motion table must be 16-byte aligned"));
    if (n_views == 0) return QR_OK;
    QR_TRY(need_ptrs({colour_in, hits, hist_out}));
    QR_TRY(aligned_16_and_4({hits, views_prev, hits_prev, hist_in, hist_out}, "views, hits and history must be 16-byte aligned",
                            {colour_in, var_in, colour_out, var_out, coords_out}, "colour, variance and coords must be 4-byte aligned"));
    if (hist_in == hist_out) return qr_fail(QR_ERR_ARG, "the taps read neighbours' history: hist_out cannot be hist_in");
    if (clamp == nullptr && moved_out != nullptr) return qr_fail(QR_ERR_ARG, "moved_out needs a clamp block");
    if (clamp != nullptr)
    {
        const uint32_t mode = clamp->flags & (QR_CLAMP_MINMAX | QR_CLAMP_VARIANCE);
        if (mode != QR_CLAMP_MINMAX && mode != QR_CLAMP_VARIANCE)
            return qr_fail(QR_ERR_ARG, "a clamp is QR_CLAMP_MINMAX or QR_CLAMP_VARIANCE: exactly one of the two");
        QR_TRY(flags_arg(clamp->flags, QR_CLAMP_MINMAX | QR_CLAMP_VARIANCE | QR_CLAMP_SHORTEN, "unknown clamp flags"));
        if (clamp->reserved[0] != 0u || clamp->reserved[1] != 0u || clamp->reserved[2] != 0u || clamp->reserved[3] != 0u)
            return qr_fail(QR_ERR_ARG, "the reserved words of the clamp block must be 0");
        if (clamp->radius < 1 || clamp->radius > QR_CLAMP_MAX_RADIUS)
            return qr_fail(QR_ERR_ARG, "radius must be 1.." + std::to_string(QR_CLAMP_MAX_RADIUS));
        if (!(clamp->gamma >= 0.0f)) return qr_fail(QR_ERR_ARG, "gamma must be 0 or more");
        if (clamp->short_len != clamp->short_len || ((clamp->flags & QR_CLAMP_SHORTEN) && !(clamp->short_len >= 1.0f)))
            return qr_fail(QR_ERR_ARG, "short_len must not be NaN, and 1 or more with QR_CLAMP_SHORTEN");
        QR_TRY(aligned_ptrs({moved_out}, 4, "moved_out must be 4-byte aligned"));
    }
    HIP_TRY(hipSetDevice(s->device));
    ReprojClampP cp;
    ReprojMovingP &mp = cp.m;
    ReprojP &rp = mp.r;
    rp.colour_in = colour_in; rp.hits = (const f32x4 *)hits; rp.var_in = var_in;
    rp.views_prev = views_prev; rp.hits_prev = (const f32x4 *)hits_prev; rp.hist_in = (const f32x4 *)hist_in;
    rp.hist_out = (f32x4 *)hist_out; rp.colour_out = colour_out; rp.var_out = var_out; rp.coords_out = coords_out;
    rp.width = width; rp.height = height; rp.flags = p->flags;
    rp.off_x = p->off_x; rp.off_y = p->off_y; rp.normal_min = p->normal_min; rp.plane_max = p->plane_max;
    rp.min_weight = p->min_weight; rp.alpha_min = p->alpha_min; rp.alpha_mom_min = p->alpha_mom_min;
    rp.max_len = p->max_len; rp.var_min_len = p->var_min_len; rp.unknown = p->unknown; rp.alb_floor = p->alb_floor;
    mp.motion = (const f32x4 *)motion_dev; mp.n_motion = (u32)n_motion;
    const dim3 grid = tile_grid(width, height, n_views, QR_REPROJ_TW, QR_REPROJ_TH), block(QR_REPROJ_BLOCK);
    if (clamp != nullptr)
    {
        cp.cl.moved_out = moved_out; cp.cl.flags = clamp->flags; cp.cl.radius = clamp->radius;
        cp.cl.gamma = clamp->gamma; cp.cl.short_len = clamp->short_len;
    }
    pick_channels(p->channels, [&](auto ch) {
        constexpr int CH = decltype(ch)::value;
        if (clamp != nullptr)
            pick(motion_dev != nullptr, [&](auto moving) {
                hipLaunchKernelGGL((qr_reproj_clamp_kernel<CH, decltype(moving)::value>), grid, block, 0, (hipStream_t)stream, cp);
            });
        else if (motion_dev == nullptr) hipLaunchKernelGGL(qr_reproject_kernel<CH>, grid, block, 0, (hipStream_t)stream, rp);
        else hipLaunchKernelGGL(qr_reproj_moving_kernel<CH>, grid, block, 0, (hipStream_t)stream, mp);
    });
    return launched();
}

extern "C" int qr_reproject_views_async(qr_device_scene *s, const float *colour_in, const qr_hit *hits, const float *var_in,
                                        const qr_view *views_prev, const qr_hit *hits_prev, const float *hist_in,
                                        int n_views, int width, int height, const qr_reproject_params *p,
                                        float *hist_out, float *colour_out, float *var_out, float *coords_out, void *stream)
{
    return reproject_launch(s, colour_in, hits, var_in, views_prev, hits_prev, hist_in, nullptr, 0, n_views, width, height, p,
                            nullptr, hist_out, colour_out, var_out, coords_out, nullptr, stream);
}

extern "C" int qr_reproject_moving_async(qr_device_scene *s, const float *colour_in, const qr_hit *hits, const float *var_in,
                                         const qr_view *views_prev, const qr_hit *hits_prev, const float *hist_in,
                                         const qr_motion *motion_dev, int n_motion,
                                         int n_views, int width, int height, const qr_reproject_params *p,
                                         float *hist_out, float *colour_out, float *var_out, float *coords_out, void *stream)
{
    return reproject_launch(s, colour_in, hits, var_in, views_prev, hits_prev, hist_in, motion_dev, n_motion, n_views, width,
                            height, p, nullptr, hist_out, colour_out, var_out, coords_out, nullptr, stream);
}

extern "C" int qr_reproject_clamped_async(qr_device_scene *s, const float *colour_in, const qr_hit *hits, const float *var_in,
                                          const qr_view *views_prev, const qr_hit *hits_prev, const float *hist_in,
                                          const qr_motion *motion_dev, int n_motion,
                                          int n_views, int width, int height, const qr_reproject_params *p,
                                          const qr_clamp_params *clamp,
                                          float *hist_out, float *colour_out, float *var_out, float *coords_out, float *moved_out,
                                          void *stream)
{
    return reproject_launch(s, colour_in, hits, var_in, views_prev, hits_prev, hist_in, motion_dev, n_motion, n_views, width,
                            height, p, clamp, hist_out, colour_out, var_out, coords_out, moved_out, stream);
}

/* ---- open lists and indexed adaptive steps (qr_openlist.hpp, qr_kernel.hpp qr_pt_list_kernel): compaction on chip ---- */

static inline int64_t pt_open_blocks(int64_t n) { return (n + QR_PT_OPEN_BLOCK - 1) / QR_PT_OPEN_BLOCK; }

extern "C" int qr_pt_adapt_list_work_bytes(qr_device_scene *s, int64_t n, uint64_t *bytes_out)
{
    QR_TRY(pt_rays_dims(s, n));
    /* one word per block; the scan works in place and needs none of its own */
    return put_bytes(bytes_out, (uint64_t)pt_open_blocks(n) * sizeof(uint32_t));
}

extern "C" int qr_pt_adapt_open_list_async(qr_device_scene *s, const void *state_dev, int64_t n,
                                           int min_samples, int max_samples, float tol2,
                                           uint32_t *index_dev, uint32_t *count_dev, void *work_dev, uint32_t flags, void *stream)
{
    QR_TRY(pt_adapt_args(s, n, 1, min_samples, max_samples, tol2, flags));
    if (n == 0) return QR_OK;
    QR_TRY(need_ptrs({state_dev, index_dev, count_dev, work_dev}));
    QR_TRY(aligned_ptrs({state_dev, index_dev, count_dev, work_dev}, 4, "state, index, count and work must be 4-byte aligned"));
    HIP_TRY(hipSetDevice(s->device));
    const unsigned nb = (unsigned)pt_open_blocks(n);
    const uint32_t *st = (const uint32_t *)state_dev;
    uint32_t *work = (uint32_t *)work_dev;
    hipLaunchKernelGGL(qr_open_count_kernel, dim3(nb), dim3(QR_PT_OPEN_BLOCK), 0, (hipStream_t)stream, st, (uint32_t)n,
                       (uint32_t)min_samples, (uint32_t)max_samples, tol2, work);
    hipLaunchKernelGGL(qr_open_scan_kernel, dim3(1), dim3(QR_PT_OPEN_CHUNK), 0, (hipStream_t)stream, work, (uint32_t)nb, count_dev);
    hipLaunchKernelGGL(qr_open_scatter_kernel, dim3(nb), dim3(QR_PT_OPEN_BLOCK), 0, (hipStream_t)stream, st, (uint32_t)n,
                       (uint32_t)min_samples, (uint32_t)max_samples, tol2, (const uint32_t *)work, index_dev);
    return launched();
}

extern "C" int qr_pt_adapt_list_rays_async(qr_device_scene *s, const qr_ray *rays_dev, const qr_ray_spread *spread_dev, int64_t n,
                                           void *state_dev, const uint32_t *index_dev, const uint32_t *count_dev, int64_t cap,
                                           int samples, int min_samples, int max_samples, float tol2,
                                           float *rgb_dev, uint32_t *open_dev, uint32_t flags, void *stream)
{
    QR_TRY(pt_adapt_args(s, n, samples, min_samples, max_samples, tol2, flags));
    if (cap < 0) return qr_fail(QR_ERR_ARG, "cap must be 0 or more: the caller's upper bound on the list's length");
    if (n == 0 || cap == 0) return QR_OK;
    QR_TRY(pt_rays_ptrs({rays_dev, state_dev, index_dev, count_dev}, rays_dev, spread_dev));
    QR_TRY(aligned_ptrs({state_dev, rgb_dev, open_dev, index_dev, count_dev}, 4, "state, rgb, open, index and count must be 4-byte aligned"));
    HIP_TRY(hipSetDevice(s->device));
    const int64_t most = cap < n ? cap : n;             /* distinct entries below n: a list holds at most n that count */
    const PtRaysP pr = pt_rays_params(rays_dev, spread_dev, n, rgb_dev);
    hipLaunchKernelGGL(qr_pt_list_kernel, ray_grid(most), dim3(QR_BLOCK), 0, (hipStream_t)stream, s->lp, pr, (uint32_t *)state_dev,
                       index_dev, count_dev, (uint32_t)most, samples, min_samples, max_samples, tol2, open_dev);
    return launched();
}

/* ---- hit records (qr_hitrec.hpp): the closest hit of qr_trace_rays_async and the surface point shading would use there ---- */

extern "C" int qr_hit_rays_async(qr_device_scene *s, const qr_ray *rays_dev, int64_t n,
                                 qr_hit *hits_dev, uint32_t flags, void *stream)
{
    QR_TRY(query_args(s, rays_dev, n, hits_dev, hits_dev, flags));
    if (n == 0) return QR_OK;
    QR_TRY(aligned_ptrs({hits_dev}, 16, "hits must be 16-byte aligned"));
    HIP_TRY(hipSetDevice(s->device));
    const ViewsP vp = {};
    pick(flags & QR_TRACE_COHERENT, [&](auto coherent) {
        hipLaunchKernelGGL((qr_hit_kernel<false, true, decltype(coherent)::value>), ray_grid(n), dim3(QR_BLOCK), 0, (hipStream_t)stream,
                           (const char *)s->d_blob, (const f32x4 *)rays_dev, (int32_t)n, vp, s->off_mat, (f32x4 *)hits_dev, s->lp.stats);
    });
    return launched();
}

extern "C" int qr_hit_views_async(qr_device_scene *s, const qr_view *views_dev, int n_views, int width, int height,
                                  qr_hit *hits_dev, uint32_t flags, void *stream)
{
    QR_TRY(need_scene(s));
    QR_TRY(view_size_args(n_views, width, height));
    QR_TRY(flags_arg(flags, 0u, "unknown view flags"));
    QR_TRY(need_query_list(s));
    QR_TRY(view_grid_arg(s, n_views, width, height));
    if (n_views == 0) return QR_OK;
    QR_TRY(need_ptrs({views_dev, hits_dev}));
    QR_TRY(aligned_ptrs({views_dev, hits_dev}, 16, "views and hits must be 16-byte aligned"));
    HIP_TRY(hipSetDevice(s->device));
    const ViewsP vp = views_params(views_dev, width, height);
    pick_walk(s, [&](auto w) {
        hipLaunchKernelGGL((qr_hit_kernel<true, decltype(w)::divk, true>), pixel_grid(width, height, n_views), dim3(QR_BLOCK), 0,
                           (hipStream_t)stream, (const char *)s->d_blob, (const f32x4 *)nullptr, 0, vp, s->off_mat, (f32x4 *)hits_dev,
                           s->lp.stats);
    });
    return launched();
}

/* ---- occlusion fans (qr_fan.hpp): per surface point, how many directions of a shared table are open ---- */

/* what the three entry points check alike, before the element count decides whether anything is launched */
static int fan_args(const qr_device_scene *s, int k, float eps, float reach, uint32_t flags, uint32_t allowed)
{
    QR_TRY(flags_arg(flags, allowed, "unknown fan flags"));
    if (k < 1 || k > QR_FAN_MAX_DIRS) return qr_fail(QR_ERR_ARG, "direction count must be 1.." + std::to_string(QR_FAN_MAX_DIRS));
    if (std::isnan(eps) || std::isnan(reach)) return qr_fail(QR_ERR_ARG, "eps and reach must not be NaN");
    return need_query_list(s);
}

/* ... and once there are elements: src is the ray, view or record array; the spin plane of a framed call, float [elements][2],
 * may be null */
static int fan_ptrs(const void *src, const qr_fan_dir *dirs, const int32_t *open, const uint32_t *mask, const float *spin)
{
    QR_TRY(need_ptrs({src, dirs, open}));
    QR_TRY(aligned_ptrs({src, dirs}, 16, "rays, views, hits and dirs must be 16-byte aligned"));
    QR_TRY(aligned_ptrs({open, mask}, 4, "open and mask must be 4-byte aligned"));
    return aligned_ptrs({spin}, 8, "spin must be 8-byte aligned");
}

static FanP fan_params(const qr_fan_dir *dirs, int k, float eps, float reach, int32_t *open, uint32_t *mask, uint32_t flags, uint64_t elems)
{
    FanP fp;
    fp.dirs = dirs; fp.k = k; fp.flip = flags & QR_FAN_FLIP;
    fp.eps = eps; fp.reach = reach > FLT_MAX ? FLT_MAX : reach;     /* +inf is taken as FLT_MAX, as in qr_trace_kernel */
    fp.open = open; fp.mask = mask; fp.elems = elems;
    return fp;
}

/* the three sources, unframed (qr_fan.hpp) or framed (qr_fan_framed.hpp: spin may be null) */
static int fan_rays(qr_device_scene *s, const qr_ray *rays_dev, int64_t n, const qr_fan_dir *dirs_dev, int k, float eps, float reach,
                    int32_t *open_dev, uint32_t *mask_dev, uint32_t flags, void *stream, bool framed, const float *spin_dev)
{
    QR_TRY(need_scene(s));
    QR_TRY(count_arg(n, "ray"));
    QR_TRY(fan_args(s, k, eps, reach, flags, QR_TRACE_COHERENT | QR_FAN_FLIP));
    if (n == 0) return QR_OK;
    QR_TRY(fan_ptrs(rays_dev, dirs_dev, open_dev, mask_dev, spin_dev));
    HIP_TRY(hipSetDevice(s->device));
    const dim3 grid = ray_grid(n), block(QR_BLOCK);
    const f32x4 *r = (const f32x4 *)rays_dev;
    const ViewsP vp = {};
    const FanP fp = fan_params(dirs_dev, k, eps, reach, open_dev, mask_dev, flags, (uint64_t)n);
    pick(flags & QR_TRACE_COHERENT, [&](auto coherent) {
        constexpr bool C = decltype(coherent)::value;
        if (framed)
            hipLaunchKernelGGL((qr_fan_framed_kernel<QR_FAN_SRC_RAYS, true, C>), grid, block, 0, (hipStream_t)stream,
                               (const char *)s->d_blob, r, (int32_t)n, vp, fp, (const float2 *)spin_dev, s->lp.stats);
        else
            hipLaunchKernelGGL((qr_fan_kernel<QR_FAN_SRC_RAYS, true, C>), grid, block, 0, (hipStream_t)stream,
                               (const char *)s->d_blob, r, (int32_t)n, vp, fp, s->lp.stats);
    });
    return launched();
}

static int fan_hits(qr_device_scene *s, const qr_hit *hits_dev, int64_t n, const qr_fan_dir *dirs_dev, int k, float eps, float reach,
                    int32_t *open_dev, uint32_t *mask_dev, uint32_t flags, void *stream, bool framed, const float *spin_dev)
{
    QR_TRY(need_scene(s));
    QR_TRY(count_arg(n, "record"));
    QR_TRY(fan_args(s, k, eps, reach, flags, QR_FAN_FLIP));
    if (n == 0) return QR_OK;
    QR_TRY(fan_ptrs(hits_dev, dirs_dev, open_dev, mask_dev, spin_dev));
    HIP_TRY(hipSetDevice(s->device));
    const dim3 grid = ray_grid(n), block(QR_BLOCK);
    const f32x4 *h = (const f32x4 *)hits_dev;
    const ViewsP vp = {};
    const FanP fp = fan_params(dirs_dev, k, eps, reach, open_dev, mask_dev, flags, (uint64_t)n);
    if (framed)
        hipLaunchKernelGGL((qr_fan_framed_kernel<QR_FAN_SRC_HITS, true, false>), grid, block, 0, (hipStream_t)stream,
                           (const char *)s->d_blob, h, (int32_t)n, vp, fp, (const float2 *)spin_dev, s->lp.stats);
    else
        hipLaunchKernelGGL((qr_fan_kernel<QR_FAN_SRC_HITS, true, false>), grid, block, 0, (hipStream_t)stream, (const char *)s->d_blob,
                           h, (int32_t)n, vp, fp, s->lp.stats);
    return launched();
}

static int fan_views(qr_device_scene *s, const qr_view *views_dev, int n_views, int width, int height, const qr_fan_dir *dirs_dev, int k,
                     float eps, float reach, int32_t *open_dev, uint32_t *mask_dev, uint32_t flags, void *stream, bool framed,
                     const float *spin_dev)
{
    QR_TRY(need_scene(s));
    QR_TRY(view_size_args(n_views, width, height));
    QR_TRY(fan_args(s, k, eps, reach, flags, QR_FAN_FLIP));
    QR_TRY(view_grid_arg(s, n_views, width, height));
    if (n_views == 0) return QR_OK;
    QR_TRY(fan_ptrs(views_dev, dirs_dev, open_dev, mask_dev, spin_dev));
    HIP_TRY(hipSetDevice(s->device));
    const dim3 grid = pixel_grid(width, height, n_views), block(QR_BLOCK);
    const ViewsP vp = views_params(views_dev, width, height);
    const FanP fp = fan_params(dirs_dev, k, eps, reach, open_dev, mask_dev, flags, (uint64_t)n_views * (uint64_t)width * (uint64_t)height);
    const f32x4 *none = nullptr;
    pick_walk(s, [&](auto w) {
        constexpr bool D = decltype(w)::divk;
        if (framed)
            hipLaunchKernelGGL((qr_fan_framed_kernel<QR_FAN_SRC_VIEW, D, true>), grid, block, 0, (hipStream_t)stream,
                               (const char *)s->d_blob, none, 0, vp, fp, (const float2 *)spin_dev, s->lp.stats);
        else
            hipLaunchKernelGGL((qr_fan_kernel<QR_FAN_SRC_VIEW, D, true>), grid, block, 0, (hipStream_t)stream, (const char *)s->d_blob,
                               none, 0, vp, fp, s->lp.stats);
    });
    return launched();
}

extern "C" int qr_fan_rays_async(qr_device_scene *s, const qr_ray *rays_dev, int64_t n, const qr_fan_dir *dirs_dev, int k,
                                 float eps, float reach, int32_t *open_dev, uint32_t *mask_dev, uint32_t flags, void *stream)
{
    return fan_rays(s, rays_dev, n, dirs_dev, k, eps, reach, open_dev, mask_dev, flags, stream, false, nullptr);
}

extern "C" int qr_fan_rays_framed_async(qr_device_scene *s, const qr_ray *rays_dev, int64_t n, const qr_fan_dir *dirs_dev, int k,
                                        const float *spin_dev, float eps, float reach, int32_t *open_dev, uint32_t *mask_dev,
                                        uint32_t flags, void *stream)
{
    return fan_rays(s, rays_dev, n, dirs_dev, k, eps, reach, open_dev, mask_dev, flags, stream, true, spin_dev);
}

extern "C" int qr_fan_hits_async(qr_device_scene *s, const qr_hit *hits_dev, int64_t n, const qr_fan_dir *dirs_dev, int k,
                                 float eps, float reach, int32_t *open_dev, uint32_t *mask_dev, uint32_t flags, void *stream)
{
    return fan_hits(s, hits_dev, n, dirs_dev, k, eps, reach, open_dev, mask_dev, flags, stream, false, nullptr);
}

extern "C" int qr_fan_hits_framed_async(qr_device_scene *s, const qr_hit *hits_dev, int64_t n, const qr_fan_dir *dirs_dev, int k,
                                        const float *spin_dev, float eps, float reach, int32_t *open_dev, uint32_t *mask_dev,
                                        uint32_t flags, void *stream)
{
    return fan_hits(s, hits_dev, n, dirs_dev, k, eps, reach, open_dev, mask_dev, flags, stream, true, spin_dev);
}

extern "C" int qr_fan_views_async(qr_device_scene *s, const qr_view *views_dev, int n_views, int width, int height,
                                  const qr_fan_dir *dirs_dev, int k, float eps, float reach, int32_t *open_dev, uint32_t *mask_dev,
                                  uint32_t flags, void *stream)
{
    return fan_views(s, views_dev, n_views, width, height, dirs_dev, k, eps, reach, open_dev, mask_dev, flags, stream, false, nullptr);
}

extern "C" int qr_fan_views_framed_async(qr_device_scene *s, const qr_view *views_dev, int n_views, int width, int height,
                                         const qr_fan_dir *dirs_dev, int k, const float *spin_dev, float eps, float reach,
                                         int32_t *open_dev, uint32_t *mask_dev, uint32_t flags, void *stream)
{
    return fan_views(s, views_dev, n_views, width, height, dirs_dev, k, eps, reach, open_dev, mask_dev, flags, stream, true, spin_dev);
}

/* ---- gather fans (qr_gather.hpp): per surface point, the weighted sum of the renderer's colours along a shared table ---- */

/* what the three entry points check alike before the element count decides whether anything is launched: the fans' checks, then
 * what ray shading refuses */
static int gather_args(const qr_device_scene *s, int k, float eps, float reach, uint32_t flags, uint32_t allowed)
{
    QR_TRY(fan_args(s, k, eps, reach, flags, allowed | QR_FAN_FLIP | QR_GATHER_COSINE | QR_GATHER_RESUME));
    return no_pt_mode(s, "fan rays carry no sample seeds");
}

/* ... and once there are elements: src is the ray, view or record array; spin as in fan_ptrs */
static int gather_ptrs(const void *src, const qr_gather_dir *dirs, const float *gather, const int32_t *count, const float *spin)
{
    QR_TRY(need_ptrs({src, dirs, gather, count}));
    QR_TRY(aligned_ptrs({src, dirs, gather}, 16, "rays, views, hits, dirs and gather must be 16-byte aligned"));
    QR_TRY(aligned_ptrs({count}, 4, "count must be 4-byte aligned"));
    return aligned_ptrs({spin}, 8, "spin must be 8-byte aligned");
}

static GatherP gather_params(const qr_gather_dir *dirs, int k, float eps, float reach, float *gather, int32_t *count, uint32_t flags)
{
    GatherP gp;
    gp.dirs = dirs; gp.k = k;
    gp.flip = flags & QR_FAN_FLIP; gp.cosine = flags & QR_GATHER_COSINE; gp.resume = flags & QR_GATHER_RESUME;
    gp.eps = eps; gp.reach = reach > FLT_MAX ? FLT_MAX : reach;     /* +inf is taken as FLT_MAX, as in qr_shade_rays_async */
    gp.gather = (f32x4 *)gather; gp.count = count;
    return gp;
}

/* the three sources, unframed (qr_gather.hpp) or framed (qr_fan_framed.hpp: spin may be null).  Rays and records take the
 * per-lane walk instance, as ray shading does; views choose as the views do */
static int gather_rays(qr_device_scene *s, const qr_ray *rays_dev, int64_t n, const qr_gather_dir *dirs_dev, int k, float eps, float reach,
                       float *gather_dev, int32_t *count_dev, uint32_t flags, void *stream, bool framed, const float *spin_dev)
{
    QR_TRY(need_scene(s));
    QR_TRY(count_arg(n, "ray"));
    QR_TRY(gather_args(s, k, eps, reach, flags, QR_TRACE_COHERENT));
    if (n == 0) return QR_OK;
    QR_TRY(gather_ptrs(rays_dev, dirs_dev, gather_dev, count_dev, spin_dev));
    HIP_TRY(hipSetDevice(s->device));
    const dim3 grid = ray_grid(n), block(QR_BLOCK);
    const f32x4 *r = (const f32x4 *)rays_dev;
    const ViewsP vp = {};
    const GatherP gp = gather_params(dirs_dev, k, eps, reach, gather_dev, count_dev, flags);
    pick(flags & QR_TRACE_COHERENT, [&](auto coherent) {
        constexpr bool C = decltype(coherent)::value;
        if (framed)
            hipLaunchKernelGGL((qr_gather_framed_kernel<QR_FAN_SRC_RAYS, true, C, QR_DIVK_WAVES>), grid, block, 0, (hipStream_t)stream,
                               s->lp, r, (int32_t)n, vp, gp, (const float2 *)spin_dev);
        else
            hipLaunchKernelGGL((qr_gather_kernel<QR_FAN_SRC_RAYS, true, C, QR_DIVK_WAVES>), grid, block, 0, (hipStream_t)stream,
                               s->lp, r, (int32_t)n, vp, gp);
    });
    return launched();
}

static int gather_hits(qr_device_scene *s, const qr_hit *hits_dev, int64_t n, const qr_gather_dir *dirs_dev, int k, float eps, float reach,
                       float *gather_dev, int32_t *count_dev, uint32_t flags, void *stream, bool framed, const float *spin_dev)
{
    QR_TRY(need_scene(s));
    QR_TRY(count_arg(n, "record"));
    QR_TRY(gather_args(s, k, eps, reach, flags, 0u));
    if (n == 0) return QR_OK;
    QR_TRY(gather_ptrs(hits_dev, dirs_dev, gather_dev, count_dev, spin_dev));
    HIP_TRY(hipSetDevice(s->device));
    const dim3 grid = ray_grid(n), block(QR_BLOCK);
    const f32x4 *h = (const f32x4 *)hits_dev;
    const ViewsP vp = {};
    const GatherP gp = gather_params(dirs_dev, k, eps, reach, gather_dev, count_dev, flags);
    if (framed)
        hipLaunchKernelGGL((qr_gather_framed_kernel<QR_FAN_SRC_HITS, true, false, QR_DIVK_WAVES>), grid, block, 0, (hipStream_t)stream,
                           s->lp, h, (int32_t)n, vp, gp, (const float2 *)spin_dev);
    else
        hipLaunchKernelGGL((qr_gather_kernel<QR_FAN_SRC_HITS, true, false, QR_DIVK_WAVES>), grid, block, 0, (hipStream_t)stream, s->lp,
                           h, (int32_t)n, vp, gp);
    return launched();
}

static int gather_views(qr_device_scene *s, const qr_view *views_dev, int n_views, int width, int height, const qr_gather_dir *dirs_dev,
                        int k, float eps, float reach, float *gather_dev, int32_t *count_dev, uint32_t flags, void *stream, bool framed,
                        const float *spin_dev)
{
    QR_TRY(need_scene(s));
    QR_TRY(view_size_args(n_views, width, height));
    QR_TRY(gather_args(s, k, eps, reach, flags, 0u));
    QR_TRY(view_grid_arg(s, n_views, width, height));
    if (n_views == 0) return QR_OK;
    QR_TRY(gather_ptrs(views_dev, dirs_dev, gather_dev, count_dev, spin_dev));
    HIP_TRY(hipSetDevice(s->device));
    const dim3 grid = pixel_grid(width, height, n_views), block(QR_BLOCK);
    const ViewsP vp = views_params(views_dev, width, height);
    const GatherP gp = gather_params(dirs_dev, k, eps, reach, gather_dev, count_dev, flags);
    const f32x4 *none = nullptr;
    pick_walk(s, [&](auto w) {
        using W = decltype(w);
        if (framed)
            hipLaunchKernelGGL((qr_gather_framed_kernel<QR_FAN_SRC_VIEW, W::divk, true, W::waves>), grid, block, 0, (hipStream_t)stream,
                               s->lp, none, 0, vp, gp, (const float2 *)spin_dev);
        else
            hipLaunchKernelGGL((qr_gather_kernel<QR_FAN_SRC_VIEW, W::divk, true, W::waves>), grid, block, 0, (hipStream_t)stream,
                               s->lp, none, 0, vp, gp);
    });
    return launched();
}

extern "C" int qr_gather_rays_async(qr_device_scene *s, const qr_ray *rays_dev, int64_t n, const qr_gather_dir *dirs_dev, int k,
                                    float eps, float reach, float *gather_dev, int32_t *count_dev, uint32_t flags, void *stream)
{
    return gather_rays(s, rays_dev, n, dirs_dev, k, eps, reach, gather_dev, count_dev, flags, stream, false, nullptr);
}

extern "C" int qr_gather_rays_framed_async(qr_device_scene *s, const qr_ray *rays_dev, int64_t n, const qr_gather_dir *dirs_dev, int k,
                                           const float *spin_dev, float eps, float reach, float *gather_dev, int32_t *count_dev,
                                           uint32_t flags, void *stream)
{
    return gather_rays(s, rays_dev, n, dirs_dev, k, eps, reach, gather_dev, count_dev, flags, stream, true, spin_dev);
}

extern "C" int qr_gather_hits_async(qr_device_scene *s, const qr_hit *hits_dev, int64_t n, const qr_gather_dir *dirs_dev, int k,
                                    float eps, float reach, float *gather_dev, int32_t *count_dev, uint32_t flags, void *stream)
{
    return gather_hits(s, hits_dev, n, dirs_dev, k, eps, reach, gather_dev, count_dev, flags, stream, false, nullptr);
}

extern "C" int qr_gather_hits_framed_async(qr_device_scene *s, const qr_hit *hits_dev, int64_t n, const qr_gather_dir *dirs_dev, int k,
                                           const float *spin_dev, float eps, float reach, float *gather_dev, int32_t *count_dev,
                                           uint32_t flags, void *stream)
{
    return gather_hits(s, hits_dev, n, dirs_dev, k, eps, reach, gather_dev, count_dev, flags, stream, true, spin_dev);
}

extern "C" int qr_gather_views_async(qr_device_scene *s, const qr_view *views_dev, int n_views, int width, int height,
                                     const qr_gather_dir *dirs_dev, int k, float eps, float reach, float *gather_dev, int32_t *count_dev,
                                     uint32_t flags, void *stream)
{
    return gather_views(s, views_dev, n_views, width, height, dirs_dev, k, eps, reach, gather_dev, count_dev, flags, stream, false, nullptr);
}

extern "C" int qr_gather_views_framed_async(qr_device_scene *s, const qr_view *views_dev, int n_views, int width, int height,
                                            const qr_gather_dir *dirs_dev, int k, const float *spin_dev, float eps, float reach,
                                            float *gather_dev, int32_t *count_dev, uint32_t flags, void *stream)
{
    return gather_views(s, views_dev, n_views, width, height, dirs_dev, k, eps, reach, gather_dev, count_dev, flags, stream, true, spin_dev);
}

/* ---- hit layers (qr_layers.hpp): the first k hits along a ray, in order ---- */

/* what the two entry points check alike, before the element count decides whether anything is launched */
static int layer_args(const qr_device_scene *s, int k, uint32_t flags, uint32_t allowed)
{
    QR_TRY(flags_arg(flags, allowed, "unknown layer flags"));
    if (k < 1 || k > QR_LAYER_MAX) return qr_fail(QR_ERR_ARG, "layer count must be 1.." + std::to_string(QR_LAYER_MAX));
    return need_query_list(s);
}

/* ... and once there are elements: src is the ray or view array; t, id and hits may be null */
static int layer_ptrs(const void *src, const int32_t *count, const float *t, const int32_t *id, const qr_hit *hits)
{
    QR_TRY(need_ptrs({src, count}));
    QR_TRY(aligned_ptrs({src, hits}, 16, "rays, views and hits must be 16-byte aligned"));
    return aligned_ptrs({count, t, id}, 4, "count, t and id must be 4-byte aligned");
}

static LayerP layer_params(const qr_device_scene *s, int k, int32_t *count, float *t, int32_t *id, qr_hit *hits, uint64_t elems)
{
    LayerP lp;
    lp.k = k; lp.off_mat = s->off_mat;
    lp.count = count; lp.t = t; lp.id = id; lp.hits = (f32x4 *)hits; lp.elems = elems;
    return lp;
}

extern "C" int qr_layer_rays_async(qr_device_scene *s, const qr_ray *rays_dev, int64_t n, int k,
                                   int32_t *count_dev, float *t_dev, int32_t *id_dev, qr_hit *hits_dev,
                                   uint32_t flags, void *stream)
{
    QR_TRY(need_scene(s));
    QR_TRY(count_arg(n, "ray"));
    QR_TRY(layer_args(s, k, flags, QR_TRACE_COHERENT));
    if (n == 0) return QR_OK;
    QR_TRY(layer_ptrs(rays_dev, count_dev, t_dev, id_dev, hits_dev));
    HIP_TRY(hipSetDevice(s->device));
    const ViewsP vp = {};
    const LayerP lp = layer_params(s, k, count_dev, t_dev, id_dev, hits_dev, (uint64_t)n);
    pick(flags & QR_TRACE_COHERENT, [&](auto coherent) {
        hipLaunchKernelGGL((qr_layer_kernel<false, true, decltype(coherent)::value>), ray_grid(n), dim3(QR_BLOCK), 0, (hipStream_t)stream,
                           (const char *)s->d_blob, (const f32x4 *)rays_dev, (int32_t)n, vp, lp, s->lp.stats);
    });
    return launched();
}

extern "C" int qr_layer_views_async(qr_device_scene *s, const qr_view *views_dev, int n_views, int width, int height, int k,
                                    int32_t *count_dev, float *t_dev, int32_t *id_dev, qr_hit *hits_dev,
                                    uint32_t flags, void *stream)
{
    QR_TRY(need_scene(s));
    QR_TRY(view_size_args(n_views, width, height));
    QR_TRY(layer_args(s, k, flags, 0u));
    QR_TRY(view_grid_arg(s, n_views, width, height));
    if (n_views == 0) return QR_OK;
    QR_TRY(layer_ptrs(views_dev, count_dev, t_dev, id_dev, hits_dev));
    HIP_TRY(hipSetDevice(s->device));
    const ViewsP vp = views_params(views_dev, width, height);
    const LayerP lp = layer_params(s, k, count_dev, t_dev, id_dev, hits_dev, (uint64_t)n_views * (uint64_t)width * (uint64_t)height);
    pick_walk(s, [&](auto w) {
        hipLaunchKernelGGL((qr_layer_kernel<true, decltype(w)::divk, true>), pixel_grid(width, height, n_views), dim3(QR_BLOCK), 0,
                           (hipStream_t)stream, (const char *)s->d_blob, (const f32x4 *)nullptr, 0, vp, lp, s->lp.stats);
    });
    return launched();
}
