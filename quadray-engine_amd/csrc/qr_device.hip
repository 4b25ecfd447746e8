/*
 * qr_device.hip - GPU half of the C ABI (include/qrhip.h): scene upload,
 * launches, timing, and qr_render0 (the reference entry point replacement,
 * core/tracer/tracer.cpp:1081 / dispatcher 5992-6104).
 *
 * No CPU fallback exists: every entry point here fails with QR_ERR_DEVICE when
 * no HIP device is usable.
 */
#include "qr_internal.h"
#include "qr_kernel.hpp"
#include "qr_query.hpp"
#include "qr_hitrec.hpp"
#include "qr_fan.hpp"
#include "qr_gather.hpp"
#include "qr_fan_framed.hpp"
#include "qr_layers.hpp"
#include "qr_openlist.hpp"
#include "qr_atrous.hpp"
#include "qr_reproject.hpp"
#include "qr_upsample.hpp"

#include <hip/hip_runtime.h>
#include <cstring>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif
#include <vector>
#include <thread>
#include <mutex>
#include <map>
#include <atomic>
#include <array>
#include <algorithm>
#include <chrono>
#include <utility>
#include <string>
#include <type_traits>
#include <initializer_list>

#include "qr_dev_mem.hpp"

struct qr_device_scene
{
    uint64_t serial = 0;        /* unique per upload for the life of the process: caches keyed on a scene (the QR_DEVICES replicas of
                                 * qr_render_host) use it -- a destroyed scene's address and its image's device address are reused */
    int device = 0;
    void *d_blob = nullptr;     /* the compiled scene image (qr_program.h), one allocation */
    uint64_t blob_bytes = 0;
    LaunchP lp = {};            /* blob pointer + launch parameters          */
    qr_frame fr = {};           /* host copy of the frame parameters        */
    qr_header hdr = {};
    unsigned long long *d_counters = nullptr;
    size_t n_cells = 0;
    int32_t n_groups = 0;
    bool divk = false;          /* some list is a long hierarchy: launch the kernel instance with the per-lane walk */
    uint32_t off_query = 0;     /* the ray-query list in the image (QR_UPLOAD_RAY_QUERIES), 0 none */
    uint32_t off_mat = 0;       /* the image's material table: hit records turn DShade::mat back into the snapshot's index */
    /* path-tracer mode (qr_scene_set_pt): what the engine keeps per frame buffer, engine.cpp:2875-2893 */
    bool pt_on = false;
    uint32_t *d_seeds = nullptr; float *d_acc = nullptr;     /* frm_row * frm_h * samples each; d_acc holds r, g, b planes */
    uint64_t pt_frames = 0;
    int pt_eager = 0;           /* 1: the reference's shading order (qr_pt_eager.hpp): its random streams, slow; 3: self-test */
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    /* the whole-frame wave schedule (host copy) and the schedules of the row selections rendered so far (launch) */
    std::vector<uint32_t> h_order;
    std::map<std::array<int32_t, 6>, SchedBuf> sub;
};

static int need_scene(const qr_device_scene *s) { return s ? QR_OK : qr_fail(QR_ERR_ARG, "null scene"); }

/* The first n seeds of the engine's seed plane, as rt_Scene::reset_pseed fills it (engine.cpp:3651-3685: a 48-bit LCG walks
 * over the slots, each slot keeps the low 32 bits): what every path-tracer state starts from. */
static std::vector<uint32_t> pt_seed_plane(size_t n)
{
    std::vector<uint32_t> seeds(n);
    unsigned long long seed = 1;
    for (size_t k = 0; k < n; k++)
    {
        seed = (seed * 25214903917ull + 11ull) & 0x0000FFFFFFFFFFFFull;
        seeds[k] = (uint32_t)seed;
    }
    return seeds;
}

extern "C" const char *qr_kernel_name(void) { return "qr_render_kernel"; }

extern "C" int qr_device_count(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

#include "qr_dev_launch.hpp"
#include "qr_dev_upload.hpp"

extern "C" int qr_scene_get_info(const qr_device_scene *s, qr_scene_info *info)
{
    if (s == nullptr || info == nullptr) return qr_fail(QR_ERR_ARG, "null argument");
    memset(info, 0, sizeof(*info));
    info->frm_w = s->fr.frm_w; info->frm_h = s->fr.frm_h;
    info->fsaa = s->fr.fsaa; info->depth = s->lp.depth;
    info->n_srf = (int32_t)s->hdr.n_srf; info->n_mat = (int32_t)s->hdr.n_mat; info->n_lgt = (int32_t)s->hdr.n_lgt;
    info->n_elm = (int32_t)s->n_cells; info->n_tiles = s->fr.tls_row * s->fr.tls_col; info->n_texels = (int32_t)s->hdr.n_texels;
    info->tile_w = s->fr.tile_w; info->tile_h = s->fr.tile_h;
    info->device_bytes = s->blob_bytes;
    return QR_OK;
}

extern "C" int qr_scene_set_depth(qr_device_scene *s, int depth)
{
    QR_TRY(need_scene(s));
    if (depth < 0 || depth > QR_MAX_DEPTH) return qr_fail(QR_ERR_ARG, "depth must be 0..10 (RT_STACK_DEPTH)");
    s->lp.depth = depth;
    return QR_OK;
}

/*
 * Path-tracer mode on / off.  Turning it on (re)starts the accumulation: the engine's seed plane (pt_seed_plane), colour planes 0.
 */
extern "C" int qr_scene_set_pt(qr_device_scene *s, int on)
{
    QR_TRY(need_scene(s));
    HIP_TRY(hipSetDevice(s->device));
    if (!on) { s->pt_on = false; return QR_OK; }
    const size_t n = (size_t)s->fr.frm_row * s->fr.frm_h * ((size_t)1 << s->fr.fsaa);
    if (s->fr.frm_row < s->fr.frm_w || n == 0 || n > ((size_t)1 << 30)) return qr_fail(QR_ERR_ARG, "bad frame stride for the sample planes");
    if (s->d_seeds == nullptr || s->d_acc == nullptr)
    {
        /* both planes or neither: a half-built pair would be taken for a finished one by the next call */
        uint32_t *seeds_dev = nullptr; float *acc_dev = nullptr;
        HIP_TRY(hipMalloc((void **)&seeds_dev, n * sizeof(uint32_t)));
        const hipError_t ea = hipMalloc((void **)&acc_dev, 3 * n * sizeof(float));
        if (ea != hipSuccess) { (void)hipFree(seeds_dev); return qr_fail(QR_ERR_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(ea)); }
        (void)hipFree(s->d_seeds); (void)hipFree(s->d_acc);
        s->d_seeds = seeds_dev; s->d_acc = acc_dev;
    }
    const std::vector<uint32_t> seeds = pt_seed_plane(n);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(s->d_seeds, seeds.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(s->d_acc, 0, 3 * n * sizeof(float)));
    s->pt_frames = 0;
    s->pt_on = true;
    s->pt_eager = on == 2 ? 1 : (on == 3 ? 3 : 0);
    return QR_OK;
}

extern "C" int qr_scene_set_rows(qr_device_scene *s, int row_begin, int row_end, int index, int thnum)
{
    QR_TRY(need_scene(s));
    const int h = s->fr.frm_h;
    if (row_begin < 0 || row_end > h || row_begin > row_end) return qr_fail(QR_ERR_ARG, "bad row range");
    if (thnum <= 0 || index < 0 || index >= thnum) return qr_fail(QR_ERR_ARG, "bad index/thnum");
    s->lp.row_begin = row_begin; s->lp.row_end = row_end;
    s->lp.index = index; s->lp.thnum = thnum;
    s->lp.group_first = row_begin / 8;
    s->lp.group_stride = 1;
    s->n_groups = row_end > row_begin ? (row_end - 1) / 8 - row_begin / 8 + 1 : 0;
    return QR_OK;
}

extern "C" int qr_scene_set_tile_rows(qr_device_scene *s, int first, int stride)
{
    QR_TRY(need_scene(s));
    const int total = (s->fr.frm_h + 7) / 8;
    if (stride <= 0 || first < 0) return qr_fail(QR_ERR_ARG, "bad tile-row selection");
    s->lp.row_begin = 0; s->lp.row_end = s->fr.frm_h;
    s->lp.index = 0; s->lp.thnum = 1;
    s->lp.group_first = first; s->lp.group_stride = stride;
    s->n_groups = first < total ? (total - first + stride - 1) / stride : 0;
    return QR_OK;
}


extern "C" int qr_render_async(qr_device_scene *s, void *frame_dev, void *stream)
{
    if (s == nullptr || frame_dev == nullptr) return qr_fail(QR_ERR_ARG, "null argument");
    QR_TRY(pt_rows_ok(s));
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(launch<false>(s, frame_dev, nullptr, (hipStream_t)stream));
    return QR_OK;
}

extern "C" int qr_render_ids_async(qr_device_scene *s, void *frame_dev, void *ids_dev, void *stream)
{
    if (s == nullptr || frame_dev == nullptr) return qr_fail(QR_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(launch<false>(s, frame_dev, (int32_t *)ids_dev, (hipStream_t)stream));
    return QR_OK;
}

/* ---- the ray API: queries, shading, views, path-traced rays and views, filter, hit records, fans, layers ---- */
#include "qr_rayapi.hpp"
#include "qr_dev_diag.hpp"

extern "C" int qr_render_count(qr_device_scene *s, void *frame_dev, void *stream, qr_ray_counts *counts)
{
    if (s == nullptr || frame_dev == nullptr || counts == nullptr) return qr_fail(QR_ERR_ARG, "null argument");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemsetAsync(s->d_counters, 0, QR_COUNTER_HEAD * sizeof(unsigned long long), st));
    HIP_TRY(launch<true>(s, frame_dev, nullptr, st));
    unsigned long long h[4];
    HIP_TRY(hipMemcpyAsync(h, s->d_counters, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    counts->primary = h[0]; counts->shadow = h[1]; counts->reflect = h[2]; counts->refract = h[3];
    return diag_print_counters(s);
}

extern "C" int qr_render_timed(qr_device_scene *s, void *frame_dev, void *stream,
                               int iters, float *avg_ms, float *min_ms)
{
    if (s == nullptr || frame_dev == nullptr || iters <= 0) return qr_fail(QR_ERR_ARG, "bad argument");
    QR_TRY(pt_rows_ok(s));
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(s->device));
    double sum = 0.0; float mn = 1e30f;
    if (s->ev0 == nullptr) { HIP_TRY(hipEventCreate(&s->ev0)); HIP_TRY(hipEventCreate(&s->ev1)); }
    for (int i = 0; i < iters; i++)
    {
        QR_TRY(diag_wavetime_clear(s, st));
        HIP_TRY(hipEventRecord(s->ev0, st));
        HIP_TRY(launch<false>(s, frame_dev, nullptr, st));
        HIP_TRY(hipEventRecord(s->ev1, st));
        HIP_TRY(hipEventSynchronize(s->ev1));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
        sum += ms; if (ms < mn) mn = ms;
    }
    if (avg_ms) *avg_ms = (float)(sum / iters);
    if (min_ms) *min_ms = mn;
    return diag_wavetime_dump(s);
}

#include "qr_dev_host.hpp"
#include "qr_dropin.hpp"
