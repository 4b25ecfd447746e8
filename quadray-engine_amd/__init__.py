"""quadray-engine_amd: Python binding of libqrhip.so (the C ABI in include/qrhip.h).

The directory name is not a valid Python identifier, so import it by path
(tests/conftest.py, bench.py and __graft_entry__.py use `load_package()` from
the repository root helper `qr_loader.py`).

PyTorch is used only for device memory, streams and torch.distributed; every
pixel is computed by the hand-written HIP kernel behind the C ABI.  There is
no CPU fallback: without the shared library or without a GPU these calls raise.
"""
import ctypes
import gzip
import math
import numbers
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QR_LIB") or os.path.join(_HERE, "libqrhip.so")   # QR_LIB: A/B experiment builds

# every symbol include/qrhip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "qr_render0", "qr_capture_snapshot", "qr_flatten", "qr_free",
    "qr_scene_upload", "qr_scene_upload_ex", "qr_program_stats", "qr_program_stats_ex", "qr_snapshot_build_lists_c", "qr_scene_destroy", "qr_scene_get_info", "qr_scene_set_depth", "qr_scene_set_pt",
    "qr_scene_set_rows", "qr_scene_set_tile_rows", "qr_render_async", "qr_render_multi_async", "qr_render_ids_async",
    "qr_render_count", "qr_render_host", "qr_render_timed", "qr_trace_rays_async", "qr_occluded_async",
    "qr_shade_rays_async", "qr_render_views_async", "qr_render_views_mean_async",
    "qr_pt_views_state_bytes", "qr_pt_views_reset", "qr_pt_views_async",
    "qr_pt_rays_state_bytes", "qr_pt_rays_reset", "qr_pt_rays_async",
    "qr_pt_adapt_state_bytes", "qr_pt_adapt_reset", "qr_pt_adapt_rays_async",
    "qr_pt_adapt_views_state_bytes", "qr_pt_adapt_views_reset", "qr_pt_adapt_views_async",
    "qr_pt_adapt_list_work_bytes", "qr_pt_adapt_open_list_async", "qr_pt_adapt_list_rays_async", "qr_hit_rays_async", "qr_hit_views_async",
    "qr_fan_rays_async", "qr_fan_views_async", "qr_fan_hits_async", "qr_layer_rays_async", "qr_layer_views_async",
    "qr_gather_rays_async", "qr_gather_views_async", "qr_gather_hits_async",
    "qr_fan_rays_framed_async", "qr_fan_views_framed_async", "qr_fan_hits_framed_async",
    "qr_gather_rays_framed_async", "qr_gather_views_framed_async", "qr_gather_hits_framed_async",
    "qr_atrous_views_async", "qr_pt_adapt_views_variance_async", "qr_reproject_views_async", "qr_reproject_moving_async",
    "qr_reproject_clamped_async",
    "qr_upsample_views_async",
    "qr_frame_register", "qr_frame_unregister",
    "qr_frame_hash", "qr_last_error", "qr_version", "qr_device_count", "qr_kernel_name", "qr_capture_index",
    # include/qr_hierarchy.h
    "qr_hierarchy_update", "qr_hierarchy_animate", "qr_hierarchy_apply", "qr_hierarchy_bounds", "qr_anim_spin", "qr_anim_swing",
]


UPLOAD_REBIN_TILES = 1
UPLOAD_RAY_QUERIES = 2      # also compile the global list for Scene.trace / Scene.occluded
TRACE_COHERENT = 1          # qr_trace_rays_async / qr_occluded_async flag: consecutive rays are neighbours
MEAN_RESUME = 1             # qr_render_views_mean_async flag: the sum starts from the `sum` buffer's contents
FAN_FLIP = 2                # qr_fan_*_async flag: every direction is traced, mirrored into the normal's hemisphere
FAN_MAX_DIRS = 1024         # QR_FAN_MAX_DIRS
GATHER_COSINE = 4           # qr_gather_*_async flag: a direction's weight is weight * |nrm . d| (weight * (nrm . d) without FAN_FLIP)
GATHER_RESUME = 8           # qr_gather_*_async flag: the sums and counts start from the output buffers' contents
PT_VIEWS_MAX_SAMPLES = 512  # QR_PT_VIEWS_MAX_SAMPLES: the most samples of one qr_pt_views_async launch
PT_VIEWS_STATE_WORDS = 4    # QR_PT_VIEWS_STATE_WORDS: 32-bit planes per view of a path-traced view state
PT_RAYS_MAX_SAMPLES = 512   # QR_PT_RAYS_MAX_SAMPLES: the most samples of one qr_pt_rays_async launch
PT_RAYS_STATE_WORDS = 4     # QR_PT_RAYS_STATE_WORDS: 32-bit planes of a path-traced ray state
PT_ADAPT_MAX_SAMPLES = 512  # QR_PT_ADAPT_MAX_SAMPLES: the most candidate samples of one qr_pt_adapt_rays_async launch
PT_ADAPT_STATE_WORDS = 8    # QR_PT_ADAPT_STATE_WORDS: 32-bit planes of an adaptive path-traced ray state
PT_ADAPT_VIEWS_MAX_SAMPLES = 512    # QR_PT_ADAPT_VIEWS_MAX_SAMPLES: the most candidate samples of one qr_pt_adapt_views_async launch
PT_OPEN_BLOCK = 1024        # QR_PT_OPEN_BLOCK: rays per workgroup of the open-list kernels
PT_OPEN_CHUNK = 1024        # QR_PT_OPEN_CHUNK: block counts one pass of the open list's scan workgroup takes
LAYER_MAX = 64              # QR_LAYER_MAX: the most layers of one qr_layer_*_async call
ATROUS_NORMAL = 1           # qr_atrous_views_async flags: the normal stop,
ATROUS_PLANE = 2            # the plane-distance stop,
ATROUS_LUMA = 4             # the luminance stop against the variance,
ATROUS_DEMODULATE = 8       # every colour read is divided by its own pixel's albedo,
ATROUS_MODULATE = 16        # the output is multiplied by the centre pixel's albedo
ATROUS_MAX_STEP = 64        # QR_ATROUS_MAX_STEP: the widest tap spacing of one pass
REPROJ_DEMODULATE = 1       # qr_reproject_views_async flag: this frame's colour is divided by its own pixel's albedo
CLAMP_MINMAX = 1            # qr_reproject_clamped_async flags: the box is the neighbourhood's minimum and maximum,
CLAMP_VARIANCE = 2          # or its mean +- gamma standard deviations (exactly one of the two);
CLAMP_SHORTEN = 4           # a pixel whose history was moved has its history length cut to short_len
CLAMP_MAX_RADIUS = 3        # QR_CLAMP_MAX_RADIUS: the widest neighbourhood of the box
UPSAMPLE_NORMAL = 1         # qr_upsample_views_async flags: the normal stop,
UPSAMPLE_PLANE = 2          # the plane-distance stop,
UPSAMPLE_SAME_ID = 4        # a tap must be the pixel's own surface and side,
UPSAMPLE_DEMODULATE = 8     # the coarse colour is divided by the albedo of its guide record,
UPSAMPLE_MODULATE = 16      # the result is multiplied by the full pixel's albedo
UPSAMPLE_MAX_FACTOR = 16    # QR_UPSAMPLE_MAX_FACTOR: the coarsest lattice


class QrError(RuntimeError):
    pass


class SceneInfo(ctypes.Structure):
    _fields_ = [("frm_w", ctypes.c_int32), ("frm_h", ctypes.c_int32), ("fsaa", ctypes.c_int32),
                ("depth", ctypes.c_int32), ("n_srf", ctypes.c_int32), ("n_mat", ctypes.c_int32),
                ("n_lgt", ctypes.c_int32), ("n_elm", ctypes.c_int32), ("n_tiles", ctypes.c_int32),
                ("n_texels", ctypes.c_int32), ("tile_w", ctypes.c_int32), ("tile_h", ctypes.c_int32),
                ("device_bytes", ctypes.c_uint64)]


class ProgramInfo(ctypes.Structure):
    _fields_ = [("bytes", ctypes.c_uint64), ("n_lists", ctypes.c_uint32), ("n_cells", ctypes.c_uint32),
                ("n_dropped", ctypes.c_uint32), ("n_clip_cells", ctypes.c_uint32), ("n_sched", ctypes.c_uint32),
                ("n_grids", ctypes.c_uint32), ("n_grid_lists", ctypes.c_uint32), ("n_dda", ctypes.c_uint32),
                ("n_pgrids", ctypes.c_uint32), ("n_pgrid_nodes", ctypes.c_uint32)]


class AtrousParams(ctypes.Structure):
    """qr_atrous_params (include/qrhip.h), 32 bytes"""
    _fields_ = [("step", ctypes.c_int32), ("channels", ctypes.c_int32), ("normal_sq", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("sigma_z", ctypes.c_float), ("sigma_l2", ctypes.c_float), ("eps_l", ctypes.c_float), ("alb_floor", ctypes.c_float)]


class ReprojectParams(ctypes.Structure):
    """qr_reproject_params (include/qrhip.h), 64 bytes"""
    _fields_ = [("channels", ctypes.c_int32), ("flags", ctypes.c_uint32), ("off_x", ctypes.c_float), ("off_y", ctypes.c_float),
                ("normal_min", ctypes.c_float), ("plane_max", ctypes.c_float), ("min_weight", ctypes.c_float),
                ("alpha_min", ctypes.c_float), ("alpha_mom_min", ctypes.c_float), ("max_len", ctypes.c_float),
                ("var_min_len", ctypes.c_float), ("unknown", ctypes.c_float), ("alb_floor", ctypes.c_float),
                ("reserved", ctypes.c_uint32 * 3)]


class ClampParams(ctypes.Structure):
    """qr_clamp_params (include/qrhip.h), 32 bytes"""
    _fields_ = [("flags", ctypes.c_uint32), ("radius", ctypes.c_int32), ("gamma", ctypes.c_float), ("short_len", ctypes.c_float),
                ("reserved", ctypes.c_uint32 * 4)]


class Motion(ctypes.Structure):
    """qr_motion (include/qrhip.h), 48 bytes: one row of hierarchy_motion's table"""
    _fields_ = [("row", (ctypes.c_float * 4) * 3)]


class UpsampleParams(ctypes.Structure):
    """qr_upsample_params (include/qrhip.h), 32 bytes"""
    _fields_ = [("factor", ctypes.c_int32), ("phase_x", ctypes.c_int32), ("phase_y", ctypes.c_int32), ("channels", ctypes.c_int32),
                ("normal_sq", ctypes.c_int32), ("flags", ctypes.c_uint32), ("sigma_z", ctypes.c_float), ("alb_floor", ctypes.c_float)]


class RayCounts(ctypes.Structure):
    _fields_ = [("primary", ctypes.c_uint64), ("shadow", ctypes.c_uint64),
                ("reflect", ctypes.c_uint64), ("refract", ctypes.c_uint64)]

    def total(self):
        return self.primary + self.shadow + self.reflect + self.refract

    def as_dict(self):
        return dict(primary=self.primary, shadow=self.shadow, reflect=self.reflect, refract=self.refract)


_lib = None


def lib():
    """Load libqrhip.so (fails loudly if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise QrError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(the gfx950 backend has no fallback path)")
    try:
        # load torch's bundled HIP runtime first so that libqrhip.so binds to the same libamdhip64
        # (two HIP runtimes in one process cannot both own the device)
        import torch  # noqa: F401
    except Exception:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, ci, cu64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    L.qr_last_error.restype = ctypes.c_char_p
    L.qr_version.restype = ctypes.c_char_p
    L.qr_kernel_name.restype = ctypes.c_char_p
    L.qr_device_count.restype = ci
    L.qr_scene_upload.argtypes = [vp, cu64, ci, ctypes.POINTER(vp)]
    L.qr_scene_upload_ex.argtypes = [vp, cu64, ci, ctypes.c_uint32, ctypes.POINTER(vp)]
    L.qr_scene_destroy.argtypes = [vp]
    L.qr_program_stats.argtypes = [vp, cu64, ctypes.POINTER(ProgramInfo)]
    L.qr_program_stats_ex.argtypes = [vp, cu64, ctypes.c_uint32, ctypes.POINTER(ProgramInfo)]
    # the ray API: a call's list is a head -- (scene, rays or records, n) or (scene, views, n_views, width, height) --, what is
    # its own, and the tail (flags, stream)
    i64, u32, cf = ctypes.c_int64, ctypes.c_uint32, ctypes.c_float
    rays, views = [vp, vp, i64], [vp, vp, ci, ci, ci]
    ray_api = {
        "qr_trace_rays": rays + [vp, vp], "qr_occluded": rays + [vp], "qr_shade_rays": rays + [vp, vp],
        "qr_render_views": views + [vp, vp, vp], "qr_render_views_mean": views + [vp, vp, cf],
        "qr_pt_views": views + [vp, ci, ci, vp, vp],
        "qr_pt_adapt_views": views + [vp, ci, ci, ci, cf, vp, vp, vp, vp], "qr_pt_adapt_views_variance": views + [cf, vp],
        "qr_pt_adapt_open_list": rays + [ci, ci, cf, vp, vp, vp],
        "qr_hit_rays": rays + [vp], "qr_hit_views": views + [vp],
        "qr_layer_rays": rays + [ci, vp, vp, vp, vp], "qr_layer_views": views + [ci, vp, vp, vp, vp],
    }
    for src, head in (("rays", rays), ("hits", rays), ("views", views)):
        for kind in ("fan", "gather"):
            ray_api[f"qr_{kind}_{src}"] = head + [vp, ci, cf, cf, vp, vp]
            ray_api[f"qr_{kind}_{src}_framed"] = head + [vp, ci, vp, cf, cf, vp, vp]       # the spin plane after k
    for name, args in ray_api.items():
        getattr(L, name + "_async").argtypes = args + [u32, vp]
    # rays and spread in front of n; the state queries and resets have neither flags nor a stream
    L.qr_pt_rays_async.argtypes = [vp, vp, vp, i64, vp, ci, ci, vp, u32, vp]
    L.qr_pt_adapt_rays_async.argtypes = [vp, vp, vp, i64, vp, ci, ci, ci, cf, vp, vp, u32, vp]
    L.qr_pt_adapt_list_rays_async.argtypes = [vp, vp, vp, i64, vp, vp, vp, i64, ci, ci, ci, cf, vp, vp, u32, vp]
    for name, head in (("qr_pt_views", views[2:]), ("qr_pt_adapt_views", views[2:]), ("qr_pt_rays", [i64]), ("qr_pt_adapt", [i64])):
        getattr(L, name + "_state_bytes").argtypes = [vp] + head + [ctypes.POINTER(cu64)]
        getattr(L, name + "_reset").argtypes = [vp] + head + [vp]
    L.qr_pt_adapt_list_work_bytes.argtypes = [vp, i64, ctypes.POINTER(cu64)]
    L.qr_atrous_views_async.argtypes = [vp, vp, vp, vp, ci, ci, ci, ctypes.POINTER(AtrousParams), vp, vp, vp]
    L.qr_reproject_views_async.argtypes = [vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ctypes.POINTER(ReprojectParams), vp, vp, vp, vp, vp]
    L.qr_reproject_moving_async.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ctypes.POINTER(ReprojectParams), vp, vp, vp, vp, vp]
    L.qr_reproject_clamped_async.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ctypes.POINTER(ReprojectParams),
                                             ctypes.POINTER(ClampParams), vp, vp, vp, vp, vp, vp]
    L.qr_upsample_views_async.argtypes = [vp, vp, vp, vp, ci, ci, ci, ctypes.POINTER(UpsampleParams), vp, vp, vp, vp]
    L.qr_snapshot_build_lists_c.argtypes =[vp, cu64, ctypes.POINTER(vp), ctypes.POINTER(cu64)]
    L.qr_free.argtypes = [vp]
    L.qr_frame_hash.argtypes = [vp, cu64]
    L.qr_frame_hash.restype = cu64
    L.qr_scene_get_info.argtypes = [vp, ctypes.POINTER(SceneInfo)]
    L.qr_scene_set_depth.argtypes = [vp, ci]
    L.qr_scene_set_pt.argtypes = [vp, ci]
    L.qr_scene_set_rows.argtypes = [vp, ci, ci, ci, ci]
    L.qr_scene_set_tile_rows.argtypes = [vp, ci, ci]
    L.qr_render_async.argtypes = [vp, vp, vp]
    L.qr_render_ids_async.argtypes = [vp, vp, vp, vp]
    L.qr_render_multi_async.argtypes = [ci, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(ci), ctypes.POINTER(ci), vp]
    L.qr_render_count.argtypes = [vp, vp, vp, ctypes.POINTER(RayCounts)]
    L.qr_render_host.argtypes = [vp, vp, ci]
    L.qr_frame_register.argtypes = [vp, ctypes.c_uint64]
    L.qr_frame_unregister.argtypes = [vp]
    L.qr_render_timed.argtypes = [vp, vp, vp, ci, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.qr_hierarchy_update.argtypes = [vp, ci, ctypes.c_uint32, vp]
    L.qr_hierarchy_bounds.argtypes = [vp, cu64, vp, ci, ctypes.c_uint32, vp]
    L.qr_hierarchy_animate.argtypes = [vp, ci, ctypes.c_int64, vp, vp, vp, ci]
    L.qr_hierarchy_apply.argtypes = [vp, cu64, vp, vp, ci, ctypes.c_uint32, ci, ctypes.c_uint32, ctypes.POINTER(vp), ctypes.POINTER(cu64)]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise QrError(f"qrhip error {rc}: {lib().qr_last_error().decode()}")


# ---- the binding's glue: every tensor check, output rule and argument rule is stated once ----

# what the helpers need of torch, by dtype name and by device index, looked up once: torch is imported lazily
_DTYPES, _DEVICES = {}, {}


def _dtypes(name):
    """(torch.Tensor, the torch dtypes a name such as "float32" or "int32 or uint32" stands for); a torch without uint32 takes
    int32 for it"""
    import torch
    found = tuple(getattr(torch, d, torch.int32) if d == "uint32" else getattr(torch, d) for d in name.split(" or "))
    dt = _DTYPES[name] = (torch.Tensor, found)
    return dt


def _ptr(t):
    """what a c_void_p slot takes for a tensor: its address, None for None"""
    return None if t is None else t.data_ptr()


def _fits(t, dtype, shape, dev=None, contiguous=True):
    """The residency predicate: is t a tensor of `dtype` (see _dtypes) and `shape`, contiguous, on cuda:dev?  In a shape None
    stands for any size and a leading ... for any number of dimensions, at least one; no shape at all: any.  dev=None asks
    for dtype and shape alone, dtype=None (of a tensor known to be one) for contiguity and device alone.  One function and
    the exact shape first: it runs several times in every call of the ray API."""
    if dtype is not None:
        tensor, dtypes = _DTYPES.get(dtype) or _dtypes(dtype)
        if not (isinstance(t, tensor) and t.dtype in dtypes):
            return False
        got = t.shape
        if not (got == shape or shape is None):
            if shape[0] is ...:
                if not (len(got) >= len(shape) and got[1 - len(shape):] == shape[1:]):
                    return False
            elif len(got) != len(shape):
                return False
            else:
                for want, have in zip(shape, got):
                    if want is not None and want != have:
                        return False
    return dev is None or ((t.is_contiguous() or not contiguous) and t.is_cuda and t.device.index == dev)


def _need(name, t, dtype, shape, dev, lead="a", suffix="", error=QrError):
    """t when it fits, else the refusal, built from the same parts"""
    if _fits(t, dtype, shape, dev):
        return t
    label = "[" + ", ".join("N" if s is None else "..." if s is ... else str(s) for s in shape) + "]"
    raise error(f"{name} must be {lead} contiguous {dtype} {label} tensor on cuda:{dev}{suffix}")


def _device(dev):
    """(torch.empty, the device cuda:dev)"""
    import torch
    made = _DEVICES[dev] = (torch.empty, torch.device("cuda", dev))
    return made


def _new(dtype, shape, dev):
    empty, device = _DEVICES.get(dev) or _device(dev)
    return empty(shape, dtype=(_DTYPES.get(dtype) or _dtypes(dtype))[1][0], device=device)


def _fill(name, t, dtype, shape, dev):
    """an output that is None (a new tensor: every element is written) or a tensor to fill"""
    return _new(dtype, shape, dev) if t is None else _need(name, t, dtype, shape, dev)


def _wanted(name, t, dtype, shape, dev):
    """an output that is True (a new tensor), False or None (not wanted: None) or a tensor to fill"""
    if t is True:
        return _new(dtype, shape, dev)
    if t is False or t is None:
        return None
    return _need(name, t, dtype, shape, dev, lead="True, False or a")


# The image filters (atrous, denoise, upsample, reproject, Temporal.step): dtype and shape of every tensor first, then the
# residency of all of them.  `error`: QrError, or ValueError for upsample.

def _stops(fn, error, **kw):
    """the stops of a filter through rays.<fn> (atrous_stops, upsample_stops, reproject_stops): what that refuses, as `error`"""
    from . import rays
    try:
        return getattr(rays, fn)(**kw)
    except (ValueError, TypeError) as e:
        raise error(str(e)) from None


def _plane(name, t, shape, error):
    """an optional float32 tensor of a filter, an input or an output: dtype and shape alone"""
    if t is not None and not _fits(t, "float32", shape):
        raise error(f"{name} must be None or a float32 {list(shape)} tensor")


def _frame_inputs(colour, hits, variance, error=QrError, lattice=None):
    """The frame inputs of a filter, dtype and shape alone: colour [N, H, W, 3|4], hits [N, H, W, 12], variance None or [N, H, W].
    lattice=(factor, phase): colour (called colour_lo) and variance are the coarse frame of the full frame of hits, which then
    comes first.  Returns (n, h, w, channels) of the full frame."""
    if lattice is None:
        if not (_fits(colour, "float32", (None, None, None, None)) and colour.shape[3] in (3, 4) and min(colour.shape) >= 1):
            raise error("colour must be a float32 [N, H, W, 3] or [N, H, W, 4] tensor")
        n, h, w, ch = (int(x) for x in colour.shape)
        if not _fits(hits, "float32", (n, h, w, 12)):
            raise error(f"hits must be a float32 [{n}, {h}, {w}, 12] tensor of qr_hit records (view_hits)")
        lo = (n, h, w)
    else:
        from . import rays
        if not (_fits(hits, "float32", (None, None, None, 12)) and min(hits.shape) >= 1):
            raise error("hits must be a float32 [N, H, W, 12] tensor of qr_hit records (view_hits) of the FULL frame")
        n, h, w = (int(x) for x in hits.shape[:3])
        wl, hl = rays.coarse_size(w, h, *lattice)
        if not (_fits(colour, "float32", (n, hl, wl, None)) and colour.shape[3] in (3, 4)):
            raise error(f"colour_lo must be a float32 [{n}, {hl}, {wl}, 3] or [{n}, {hl}, {wl}, 4] tensor: the coarse frame of "
                        f"a {w} x {h} frame at factor {lattice[0]}, phase {tuple(lattice[1])} (rays.coarse_size)")
        ch, lo = int(colour.shape[3]), (n, hl, wl)
    _plane("variance", variance, lo, error)
    return n, h, w, ch


def _resident(dev, error, *tensors):
    """the residency pass: every (tensor, name) that is given is contiguous and on cuda:dev"""
    for t, what in tensors:
        if t is not None and not _fits(t, None, None, dev):
            raise error(f"{what} must be contiguous and on cuda:{dev}")


_FAN_FNS = {}       # (fan | gather, rays | hits | views, plain) -> the library's entry point, looked up once


def _fan_fn(what, kind, plain):
    """qr_{fan|gather}_{rays|hits|views}{_framed}_async"""
    fn = _FAN_FNS[what, kind, plain] = getattr(lib(), f"qr_{what}_{kind}{'' if plain else '_framed'}_async")
    return fn


def _dirs_arg(dirs, eps, reach, pad, dev):
    """(dirs as a contiguous float32 [K, 4] tensor, K, eps, reach) of a fan call; a [K, 3] table gets `pad` in column 3.
    dirs need not be contiguous: they are made so"""
    if not (_fits(dirs, "float32", (None, None), dev, contiguous=False) and dirs.shape[1] in (3, 4)):
        raise QrError(f"dirs must be a float32 [K, 3] or [K, 4] tensor on cuda:{dev}")
    k = dirs.shape[0]
    if not 1 <= k <= FAN_MAX_DIRS:
        raise QrError(f"dirs must hold 1..{FAN_MAX_DIRS} directions, got {k}")
    if eps is None or math.isnan(eps) or math.isnan(reach):
        raise QrError("eps (the step off the surface, in units of |dir|) is required; eps and reach must not be NaN")
    if dirs.shape[1] == 3:
        import torch
        d4 = torch.full((k, 4), pad, dtype=torch.float32, device=dirs.device)
        d4[:, 0:3] = dirs
    else:
        d4 = dirs.contiguous()
    return d4, k, float(eps), float(reach)


def read_snapshot(path):
    """Return the raw snapshot bytes of a .qrs or .qrs.gz file."""
    with open(path, "rb") as f:
        raw = f.read()
    return gzip.decompress(raw) if path.endswith(".gz") else raw


def frame_register(arr):
    """qr_frame_register on a numpy array the caller keeps alive until frame_unregister(arr)."""
    _check(lib().qr_frame_register(arr.ctypes.data_as(ctypes.c_void_p), arr.nbytes))


def frame_unregister(arr):
    _check(lib().qr_frame_unregister(arr.ctypes.data_as(ctypes.c_void_p)))


def frame_hash(frame):
    """FNV-1a-64 fingerprint of a frame (numpy uint32 array or CUDA int32 tensor), as in tests/golden/manifest.json."""
    import numpy as np
    if hasattr(frame, "cpu"):
        frame = frame.cpu().numpy()
    f = np.ascontiguousarray(frame).view(np.uint32)
    return int(lib().qr_frame_hash(f.ctypes.data_as(ctypes.c_void_p), f.size))


def build_lists(blob):
    """Per-surface shadow / reflection / light lists from the global list (host pass, no GPU): returns a new snapshot."""
    out, n = ctypes.c_void_p(), ctypes.c_uint64()
    buf = ctypes.create_string_buffer(blob, len(blob))
    _check(lib().qr_snapshot_build_lists_c(buf, len(blob), ctypes.byref(out), ctypes.byref(n)))
    try:
        return ctypes.string_at(out, n.value)
    finally:
        lib().qr_free(out)


# ---- object hierarchy (include/qr_hierarchy.h): numpy record arrays in the C layout of qr_node / qr_node_state ----

def node_dtype():
    import numpy as np
    return np.dtype([("parent", "<i4"), ("tag", "<i4"), ("scl", "<f4", 3), ("rot", "<f4", 3), ("pos", "<f4", 3),
                     ("shape", "<f4", 3), ("srf", "<i4"), ("inb", "<i4"), ("bvb", "<i4"), ("lgt", "<i4"), ("anim", "<i4"),
                     ("pov", "<f4"), ("bvnode", "<i4"), ("nverts", "<i4"), ("lmin", "<f4", 3), ("lmax", "<f4", 3),
                     ("tex", "<f4", 8), ("has_tex", "<i4"), ("pad_", "<i4", 3)])


def node_bounds_dtype():
    import numpy as np
    return np.dtype([("bmin", "<f4", 3), ("bmax", "<f4", 3), ("cmin", "<f4", 3), ("cmax", "<f4", 3), ("mid", "<f4", 3), ("rad", "<f4"),
                     ("nverts", "<i4"), ("inmin", "<f4", 3), ("inmax", "<f4", 3), ("inmid", "<f4", 3), ("inrad", "<f4"),
                     ("trmin", "<f4", 3), ("trmax", "<f4", 3), ("trrad", "<f4"), ("inb_form", "<i4"), ("bvb_form", "<i4")])


def node_state_dtype():
    import numpy as np
    return np.dtype([("mtx", "<f4", 16), ("map", "<i4", 4), ("sgn", "<i4", 4), ("scl", "<f4", 4), ("trnode", "<i4"),
                     ("obj_has_trm", "<i4"), ("mtx_has_trm", "<i4"), ("pad", "<i4")])


HIER_RESET_TILES = 1
HIER_BOUNDS = 2
HIER_REGROUP = 4
ANIM_SPIN, ANIM_SWING = "spin", "swing"


def hierarchy_update(nodes, opts):
    """Hierarchical transform update (qr_hierarchy_update): nodes (node_dtype array) -> node_state_dtype array."""
    import numpy as np
    nodes = np.ascontiguousarray(nodes, dtype=node_dtype())
    out = np.zeros(len(nodes), dtype=node_state_dtype())
    _check(lib().qr_hierarchy_update(nodes.ctypes.data_as(ctypes.c_void_p), len(nodes), opts, out.ctypes.data_as(ctypes.c_void_p)))
    return out


def hierarchy_bounds(blob, nodes, opts):
    """Bounding and clipping boxes of every node (qr_hierarchy_bounds): node_bounds_dtype array."""
    import numpy as np
    nodes = np.ascontiguousarray(nodes, dtype=node_dtype())
    out = np.zeros(len(nodes), dtype=node_bounds_dtype())
    buf = ctypes.create_string_buffer(blob, len(blob))
    _check(lib().qr_hierarchy_bounds(buf, len(blob), nodes.ctypes.data_as(ctypes.c_void_p), len(nodes), opts, out.ctypes.data_as(ctypes.c_void_p)))
    return out


class _AnimParams(ctypes.Structure):
    _fields_ = [("axis", ctypes.c_int32), ("rate", ctypes.c_float), ("period", ctypes.c_float), ("pad", ctypes.c_int32)]


def hierarchy_animate(nodes, time, node_time, animators):
    """Run the animators (qr_hierarchy_animate) in place on nodes / node_time (int64 array, -1 = never updated).
    animators[k] is (ANIM_SPIN, axis, rate), (ANIM_SWING, axis, rate, period) or a Python callable
    f(time, last_time, trm) with trm a 9-float numpy view (scl, rot, pos) it changes in place."""
    import numpy as np
    assert nodes.dtype == node_dtype() and nodes.flags["C_CONTIGUOUS"] and node_time.dtype == np.int64
    proto = ctypes.CFUNCTYPE(None, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_float), ctypes.c_void_p)
    n = len(animators)
    fns, users, keep = (ctypes.c_void_p * max(n, 1))(), (ctypes.c_void_p * max(n, 1))(), []
    for k, a in enumerate(animators):
        if callable(a):
            cb = proto(lambda t, lt, trm, _u, a=a: a(t, lt, np.ctypeslib.as_array(trm, shape=(9,))))
            keep.append(cb)
            fns[k] = ctypes.cast(cb, ctypes.c_void_p).value
        else:
            prm = _AnimParams(int(a[1]), float(a[2]), float(a[3]) if len(a) > 3 else 0.0, 0)
            keep.append(prm)
            fns[k] = ctypes.cast(lib().qr_anim_spin if a[0] == ANIM_SPIN else lib().qr_anim_swing, ctypes.c_void_p).value
            users[k] = ctypes.addressof(prm)
    _check(lib().qr_hierarchy_animate(nodes.ctypes.data_as(ctypes.c_void_p), len(nodes), int(time),
                                      node_time.ctypes.data_as(ctypes.c_void_p), fns, users, n))


def hierarchy_apply(blob, nodes, opts, camera=-1, base=None, flags=0):
    """Write the transform fields the nodes imply into a copy of the snapshot (qr_hierarchy_apply); base: the nodes the
    snapshot was captured with (enables the scope checks).  Rebuild the lists afterwards (build_lists)."""
    import numpy as np
    nodes = np.ascontiguousarray(nodes, dtype=node_dtype())
    bp = None
    if base is not None:
        base = np.ascontiguousarray(base, dtype=node_dtype())
        assert len(base) == len(nodes)
        bp = base.ctypes.data_as(ctypes.c_void_p)
    out, n = ctypes.c_void_p(), ctypes.c_uint64()
    buf = ctypes.create_string_buffer(blob, len(blob))
    _check(lib().qr_hierarchy_apply(buf, len(blob), bp, nodes.ctypes.data_as(ctypes.c_void_p), len(nodes), opts, camera, flags,
                                    ctypes.byref(out), ctypes.byref(n)))
    try:
        return ctypes.string_at(out, n.value)
    finally:
        lib().qr_free(out)


def hierarchy_records_after_apply(blob, nodes, opts):
    """The node table as it stands after hierarchy_apply(blob, nodes, ...): an array that became the transform node of surfaces
    and had no record got one -- the k-th such array in node order holds record n_srf + k (include/qr_hierarchy.h).  Use it
    as `base` (and for `srf` of the next table) when the patched snapshot is patched again."""
    import struct
    import numpy as np
    nodes = np.ascontiguousarray(nodes, dtype=node_dtype()).copy()
    st = hierarchy_update(nodes, opts)
    n_srf = struct.unpack_from("<I", blob, 16)[0]
    heads = set()
    for i in range(len(nodes)):
        t = int(st[i]["trnode"])
        if 0 <= nodes[i]["tag"] < 9 and nodes[i]["srf"] >= 0 and t >= 0 and t != i:
            heads.add(t)
    for g in sorted(heads):
        if nodes[g]["srf"] < 0:
            nodes[g]["srf"] = n_srf
            n_srf += 1
    return nodes


def hierarchy_motion(nodes_prev, nodes_cur, opts, n_srf):
    """The motion table of qr_reproject_moving_async (Scene.reproject(motion=), Temporal.step(motion=)) between two node tables
    of one hierarchy: float32 [n_srf, 12], n_srf the record count of the CURRENT snapshot (after hierarchy_apply, which may
    have appended transform-node records).  Row s is three rows (a0 a1 a2 t) of the affine map that takes a world point on
    surface record s now to where that material point was in the previous frame: prev = A . pos + t.

    In float64 from hierarchy_update of both tables: W(node) = mtx[node] where trnode is -1 or the node itself, else mtx[node]
    @ mtx[trnode] (4 x 4 row-major, the position in row 3, applied to row vectors); X = inv(W_cur) @ W_prev, A = X[:3, :3].T,
    t = X[3, :3], rounded once to float32.  A node whose two world matrices are bit-equal gets the exact identity row.  Rows of
    quiet NaN ("no history": conservative, never wrong) go to records that no surface node (tag 0..8, srf >= 0) names -- arrays,
    bounding volumes, appended transform-node records --, to surfaces whose A is not a rotation (max |A A^T - I| > 1e-4: a
    scaler changed) and to surfaces whose W_cur is singular.  Both tables must have the same length, parents and tags."""
    import numpy as np
    prev = np.ascontiguousarray(nodes_prev, dtype=node_dtype())
    cur = np.ascontiguousarray(nodes_cur, dtype=node_dtype())
    if prev.shape != cur.shape or prev.ndim != 1:
        raise ValueError("nodes_prev and nodes_cur must be node tables of the same length")
    if not (np.array_equal(prev["parent"], cur["parent"]) and np.array_equal(prev["tag"], cur["tag"])):
        raise ValueError("nodes_prev and nodes_cur must have the same parents and tags: one hierarchy at two times")
    if isinstance(n_srf, bool) or not isinstance(n_srf, (int, np.integer)) or not 0 <= n_srf <= 1 << 30:
        raise ValueError("n_srf must be the record count of the current snapshot, 0..2^30")

    def world(nodes):
        st = hierarchy_update(nodes, opts)
        out = []
        for i in range(len(nodes)):
            m, t = st[i]["mtx"].reshape(4, 4).astype(np.float64), int(st[i]["trnode"])
            out.append(m if t < 0 or t == i else m @ st[t]["mtx"].reshape(4, 4).astype(np.float64))
        return out

    table = np.full((int(n_srf), 12), np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0], dtype=np.float32)
    wp, wc = world(prev), world(cur)
    for i in range(len(cur)):
        s = int(cur[i]["srf"])
        if not (0 <= cur[i]["tag"] < 9 and 0 <= s < n_srf):
            continue
        if wp[i].tobytes() == wc[i].tobytes():
            table[s] = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
            continue
        with np.errstate(all="ignore"):
            try:
                x = np.linalg.inv(wc[i]) @ wp[i]
            except np.linalg.LinAlgError:
                continue
            rot = x[:3, :3].T
            if not (np.isfinite(x).all() and np.abs(rot @ rot.T - np.eye(3)).max() <= 1e-4):
                continue
            table[s] = np.concatenate([rot, x[3, :3, None]], axis=1).reshape(12).astype(np.float32)
    return table


def program_stats(blob, flags=0):
    """Validate + compile a snapshot on the host (no GPU): the device image's size and cell counts.
    flags: upload flags the image is built with (UPLOAD_RAY_QUERIES; the GPU binning of UPLOAD_REBIN_TILES is refused)."""
    info = ProgramInfo()
    buf = ctypes.create_string_buffer(blob, len(blob))
    if flags:
        _check(lib().qr_program_stats_ex(buf, len(blob), flags, ctypes.byref(info)))
    else:
        _check(lib().qr_program_stats(buf, len(blob), ctypes.byref(info)))
    return info


class Scene:
    """A snapshot resident on one GPU (qr_device_scene)."""

    def __init__(self, blob, device=0, rebin_tiles=False, ray_queries=False):
        """rebin_tiles: rebuild the per-tile lists on the GPU from the camera list
        (QR_UPLOAD_REBIN_TILES, include/qrhip.h) instead of using the snapshot's.
        ray_queries: also compile the global list for trace() / occluded() (QR_UPLOAD_RAY_QUERIES)."""
        self._h = ctypes.c_void_p()
        self._buf = ctypes.create_string_buffer(blob, len(blob))
        flags = (UPLOAD_REBIN_TILES if rebin_tiles else 0) | (UPLOAD_RAY_QUERIES if ray_queries else 0)
        _check(lib().qr_scene_upload_ex(self._buf, len(blob), device, flags, ctypes.byref(self._h)))
        self.device = device
        self.info = SceneInfo()
        _check(lib().qr_scene_get_info(self._h, ctypes.byref(self.info)))

    @property
    def width(self):
        return self.info.frm_w

    @property
    def height(self):
        return self.info.frm_h

    def close(self):
        if self._h:
            lib().qr_scene_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_depth(self, depth):
        _check(lib().qr_scene_set_depth(self._h, depth))
        self.info.depth = depth

    def set_pt(self, on=True, eager=False):
        """Path-tracer mode: every render() then adds one sample per pixel sample; the frame is the running mean.
        eager: shade in the reference's order (every hit that passes the depth test, at once): its random streams."""
        _check(lib().qr_scene_set_pt(self._h, (2 if eager else 1) if on else 0))

    def set_rows(self, row_begin, row_end, index=0, thnum=1):
        _check(lib().qr_scene_set_rows(self._h, row_begin, row_end, index, thnum))

    def set_tile_rows(self, first, stride):
        _check(lib().qr_scene_set_tile_rows(self._h, first, stride))

    def new_frame(self):
        import torch
        return torch.zeros((self.height, self.width), dtype=torch.int32, device=f"cuda:{self.device}")

    @staticmethod
    def _stream_ptr(stream):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        return ctypes.c_void_p(s.cuda_stream)

    def render(self, frame=None, stream=None, ids=None):
        """Asynchronous launch on `stream` (default: torch's current stream)."""
        if frame is None:
            frame = self.new_frame()
        sp = self._stream_ptr(stream)
        if ids is None:
            _check(lib().qr_render_async(self._h, frame.data_ptr(), sp))
        else:
            _check(lib().qr_render_ids_async(self._h, frame.data_ptr(), ids.data_ptr(), sp))
        return frame

    # The three sources of the ray API: caller rays, caller views, caller hit records.  Each gives (kind, the head of the C
    # argument list after the scene, the shape of the elements).

    def _rays_arg(self, rays):
        return _need("rays", rays, "float32", (None, 8), self.device, suffix=" (org xyz, tmin, dir xyz, tmax per row)")

    def _rays_src(self, rays):
        n = self._rays_arg(rays).shape[0]
        return "rays", (rays.data_ptr(), n), (n,)

    def _views_src(self, views, width, height):
        _need("views", views, "float32", (None, 16), self.device,
              suffix=" (org xyz, t_min, dir xyz, t_max, hor xyz, 0, ver xyz, 0 per row)")
        w = self.width if width is None else width
        h = self.height if height is None else height
        if not ((type(w) is int or isinstance(w, numbers.Integral)) and (type(h) is int or isinstance(h, numbers.Integral))
                and w >= 1 and h >= 1):                                     # a plain int first: the ABC test is the slow one
            raise QrError("width and height must be positive integers")
        n, w, h = views.shape[0], int(w), int(h)
        return "views", (views.data_ptr(), n, w, h), (n, h, w)

    def _hits_src(self, hits):
        _need("hits", hits, "float32", (..., 12), self.device, suffix=" (qr_hit records)")
        return "hits", (hits.data_ptr(), hits.numel() // 12), tuple(hits.shape[:-1])

    def _rays_call(self, fn, rays, coherent, stream, *outs):
        """one of the plain ray queries: `outs` are (dtype, the shape after [N]) or None for an output that is not wanted"""
        _, head, shape = self._rays_src(rays)
        outs = [o and _new(o[0], shape + o[1], self.device) for o in outs]
        _check(fn(self._h, *head, *map(_ptr, outs), TRACE_COHERENT if coherent else 0, self._stream_ptr(stream)))
        return outs

    def _hit_records(self, src, flags, stream):
        kind, head, shape = src
        out = _new("float32", shape + (12,), self.device)
        _check(getattr(lib(), f"qr_hit_{kind}_async")(self._h, *head, out.data_ptr(), flags, self._stream_ptr(stream)))
        return out

    def trace(self, rays, stream=None, coherent=False):
        """Closest hit of every ray (qr_trace_rays_async): rays float32 [N, 8] = (org xyz, tmin, dir xyz, tmax) on the scene's
        device.  Returns new tensors (t float32 [N]: t of the hit, tmax when none; ids int32 [N]: surface << 1 | side, -1 none).
        coherent: consecutive rays are neighbours (packet walks on long lists too).  Asynchronous on `stream`."""
        t, ids = self._rays_call(lib().qr_trace_rays_async, rays, coherent, stream, ("float32", ()), ("int32", ()))
        return t, ids

    def occluded(self, rays, stream=None, coherent=False):
        """Does a surface that casts a shadow (the renderer's rule) lie at tmin < t < tmax on each ray (qr_occluded_async)?
        Returns a new bool tensor [N].  Asynchronous on `stream`."""
        import torch
        occ, = self._rays_call(lib().qr_occluded_async, rays, coherent, stream, ("uint8", ()))
        return occ.view(torch.bool)

    def shade(self, rays, stream=None, coherent=False, ids=False):
        """The renderer's colour for every ray (qr_shade_rays_async): rays as for trace(); the first hit walks the ray-query
        list, everything after it -- shadows, reflection and refraction to the scene's current depth (set_depth) -- is the
        renderer's.  Returns a new float32 [N, 3] tensor of linear colour, before the frame's output step (rays.pack_colors);
        with ids=True also the first hit's id (int32 [N], surface << 1 | side, -1 none).  Asynchronous on `stream`."""
        rgb, hid = self._rays_call(lib().qr_shade_rays_async, rays, coherent, stream, ("float32", (3,)),
                                   ("int32", ()) if ids else None)
        return (rgb, hid) if ids else rgb

    def hits(self, rays, stream=None, coherent=False):
        """Hit records (qr_hit_rays_async): the closest hit of every ray -- the one trace() finds -- and the surface point the
        renderer would shade there.  rays as for trace().  Returns a new float32 [N, 12] tensor, one qr_hit per row: pos xyz, t,
        nrm xyz, id, alb xyz, mat -- id (surface << 1 | side) and mat (snapshot material index) are int32 bits in float32 slots,
        rays.hit_fields splits a record into typed views.  nrm: the world-space unit normal shading uses, facing the incoming
        ray; alb: the texture colour shading multiplies light by.  A miss has t = tmax, id = mat = -1 and zeros elsewhere.
        Nothing is lit: depth and path-tracer mode do not matter.  Asynchronous on `stream`."""
        return self._hit_records(self._rays_src(rays), TRACE_COHERENT if coherent else 0, stream)

    def view_hits(self, views, width=None, height=None, stream=None):
        """Hit records of whole frames (qr_hit_views_async): a G-buffer -- position, normal, albedo, ids, materials, depth --
        of the resident scene from caller-supplied cameras.  views, width, height as for render_views; the rays are the ones
        it traces (rays.view_rays(view, width, height, blob, sample=0): with FSAA the record is sample 0's, as its ids and
        depth are).  Returns a new float32 [N, H, W, 12] tensor of qr_hit records (see hits(), rays.hit_fields); every pixel
        of every view is written.  Asynchronous on `stream`."""
        return self._hit_records(self._views_src(views, width, height), 0, stream)

    def _atrous_args(self, colour, hits, variance, out, variance_out):
        """the tensors of atrous() / denoise(): dtype and shape first, then contiguity and device.  Returns (n, h, w, channels)."""
        dims = _frame_inputs(colour, hits, variance)
        _plane("out", out, dims, QrError)
        if variance_out is not None and variance is None:
            raise QrError("variance_out needs a variance")
        _plane("variance_out", variance_out, dims[:3], QrError)
        _resident(self.device, QrError, (colour, "colour"), (hits, "hits"), (variance, "variance"), (out, "out"),
                  (variance_out, "variance_out"))
        return dims

    def _atrous_launch(self, colour, variance, hits, dims, step, stops, out, variance_out, stream):
        n, h, w, ch = dims
        flags, nsq, sz, sl2, el, af = stops
        p = AtrousParams(step, ch, nsq, flags, float(sz), float(sl2), float(el), float(af))
        _check(lib().qr_atrous_views_async(self._h, _ptr(colour), _ptr(variance), _ptr(hits), n, w, h, ctypes.byref(p),
                                           _ptr(out), _ptr(variance_out), self._stream_ptr(stream)))

    def atrous(self, colour, hits, variance=None, step=1, normal_power=128, plane=None, luma=None, luma_eps=1e-6, demodulate=False,
               modulate=False, albedo_floor=1 / 256, out=None, variance_out=None, stream=None):
        """One pass of the guided a-trous filter (qr_atrous_views_async; rays.atrous_pass is its arithmetic): an edge-avoiding
        5x5 average of colour (float32 [N, H, W, 3|4]: PtAdaptiveViews.step(mean=True), render_views_mean's sum, view_gather)
        with taps `step` pixels apart (1..ATROUS_MAX_STEP), guided by hits (view_hits of the same views) and, with a variance
        (float32 [N, H, W]: PtAdaptiveViews.variance), by the luminance against it.  normal_power: None or a power of two 1..128,
        the exponent of max(0, n . n'); plane: sigma_z in world units, or None; luma: the tolerance in standard deviations, or
        None (without a variance: in units of 1); demodulate / modulate: divide every colour read by its pixel's albedo / multiply
        the output by it, albedo_floor the smallest albedo divided by.  The defaults are SVGF's customary starting points, not
        tuned.  out / variance_out: tensors to write, neither the inputs.  Returns colour_out, or (colour_out, variance_out) with
        a variance.  Asynchronous on `stream`."""
        import torch
        stops = _stops("atrous_stops", QrError, normal_power=normal_power, plane=plane, luma=luma, luma_eps=luma_eps,
                       demodulate=demodulate, modulate=modulate, albedo_floor=albedo_floor)
        if isinstance(step, bool) or not isinstance(step, numbers.Integral) or not 1 <= step <= ATROUS_MAX_STEP:
            raise QrError(f"step must be an integer, 1..{ATROUS_MAX_STEP}")
        dims = self._atrous_args(colour, hits, variance, out, variance_out)
        if out is None:
            out = torch.empty_like(colour)              # not _new: torch.empty with its keywords cost 0.7 us more per tensor
        if variance is not None and variance_out is None:
            variance_out = torch.empty_like(variance)
        self._atrous_launch(colour, variance, hits, dims, int(step), stops, out, variance_out, stream)
        return out if variance is None else (out, variance_out)

    def denoise(self, colour, hits, variance=None, passes=5, albedo=False, **stops):
        """The whole filter (rays.denoise): `passes` (1..7) atrous passes with step = 1, 2, 4, ... on `stream` (stream=, default
        torch's current stream), each fed the one before.  It ping-pongs between two scratch tensors of its own and never
        writes colour or variance.  albedo=True divides by the albedo on the first pass and multiplies on the last.  stops:
        normal_power, plane, luma, luma_eps, albedo_floor as atrous() takes them.  Returns (colour, variance or None), new
        tensors."""
        import torch
        stream = stops.pop("stream", None)
        if isinstance(passes, bool) or not isinstance(passes, numbers.Integral) or not 1 <= passes <= 7:
            raise QrError("passes must be an integer, 1..7")
        if "demodulate" in stops or "modulate" in stops:
            raise QrError("denoise sets demodulate and modulate itself (albedo=True)")
        per_pass = [_stops("atrous_stops", QrError, demodulate=bool(albedo) and k == 0, modulate=bool(albedo) and k == passes - 1, **stops)
                    for k in range(passes)]
        dims = self._atrous_args(colour, hits, variance, None, None)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            cbuf = [torch.empty_like(colour) for _ in range(min(passes, 2))]
            vbuf = [torch.empty_like(variance) for _ in range(min(passes, 2))] if variance is not None else [None, None]
        c, v = colour, variance
        for k in range(passes):
            co, vo = cbuf[k & 1], vbuf[k & 1]
            self._atrous_launch(c, v, hits, dims, 1 << k, per_pass[k], co, vo, stream)
            c, v = co, vo
        return c, v

    def _upsample_args(self, colour_lo, hits, factor, phase, variance, out, variance_out, weight):
        """the tensors of upsample(), as _atrous_args takes its own but with ValueError.  Returns ((n, h, w, channels), the
        weight to fill: a tensor, a new one, or None)."""
        n, h, w, _ = dims = _frame_inputs(colour_lo, hits, variance, ValueError, (factor, phase))
        if variance_out is not None and variance is None:
            raise ValueError("variance_out needs a variance")
        _plane("out", out, dims, ValueError)
        _plane("variance_out", variance_out, (n, h, w), ValueError)
        if weight is None or isinstance(weight, bool):
            weight = True if weight else None
        elif not _fits(weight, "float32", (n, h, w)):
            raise ValueError(f"weight must be True, False or a float32 [{n}, {h}, {w}] tensor")
        _resident(self.device, ValueError, (colour_lo, "colour_lo"), (hits, "hits"), (variance, "variance"), (out, "out"),
                  (variance_out, "variance_out"), (None if weight is True else weight, "weight"))
        return dims, _new("float32", (n, h, w), self.device) if weight is True else weight

    def upsample(self, colour_lo, hits, factor, phase=(0, 0), variance=None, normal_power=128, plane=None, same_id=False,
                 demodulate=False, modulate=False, albedo_floor=1 / 256, out=None, variance_out=None, weight=False, stream=None):
        """Guided upsampling (qr_upsample_views_async; rays.upsample_pass is its arithmetic): coarse light colour_lo (float32
        [N, Hl, Wl, 3|4], computed for every factor-th pixel from `phase` = (px, py) on: hit_gather on rays.coarse_hits(hits,
        factor, phase), or pt_views / pt_adaptive_views / render_views on rays.coarse_view at rays.coarse_size) brought to the
        full frame of hits (view_hits, float32 [N, H, W, 12]) through the four lattice points around each pixel, weighted
        bilinearly and by the guide: normal_power (None or a power of two 1..128), plane (sigma_z in world units, or None),
        same_id (only taps of the pixel's own surface).  variance: float32 [N, Hl, Wl] or None.  demodulate divides the coarse
        colour by its lattice pixel's albedo, modulate multiplies the result by the full pixel's; albedo_floor the smallest
        albedo divided by.  The stops are starting points, not tuned.  out / variance_out: tensors to write; weight: True (a
        new tensor), False or a tensor to fill with the taken taps' weight (0: only taps of bilinear weight 0; -1: no tap, the
        nearest coarse pixel: what a host may trace again).  A wrong tensor is a ValueError.  Returns the colour, or a tuple of
        the colour, the variance (with a variance) and the weight (when wanted).  Asynchronous on `stream`."""
        flags, nsq, sz, af = _stops("upsample_stops", ValueError, normal_power=normal_power, plane=plane, same_id=same_id,
                                    demodulate=demodulate, modulate=modulate, albedo_floor=albedo_floor)
        (n, h, w, ch), weight = self._upsample_args(colour_lo, hits, factor, phase, variance, out, variance_out, weight)
        if out is None:
            out = _new("float32", (n, h, w, ch), self.device)
        if variance is not None and variance_out is None:
            variance_out = _new("float32", (n, h, w), self.device)
        p = UpsampleParams(int(factor), int(phase[0]), int(phase[1]), ch, nsq, flags, float(sz), float(af))
        _check(lib().qr_upsample_views_async(self._h, _ptr(colour_lo), _ptr(variance), _ptr(hits), n, w, h, ctypes.byref(p),
                                             _ptr(out), _ptr(variance_out), _ptr(weight), self._stream_ptr(stream)))
        got = (out,) + (() if variance is None else (variance_out,)) + (() if weight is None else (weight,))
        return got[0] if len(got) == 1 else got

    def _reproject_args(self, colour, hits, prev, variance, out, colour_out, variance_out, coords):
        """the tensors of reproject(): dtype and shape first, then contiguity and device.  Returns ((n, h, w, channels), the
        previous triple or three None, (out, colour_out, variance_out, coords)) with the outputs that are wanted made."""
        dev = self.device
        n, h, w, ch = _frame_inputs(colour, hits, variance)
        if prev is None:
            prev = (None, None, None)
        elif not (isinstance(prev, (tuple, list)) and len(prev) == 3 and _fits(prev[0], "float32", (n, 16))
                  and _fits(prev[1], "float32", (n, h, w, 12)) and _fits(prev[2], "float32", (n, h, w, 8))):
            raise QrError(f"prev must be None or (views_prev float32 [{n}, 16], hits_prev float32 [{n}, {h}, {w}, 12], "
                          f"history float32 [{n}, {h}, {w}, 8])")
        _resident(dev, QrError, (colour, "colour"), (hits, "hits"), (variance, "variance"), (prev[0], "views_prev"), (prev[1], "hits_prev"),
                  (prev[2], "history"))
        out = _fill("out", out, "float32", (n, h, w, 8), dev)
        if prev[2] is not None and out.data_ptr() == prev[2].data_ptr():
            raise QrError("out must not be the previous history: the taps read neighbours")
        return (n, h, w, ch), prev, (out, _wanted("colour_out", colour_out, "float32", (n, h, w, ch), dev),
                                     _wanted("variance_out", variance_out, "float32", (n, h, w), dev),
                                     _wanted("coords", coords, "float32", (n, h, w, 2), dev))

    def _motion_arg(self, motion):
        """the motion table of reproject() / Temporal.step(): None, or a contiguous float32 [n, 12] tensor (n >= 1) on the
        scene's device (hierarchy_motion makes it); ValueError for anything else"""
        if motion is None:
            return None
        motion = _need("motion", motion, "float32", (None, 12), self.device, error=ValueError)
        if not 1 <= motion.shape[0] <= 1 << 30:
            raise ValueError("motion must have 1..2^30 rows")
        return motion

    @staticmethod
    def _clamp_arg(clamp, moved=None):
        """the clamp block of reproject() / Temporal before any tensor is looked at: None, or a rays.clamp_stops dict, returned
        as (flags, radius, gamma, short_len); ValueError for what the call would refuse and for a moved plane without a block"""
        from . import rays
        if clamp is not None:
            return rays._clamp_params(clamp)
        if not (moved is False or moved is None):
            raise ValueError("moved needs a clamp")
        return None

    def _moved_arg(self, moved, dims):
        """the moved plane of reproject(): False or None (None), True (a new tensor) or a float32 [N, H, W] tensor to fill"""
        try:
            return _wanted("moved", moved, "float32", dims[:3], self.device)
        except QrError as e:
            raise ValueError(str(e)) from None

    def _reproject_launch(self, colour, hits, variance, prev, dims, stops, outs, stream, motion=None, clamp=None, moved=None):
        n, h, w, ch = dims
        p = ReprojectParams(ch, *(stops[k] for k in ("flags", "off_x", "off_y", "normal_min", "plane_max", "min_weight", "alpha_min",
                                                     "alpha_mom_min", "max_len", "var_min_len", "unknown", "alb_floor")))
        if clamp is not None:
            c = ClampParams(int(clamp[0]), int(clamp[1]), float(clamp[2]), float(clamp[3]))
            table = (None, 0) if motion is None else (motion.data_ptr(), int(motion.shape[0]))
            _check(lib().qr_reproject_clamped_async(self._h, _ptr(colour), _ptr(hits), _ptr(variance), _ptr(prev[0]), _ptr(prev[1]),
                                                    _ptr(prev[2]), *table, n, w, h, ctypes.byref(p), ctypes.byref(c),
                                                    *map(_ptr, outs), _ptr(moved), self._stream_ptr(stream)))
            return
        fn, table = (lib().qr_reproject_views_async, ()) if motion is None else \
            (lib().qr_reproject_moving_async, (motion.data_ptr(), int(motion.shape[0])))
        _check(fn(self._h, _ptr(colour), _ptr(hits), _ptr(variance), _ptr(prev[0]), _ptr(prev[1]), _ptr(prev[2]), *table, n, w, h,
                  ctypes.byref(p), *map(_ptr, outs), self._stream_ptr(stream)))

    def reproject(self, colour, hits, prev=None, variance=None, out=None, colour_out=True, variance_out=True, coords=False,
                  stream=None, motion=None, clamp=None, moved=False, **params):
        """Temporal reprojection (qr_reproject_views_async; rays.reproject_pass is its arithmetic): blend this frame's noisy colour
        (float32 [N, H, W, 3|4]) into the history of the frame before, fetched where this frame's hits (view_hits of the current
        cameras) fall in the previous cameras and kept only on the same surface.  prev = (views_prev [N, 16], hits_prev, history
        [N, H, W, 8]) of the frame before, None for a first frame; variance (float32 [N, H, W], PtAdaptiveViews.variance): what
        a short history hands out.  out: the history tensor to write (a new one by default, never prev's); colour_out,
        variance_out, coords: True (a new tensor), False or a tensor to fill.  params: normal_min, plane_max, min_weight,
        alpha_min, alpha_mom_min, max_len, var_min_len, unknown, albedo_floor, demodulate, off as rays.reproject_stops takes
        them -- starting points, not tuned.  motion=None: static scenes under a moving camera.  motion (float32 [n, 12] on
        the scene's device, hierarchy_motion of the previous and the current node table; ValueError for anything else): an
        animated scene patched by hierarchy_apply -- every pixel's point and normal are taken to where its surface was in the
        previous frame before the projection and the tap tests (qr_reproject_moving_async).  clamp: None, or a
        rays.clamp_stops block (qr_reproject_clamped_async; a bad one is a ValueError): the fetched history colour is held to
        the box of this frame's colours around the pixel before it is blended, so that light which changed on a surface that
        did not move -- a shadow that went on -- does not trail.  moved (it needs a clamp): True for a new float32 [N, H, W]
        tensor, or a tensor to fill, with how far each pixel's history was moved (-1: a fresh entry).  Returns (history,
        colour, variance), with coords wanted (history, colour, variance, coords); what is not wanted is None; with moved, the
        result is extended by that one tensor.  Asynchronous on `stream`."""
        motion = self._motion_arg(motion)
        stops = _stops("reproject_stops", QrError, **params)
        clamp = self._clamp_arg(clamp, moved)
        dims, prev, outs = self._reproject_args(colour, hits, prev, variance, out, colour_out, variance_out, coords)
        moved = self._moved_arg(moved, dims)
        self._reproject_launch(colour, hits, variance, prev, dims, stops, outs, stream, motion, clamp, moved)
        got = outs[:3] if outs[3] is None else outs
        return got if moved is None else got + (moved,)

    def temporal(self, n_views, width, height, channels=3, clamp=None, **params):
        """A temporal accumulator over frames of n_views moving cameras at width x height (rays.temporal is its chain): returns
        a Temporal whose step(colour, hits, views, variance=None, motion=None, scene=None) reprojects against the frame
        before.  params as for reproject(); clamp: None or a rays.clamp_stops block applied on every step (ValueError for a
        bad one)."""
        return Temporal(self, n_views, width, height, channels, clamp=clamp, **params)

    def _fan_args(self, dirs, eps, reach, shape, mask):
        """(dirs as a contiguous float32 [K, 4] tensor, K, eps, reach, open, mask or None) of an occlusion-fan call whose
        elements have `shape`"""
        d4, k, eps, reach = _dirs_arg(dirs, eps, reach, 0.0, self.device)
        opn = _new("int32", shape, self.device)                                         # every element is written
        msk = _new("int32", ((k + 31) // 32,) + tuple(shape), self.device) if mask else None
        return d4, k, eps, reach, opn, msk

    def _spin_arg(self, frame, spin, shape):
        """the spin plane of a framed fan call whose elements have `shape`, as a pointer (None: no spin); ValueError when it
        cannot be one"""
        if spin is None:
            return None
        if not frame:
            raise ValueError("spin needs frame=True: it turns the table about the normal of a framed fan")
        return _need("spin", spin, "float32", tuple(shape) + (2,), self.device, error=ValueError).data_ptr()

    def _occlusion(self, src, dirs, eps, reach, flags, mask, stream, frame, spin):
        """the occlusion fans of any source: its spin, dirs, K and eps checks in that order, then the launch (the spin plane
        after k when framed)"""
        kind, head, shape = src
        sp = None if spin is None else self._spin_arg(frame, spin, shape)
        d4, k, eps, reach, opn, msk = self._fan_args(dirs, eps, reach, shape, mask)
        fn = _FAN_FNS.get(("fan", kind, not frame)) or _fan_fn("fan", kind, not frame)
        _check(fn(self._h, *head, d4.data_ptr(), k, *((sp,) if frame else ()), eps, reach, opn.data_ptr(), _ptr(msk), flags,
                  self._stream_ptr(stream)))
        return (opn, msk) if mask else opn

    def _gather(self, src, dirs, eps, reach, flags, out, count, resume, stream, frame, spin):
        """the gather fans of any source: its spin, resume, out, count, dirs, K and eps checks in that order, then the launch
        (the spin plane after k when framed)"""
        kind, head, shape = src
        sp = None if spin is None else self._spin_arg(frame, spin, shape)
        d4, k, eps, reach, out, count = self._gather_args(dirs, eps, reach, shape, out, count, resume)
        fn = _FAN_FNS.get(("gather", kind, not frame)) or _fan_fn("gather", kind, not frame)
        _check(fn(self._h, *head, d4.data_ptr(), k, *((sp,) if frame else ()), eps, reach, out.data_ptr(), count.data_ptr(),
                  flags, self._stream_ptr(stream)))
        return out, count

    def occlusion(self, rays, dirs, eps, reach=float("inf"), flip=False, mask=False, coherent=False, stream=None, frame=False,
                  spin=None):
        """Occlusion fans from the first hits of caller rays (qr_fan_rays_async): for every ray, the surface point hits() gives
        (pos, nrm, id) and from it one visibility ray per row of `dirs` (float32 [K, 3] or [K, 4] on the scene's device, K <=
        1024, shared by all rays; [K, 3] is padded), in ONE launch: no hit record and no fan ray reaches memory.  Direction k is
        traced iff 0 < nrm . dirs[k] (flip=True: always, as -dirs[k] where the dot product is negative) and is open iff
        occluded() answers False for the ray (pos, eps, +-dirs[k], reach); rays.fan_rays states the composition exactly.
        Returns open (int32 [N]: the number of open directions, -1 where the ray hits nothing); with mask=True (open, mask):
        mask int32 [ceil(K / 32), N], bit k & 31 of plane k >> 5 set iff direction k is open (rays.fan_bits unpacks it).
        eps: the step off the surface in units of |dir| (there is no self-exclusion).  coherent: as for trace(); results do not
        depend on it.  Nothing is lit: depth and path-tracer mode do not matter.  Asynchronous on `stream`.
        frame=True (qr_fan_rays_framed_async): `dirs` is in every surface point's own frame, local +z its normal
        (rays.fan_frame), so a hemisphere table such as rays.cosine_dirs wastes no direction; direction k is traced iff
        0 < dirs[k, 2] (flip=True: always, mirrored where dirs[k, 2] < 0) and the point's frame is valid.  spin (needs frame):
        float32 [N, 2] = (cos, sin) of a turn of the table about the normal per element (rays.spins), on the scene's device,
        contiguous.  rays.fan_rays(frame=True) states the composition exactly."""
        flags = (TRACE_COHERENT if coherent else 0) | (FAN_FLIP if flip else 0)
        return self._occlusion(self._rays_src(rays), dirs, eps, reach, flags, mask, stream, frame, spin)

    def view_occlusion(self, views, dirs, width=None, height=None, eps=None, reach=float("inf"), flip=False, mask=False, stream=None,
                       frame=False, spin=None):
        """Occlusion fans from every pixel of caller-supplied cameras (qr_fan_views_async): ambient occlusion or sky visibility
        of whole frames in one launch.  views, width, height as for view_hits -- the surface point of a pixel is its record there
        (sample 0's under FSAA) -- dirs, eps (required), reach, flip, mask as for occlusion().  Returns open int32 [N, H, W]
        (-1 where the pixel shows nothing), with mask=True (open, mask int32 [ceil(K / 32), N, H, W]).  Asynchronous on `stream`.
        frame, spin (float32 [N, H, W, 2]) as for occlusion() (qr_fan_views_framed_async)."""
        return self._occlusion(self._views_src(views, width, height), dirs, eps, reach, FAN_FLIP if flip else 0, mask, stream,
                               frame, spin)

    def hit_occlusion(self, hits, dirs, eps, reach=float("inf"), flip=False, mask=False, stream=None, frame=False, spin=None):
        """Occlusion fans from caller-supplied hit records (qr_fan_hits_async): hits float32 [..., 12] on the scene's device,
        contiguous (hits(), view_hits(), or a host's own points: pos in columns 0:3, nrm in 4:7, the int32 bits of an id >= 0 in
        column 7; the rest is not read) -- second-bounce AO, lightmap texels, probes.  No first walk.  dirs, eps, reach, flip,
        mask as for occlusion().  Returns open int32 [...] (-1 where id < 0), with mask=True (open, mask int32
        [ceil(K / 32), ...]).  Asynchronous on `stream`.  frame, spin (float32 [..., 2]) as for occlusion()
        (qr_fan_hits_framed_async)."""
        return self._occlusion(self._hits_src(hits), dirs, eps, reach, FAN_FLIP if flip else 0, mask, stream, frame, spin)

    def _gather_args(self, dirs, eps, reach, shape, out, count, resume):
        """(dirs as a contiguous float32 [K, 4] tensor, K, eps, reach, gather, count) of a gather-fan call whose elements have
        `shape`; [K, 3] tables get weight 1.0"""
        if resume and (out is None or count is None):
            raise QrError("resume=True needs both buffers: out (the sums so far) and count")
        shape = tuple(shape)
        # _fill in two halves: the buffers are checked before dirs and made after, so that a refused table allocates nothing
        if out is not None:
            _need("out", out, "float32", shape + (4,), self.device)
        if count is not None:
            _need("count", count, "int32", shape, self.device)
        d4, k, eps, reach = _dirs_arg(dirs, eps, reach, 1.0, self.device)
        if out is None:
            out = _new("float32", shape + (4,), self.device)
        if count is None:
            count = _new("int32", shape, self.device)
        return d4, k, eps, reach, out, count

    @staticmethod
    def _gather_flags(flip, cosine, resume, coherent=False):
        return ((TRACE_COHERENT if coherent else 0) | (FAN_FLIP if flip else 0) | (GATHER_COSINE if cosine else 0)
                | (GATHER_RESUME if resume else 0))

    def gather(self, rays, dirs, eps, reach=float("inf"), flip=False, cosine=False, coherent=False, out=None, count=None,
               resume=False, stream=None, frame=False, spin=None):
        """Gather fans from the first hits of caller rays (qr_gather_rays_async): for every ray, the surface point hits() gives
        and from it one SHADED ray per row of `dirs` (float32 [K, 4] on the scene's device: direction xyz, weight; [K, 3]: weight
        1.0; K <= 1024, shared by all rays), folded into one weighted sum per ray in ONE launch: no hit record, fan ray or
        per-direction colour reaches memory.  Direction k is traced as for occlusion() (rays.fan_rays: iff 0 < nrm . dirs[k];
        flip=True: always, as -dirs[k] where the dot product is negative); its colour is what shade() returns for the ray
        (pos, eps, +-dirs[k], reach), at the scene's current depth; its weight is dirs[k, 3], times the dot product (its
        absolute value with flip) with cosine=True.  rays.gather_fold states the sum exactly.
        Returns (gather float32 [N, 4]: sum of colour * weight in r, g, b and the sum of weights in w; count int32 [N]: traced
        directions, -1 and a zero row where the ray hits nothing).  out, count: buffers to write into; resume=True (needs
        both): the sums and counts start from their contents, so that a table sent in consecutive chunks gives the bits of
        one call.  coherent: as for trace(); results do not depend on it.  Asynchronous on `stream`.
        frame=True (qr_gather_rays_framed_async): `dirs` is in every surface point's own frame, local +z its normal, as for
        occlusion(); the dot product is dirs[k, 2], the table's own cosine.  With rays.cosine_dirs the plain sum
        (cosine=False) is the irradiance estimate.  spin (needs frame): float32 [N, 2], as for occlusion().
        rays.gather_fold(frame=True) states the sum exactly."""
        return self._gather(self._rays_src(rays), dirs, eps, reach, self._gather_flags(flip, cosine, resume, coherent), out, count,
                            resume, stream, frame, spin)

    def view_gather(self, views, dirs, width=None, height=None, eps=None, reach=float("inf"), flip=False, cosine=False,
                    out=None, count=None, resume=False, stream=None, frame=False, spin=None):
        """Gather fans from every pixel of caller-supplied cameras (qr_gather_views_async): one-bounce irradiance or sky light
        of whole frames in one launch.  views, width, height as for view_hits -- the surface point of a pixel is its record
        there (sample 0's under FSAA) -- the rest as for gather(); eps is required.  Returns (gather float32 [N, H, W, 4],
        count int32 [N, H, W]).  Asynchronous on `stream`.  frame, spin (float32 [N, H, W, 2]) as for gather()
        (qr_gather_views_framed_async)."""
        return self._gather(self._views_src(views, width, height), dirs, eps, reach, self._gather_flags(flip, cosine, resume), out,
                            count, resume, stream, frame, spin)

    def hit_gather(self, hits, dirs, eps, reach=float("inf"), flip=False, cosine=False, out=None, count=None, resume=False,
                   stream=None, frame=False, spin=None):
        """Gather fans from caller-supplied hit records (qr_gather_hits_async): hits as for hit_occlusion() (float32 [..., 12]:
        pos in columns 0:3, nrm in 4:7, the int32 bits of an id >= 0 in column 7) -- lightmap texels, probes, a second bounce.
        No first walk.  The rest as for gather().  Returns (gather float32 [..., 4], count int32 [...]).  Asynchronous on
        `stream`.  frame, spin (float32 [..., 2]) as for gather() (qr_gather_hits_framed_async)."""
        return self._gather(self._hits_src(hits), dirs, eps, reach, self._gather_flags(flip, cosine, resume), out, count, resume,
                            stream, frame, spin)

    def _layers(self, src, k, t, ids, hits, flags, stream):
        """the hit layers of either source: (count, t or None, ids or None) and, with hits, the records"""
        kind, head, shape = src
        if not (isinstance(k, numbers.Integral) and 1 <= k <= LAYER_MAX):
            raise QrError(f"k must be an integer 1..{LAYER_MAX} (layers), got {k!r}")
        k = int(k)
        cnt = _new("int32", shape, self.device)                                         # every element of every plane is written
        tt = _new("float32", (k,) + shape, self.device) if t else None
        ii = _new("int32", (k,) + shape, self.device) if ids else None
        hh = _new("float32", (k,) + shape + (12,), self.device) if hits else None
        _check(getattr(lib(), f"qr_layer_{kind}_async")(self._h, *head, k, cnt.data_ptr(), _ptr(tt), _ptr(ii), _ptr(hh), flags,
                                                        self._stream_ptr(stream)))
        return (cnt, tt, ii, hh) if hits else (cnt, tt, ii)

    def trace_layers(self, rays, k, t=True, ids=True, hits=False, coherent=False, stream=None):
        """The first k hits along every ray, in order, in ONE launch (qr_layer_rays_async): picking through glass, thickness and
        entry / exit pairs, order-independent transparency, "how many surfaces lie between A and B".  rays as for trace(); k:
        1..LAYER_MAX.  Layer 0 is exactly trace()'s answer for the ray; layer j + 1 is its answer for the same ray with tmin = t
        of layer j, bit for bit, no epsilon (rays.layers_of states the composition).  A ray ends at its first miss.
        Returns (count, t, ids) or, with hits=True, (count, t, ids, hits): count int32 [N]: hits found, 0..k (k: there may be
        more); t float32 [k, N] and ids int32 [k, N]: plane j is layer j, with the miss values t = tmax (FLT_MAX for +inf),
        id = -1 from layer `count` on; hits float32 [k, N, 12]: layer j's qr_hit record (see hits()), the miss record from
        layer `count` on.  t=False / ids=False: that output is not computed and None stands in its place.  t is strictly
        increasing over a ray's hits; surfaces at bit-equal t collapse to the first in list order.  rays.next_rays(rays, t[-1],
        ids[-1]) gives the rays that resume where this call stopped: k1 layers, then k2 on them, equal one call with k1 + k2.
        coherent: as for trace(); results do not depend on it.  Nothing is lit: depth and path-tracer mode do not matter.
        Asynchronous on `stream`."""
        return self._layers(self._rays_src(rays), k, t, ids, hits, TRACE_COHERENT if coherent else 0, stream)

    def view_layers(self, views, k, width=None, height=None, t=True, ids=True, hits=False, stream=None):
        """The first k hits behind every pixel of caller-supplied cameras (qr_layer_views_async): layered depth images, x-ray
        views, thickness maps.  views, width, height as for view_hits -- the rays are the ones it traces, sample 0's under FSAA
        -- k, t, ids, hits as for trace_layers().  Returns (count int32 [N, H, W], t float32 [k, N, H, W], ids int32
        [k, N, H, W]) and, with hits=True, hits float32 [k, N, H, W, 12].  Layer 0 is view_hits' answer.  Asynchronous on
        `stream`."""
        return self._layers(self._views_src(views, width, height), k, t, ids, hits, 0, stream)

    def render_views(self, views, width=None, height=None, frames=None, ids=False, depth=False, stream=None):
        """Whole frames of the resident scene from caller-supplied cameras (qr_render_views_async): views float32 [N, 16] on the
        scene's device, one qr_view per row (org xyz, t_min, dir xyz, t_max, hor xyz, 0, ver xyz, 0: rays.view_of, rays.look_at),
        all rendered at width x height (default: the snapshot's size) in one launch, at the scene's current depth (set_depth)
        and with the snapshot's FSAA, gamma and output step.  Returns `frames` (int32 [N, H, W] like new_frame; a new tensor
        unless given), followed by the first hit's ids (int32 [N, H, W], surface << 1 | side, -1 none) with ids=True and the
        first hit's t (float32 [N, H, W], the view's t_max where none) with depth=True.  Asynchronous on `stream`."""
        _, head, shape = self._views_src(views, width, height)
        frames = _fill("frames", frames, "int32", shape, self.device)
        hid = _new("int32", shape, self.device) if ids else None
        dep = _new("float32", shape, self.device) if depth else None
        _check(lib().qr_render_views_async(self._h, *head, frames.data_ptr(), _ptr(hid), _ptr(dep), 0, self._stream_ptr(stream)))
        out = (frames,) + ((hid,) if ids else ()) + ((dep,) if depth else ())
        return out if len(out) > 1 else frames

    def render_views_mean(self, views, width=None, height=None, sum=None, frame=True, scale=None, resume=False, stream=None):
        """One frame that is the mean of many views (qr_render_views_mean_async): views, width, height as for render_views; every
        view's linear pixel colour (render_views' arithmetic up to and including the FSAA reduce) is added in array order, one
        fp32 add per channel and view, into `sum` (float32 [H, W, 3]; a new tensor unless given), and with frame=True (or an
        int32 [H, W] tensor to fill) the rest of the output step is applied to sum * scale.  scale=None: float32(1) /
        float32(n_views).  resume=True: the sum starts from the contents of `sum` (required then, as is `scale` when a frame is
        wanted: 1 / the number of views added so far, this call's included) -- views cut into several resumed calls give the bits
        of one call.  Returns (frame or None, sum).  One wave renders a footprint of all views: meant for full-size frames.
        Asynchronous on `stream`."""
        import numpy as np
        _, head, (n, h, w) = self._views_src(views, width, height)
        if resume and sum is None:
            raise QrError("resume=True needs the `sum` tensor of the earlier calls")
        sum = _fill("sum", sum, "float32", (h, w, 3), self.device)
        frame = _wanted("frame", frame, "int32", (h, w), self.device)
        if frame is not None:
            if scale is None:
                if resume:
                    raise QrError("resume=True with a frame needs `scale`: 1 / the number of views added so far")
                scale = np.float32(1) / np.float32(max(n, 1))
            scale = float(np.float32(scale))
            if not (np.isfinite(scale) and scale > 0.0):
                raise QrError("scale must be finite and greater than 0")
        _check(lib().qr_render_views_mean_async(self._h, *head, sum.data_ptr(), _ptr(frame), scale if frame is not None else 1.0,
                                                MEAN_RESUME if resume else 0, self._stream_ptr(stream)))
        return frame, sum

    def pt_views(self, views, width=None, height=None, state=None, samples=0):
        """Progressive path-traced frames from caller-supplied cameras (qr_pt_views_async): returns a PtViews accumulator for
        `views` (as for render_views) at width x height.  state=None: a new state tensor, reset (every view starts from the
        seed plane rays.pt_seeds gives, means 0).  state=<tensor>, samples=<count>: continue a checkpoint -- an int32
        [N, 4, H * W * samples_per_pixel] tensor on the scene's device holding `samples` samples."""
        return PtViews(self, views, width, height, state, samples)

    def pt_rays(self, n, state=None, samples=0):
        """Progressive path-traced samples for caller rays (qr_pt_rays_async): returns a PtRays accumulator for `n` rays.
        state=None: a new state tensor, reset (ray i starts from seed i of rays.pt_seeds(n, 1, 1), means 0).  state=<tensor>,
        samples=<count>: continue a checkpoint -- an int32 [4, n] tensor on the scene's device holding `samples` samples."""
        return PtRays(self, n, state, samples)

    def pt_adaptive(self, n, min_samples, max_samples, tol, state=None):
        """Adaptive path-traced samples for caller rays (qr_pt_adapt_rays_async): returns a PtAdaptive accumulator for `n` rays
        that keeps a sample count and a noise estimate per ray and stops a ray once the standard error of its mean is at most
        `tol` in every channel (linear colour units), between `min_samples` and `max_samples` samples per ray since the reset.
        state=None: a new state tensor, reset.  state=<tensor>: continue from an int32 [8, n] tensor on the scene's device."""
        return PtAdaptive(self, n, min_samples, max_samples, tol, state)

    def pt_adaptive_views(self, views, width=None, height=None, min_samples=0, max_samples=64, tol=0.0, state=None):
        """Adaptive path-traced frames from caller-supplied cameras (qr_pt_adapt_views_async): returns a PtAdaptiveViews
        accumulator for `views` (as for render_views) at width x height that keeps a sample count and a noise estimate per pixel
        sample and stops a pixel sample once the standard error of its mean is at most `tol` in every channel, between
        `min_samples` and `max_samples` samples since the reset.  state=None: a new state tensor, reset.  state=<tensor>:
        continue from an int32 [N, 8, H * W * samples_per_pixel] tensor on the scene's device."""
        return PtAdaptiveViews(self, views, width, height, min_samples, max_samples, tol, state)

    def render_count(self, frame=None, stream=None):
        if frame is None:
            frame = self.new_frame()
        c = RayCounts()
        _check(lib().qr_render_count(self._h, frame.data_ptr(), self._stream_ptr(stream), ctypes.byref(c)))
        return frame, c

    def render_timed(self, frame, iters, stream=None):
        avg, mn = ctypes.c_float(), ctypes.c_float()
        _check(lib().qr_render_timed(self._h, frame.data_ptr(), self._stream_ptr(stream), iters, ctypes.byref(avg),
                                     ctypes.byref(mn)))
        return avg.value, mn.value

    def render_host(self, out=None, row_pixels=None):
        """qr_render_host into a new (or the given) host frame; `row_pixels`: its stride in pixels."""
        import numpy as np
        if out is None:
            out = np.zeros((self.height, self.width), dtype=np.uint32)
        _check(lib().qr_render_host(self._h, out.ctypes.data_as(ctypes.c_void_p), self.width if row_pixels is None else row_pixels))
        return out


_UNCOUNTED = object()      # _adopt's `samples` of the adaptive accumulators, whose state holds the counts itself
_LIST = "int32 or uint32"   # what an open list's index and count, and an open counter, may be


class _Accumulator:
    """What the four accumulators share: how a state is adopted, and the caller rays of a step."""

    def _adopt(self, query, head, shape, state, samples=_UNCOUNTED):
        """Ask the library for the state's size (`query` with `head`), hold it against the layout, and take the state: a new
        one, reset, or the caller's, checked.  samples (the two plain accumulators): how many the caller's state holds"""
        nbytes = ctypes.c_uint64()
        _check(query(self.scene._h, *head, ctypes.byref(nbytes)))
        assert nbytes.value == 4 * math.prod(shape)
        if state is None:
            if samples is not _UNCOUNTED and samples != 0:
                raise QrError("a new state holds no samples: pass the state tensor that holds them")
            self.state = _new("int32", shape, self.scene.device)
            self.reset()
        else:
            self.state = _need("state", state, "int32", shape, self.scene.device)
            if samples is not _UNCOUNTED:
                if not (isinstance(samples, int) and samples >= 0):
                    raise QrError("samples must be the non-negative number of samples the state holds")
                self.samples = samples

    def _ray_args(self, rays, spread, rgb):
        """(rays, spread or None, rgb or None) of a step over caller rays"""
        n, dev = self.n, self.scene.device
        rays = self.scene._rays_arg(rays)
        if rays.shape[0] != n:
            raise QrError(f"this accumulation holds {n} rays, got {rays.shape[0]}")
        if spread is not None:
            _need("spread", spread, "float32", (n, 8), dev, lead="None or a", suffix=" (du xyz, pad, dv xyz, pad per row)")
        return rays, spread, _wanted("rgb", rgb, "float32", (n, 3), dev)


class _Adaptive(_Accumulator):
    """What the two adaptive accumulators share: the stop rule, the open list of a state block, the open counter."""

    def _rule(self, min_samples, max_samples, tol):
        import numpy as np
        if not (isinstance(min_samples, int) and isinstance(max_samples, int)
                and 0 <= min_samples <= max_samples and 1 <= max_samples < (1 << 24)):
            raise QrError("min_samples and max_samples must be integers, 0 <= min_samples <= max_samples, 1 <= max_samples < 2^24")
        try:
            t = np.float32(tol)
        except (TypeError, ValueError):
            raise QrError("tol must be a number") from None
        with np.errstate(over="ignore", invalid="ignore"):
            tol2 = t * t
        if not (t >= 0 and np.isfinite(tol2)):
            raise QrError("tol must be a finite number, 0 or more, whose square is finite in float32")
        self.min_samples, self.max_samples, self.tol, self.tol2 = min_samples, max_samples, float(t), tol2
        self._list_work = self._list_index = self._list_count = None

    def _open_list(self, block, n, index, count, stream):
        """qr_pt_adapt_open_list_async on `block`, a state of n columns; index, count: the caller's, or the accumulator's own"""
        import torch
        scene = self.scene
        if index is None:
            if self._list_index is None:
                self._list_index = _new("int32", (n,), scene.device)
            index = self._list_index
        if count is None:
            if self._list_count is None:
                self._list_count = torch.zeros((1,), dtype=torch.int32, device=f"cuda:{scene.device}")
            count = self._list_count
        index, count = _need("index", index, _LIST, (n,), scene.device), _need("count", count, _LIST, (1,), scene.device)
        if self._list_work is None:
            nbytes = ctypes.c_uint64()
            _check(lib().qr_pt_adapt_list_work_bytes(scene._h, n, ctypes.byref(nbytes)))
            self._list_work = _new("int32", (max(1, nbytes.value // 4),), scene.device)
        _check(lib().qr_pt_adapt_open_list_async(scene._h, block.data_ptr(), n, self.min_samples, self.max_samples,
                                                 float(self.tol2), index.data_ptr(), count.data_ptr(),
                                                 self._list_work.data_ptr(), 0, Scene._stream_ptr(stream)))
        return index, count

    def _open_counter(self, open, samples, most, stream):
        """the open counter of a step: None, a new one-element tensor or the caller's, zeroed on `stream` once `samples`
        (1..most), the last thing a step checks, has passed"""
        dev = self.scene.device
        opent = None
        if open is True:
            opent = _new("int32", (1,), dev)
        elif not (open is False or open is None):
            if not (_fits(open, _LIST, None, dev) and open.numel() == 1):
                raise QrError(f"open must be True, False or a one-element int32 or uint32 tensor on cuda:{dev}")
            opent = open
        if not isinstance(samples, int):
            raise QrError("samples must be an integer")
        if not 1 <= samples <= most:
            raise QrError(f"samples must be 1..{most}")
        if opent is not None:
            import torch
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
                opent.zero_()
        return opent


class PtViews(_Accumulator):
    """A path-traced accumulation over caller cameras (Scene.pt_views; include/qrhip.h qr_pt_views_async).

    state: int32 [N, 4, H * W * samples_per_pixel] on the scene's device -- per view the generator states (plane 0) and the
    float32 running means of r, g, b (planes 1..3, bits in int32 slots), slot (y * W + x) * samples_per_pixel + k.
    samples: how many samples the state holds.  step() adds more; the state and `samples` are all there is to checkpoint.
    The scene's own path-tracer mode (set_pt) neither matters nor is touched."""

    def __init__(self, scene, views, width=None, height=None, state=None, samples=0):
        _, (_, n, w, h), _ = scene._views_src(views, width, height)
        self.scene, self.views, self.width, self.height = scene, views, w, h
        self.slots = (w * h) << scene.info.fsaa
        self._adopt(lib().qr_pt_views_state_bytes, (n, w, h), (n, PT_VIEWS_STATE_WORDS, self.slots), state, samples)

    def reset(self):
        """Restart the accumulation: seeds as rays.pt_seeds in every view, means 0, samples 0.  Synchronous (qr_pt_views_reset)."""
        _check(lib().qr_pt_views_reset(self.scene._h, self.views.shape[0], self.width, self.height, self.state.data_ptr()))
        self.samples = 0

    def clone(self):
        """A checkpoint: an accumulator with a copy of the state (on the current stream) that continues independently."""
        return PtViews(self.scene, self.views, self.width, self.height, self.state.clone(), self.samples)

    def step(self, samples=1, frames=None, mean=False, stream=None):
        """Add `samples` (1 .. PT_VIEWS_MAX_SAMPLES) samples to every pixel sample of every view in ONE launch and return the
        packed running-mean frames (int32 [N, H, W]; a new tensor unless given); with mean=True (or a float32 [N, H, W, 3]
        tensor to fill) also the pixels' linear colours after the FSAA reduce, before gamma and packing: (frames, mean).
        The scene's current depth (set_depth) applies.  Asynchronous on `stream`."""
        n, h, w, dev = self.views.shape[0], self.height, self.width, self.scene.device
        frames = _fill("frames", frames, "int32", (n, h, w), dev)
        mean = _wanted("mean", mean, "float32", (n, h, w, 3), dev)
        if not isinstance(samples, int):
            raise QrError("samples must be an integer")
        _check(lib().qr_pt_views_async(self.scene._h, self.views.data_ptr(), n, w, h, self.state.data_ptr(), self.samples, samples,
                                       frames.data_ptr(), _ptr(mean), 0, Scene._stream_ptr(stream)))
        if n > 0:
            self.samples += samples
        return (frames, mean) if mean is not None else frames


class PtRays(_Accumulator):
    """A path-traced accumulation over caller rays (Scene.pt_rays; include/qrhip.h qr_pt_rays_async).

    state: int32 [4, N] on the scene's device -- the generator states (plane 0) and the float32 running means of r, g, b
    (planes 1..3, bits in int32 slots), ray i in column i; the host may edit it.  samples: how many samples the state holds.
    step() adds more; the state and `samples` are all there is to checkpoint.  The state belongs to the accumulation, not to a
    ray set: rays and spread may differ from step to step.  The scene's own path-tracer mode (set_pt) neither matters nor is
    touched."""

    def __init__(self, scene, n, state=None, samples=0):
        if not (isinstance(n, int) and n >= 0):
            raise QrError("n must be the non-negative number of rays")
        self.scene, self.n = scene, n
        self._adopt(lib().qr_pt_rays_state_bytes, (n,), (PT_RAYS_STATE_WORDS, n), state, samples)

    def reset(self):
        """Restart the accumulation: seeds as rays.pt_seeds(n, 1, 1), means 0, samples 0.  Synchronous (qr_pt_rays_reset)."""
        _check(lib().qr_pt_rays_reset(self.scene._h, self.n, self.state.data_ptr()))
        self.samples = 0

    def clone(self):
        """A checkpoint: an accumulator with a copy of the state (on the current stream) that continues independently."""
        return PtRays(self.scene, self.n, self.state.clone(), self.samples)

    def step(self, rays, samples=1, spread=None, rgb=True, stream=None):
        """Add `samples` (1 .. PT_RAYS_MAX_SAMPLES) path-tracer samples to every ray in ONE launch: rays float32 [N, 8] as for
        Scene.trace; spread: None or float32 [N, 8] = (du xyz, pad, dv xyz, pad), along which every sample's direction is
        jittered (rays.pt_jitter, rays.spread_rays).  Returns the running means after the call, float32 [N, 3] linear colour
        before any clamp (a new tensor with rgb=True, or the given tensor filled), or None with rgb=False.  The scene's
        current depth (set_depth) applies.  Asynchronous on `stream`."""
        rays, spread, rgb = self._ray_args(rays, spread, rgb)
        if not isinstance(samples, int):
            raise QrError("samples must be an integer")
        _check(lib().qr_pt_rays_async(self.scene._h, rays.data_ptr(), _ptr(spread), self.n, self.state.data_ptr(), self.samples,
                                      samples, _ptr(rgb), 0, Scene._stream_ptr(stream)))
        if self.n > 0:
            self.samples += samples
        return rgb


class PtAdaptive(_Adaptive):
    """An adaptive path-traced accumulation over caller rays (Scene.pt_adaptive; include/qrhip.h qr_pt_adapt_rays_async).

    state: int32 [8, N] on the scene's device, ray i in column i -- plane 0 the generator states, planes 1..3 the float32
    running means of r, g, b (as PtRays keeps them), plane 4 the number of samples the ray holds, planes 5..7 Welford's M2 of
    r, g, b (float32 bits in int32 slots).  counts: a view of plane 4.  The state is all there is: the host may read it, edit
    it, copy it and continue from it.  tol2: float32(tol) * float32(tol), the squared tolerance the stop rule uses
    (rays.pt_adapt_open states the rule, rays.pt_adapt_fold the update).  A wave of 64 consecutive rays runs as long as its
    slowest ray; open_list() writes the indices of the rays still open, on the device, and step(..., index=, count=) serves 64
    listed rays per wave instead -- a ray's result depends on nothing but its own column, ray and spread, so the state is bit
    for bit the plain step's (rays.pt_adapt_open_list, rays.pt_adapt_fold_list)."""

    def __init__(self, scene, n, min_samples, max_samples, tol, state=None):
        if not (isinstance(n, int) and n >= 0):
            raise QrError("n must be the non-negative number of rays")
        self._rule(min_samples, max_samples, tol)
        self.scene, self.n = scene, n
        self._adopt(lib().qr_pt_adapt_state_bytes, (n,), (PT_ADAPT_STATE_WORDS, n), state)

    @property
    def counts(self):
        """plane 4 of the state (a view): the number of samples every ray holds"""
        return self.state[4]

    def reset(self):
        """Restart the accumulation: seeds as rays.pt_seeds(n, 1, 1), every other plane 0.  Synchronous (qr_pt_adapt_reset)."""
        _check(lib().qr_pt_adapt_reset(self.scene._h, self.n, self.state.data_ptr()))

    def clone(self):
        """A checkpoint: an accumulator with a copy of the state (on the current stream) that continues independently."""
        return PtAdaptive(self.scene, self.n, self.min_samples, self.max_samples, self.tol, self.state.clone())

    def open_list(self, index=None, count=None, stream=None):
        """The open list of the state (qr_pt_adapt_open_list_async): index[:count] = the indices of the rays the stop rule would
        still let take a sample, ascending; index[count:] is not written.  Returns (index int32 [n], count int32 [1]), the
        accumulator's own tensors (allocated on first use, written again by every call) or the caller's.  Nothing is read back:
        hand both to step(..., index=, count=).  The work buffer belongs to the accumulator.  Asynchronous on `stream`."""
        return self._open_list(self.state, self.n, index, count, stream)

    def step(self, rays, samples=1, spread=None, rgb=True, open=False, stream=None, index=None, count=None, cap=None):
        """Offer every ray up to `samples` (1 .. PT_ADAPT_MAX_SAMPLES) candidate samples in ONE launch; a ray takes them while the
        stop rule on its own column lets it.  rays, spread and rgb as for PtRays.step; rgb holds the means of every ray, taken
        or not.  open: False, True (a new one-element int32 tensor) or a one-element int32 / uint32 tensor on the scene's
        device; step zeroes it on `stream` and the launch adds the number of rays that would still take a sample.  Returns rgb,
        or (rgb, open) when open is wanted.  The scene's current depth applies.  Asynchronous on `stream`.
        index, count: step the LISTED rays only (qr_pt_adapt_list_rays_async), 64 list entries per wave -- index an int32 or
        uint32 tensor of ray indices on the scene's device (open_list()'s, or any list of distinct indices; an entry >= n is
        skipped), count a one-element tensor there holding the list's length, which is read on the device.  cap: the host's upper
        bound on that length, at most len(index); it sizes the launch and defaults to n or len(index), whichever is less; the
        `open` read back after a step is the next open list's length.  The first min(cap, count) entries are served.  rgb rows
        of unlisted rays are NOT written; open counts listed rays only.  The state is bit for bit what the plain step gives on
        the listed columns; the others are untouched."""
        import torch
        n, dev = self.n, self.scene.device
        if index is None:
            if count is not None or cap is not None:
                raise QrError("count and cap belong to a list: pass index")
        else:
            if count is None:
                raise QrError("index needs count: a one-element tensor holding the list's length (open_list() returns both)")
            if not (isinstance(index, torch.Tensor) and index.dim() == 1):      # any length: only then is there a shape to ask for
                raise QrError(f"index must be a contiguous {_LIST} [length] tensor on cuda:{dev}")
            index, count = _need("index", index, _LIST, (index.shape[0],), dev), _need("count", count, _LIST, (1,), dev)
            if cap is None:
                cap = min(n, index.shape[0])
            if not (isinstance(cap, int) and 0 <= cap <= index.shape[0]):
                raise QrError(f"cap must be an integer, 0..{index.shape[0]}: it bounds the entries of index that are read")
        rays, spread, rgb = self._ray_args(rays, spread, rgb)
        opent = self._open_counter(open, samples, PT_ADAPT_MAX_SAMPLES, stream)
        # the list entry point takes (index, count, cap) after the state; everything else is the plain step's
        fn, listed = (lib().qr_pt_adapt_rays_async, ()) if index is None else \
                     (lib().qr_pt_adapt_list_rays_async, (index.data_ptr(), count.data_ptr(), cap))
        _check(fn(self.scene._h, rays.data_ptr(), _ptr(spread), n, self.state.data_ptr(), *listed, samples, self.min_samples,
                  self.max_samples, float(self.tol2), _ptr(rgb), _ptr(opent), 0, Scene._stream_ptr(stream)))
        return (rgb, opent) if opent is not None else rgb


class PtAdaptiveViews(_Adaptive):
    """An adaptive path-traced accumulation over caller cameras (Scene.pt_adaptive_views; include/qrhip.h
    qr_pt_adapt_views_async).

    state: int32 [N, 8, H * W * samples_per_pixel] on the scene's device, slot (y * W + x) * samples_per_pixel + k -- per view
    planes 0..3 as PtViews keeps them (generator states, float32 running means of r, g, b), plane 4 the number of samples the
    slot holds, planes 5..7 Welford's M2 of r, g, b: state[j] is a PtAdaptive state of `slots` columns.  counts: a view of plane
    4, [N, slots].  The state is all there is: the host may read it, edit it, copy it and continue from it.  tol2:
    float32(tol) * float32(tol).  The rule is per slot (rays.pt_adapt_open on state[j]), the update rays.pt_adapt_fold's.  A
    wave is one footprint and runs as long as its slowest slot."""

    def __init__(self, scene, views, width=None, height=None, min_samples=0, max_samples=64, tol=0.0, state=None):
        _, (_, n, w, h), _ = scene._views_src(views, width, height)
        self._rule(min_samples, max_samples, tol)
        self.scene, self.views, self.width, self.height = scene, views, w, h
        self.slots = (w * h) << scene.info.fsaa
        self._adopt(lib().qr_pt_adapt_views_state_bytes, (n, w, h), (n, PT_ADAPT_STATE_WORDS, self.slots), state)

    @property
    def counts(self):
        """plane 4 of the state (a view), [N, slots]: the number of samples every pixel sample holds"""
        return self.state[:, 4]

    def variance(self, out=None, unknown=1.0, stream=None):
        """The variance per pixel of the running mean (qr_pt_adapt_views_variance_async; rays.pt_adapt_view_variance): per slot
        Welford's M2 summed over r, g, b, divided by 3 m (m - 1), `unknown` where the slot holds fewer than 2 samples; per pixel
        the sum over its slots divided by their number squared.  What Scene.atrous / Scene.denoise take as `variance`.
        Returns float32 [N, H, W] (a new tensor unless given).  The state is only read.  Asynchronous on `stream`."""
        n, h, w = self.views.shape[0], self.height, self.width
        out = _fill("out", out, "float32", (n, h, w), self.scene.device)
        try:
            unknown = float(unknown)
        except (TypeError, ValueError):
            raise QrError("unknown must be a number") from None
        _check(lib().qr_pt_adapt_views_variance_async(self.scene._h, self.state.data_ptr(), n, w, h, unknown, out.data_ptr(), 0,
                                                      Scene._stream_ptr(stream)))
        return out

    def reset(self):
        """Restart the accumulation: seeds as rays.pt_seeds in every view, every other plane 0.  Synchronous
        (qr_pt_adapt_views_reset)."""
        _check(lib().qr_pt_adapt_views_reset(self.scene._h, self.views.shape[0], self.width, self.height, self.state.data_ptr()))

    def clone(self):
        """A checkpoint: an accumulator with a copy of the state (on the current stream) that continues independently."""
        return PtAdaptiveViews(self.scene, self.views, self.width, self.height, self.min_samples, self.max_samples, self.tol,
                               self.state.clone())

    def open_list(self, view, index=None, count=None, stream=None):
        """The open list of one view's block (qr_pt_adapt_open_list_async on state[view] with n = slots): index[:count] = the
        slots of that view the stop rule would still let take a sample, ascending; index[count:] is not written.  Returns
        (index int32 [slots], count int32 [1]), the accumulator's own tensors (allocated on first use, written again by every
        call) or the caller's.  Asynchronous on `stream`."""
        if not (isinstance(view, int) and 0 <= view < self.views.shape[0]):
            raise QrError(f"view must be an integer, 0..{self.views.shape[0] - 1}")
        return self._open_list(self.state[view], self.slots, index, count, stream)

    def step(self, samples=1, frames=None, mean=False, counts=False, open=False, stream=None):
        """Offer every pixel sample of every view up to `samples` (1 .. PT_ADAPT_VIEWS_MAX_SAMPLES) candidate samples in ONE
        launch; a slot takes them while the stop rule on its own column lets it.  Returns the packed running-mean frames (int32
        [N, H, W]; a new tensor unless given), every pixel written.  mean: as PtViews.step (float32 [N, H, W, 3]).  counts:
        False, True or an int32 [N, H, W] tensor: the samples every pixel holds, summed over its slots.  open: False, True or a
        one-element int32 / uint32 tensor on the scene's device; step zeroes it on `stream` and the launch adds the number of
        slots that would still take a sample.  Returns frames alone, or the tuple (frames, mean, counts, open) without the ones
        not wanted.  The scene's current depth (set_depth) applies.  Asynchronous on `stream`."""
        n, h, w, dev = self.views.shape[0], self.height, self.width, self.scene.device
        frames = _fill("frames", frames, "int32", (n, h, w), dev)
        mean = _wanted("mean", mean, "float32", (n, h, w, 3), dev)
        counts = _wanted("counts", counts, "int32", (n, h, w), dev)
        opent = self._open_counter(open, samples, PT_ADAPT_VIEWS_MAX_SAMPLES, stream)
        _check(lib().qr_pt_adapt_views_async(self.scene._h, self.views.data_ptr(), n, w, h, self.state.data_ptr(), samples,
                                             self.min_samples, self.max_samples, float(self.tol2), frames.data_ptr(), _ptr(mean),
                                             _ptr(counts), _ptr(opent), 0, Scene._stream_ptr(stream)))
        out = (frames,) + tuple(t for t in (mean, counts, opent) if t is not None)
        return out if len(out) > 1 else frames


class Temporal:
    """A temporal accumulation over the frames of moving cameras (Scene.temporal; include/qrhip.h qr_reproject_views_async;
    rays.Temporal is its chain in numpy).

    It owns two history tensors (float32 [N, H, W, 8]: c0 c1 c2 c3 m1 m2 len 0 per pixel) that it alternates between, and
    clones of the last step's hit records and cameras: a copy of 48 B per pixel and step, on the step's stream, so that the
    caller may reuse its own tensors at once.  `frames`: steps since the start or the last reset().  Static scenes under a
    moving camera, and with step(motion=, scene=) scenes animated through hierarchy_apply; with clamp= (a rays.clamp_stops
    block) every step holds the history to the frame's neighbourhood colours (qr_reproject_clamped_async); the stops (normal_min, plane_max,
    ...: rays.reproject_stops) are starting points, not tuned."""

    def __init__(self, scene, n_views, width, height, channels=3, clamp=None, **params):
        if not (all(isinstance(x, int) and not isinstance(x, bool) and x >= 1 for x in (n_views, width, height)) and channels in (3, 4)):
            raise QrError("n_views, width and height must be positive integers and channels 3 or 4")
        self.scene, self.shape, self.channels = scene, (n_views, height, width), channels
        self.params = _stops("reproject_stops", QrError, **params)
        self._clamp = Scene._clamp_arg(clamp)
        self.clamp = None if clamp is None else dict(clamp)
        self._hist = [_new("float32", self.shape + (8,), scene.device) for _ in range(2)]
        self._cur, self._hits, self._views, self.frames = 0, None, None, 0

    def reset(self):
        """The next step is a first frame: every pixel fresh.  Nothing is launched."""
        self._hits = self._views = None
        self.frames = 0

    def clone(self):
        """A checkpoint: an accumulator with copies of the history, records and cameras (on the current stream) that continues
        independently."""
        other = Temporal(self.scene, self.shape[0], self.shape[2], self.shape[1], self.channels, clamp=self.clamp)
        other.params = dict(self.params)
        other._cur, other.frames = self._cur, self.frames
        if self._hits is not None:
            other._hist[self._cur].copy_(self._hist[self._cur])
            other._hits, other._views = self._hits.clone(), self._views.clone()
        return other

    @property
    def history(self):
        """the entries after the last step, float32 [N, H, W, 8] (a view: the step after next overwrites it); None before the first"""
        return None if self._hits is None else self._hist[self._cur]

    @property
    def length(self):
        """the history length per pixel after the last step, a float32 [N, H, W] view of `history`; None before the first"""
        return None if self._hits is None else self._hist[self._cur][..., 6]

    def step(self, colour, hits, views, variance=None, stream=None, motion=None, scene=None):
        """One frame: colour (float32 [N, H, W, channels]), hits (view_hits of `views`) and views (float32 [N, 16], this frame's
        cameras) against the frame before; variance and motion as for Scene.reproject.  scene: the Scene to launch on, by
        default the one the accumulator was made with -- an animated host uploads a new Scene every frame and may close the
        old one; the reprojection reads nothing of a scene but its device, which must be the accumulator's (QrError).
        Returns (colour, variance), new tensors: the accumulated colour -- demodulated with demodulate=True:
        Scene.atrous(modulate=True) as the last filter pass multiplies back -- and its variance, what Scene.denoise takes.
        Asynchronous on `stream`."""
        import torch
        scn = self.scene if scene is None else scene
        if not isinstance(scn, Scene) or scn.device != self.scene.device:
            raise QrError(f"scene must be a Scene on the accumulator's device cuda:{self.scene.device}")
        motion = scn._motion_arg(motion)
        n, h, w = self.shape
        if not (_fits(colour, "float32", (n, h, w, self.channels)) and _fits(views, "float32", (n, 16), scn.device)):
            raise QrError(f"this accumulation holds float32 colour [{n}, {h}, {w}, {self.channels}] and views [{n}, 16] on cuda:{scn.device}")
        prev = None if self._hits is None else (self._views, self._hits, self._hist[self._cur])
        dims, prev, outs = scn._reproject_args(colour, hits, prev, variance, self._hist[self._cur ^ 1], True, True, False)
        scn._reproject_launch(colour, hits, variance, prev, dims, self.params, outs, stream, motion, self._clamp)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            self._hits, self._views = hits.clone(), views.clone()
        self._cur ^= 1
        self.frames += 1
        return outs[1], outs[2]


class MultiRender:
    """Prepared multi-target launch (qr_render_multi_async): targets = [(scene, frame tensor, row_begin, row_end)].
    The ctypes argument arrays are built once; call it with a stream to launch."""

    def __init__(self, targets):
        n = len(targets)
        self.n = n
        self._keep = targets
        self._scenes = (ctypes.c_void_p * n)(*[t[0]._h.value for t in targets])
        self._frames = (ctypes.c_void_p * n)(*[t[1].data_ptr() for t in targets])
        self._r0 = (ctypes.c_int * n)(*[int(t[2]) for t in targets])
        self._r1 = (ctypes.c_int * n)(*[int(t[3]) for t in targets])

    def __call__(self, stream=None):
        _check(lib().qr_render_multi_async(self.n, self._scenes, self._frames, self._r0, self._r1, Scene._stream_ptr(stream)))
