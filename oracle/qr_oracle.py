"""TEST INFRASTRUCTURE: ctypes binding of oracle/libqr_oracle.so (the CPU restatement).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libqr_oracle.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(LIB_PATH)
        L.qro_render.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                 ctypes.c_int, ctypes.c_void_p]
        L.qro_render.restype = ctypes.c_int
        L.qro_render2.argtypes = L.qro_render.argtypes + [ctypes.c_int]
        L.qro_render2.restype = ctypes.c_int
        L.qro_last_flops.restype = ctypes.c_uint64
        L.qro_info.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        L.qro_info.restype = ctypes.c_int
        L.qro_hash.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
        L.qro_hash.restype = ctypes.c_uint64
        L.qro_trace_rays.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p]
        L.qro_trace_rays.restype = ctypes.c_int
        L.qro_render_pt.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.qro_render_pt.restype = ctypes.c_int
        L.qro_pt_trace_sample.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                          ctypes.c_void_p]
        L.qro_pt_trace_sample.restype = ctypes.c_int
        _lib = L
    return _lib


def info(blob):
    out = (ctypes.c_int32 * 8)()
    buf = ctypes.create_string_buffer(blob, len(blob))
    rc = lib().qro_info(buf, len(blob), out)
    if rc != 0:
        raise RuntimeError(f"qro_info rc={rc}")
    return dict(w=out[0], h=out[1], fsaa=out[2], depth=out[3], n_srf=out[4], n_elm=out[5], index=out[6], thnum=out[7])


def render(blob, depth=-1, threads=0, want_ids=False, rows=None, index=0, thnum=1, deferred=False):
    """Render a snapshot on the CPU. Returns (frame uint32 [h,w], ids or None, counts dict).
    deferred=False is the reference's semantics (every depth-test winner is shaded);
    deferred=True shades only the final hit (same pixels, the HIP backend's ray count)."""
    i = info(blob)
    w, h = i["w"], i["h"]
    frame = np.zeros((h, w), dtype=np.uint32)
    ids = np.full((h, w), -1, dtype=np.int32) if want_ids else None
    counts = (ctypes.c_uint64 * 4)()
    buf = ctypes.create_string_buffer(blob, len(blob))
    r0, r1 = rows if rows is not None else (0, h)
    rc = lib().qro_render2(buf, len(blob), frame.ctypes.data, ids.ctypes.data if want_ids else None,
                           depth, r0, r1, index, thnum, threads, counts, 1 if deferred else 0)
    if rc != 0:
        raise RuntimeError(f"qro_render rc={rc}")
    return frame, ids, dict(primary=counts[0], shadow=counts[1], reflect=counts[2], refract=counts[3],
                            flops=int(lib().qro_last_flops()))


def frame_hash(frame):
    f = np.ascontiguousarray(frame, dtype=np.uint32)
    return int(lib().qro_hash(f.ctypes.data, f.size))


_MODES = {"trace": 0, "occluded": 1, "shade": 2}


def trace_rays(blob, rays, mode, depth=None, threads=0):
    """Caller rays (float32 [N, 8], qr_ray layout) against the snapshot's global list, restated on the CPU
    (qro_trace_rays): the answers of Scene.trace / Scene.occluded / Scene.shade.
      mode "trace":    (t float32 [N], id int32 [N])
      mode "occluded": occ bool [N]
      mode "shade":    (rgb float32 [N, 3] before clamp1, first hit's id int32 [N]) at `depth` (None: the snapshot's)"""
    r = np.ascontiguousarray(rays, dtype=np.float32)
    if r.ndim != 2 or r.shape[1] != 8:
        raise ValueError(f"rays must be [N, 8], got {list(r.shape)}")
    n = r.shape[0]
    t = np.zeros(n, dtype=np.float32)
    ids = np.full(n, -1, dtype=np.int32)
    occ = np.zeros(n, dtype=np.uint8)
    rgb = np.zeros((n, 3), dtype=np.float32)
    buf = ctypes.create_string_buffer(blob, len(blob))
    rc = lib().qro_trace_rays(buf, len(blob), r.ctypes.data, n, _MODES[mode], -1 if depth is None else int(depth),
                              threads, t.ctypes.data, ids.ctypes.data, occ.ctypes.data, rgb.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"qro_trace_rays rc={rc}")
    if mode == "trace":
        return t, ids
    if mode == "occluded":
        return occ.astype(bool)
    return rgb, ids


_PT_ORDERS = {"reference": 0, "kernel": 1}
PT_STATS = ("roulette_draws", "roulette_deaths", "bounces", "split_reflect", "split_refract", "split_tir_skipped")
PT_STAGES = ("jitter_h", "jitter_v", "roulette", "bounce_r", "bounce_phi", "split")


def render_pt(blob, frames, depth=-1, order="reference", threads=0, want_mean=False, want_stats=False):
    """Path tracer on the CPU (qro_render_pt): `frames` accumulated frames from fresh seeds, the last packed frame.
    order "reference": every depth-test winner is shaded at once, as the reference does (pinned to tests/golden/pt);
    order "kernel": numbers are drawn for the final hit of a walk only, children in the fast kernel's order
    ("Path-tracer instance").  The result does not depend on `threads`.
    Returns the frame uint32 [h, w]; with want_mean / want_stats a tuple (frame[, mean float32 [h, w, 3]][, stats dict
    with the keys PT_STATS, counted over all samples and frames])."""
    i = info(blob)
    w, h = i["w"], i["h"]
    frame = np.zeros((h, w), dtype=np.uint32)
    mean = np.zeros((h, w, 3), dtype=np.float32) if want_mean else None
    stats = (ctypes.c_uint64 * 6)()
    buf = ctypes.create_string_buffer(blob, len(blob))
    rc = lib().qro_render_pt(buf, len(blob), int(frames), int(depth), _PT_ORDERS[order], int(threads), frame.ctypes.data,
                             mean.ctypes.data if want_mean else None, stats)
    if rc != 0:
        raise RuntimeError(f"qro_render_pt rc={rc}")
    out = [frame]
    if want_mean:
        out.append(mean)
    if want_stats:
        out.append(dict(zip(PT_STATS, (int(v) for v in stats))))
    return frame if len(out) == 1 else tuple(out)


def pt_trace_sample(blob, frames, x, y, k=0, depth=-1, order="kernel", cap=4096):
    """Debug aid (qro_pt_trace_sample): the numbers one sample draws over `frames` frames, in drawing order, as a list of
    (level, stage name, value), and the sample's running-mean colour float32 [3]."""
    out = np.zeros((cap, 3), dtype=np.float32)
    col = np.zeros(3, dtype=np.float32)
    buf = ctypes.create_string_buffer(blob, len(blob))
    n = lib().qro_pt_trace_sample(buf, len(blob), int(frames), int(depth), _PT_ORDERS[order], int(x), int(y), int(k),
                                  out.ctypes.data, cap, col.ctypes.data)
    if n < 0:
        raise RuntimeError(f"qro_pt_trace_sample rc={n}")
    return [(int(l), PT_STAGES[int(s)], float(v)) for l, s, v in out[:n]], col
