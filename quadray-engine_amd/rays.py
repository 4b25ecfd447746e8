"""Ray batches for Scene.trace / Scene.occluded (include/qrhip.h qr_trace_rays_async): one ray per row of a float32 [N, 8]
array, (org x, y, z, tmin, dir x, y, z, tmax) -- the layout of qr_ray.

camera_rays turns a snapshot's camera into such a batch: the primary rays of the render kernel (qr_kernel.hpp, the reference's
tracer.cpp:1287-1322) in its own fp32 operation order, so that tracing them gives the frame's hit ids bit for bit.
"""
import struct

import numpy as np

# qr_frame (include/qr_scene.h) as 49 little-endian 32-bit words
_F_TMAX, _F_DIR, _F_HOR, _F_VER, _F_HORA, _F_VERA = 0, 1, 4, 7, 10, 14
_F_TMIN, _F_ORG, _F_FSAA, _F_W, _F_H = 24, 25, 30, 31, 32


def frame_record(blob):
    """The snapshot's qr_frame as (float32 view, int32 view) of its 49 words (copies)."""
    off = struct.unpack_from("<I", blob, 4 * 10)[0]          # qr_header.off_frame
    w = np.frombuffer(blob, dtype=np.int32, count=49, offset=off).copy()
    return w.view(np.float32), w


def camera_rays(blob, sample=0):
    """Primary rays of every pixel of the snapshot's frame, row-major: float32 [H*W, 8].

    Every step is one IEEE fp32 operation (numpy float32, no fused multiply-add), in the kernel's order:
    hs = x + hor_a, vs = y + ver_a (plus the zero jitter of a non-path-traced frame), the six products hor * hs and
    ver * vs, their sums, then + dir.  tmin / tmax are the frame's t_min / t_max.  `sample`: which FSAA sub-sample
    (0 .. 2^fsaa - 1) of a frame captured with anti-aliasing."""
    f, i = frame_record(blob)
    fsaa, w, h = int(i[_F_FSAA]), int(i[_F_W]), int(i[_F_H])
    if not 0 <= sample < (1 << fsaa):
        raise ValueError(f"sample must be 0..{(1 << fsaa) - 1} for fsaa {fsaa}")
    x = np.tile(np.arange(w, dtype=np.float32), h)
    y = np.repeat(np.arange(h, dtype=np.float32), w)
    if fsaa == 0:
        ai = np.zeros(w * h, dtype=np.int64)
    elif fsaa == 1:
        ai = (np.tile(np.arange(w), h) & 1) * 2 + sample
    else:
        ai = np.full(w * h, sample, dtype=np.int64)
    zero = np.float32(0.0)
    hs = (x + f[_F_HORA:_F_HORA + 4][ai]) + zero
    vs = (y + f[_F_VERA:_F_VERA + 4][ai]) + zero
    out = np.empty((w * h, 8), dtype=np.float32)
    for k in range(3):
        a = f[_F_HOR + k] * hs
        b = f[_F_VER + k] * vs
        out[:, 4 + k] = (a + b) + f[_F_DIR + k]
        out[:, k] = f[_F_ORG + k]
    out[:, 3] = f[_F_TMIN]
    out[:, 7] = f[_F_TMAX]
    return out
