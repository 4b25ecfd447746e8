"""Ray batches for Scene.trace / Scene.occluded / Scene.shade (include/qrhip.h qr_trace_rays_async, qr_shade_rays_async): one
ray per row of a float32 [N, 8] array, (org x, y, z, tmin, dir x, y, z, tmax) -- the layout of qr_ray.

camera_rays turns a snapshot's camera into such a batch: the primary rays of the render kernel (qr_kernel.hpp, the reference's
tracer.cpp:1287-1322) in its own fp32 operation order, so that tracing them gives the frame's hit ids bit for bit.
pack_colors is the frame's output step (clamp, FSAA reduce, gamma, scale, pack) for the linear colours Scene.shade returns.
Together they give the frame that a walk of the global list renders (with the snapshot's own tile lists the frame can differ
only where the engine's tiles hold other surfaces than its global list):

    scn = Scene(blob, ray_queries=True)
    ns = 1 << fsaa                                  # the snapshot's FSAA: 0, 1 or 2
    rgb = torch.stack([scn.shade(torch.from_numpy(camera_rays(blob, sample=k)).cuda()) for k in range(ns)])
    frame = pack_colors(rgb.cpu().numpy(), blob)    # uint32 [H, W], 0x00RRGGBB
"""
import struct

import numpy as np

# qr_frame (include/qr_scene.h) as 49 little-endian 32-bit words
_F_TMAX, _F_DIR, _F_HOR, _F_VER, _F_HORA, _F_VERA = 0, 1, 4, 7, 10, 14
_F_TMIN, _F_ORG, _F_FSAA, _F_W, _F_H = 24, 25, 30, 31, 32
_F_CLAMP, _F_CMASK, _F_FLAGS = 18, 19, 28
PROP_GAMMA = 0x40                                           # QR_PROP_GAMMA in qr_frame.ctx_flags


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


def _cvt_near(x):
    """the kernel's cvt_near: round to nearest even; outside the int32 range (and NaN) 0x80000000"""
    f = np.rint(x)
    ok = (f >= np.float32(-2147483648.0)) & (f < np.float32(2147483648.0))
    return np.where(ok, np.where(ok, f, np.float32(0)).astype(np.int64), np.int64(-2147483648))


def pack_colors(rgb, blob):
    """The frame's output step (qr_kernel.hpp XX_end) for the linear colours Scene.shade gives for camera_rays(blob, sample=k),
    k = 0 .. 2^fsaa - 1: rgb float32 [H*W, 3] (fsaa 0) or [ns, H*W, 3] (sample k in row k).  Returns the uint32 [H, W] frame.

    Every step is one IEEE fp32 operation (numpy float32, no fused operations), in the kernel's order: clamp1 of each sample
    (x < 1 ? x : 1); the FSAA reduce -- every sample * 0.5, samples (0, 1) and (2, 3) added, and for 4x once more * 0.5 and the
    two sums added; the square root when ctx_flags holds QR_PROP_GAMMA; * clamp, round to nearest even, & cmask, packed as
    r << 16 | g << 8 | b."""
    f, i = frame_record(blob)
    fsaa, w, h = int(i[_F_FSAA]), int(i[_F_W]), int(i[_F_H])
    ns = 1 << fsaa
    c = np.asarray(rgb)
    if c.ndim == 2:
        c = c[None]
    if c.dtype != np.float32 or c.shape != (ns, w * h, 3):
        raise ValueError(f"rgb must be float32 [{w * h}, 3] or [{ns}, {w * h}, 3] for this snapshot (fsaa {fsaa}), got "
                         f"{c.dtype} {list(c.shape)}")
    one, half = np.float32(1.0), np.float32(0.5)
    c = np.where(c < one, c, one)                           # clamp1: NaN gives 1 as well
    if fsaa >= 1:
        c = c * half
        c = np.stack([c[0] + c[1]] if fsaa == 1 else [c[0] + c[1], c[2] + c[3]])
    if fsaa >= 2:
        c = c * half
        c = (c[0] + c[1])[None]
    c = c[0]
    if int(i[_F_FLAGS]) & PROP_GAMMA:
        c = np.sqrt(c)
    c = c * f[_F_CLAMP]
    q = _cvt_near(c) & np.int64(np.uint32(i[_F_CMASK]))
    p = (q[:, 0] << 16) | (q[:, 1] << 8) | q[:, 2]
    return (p & np.int64(0xFFFFFFFF)).astype(np.uint32).reshape(h, w)
