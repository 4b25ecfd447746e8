"""Helpers of tests/test_ray_query.py: snapshot rewrites that make an oracle frame the answer to a ray query, and the host-side
facts (surfaces, CHECK_SHAD) the tests check query results against."""
import struct

import numpy as np

PROP_LIGHT, PROP_TRANSP, PROP_REFRACT = 0x10, 0x400, 0x2000


def _hdr(blob):
    return struct.unpack_from("<26I", blob, 0)


def one_tile(blob):
    """The snapshot with ONE tile that spans the frame and holds the global list `clist` (nothing else changed)."""
    b = bytearray(blob)
    off_frame = _hdr(b)[10]
    fi = np.frombuffer(b, dtype=np.int32, count=49, offset=off_frame).copy()
    fi[34], fi[35], fi[36], fi[37] = fi[31], fi[32], 1, 1           # tile_w, tile_h = frm_w, frm_h; one tile
    b[off_frame:off_frame + 196] = fi.tobytes()
    struct.pack_into("<I", b, 4 * 8, 1)                             # n_tiles
    struct.pack_into("<i", b, _hdr(b)[15], int(fi[38]))             # tiles[0] = clist
    return bytes(b)


def with_frame(blob, w=None, h=None, org=None, dir=None, hor=None, ver=None, t_min=None):
    """The snapshot rewritten to fsaa 0, depth 0, no path tracing, the whole frame in one call (index 0 of 1) and ONE tile
    that spans the frame and holds the global list `clist`: what a walk of the global list from this camera sees.
    Camera fields and the frame size may be replaced."""
    b = bytearray(blob)
    off_frame = _hdr(b)[10]
    fi = np.frombuffer(b, dtype=np.int32, count=49, offset=off_frame).copy()
    ff = fi.view(np.float32)
    for val, at in ((dir, 1), (hor, 4), (ver, 7), (org, 25)):
        if val is not None:
            ff[at:at + 3] = np.asarray(val, dtype=np.float32)
    if t_min is not None:
        ff[24] = np.float32(t_min)
    if w is not None:
        fi[31] = w
    if h is not None:
        fi[32] = h
    fi[33] = fi[31]                                                 # frm_row
    fi[29], fi[30], fi[41] = 0, 0, 0                                # depth, fsaa, pt_on
    fi[39], fi[40] = 0, 1                                           # index, thnum
    b[off_frame:off_frame + 196] = fi.tobytes()
    return one_tile(bytes(b))


def frame_words(blob):
    fi = np.frombuffer(blob, dtype=np.int32, count=49, offset=_hdr(blob)[10]).copy()
    return fi, fi.view(np.float32)


def surfaces(blob):
    """qr_surface records (include/qr_scene.h) as a [n_srf, 64] int32 array and its float32 view."""
    h = _hdr(blob)
    s = np.frombuffer(blob, dtype=np.int32, count=h[4] * 64, offset=h[11]).reshape(h[4], 64).copy()
    return s, s.view(np.float32)


def real_surfaces(blob):
    s, _ = surfaces(blob)
    return np.nonzero((s[:, 37] >= 0) & (s[:, 37] < 9))[0]          # srf_t[3]: tag of a real surface


def casts(blob):
    """[n_srf, 2] bool: does a hit on side 0 / 1 of the surface cast a shadow (CHECK_SHAD: light surfaces and transparent
    surfaces that do not refract do not)"""
    s, _ = surfaces(blob)
    p = s[:, 42:44]
    return ~(((p & PROP_LIGHT) != 0) | (((p & PROP_TRANSP) != 0) & ((p & PROP_REFRACT) == 0)))


def scene_box(blob):
    """low / high corner of the real surfaces' positions"""
    _, f = surfaces(blob)
    p = f[real_surfaces(blob), 0:3].astype(np.float64)
    return p.min(axis=0), p.max(axis=0)


def random_cameras(blob, seed, n=8, size=64, jitter=None):
    """n seeded cameras among the objects: origin at a real surface's position plus a jitter of a few scene units, aimed at
    another surface's position, random orthogonal hor / ver (60 degrees across the frame); t_min 0 for the first half,
    the snapshot's own for the rest.  Returns [(snapshot rewritten to that camera, size x size)]."""
    rng = np.random.default_rng(seed)
    _, f = surfaces(blob)
    _, ff = frame_words(blob)
    real = real_surfaces(blob)
    lo, hi = scene_box(blob)
    ext = float(np.max(hi - lo)) if len(real) > 1 else 1.0
    jit = jitter if jitter is not None else max(0.02 * ext, 1e-3)
    out = []
    for c in range(n):
        a, b = rng.choice(real, 2, replace=False)
        org = f[a, 0:3].astype(np.float64) + rng.uniform(-jit, jit, 3)
        tgt = f[b, 0:3].astype(np.float64)
        fwd = tgt - org
        if np.linalg.norm(fwd) < 1e-6:
            fwd = rng.normal(size=3)
        fwd /= np.linalg.norm(fwd)
        up = rng.normal(size=3)
        hor = np.cross(fwd, up); hor /= np.linalg.norm(hor)
        ver = np.cross(fwd, hor)
        s = np.tan(np.radians(30.0)) / (size / 2)
        hor *= s; ver *= s
        d = fwd - hor * (size / 2) - ver * (size / 2)
        t_min = 0.0 if c < n // 2 else float(ff[24])
        out.append(with_frame(blob, w=size, h=size, org=org, dir=d, hor=hor, ver=ver, t_min=t_min))
    return out
