"""Adversarial ray families for tests/test_ray_edges.py: caller rays that camera fans never send.

Every generator is deterministic (seeded by zlib.crc32 of the scene name) and returns float32 [N, 8] in qr_ray layout
(org x, y, z, tmin, dir x, y, z, tmax).  The families:
  axis       parallel bundles along +-x, +-y, +-z from a lattice of origins inside and outside the scene box; the zero
             components are +0.0 in one copy and -0.0 in the other
  near_axis  the axis rays with the zeros replaced by +-1e-20, +-1e-30, +-1e-38 and +-1.4e-45 (both sides of the box
             cull's 1e-30 substitution, and denormals)
  grid       only on lists with a uniform grid (QR_LISTF_DDA): origins exactly on cell faces, edges and corners and on the
             grid box, rays inside a cell-face plane, rays through the box's edges and corners, sparse waves
  interval   tmin / tmax at exactly an oracle hit's t and the floats next to it, tmin == tmax, tmin > tmax, tmax = 0 and a
             denormal, tmin = -1, -extent and -FLT_MAX from origins in the middle of the scene
  scale      random rays inside the box with dir * 2^k, k in {-60, -40, -20, 0, 20, 40}, and tmin / tmax * 2^-k
  far        origins 1e3 and 1e6 scene extents away, aimed at surfaces, and origins just inside and just outside the
             image's reach (the largest origin coordinate the kernel's culls are used for)
  probe      rays that start at earlier hit points, hemisphere directions, tmin 0 or 1e-4 * t (AO and light probes)
  mixed      all of them concatenated and shuffled (an odd count)

The crowd_* scenes hold engine-authored surfaces of every tag, axis map and min/max pattern the fixtures have (tests/_crowd.py).

The scenes (SCENES) and how each is uploaded (environment of the image build) live here as well, so that the CPU coverage
test and the GPU tests see the same query lists.
"""
import os
import zlib

import numpy as np

import _rayq

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
DENORM_MIN = np.float32(1.4e-45)

LISTF_DIV, LISTF_LONG, LISTF_WORLD, LISTF_DDA = 1, 2, 4, 16              # qr_program.h QR_LISTF_*
DDA_ENV = {"QR_DDA": "64"}

# name -> (how the snapshot is made, environment at upload)
SCENES = {
    "demo01_160": ("fixture", {}),
    "demo02_160_gf_d5": ("fixture", {}),
    "test05_160_j14": ("fixture", {}),
    "test07_160_j3": ("fixture", {}),
    "swarm_demo01_240": ("fixture", {}),
    "synth_small": ("synth", {}),
    "synth_small_dda": ("synth", DDA_ENV),
    "synth_flat": ("synth_flat", {}),
    "synth_flat_dda": ("synth_flat", DDA_ENV),
    "synth_dense_dda": ("dense", DDA_ENV),
    "crowd_hier": ("crowd_hier", {}),
    "crowd_flat_dda": ("crowd_flat", DDA_ENV),
    "crowd_dense_dda": ("crowd_dense", DDA_ENV),
}
FAMILIES = ["axis", "near_axis", "grid", "interval", "scale", "far", "probe", "mixed"]

_BLOBS = {}


def _synth_mod():
    import importlib
    from qr_loader import load_package
    load_package()
    return importlib.import_module("quadray_engine_amd.synth")


def scene_blob(name):
    """the snapshot of a scene of SCENES"""
    if name not in _BLOBS:
        kind, _ = SCENES[name]
        if kind == "fixture":
            from conftest import load_blob
            b = load_blob(name)
        elif kind in ("synth", "synth_flat"):
            from test_ray_query import SYNTH_SMALL
            b = _synth_mod().make_scene(hierarchy=kind == "synth", **SYNTH_SMALL)
        elif kind == "dense":                   # the dense cloud of test_synth.py (seed 4): many equal depths
            from qr_loader import load_package
            kw = dict(n_objects=900, width=320, height=180, depth=6, box=9.0, seed=4)
            b = load_package().build_lists(_synth_mod().make_scene(shadow_lists=False, **kw))
        else:                                   # engine-authored surfaces of every kind (tests/_crowd.py)
            import _crowd
            if kind == "crowd_hier":            # a long hierarchy: hand-over walk
                b = _crowd.make_crowd(**_crowd.HIER)
            elif kind == "crowd_flat":          # a flat list with four unbounded members, a grid over it
                b = _crowd.make_crowd(**dict(_crowd.OPEN, hierarchy=False))
            else:                               # dense, built lists: list order decides between equal depths
                from qr_loader import load_package
                b = load_package().build_lists(_crowd.make_crowd(**_crowd.DENSE))
        _BLOBS[name] = b
    return _BLOBS[name]


class upload_env:
    """the scene's environment while its image is built (Scene(...) or program_stats)"""
    def __init__(self, name):
        self.env = SCENES[name][1]

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def query_image(qr, name, tmp_path):
    """(DevHeader word 55: the query list's offset with its QR_LISTF_* bits, the dumped image as uint32 words)"""
    p = os.path.join(str(tmp_path), f"qimg_{name}.bin")
    old = os.environ.get("QR_DUMP_IMAGE")
    os.environ["QR_DUMP_IMAGE"] = p
    try:
        with upload_env(name):
            qr.program_stats(scene_blob(name), qr.UPLOAD_RAY_QUERIES)
    finally:
        if old is None:
            del os.environ["QR_DUMP_IMAGE"]
        else:
            os.environ["QR_DUMP_IMAGE"] = old
    img = np.fromfile(p, dtype=np.uint32)
    os.remove(p)
    return int(img[55]), img


def dda_grid(off_query, img):
    """the CDda record in front of a grid-carrying query list (qr_program.h; walk_dda reads it as g0..g3):
    (low corner float32 [3], cells per axis int [3], units per cell float32 [3]), or None without a grid"""
    if not off_query & LISTF_DDA:
        return None
    w = img[((off_query & ~31) - 64) // 4:(off_query & ~31) // 4]
    org = w[0:3].view(np.float32).copy()
    dims = np.array([w[3] & 255, (w[3] >> 8) & 255, (w[3] >> 16) & 255], dtype=np.int64)
    size = w[8:11].view(np.float32).copy()
    return org, dims, size


# ------------------------------------------------------------------------------------------------------------ helpers

def _rng(name, family):
    return np.random.default_rng([zlib.crc32(name.encode()), zlib.crc32(family.encode())])


def _box(blob):
    lo, hi = _rayq.scene_box(blob)
    ext = float(np.max(hi - lo))
    if ext <= 0:
        ext = 1.0
    return lo, hi, ext


def _rays(org, dir, tmin=0.0, tmax=np.inf):
    org = np.asarray(org, dtype=np.float32).reshape(-1, 3)
    dir = np.asarray(dir, dtype=np.float32).reshape(-1, 3)
    n = max(len(org), len(dir))
    out = np.empty((n, 8), dtype=np.float32)
    out[:, 0:3] = org
    out[:, 4:7] = dir
    out[:, 3] = np.asarray(tmin, dtype=np.float32)
    out[:, 7] = np.asarray(tmax, dtype=np.float32)
    return out


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _targets(blob, rng, n):
    _, f = _rayq.surfaces(blob)
    real = _rayq.real_surfaces(blob)
    return f[rng.choice(real, n), 0:3].astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ families

def axis(blob, name):
    """parallel bundles along the six axis directions; every zero component +0.0 in one copy, -0.0 in the other"""
    lo, hi, ext = _box(blob)
    mid = (lo + hi) / 2
    g = np.linspace(-0.2, 1.2, 5)
    out = []
    for k in range(3):
        i, j = [a for a in range(3) if a != k]
        for s in (1.0, -1.0):
            for along in (-0.6, 0.0, 0.5):                          # outside behind, at the box face, inside
                for u in g:
                    for v in g:
                        o = mid.copy()
                        o[i] = lo[i] + u * (hi[i] - lo[i] if hi[i] > lo[i] else ext)
                        o[j] = lo[j] + v * (hi[j] - lo[j] if hi[j] > lo[j] else ext)
                        o[k] = (lo[k] if s > 0 else hi[k]) - s * along * ext
                        d = np.zeros(3); d[k] = s
                        out.append(np.concatenate([o, [0.0], d, [np.inf]]))
    r = np.asarray(out, dtype=np.float32)
    neg = r.copy()
    z = neg[:, 4:7] == 0
    neg[:, 4:7][z] = np.float32(-0.0)
    return np.concatenate([r, neg])


def near_axis(blob, name):
    """the axis rays, zero components replaced by +-1e-20, +-1e-30, +-1e-38, +-1.4e-45 (random sign per component)"""
    rng = _rng(name, "near_axis")
    base = axis(blob, name)
    base = base[: len(base) // 2]
    out = []
    for m in (1e-20, 1e-30, 1e-38, 1.4e-45):
        r = base.copy()
        z = r[:, 4:7] == 0
        sg = rng.choice([-1.0, 1.0], size=z.shape)
        d = r[:, 4:7]
        d[z] = (sg * np.float32(m)).astype(np.float32)[z]
        out.append(r)
    return np.concatenate(out)


def grid(blob, name, g):
    """rays that test the uniform grid's DDA; g = dda_grid(...) (None: an empty family)"""
    if g is None:
        return np.zeros((0, 8), dtype=np.float32)
    rng = _rng(name, "grid")
    org, dims, size = g
    ends = (org + size * dims.astype(np.float32)).astype(np.float32)

    def lattice(axes, n):
        """points with the coordinates of `axes` exactly on cell faces (org + i * size as float32), the others random"""
        p = (org + rng.uniform(0, 1, (n, 3)) * (ends - org)).astype(np.float32)
        for a in axes:
            i = rng.integers(0, dims[a] + 1, n).astype(np.float32)
            p[:, a] = org[a] + i * size[a]
        return p

    def rnd_dir(n):
        return _unit(rng.normal(size=(n, 3))).astype(np.float32)

    # sparse waves, first in the family so that each block of 64 rays is one wave of the kernel: 4 lanes aimed into the box,
    # the other 60 away from it (the segment split and the re-split of walk_dda)
    ext = float(np.max(ends - org))
    mid = (org + ends) / 2
    sparse = []
    for wave in range(4):
        o = mid + _unit(rng.normal(size=(64, 3))) * 2.0 * ext
        d = _unit(o - mid)                                                           # away from the box
        into = rng.choice(64, 4, replace=False)
        d[into] = _unit(mid + rng.uniform(-0.3, 0.3, (4, 3)) * ext - o[into])
        sparse.append(_rays(o, d))
    out = []
    for axes in ((0,), (1,), (2,), (0, 1), (1, 2), (0, 2), (0, 1, 2)):              # faces, edges, corners
        out.append(_rays(lattice(axes, 48), rnd_dir(48)))
    # on the grid box itself: one coordinate at the low or high end, aimed inwards and outwards
    p = lattice((), 96)
    a = rng.integers(0, 3, 96)
    hi_end = rng.integers(0, 2, 96).astype(bool)
    p[np.arange(96), a] = np.where(hi_end, ends[a], org[a])
    out.append(_rays(p, rnd_dir(96)))
    # inside a cell-face plane: the coordinate on a face, its direction component zero
    for a in range(3):
        p = lattice((a,), 48)
        d = rnd_dir(48)
        d[:, a] = 0.0
        out.append(_rays(p, _unit(d.astype(np.float64)).astype(np.float32)))
    # through the box's corners and edges from outside: t_in == t_out or nearly
    c = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64)
    corners = org + c * (ends - org)
    mids = []
    for a in range(3):                                                               # edge midpoints
        for u in (0, 1):
            for v in (0, 1):
                q = np.empty(3); b = [x for x in range(3) if x != a]
                q[a] = (org[a] + ends[a]) / 2; q[b[0]] = (org, ends)[u][b[0]]; q[b[1]] = (org, ends)[v][b[1]]
                mids.append(q)
    pts = np.concatenate([corners, np.array(mids)])
    ext = float(np.max(ends - org))
    d = rnd_dir(len(pts) * 4).astype(np.float64)
    tgt = np.repeat(pts, 4, axis=0)
    o = tgt - d * ext
    out.append(_rays(o, (tgt - o).astype(np.float32)))
    return np.concatenate(sparse + out)


def _hits(blob, oracle, name, n, family):
    """n seeded rays from inside the scene box at surfaces, and the oracle's (t, id) for them"""
    rng = _rng(name, family)
    lo, hi, ext = _box(blob)
    o = lo + rng.uniform(0.1, 0.9, (n, 3)) * np.maximum(hi - lo, 1e-3 * ext)
    d = _targets(blob, rng, n) - o
    d[np.linalg.norm(d, axis=1) < 1e-6] = 1.0
    r = _rays(o, _unit(d))
    t, ids = oracle.trace_rays(blob, r, "trace")
    return r, t, ids


def interval(blob, name, oracle):
    """tmin / tmax at and around oracle hits, degenerate intervals, negative tmin from the middle of the scene"""
    r, t, ids = _hits(blob, oracle, name, 256, "interval")
    h = ids >= 0
    r, t = r[h], t[h]
    up, dn = np.nextafter(t, F32(np.inf)), np.nextafter(t, F32(-np.inf))
    out = []
    for tmx in (t, up, dn):                                     # the hit at the end of the interval
        q = r.copy(); q[:, 7] = tmx; out.append(q)
    for tmn in (t, up, dn):                                     # ... and at its start
        q = r.copy(); q[:, 3] = tmn; out.append(q)
    q = r.copy(); q[:, 3] = t * F32(0.5); q[:, 7] = q[:, 3]; out.append(q)          # tmin == tmax
    q = r.copy(); q[:, 3] = up; q[:, 7] = dn; out.append(q)                          # tmin > tmax
    q = r.copy(); q[:, 7] = 0.0; out.append(q)
    q = r.copy(); q[:, 7] = DENORM_MIN; out.append(q)
    q = r.copy(); q[:, 3] = -DENORM_MIN; q[:, 7] = DENORM_MIN; out.append(q)
    # negative tmin from the middle of the scene: surfaces behind the origin count
    rng = _rng(name, "interval_neg")
    lo, hi, ext = _box(blob)
    mid = (lo + hi) / 2
    o = mid + rng.uniform(-0.25, 0.25, (128, 3)) * np.maximum(hi - lo, 1e-3 * ext)
    d = _unit(_targets(blob, rng, 128) - o)
    for tmn in (-1.0, -ext, -FLT_MAX):
        out.append(_rays(o, d, tmin=tmn))
        out.append(_rays(o, -d, tmin=tmn))                      # the target behind the origin
    q = _rays(o, -d, tmin=-ext, tmax=0.0); out.append(q)         # only what lies behind
    return np.concatenate(out)


def scale(blob, name):
    """random rays inside the box, dir * 2^k and tmin / tmax * 2^-k"""
    rng = _rng(name, "scale")
    lo, hi, ext = _box(blob)
    n = 96
    o = lo + rng.uniform(0, 1, (n, 3)) * np.maximum(hi - lo, 1e-3 * ext)
    d = _unit(np.concatenate([_targets(blob, rng, n // 2) - o[: n // 2], rng.normal(size=(n - n // 2, 3))]))
    tmin = np.where(rng.uniform(size=n) < 0.5, 0.0, 0.01 * ext)
    tmax = np.where(rng.uniform(size=n) < 0.5, np.inf, 2.0 * ext)
    out = []
    for k in (-60, -40, -20, 0, 20, 40):
        s = np.float32(2.0 ** k)
        out.append(_rays(o, d.astype(np.float32) * s, tmin=(tmin.astype(np.float32) / s), tmax=(tmax.astype(np.float32) / s)))
    return np.concatenate(out)


def far(blob, name, reach=None):
    """origins 1e3 and 1e6 extents away, aimed at surfaces; with `reach` (DevHeader::reach of the query image) also origins
    whose largest coordinate is 0.95 and 1.05 times it, on either side of where the kernel stops using its culls"""
    rng = _rng(name, "far")
    lo, hi, ext = _box(blob)
    mid = (lo + hi) / 2
    out = []
    for dist in (1e3, 1e6):
        n = 96
        o = mid + _unit(rng.normal(size=(n, 3))) * dist * ext
        tgt = _targets(blob, rng, n)
        out.append(_rays(o, _unit(tgt - o)))
        out.append(_rays(o, (tgt - o)))                          # not unit: t near 1
    if reach:
        for f in (0.95, 1.05):
            n = 96
            o = rng.uniform(-1, 1, (n, 3)) * f * reach
            k = rng.integers(0, 3, n)
            o[np.arange(n), k] = np.sign(o[np.arange(n), k]) * f * reach
            tgt = _targets(blob, rng, n)
            out.append(_rays(o, _unit(tgt - o)))
    return np.concatenate(out)


def probe(blob, name, oracle):
    """rays from earlier hit points, directions in the hemisphere facing back along the incoming ray, tmin 0 or 1e-4 * t"""
    rng = _rng(name, "probe")
    r, t, ids = _hits(blob, oracle, name, 192, "probe")
    h = ids >= 0
    r, t = r[h], t[h]
    p = (r[:, 0:3] + r[:, 4:7] * t[:, None]).astype(np.float32)
    out = []
    for tmin_f in (0.0, 1e-4):
        d = _unit(rng.normal(size=(len(p), 3)))
        back = -r[:, 4:7].astype(np.float64)
        d = np.where((np.sum(d * back, axis=1) < 0)[:, None], -d, d)
        out.append(_rays(p, d, tmin=(t * np.float32(tmin_f)).astype(np.float32)))
    return np.concatenate(out)


def reach_of(img):
    """DevHeader::reach (word 56) of a dumped image"""
    return float(img[56:57].view(np.float32)[0])


def family(blob, name, fam, oracle, g=None, reach=None):
    """one family's rays for scene `name`; `g`: dda_grid of its query list (grid family), `reach`: reach_of its image (far)"""
    if fam == "axis":
        return axis(blob, name)
    if fam == "near_axis":
        return near_axis(blob, name)
    if fam == "grid":
        return grid(blob, name, g)
    if fam == "interval":
        return interval(blob, name, oracle)
    if fam == "scale":
        return scale(blob, name)
    if fam == "far":
        return far(blob, name, reach)
    if fam == "probe":
        return probe(blob, name, oracle)
    if fam == "mixed":
        return mixed(blob, name, oracle, g, reach)
    raise KeyError(fam)


def mixed(blob, name, oracle, g=None, reach=None):
    """every family, shuffled into incoherent waves; an odd count"""
    rng = _rng(name, "mixed")
    r = np.concatenate([family(blob, name, f, oracle, g, reach) for f in FAMILIES if f != "mixed"])
    r = r[rng.permutation(len(r))]
    return r if len(r) % 2 else r[:-1]
