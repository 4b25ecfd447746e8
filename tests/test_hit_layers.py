"""Hit layers (include/qrhip.h qr_layer_rays_async / qr_layer_views_async; Scene.trace_layers, Scene.view_layers): the first k hits
along caller rays and behind the pixels of caller cameras, in order, in one launch.

The truth is a composition of pieces the oracle already covers: rays.layers_of (pinned below against a scalar loop of single
np.float32 steps) over oracle.trace_rays(..., "trace") gives count, t and ids; the record of layer j is the oracle's hit record
(tests/hitrec_oracle.c through test_hit_records._helper) of that layer's ray, rays.next_rays applied j times.  Every comparison is
bit for bit: t as uint32, records with test_hit_records._same_records, no tolerance and no element left out.
"""
import ctypes
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import _rayq
import _rayset as RS
from conftest import ROOT, load_blob
from test_hit_records import ASM, GUARD_LIB, _cuda, _helper, _ray_sets, _rays_mod, _rs_scene, _same_records
from test_ray_query import ORIGIN_CASES, _blob

FLT_MAX = np.finfo(np.float32).max
CAMERA_CASES = ["demo01_160", "demo02_160", "demo03_160", "synth_small"]
K_VALUES = [1, 2, 3, 12]
VIEW_SIZES = [(64, 64), (67, 45), (9, 130)]
VIEW_CASES = ["demo01_160", "demo03_160", "synth_small"]


@pytest.fixture(scope="module")
def rays_mod():
    return _rays_mod()


@pytest.fixture(scope="module")
def helper():
    return _helper()


# ------------------------------------------------------------------------------------------------------------- the truth

def _trace_of(oracle, blob):
    return lambda r: oracle.trace_rays(blob, r, "trace", threads=16)


_TRUTH = {}


def _truth(oracle, rays_mod, blob, rays, k, key=None):
    """(count int32 [N], t float32 [k, N], ids int32 [k, N]): rays.layers_of over the oracle's closest-hit query.  With `key` the
    result is computed once and shared (it is never written to)."""
    if key is not None and (key, k) in _TRUTH:
        return _TRUTH[(key, k)]
    out = rays_mod.layers_of(_trace_of(oracle, blob), rays, k)
    if key is not None:
        _TRUTH[(key, k)] = out
    return out


def _prefix(truth, k):
    """the truth of k layers from the truth of more: the first k planes, and the hits among them"""
    _, t, ids = truth
    assert k <= len(t)
    return (ids[:k] >= 0).sum(axis=0).astype(np.int32), t[:k], ids[:k]


def _layer_rays(rays_mod, rays, truth):
    """[k] ray batches: layer j's rays, next_rays applied j times"""
    _, t, ids = truth
    out, cur = [], np.ascontiguousarray(rays, dtype=np.float32)
    for j in range(len(t)):
        out.append(cur)
        cur = rays_mod.next_rays(cur, t[j], ids[j])
    return out


def _truth_records(helper, rays_mod, blob, rays, truth):
    """float32 [k, N, 12]: the oracle's hit record of every layer's ray; its t and id are the planes of `truth`, bit for bit"""
    _, t, ids = truth
    rec = np.stack([helper(blob, r) for r in _layer_rays(rays_mod, rays, truth)])
    assert (rec[:, :, 3].view(np.uint32) == t.view(np.uint32)).all() and (rec.view(np.int32)[:, :, 7] == ids).all(), \
        "the two truth sources disagree: the hit-record helper and layers_of over the oracle's trace"
    return rec


def _np(x):
    return None if x is None else x.cpu().numpy()


def _same(where, rays, got, want, want_rec=None):
    """count, t and ids of a call against the truth, every element; records too where the call returned them"""
    cnt, t, ids = (_np(a) for a in got[:3])
    w_cnt, w_t, w_ids = want
    k = len(w_t)
    n = w_cnt.size
    assert cnt.dtype == np.int32 and cnt.size == n, f"{where}: count is {cnt.dtype} {cnt.shape}"
    bad = cnt.reshape(-1) != w_cnt
    assert not bad.any(), (f"{where}: {int(bad.sum())} of {n} counts differ; first at {int(np.nonzero(bad)[0][0])}: "
                           f"got {cnt.reshape(-1)[bad][0]} want {w_cnt[bad][0]}")
    if t is not None:
        assert t.dtype == np.float32 and t.shape[0] == k and t.size == k * n, f"{where}: t is {t.dtype} {t.shape}"
        bad = t.reshape(k, n).view(np.uint32) != w_t.view(np.uint32)
        assert not bad.any(), (f"{where}: {int(bad.sum())} of {k * n} t differ in some bit; first at (layer, element) "
                               f"{np.argwhere(bad)[0].tolist()}: got {t.reshape(k, n)[bad][0]!r} want {w_t[bad][0]!r}")
    if ids is not None:
        assert ids.dtype == np.int32 and ids.shape[0] == k and ids.size == k * n, f"{where}: ids is {ids.dtype} {ids.shape}"
        bad = ids.reshape(k, n) != w_ids
        assert not bad.any(), (f"{where}: {int(bad.sum())} of {k * n} ids differ; first at (layer, element) "
                               f"{np.argwhere(bad)[0].tolist()}: got {ids.reshape(k, n)[bad][0]} want {w_ids[bad][0]}")
    if want_rec is not None:
        rec = _np(got[3])
        assert rec.dtype == np.float32 and rec.shape[0] == k and rec.shape[-1] == 12 and rec.size == k * n * 12, f"{where}: hits is {rec.shape}"
        for j in range(k):
            _same_records(f"{where} layer {j}", rays, rec[j].reshape(n, 12), want_rec[j])


# ------------------------------------------------------------------------------------------------------------------- CPU

def test_symbols_in_library(qr):
    L = ctypes.CDLL(qr.LIB_PATH)
    for sym in ("qr_layer_rays_async", "qr_layer_views_async"):
        assert hasattr(L, sym), sym
        assert sym in qr.ABI_SYMBOLS
    assert qr.LAYER_MAX == 64
    hdr = open(os.path.join(ROOT, "include", "qrhip.h")).read()
    assert "#define QR_LAYER_MAX 64" in hdr
    assert "int qr_layer_rays_async(" in hdr and "int qr_layer_views_async(" in hdr


# hand-made rows and a hand-made world: along every ray the same surfaces, at these t (two of them one ulp apart, one behind the
# origin); the closest-hit query over it in single np.float32 comparisons
_T_SURF = [np.float32(-0.5), np.float32(1.0), np.float32(2.0), np.nextafter(np.float32(2.0), np.float32(4.0)), np.float32(5.0)]


def _hand_rows():
    r = np.zeros((7, 8), dtype=np.float32)
    r[:, 4:7] = (0, 0, 1)
    r[:, 0] = np.arange(7)
    r[0, 3], r[0, 7] = 0.0, np.inf              # +inf tmax: four layers, then the miss value FLT_MAX
    r[1, 3], r[1, 7] = -1.0, 3.0                # negative tmin: the surface behind the origin counts
    r[2, 3], r[2, 7] = 1.0, 2.0                 # tmin and tmax ON surfaces: neither counts, nothing between
    r[3, 3], r[3, 7] = 0.5, 0.5                 # an empty interval
    r[4, 3], r[4, 7] = 5.0, np.inf              # ended before it began, unbounded
    r[5, 3], r[5, 7] = -np.inf, 6.0             # everything
    r[6, 3], r[6, 7] = 1.5, np.nextafter(np.float32(2.0), np.float32(4.0))      # tmax ON the surface one ulp behind 2
    return r


def _hand_trace_row(tmin, tmax):
    tmax = np.float32(FLT_MAX) if tmax > np.float32(FLT_MAX) else np.float32(tmax)
    for i, ts in enumerate(_T_SURF):
        if np.float32(tmin) < ts and ts < tmax:
            return ts, np.int32(2 * i)
    return tmax, np.int32(-1)


def _hand_trace(rays):
    out = [_hand_trace_row(r[3], r[7]) for r in rays]
    return (np.array([o[0] for o in out], dtype=np.float32).reshape(-1), np.array([o[1] for o in out], dtype=np.int32).reshape(-1))


def _hand_layers_scalar(rays, k):
    """the stated composition, one ray and one np.float32 at a time"""
    n = len(rays)
    cnt = np.zeros(n, dtype=np.int32)
    t = np.zeros((k, n), dtype=np.float32)
    ids = np.zeros((k, n), dtype=np.int32)
    for i in range(n):
        tmin, tmax = np.float32(rays[i, 3]), np.float32(rays[i, 7])
        ended = False
        for j in range(k):
            if ended:
                tj, ij = (np.float32(FLT_MAX) if tmax > np.float32(FLT_MAX) else tmax), np.int32(-1)
            else:
                tj, ij = _hand_trace_row(tmin, tmax)
            t[j, i], ids[j, i] = tj, ij
            if ij >= 0:
                cnt[i] += 1
                tmin = tj
            else:
                ended = True
    return cnt, t, ids


def test_next_rays_and_layers_of_pinned(rays_mod):
    import torch
    rays = _hand_rows()
    # next_rays: tmin = t where the ray hit; tmin = tmax, +inf taken as FLT_MAX, where it ended; the rest untouched
    t0, i0 = _hand_trace(rays)
    assert i0.tolist() == [2, 0, -1, -1, -1, 0, 4]
    want = rays.copy()
    for i in range(len(rays)):
        want[i, 3] = t0[i] if i0[i] >= 0 else (np.float32(FLT_MAX) if rays[i, 7] > np.float32(FLT_MAX) else rays[i, 7])
    assert want[4, 3] == FLT_MAX and np.isinf(want[4, 7]) and want[2, 3] == 2.0 and want[3, 3] == 0.5 and want[1, 3] == -0.5
    for conv in (lambda a: a, torch.from_numpy):
        src = rays.copy()
        got = np.asarray(rays_mod.next_rays(conv(src), conv(t0.copy()), conv(i0.copy())))
        assert got.dtype == np.float32 and (got.view(np.uint32) == want.view(np.uint32)).all()
        assert (src.view(np.uint32) == rays.view(np.uint32)).all(), "next_rays wrote to its input"
    # an ended ray stays ended: its interval is empty, the query answers the miss value
    t1, i1 = _hand_trace(want)
    assert (i1[i0 < 0] == -1).all() and t1[4] == FLT_MAX and t1[2] == 2.0
    for k in (1, 2, 5, 7):
        w_cnt, w_t, w_ids = _hand_layers_scalar(rays, k)
        cnt, t, ids = rays_mod.layers_of(_hand_trace, rays, k)
        assert cnt.dtype == np.int32 and t.dtype == np.float32 and ids.dtype == np.int32
        assert t.shape == (k, 7) and ids.shape == (k, 7) and cnt.shape == (7,)
        assert (cnt == w_cnt).all() and (ids == w_ids).all() and (t.view(np.uint32) == w_t.view(np.uint32)).all(), k
    cnt, t, ids = rays_mod.layers_of(_hand_trace, rays, 7)
    assert cnt.tolist() == [4, 4, 0, 0, 0, 5, 1]
    assert ids[:, 0].tolist() == [2, 4, 6, 8, -1, -1, -1] and t[4, 0] == FLT_MAX          # +inf tmax
    assert ids[:, 1].tolist() == [0, 2, 4, 6, -1, -1, -1] and t[4:, 1].tolist() == [3.0] * 3   # from behind the origin up to tmax
    assert t[1, 0] == 2.0 and t[2, 0] == np.nextafter(np.float32(2.0), np.float32(4.0)), "hits one ulp apart are both kept"
    assert ids[:, 6].tolist() == [4] + [-1] * 6, "a surface ON tmax does not count"
    hit = ids >= 0
    for i in range(7):
        th = t[hit[:, i], i]
        assert (np.diff(th) > 0).all(), "t is not strictly increasing over a ray's hits"
    # resuming: k1 layers, then k2 on next_rays of the last plane, are one call with k1 + k2
    c2, t2, i2 = rays_mod.layers_of(_hand_trace, rays, 2)
    c3, t3, i3 = rays_mod.layers_of(_hand_trace, rays_mod.next_rays(rays, t2[-1], i2[-1]), 3)
    c5, t5, i5 = rays_mod.layers_of(_hand_trace, rays, 5)
    assert (np.concatenate([t2, t3]).view(np.uint32) == t5.view(np.uint32)).all() and (np.concatenate([i2, i3]) == i5).all()
    assert (c2 + c3 == c5).all()
    for bad in (rays[:, :7], rays.astype(np.float64)):
        with pytest.raises(ValueError):
            rays_mod.next_rays(bad, t0, i0)
    with pytest.raises(ValueError):
        rays_mod.next_rays(rays, t0[:3], i0[:3])
    with pytest.raises(ValueError):
        rays_mod.layers_of(_hand_trace, rays, 0)


def test_layer_kernels_in_resource_check():
    """the build's register check knows the four hit-layer instances, allows them no vector spill and no private segment and
    no more registers than the hit-record instance each one mirrors, and the build's assembly passes it"""
    import importlib.util
    path = os.path.join(ROOT, "tools", "check_kernel_resources.py")
    spec = importlib.util.spec_from_file_location("check_kernel_resources", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    frags = sorted(f for f in m.LIMITS if "qr_layer_kernel" in f)
    assert len(frags) == 4
    for f in frags:
        mirror = f.replace("15qr_layer_kernel", "13qr_hit_kernel")
        assert mirror in m.LIMITS, f
        assert m.LIMITS[f][1] == 0 and m.LIMITS[f][2] == 0 and m.LIMITS[f][0] <= m.LIMITS[mirror][0] <= 168, f
    assert m.LIMITS["15qr_layer_kernelILb1ELb0ELb1EE"][0] == 128
    r = subprocess.run([sys.executable, path, ASM, "--print"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("qr_layer_kernel") == 4


def _seeded_views(rays_mod, blob, seed, n=8):
    return [rays_mod.view_of(c) for c in _rayq.random_cameras(blob, seed, n=n, size=64)]


def test_inputs_have_layers(oracle, rays_mod):
    """conditions on the inputs of the GPU tests, on the CPU oracle alone, so that none of them passes vacuously"""
    # demo01_160's camera rays at its own size: many rays with three layers and more, at most 8
    blob = load_blob("demo01_160")
    rays = rays_mod.camera_rays(blob)
    cnt, t, ids = _truth(oracle, rays_mod, blob, rays, 12, key="demo01_160 camera")
    print(f"demo01_160 camera: {int((cnt >= 3).sum())} of {len(cnt)} rays with >= 3 layers, max {int(cnt.max())}")
    assert (cnt >= 3).sum() >= 2000 and cnt.max() == 8
    # t strictly increases over a ray's hits, and the planes from `count` on hold the miss values
    for j in range(1, 12):
        both = ids[j] >= 0
        assert (ids[j - 1][both] >= 0).all() and (t[j][both] > t[j - 1][both]).all()
    tmax = np.where(rays[:, 7] > FLT_MAX, FLT_MAX, rays[:, 7]).astype(np.float32)
    assert (t[ids < 0] == np.tile(tmax, (12, 1))[ids < 0]).all()
    # mixed waves: some group of 64 consecutive rays (one wave of a caller-ray launch) has lanes that end at different layers
    g = cnt[: len(cnt) // 64 * 64].reshape(-1, 64)
    mixed = int((g.min(axis=1) != g.max(axis=1)).sum())
    print(f"demo01_160 camera: {mixed} of {len(g)} waves have lanes that end at different layers")
    assert mixed >= 10
    # the own camera at 64x64 crops to a corner: at most 2 layers; views use the own size or seeded cameras instead
    c64 = _truth(oracle, rays_mod, blob, rays_mod.view_rays(rays_mod.view_of(blob), 64, 64, blob), 12)[0]
    assert c64.max() <= 2
    # demo03_160's camera rays reach 11 layers
    blob3 = load_blob("demo03_160")
    c3 = _truth(oracle, rays_mod, blob3, rays_mod.camera_rays(blob3), 12, key="demo03_160 camera")[0]
    print(f"demo03_160 camera: max {int(c3.max())} layers")
    assert c3.max() == 11
    # of the 24 seeded views of demo03_160 (8 cameras, 3 sizes) at least 12 have >= 100 pixels with >= 3 layers
    good = 0
    for (w, h) in VIEW_SIZES:
        for v in _seeded_views(rays_mod, blob3, 1):
            c = _truth(oracle, rays_mod, blob3, rays_mod.view_rays(v, w, h, blob3), 3)[0]
            good += int((c >= 3).sum() >= 100)
    print(f"demo03_160: {good} of 24 seeded views have >= 100 pixels with >= 3 layers")
    assert good >= 12


def test_far_family_saturates_the_count(qr, oracle, rays_mod, tmp_path):
    """the `far` family on synth_small has rays with more than 64 hits: count == k == 64, "there may be more" """
    name = "synth_small"
    blob = RS.scene_blob(name)
    _, img = RS.query_image(qr, name, tmp_path)
    rays = RS.far(blob, name, RS.reach_of(img))
    c65 = _truth(oracle, rays_mod, blob, rays, 65)[0]
    c64 = _truth(oracle, rays_mod, blob, rays, 64, key="synth_small far")[0]
    print(f"synth_small far: {int((c65 > 64).sum())} of {len(rays)} rays with more than 64 hits")
    assert (c65 > 64).sum() >= 10
    assert (c64[c65 > 64] == 64).all() and (c64 == np.minimum(c65, 64)).all()


# ------------------------------------------------------------------------------------------------------------------- GPU

def _sync():
    import torch
    torch.cuda.synchronize()


def _layers(scn, rays, k, **kw):
    out = scn.trace_layers(_cuda(scn, rays), k, **kw)
    _sync()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", CAMERA_CASES)
def test_gpu_layers_camera_rays(qr, oracle, rays_mod, helper, name):
    """k = 1, 2, 3, 12 with and without `coherent`: count, t, ids and records against the truth; layer 0 is Scene.trace"""
    blob = _blob(name)
    rays = rays_mod.camera_rays(blob)
    full = _truth(oracle, rays_mod, blob, rays, 12, key=f"{name} camera")
    rec = _truth_records(helper, rays_mod, blob, rays, full)
    scn = qr.Scene(blob, ray_queries=True)
    try:
        t0, i0 = scn.trace(_cuda(scn, rays))
        _sync()
        for k in K_VALUES:
            for coherent in (False, True):
                got = _layers(scn, rays, k, hits=True, coherent=coherent)
                assert tuple(got[0].shape) == (len(rays),) and tuple(got[1].shape) == (k, len(rays))
                assert tuple(got[2].shape) == (k, len(rays)) and tuple(got[3].shape) == (k, len(rays), 12)
                _same(f"{name} camera k={k} coherent={coherent}", rays, got, _prefix(full, k), rec[:k])
                assert (_np(got[1][0]).view(np.uint32) == _np(t0).view(np.uint32)).all(), f"{name}: layer 0 is not trace()'s t"
                assert (got[2][0] == i0).all().item(), f"{name}: layer 0 is not trace()'s id"
    finally:
        scn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ORIGIN_CASES + ["synth_small_dda", "crowd_flat_dda"])
def test_gpu_layers_edge_families(qr, oracle, rays_mod, helper, name, tmp_path):
    """the adversarial families of tests/_rayset.py (the grid family on the scene whose query list carries a uniform grid) at
    k = 4; on synth_small the far family once more at k = 64, where the count saturates"""
    blob = RS.scene_blob(name)
    off, img = RS.query_image(qr, name, tmp_path)
    scn = _rs_scene(qr, name)
    try:
        for label, rays in _ray_sets(blob, name, oracle, rays_mod, RS.dda_grid(off, img), RS.reach_of(img))[1:]:
            want = _truth(oracle, rays_mod, blob, rays, 4)
            rec = _truth_records(helper, rays_mod, blob, rays, want)
            for coherent in (False, True):
                got = _layers(scn, rays, 4, hits=True, coherent=coherent)
                _same(f"{name} {label} k=4 coherent={coherent}", rays, got, want, rec)
            if name == "synth_small" and label == "far":
                want = _truth(oracle, rays_mod, blob, rays, 64, key="synth_small far")
                assert (want[0] == 64).sum() >= 10
                rec = _truth_records(helper, rays_mod, blob, rays, want)
                for coherent in (False, True):
                    got = _layers(scn, rays, 64, hits=True, coherent=coherent)
                    _same(f"{name} far k=64 coherent={coherent}", rays, got, want, rec)
    finally:
        scn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_gpu_layers_batch_sizes(qr, oracle, rays_mod, helper, n):
    """partial waves at k = 3: nothing is written past n in any plane, and nothing past plane k - 1 (sentinel-filled buffers)"""
    import torch
    name = "synth_small"
    blob = RS.scene_blob(name)
    r = RS.mixed(blob, name, oracle)
    rays = np.concatenate([r] * (n // len(r) + 1))[:n]
    k = 3
    want = _truth(oracle, rays_mod, blob, rays, k)
    rec = _truth_records(helper, rays_mod, blob, rays, want)
    scn = _rs_scene(qr, name)
    try:
        for coherent in (False, True):
            _same(f"{name} n={n} coherent={coherent}", rays, _layers(scn, rays, k, hits=True, coherent=coherent), want, rec)
        # raw call: planes of stride n in buffers with room behind every plane's end and a whole plane behind the last
        dev = f"cuda:{scn.device}"
        cnt = torch.full((n + 64,), 77, dtype=torch.int32, device=dev)
        t = torch.full((k + 1, n), 7.0, dtype=torch.float32, device=dev)
        ids = torch.full((k + 1, n), 77, dtype=torch.int32, device=dev)
        hits = torch.full((k + 1, n, 12), 7.0, dtype=torch.float32, device=dev)
        r_dev = _cuda(scn, rays)
        vp = lambda x: ctypes.c_void_p(x.data_ptr())
        rc = qr.lib().qr_layer_rays_async(scn._h, vp(r_dev), n, k, vp(cnt), vp(t), vp(ids), vp(hits), 0, None)
        _sync()
        assert rc == 0
        assert (cnt[n:] == 77).all().item(), "count written past the end of the batch"
        assert (t[k] == 7.0).all().item() and (ids[k] == 77).all().item() and (hits[k] == 7.0).all().item(), "written past plane k - 1"
        _same(f"{name} n={n} raw", rays, (cnt[:n], t[:k], ids[:k], hits[:k]), want, rec)
        # ... and one element fewer than the buffers' stride: the last element of every plane stays
        if n > 1:
            cnt.fill_(77); t.fill_(7.0); ids.fill_(77); hits.fill_(7.0)
            m = n - 1
            rc = qr.lib().qr_layer_rays_async(scn._h, vp(r_dev), m, k, vp(cnt), vp(t), vp(ids), vp(hits), 0, None)
            _sync()
            assert rc == 0 and (cnt[m:] == 77).all().item()
            flat_t, flat_i, flat_h = t.reshape(-1), ids.reshape(-1), hits.reshape(-1, 12)
            assert (flat_t[k * m:] == 7.0).all().item() and (flat_i[k * m:] == 77).all().item() and (flat_h[k * m:] == 7.0).all().item(), \
                "planes of stride n - 1 written past their end"
            w3 = (want[0][:m], want[1][:, :m], want[2][:, :m])
            _same(f"{name} n={m} raw", rays[:m], (cnt[:m], flat_t[:k * m].reshape(k, m), flat_i[:k * m].reshape(k, m),
                                                 flat_h[:k * m].reshape(k, m, 12)), w3, rec[:, :m])
    finally:
        scn.close()


def _check_view_layers(scn, oracle, rays_mod, helper, blob, where, views, w, h, k, key=None):
    """view_layers of several views in ONE launch, with records, against the truth on view_rays(sample 0)"""
    got = scn.view_layers(_cuda(scn, np.stack(views)), k, w, h, hits=True)
    _sync()
    nv = len(views)
    assert tuple(got[0].shape) == (nv, h, w) and tuple(got[1].shape) == (k, nv, h, w)
    assert tuple(got[2].shape) == (k, nv, h, w) and tuple(got[3].shape) == (k, nv, h, w, 12)
    layered = 0
    for j, v in enumerate(views):
        rays = rays_mod.view_rays(v, w, h, blob, sample=0)
        want = _truth(oracle, rays_mod, blob, rays, k, key=None if key is None else f"{key} view {j} {w}x{h}")
        rec = _truth_records(helper, rays_mod, blob, rays, want)
        _same(f"{where} view {j} at {w}x{h} k={k}", rays, (got[0][j], got[1][:, j], got[2][:, j], got[3][:, j]), want, rec)
        layered += int((want[0] >= min(k, 3)).sum())
    return layered


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["demo01_160", "demo03_160", "demo01_160_gf_aa4"])
def test_gpu_view_layers_own_camera(qr, oracle, rays_mod, helper, name):
    """the snapshot's own camera at the snapshot's size, twice in one launch (two views); the FSAA fixture gives sample 0's rays"""
    blob = load_blob(name)
    fi, _ = _rayq.frame_words(blob)
    w, h = int(fi[31]), int(fi[32])
    v = rays_mod.view_of(blob)
    other = rays_mod.view_of(_rayq.random_cameras(blob, seed=zlib.crc32(name.encode()), n=1)[0])
    scn = qr.Scene(blob, ray_queries=True)
    try:
        layered = _check_view_layers(scn, oracle, rays_mod, helper, blob, name, [v, other], w, h, 5)
        assert layered >= 1000, f"{name}: only {layered} pixels with 3 layers or more"
        # layer 0 is view_hits
        import torch
        got = scn.view_layers(_cuda(scn, v[None]), 2, w, h, hits=True)
        vh = scn.view_hits(_cuda(scn, v[None]), w, h)
        _sync()
        assert torch.equal(got[3][0].view(torch.int32), vh.view(torch.int32)), f"{name}: layer 0 is not view_hits"
    finally:
        scn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", VIEW_CASES)
def test_gpu_view_layers_seeded_cameras(qr, oracle, rays_mod, helper, name):
    """eight seeded cameras among the objects in ONE launch per size, sizes that are no multiple of a footprint, k = 3"""
    blob = _blob(name)
    views = _seeded_views(rays_mod, blob, 1)
    scn = qr.Scene(blob, ray_queries=True)
    layered = 0
    try:
        for (w, h) in VIEW_SIZES:
            layered += _check_view_layers(scn, oracle, rays_mod, helper, blob, name, views, w, h, 3)
    finally:
        scn.close()
    assert layered >= 1000, f"{name}: only {layered} pixels with 3 layers"


@pytest.mark.gpu
def test_gpu_resume(qr, oracle, rays_mod):
    """2 + 3 layers and 1 + 1 + 1 + 1 + 1 layers through rays.next_rays on the device equal one call with k = 5, in every bit"""
    import torch
    blob = load_blob("demo03_160")
    rays_np = rays_mod.camera_rays(blob)
    want = _prefix(_truth(oracle, rays_mod, blob, rays_np, 12, key="demo03_160 camera"), 5)
    assert (want[0] == 5).sum() >= 100 and (want[0] < 5).sum() >= 100
    scn = qr.Scene(blob, ray_queries=True)
    try:
        rays = _cuda(scn, rays_np)
        one = scn.trace_layers(rays, 5, hits=True)
        _sync()
        _same("k=5", rays_np, one[:3], want)
        for split in ([2, 3], [1, 1, 1, 1, 1]):
            cur, cs, ts, iss, hs = rays, [], [], [], []
            for k in split:
                c, t, i, h = scn.trace_layers(cur, k, hits=True)
                cs.append(c); ts.append(t); iss.append(i); hs.append(h)
                cur = rays_mod.next_rays(cur, t[-1], i[-1])
            _sync()
            assert torch.equal(torch.cat(ts).view(torch.int32), one[1].view(torch.int32)), f"{split}: t differs from one call"
            assert torch.equal(torch.cat(iss), one[2]), f"{split}: ids differ from one call"
            assert torch.equal(torch.cat(hs).view(torch.int32), one[3].view(torch.int32)), f"{split}: records differ from one call"
            assert torch.equal(sum(cs), one[0]), f"{split}: counts do not add up"
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_partial_outputs(qr, rays_mod):
    """count-only, t-only and ids-only calls give the full call's fields; the same for views"""
    import torch
    blob = load_blob("demo03_160")
    scn = qr.Scene(blob, ray_queries=True)
    try:
        rays = _cuda(scn, rays_mod.camera_rays(blob))
        views = _cuda(scn, np.stack(_seeded_views(rays_mod, blob, 1, n=2)))
        calls = [("rays", lambda **kw: scn.trace_layers(rays, 6, **kw)),
                 ("rays coherent", lambda **kw: scn.trace_layers(rays, 6, coherent=True, **kw)),
                 ("views", lambda **kw: scn.view_layers(views, 6, 67, 45, **kw))]
        for label, f in calls:
            c, t, i, h = f(hits=True)
            assert (c > 0).any().item() and (c < 6).any().item()
            out = f(t=False, ids=False)
            assert len(out) == 3 and out[1] is None and out[2] is None and torch.equal(out[0], c), f"{label}: count-only"
            out = f(ids=False)
            assert out[2] is None and torch.equal(out[0], c) and torch.equal(out[1].view(torch.int32), t.view(torch.int32)), f"{label}: t-only"
            out = f(t=False)
            assert out[1] is None and torch.equal(out[0], c) and torch.equal(out[2], i), f"{label}: ids-only"
            out = f(t=False, ids=False, hits=True)
            assert out[1] is None and out[2] is None and torch.equal(out[3].view(torch.int32), h.view(torch.int32)), f"{label}: records-only"
            out = f()
            assert len(out) == 3 and torch.equal(out[1].view(torch.int32), t.view(torch.int32)) and torch.equal(out[2], i)
            # the count is the number of hit planes, the records carry the planes
            assert torch.equal((i >= 0).sum(dim=0).to(torch.int32), c)
            assert torch.equal(h[..., 3].view(torch.int32), t.view(torch.int32)) and torch.equal(h.view(torch.int32)[..., 7], i)
        _sync()
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_layers_ignore_path_tracer_mode_and_depth(qr, oracle, rays_mod, helper):
    """nothing is lit: the layers do not depend on the recursion depth or on path-tracer mode"""
    blob = load_blob("demo02_160_gf_d5")
    rays = rays_mod.camera_rays(blob)
    want = _truth(oracle, rays_mod, blob, rays, 4)
    rec = _truth_records(helper, rays_mod, blob, rays, want)
    assert (want[0] >= 3).sum() >= 100
    scn = qr.Scene(blob, ray_queries=True)
    try:
        view = _cuda(scn, rays_mod.view_of(blob)[None])
        scn.set_depth(0)
        _same("depth 0", rays, _layers(scn, rays, 4, hits=True), want, rec)
        scn.set_pt(True)
        _same("path-tracer mode", rays, _layers(scn, rays, 4, hits=True), want, rec)
        got = scn.view_layers(view, 4, hits=True)
        _sync()
        _same("path-tracer mode, view", rays, got, want, rec)
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_refusals(qr, rays_mod):
    import torch
    blob = load_blob("demo01_160")
    L = qr.lib()
    dev = "cuda:0"
    ARG, UNSUP = -1, -3
    rays = torch.from_numpy(rays_mod.camera_rays(blob)[:128]).to(dev)
    w, h = 67, 45
    vt = torch.from_numpy(np.stack([rays_mod.view_of(blob)] * 2)).to(dev)
    k = 4
    # room for the largest call below: QR_LAYER_MAX planes of two views
    cnt = torch.zeros((2 * h * w,), dtype=torch.int32, device=dev)
    tt = torch.zeros((64 * 2 * h * w + 4,), dtype=torch.float32, device=dev)
    ii = torch.zeros((64 * 2 * h * w + 4,), dtype=torch.int32, device=dev)
    hh = torch.zeros((64 * 2 * h * w + 1, 12), dtype=torch.float32, device=dev)
    vp = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)

    def f_rays(s, r=vp(rays), n=64, k=k, c=vp(cnt), t=vp(tt), i=vp(ii), hits=vp(hh), flags=0):
        return L.qr_layer_rays_async(s, r, n, k, c, t, i, hits, flags, None)

    def f_views(s, v=vp(vt), n=2, w=w, h=h, k=k, c=vp(cnt), t=vp(tt), i=vp(ii), hits=vp(hh), flags=0):
        return L.qr_layer_views_async(s, v, n, w, h, k, c, t, i, hits, flags, None)

    plain = qr.Scene(blob)
    for f in (f_rays, f_views):
        assert f(plain._h) == UNSUP
    with pytest.raises(qr.QrError, match="QR_UPLOAD_RAY_QUERIES"):
        plain.trace_layers(rays, 2)
    with pytest.raises(qr.QrError, match="QR_UPLOAD_RAY_QUERIES"):
        plain.view_layers(vt, 2, w, h)
    plain.close()

    scn = qr.Scene(blob, ray_queries=True)
    for f in (f_rays, f_views):
        assert f(None) == ARG
        assert f(scn._h, c=None) == ARG                                                         # count is required
        assert f(scn._h, k=0) == ARG and f(scn._h, k=-1) == ARG and f(scn._h, k=65) == ARG
        assert f(scn._h, c=vp(cnt, 2)) == ARG and f(scn._h, t=vp(tt, 1)) == ARG and f(scn._h, i=vp(ii, 2)) == ARG     # misaligned
        assert f(scn._h, hits=vp(hh, 4)) == ARG and f(scn._h, hits=vp(hh, 8)) == ARG
        assert f(scn._h, flags=2) == ARG and f(scn._h, flags=0x80000000) == ARG
        assert f(scn._h, n=0) == 0 and f(scn._h, None, 0, c=None, t=None, i=None, hits=None) == 0
        assert f(scn._h, n=-1) == ARG
        assert f(scn._h) == 0 and f(scn._h, t=None, i=None, hits=None) == 0 and f(scn._h, t=None) == 0
        assert f(scn._h, k=64, n=1) == 0
    assert f_rays(scn._h, None) == ARG and f_rays(scn._h, vp(rays, 4)) == ARG and f_rays(scn._h, n=1 << 31) == ARG
    assert f_rays(scn._h, flags=1) == 0                                                         # QR_TRACE_COHERENT
    assert f_views(scn._h, flags=1) == ARG
    # views: the limits of qr_hit_views_async
    assert f_views(scn._h, v=None) == ARG and f_views(scn._h, v=vp(vt, 8)) == ARG
    assert f_views(scn._h, w=0) == ARG and f_views(scn._h, h=0) == ARG and f_views(scn._h, w=16385) == ARG
    assert f_views(scn._h, n=65536) == ARG and f_views(scn._h, n=65535, w=16384, h=16384) == ARG
    _sync()
    # the Python layer
    for bad in (rays.double(), rays[:, :7].contiguous(), rays.cpu(), rays[:, ::2], rays.reshape(-1), rays.cpu().numpy()):
        with pytest.raises(qr.QrError, match="rays must be"):
            scn.trace_layers(bad, 2)
    for bad in (vt.double(), vt[:, :15].contiguous(), vt.cpu(), vt[:, ::2], vt.reshape(-1), vt.cpu().numpy()):
        with pytest.raises(qr.QrError, match="views must be"):
            scn.view_layers(bad, 2, w, h)
    for bad_k in (0, 65, -1, 2.5, None):
        with pytest.raises(qr.QrError, match="k must be"):
            scn.trace_layers(rays, bad_k)
        with pytest.raises(qr.QrError, match="k must be"):
            scn.view_layers(vt, bad_k, w, h)
    for bw, bh in ((0, h), (w, -1), (w, 2.5), (16385, h)):
        with pytest.raises(qr.QrError):
            scn.view_layers(vt, 2, bw, bh)
    c, t, i, hits = scn.trace_layers(rays[:0], 3, hits=True)
    assert tuple(c.shape) == (0,) and tuple(t.shape) == (3, 0) and tuple(i.shape) == (3, 0) and tuple(hits.shape) == (3, 0, 12)
    assert c.dtype == torch.int32 and t.dtype == torch.float32 and i.dtype == torch.int32 and hits.dtype == torch.float32
    c, t, i = scn.view_layers(vt[:0], 3, w, h)
    assert tuple(c.shape) == (0, h, w) and tuple(t.shape) == (3, 0, h, w) and tuple(i.shape) == (3, 0, h, w)
    c, t, i = scn.view_layers(vt, 2)                                                           # the snapshot's size by default
    assert tuple(c.shape) == (2, scn.height, scn.width) and tuple(t.shape) == (2, 2, scn.height, scn.width)
    assert tuple(scn.trace_layers(rays, 64)[1].shape) == (64, 128)
    _sync()
    scn.close()


# the same comparisons once through the guarded diagnostic build (make guard: walk statistics on, every cell offset of the per-lane
# walks checked before it is loaded), as tests/test_hit_records.py does: the library is chosen when the package is imported, hence
# the child process: this file run as a script.

def _guard_child():
    from qr_loader import load_package
    qr = load_package()
    assert qr.LIB_PATH == GUARD_LIB, qr.LIB_PATH
    import qr_oracle
    rays_mod, helper = _rays_mod(), _helper()
    done = 0
    for name in ("synth_small", "synth_small_dda"):
        blob = RS.scene_blob(name)
        scn = _rs_scene(qr, name)
        for label, rays in (("camera", rays_mod.camera_rays(blob)), ("mixed", RS.mixed(blob, name, qr_oracle))):
            want = _truth(qr_oracle, rays_mod, blob, rays, 4)
            rec = _truth_records(helper, rays_mod, blob, rays, want)
            for coherent in (False, True):
                _same(f"guard {name} {label} coherent={coherent}", rays, _layers(scn, rays, 4, hits=True, coherent=coherent), want, rec)
        views = [rays_mod.view_of(blob)] + [rays_mod.view_of(c) for c in _rayq.random_cameras(blob, seed=11, n=2)]
        _check_view_layers(scn, qr_oracle, rays_mod, helper, blob, f"guard {name}", views, 67, 45, 4)
        scn.close()
        done += 1
        print(f"{name} guard_ok 1", flush=True)
    return 0 if done == 2 else 1


@pytest.mark.gpu
def test_gpu_guarded_build_gives_the_same_layers():
    assert os.path.exists(GUARD_LIB), "libqrhip_guard.so is missing: build() makes it (make -C quadray-engine_amd/csrc guard)"
    env = dict(os.environ, QR_LIB=GUARD_LIB)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-child"], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.count("guard_ok 1") == 2 and "QR_GUARD" not in out.stderr, out.stdout + out.stderr[-3000:]


if __name__ == "__main__":
    sys.exit(_guard_child() if "--guard-child" in sys.argv else 2)
