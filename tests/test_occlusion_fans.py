"""Occlusion fans (include/qrhip.h qr_fan_rays_async / qr_fan_views_async / qr_fan_hits_async; Scene.occlusion, Scene.view_occlusion,
Scene.hit_occlusion): per surface point the number of open directions of a shared direction table, and one bit per direction.

The truth is a composition of pieces the oracle already covers: the oracle's hit records (tests/hitrec_oracle.c through
test_hit_records._helper), rays.fan_rays in numpy (pinned below against a scalar loop of single np.float32 operations), then
oracle.trace_rays(..., "occluded") on the traced rays, then counts and mask words.  The answers are integers: the GPU must give
them in every element, bit for bit, with no tolerance and no element left out.
"""
import ctypes
import math
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import _rayq
import _rayset as RS
from conftest import ROOT, load_blob
from test_hit_records import GUARD_LIB, _cuda, _fields, _helper, _ray_sets, _rays_mod, _rs_scene
from test_ray_query import _blob

INF = float("inf")
EPS, REACH = 1e-3, 2.0
CONDITION_CASES = ["demo01_160", "demo02_160", "demo03_160"]
VIEW_CASES = CONDITION_CASES + ["demo01_160_gf_aa4", "synth_small"]
VIEW_SIZES = [(64, 64), (67, 45), (9, 130)]
K_VALUES = [1, 31, 32, 33, 64, 65]


@pytest.fixture(scope="module")
def rays_mod():
    return _rays_mod()


@pytest.fixture(scope="module")
def helper():
    return _helper()


# ------------------------------------------------------------------------------------------------------------- the truth

def _open_bits(oracle, rays_mod, blob, hits, dirs, eps, reach, flip):
    """(open bool [N, K], traced bool [N, K]) of hit records `hits` (numpy [N, 12]): fan_rays, then the oracle's occlusion query
    on the traced rays"""
    rays, traced = rays_mod.fan_rays(hits, np.ascontiguousarray(dirs, dtype=np.float32), np.float32(eps), np.float32(reach), flip)
    n, k = traced.shape
    occ = np.zeros(n * k, dtype=bool)
    idx = np.nonzero(traced.reshape(-1))[0]
    if len(idx):
        occ[idx] = oracle.trace_rays(blob, rays.reshape(-1, 8)[idx], "occluded", threads=16)
    return traced & ~occ.reshape(n, k), traced


def _pack(open_bits, hid):
    """(open int32 [N], mask uint32 [ceil(K / 32), N]) from open bool [N, K] and the records' ids"""
    n, k = open_bits.shape
    cnt = np.where(hid >= 0, open_bits.sum(axis=1), -1).astype(np.int32)
    planes = np.zeros(((k + 31) // 32, n), dtype=np.uint32)
    for j in range(k):
        planes[j >> 5] |= open_bits[:, j].astype(np.uint32) << np.uint32(j & 31)
    return cnt, planes


def _truth(oracle, rays_mod, blob, hits, dirs, eps, reach, flip):
    bits, _ = _open_bits(oracle, rays_mod, blob, hits, dirs, eps, reach, flip)
    return _pack(bits, _fields(hits)[3])


def _same(where, got_open, got_mask, want_open, want_mask):
    go = got_open.cpu().numpy().reshape(-1)
    assert go.dtype == np.int32 and go.shape == want_open.shape, f"{where}: open is {go.dtype} {go.shape}"
    bad = go != want_open
    assert not bad.any(), (f"{where}: {int(bad.sum())} of {len(go)} counts differ; first at {int(np.nonzero(bad)[0][0])}: "
                           f"got {go[bad][0]} want {want_open[bad][0]}")
    if got_mask is not None:
        gm = got_mask.cpu().numpy().view(np.uint32)
        assert gm.shape[0] == want_mask.shape[0], f"{where}: {gm.shape[0]} mask planes for {want_mask.shape[0]}"
        gm = gm.reshape(gm.shape[0], -1)
        assert gm.shape == want_mask.shape, f"{where}: mask {gm.shape} for {want_mask.shape}"
        bad = gm != want_mask
        assert not bad.any(), (f"{where}: {int(bad.sum())} mask words differ; first at {np.argwhere(bad)[0].tolist()}: "
                               f"got {gm[bad][0]:#x} want {want_mask[bad][0]:#x}")


def _dirs16(rays_mod):
    return rays_mod.sphere_dirs(16)


# ------------------------------------------------------------------------------------------------------------------- CPU

def test_symbols_in_library(qr):
    L = ctypes.CDLL(qr.LIB_PATH)
    for sym in ("qr_fan_rays_async", "qr_fan_views_async", "qr_fan_hits_async"):
        assert hasattr(L, sym), sym
        assert sym in qr.ABI_SYMBOLS
    assert qr.FAN_FLIP == 2 and qr.FAN_MAX_DIRS == 1024
    hdr = open(os.path.join(ROOT, "include", "qrhip.h")).read()
    assert "#define QR_FAN_MAX_DIRS 1024" in hdr and "#define QR_FAN_FLIP 2u" in hdr


def _fan_records():
    """hand-made records: normals whose dot product with the table is exactly 0, -0.0, positive, negative and NaN; a miss"""
    h = np.zeros((7, 12), dtype=np.float32)
    i = h.view(np.int32)
    h[:, 0:3] = [(1, 2, 3), (-1, 0.5, 4), (0, 0, 0), (9, 9, 9), (2, 2, 2), (5, 6, 7), (1, 1, 1)]
    h[0, 4:7] = (0, 0, 1)
    h[1, 4:7] = (np.sqrt(0.5), 0, np.sqrt(0.5))
    h[2, 4:7] = (0, 0, 0)                       # a miss: the stated zeros
    h[3, 4:7] = (np.nan, 0, 1)
    h[4, 4:7] = (0, -1, 0)
    h[5, 4:7] = (-0.0, -0.0, -1)
    h[6, 4:7] = (0.1, 0.2, np.nan)
    i[:, 7] = [4, 9, -1, 2, 0, 7, 3]
    i[:, 11] = [0, 1, -1, 0, 0, 2, 1]
    d = np.array([(0, 0, 1), (1, 0, 0), (0, 1, 0), (0, 0, -1), (1, 0, -1), (-1, 0, 1), (0.3, -0.2, 0.1), (0, -0.0, 0),
                  (1e-20, 1e20, 3), (-2, 0, 0), (0, 0, np.nan)], dtype=np.float32)
    return h, d


def _fan_scalar(h, d, eps, reach, flip):
    """the stated operations, one np.float32 at a time"""
    n, k = len(h), len(d)
    rays = np.zeros((n, k, 8), dtype=np.float32)
    traced = np.zeros((n, k), dtype=bool)
    ids = h.view(np.int32)[:, 7]
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(n):
            nx, ny, nz = (np.float32(v) for v in h[a, 4:7])
            for b in range(k):
                dx, dy, dz = (np.float32(v) for v in d[b, 0:3])
                p0 = np.float32(nx * dx); p1 = np.float32(ny * dy); p2 = np.float32(nz * dz)
                s = np.float32(p0 + p1)
                dot = np.float32(s + p2)
                if flip:
                    if dot < np.float32(0):
                        dx, dy, dz = np.float32(-dx), np.float32(-dy), np.float32(-dz)
                    tr = True
                else:
                    tr = bool(np.float32(0) < dot)
                traced[a, b] = tr and ids[a] >= 0
                rays[a, b] = (h[a, 0], h[a, 1], h[a, 2], np.float32(eps), dx, dy, dz, np.float32(reach))
    return rays, traced


@pytest.mark.parametrize("flip", [False, True])
def test_fan_rays_pinned(rays_mod, flip):
    import torch
    h, d = _fan_records()
    want_r, want_t = _fan_scalar(h, d, 1e-3, INF, flip)
    # what the cases are there for: dot exactly +0.0 and -0.0 (closed without flip, not flipped with it), NaN, a miss
    assert not want_t[2].any() and want_t.any()
    if not flip:
        assert not want_t[0, 1] and not want_t[5, 1] and not want_t[3, 0] and want_t[0, 0] and not want_t[:, 10].any()
    else:
        assert want_t[[0, 1, 3, 4, 5, 6]].all()
        assert want_r[0, 3, 6] == 1.0 and want_r[0, 1, 4] == 1.0 and want_r[5, 1, 4] == 1.0 and want_r[3, 0, 6] == 1.0
    for d_in in (d, np.concatenate([d, np.full((len(d), 1), 7.0, dtype=np.float32)], axis=1)):
        for conv in (lambda a: a, torch.from_numpy):
            r, t = rays_mod.fan_rays(conv(h.copy()), conv(d_in.copy()), 1e-3, INF, flip)
            r, t = np.asarray(r), np.asarray(t)
            assert r.dtype == np.float32 and r.shape == (7, len(d), 8) and t.dtype == bool and t.shape == (7, len(d))
            assert (t == want_t).all()
            assert (r.view(np.uint32) == want_r.view(np.uint32)).all(), "fan_rays differs from the scalar loop in some bit"
    assert "0 < dot" in rays_mod.fan_rays.__doc__
    with pytest.raises(ValueError):
        rays_mod.fan_rays(h, d.astype(np.float64), 1e-3)
    with pytest.raises(ValueError):
        rays_mod.fan_rays(h, d[:, :2], 1e-3)


def test_fan_bits_pinned(rays_mod):
    import torch
    m = np.zeros((2, 3), dtype=np.uint32)
    m[0, 0], m[1, 0] = 0x80000001, 0x1          # directions 0, 31, 32
    m[0, 1] = 0x00000006                        # 1, 2
    m[1, 2] = 0x2                               # 33 (past k = 33: dropped)
    for mm in (m, m.view(np.int32), torch.from_numpy(m.view(np.int32))):
        b = np.asarray(rays_mod.fan_bits(mm, 33))
        assert b.dtype == bool and b.shape == (3, 33)
        assert np.nonzero(b[0])[0].tolist() == [0, 31, 32] and np.nonzero(b[1])[0].tolist() == [1, 2] and not b[2].any()
    b = rays_mod.fan_bits(m.reshape(2, 1, 3), 34)
    assert b.shape == (1, 3, 34) and b[0, 2, 33]
    with pytest.raises(ValueError):
        rays_mod.fan_bits(m, 65)
    with pytest.raises(ValueError):
        rays_mod.fan_bits(m, 32)


def test_sphere_dirs_pinned(rays_mod):
    d = rays_mod.sphere_dirs(16)
    assert d.dtype == np.float32 and d.shape == (16, 3)
    assert (np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0) <= 1e-6).all()
    for i, row in ((0, d[0]), (15, d[15])):
        x = i + 0.5
        z = 1.0 - 2.0 * x / 16
        phi = x * math.pi * (3.0 - math.sqrt(5.0))
        s = math.sqrt(1.0 - z * z)
        want = np.array([s * math.cos(phi), s * math.sin(phi), z], dtype=np.float32)
        assert (row == want).all(), (i, row.tolist(), want.tolist())
    assert d[0].tolist() == [0.12610112130641937, 0.3243335485458374, 0.9375]
    assert d[15].tolist() == [0.3054388761520386, -0.16673584282398224, -0.9375]
    assert (d[:, 2] == (1.0 - 2.0 * (np.arange(16) + 0.5) / 16).astype(np.float32)).all()
    assert rays_mod.sphere_dirs(1).shape == (1, 3)
    with pytest.raises(ValueError):
        rays_mod.sphere_dirs(0)


@pytest.mark.parametrize("name", CONDITION_CASES)
def test_inputs_exercise_both_answers(oracle, rays_mod, helper, name):
    """a condition on the inputs the GPU tests use, on the CPU oracle alone: with sphere_dirs(16), eps 1e-3, reach 2 the traced
    directions are neither all open nor all closed, and the counts spread"""
    blob = load_blob(name)
    hits = helper(blob, rays_mod.camera_rays(blob))
    hid = _fields(hits)[3]
    for flip in (False, True):
        bits, traced = _open_bits(oracle, rays_mod, blob, hits, _dirs16(rays_mod), EPS, REACH, flip)
        n_tr = int(traced.sum())
        n_open = int(bits.sum())
        counts = np.unique(bits.sum(axis=1)[hid >= 0])
        print(f"{name} flip={flip}: {n_tr} traced, {n_open / n_tr:.3f} open, {1 - n_open / n_tr:.3f} occluded, counts {counts.tolist()}")
        assert n_tr > 10000
        assert n_open >= 0.05 * n_tr and (n_tr - n_open) >= 0.05 * n_tr
        assert len(counts) >= 8


def test_fan_kernels_in_resource_check():
    """the build's register check knows the five fan instances and allows them no spill and no private segment"""
    import importlib.util
    path = os.path.join(ROOT, "tools", "check_kernel_resources.py")
    spec = importlib.util.spec_from_file_location("check_kernel_resources", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    frags = sorted(f for f in m.LIMITS if "qr_fan_kernel" in f)
    assert len(frags) == 5
    for f in frags:
        assert m.LIMITS[f][1] == 0 and m.LIMITS[f][2] == 0 and m.LIMITS[f][0] <= 168, f


# ------------------------------------------------------------------------------------------------------------------- GPU

def _sync():
    import torch
    torch.cuda.synchronize()


def _view_truth(oracle, rays_mod, helper, blob, view, w, h):
    return helper(blob, rays_mod.view_rays(view, w, h, blob, sample=0))


def _check_view_fans(scn, oracle, rays_mod, helper, blob, where, views, w, h, dirs, eps=EPS, reach=REACH, flips=(False, True)):
    """view_occlusion of several views in one launch, with mask, against the truth; returns the hit records of the views"""
    hits = np.concatenate([_view_truth(oracle, rays_mod, helper, blob, v, w, h) for v in views])
    for flip in flips:
        opn, msk = scn.view_occlusion(_cuda(scn, np.stack(views)), _cuda(scn, dirs), w, h, eps=eps, reach=reach, flip=flip, mask=True)
        _sync()
        assert tuple(opn.shape) == (len(views), h, w) and tuple(msk.shape) == ((len(dirs) + 31) // 32, len(views), h, w)
        want_o, want_m = _truth(oracle, rays_mod, blob, hits, dirs, eps, reach, flip)
        _same(f"{where} {w}x{h} flip={flip}", opn, msk, want_o, want_m)
    return hits


@pytest.mark.gpu
@pytest.mark.parametrize("name", VIEW_CASES)
def test_gpu_view_occlusion(qr, oracle, rays_mod, helper, name):
    """the snapshot's own camera and two seeded cameras among the objects in ONE launch per size, sizes that are no multiple of
    a footprint, both flip settings, with mask; the FSAA fixture gives sample 0's record"""
    blob = _blob(name)
    views = [rays_mod.view_of(blob)] + [rays_mod.view_of(c) for c in _rayq.random_cameras(blob, seed=zlib.crc32(name.encode()), n=2)]
    scn = qr.Scene(blob, ray_queries=True)
    try:
        for (w, h) in VIEW_SIZES:
            _check_view_fans(scn, oracle, rays_mod, helper, blob, name, views, w, h, _dirs16(rays_mod))
    finally:
        scn.close()


def _occlusion(scn, rays, dirs, **kw):
    out = scn.occlusion(_cuda(scn, rays), _cuda(scn, dirs), EPS, REACH, mask=True, **kw)
    _sync()
    return out


@pytest.mark.gpu
def test_gpu_ray_occlusion_families(qr, oracle, rays_mod, helper):
    """camera rays and the adversarial families of tests/_rayset.py as the rays whose first hits carry the fans"""
    name = "synth_small"
    blob = RS.scene_blob(name)
    dirs = _dirs16(rays_mod)
    scn = _rs_scene(qr, name)
    try:
        for label, rays in _ray_sets(blob, name, oracle, rays_mod):
            hits = helper(blob, rays)
            for flip in (False, True):
                want_o, want_m = _truth(oracle, rays_mod, blob, hits, dirs, EPS, REACH, flip)
                for coherent in (False, True):
                    opn, msk = _occlusion(scn, rays, dirs, flip=flip, coherent=coherent)
                    _same(f"{name} {label} flip={flip} coherent={coherent}", opn, msk, want_o, want_m)
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_ray_occlusion_on_a_grid_list(qr, oracle, rays_mod, helper, tmp_path):
    """fans over a list with a uniform grid and four unbounded members (crowd_flat_dda, tests/_crowd.py): first hits of the
    grid family -- rays on cell faces, sparse waves -- and of the mixed family carry the fans, so that the fan rounds' idle
    lanes are what walk_dda's segment split hands work to"""
    name = "crowd_flat_dda"
    blob = RS.scene_blob(name)
    off, img = RS.query_image(qr, name, tmp_path)
    g = RS.dda_grid(off, img)
    assert g is not None
    dirs = _dirs16(rays_mod)
    scn = _rs_scene(qr, name)
    try:
        for label, rays in (("grid", RS.grid(blob, name, g)), ("mixed", RS.mixed(blob, name, oracle, g, RS.reach_of(img)))):
            hits = helper(blob, rays)
            assert (_fields(hits)[3] >= 0).sum() > 100, label
            for flip in (False, True):
                want_o, want_m = _truth(oracle, rays_mod, blob, hits, dirs, EPS, REACH, flip)
                for coherent in (False, True):
                    opn, msk = _occlusion(scn, rays, dirs, flip=flip, coherent=coherent)
                    _same(f"{name} {label} flip={flip} coherent={coherent}", opn, msk, want_o, want_m)
    finally:
        scn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_gpu_ray_occlusion_batch_sizes(qr, oracle, rays_mod, helper, n):
    """partial waves, with and without `coherent`; nothing is written past the end of open or of a mask plane"""
    import torch
    name = "synth_small"
    blob = RS.scene_blob(name)
    rays = RS.mixed(blob, name, oracle)[:n]
    assert len(rays) == n
    dirs = rays_mod.sphere_dirs(33)
    hits = helper(blob, rays)
    scn = _rs_scene(qr, name)
    try:
        want_o, want_m = _truth(oracle, rays_mod, blob, hits, dirs, EPS, REACH, True)
        for coherent in (False, True):
            opn, msk = _occlusion(scn, rays, dirs, flip=True, coherent=coherent)
            _same(f"{name} n={n} coherent={coherent}", opn, msk, want_o, want_m)
        o = torch.full((n + 64,), 77, dtype=torch.int32, device="cuda:0")
        m = torch.full((2 * n + 64,), 77, dtype=torch.int32, device="cuda:0")
        r_dev, d_dev = _cuda(scn, rays), _cuda(scn, np.concatenate([dirs, np.zeros((33, 1), np.float32)], axis=1))
        vp = lambda x: ctypes.c_void_p(x.data_ptr())
        rc = qr.lib().qr_fan_rays_async(scn._h, vp(r_dev), n, vp(d_dev), 33, EPS, REACH, vp(o), vp(m), qr.FAN_FLIP, None)
        _sync()
        assert rc == 0 and (o[n:] == 77).all().item() and (m[2 * n:] == 77).all().item(), "written past the end of the batch"
        _same(f"{name} n={n} raw", o[:n], m[:2 * n].reshape(2, n), want_o, want_m)
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_whole_wave_of_misses(qr, oracle, rays_mod, helper):
    """a batch in which a whole wave misses: every open is -1 and every mask word 0 there, the hits next to it are served"""
    blob = load_blob("demo01_160")
    cam = rays_mod.camera_rays(blob)
    lo, hi = _rayq.scene_box(blob)
    away = np.zeros((64, 8), dtype=np.float32)
    away[:, 0:3] = hi + 10.0
    away[:, 4:7] = (1.0, 2.0, 3.0)
    away[:, 7] = np.inf
    rays = np.concatenate([away, cam[len(cam) // 2:len(cam) // 2 + 70], away])
    hits = helper(blob, rays)
    assert (_fields(hits)[3][:64] == -1).all() and (_fields(hits)[3][64:134] >= 0).any()
    dirs = rays_mod.sphere_dirs(40)
    scn = qr.Scene(blob, ray_queries=True)
    try:
        for flip in (False, True):
            opn, msk = _occlusion(scn, rays, dirs, flip=flip)
            _same(f"misses flip={flip}", opn, msk, *_truth(oracle, rays_mod, blob, hits, dirs, EPS, REACH, flip))
            assert (opn[:64] == -1).all().item() and (opn[134:] == -1).all().item()
            assert (msk[:, :64] == 0).all().item() and (msk[:, 134:] == 0).all().item()
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_direction_counts_at_mask_word_boundaries(qr, oracle, rays_mod, helper):
    """K = 1, 31, 32, 33, 64, 65 on one 64x64 view: exactly ceil(K / 32) planes, bits past K are 0.  The directions are prefixes of
    one table, so one oracle run over the longest gives every truth."""
    blob = load_blob("demo01_160")
    view = rays_mod.view_of(blob)
    table = rays_mod.sphere_dirs(65)
    hits = _view_truth(oracle, rays_mod, helper, blob, view, 64, 64)
    hid = _fields(hits)[3]
    scn = qr.Scene(blob, ray_queries=True)
    try:
        for flip in (False, True):
            bits, _ = _open_bits(oracle, rays_mod, blob, hits, table, EPS, REACH, flip)
            for k in K_VALUES:
                opn, msk = scn.view_occlusion(_cuda(scn, view[None]), _cuda(scn, table[:k]), 64, 64, eps=EPS, reach=REACH, flip=flip, mask=True)
                _sync()
                assert msk.shape[0] == (k + 31) // 32
                want_o, want_m = _pack(bits[:, :k], hid)
                _same(f"K={k} flip={flip}", opn, msk, want_o, want_m)
                if k & 31:
                    assert (msk[-1].cpu().numpy().view(np.uint32) >> np.uint32(k & 31) == 0).all(), f"K={k}: bits past K are set"
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_whole_table_below_the_horizon(qr, oracle, rays_mod, helper):
    """without flip, a table whose every direction points into the most common plane of the view: those pixels trace nothing
    (whole waves of them take the wave-level skip) and count 0 -- not -1, they are hits"""
    blob = load_blob("demo01_160")
    view = rays_mod.view_of(blob)
    fi, _ = _rayq.frame_words(blob)
    w, h = int(fi[31]), int(fi[32])
    hits = _view_truth(oracle, rays_mod, helper, blob, view, w, h)
    _, _, nrm, hid, _, _ = _fields(hits)
    normals, cnt = np.unique(nrm[hid >= 0], axis=0, return_counts=True)
    floor = normals[np.argmax(cnt)]
    on_floor = (hid >= 0) & (nrm == floor).all(axis=1)
    assert on_floor.sum() >= 2000, "the view shows too little of one plane"
    sph = rays_mod.sphere_dirs(64)
    dirs = sph[sph.astype(np.float64) @ floor.astype(np.float64) < -0.05]
    assert len(dirs) >= 16
    scn = qr.Scene(blob, ray_queries=True)
    try:
        opn, msk = scn.view_occlusion(_cuda(scn, view[None]), _cuda(scn, dirs), w, h, eps=EPS, reach=REACH, mask=True)
        _sync()
        _same("below the horizon", opn, msk, *_truth(oracle, rays_mod, blob, hits, dirs, EPS, REACH, False))
        o = opn.cpu().numpy().reshape(-1)
        assert (o[on_floor] == 0).all() and (o[hid < 0] == -1).all()
    finally:
        scn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["reach_inf", "empty_interval", "tiny_dirs", "huge_dirs"])
def test_gpu_eps_reach_and_direction_lengths(qr, oracle, rays_mod, helper, case):
    """reach = inf; reach smaller than eps (an empty interval: everything traced is open); directions of length 2^-20 and 2^20
    with eps and reach scaled to the same distances (t is in units of |dir|)"""
    blob = load_blob("demo02_160" if case == "reach_inf" else "demo03_160")     # demo02 is a closed room: at reach = inf nearly all is closed
    view = rays_mod.view_of(blob)
    dirs = _dirs16(rays_mod)
    eps, reach = EPS, REACH
    if case == "reach_inf":
        reach = INF
    elif case == "empty_interval":
        eps, reach = 1e-3, 1e-4
    else:
        s = np.float32(2.0 ** -20 if case == "tiny_dirs" else 2.0 ** 20)
        dirs = dirs * s
        eps, reach = float(np.float32(EPS) / s), float(np.float32(REACH) / s)
    scn = qr.Scene(blob, ray_queries=True)
    try:
        hits = _check_view_fans(scn, oracle, rays_mod, helper, blob, case, [view], 64, 64, dirs, eps, reach)
        if case == "empty_interval":
            for flip in (False, True):
                bits, traced = _open_bits(oracle, rays_mod, blob, hits, dirs, eps, reach, flip)
                assert traced.any() and (bits == traced).all()
        if case in ("tiny_dirs", "huge_dirs"):
            # the same distances: the same answers as the unit table
            a = _truth(oracle, rays_mod, blob, hits, dirs, eps, reach, True)
            b = _truth(oracle, rays_mod, blob, hits, _dirs16(rays_mod), EPS, REACH, True)
            print(f"{case}: {int((a[0] != b[0]).sum())} of {len(a[0])} counts differ from the unit table's")
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_sources_agree(qr, rays_mod):
    """hit_occlusion(view_hits(v)) == view_occlusion(v); occlusion(rays) == hit_occlusion(hits(rays)); open is the popcount of
    the mask; a call without mask gives the same open"""
    import torch
    blob = load_blob("demo02_160")
    views = [rays_mod.view_of(blob)] + [rays_mod.view_of(c) for c in _rayq.random_cameras(blob, seed=5, n=2)]
    dirs = rays_mod.sphere_dirs(40)
    scn = qr.Scene(blob, ray_queries=True)
    try:
        v_dev, d_dev = _cuda(scn, np.stack(views)), _cuda(scn, dirs)
        rays = _cuda(scn, rays_mod.camera_rays(blob))
        for flip in (False, True):
            o_v, m_v = scn.view_occlusion(v_dev, d_dev, 67, 45, eps=EPS, reach=REACH, flip=flip, mask=True)
            o_h, m_h = scn.hit_occlusion(scn.view_hits(v_dev, 67, 45), d_dev, EPS, REACH, flip=flip, mask=True)
            assert tuple(o_h.shape) == (3, 45, 67) and tuple(m_h.shape) == (2, 3, 45, 67)
            assert torch.equal(o_v, o_h) and torch.equal(m_v, m_h), f"view source and record source disagree (flip={flip})"
            assert torch.equal(scn.view_occlusion(v_dev, d_dev, 67, 45, eps=EPS, reach=REACH, flip=flip), o_v)
            assert torch.equal(scn.hit_occlusion(scn.view_hits(v_dev, 67, 45), d_dev, EPS, REACH, flip=flip), o_v)
            bits = rays_mod.fan_bits(m_v, 40)
            assert tuple(bits.shape) == (3, 45, 67, 40)
            pop = bits.sum(dim=-1).to(torch.int32)
            assert torch.equal(torch.where(o_v >= 0, o_v, torch.zeros_like(o_v)), pop)
            assert (o_v >= 0).any().item() and (pop > 0).any().item()
            for coherent in (False, True):
                o_r, m_r = scn.occlusion(rays, d_dev, EPS, REACH, flip=flip, mask=True, coherent=coherent)
                o_q, m_q = scn.hit_occlusion(scn.hits(rays), d_dev, EPS, REACH, flip=flip, mask=True)
                assert torch.equal(o_r, o_q) and torch.equal(m_r, m_q), f"ray source and record source disagree (flip={flip})"
                assert torch.equal(scn.occlusion(rays, d_dev, EPS, REACH, flip=flip, coherent=coherent), o_r)
            # [K, 4] tables: the pad column is ignored
            d4 = torch.cat([d_dev, torch.full((40, 1), float("nan"), device=d_dev.device)], dim=1).contiguous()
            assert torch.equal(scn.occlusion(rays, d4, EPS, REACH, flip=flip), o_r)
        _sync()
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_refusals(qr, rays_mod):
    import torch
    blob = load_blob("demo01_160")
    L = qr.lib()
    dev = "cuda:0"
    ARG, UNSUP = -1, -3
    nan = float("nan")
    rays = torch.from_numpy(rays_mod.camera_rays(blob)[:128]).to(dev)
    hits = torch.zeros((128, 12), dtype=torch.float32, device=dev)
    w, h = 67, 45
    vt = torch.from_numpy(np.stack([rays_mod.view_of(blob)] * 2)).to(dev)
    dirs = torch.zeros((1024, 4), dtype=torch.float32, device=dev)
    dirs[:, 2] = 1.0
    opn = torch.zeros((2 * h * w,), dtype=torch.int32, device=dev)
    msk = torch.zeros((32 * 2 * h * w,), dtype=torch.int32, device=dev)
    vp = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)

    def f_rays(s, r=vp(rays), n=64, d=vp(dirs), k=16, eps=EPS, reach=REACH, o=vp(opn), m=vp(msk), flags=0):
        return L.qr_fan_rays_async(s, r, n, d, k, eps, reach, o, m, flags, None)

    def f_hits(s, r=vp(hits), n=64, d=vp(dirs), k=16, eps=EPS, reach=REACH, o=vp(opn), m=vp(msk), flags=0):
        return L.qr_fan_hits_async(s, r, n, d, k, eps, reach, o, m, flags, None)

    def f_views(s, v=vp(vt), n=2, w=w, h=h, d=vp(dirs), k=16, eps=EPS, reach=REACH, o=vp(opn), m=vp(msk), flags=0):
        return L.qr_fan_views_async(s, v, n, w, h, d, k, eps, reach, o, m, flags, None)

    plain = qr.Scene(blob)
    for f in (f_rays, f_hits, f_views):
        assert f(plain._h) == UNSUP
    with pytest.raises(qr.QrError, match="QR_UPLOAD_RAY_QUERIES"):
        plain.occlusion(rays, dirs, EPS)
    plain.close()

    scn = qr.Scene(blob, ray_queries=True)
    for f in (f_rays, f_hits, f_views):
        assert f(None) == ARG
        assert f(scn._h, d=None) == ARG and f(scn._h, o=None) == ARG
        assert f(scn._h, d=vp(dirs, 4)) == ARG and f(scn._h, d=vp(dirs, 8)) == ARG            # misaligned
        assert f(scn._h, o=vp(opn, 2)) == ARG and f(scn._h, m=vp(msk, 1)) == ARG
        assert f(scn._h, k=0) == ARG and f(scn._h, k=-3) == ARG and f(scn._h, k=1025) == ARG
        assert f(scn._h, eps=nan) == ARG and f(scn._h, reach=nan) == ARG
        assert f(scn._h, flags=4) == ARG and f(scn._h, flags=0x80000000) == ARG
        assert f(scn._h, n=0) == 0 and f(scn._h, None, 0, o=None, m=None, d=None) == 0
        assert f(scn._h, n=-1) == ARG
        assert f(scn._h) == 0 and f(scn._h, m=None) == 0 and f(scn._h, flags=2) == 0            # QR_FAN_FLIP
        assert f(scn._h, k=1024, n=1) == 0 and f(scn._h, eps=-1.0, reach=INF) == 0
    for f in (f_rays, f_hits):
        assert f(scn._h, None) == ARG and f(scn._h, vp(rays, 4)) == ARG and f(scn._h, n=1 << 31) == ARG
    assert f_rays(scn._h, flags=1) == 0 and f_rays(scn._h, flags=3) == 0                        # QR_TRACE_COHERENT
    assert f_hits(scn._h, flags=1) == ARG and f_views(scn._h, flags=1) == ARG
    # views: the limits of qr_hit_views_async
    assert f_views(scn._h, v=None) == ARG and f_views(scn._h, v=vp(vt, 8)) == ARG
    assert f_views(scn._h, w=0) == ARG and f_views(scn._h, h=0) == ARG and f_views(scn._h, w=16385) == ARG
    assert f_views(scn._h, n=65536) == ARG and f_views(scn._h, n=65535, w=16384, h=16384) == ARG
    _sync()
    # the Python layer
    for bad in (dirs.double(), dirs[:, :2], dirs.cpu(), dirs[:0], torch.zeros((1025, 3), device=dev), dirs.cpu().numpy()):
        with pytest.raises(qr.QrError, match="dirs must"):
            scn.occlusion(rays, bad, EPS)
    with pytest.raises(qr.QrError, match="eps"):
        scn.view_occlusion(vt, dirs[:4], w, h)
    with pytest.raises(qr.QrError, match="eps"):
        scn.occlusion(rays, dirs[:4], nan)
    with pytest.raises(qr.QrError, match="rays must be"):
        scn.occlusion(rays.cpu(), dirs[:4], EPS)
    with pytest.raises(qr.QrError, match="views must be"):
        scn.view_occlusion(vt.cpu(), dirs[:4], w, h, eps=EPS)
    for bad in (hits.double(), hits[:, :11].contiguous(), hits.cpu(), hits[:, ::2], hits.reshape(-1)):
        with pytest.raises(qr.QrError, match="hits must be"):
            scn.hit_occlusion(bad, dirs[:4], EPS)
    e, em = scn.occlusion(rays[:0], dirs[:40], EPS, mask=True)
    assert tuple(e.shape) == (0,) and tuple(em.shape) == (2, 0) and e.dtype == torch.int32
    assert tuple(scn.view_occlusion(vt, dirs[:4], eps=EPS).shape) == (2, scn.height, scn.width)
    # records with id < 0 (all-zero records carry id 0: hits): -1 and an empty mask
    miss = hits.clone()
    miss.view(torch.int32)[:, 7] = -1
    o, m = scn.hit_occlusion(miss, dirs[:4], EPS, mask=True)
    _sync()
    assert (o == -1).all().item() and (m == 0).all().item()
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
    name = "synth_small"
    blob = RS.scene_blob(name)
    dirs = rays_mod.sphere_dirs(33)
    scn = _rs_scene(qr, name)
    views = [rays_mod.view_of(blob)] + [rays_mod.view_of(c) for c in _rayq.random_cameras(blob, seed=11, n=2)]
    _check_view_fans(scn, qr_oracle, rays_mod, helper, blob, f"guard {name}", views, 67, 45, dirs)
    rays = RS.mixed(blob, name, qr_oracle)
    hits = helper(blob, rays)
    for flip in (False, True):
        want = _truth(qr_oracle, rays_mod, blob, hits, dirs, EPS, REACH, flip)
        for coherent in (False, True):
            opn, msk = _occlusion(scn, rays, dirs, flip=flip, coherent=coherent)
            _same(f"guard {name} mixed flip={flip} coherent={coherent}", opn, msk, *want)
        opn, msk = scn.hit_occlusion(_cuda(scn, hits), _cuda(scn, dirs), EPS, REACH, flip=flip, mask=True)
        _sync()
        _same(f"guard {name} records flip={flip}", opn, msk, *want)
    scn.close()
    print(f"{name} guard_ok 1", flush=True)
    return 0


@pytest.mark.gpu
def test_gpu_guarded_build_gives_the_same_fans():
    assert os.path.exists(GUARD_LIB), "libqrhip_guard.so is missing: build() makes it (make -C quadray-engine_amd/csrc guard)"
    env = dict(os.environ, QR_LIB=GUARD_LIB)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-child"], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.count("guard_ok 1") == 1 and "QR_GUARD" not in out.stderr, out.stdout + out.stderr[-3000:]


if __name__ == "__main__":
    sys.exit(_guard_child() if "--guard-child" in sys.argv else 2)
