"""Framed fans (include/qrhip.h qr_fan_*_framed_async / qr_gather_*_framed_async; frame=True, spin= on Scene.occlusion, view_occlusion,
hit_occlusion, gather, view_gather, hit_gather): the direction table in every surface point's own frame, turned about the normal by
a per-element spin.

The truth is the composition the two fan test files use, with the framed rays: the oracle's hit records, rays.fan_rays(frame=True)
(pinned below, with rays.fan_frame and rays.gather_fold(frame=True), against scalar loops of single np.float32 operations), then
the oracle's occlusion query or shade() on the traced rays, then counts, mask words or the fold.  The GPU must give every word bit
for bit.  Sums that are NaN on both sides are compared by NaN-ness, not payload, as tests/test_gather_fans.py does.

Orthonormality bound: |u.v|, |u.n|, |v.n|, ||u| - 1| and ||v| - 1| in float64 are at most 1e-6 for unit normals and unit spins --
measured on the CPU over 2 000 000 random unit normals plus the axes the worst is 1.9e-7; the bound is about five times that.
"""
import ctypes
import inspect
import os
import subprocess
import sys
import types
import zlib

import numpy as np
import pytest

import _rayq
import _rayset as RS
import test_gather_fans as GF
import test_occlusion_fans as OF
from conftest import ROOT, load_blob
from test_hit_records import GUARD_LIB, _cuda, _fields, _helper, _ray_sets, _rays_mod, _rs_scene
from test_ray_query import _blob

INF = float("inf")
EPS, REACH = 1e-3, 2.0
F = np.float32
FLT_MAX = np.finfo(np.float32).max
COMBOS = [(False, False), (False, True), (True, False), (True, True)]      # (flip, cosine)
VIEW_SIZES = [(64, 64), (67, 45), (9, 130)]
K_VALUES = [1, 2, 33, 65]
SYMBOLS = ["qr_fan_rays_framed_async", "qr_fan_views_framed_async", "qr_fan_hits_framed_async",
           "qr_gather_rays_framed_async", "qr_gather_views_framed_async", "qr_gather_hits_framed_async"]
METHODS = ["occlusion", "view_occlusion", "hit_occlusion", "gather", "view_gather", "hit_gather"]


@pytest.fixture(scope="module")
def rays_mod():
    return _rays_mod()


@pytest.fixture(scope="module")
def helper():
    return _helper()


def _sync():
    import torch
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- the truth

def _table(rays_mod, k=16):
    """sphere_dirs(k) -- rows above and below the local horizon -- with weights that differ from row to row, some negative"""
    return GF._table(rays_mod, k)


def _framed(rays_mod, hits, dirs, eps, reach, flip, spin):
    return rays_mod.fan_rays(hits, np.ascontiguousarray(dirs, dtype=np.float32), F(eps), F(reach), flip, frame=True, spin=spin)


def _occ_truth(oracle, rays_mod, blob, hits, dirs, eps, reach, flip, spin):
    """(open int32 [N], mask uint32 [planes, N], open bits bool [N, K]) of the framed occlusion fan"""
    rays, traced = _framed(rays_mod, hits, dirs, eps, reach, flip, spin)
    n, k = traced.shape
    occ = np.zeros(n * k, dtype=bool)
    idx = np.nonzero(traced.reshape(-1))[0]
    if len(idx):
        occ[idx] = oracle.trace_rays(blob, rays.reshape(-1, 8)[idx], "occluded", threads=16)
    bits = traced & ~occ.reshape(n, k)
    return OF._pack(bits, _fields(hits)[3]) + (bits,)


def _colours(oracle, rays_mod, blob, hits, dirs, eps, reach, flip, spin, depth=None):
    """float32 [N, K, 3]: the oracle's shade() of every traced framed fan ray; zeros elsewhere"""
    rays, traced = _framed(rays_mod, hits, dirs, eps, reach, flip, spin)
    n, k = traced.shape
    col = np.zeros((n * k, 3), dtype=np.float32)
    idx = np.nonzero(traced.reshape(-1))[0]
    if len(idx):
        col[idx] = oracle.trace_rays(blob, rays.reshape(-1, 8)[idx], "shade", depth=depth, threads=16)[0]
    return col.reshape(n, k, 3)


def _fold(rays_mod, hits, dirs, col, flip, cosine, spin, start=None):
    return rays_mod.gather_fold(hits, dirs, col, flip, cosine, start=start, frame=True, spin=spin)


def _flat(spin):
    return None if spin is None else np.ascontiguousarray(spin.reshape(-1, 2))


def _dev(scn, spin):
    return None if spin is None else _cuda(scn, spin)


# ------------------------------------------------------------------------------------------------------------------- CPU

def test_symbols_keywords_and_header(qr):
    L = ctypes.CDLL(qr.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "qrhip.h")).read()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in qr.ABI_SYMBOLS and f"int {sym}(" in hdr
    for text in ("const float *spin_dev", "a  = -1 / (s + nz)", "dot = z", "|w| <= FLT_MAX", "8-byte aligned", "Duff et al. 2017"):
        assert text in hdr, text
    for fn in METHODS:
        p = inspect.signature(getattr(qr.Scene, fn)).parameters
        assert p["frame"].default is False and p["spin"].default is None, fn


def test_framed_kernels_in_resource_check():
    """the build's register check knows the ten framed instances and holds each to its unframed twin's budget"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_kernel_resources", os.path.join(ROOT, "tools", "check_kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    fan = sorted(f for f in m.LIMITS if "qr_fan_framed_kernel" in f)
    gat = sorted(f for f in m.LIMITS if "qr_gather_framed_kernel" in f)
    assert len(fan) == 5 and len(gat) == 5
    for f in fan:
        assert m.LIMITS[f] == m.LIMITS[f.replace("20qr_fan_framed_kernel", "13qr_fan_kernel")], f
    for f in gat:
        assert m.LIMITS[f] == m.LIMITS[f.replace("23qr_gather_framed_kernel", "16qr_gather_kernel")], f


def _ok(w):
    return bool(np.abs(w) <= FLT_MAX)          # a NaN fails the comparison


def _frame_scalar(n, spin):
    """the stated operations, one np.float32 at a time: (u, v, valid)"""
    nx, ny, nz = (F(x) for x in n)
    c, sn = (F(1), F(0)) if spin is None else (F(spin[0]), F(spin[1]))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = F(-1) if bool(nz < F(0)) else F(1)
        a = F(F(-1) / F(s + nz))
        b = F(F(nx * ny) * a)
        sx = F(s * nx)
        t = (F(F(1) + F(F(sx * nx) * a)), F(s * b), F(-sx))
        bt = (b, F(s + F(F(ny * ny) * a)), F(-ny))
        u = [F(F(t[i] * c) + F(bt[i] * sn)) for i in range(3)]
        v = [F(F(bt[i] * c) - F(t[i] * sn)) for i in range(3)]
    return u, v, all(_ok(w) for w in (nx, ny, nz, *u, *v))


def _rays_scalar(h, d, eps, reach, flip, spin):
    """framed fan_rays, one np.float32 at a time"""
    n, k = len(h), len(d)
    rays = np.zeros((n, k, 8), dtype=np.float32)
    traced = np.zeros((n, k), dtype=bool)
    ids = h.view(np.int32)[:, 7]
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(n):
            nrm = [F(x) for x in h[a, 4:7]]
            u, v, valid = _frame_scalar(nrm, None if spin is None else spin[a])
            for b in range(k):
                x, y, z = (F(q) for q in d[b, 0:3])
                if flip:
                    if bool(z < F(0)):
                        x, y, z = F(-x), F(-y), F(-z)
                    rule = True
                else:
                    rule = bool(F(0) < z)
                dd = [F(F(F(u[i] * x) + F(v[i] * y)) + F(nrm[i] * z)) for i in range(3)]
                traced[a, b] = rule and valid and ids[a] >= 0
                rays[a, b] = (h[a, 0], h[a, 1], h[a, 2], F(eps), dd[0], dd[1], dd[2], F(reach))
    return rays, traced


def _fold_scalar(h, d, col, flip, cosine, spin, start=None):
    n, k = len(h), len(d)
    ids = h.view(np.int32)[:, 7]
    acc = np.zeros((n, 4), dtype=np.float32) if start is None else start[0].copy()
    cnt = np.zeros(n, dtype=np.int32) if start is None else start[1].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(n):
            if ids[a] < 0:
                acc[a], cnt[a] = 0, -1
                continue
            if not _frame_scalar(h[a, 4:7], None if spin is None else spin[a])[2]:
                acc[a], cnt[a] = 0, 0
                continue
            for b in range(k):
                z = F(d[b, 2])
                if not flip and not bool(F(0) < z):
                    continue
                wgt = F(d[b, 3]) if d.shape[1] == 4 else F(1)
                if cosine:
                    wgt = F(wgt * (F(-z) if (flip and bool(z < F(0))) else z))
                for ch in range(3):
                    acc[a, ch] = F(acc[a, ch] + F(F(col[a, b, ch]) * wgt))
                acc[a, 3] = F(acc[a, 3] + wgt)
                cnt[a] += 1
    return acc, cnt


NORMALS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0, 0, -0.0), (6e-4, 3e-4, -1),
           (0.6, np.nan, 0.8), (np.inf, 0, 1), (1e30, 1e30, 0), (0.36, 0.48, 0.8)]
SPINS = [(1, 0), (0, 1), (0.3, -2.0), (np.nan, 1), (np.sqrt(0.5), -np.sqrt(0.5))]


def _records():
    """(records [13, 12], table [10, 4], two spin planes [13, 2]): NORMALS on made-up points, record 12 a miss; rows whose z is
    exactly 0, -0.0, negative, NaN; every spin of SPINS on every kind of normal between the two planes"""
    h = np.zeros((len(NORMALS) + 1, 12), dtype=np.float32)
    i = h.view(np.int32)
    h[:, 0:3] = np.arange(3 * len(h)).reshape(-1, 3) * 0.25
    h[:len(NORMALS), 4:7] = NORMALS
    h[-1, 4:7] = (0, 0, 1)
    i[:, 7] = np.arange(len(h))
    i[-1, 7] = -1
    d = np.array([(0, 0, 1, 0.5), (1, 0, 0, 2), (0.6, 0, -0.0, 1), (0, 0.8, -0.6, -1.5), (0.3, -0.2, 0.1, 0.7), (0, 1, np.nan, 1),
                  (-0.48, 0.6, 0.64, 3), (1e-20, 1e20, 3, 0.25), (0, 0, -1, 1), (0.6, 0.8, 0.0, 1.25)], dtype=np.float32)
    s1 = np.array([SPINS[j % len(SPINS)] for j in range(len(h))], dtype=np.float32)
    s2 = np.array([SPINS[(j + 2) % len(SPINS)] for j in range(len(h))], dtype=np.float32)
    return h, d, s1, s2


def _bits_or_nan(where, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, f"{where}: {got.dtype} {got.shape}"
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), f"{where}: {int(bad.sum())} words differ; first at {np.argwhere(bad)[0].tolist()}: {got[bad][0]!r} != {want[bad][0]!r}"


def test_fan_frame_pinned(rays_mod):
    import torch
    h, _, s1, s2 = _records()
    nrm = np.ascontiguousarray(h[:, 4:7])
    for label, spin in (("none", None), ("plane 1", s1), ("plane 2", s2)):
        want = [_frame_scalar(nrm[a], None if spin is None else spin[a]) for a in range(len(nrm))]
        wu, wv = np.array([w[0] for w in want], dtype=np.float32), np.array([w[1] for w in want], dtype=np.float32)
        wok = np.array([w[2] for w in want])
        if spin is None:
            # what the cases are there for
            assert wok[:8].all() and wok[11] and not wok[8:11].any(), wok.tolist()
            assert wu[4].tolist() == [1, 0, 0] and wv[4].tolist() == [0, 1, 0]                      # +z: the identity
            assert wu[5].tolist() == [1, 0, 0] and wv[5].tolist() == [0, -1, 0]                     # -z: s = -1, a = 1/2
            assert wu[6].tolist() == [1, 0, 0] and wv[6].tolist() == [0, 1, 0], "-0.0 gives s = +1"
            assert np.isinf(wu[10]).any() or np.isnan(wu[10]).any(), "the 1e30 normal's frame overflows"
        else:
            assert not wok[[j for j in range(len(nrm)) if np.isnan(spin[j]).any()]].any(), "a NaN spin gives an invalid frame"
        for conv in (lambda a: a, torch.from_numpy):
            u, v, ok = rays_mod.fan_frame(conv(nrm.copy()), None if spin is None else conv(spin.copy()))
            assert np.asarray(ok).dtype == bool and (np.asarray(ok) == wok).all(), label
            _bits_or_nan(f"u {label}", u, wu)
            _bits_or_nan(f"v {label}", v, wv)
    # spin (1, 0) equals no spin, bit for bit; other leading shapes
    ones = np.tile(np.array([[1, 0]], dtype=np.float32), (len(nrm), 1))
    a, b = rays_mod.fan_frame(nrm), rays_mod.fan_frame(nrm, ones)
    _bits_or_nan("spin (1, 0) u", b[0], a[0]); _bits_or_nan("spin (1, 0) v", b[1], a[1])
    assert (a[2] == b[2]).all()
    u2, v2, ok2 = rays_mod.fan_frame(nrm[:12].reshape(3, 4, 3), s1[:12].reshape(3, 4, 2))
    assert u2.shape == (3, 4, 3) and ok2.shape == (3, 4)
    _bits_or_nan("reshaped", u2.reshape(-1, 3), rays_mod.fan_frame(nrm[:12], s1[:12])[0])
    for bad in ((nrm.astype(np.float64), None), (nrm[:, :2], None), (nrm, s1[:5]), (nrm, s1.astype(np.float64))):
        with pytest.raises(ValueError):
            rays_mod.fan_frame(*bad)


@pytest.mark.parametrize("flip", [False, True])
def test_framed_fan_rays_pinned(rays_mod, flip):
    import torch
    h, d, s1, s2 = _records()
    for label, spin in (("none", None), ("plane 1", s1), ("plane 2", s2)):
        want_r, want_t = _rays_scalar(h, d, 1e-3, INF, flip, spin)
        assert not want_t[12].any() and want_t.any()
        if spin is None:
            assert not want_t[8:11].any(), "invalid frames trace nothing"
            if flip:
                assert want_t[:8].all() and want_t[11].all(), "a valid frame traces every row under flip, the NaN row too"
                assert want_r[4, 3, 4:7].tolist() == [-0.0, pytest.approx(-0.8), pytest.approx(0.6)]      # mirrored
                assert want_r[4, 2, 4] == F(0.6), "a -0.0 row is not mirrored"
            else:
                assert (want_t[4] == [True, False, False, False, True, False, True, True, False, False]).all(), want_t[4].tolist()
            # normal (0, 0, 1), no spin: d is the table row for finite rows
            fin = np.isfinite(d[:, 0:3]).all(axis=1) & ((d[:, 2] >= 0) | (not flip))
            assert (want_r[4, fin, 4:7] == d[fin, 0:3]).all()
        for d_in in (d, d[:, 0:3].copy()):
            for conv in (lambda a: a, torch.from_numpy):
                r, t = rays_mod.fan_rays(conv(h.copy()), conv(d_in.copy()), 1e-3, INF, flip, frame=True,
                                         spin=None if spin is None else conv(spin.copy()))
                r, t = np.asarray(r), np.asarray(t)
                assert r.shape == (13, 10, 8) and t.dtype == bool and (t == want_t).all(), label
                _bits_or_nan(f"framed fan_rays flip={flip} {label}", r, want_r)
    with pytest.raises(ValueError):
        rays_mod.fan_rays(h, d, 1e-3, spin=s1)                                 # spin without frame
    with pytest.raises(ValueError):
        rays_mod.fan_rays(h, d, 1e-3, frame=True, spin=s1[:4])
    assert "dot = z" in rays_mod.fan_rays.__doc__


@pytest.mark.parametrize("flip,cosine", COMBOS)
def test_framed_gather_fold_pinned(rays_mod, flip, cosine):
    h, d, s1, _ = _records()
    col = np.random.default_rng(5).uniform(0, 3, (len(h), len(d), 3)).astype(np.float32)
    col[1, 2] = (0.0, -0.0, 1e30)
    for spin in (None, s1):
        want = _fold_scalar(h, d, col, flip, cosine, spin)
        assert want[1][12] == -1 and (want[1][8:11] == 0).all() and (want[0][[8, 9, 10, 12]].view(np.uint32) == 0).all()
        valid = [j for j in range(12) if _frame_scalar(h[j, 4:7], None if spin is None else spin[j])[2]]
        assert (want[1][valid] == (10 if flip else 4)).all(), want[1].tolist()
        assert np.isnan(want[0][valid]).any(axis=None) == (flip and cosine), "the NaN row is traced under flip only; its z is the cosine"
        got = rays_mod.gather_fold(h.copy(), d.copy(), col.copy(), flip, cosine, frame=True, spin=spin)
        GF._same(f"framed fold flip={flip} cosine={cosine}", got[0], got[1], *want, nan_ok=True)
        d3 = d[:, 0:3].copy()
        got = rays_mod.gather_fold(h, d3, col, flip, cosine, frame=True, spin=spin)
        GF._same("framed fold, three columns", got[0], got[1], *_fold_scalar(h, d3, col, flip, cosine, spin), nan_ok=True)
        # a table cut into chunks and folded with start= equals one fold; invalid frames and misses ignore the start
        one = rays_mod.gather_fold(h, d, col, flip, cosine, frame=True, spin=spin)
        for a in (1, 4, 9):
            first = rays_mod.gather_fold(h, d[:a], col[:, :a], flip, cosine, frame=True, spin=spin)
            both = rays_mod.gather_fold(h, d[a:], col[:, a:], flip, cosine, start=first, frame=True, spin=spin)
            GF._same(f"chunks {a}", both[0], both[1], *one, nan_ok=True)
        junk = (np.full((13, 4), 5.0, np.float32), np.full(13, 9, np.int32))
        g, c = rays_mod.gather_fold(h, d[:1], col[:, :1], flip, cosine, start=junk, frame=True, spin=spin)
        assert c[12] == -1 and (c[8:11] == 0).all() and (g[[8, 9, 10, 12]].view(np.uint32) == 0).all()
    with pytest.raises(ValueError):
        rays_mod.gather_fold(h, d, col, flip, cosine, spin=s1)


def test_identities(rays_mod):
    """normal (0, 0, 1) without spin: the framed rays, traced rule and weights are the unframed ones for finite rows; spin (1, 0)
    equals no spin: all bit for bit"""
    rng = np.random.default_rng(3)
    h = np.zeros((5, 12), dtype=np.float32)
    h[:, 0:3] = rng.uniform(-2, 2, (5, 3))
    h[:, 4:7] = (0, 0, 1)
    h.view(np.int32)[:, 7] = [3, 0, -1, 8, 1]
    d = np.concatenate([rays_mod.sphere_dirs(24), rng.uniform(-2, 2, (24, 1)).astype(np.float32)], axis=1)
    d[5, 2], d[6, 2] = 0.0, -0.0
    col = rng.uniform(0, 2, (5, 24, 3)).astype(np.float32)
    ones = np.tile(np.array([[1, 0]], dtype=np.float32), (5, 1))
    for flip in (False, True):
        r0, t0 = rays_mod.fan_rays(h, d, 1e-3, 2.0, flip)
        r1, t1 = rays_mod.fan_rays(h, d, 1e-3, 2.0, flip, frame=True)
        r2, t2 = rays_mod.fan_rays(h, d, 1e-3, 2.0, flip, frame=True, spin=ones)
        assert (t0 == t1).all() and (t1 == t2).all() and t1.any()
        # x * 1 + y * 0 + ... may turn a -0.0 component into +0.0: values are equal, and bits wherever the component is not zero
        assert (r0 == r1).all() and (r0.view(np.uint32) == r1.view(np.uint32))[r0 != 0].all()
        assert (r1.view(np.uint32) == r2.view(np.uint32)).all()
        for cosine in (False, True):
            a = rays_mod.gather_fold(h, d, col, flip, cosine)
            b = rays_mod.gather_fold(h, d, col, flip, cosine, frame=True)
            c = rays_mod.gather_fold(h, d, col, flip, cosine, frame=True, spin=ones)
            GF._same(f"identity flip={flip} cosine={cosine}", b[0], b[1], *a)
            GF._same(f"unit spin flip={flip} cosine={cosine}", c[0], c[1], *b)


def test_orthonormal(rays_mod):
    """(u, v, n) for seeded unit normals and unit spins, in float64: the module docstring's bound"""
    rng = np.random.default_rng(11)
    n = rng.normal(size=(200000, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n = np.concatenate([n, np.eye(3), -np.eye(3)]).astype(np.float32)
    spin = rays_mod.spins(len(n), 7)
    for sp in (None, spin):
        u, v, ok = rays_mod.fan_frame(n, sp)
        assert ok.all()
        u, v, m = u.astype(np.float64), v.astype(np.float64), n.astype(np.float64)
        dot = lambda a, b: np.abs((a * b).sum(axis=1)).max()
        worst = max(dot(u, v), dot(u, m), dot(v, m), np.abs(np.linalg.norm(u, axis=1) - 1).max(), np.abs(np.linalg.norm(v, axis=1) - 1).max())
        print(f"orthonormality, spin {'yes' if sp is not None else 'no'}: worst {worst:.3g}")
        assert worst <= 1e-6
        assert (np.abs(np.cross(u, v) - m) <= 2e-6).all(), "right-handed: u x v = n"


def test_cosine_dirs_and_spins(rays_mod):
    for n in (1, 16, 64, 1000):
        d = rays_mod.cosine_dirs(n)
        assert d.dtype == np.float32 and d.shape == (n, 4)
        assert (d[:, 2] > 0).all()
        assert (np.abs(np.linalg.norm(d[:, 0:3].astype(np.float64), axis=1) - 1.0) <= 1e-6).all()
        assert abs(d[:, 3].astype(np.float64).sum() - 1.0) <= 1e-6 and (d[:, 3] == F(1.0 / n)).all()
    d = rays_mod.cosine_dirs(16)
    i = np.arange(16) + 0.5
    r, phi = np.sqrt(i / 16), i * np.pi * (3.0 - np.sqrt(5.0))
    assert (d[:, 0] == (r * np.cos(phi)).astype(np.float32)).all() and (d[:, 1] == (r * np.sin(phi)).astype(np.float32)).all()
    assert (d[:, 2] == np.sqrt(1.0 - r * r).astype(np.float32)).all()
    assert abs((d[:, 2].astype(np.float64)).mean() - 2.0 / 3.0) < 0.01, "the mean cosine of a cosine-distributed hemisphere is 2/3"
    with pytest.raises(ValueError):
        rays_mod.cosine_dirs(0)
    s = rays_mod.spins((3, 5), 42)
    assert s.dtype == np.float32 and s.shape == (3, 5, 2)
    a = np.random.default_rng(42).uniform(0, 2 * np.pi, (3, 5))
    assert (s[..., 0] == np.cos(a).astype(np.float32)).all() and (s[..., 1] == np.sin(a).astype(np.float32)).all()
    assert rays_mod.spins(7, 1).shape == (7, 2) and (rays_mod.spins(7, 1) != rays_mod.spins(7, 2)).any()


def test_python_refusals_without_a_gpu(qr):
    """what Scene refuses about `spin` before anything reaches the library: ValueError"""
    import torch
    me = types.SimpleNamespace(device=0)
    f = lambda *a: qr.Scene._spin_arg(me, *a)
    assert f(False, None, (8,)) is None and f(True, None, (8,)) is None
    ok = torch.zeros((8, 2), dtype=torch.float32)
    with pytest.raises(ValueError, match="frame=True"):
        f(False, ok, (8,))
    for bad in (ok, ok.double(), ok.numpy(), torch.zeros((8, 3)), torch.zeros((4, 2, 2))):        # a CPU tensor: another device
        with pytest.raises(ValueError, match="spin must be"):
            f(True, bad, (8,))


# ------------------------------------------------------------------------------------------------------------------- GPU

def _check_views(scn, oracle, rays_mod, helper, blob, where, views, w, h, dirs, seed, eps=EPS, reach=REACH, combos=COMBOS,
                 spins=(False, True), occlusion=True, depth=None):
    """view_occlusion (with and without mask) and view_gather of several views in one launch each, framed, without and with a
    spin plane, against the truth; returns the hit records"""
    import torch
    hits = np.concatenate([OF._view_truth(oracle, rays_mod, helper, blob, v, w, h) for v in views])
    v_dev, d_dev = _cuda(scn, np.stack(views)), _cuda(scn, dirs)
    for spun in spins:
        spin = rays_mod.spins((len(views), h, w), seed) if spun else None
        kw = dict(eps=eps, reach=reach, frame=True, spin=_dev(scn, spin))
        for flip in sorted({f for f, _ in combos}):
            tag = f"{where} {w}x{h} flip={flip} spin={spun}"
            if occlusion:
                opn, msk = scn.view_occlusion(v_dev, d_dev, w, h, flip=flip, mask=True, **kw)
                _sync()
                assert tuple(opn.shape) == (len(views), h, w) and tuple(msk.shape) == ((len(dirs) + 31) // 32, len(views), h, w)
                want = _occ_truth(oracle, rays_mod, blob, hits, dirs, eps, reach, flip, _flat(spin))
                OF._same(tag, opn, msk, want[0], want[1])
                assert torch.equal(scn.view_occlusion(v_dev, d_dev, w, h, flip=flip, **kw), opn), f"{tag}: without mask"
            col = _colours(oracle, rays_mod, blob, hits, dirs, eps, reach, flip, _flat(spin), depth)
            assert (col != 0).any(axis=2).sum() > 100, f"{tag}: the fan rays see too little light"
            for cosine in [c for f, c in combos if f == flip]:
                g, c = scn.view_gather(v_dev, d_dev, w, h, flip=flip, cosine=cosine, **kw)
                _sync()
                assert tuple(g.shape) == (len(views), h, w, 4) and tuple(c.shape) == (len(views), h, w)
                GF._same(f"{tag} cosine={cosine}", g, c, *_fold(rays_mod, hits, dirs, col, flip, cosine, _flat(spin)))
    return hits


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["demo01_160", "demo01_160_gf_aa4", "synth_small"])
def test_gpu_framed_views(qr, oracle, rays_mod, helper, name):
    """the snapshot's own camera and a seeded camera among the objects in ONE launch per size, sizes that are no multiple of a
    footprint, without and with FSAA (sample 0's point), without and with spin; flip x mask, flip x cosine"""
    blob = _blob(name)
    seed = zlib.crc32(name.encode())
    views = [rays_mod.view_of(blob)] + [rays_mod.view_of(c) for c in _rayq.random_cameras(blob, seed=seed, n=1)]
    scn = qr.Scene(blob, ray_queries=True)
    try:
        for (w, h) in VIEW_SIZES:
            _check_views(scn, oracle, rays_mod, helper, blob, name, views, w, h, _table(rays_mod), seed & 0xffff)
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_direction_counts_and_a_table_below_the_horizon(qr, oracle, rays_mod, helper):
    """K = 1, 2, 33 and 65 (mask-word boundaries) on one spun 64x64 view: the tables are prefixes of one table, so one oracle run
    over the longest gives every truth.  Then a table wholly below the local horizon: without flip 0 and a zero row on every
    hit, -1 on every miss (no walk: the whole wave skips every row)"""
    blob = load_blob("demo01_160")
    table = _table(rays_mod, 65)
    view, hits = GF._busy_view(oracle, rays_mod, helper, blob, 64, 64)
    hid = _fields(hits)[3]
    spin = rays_mod.spins((1, 64, 64), 9)
    scn = qr.Scene(blob, ray_queries=True)
    try:
        v_dev, s_dev = _cuda(scn, view[None]), _cuda(scn, spin)
        for flip in (False, True):
            bits = _occ_truth(oracle, rays_mod, blob, hits, table, EPS, REACH, flip, _flat(spin))[2]
            col = _colours(oracle, rays_mod, blob, hits, table, EPS, REACH, flip, _flat(spin))
            for k in K_VALUES:
                kw = dict(eps=EPS, reach=REACH, flip=flip, frame=True, spin=s_dev)
                opn, msk = scn.view_occlusion(v_dev, _cuda(scn, table[:k]), 64, 64, mask=True, **kw)
                g, c = scn.view_gather(v_dev, _cuda(scn, table[:k]), 64, 64, cosine=True, **kw)
                _sync()
                assert msk.shape[0] == (k + 31) // 32
                OF._same(f"K={k} flip={flip}", opn, msk, *OF._pack(bits[:, :k], hid))
                if k & 31:
                    assert (msk[-1].cpu().numpy().view(np.uint32) >> np.uint32(k & 31) == 0).all(), f"K={k}: bits past K are set"
                GF._same(f"K={k} flip={flip}", g, c, *_fold(rays_mod, hits, table[:k], col[:, :k], flip, True, _flat(spin)))
        below = table[table[:, 2] < 0][:20]
        assert len(below) == 20
        kw = dict(eps=EPS, reach=REACH, frame=True, spin=s_dev)
        opn, msk = scn.view_occlusion(v_dev, _cuda(scn, below), 64, 64, mask=True, **kw)
        g, c = scn.view_gather(v_dev, _cuda(scn, below), 64, 64, cosine=True, **kw)
        _sync()
        o, m = opn.cpu().numpy().reshape(-1), msk.cpu().numpy()
        gg, cc = g.cpu().numpy().reshape(-1, 4), c.cpu().numpy().reshape(-1)
        want = np.where(hid >= 0, 0, -1)
        assert (hid >= 0).any() and (hid < 0).any()
        assert (o == want).all() and (cc == want).all() and (m == 0).all() and (gg.view(np.uint32) == 0).all()
        # with flip the same table is traced in full
        c2 = scn.view_gather(v_dev, _cuda(scn, below), 64, 64, flip=True, **kw)[1].cpu().numpy().reshape(-1)
        assert (c2 == np.where(hid >= 0, 20, -1)).all()
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_cosine_table_traces_every_direction_and_spin_shows(qr, oracle, rays_mod, helper):
    """cosine_dirs(16) without flip: framed, every hit element traces all 16 (count 16; with an empty interval, reach < eps,
    everything traced is open: open 16), where the unframed call with the same table traces fewer.  Two different spin planes
    give different results; spin (1, 0) equals none, bit for bit; the framed call with a real reach matches the truth."""
    import torch
    blob = load_blob("demo02_160")             # a closed room: the hemisphere above every point sees lit walls
    dirs = rays_mod.cosine_dirs(16)
    view, hits = GF._busy_view(oracle, rays_mod, helper, blob, 64, 64)
    hit = _fields(hits)[3] >= 0
    scn = qr.Scene(blob, ray_queries=True)
    try:
        v_dev, d_dev = _cuda(scn, view[None]), _cuda(scn, dirs)
        flat = lambda t: t.cpu().numpy().reshape(-1)
        g_f, c_f = scn.view_gather(v_dev, d_dev, 64, 64, eps=EPS, reach=REACH, frame=True)
        g_u, c_u = scn.view_gather(v_dev, d_dev, 64, 64, eps=EPS, reach=REACH)
        o_f = scn.view_occlusion(v_dev, d_dev, 64, 64, eps=1e-3, reach=1e-4, frame=True)
        o_u = scn.view_occlusion(v_dev, d_dev, 64, 64, eps=1e-3, reach=1e-4)
        _sync()
        assert (flat(c_f)[hit] == 16).all() and (flat(c_f)[~hit] == -1).all()
        assert (flat(o_f)[hit] == 16).all() and (flat(o_f)[~hit] == -1).all()
        assert (flat(c_u)[hit] < 16).sum() > hit.sum() // 4 and (flat(o_u)[hit] < 16).sum() > hit.sum() // 4
        w = g_f.cpu().numpy().reshape(-1, 4)[hit, 3].astype(np.float64)
        assert (np.abs(w - 1.0) <= 16 * 2.0 ** -24).all(), "acc.w is the sum of sixteen 1/16: 1"
        col = _colours(oracle, rays_mod, blob, hits, dirs, EPS, REACH, False, None)
        assert (col != 0).any(axis=2).sum() > 1000, "the fan rays see too little light"
        GF._same("cosine table", g_f, c_f, *_fold(rays_mod, hits, dirs, col, False, False, None))
        # spins
        kw = dict(eps=EPS, reach=REACH, frame=True)
        sa, sb = _cuda(scn, rays_mod.spins((1, 64, 64), 1)), _cuda(scn, rays_mod.spins((1, 64, 64), 2))
        unit = torch.zeros((1, 64, 64, 2), device=v_dev.device); unit[..., 0] = 1.0
        ga, gb, g1 = (scn.view_gather(v_dev, d_dev, 64, 64, spin=s, **kw)[0] for s in (sa, sb, unit))
        oa, ob, o1 = (scn.view_occlusion(v_dev, d_dev, 64, 64, spin=s, mask=True, **kw) for s in (sa, sb, unit))
        o0 = scn.view_occlusion(v_dev, d_dev, 64, 64, mask=True, **kw)
        _sync()
        bits = lambda t: t.view(torch.int32)
        assert (bits(ga) != bits(gb)).any(dim=-1).sum().item() > hit.sum() // 4, "two spin planes give the same sums"
        assert (oa[1] != ob[1]).sum().item() > hit.sum() // 8, "two spin planes give the same masks"
        assert torch.equal(bits(g1), bits(g_f)), "spin (1, 0) differs from no spin"
        assert torch.equal(o1[0], o0[0]) and torch.equal(o1[1], o0[1])
    finally:
        scn.close()


def _ray_calls(scn, rays, dirs, spin, flip, cosine, coherent):
    kw = dict(flip=flip, coherent=coherent, frame=True, spin=_dev(scn, spin))
    opn, msk = scn.occlusion(_cuda(scn, rays), _cuda(scn, dirs), EPS, REACH, mask=True, **kw)
    g, c = scn.gather(_cuda(scn, rays), _cuda(scn, dirs), EPS, REACH, cosine=cosine, **kw)
    _sync()
    return opn, msk, g, c


@pytest.mark.gpu
def test_gpu_framed_ray_families(qr, oracle, rays_mod, helper):
    """camera rays and the adversarial families of tests/_rayset.py as the rays whose first hits carry the fans, without and with
    spin; QR_TRACE_COHERENT gives the same bits, with and without spin"""
    name = "synth_small"
    blob = RS.scene_blob(name)
    dirs = _table(rays_mod)
    scn = _rs_scene(qr, name)
    try:
        for label, rays in _ray_sets(blob, name, oracle, rays_mod):
            hits = helper(blob, rays)
            for spin in (None, rays_mod.spins(len(rays), 3)):
                for flip in (False, True):
                    want_o = _occ_truth(oracle, rays_mod, blob, hits, dirs, EPS, REACH, flip, spin)
                    col = _colours(oracle, rays_mod, blob, hits, dirs, EPS, REACH, flip, spin)
                    want_g = _fold(rays_mod, hits, dirs, col, flip, not flip, spin)
                    for coherent in (False, True):
                        opn, msk, g, c = _ray_calls(scn, rays, dirs, spin, flip, not flip, coherent)
                        tag = f"{name} {label} flip={flip} spin={spin is not None} coherent={coherent}"
                        OF._same(tag, opn, msk, want_o[0], want_o[1])
                        GF._same(tag, g, c, *want_g)
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_framed_rays_on_a_crowd_scene(qr, oracle, rays_mod, helper, tmp_path):
    """fans over a list with a uniform grid and four unbounded members (crowd_flat_dda), engine-authored surfaces of every kind"""
    name = "crowd_flat_dda"
    blob = RS.scene_blob(name)
    off, img = RS.query_image(qr, name, tmp_path)
    g = RS.dda_grid(off, img)
    assert g is not None
    dirs = _table(rays_mod)
    scn = _rs_scene(qr, name)
    try:
        rays = RS.mixed(blob, name, oracle, g, RS.reach_of(img))
        hits = helper(blob, rays)
        assert (_fields(hits)[3] >= 0).sum() > 100
        spin = rays_mod.spins(len(rays), 4)
        for flip in (False, True):
            want_o = _occ_truth(oracle, rays_mod, blob, hits, dirs, EPS, REACH, flip, spin)
            col = _colours(oracle, rays_mod, blob, hits, dirs, EPS, REACH, flip, spin)
            assert (col != 0).any()
            for coherent in (False, True):
                opn, msk, gg, c = _ray_calls(scn, rays, dirs, spin, flip, True, coherent)
                OF._same(f"{name} flip={flip} coherent={coherent}", opn, msk, want_o[0], want_o[1])
                GF._same(f"{name} flip={flip} coherent={coherent}", gg, c, *_fold(rays_mod, hits, dirs, col, flip, True, spin))
    finally:
        scn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_gpu_framed_ray_batch_sizes(qr, oracle, rays_mod, helper, n):
    """partial waves through the C ABI into sentinel-tailed outputs: nothing is written past the end of open, a mask plane,
    gather or count; a permuted batch (rays and spins) gives permuted rows"""
    import torch
    name = "synth_small"
    blob = RS.scene_blob(name)
    rays = RS.mixed(blob, name, oracle)[:n]
    assert len(rays) == n
    dirs = _table(rays_mod, 33)
    spin = rays_mod.spins(n, n)
    hits = helper(blob, rays)
    scn = _rs_scene(qr, name)
    try:
        want_o = _occ_truth(oracle, rays_mod, blob, hits, dirs, EPS, REACH, True, spin)
        want_g = _fold(rays_mod, hits, dirs, _colours(oracle, rays_mod, blob, hits, dirs, EPS, REACH, True, spin), True, True, spin)
        dev = f"cuda:{scn.device}"
        o = torch.full((n + 64,), 77, dtype=torch.int32, device=dev)
        m = torch.full((2 * n + 64,), 77, dtype=torch.int32, device=dev)
        go = torch.full((4 * n + 64,), 77.0, dtype=torch.float32, device=dev)
        co = torch.full((n + 64,), 77, dtype=torch.int32, device=dev)
        r_dev, d_dev, s_dev = _cuda(scn, rays), _cuda(scn, dirs), _cuda(scn, spin)
        vp = lambda x: ctypes.c_void_p(x.data_ptr())
        L = qr.lib()
        rc1 = L.qr_fan_rays_framed_async(scn._h, vp(r_dev), n, vp(d_dev), 33, vp(s_dev), EPS, REACH, vp(o), vp(m), qr.FAN_FLIP, None)
        rc2 = L.qr_gather_rays_framed_async(scn._h, vp(r_dev), n, vp(d_dev), 33, vp(s_dev), EPS, REACH, vp(go), vp(co),
                                            qr.FAN_FLIP | qr.GATHER_COSINE, None)
        _sync()
        assert rc1 == 0 and rc2 == 0
        assert (o[n:] == 77).all().item() and (m[2 * n:] == 77).all().item(), "written past the end of the batch"
        assert (go[4 * n:] == 77.0).all().item() and (co[n:] == 77).all().item(), "written past the end of the batch"
        OF._same(f"n={n} raw", o[:n], m[:2 * n].reshape(2, n), want_o[0], want_o[1])
        GF._same(f"n={n} raw", go[:4 * n].reshape(n, 4), co[:n], *want_g)
        perm = np.random.default_rng(n).permutation(n)
        opn, msk, g, c = _ray_calls(scn, rays[perm], dirs, spin[perm], True, True, False)
        OF._same(f"n={n} permuted", opn, msk, want_o[0][perm], want_o[1][:, perm])
        GF._same(f"n={n} permuted", g, c, want_g[0][perm], want_g[1][perm])
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_framed_records(qr, oracle, rays_mod, helper):
    """the CPU list's normals and spins on real surface points of a scene (more than one wave of them): invalid frames -- a NaN
    or Inf component, the 1e30 normal, a NaN spin -- give open 0 / count 0, zero mask bits and a zero row, a miss -1; the
    occlusion fan also gets rows with z = 0, -0.0 and NaN (a NaN direction walks, as in tests/test_occlusion_fans.py).  Records
    with normal (0, 0, 1) equal the unframed call on the same GPU."""
    import torch
    blob = load_blob("demo02_160")
    cam = rays_mod.camera_rays(blob)
    real = helper(blob, cam)
    on = np.nonzero(_fields(real)[3] >= 0)[0]
    h0, d_occ, s1, _ = _records()
    reps = 6
    h = np.tile(h0, (reps, 1))                                  # 78 records
    spin = np.tile(s1, (reps, 1))
    h[:, 0:3] = real[on[np.linspace(0, len(on) - 1, len(h)).astype(int)], 0:3]
    d_gat = _table(rays_mod)
    scn = qr.Scene(blob, ray_queries=True)
    try:
        for sp in (None, spin):
            ok = rays_mod.fan_frame(np.ascontiguousarray(h[:, 4:7]), sp)[2]
            bad = ~ok & (_fields(h)[3] >= 0)
            assert bad.sum() >= 3 * reps and ok.sum() >= 4 * reps
            for flip in (False, True):
                want = _occ_truth(oracle, rays_mod, blob, h, d_occ, EPS, REACH, flip, sp)
                opn, msk = scn.hit_occlusion(_cuda(scn, h), _cuda(scn, d_occ), EPS, REACH, flip=flip, mask=True, frame=True, spin=_dev(scn, sp))
                _sync()
                OF._same(f"records flip={flip} spin={sp is not None}", opn, msk, want[0], want[1])
                o, m = opn.cpu().numpy(), msk.cpu().numpy()
                assert (o[bad] == 0).all() and (m[:, bad] == 0).all() and (o[12::13] == -1).all()
                col = _colours(oracle, rays_mod, blob, h, d_gat, EPS, REACH, flip, sp)
                assert (col != 0).any()
                for cosine in (False, True):
                    g, c = scn.hit_gather(_cuda(scn, h), _cuda(scn, d_gat), EPS, REACH, flip=flip, cosine=cosine, frame=True, spin=_dev(scn, sp))
                    _sync()
                    GF._same(f"records flip={flip} cosine={cosine} spin={sp is not None}", g, c,
                             *_fold(rays_mod, h, d_gat, col, flip, cosine, sp), nan_ok=True)
                    gg, cc = g.cpu().numpy(), c.cpu().numpy()
                    assert (cc[bad] == 0).all() and (gg[bad].view(np.uint32) == 0).all() and (cc[12::13] == -1).all()
        # normal (0, 0, 1): the framed call is the unframed one (the weights are the table's z either way)
        up = h.copy()
        up[:, 4:7] = (0, 0, 1)
        u_dev, d_dev = _cuda(scn, up), _cuda(scn, d_gat)
        for flip, cosine in COMBOS:
            a = scn.hit_gather(u_dev, d_dev, EPS, REACH, flip=flip, cosine=cosine)
            b = scn.hit_gather(u_dev, d_dev, EPS, REACH, flip=flip, cosine=cosine, frame=True)
            oa = scn.hit_occlusion(u_dev, d_dev, EPS, REACH, flip=flip, mask=True)
            ob = scn.hit_occlusion(u_dev, d_dev, EPS, REACH, flip=flip, mask=True, frame=True)
            _sync()
            assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), f"+z gather {flip} {cosine}"
            assert torch.equal(oa[0], ob[0]) and torch.equal(oa[1], ob[1]) and (a[1] > 0).any().item(), f"+z occlusion {flip}"
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_sources_agree_and_resume(qr, oracle, rays_mod, helper):
    """the three sources against each other, spun: hit_*(view_hits(v)) == view_*(v), *(rays) == hit_*(hits(rays)) with and
    without `coherent`; then 16 = 5 + 11 = 16 x 1 resumed chunks against one call for every source, the one call against the
    truth"""
    import torch
    blob = load_blob("demo03_160")
    dirs = _table(rays_mod)
    w, h = 67, 45
    view, hits = GF._busy_view(oracle, rays_mod, helper, blob, w, h)
    spin = rays_mod.spins((1, h, w), 21)
    scn = qr.Scene(blob, ray_queries=True)
    try:
        v_dev, d_dev, s_dev = _cuda(scn, view[None]), _cuda(scn, dirs), _cuda(scn, spin)
        s_flat = s_dev.reshape(-1, 2)
        rays = _cuda(scn, rays_mod.view_rays(view, w, h, blob, sample=0))
        bits = lambda t: t.view(torch.int32)
        for flip in (False, True):
            kw = dict(flip=flip, frame=True)
            o_v = scn.view_occlusion(v_dev, d_dev, w, h, eps=EPS, reach=REACH, mask=True, spin=s_dev, **kw)
            o_h = scn.hit_occlusion(scn.view_hits(v_dev, w, h), d_dev, EPS, REACH, mask=True, spin=s_dev, **kw)
            assert torch.equal(o_v[0], o_h[0]) and torch.equal(o_v[1], o_h[1]), f"view and record source disagree flip={flip}"
            for coherent in (False, True):
                o_r = scn.occlusion(rays, d_dev, EPS, REACH, mask=True, coherent=coherent, spin=s_flat, **kw)
                assert torch.equal(o_r[0], o_v[0].reshape(-1)) and torch.equal(o_r[1], o_v[1].reshape(1, -1)), f"ray source flip={flip}"
        calls = {
            "views": lambda d, **kw: scn.view_gather(v_dev, d, w, h, eps=EPS, reach=REACH, frame=True, spin=s_dev, **kw),
            "rays": lambda d, **kw: scn.gather(rays, d, EPS, REACH, frame=True, spin=s_flat, **kw),
            "coherent rays": lambda d, **kw: scn.gather(rays, d, EPS, REACH, frame=True, spin=s_flat, coherent=True, **kw),
            "hits": lambda d, **kw: scn.hit_gather(_cuda(scn, hits), d, EPS, REACH, frame=True, spin=s_flat, **kw),
        }
        for flip, cosine in ((False, True), (True, False)):
            col = _colours(oracle, rays_mod, blob, hits, dirs, EPS, REACH, flip, _flat(spin))
            want = _fold(rays_mod, hits, dirs, col, flip, cosine, _flat(spin))
            for src, call in calls.items():
                one_g, one_c = call(d_dev, flip=flip, cosine=cosine)
                _sync()
                GF._same(f"{src} one call flip={flip}", one_g, one_c, *want)
                for cuts in ((0, 5, 16), tuple(range(17))):
                    g = torch.full_like(one_g, 123.0)
                    c = torch.full_like(one_c, 123)
                    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                        rg, rc = call(d_dev[a:b].contiguous(), flip=flip, cosine=cosine, out=g, count=c, resume=i > 0)
                        assert rg is g and rc is c
                    _sync()
                    GF._same(f"{src} resumed {len(cuts) - 1} chunks flip={flip}", g, c, *want)
    finally:
        scn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [0, None, 10])
def test_gpu_framed_depths(qr, oracle, rays_mod, helper, depth):
    """the framed fan rays are shaded at the scene's current depth: 0, the snapshot's own and 10, on the Gamma + Fresnel fixture"""
    blob = load_blob("demo02_160_gf_d5")
    view, _ = GF._busy_view(oracle, rays_mod, helper, blob, 64, 64)
    scn = qr.Scene(blob, ray_queries=True)
    try:
        if depth is not None:
            scn.set_depth(depth)
        _check_views(scn, oracle, rays_mod, helper, blob, f"depth {depth}", [view], 64, 64, _table(rays_mod), 31,
                     combos=[(False, True), (True, False)], spins=(True,), occlusion=False, depth=depth)
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_framed_refusals(qr, rays_mod):
    """every C-level refusal of the six framed entry points -- the matching call's, and a misaligned spin -- with sentinel-filled
    outputs untouched after all of them; then the Python layer's ValueErrors"""
    import torch
    blob = load_blob("demo01_160")
    L = qr.lib()
    dev = "cuda:0"
    ARG, UNSUP = -1, -3
    nan = float("nan")
    rays = torch.from_numpy(rays_mod.camera_rays(blob)[:128]).to(dev)
    hits = torch.zeros((128, 12), dtype=torch.float32, device=dev)
    hits[:, 6] = 1.0
    w, h = 67, 45
    vt = torch.from_numpy(np.stack([rays_mod.view_of(blob)] * 2)).to(dev)
    dirs = torch.zeros((1024, 4), dtype=torch.float32, device=dev)
    dirs[:, 2:4] = 1.0
    spin = torch.zeros((2 * h * w + 1, 2), dtype=torch.float32, device=dev)
    spin[:, 0] = 1.0
    opn = torch.full((2 * h * w,), 77, dtype=torch.int32, device=dev)
    msk = torch.full((32 * 2 * h * w,), 77, dtype=torch.int32, device=dev)
    gat = torch.full((2 * h * w, 4), 7.5, dtype=torch.float32, device=dev)
    cnt = torch.full((2 * h * w,), 77, dtype=torch.int32, device=dev)
    vp = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)

    def mk(fn, views, a, b):
        if views:
            return lambda s, v=vp(vt), n=2, w=w, h=h, d=vp(dirs), k=16, sp=vp(spin), eps=EPS, reach=REACH, a=a, b=b, flags=0: \
                fn(s, v, n, w, h, d, k, sp, eps, reach, a, b, flags, None)
        return lambda s, r, n=64, d=vp(dirs), k=16, sp=vp(spin), eps=EPS, reach=REACH, a=a, b=b, flags=0: \
            fn(s, r, n, d, k, sp, eps, reach, a, b, flags, None)

    fans = {"rays": mk(L.qr_fan_rays_framed_async, False, vp(opn), vp(msk)), "hits": mk(L.qr_fan_hits_framed_async, False, vp(opn), vp(msk)),
            "views": mk(L.qr_fan_views_framed_async, True, vp(opn), vp(msk))}
    gats = {"rays": mk(L.qr_gather_rays_framed_async, False, vp(gat), vp(cnt)), "hits": mk(L.qr_gather_hits_framed_async, False, vp(gat), vp(cnt)),
            "views": mk(L.qr_gather_views_framed_async, True, vp(gat), vp(cnt))}
    src = {"rays": vp(rays), "hits": vp(hits)}

    def call(table, name, s, **kw):
        return table[name](s, **kw) if name == "views" else table[name](s, kw.pop("r", src[name]), **kw)

    plain = qr.Scene(blob)
    for table in (fans, gats):
        for name in table:
            assert call(table, name, plain._h) == UNSUP
    with pytest.raises(qr.QrError, match="QR_UPLOAD_RAY_QUERIES"):
        plain.occlusion(rays, dirs[:4], EPS, frame=True)
    plain.close()

    scn = qr.Scene(blob, ray_queries=True)
    for table, bad_flag in ((fans, 4), (gats, 16)):
        for name in table:
            f = lambda **kw: call(table, name, scn._h, **kw)
            assert call(table, name, None) == ARG
            assert f(d=None) == ARG and f(a=None) == ARG
            assert f(d=vp(dirs, 4)) == ARG and f(d=vp(dirs, 8)) == ARG                              # misaligned
            assert f(sp=vp(spin, 4)) == ARG and f(sp=vp(spin, 2)) == ARG, "a misaligned spin is refused"
            assert f(k=0) == ARG and f(k=-3) == ARG and f(k=1025) == ARG
            assert f(eps=nan) == ARG and f(reach=nan) == ARG
            assert f(flags=bad_flag) == ARG and f(flags=0x80000000) == ARG
            assert f(n=-1) == ARG
            assert f(n=0) == 0
            if name == "views":
                assert f(v=None) == ARG and f(v=vp(vt, 8)) == ARG and f(w=0) == ARG and f(h=0) == ARG and f(w=16385) == ARG
                assert f(n=65536) == ARG and f(flags=1) == ARG
            else:
                assert f(r=None) == ARG and f(r=vp(rays, 4)) == ARG and f(n=1 << 31) == ARG
                assert (f(flags=1) == 0) == (name == "rays"), "QR_TRACE_COHERENT: caller rays only"
    for name in gats:
        assert call(gats, name, scn._h, b=None) == ARG and call(gats, name, scn._h, a=vp(gat, 8)) == ARG
        assert call(gats, name, scn._h, b=vp(cnt, 2)) == ARG
    for name in fans:
        assert call(fans, name, scn._h, a=vp(opn, 2)) == ARG and call(fans, name, scn._h, b=vp(msk, 1)) == ARG
    scn.set_pt(True)                                            # a scene in its own path-tracer mode: as shade()
    for name in gats:
        assert call(gats, name, scn._h) == UNSUP
    scn.set_pt(False)
    _sync()
    # nothing was written: every call so far was refused, had n == 0, or (flags=1 on caller rays) wrote 64 elements
    assert (opn[64:] == 77).all().item() and (msk[64:16 * 2 * h * w] == 77).all().item()
    assert (gat[64:] == 7.5).all().item() and (cnt[64:] == 77).all().item(), "a refused call wrote something"
    # calls that are served: spin null, spin aligned at an odd element, every flag, 1024 directions
    for table, flags in ((fans, 2), (gats, 2 | 4 | 8)):
        for name in table:
            f = lambda **kw: call(table, name, scn._h, **kw)
            assert f() == 0 and f(sp=None) == 0 and f(sp=vp(spin, 8)) == 0 and f(flags=flags) == 0 and f(k=1024, n=1) == 0
    assert call(fans, "rays", scn._h, b=None) == 0, "no mask wanted"
    _sync()
    # the Python layer
    sp = spin[:128].contiguous()
    with pytest.raises(ValueError, match="frame=True"):
        scn.occlusion(rays, dirs[:4], EPS, spin=sp)
    with pytest.raises(ValueError, match="frame=True"):
        scn.view_gather(vt, dirs[:4], w, h, eps=EPS, spin=spin[:2 * h * w].reshape(2, h, w, 2))
    for bad in (sp[:127], sp.double(), sp.cpu(), spin[:256:2], sp.reshape(-1), sp.cpu().numpy(), torch.zeros((128, 3), device=dev)):
        for fn, first in ((scn.occlusion, rays), (scn.gather, rays), (scn.hit_occlusion, hits), (scn.hit_gather, hits)):
            with pytest.raises(ValueError, match="spin must be"):
                fn(first, dirs[:4], EPS, frame=True, spin=bad)
    for fn in (scn.view_occlusion, scn.view_gather):
        with pytest.raises(ValueError, match="spin must be"):
            fn(vt, dirs[:4], w, h, eps=EPS, frame=True, spin=spin[:2 * h * w])                     # [N * H * W, 2], not [N, H, W, 2]
    with pytest.raises(qr.QrError, match="dirs must"):
        scn.occlusion(rays, dirs.double(), EPS, frame=True)
    with pytest.raises(qr.QrError, match="resume=True needs both buffers"):
        scn.gather(rays, dirs[:4], EPS, frame=True, resume=True)
    e, ec = scn.gather(rays[:0], dirs[:40], EPS, frame=True, spin=sp[:0])
    assert tuple(e.shape) == (0, 4) and tuple(ec.shape) == (0,)
    assert tuple(scn.view_occlusion(vt, dirs[:4], eps=EPS, frame=True).shape) == (2, scn.height, scn.width)
    miss = hits.clone()
    miss.view(torch.int32)[:, 7] = -1
    g, c = scn.hit_gather(miss, dirs[:4], EPS, frame=True, spin=sp, out=torch.full((128, 4), 3.0, device=dev),
                          count=torch.full((128,), 3, dtype=torch.int32, device=dev), resume=True)
    o, m = scn.hit_occlusion(miss, dirs[:4], EPS, frame=True, spin=sp, mask=True)
    _sync()
    assert (c == -1).all().item() and (g.view(torch.int32) == 0).all().item() and (o == -1).all().item() and (m == 0).all().item()
    scn.close()


# once more through the guarded diagnostic build (make guard), as the two fan test files do: the library is chosen when the
# package is imported, hence the child process: this file run as a script.

def _guard_child():
    from qr_loader import load_package
    qr = load_package()
    assert qr.LIB_PATH == GUARD_LIB, qr.LIB_PATH
    import qr_oracle
    rays_mod, helper = _rays_mod(), _helper()
    name = "synth_small"
    blob = RS.scene_blob(name)
    dirs = _table(rays_mod)
    scn = _rs_scene(qr, name)
    views = [rays_mod.view_of(blob)] + [rays_mod.view_of(c) for c in _rayq.random_cameras(blob, seed=11, n=1)]
    _check_views(scn, qr_oracle, rays_mod, helper, blob, f"guard {name}", views, 67, 45, dirs, 5, combos=[(False, True), (True, False)],
                 spins=(True,))
    rays = RS.mixed(blob, name, qr_oracle)
    hits = helper(blob, rays)
    spin = rays_mod.spins(len(rays), 6)
    want_o = _occ_truth(qr_oracle, rays_mod, blob, hits, dirs, EPS, REACH, True, spin)
    want_g = _fold(rays_mod, hits, dirs, _colours(qr_oracle, rays_mod, blob, hits, dirs, EPS, REACH, True, spin), True, True, spin)
    for coherent in (False, True):
        opn, msk, g, c = _ray_calls(scn, rays, dirs, spin, True, True, coherent)
        OF._same(f"guard {name} mixed coherent={coherent}", opn, msk, want_o[0], want_o[1])
        GF._same(f"guard {name} mixed coherent={coherent}", g, c, *want_g)
    kw = dict(flip=True, frame=True, spin=_cuda(scn, spin))
    opn, msk = scn.hit_occlusion(_cuda(scn, hits), _cuda(scn, dirs), EPS, REACH, mask=True, **kw)
    g, c = scn.hit_gather(_cuda(scn, hits), _cuda(scn, dirs), EPS, REACH, cosine=True, **kw)
    _sync()
    OF._same(f"guard {name} records", opn, msk, want_o[0], want_o[1])
    GF._same(f"guard {name} records", g, c, *want_g)
    scn.close()
    print(f"{name} guard_ok 1", flush=True)
    return 0


@pytest.mark.gpu
def test_gpu_guarded_build_gives_the_same_framed_fans():
    assert os.path.exists(GUARD_LIB), "libqrhip_guard.so is missing: build() makes it (make -C quadray-engine_amd/csrc guard)"
    env = dict(os.environ, QR_LIB=GUARD_LIB)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-child"], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.count("guard_ok 1") == 1 and "QR_GUARD" not in out.stderr, out.stdout + out.stderr[-3000:]


if __name__ == "__main__":
    sys.exit(_guard_child() if "--guard-child" in sys.argv else 2)
