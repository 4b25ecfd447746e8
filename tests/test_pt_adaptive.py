"""Adaptive path-traced rays (include/qrhip.h qr_pt_adapt_rays_async, Scene.pt_adaptive): path-tracer samples for caller rays with a
sample count and Welford's M2 per ray in an int32 [8, N] state the caller owns, and a stop rule evaluated on chip before every
sample; and the host side of it in quadray-engine_amd/rays.py (pt_adapt_fold, pt_adapt_open).

Every GPU comparison is bit for bit over all eight state planes, rgb and open.  The truth is rays.pt_adapt_fold over
tests/ptadapt_oracle.c (qrp_pt_samples): the raw colour of each of a ray's consecutive samples and the generator word after
each, read out of the oracle's path tracer -- no mean, no count and no rule in it.  The CPU tests pin that translation unit to
tests/ptrays_oracle.c (qrp_pt_rays), the fold to a float64 two-pass sum, and show that the inputs discriminate, before any GPU
is involved.

Scenes, cameras and rays: those of tests/test_pt_rays.py -- view_rays(cam, 64, 64, base, 0), 4096 rays, the pinhole spread.
The settings of the seeded-view tests: min_samples 2, max_samples 12, 12 candidates, one tolerance per scene (TOL).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _ptpatch
import _rayset as RS
import test_pt_rays as TPR
import test_pt_views as TPV
from conftest import ROOT
from test_pt_views import SCENES, _base, _bits, _cams, _rays_mod

ASM = TPV.ASM
GUARD_LIB = TPV.GUARD_LIB
GUARD_CASE = ("patched:demo02_160_gf_aa4", 2)               # scene, view
ARG, UNSUP = -1, -3
MIN, MAX, CAND = 2, 12, 12
# The tolerance on the standard error of the mean per scene, in linear colour units (tol2 = float32(tol) ** 2): fixed here after
# running test_inputs_discriminate, which prints what each value gives
TOL = {"pt:test18_160_pt": 0.07, "pt:test18_160_gf_aa4_pt": 0.07, "patched:demo01_160": 0.3, "patched:demo02_160_gf_aa4": 0.2,
       "patched:demo03_160": 0.07, "patched:test13_160_gf_aa4": 0.2}
VIEW = TPR.VIEW
_view_rays = TPR._view_rays


@pytest.fixture(scope="module")
def rays_mod():
    return _rays_mod()


def _tol2(tol):
    t = np.float32(tol)
    return t * t


# ------------------------------------------------------------------------------------------------- the truth (CPU)

_TU = None


def _tu():
    global _TU
    if _TU is None:
        import __graft_entry__ as g
        L = ctypes.CDLL(g.build_ptadapt_oracle())
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.qrp_pt_samples.argtypes = [vp, ctypes.c_uint64, vp, vp, ctypes.c_int64, vp, ci, ci, ci, vp, vp]
        L.qrp_pt_samples.restype = ci
        _TU = L
    return _TU


def _samples(blob, rays, spread, rng_in, samples, depth=None):
    """qrp_pt_samples: (cols float32 [N, S, 3], rngs uint32 [N, S]) of the S consecutive samples of every ray from rng_in"""
    r = np.ascontiguousarray(rays, dtype=np.float32)
    n = r.shape[0]
    assert r.shape == (n, 8)
    sp = None if spread is None else np.ascontiguousarray(spread, dtype=np.float32)
    assert sp is None or sp.shape == (n, 8)
    rin = np.ascontiguousarray(rng_in).view(np.uint32).copy()
    assert rin.shape == (n,)
    cols = np.zeros((n, samples, 3), dtype=np.float32)
    rngs = np.zeros((n, samples), dtype=np.uint32)
    buf = ctypes.create_string_buffer(blob, len(blob))
    rc = _tu().qrp_pt_samples(buf, len(blob), r.ctypes.data, None if sp is None else sp.ctypes.data, n, rin.ctypes.data,
                              int(samples), -1 if depth is None else int(depth), 16, cols.ctypes.data, rngs.ctypes.data)
    assert rc == 0, rc
    return cols, rngs


def _fresh(rm, n):
    """the state after a reset: plane 0 = pt_seeds(n, 1, 1), every other plane 0"""
    st = np.zeros((8, n), dtype=np.uint32)
    st[0] = rm.pt_seeds(n, 1, 1)
    return st


_SEQ = {}


def _seq(rm, scene, j, spread, depth=None):
    """the CAND candidate samples of view j's rays from a fresh state; computed once, read-only"""
    key = (scene, j, bool(spread), depth)
    if key not in _SEQ:
        r, sp = _view_rays(rm, scene, j)
        cols, rngs = _samples(_base(scene), r, sp if spread else None, rm.pt_seeds(len(r), 1, 1), CAND, depth)
        cols.setflags(write=False); rngs.setflags(write=False)
        _SEQ[key] = (cols, rngs)
    return _SEQ[key]


def _window(seq, state, samples):
    """the next `samples` candidates of every ray of a state that was reached from a fresh one on the rays of `seq`: ray i holds
    m = plane 4 samples, so its candidates are numbers m .. m + samples - 1 of its sequence.  Past the sequence's end: NaN
    colours, which poison whatever takes them"""
    cols, rngs = seq
    n, total = rngs.shape
    m = state.view(np.uint32)[4].astype(np.int64)
    idx = m[:, None] + np.arange(samples)[None, :]
    ok = idx < total
    idx = np.where(ok, idx, 0)
    rows = np.arange(n)[:, None]
    c = np.where(ok[:, :, None], cols[rows, idx], np.float32(np.nan)).astype(np.float32)
    return c, np.where(ok, rngs[rows, idx], np.uint32(0xDEADBEEF)).astype(np.uint32)


def _truth(rm, scene, j, spread, splits=(CAND,), mn=MIN, mx=MAX, tol=None, depth=None):
    """[(state, rgb, open) after every call] of the fold for view j from a fresh state"""
    t2 = _tol2(TOL[scene] if tol is None else tol)
    seq = _seq(rm, scene, j, spread, depth)
    st = _fresh(rm, seq[1].shape[0])
    out = []
    for s in splits:
        c, g = _window(seq, st, s)
        st, rgb, op = rm.pt_adapt_fold(st, c, g, mn, mx, t2)
        out.append((st, rgb, op))
    return out


def _truth_call(rm, blob, rays, spread, state, samples, mn, mx, tol, depth=None):
    """(state', rgb, open) of one call on any state and any rays: the fold over the samples from the state's generator words"""
    c, g = _samples(blob, rays, spread, state.view(np.uint32)[0], samples, depth)
    return rm.pt_adapt_fold(state, c, g, mn, mx, _tol2(tol))


# ---------------------------------------------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("scene", ["pt:test18_160_pt", "pt:test18_160_gf_aa4_pt", "patched:demo02_160_gf_aa4"])
@pytest.mark.parametrize("spread", [True, False])
def test_tu_is_the_oracles_path_tracer_and_the_fold_is_welfords(rays_mod, scene, spread):
    """min = max = 5 from a fresh state: planes 0..3 of the fold over qrp_pt_samples are qrp_pt_rays' (tests/ptrays_oracle.c) with
    done = 0, samples = 5, word for word, and plane 4 is 5 everywhere.  Planes 5..7 agree with the float64 two-pass sum of
    squared deviations of the colours; so do the 12-sample ones.

    The bound.  With eps = 2^-24 (half an ulp, the relative error of one fp32 operation) every update computes p = d1 * d2 from
    a mean that carries the rounding of the k - 1 updates before it (each: two products, a sum, and the rounding of o and u:
    at most 5 eps relative to the largest of |col|, |mean|) and adds it with one more rounding.  Measured against
    S = sum |col - mean64|^2 + n * max|col|^2 -- the exact M2 plus the scale the cancelling differences d1, d2 are rounded at --
    the error of M2 after n samples is at most n updates * (5 (n - 1) + 4) eps * that scale: for n <= 12, 12 * 59 * 2^-24 < 4.3e-5.
    The bound used is 5e-5 * (M2_64 + n * max|col|^2): a rounding bound, not a measurement."""
    j = VIEW[scene]
    r, sp = _view_rays(rays_mod, scene, j)
    n = len(r)
    cols, rngs = _seq(rays_mod, scene, j, spread)
    st, rgb, op = rays_mod.pt_adapt_fold(_fresh(rays_mod, n), cols[:, :5], rngs[:, :5], 5, 5, _tol2(0.5))
    wrgb, wst, _ = TPR._tu_run(_base(scene), r, sp if spread else None, TPR._fresh(rays_mod, n), 0, 5)
    assert (st[:4] == wst).all(), f"{scene}: {int((st[:4] != wst).any(axis=0).sum())} of {n} columns differ from qrp_pt_rays"
    assert (_bits(rgb) == _bits(wrgb)).all() and (st[4] == 5).all() and op == 0
    assert (rgb != 0).any()
    for ns in (5, 12):
        st, _, _ = rays_mod.pt_adapt_fold(_fresh(rays_mod, n), cols[:, :ns], rngs[:, :ns], ns, ns, _tol2(0.5))
        c64 = cols[:, :ns].astype(np.float64)
        m2 = ((c64 - c64.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)                 # [n, 3]
        got = st[5:8].view(np.float32).T.astype(np.float64)
        bound = 5e-5 * (m2 + ns * (c64 ** 2).max(axis=1))
        err = np.abs(got - m2)
        print(f"{scene} spread={spread} {ns} samples: largest M2 {m2.max():.4g}, largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3g}")
        assert (st[4] == ns).all() and (err <= bound).all()
        assert (m2 > 0).mean() > 0.1, "the colours of a ray's samples do not differ"


def _rows(rm, scene, tol):
    """per seeded view (with the spread): fraction stopped early with m >= 2, fraction at MAX, distinct counts, waves all early"""
    rows = []
    for j in range(4):
        st, _, op = _truth(rm, scene, j, True, tol=tol)[0]
        m = st[4]
        early = float(((m >= 2) & (m < MAX)).mean())
        full = float((m == MAX).mean())
        waves = int((m.reshape(-1, 64) < MAX).all(axis=1).sum())
        rows.append((early, full, len(np.unique(m)), waves, op))
    return rows


@pytest.mark.parametrize("scene", SCENES)
def test_inputs_discriminate(rays_mod, scene):
    """A condition on the test inputs, checked with the truth alone, at min 2, max 12, 12 candidates and the scene's TOL:
      - at least two of the four seeded views have >= 15 % of the rays stopped before max with m >= 2;
      - >= 15 % of the rays reach max, in a view that also meets the line above -- the view the single-view tests use (VIEW),
        where they name one -- so that both kinds of ray sit side by side in the same waves;
      - the counts of some view take >= 4 distinct values;
      - some wave-aligned group of 64 consecutive rays has every ray stopped before sample 12 (the early wave exit);
      - tol2 doubled changes plane 4 on >= 5 % of that view's rays.
    Five of the six scenes have two views and more with both >= 15 % stopped early and >= 15 % at max, and the test says so.
    pt:test18_160_gf_aa4_pt cannot: its views 2 and 3 see no light at all (every ray stops at m = 2) and in view 0 only the
    11.7 % of rays whose first two samples differ can ever go past m = 2, whatever the tolerance (figures at tol2 = 0: stopped
    early / at max 88.3 / 11.7, 68.2 / 31.8, 100 / 0, 100 / 0 per cent); view 1 carries both kinds there"""
    rows = _rows(rays_mod, scene, TOL[scene])
    print(f"{scene} tol {TOL[scene]}: early % / at max % / distinct counts / waves all early / open, per view: "
          + "; ".join(f"{100 * e:.1f} {100 * f:.1f} {d} {w} {o}" for e, f, d, w, o in rows))
    assert sum(e >= 0.15 for e, *_ in rows) >= 2, rows
    ok = [e >= 0.15 and f >= 0.15 for e, f, _, _, _ in rows]
    assert sum(ok) >= (1 if scene == "pt:test18_160_gf_aa4_pt" else 2), rows
    assert scene not in VIEW or ok[VIEW[scene]], rows
    assert max(d for _, _, d, _, _ in rows) >= 4, rows
    assert sum(w for _, _, _, w, _ in rows) >= 1, rows
    assert all(o == 0 for *_, o in rows), "after 12 candidates at max 12 nothing is open"
    j = VIEW.get(scene, [i for i, k in enumerate(ok) if k][0])
    seq = _seq(rays_mod, scene, j, True)
    n = seq[1].shape[0]
    a = rays_mod.pt_adapt_fold(_fresh(rays_mod, n), seq[0], seq[1], MIN, MAX, _tol2(TOL[scene]))[0]
    b = rays_mod.pt_adapt_fold(_fresh(rays_mod, n), seq[0], seq[1], MIN, MAX, np.float32(2) * _tol2(TOL[scene]))[0]
    moved = float((a[4] != b[4]).mean())
    print(f"{scene} view {j}: tol2 doubled changes the count of {100 * moved:.1f} % of the rays")
    assert moved >= 0.05


def test_rule_on_a_constructed_state(rays_mod):
    """pt_adapt_open on states written by hand: the m < 2 clause (M2 = 0 <= lim = 0 would otherwise stop a ray after its first
    sample), <= and not < (M2 == lim converges), NaN never converges, min and max, m read as unsigned; and the fold leaves the
    columns it does not take bit for bit and keeps a prefix of the candidates"""
    f = lambda *v: np.array(v, dtype=np.float32).view(np.uint32)
    t2 = np.float32(0.25)
    #            m    M2r   M2g   M2b      open at min 0, max 12
    cases = [(0,   0.0,  0.0,  0.0,   True),        # m < 2
             (1,   0.0,  0.0,  0.0,   True),        # m < 2: lim = 1 * 0 * tol2 = 0 and M2 = 0 <= 0
             (2,   0.5,  0.5,  0.5,   False),       # lim = 2 * 1 * 0.25 = 0.5: M2 == lim converges (<=)
             (2,   0.5,  np.float32(0.5) + np.float32(2.0 ** -24), 0.5, True),
             (2,   0.0,  0.0,  0.50001, True),      # one channel is enough to go on
             (3,   1.5,  1.5,  1.5,   False),       # lim = 3 * 2 * 0.25
             (3,   np.nan, 0.0, 0.0,  True),        # a NaN never converges
             (5,   -1.0, -np.inf, 0.0, False),
             (11,  np.inf, 0.0, 0.0,  True),
             (12,  np.inf, np.nan, 9e9, False),     # m >= max
             (13,  np.inf, 0.0, 0.0,  False),
             (0xFFFFFFFF, np.nan, 0.0, 0.0, False)] # unsigned
    st = np.zeros((8, len(cases)), dtype=np.uint32)
    for i, (m, a, b, c, _) in enumerate(cases):
        st[4, i] = m
        st[5:8, i] = f(a, b, c)
    got = rays_mod.pt_adapt_open(st, 0, 12, t2)
    assert got.dtype == bool and got.tolist() == [c[4] for c in cases], got.tolist()
    assert rays_mod.pt_adapt_open(st.view(np.int32), 0, 12, t2).tolist() == got.tolist()
    # min_samples: everything below it is open whatever M2 says, up to max
    assert rays_mod.pt_adapt_open(st, 12, 12, t2).tolist() == [c[0] < 12 for c in cases]
    assert rays_mod.pt_adapt_open(st, 3, 12, t2).tolist() == [c[4] or c[0] == 2 for c in cases]
    # the fold: constant colours give M2 = 0 exactly, so at tol2 = 0 a ray stops after two samples; columns that do not take
    # a candidate keep every bit, NaN and sentinels included
    n = len(cases)
    st[0] = np.arange(n) + 100
    st[1:4] = f(7.0)[0]
    cols = np.full((n, 4, 3), 3.0, dtype=np.float32)
    rngs = (np.arange(n * 4, dtype=np.uint32) + 1000).reshape(n, 4)
    out, rgb, op = rays_mod.pt_adapt_fold(st, cols, rngs, 0, 12, np.float32(0))
    keep = ~rays_mod.pt_adapt_open(st, 0, 12, np.float32(0))
    assert keep.any() and not keep.all()
    assert (out[:, keep] == st[:, keep]).all() and (_bits(rgb[keep]) == st[1:4, keep].T).all()
    assert out[4, 0] == 2 and out[0, 0] == rngs[0, 1] and (out[5:8, 0] == 0).all() and (rgb[0] == 3.0).all()
    assert out[4, 1] == 5 and out[0, 1] == rngs[1, 3], "mean 7 then 3, 3, 3, 3: M2 > 0 = lim, the ray goes on"
    assert out[4, 6] == 7 and np.isnan(out[5, 6:7].view(np.float32)).all()
    assert op == int(rays_mod.pt_adapt_open(out, 0, 12, np.float32(0)).sum()) and op >= 2
    with pytest.raises(ValueError):
        rays_mod.pt_adapt_fold(st, cols[:3], rngs, 0, 12, t2)
    with pytest.raises(ValueError):
        rays_mod.pt_adapt_open(st[:4], 0, 12, t2)


def test_pt_adaptive_abi_and_constants(qr):
    """the library exports the three entry points, the header declares them, and its constants are the module's"""
    L = qr.lib()
    with open(os.path.join(ROOT, "include", "qrhip.h")) as f:
        hdr = f.read()
    for sym in ("qr_pt_adapt_state_bytes", "qr_pt_adapt_reset", "qr_pt_adapt_rays_async"):
        assert hasattr(L, sym), sym
        assert sym in qr.ABI_SYMBOLS and f"int {sym}(" in hdr, sym
    assert f"#define QR_PT_ADAPT_MAX_SAMPLES {qr.PT_ADAPT_MAX_SAMPLES} " in hdr and qr.PT_ADAPT_MAX_SAMPLES == 512
    assert f"#define QR_PT_ADAPT_STATE_WORDS {qr.PT_ADAPT_STATE_WORDS} " in hdr and qr.PT_ADAPT_STATE_WORDS == 8
    assert "int samples, int min_samples, int max_samples, float tol2," in hdr
    assert hasattr(qr.Scene, "pt_adaptive") and hasattr(qr, "PtAdaptive")
    for m in ("step", "reset", "clone"):
        assert callable(getattr(qr.PtAdaptive, m))
    assert isinstance(qr.PtAdaptive.counts, property)
    rm = _rays_mod()
    assert callable(rm.pt_adapt_fold) and callable(rm.pt_adapt_open)


def test_pt_adapt_kernel_in_resource_check():
    """the build's register check lists the kernel once, at the path-traced ray kernel's budget (168 VGPRs, nothing spilled,
    2128 B of private segment), and the built assembly passes it"""
    import importlib.util
    path = os.path.join(ROOT, "tools", "check_kernel_resources.py")
    spec = importlib.util.spec_from_file_location("check_kernel_resources", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    frags = [f for f in m.LIMITS if "qr_pt_adapt_kernel" in f]
    assert frags == ["18qr_pt_adapt_kernel"]
    assert m.LIMITS[frags[0]] == (168, 0, 2128) == m.LIMITS["17qr_pt_rays_kernel"]
    r = subprocess.run([sys.executable, path, ASM, "--print"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("qr_pt_adapt_kernel") == 1


# ---------------------------------------------------------------------------------------------------------------- GPU

_t, _host = TPR._t, TPR._host


def _dev_state(scn, st):
    import torch
    return torch.from_numpy(np.ascontiguousarray(st).view(np.int32).copy()).to(f"cuda:{scn.device}")


def _acc(scn, n, mn=MIN, mx=MAX, tol=None, state=None):
    return scn.pt_adaptive(n, mn, mx, tol, state=None if state is None else _dev_state(scn, state))


def _step(acc, rt, samples, st=None):
    """one step with rgb and open: (state uint32 [8, N], rgb, open) on the host"""
    rgb, op = acc.step(rt, samples, spread=st, open=True)
    assert tuple(rgb.shape) == (acc.n, 3) and op.numel() == 1
    return _host(acc.state).view(np.uint32), _host(rgb), int(_host(op).view(np.uint32)[0])


def _run(scn, rays, spread, splits, mn=MIN, mx=MAX, tol=None, state=None):
    """an accumulation (fresh, or started from `state`) stepped by `splits`: [(state, rgb, open) after every call]"""
    acc = _acc(scn, len(rays), mn, mx, tol, state)
    rt, st = _t(scn, rays), None if spread is None else _t(scn, spread)
    return [_step(acc, rt, s, st) for s in splits]


def _same(got, want, what):
    (gst, grgb, gop), (wst, wrgb, wop) = got, want
    gst, wst = gst.view(np.uint32), wst.view(np.uint32)
    assert gst.shape == wst.shape and grgb.shape == wrgb.shape and grgb.dtype == np.float32
    bad = [int((gst[p] != wst[p]).sum()) for p in range(8)]
    nr = int((_bits(grgb) != _bits(wrgb)).any(axis=1).sum())
    assert not any(bad) and nr == 0 and gop == wop, \
        f"{what}: of {gst.shape[1]} rays, per plane {bad} state words differ, {nr} rays differ in rgb; open {gop}, want {wop}"
    assert (_bits(grgb) == gst[1:4].T).all(), f"{what}: rgb is not the state's means"


@pytest.mark.gpu
@pytest.mark.parametrize("scene", SCENES)
def test_gpu_seeded_views_equal_the_fold(qr, rays_mod, scene):
    """the four seeded views' rays, with and without the spread, min 2, max 12, the scene's tolerance, 12 candidates in one
    call: all eight planes, rgb and open are the fold's over the oracle's samples"""
    scn = qr.Scene(_base(scene), ray_queries=True)
    got = {}
    for j in range(4):
        r, sp = _view_rays(rays_mod, scene, j)
        for spread in (True, False):
            got[j, spread] = _run(scn, r, sp if spread else None, (CAND,), tol=TOL[scene])[0]
    scn.close()
    for (j, spread), g in got.items():
        _same(g, _truth(rays_mod, scene, j, spread)[0], f"{scene} view {j} spread={spread}")


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["pt:test18_160_pt", "patched:demo02_160_gf_aa4"])
def test_gpu_splits(qr, rays_mod, scene):
    """12 candidates as 5 + 7, 1 x 12 and 3 + 3 + 3 + 3: state, rgb and open after EVERY call are the fold's, and the final
    ones are those of one call of 12"""
    j = VIEW[scene]
    r, sp = _view_rays(rays_mod, scene, j)
    splits = [(5, 7), (1,) * 12, (3, 3, 3, 3), (12,)]
    scn = qr.Scene(_base(scene), ray_queries=True)
    got = [_run(scn, r, sp, s, tol=TOL[scene]) for s in splits]
    scn.close()
    opens = []
    for s, g in zip(splits, got):
        want = _truth(rays_mod, scene, j, True, s)
        for k in range(len(s)):
            _same(g[k], want[k], f"{scene}: split {s}, call {k}")
        _same(g[-1], got[-1][0], f"{scene}: split {s} against 12 in one call")
        opens.append([x[2] for x in g])
    assert opens[0][0] > 0 and opens[1][0] == len(r) and opens[2][-1] == 0, opens


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["pt:test18_160_gf_aa4_pt", "patched:demo01_160"])
def test_gpu_min_equals_max_is_pt_rays(qr, rays_mod, scene):
    """min = max = 7: planes 0..3 are Scene.pt_rays' state on the same GPU after 7 samples (in 3 + 4 here, 7 there), plane 4
    is 7 and open is 0"""
    r, sp = _view_rays(rays_mod, scene, VIEW[scene])
    scn = qr.Scene(_base(scene), ray_queries=True)
    a = _run(scn, r, sp, (3, 4), mn=7, mx=7, tol=TOL[scene])
    more = _run(scn, r, sp, (9,), mn=7, mx=7, tol=0.0)[0]
    prgb, pst = TPR._run(scn, r, sp, (7,))
    scn.close()
    st, rgb, op = a[1]
    assert (st[:4] == pst.view(np.uint32)).all(), f"{scene}: {int((st[:4] != pst.view(np.uint32)).any(axis=0).sum())} columns differ from pt_rays"
    assert (_bits(rgb) == _bits(prgb)).all() and (st[4] == 7).all() and op == 0 and a[0][2] == len(r)
    assert (st[5:8] != 0).any()
    _same(more, a[1], f"{scene}: 9 candidates at max 7")


@pytest.mark.gpu
def test_gpu_retired_rays_are_untouched(qr, rays_mod):
    """after 6 candidates some rays have converged and some are open; a second call with OTHER rays and another spread leaves
    the converged columns bit-identical in all eight planes while rgb still reports their means, and the others advance as the
    fold says on the new rays"""
    scene = "patched:demo02_160_gf_aa4"
    j = VIEW[scene]
    r, sp = _view_rays(rays_mod, scene, j)
    r2, sp2 = _view_rays(rays_mod, scene, (j + 1) % 4)
    sp2 = (sp2 * np.float32(0.5)).astype(np.float32)
    first = _truth(rays_mod, scene, j, True, (6,))[0]
    done = ~rays_mod.pt_adapt_open(first[0], MIN, MAX, _tol2(TOL[scene]))
    assert 0.1 < done.mean() < 0.9 and first[2] == int((~done).sum())
    scn = qr.Scene(_base(scene), ray_queries=True)
    acc = _acc(scn, len(r), tol=TOL[scene])
    a = _step(acc, _t(scn, r), 6, _t(scn, sp))
    b = _step(acc, _t(scn, r2), 6, _t(scn, sp2))
    scn.close()
    _same(a, first, f"{scene}: the first 6")
    assert (b[0][:, done] == a[0][:, done]).all(), "a converged column changed"
    assert (_bits(b[1][done]) == a[0][1:4, done].T).all(), "rgb does not report the converged rays' means"
    want = _truth_call(rays_mod, _base(scene), r2, sp2, first[0], 6, MIN, MAX, TOL[scene])
    _same(b, want, f"{scene}: 6 more on other rays")
    assert (b[0][4, ~done] > a[0][4, ~done]).all()


@pytest.mark.gpu
def test_gpu_permutation_and_single_rays(qr, rays_mod):
    """rays permuted together with their state columns give permuted results; ray i of a batch is ray i alone"""
    scene = "pt:test18_160_pt"
    r, sp = _view_rays(rays_mod, scene, VIEW[scene])
    n = len(r)
    perm = np.random.default_rng(11).permutation(n)
    st0 = _fresh(rays_mod, n)
    scn = qr.Scene(_base(scene), ray_queries=True)
    a = _run(scn, r, sp, (CAND,), tol=TOL[scene])[0]
    b = _run(scn, r[perm], sp[perm], (CAND,), tol=TOL[scene], state=st0[:, perm])[0]
    picks = [0, 63, 64, 2077, n - 1]
    alone = [_run(scn, r[i:i + 1], sp[i:i + 1], (CAND,), tol=TOL[scene], state=st0[:, i:i + 1])[0] for i in picks]
    scn.close()
    _same(a, _truth(rays_mod, scene, VIEW[scene], True)[0], scene)
    _same(b, (a[0][:, perm], a[1][perm], a[2]), f"{scene}: permuted rays")
    assert (a[0][4] != b[0][4]).mean() > 0.1, "the permutation moved nothing"
    for i, one in zip(picks, alone):
        open_i = int(rays_mod.pt_adapt_open(a[0][:, i:i + 1], MIN, MAX, _tol2(TOL[scene])).sum())
        _same(one, (a[0][:, i:i + 1], a[1][i:i + 1], open_i), f"{scene}: ray {i} alone")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 129])
def test_gpu_batch_sizes_and_bounds(qr, rays_mod, n):
    """partial and full waves; state, rgb and open carved out of larger sentinel-filled buffers: the fold's bits, and reset and
    launch leave the tails -- the word after open among them -- alone"""
    import torch
    scene = "patched:demo02_160_gf_aa4"
    r, sp = _view_rays(rays_mod, scene, VIEW[scene])
    r, sp = r[1000:1000 + n], sp[1000:1000 + n]
    TAIL, SI, SF = 4096, 0x5A5A5A5A, 12345.0
    scn = qr.Scene(_base(scene), ray_queries=True)
    dev = f"cuda:{scn.device}"
    stb = torch.full((8 * n + TAIL,), SI, dtype=torch.int32, device=dev)
    rgbb = torch.full((3 * n + TAIL,), SF, dtype=torch.float32, device=dev)
    opb = torch.full((4,), SI, dtype=torch.int32, device=dev)
    acc = scn.pt_adaptive(n, MIN, MAX, TOL[scene], state=stb[:8 * n].view(8, n))
    acc.reset()
    torch.cuda.synchronize()
    assert (stb[8 * n:] == SI).all(), "reset wrote past the state"
    assert (_host(acc.state).view(np.uint32) == _fresh(rays_mod, n)).all()
    out, op = acc.step(_t(scn, r), 7, spread=_t(scn, sp), rgb=rgbb[:3 * n].view(n, 3), open=opb[1:2])
    assert out.data_ptr() == rgbb.data_ptr() and op.data_ptr() == opb[1:2].data_ptr()
    got = (_host(acc.state).view(np.uint32), _host(out), int(_host(opb)[1]))
    none = acc.clone().step(_t(scn, r), 1, spread=_t(scn, sp), rgb=False)
    tails_ok = bool((stb[8 * n:] == SI).all()) and bool((rgbb[3 * n:] == SF).all())
    op_ok = _host(opb)[[0, 2, 3]].tolist() == [SI] * 3
    counts = _host(acc.counts)
    scn.close()
    assert none is None and tails_ok and op_ok, f"n = {n}: a tail was written"
    want = _truth_call(rays_mod, _base(scene), r, sp, _fresh(rays_mod, n), 7, MIN, MAX, TOL[scene])
    _same(got, want, f"{scene} n = {n}")
    assert (counts.view(np.uint32) == want[0][4]).all()


@pytest.mark.gpu
def test_gpu_edited_state(qr, rays_mod):
    """a state edited by the host: columns with m >= max take nothing, columns with m = 0, 1 always take, a NaN in an M2 plane
    never converges and stops at max; and tol2 = 0 stops exactly the rays whose three M2 are <= 0 -- the rays that miss
    everything, whose samples are all equal"""
    scene = "patched:demo01_160"
    blob = _base(scene)
    r, sp = _view_rays(rays_mod, scene, VIEW[scene])
    n = len(r)
    f32 = lambda v: np.array([v], dtype=np.float32).view(np.uint32)[0]
    st = _truth(rays_mod, scene, VIEW[scene], True, (4,), tol=0.05)[0][0].copy()
    rng = np.random.default_rng(5)
    kind = rng.integers(0, 6, n)
    st[4, kind == 1] = MAX                                              # full: nothing
    st[4, kind == 2] = 0xFFFFFF00                                       # far above max, unsigned: nothing
    st[4, kind == 3] = rng.integers(0, 2, int((kind == 3).sum()))      # m = 0, 1 with an M2 the rule would call converged
    st[5:8, kind == 3] = 0
    st[6, kind == 4] = f32(np.nan)                                      # never converges: runs to max
    st[5:8, kind == 5] = f32(-1.0)                                      # a negative M2 is below every limit
    scn = qr.Scene(blob, ray_queries=True)
    got = _run(scn, r, sp, (CAND,), tol=0.05, state=st)[0]
    zero = _run(scn, r, sp, (CAND,), tol=0.0)[0]
    scn.close()
    want = _truth_call(rays_mod, blob, r, sp, st, CAND, MIN, MAX, 0.05)
    _same(got, want, f"{scene}: edited state")
    gm = got[0][4]
    assert (got[0][:, (kind == 1) | (kind == 2)] == st[:, (kind == 1) | (kind == 2)]).all()
    assert (gm[kind == 3] > st[4, kind == 3]).all() and (gm[kind == 3] >= 2).all()
    assert (gm[kind == 4] == MAX).all() and np.isnan(got[0][6, kind == 4].view(np.float32)).all()
    # tol2 = 0 from a fresh state: a ray stops (at m = 2) exactly when its M2 are <= 0
    _same(zero, _truth(rays_mod, scene, VIEW[scene], True, tol=0.0)[0], f"{scene}: tol2 = 0")
    m2 = zero[0][5:8].view(np.float32)
    quiet = (m2 <= 0).all(axis=0)
    assert (zero[0][4][quiet] == 2).all() and (zero[0][4][~quiet] == MAX).all() and 0 < quiet.mean() < 1 and zero[2] == 0
    cols = _seq(rays_mod, scene, VIEW[scene], True)[0]
    assert (cols[quiet, 0] == cols[quiet, 1]).all(), "a quiet ray's first two samples are equal"
    missed = (cols == 0).all(axis=(1, 2))
    assert missed.any() and quiet[missed].all(), "the rays that miss everything stop at once"


@pytest.mark.gpu
def test_gpu_loop_until_nothing_is_open(qr, rays_mod):
    """step 3 candidates at a time until open == 0, at max 12: the number of calls, open after each and the final state are the
    fold's"""
    scene = "pt:test18_160_gf_aa4_pt"
    j = VIEW[scene]
    r, sp = _view_rays(rays_mod, scene, j)
    want = _truth(rays_mod, scene, j, True, (3, 3, 3, 3))
    calls = [k for k, w in enumerate(want) if w[2] == 0][0] + 1
    scn = qr.Scene(_base(scene), ray_queries=True)
    acc = _acc(scn, len(r), tol=TOL[scene])
    rt, st = _t(scn, r), _t(scn, sp)
    got = []
    while len(got) < 8:
        got.append(_step(acc, rt, 3, st))
        if got[-1][2] == 0:
            break
    scn.close()
    assert len(got) == calls and [g[2] for g in got] == [w[2] for w in want[:calls]]
    _same(got[-1], want[calls - 1], f"{scene}: after {calls} calls of 3")
    assert got[0][2] > 0


@pytest.mark.gpu
def test_gpu_checkpoint_and_the_scenes_own_mode(qr, rays_mod):
    """clone() after 5 candidates: original and copy, each continued by 7, are equal and the fold's; reset() starts over; a
    state that left the device and came back continues like the clone; and the bits are the same with the scene inside its own
    path-tracer mode, which the call neither needs nor touches"""
    import torch
    scene = "pt:test18_160_pt"
    j = VIEW[scene]
    r, sp = _view_rays(rays_mod, scene, j)
    scn = qr.Scene(_base(scene), ray_queries=True)
    rt, st = _t(scn, r), _t(scn, sp)
    acc = _acc(scn, len(r), tol=TOL[scene])
    five = _step(acc, rt, 5, st)
    cp = acc.clone()
    assert cp.state.data_ptr() != acc.state.data_ptr() and cp.tol2 == acc.tol2 and (cp.min_samples, cp.max_samples) == (MIN, MAX)
    back = scn.pt_adaptive(len(r), MIN, MAX, TOL[scene], state=torch.from_numpy(five[0].view(np.int32).copy()).to(acc.state.device))
    scn.set_pt(True)
    f = scn.new_frame()
    scn.render(f)
    a = _step(acc, rt, 7, st)
    scn.render(f)
    scn.set_pt(False)
    b = _step(cp, rt, 7, st)
    c = _step(back, rt, 7, st)
    acc.reset()
    assert (_host(acc.state).view(np.uint32) == _fresh(rays_mod, len(r))).all() and int(_host(acc.counts).sum()) == 0
    one = _step(acc, rt, 1, st)
    scn.close()
    want = _truth(rays_mod, scene, j, True, (5, 7))
    _same(five, want[0], f"{scene}: 5 candidates")
    _same(a, want[1], f"{scene}: 7 more inside the scene's path-tracer mode")
    _same(b, a, f"{scene}: the clone")
    _same(c, a, f"{scene}: a state restored from the host")
    _same(one, _truth(rays_mod, scene, j, True, (1,))[0], f"{scene}: after reset()")
    assert acc.tol2.dtype == np.float32 and acc.tol2 == np.float32(TOL[scene]) * np.float32(TOL[scene])


@pytest.mark.gpu
def test_gpu_depth_sweep(qr, rays_mod):
    """depths 0, 1, 3 and 10 on the second seeded view of test18"""
    scene = "pt:test18_160_pt"
    j = VIEW[scene]
    r, sp = _view_rays(rays_mod, scene, j)
    scn = qr.Scene(_base(scene), ray_queries=True)
    got = {}
    for depth in (0, 1, 3, 10):
        scn.set_depth(depth)
        got[depth] = _run(scn, r, sp, (CAND,), tol=TOL[scene])[0]
    scn.close()
    for depth, g in got.items():
        _same(g, _truth(rays_mod, scene, j, True, depth=depth)[0], f"{scene} depth {depth}")
    assert all((got[0][0][4] != got[d][0][4]).any() for d in (3, 10)), "the depth does not show in the counts"


@pytest.mark.gpu
def test_gpu_refusals(qr, rays_mod):
    """every refusal of the contract, each followed by a check that state, rgb and open are unchanged"""
    import torch
    scene = "pt:test18_160_pt"
    blob = _base(scene)
    r, sp = _view_rays(rays_mod, scene, VIEW[scene])
    n = 130
    r, sp = r[:n], sp[:n]
    L = qr.lib()
    dev = "cuda:0"
    SF, SI = 12345.0, 0x5A5A5A5A
    rt, st = torch.from_numpy(r.copy()).to(dev), torch.from_numpy(sp.copy()).to(dev)
    rgb = torch.full((n, 3), SF, dtype=torch.float32, device=dev)
    op = torch.full((2,), SI, dtype=torch.int32, device=dev)
    vp = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)

    plain = qr.Scene(blob)
    scn = qr.Scene(blob, ray_queries=True)
    acc = scn.pt_adaptive(n, MIN, MAX, 0.1)
    state = acc.state
    before = _host(state).copy()
    t2 = float(acc.tol2)

    def call(s, rays=vp(rt), spread=vp(st), n=n, state=vp(state), samples=1, mn=MIN, mx=MAX, tol2=t2, rgb=vp(rgb), open=vp(op), flags=0):
        return L.qr_pt_adapt_rays_async(s, rays, spread, n, state, samples, mn, mx, ctypes.c_float(tol2), rgb, open, flags, None)

    def refused(rc, want, text):
        assert rc == want and text in L.qr_last_error().decode(), (rc, L.qr_last_error().decode())
        torch.cuda.synchronize()
        assert bool((rgb == SF).all()) and bool((op == SI).all()) and (_host(state) == before).all(), "a refused call wrote something"

    refused(call(plain._h), UNSUP, "QR_UPLOAD_RAY_QUERIES")
    with pytest.raises(qr.QrError, match="QR_UPLOAD_RAY_QUERIES"):
        plain.pt_adaptive(n, MIN, MAX, 0.1).step(rt)
    plain.close()
    refused(call(None), ARG, "null scene")
    for kw in (dict(n=-1), dict(n=1 << 31), dict(n=1 << 40)):
        refused(call(scn._h, **kw), ARG, "ray count")
    for kw in (dict(flags=1), dict(flags=2), dict(flags=0x80000000)):
        refused(call(scn._h, **kw), ARG, "flags")
    for kw in (dict(rays=None), dict(state=None)):
        refused(call(scn._h, **kw), ARG, "null argument")
    for kw in (dict(rays=vp(rt, 4)), dict(rays=vp(rt, 8)), dict(spread=vp(st, 4)), dict(spread=vp(st, 8))):
        refused(call(scn._h, **kw), ARG, "16-byte aligned")
    for kw in (dict(state=vp(state, 2)), dict(rgb=vp(rgb, 1)), dict(rgb=vp(rgb, 2)), dict(open=vp(op, 1)), dict(open=vp(op, 2))):
        refused(call(scn._h, **kw), ARG, "4-byte aligned")
    for kw in (dict(samples=0), dict(samples=-1), dict(samples=513)):
        refused(call(scn._h, **kw), ARG, "samples must be")
    for kw in (dict(mn=-1), dict(mx=0, mn=0), dict(mx=-5, mn=-7), dict(mn=13), dict(mn=3, mx=2), dict(mx=1 << 24), dict(mx=0x7FFFFFFF, mn=0)):
        refused(call(scn._h, **kw), ARG, "min_samples and max_samples")
    for bad in (-1e-30, -1.0, float("nan"), float("inf"), float("-inf")):
        refused(call(scn._h, tol2=bad), ARG, "tol2")
    # the size query and the reset refuse the same counts
    nb = ctypes.c_uint64(7)
    assert L.qr_pt_adapt_state_bytes(scn._h, n, ctypes.byref(nb)) == 0 and nb.value == 8 * n * 4
    assert L.qr_pt_adapt_state_bytes(scn._h, -1, ctypes.byref(nb)) == ARG and nb.value == 8 * n * 4
    assert L.qr_pt_adapt_state_bytes(scn._h, 1 << 31, ctypes.byref(nb)) == ARG
    assert L.qr_pt_adapt_state_bytes(scn._h, n, None) == ARG and L.qr_pt_adapt_state_bytes(None, n, ctypes.byref(nb)) == ARG
    assert L.qr_pt_adapt_reset(scn._h, n, None) == ARG and L.qr_pt_adapt_reset(scn._h, -1, vp(state)) == ARG
    assert L.qr_pt_adapt_reset(scn._h, n, vp(state, 2)) == ARG and L.qr_pt_adapt_reset(None, n, vp(state)) == ARG
    assert L.qr_pt_adapt_reset(scn._h, 0, None) == 0
    # the empty call: no launch
    assert call(scn._h, n=0) == 0 and call(scn._h, n=0, rays=None, spread=None, state=None, rgb=None, open=None) == 0
    torch.cuda.synchronize()
    assert (rgb == SF).all() and (op == SI).all() and (_host(state) == before).all(), "a refused or empty call wrote something"
    # the accepted edges: min = 0, min = max, max = 2^24 - 1, tol2 = 0, no rgb, no open
    assert call(scn._h, mn=0, mx=(1 << 24) - 1, tol2=0.0, rgb=None, open=None) == 0
    torch.cuda.synchronize()
    assert (rgb == SF).all() and (op == SI).all() and (_host(state)[4] == 1).all()
    acc.reset()

    # the Python object
    good = state.clone()
    for bad in (good[:4], good[:, :n - 1], good.reshape(-1), good.float(), good.cpu(), good.cpu().numpy(), good[:, ::2]):
        with pytest.raises(qr.QrError, match="state must be"):
            scn.pt_adaptive(n, MIN, MAX, 0.1, state=bad)
    for badn in (-1, 1.5, None):
        with pytest.raises(qr.QrError, match="n must be"):
            scn.pt_adaptive(badn, MIN, MAX, 0.1)
    for mn, mx in ((-1, 4), (5, 4), (0, 0), (0, 1 << 24), (1.0, 4), (1, None)):
        with pytest.raises(qr.QrError, match="min_samples and max_samples"):
            scn.pt_adaptive(n, mn, mx, 0.1)
    for badt in (-0.1, float("nan"), float("inf"), 1e30, "x", None):
        with pytest.raises(qr.QrError, match="tol must be"):
            scn.pt_adaptive(n, MIN, MAX, badt)
    for bad in (rt.double(), rt[:, :7].contiguous(), rt.cpu(), rt.reshape(-1)):
        with pytest.raises(qr.QrError, match="rays must be"):
            acc.step(bad)
    with pytest.raises(qr.QrError, match="holds 130 rays"):
        acc.step(rt[:64])
    for bad in (st.double(), st[:64], st.cpu(), st[:, :4].contiguous(), sp):
        with pytest.raises(qr.QrError, match="spread must be"):
            acc.step(rt, spread=bad)
    for badc in (rgb[:1], rgb.double(), rgb.cpu()):
        with pytest.raises(qr.QrError, match="rgb must be"):
            acc.step(rt, rgb=badc)
    for bado in (op, op.float()[:1], op.cpu()[:1], 1):
        with pytest.raises(qr.QrError, match="open must be"):
            acc.step(rt, open=bado)
    for bads in (0, 513, -2, 1.5):
        with pytest.raises(qr.QrError, match="samples must be"):
            acc.step(rt, bads)
    torch.cuda.synchronize()
    assert (op == SI).all() and (_host(acc.state).view(np.uint32) == _fresh(rays_mod, n)).all()

    got = _step(acc, rt, 3, st)
    scn.close()
    _same(got, _truth_call(rays_mod, blob, r, sp, _fresh(rays_mod, n), 3, MIN, MAX, 0.1), f"{scene}: after the refusals")


@pytest.mark.gpu
def test_gpu_adversarial_rays(qr, oracle, rays_mod, tmp_path):
    """one adversarial ray family ("mixed": signed zeros, denormals, intervals at a hit's t, scaled directions, far origins,
    probes) on a fixture with emission patched on, and on the crowd scene with a grid over a flat list (crowd_flat_dda), at
    min 2, max 12, 12 candidates, with a seeded spread"""
    lit = 0
    for name, tol in (("demo01_160", TOL["patched:demo01_160"]), ("crowd_flat_dda", TOL["patched:demo01_160"])):
        plain = RS.scene_blob(name)
        blob = _ptpatch.pt_patch(plain)
        off, img = RS.query_image(qr, name, tmp_path)
        r = RS.family(plain, name, "mixed", oracle, RS.dda_grid(off, img), RS.reach_of(img))
        assert len(r) > 64
        sp = TPR._family_spread(name, "mixed", len(r))
        with RS.upload_env(name):
            scn = qr.Scene(blob, ray_queries=True)
        got = _run(scn, r, sp, (CAND,), tol=tol)[0]
        scn.close()
        want = _truth_call(rays_mod, blob, r, sp, _fresh(rays_mod, len(r)), CAND, MIN, MAX, tol)
        _same(got, want, f"{name}: family mixed")
        lit += int((want[1] != 0).any(axis=1).sum())
        print(f"{name}: {len(r)} rays, counts {np.bincount(want[0][4], minlength=MAX + 1).tolist()}")
    assert lit > 0, "no ray saw light"


# One case once more through the guarded diagnostic build (make guard: QR_STATS + QR_GUARD), as the other feature files do.  The
# library is chosen when the package is imported, hence the child process: this file run as a script.

def _guard_child():
    from qr_loader import load_package
    qr = load_package()
    assert qr.LIB_PATH == GUARD_LIB, qr.LIB_PATH
    rm = _rays_mod()
    scene, j = GUARD_CASE
    r, sp = _view_rays(rm, scene, j)
    scn = qr.Scene(_base(scene), ray_queries=True)
    got = _run(scn, r, sp, (CAND,), tol=TOL[scene])[0]
    bare = _run(scn, r, None, (CAND,), tol=TOL[scene])[0]
    scn.close()
    _same(got, _truth(rm, scene, j, True)[0], f"{scene}: guarded build")
    _same(bare, _truth(rm, scene, j, False)[0], f"{scene}: guarded build, no spread")
    print(f"{scene} guard_ok 1", flush=True)
    return 0


@pytest.mark.gpu
def test_gpu_guarded_build_gives_the_same_adaptive_rays():
    assert os.path.exists(GUARD_LIB), "libqrhip_guard.so is missing: build() makes it (make -C quadray-engine_amd/csrc guard)"
    env = dict(os.environ, QR_LIB=GUARD_LIB)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-child"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.count("guard_ok 1") == 1 and "QR_GUARD" not in out.stderr, out.stdout + out.stderr[-3000:]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.exit(_guard_child() if "--guard-child" in sys.argv else 2)
