"""Adaptive path-traced views (include/qrhip.h qr_pt_adapt_views_async, Scene.pt_adaptive_views): path-traced frames from caller
cameras with a sample count and Welford's M2 per pixel sample in an int32 [N, 8, slots] state the caller owns, and the adaptive
rays' stop rule evaluated on chip before every sample; and the host side of it in quadray-engine_amd/rays.py
(pt_adapt_view_counts, pt_adapt_view_frames; the fold is pt_adapt_fold on every state[j]).

Every comparison is bit for bit: all eight state planes, frames, mean, counts and open.  The truth is rays.pt_adapt_fold over
tests/ptaview_oracle.c (qrv_pt_samples): for the base snapshot rewritten to one view and size (_view_snapshot) and a generator
word per slot, the raw colour of each of a slot's consecutive samples and the generator word after each, read out of the
oracle's own sample() -- no mean, no count and no rule in it.  The CPU tests pin that translation unit to oracle.render_pt and
show that the inputs discriminate, before any GPU is involved.

Scenes, cameras and sizes: those of tests/test_pt_views.py; scene i of SCENES is run at SIZES[i % 3] (CASE), so that every size
meets a scene with and without FSAA.  Settings: min_samples 2, max_samples 12, 12 candidates, one tolerance per scene (TOL).
"""
import ctypes
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import _ptpatch
import _rayq
import _rayset as RS
import test_pt_adaptive as TPA
import test_pt_views as TPV
from conftest import ROOT
from test_pt_views import SCENES, SIZES, _base, _bits, _cams, _fsaa, _rays_mod
from test_render_views import _view_snapshot

ASM = TPV.ASM
GUARD_LIB = TPV.GUARD_LIB
ARG, UNSUP = -1, -3
MIN, MAX, CAND = 2, 12, 12
CASE = {s: SIZES[i % 3] for i, s in enumerate(SCENES)}
GUARD_CASE = "patched:demo02_160_gf_aa4"
# The tolerance on the standard error of the mean per scene, in linear colour units (tol2 = float32(tol) ** 2): fixed here after
# running test_inputs_discriminate, which prints what each value gives
TOL = {"pt:test18_160_pt": 0.07, "pt:test18_160_gf_aa4_pt": 0.07, "patched:demo01_160": 0.3, "patched:demo02_160_gf_aa4": 0.2,
       "patched:demo03_160": 0.07, "patched:test13_160_gf_aa4": 0.2}
_tol2 = TPA._tol2
_window = TPA._window


@pytest.fixture(scope="module")
def rays_mod():
    return _rays_mod()


def _ns(scene):
    return 1 << _fsaa(_base(scene))


def _lanes(w, h, fsaa):
    """per slot of a w x h frame: (footprint number, lane) as qr_pt_adapt_views_kernel places it -- footprints of 8x8, 8x4 or
    4x4 pixels, lane = (row in the footprint * its width + column) * samples per pixel + k"""
    ns = 1 << fsaa
    fw, fh = (4 if fsaa == 2 else 8), (8 if fsaa == 0 else 4)
    si = np.arange(w * h * ns)
    p, k = si // ns, si % ns
    x, y = p % w, p // w
    fcols = (w + fw - 1) // fw
    return (y // fh) * fcols + x // fw, ((y % fh) * fw + x % fw) * ns + k


# ------------------------------------------------------------------------------------------------- the truth (CPU)

_TU = None


def _tu():
    global _TU
    if _TU is None:
        import __graft_entry__ as g
        L = ctypes.CDLL(g.build_ptaview_oracle())
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.qrv_pt_samples.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_int64, ci, ci, ci, vp, vp]
        L.qrv_pt_samples.restype = ci
        _TU = L
    return _TU


def _samples(snap, rng_in, samples, depth=None):
    """qrv_pt_samples on a one-view snapshot: (cols float32 [slots, S, 3], rngs uint32 [slots, S]) from the words rng_in"""
    rin = np.ascontiguousarray(rng_in).view(np.uint32).copy()
    n = rin.shape[0]
    cols = np.zeros((n, samples, 3), dtype=np.float32)
    rngs = np.zeros((n, samples), dtype=np.uint32)
    buf = ctypes.create_string_buffer(snap, len(snap))
    rc = _tu().qrv_pt_samples(buf, len(snap), rin.ctypes.data, n, int(samples), -1 if depth is None else int(depth), 16,
                              cols.ctypes.data, rngs.ctypes.data)
    assert rc == 0, rc
    return cols, rngs


def _fresh(rm, nv, w, h, ns):
    """the state after a reset: plane 0 of every view = pt_seeds(w, h, ns), every other plane 0"""
    st = np.zeros((nv, 8, w * h * ns), dtype=np.uint32)
    st[:, 0] = rm.pt_seeds(w, h, ns)
    return st


_SEQ = {}


def _seq(rm, scene, j, w, h, depth=None):
    """the CAND candidate samples of every slot of seeded view j at w x h from a fresh state; computed once, read-only"""
    key = (scene, j, w, h, depth)
    if key not in _SEQ:
        snap = _view_snapshot(_base(scene), _cams(rm, scene)[j], w, h)
        cols, rngs = _samples(snap, rm.pt_seeds(w, h, _ns(scene)), CAND, depth)
        cols.setflags(write=False); rngs.setflags(write=False)
        _SEQ[key] = (cols, rngs)
    return _SEQ[key]


def _outputs(rm, blob, st, w, h, op):
    """(state, frames, mean, counts, open) of a state: the numpy specification of the call's outputs"""
    fsaa = _fsaa(blob)
    f, m = rm.pt_adapt_view_frames(st, blob, w, h)
    return st, f, m, rm.pt_adapt_view_counts(st, 1 << fsaa).reshape(st.shape[0], h, w), op


def _truth(rm, scene, js, w, h, splits=(CAND,), mn=MIN, mx=MAX, tol=None, depth=None, tol2=None):
    """[(state [N, 8, slots], frames, mean, counts, open) after every call] of the fold for the seeded views js from a fresh state"""
    t2 = _tol2(TOL[scene] if tol is None else tol) if tol2 is None else np.float32(tol2)
    st = _fresh(rm, len(js), w, h, _ns(scene))
    out = []
    for s in splits:
        op = 0
        for i, j in enumerate(js):
            seq = _seq(rm, scene, j, w, h, depth)
            c, g = _window(seq, st[i], s)
            st[i], _, o = rm.pt_adapt_fold(st[i], c, g, mn, mx, t2)
            op += o
        out.append(_outputs(rm, _base(scene), st.copy(), w, h, op))
    return out


def _truth_call(rm, blob, views, w, h, state, samples, mn, mx, tol, depth=None):
    """(state', frames, mean, counts, open) of one call on any state: the fold over the samples from the state's generator words"""
    st = np.ascontiguousarray(state).view(np.uint32).copy()
    op = 0
    for i, v in enumerate(views):
        c, g = _samples(_view_snapshot(blob, v, w, h), st[i, 0], samples, depth)
        st[i], _, o = rm.pt_adapt_fold(st[i], c, g, mn, mx, _tol2(tol))
        op += o
    return _outputs(rm, blob, st, w, h, op)


# ---------------------------------------------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("scene", ["pt:test18_160_pt", "pt:test18_160_gf_aa4_pt", "patched:demo02_160_gf_aa4"])
def test_tu_is_the_oracles_path_tracer(oracle, rays_mod, scene):
    """min = max = n from pt_seeds, n = 1, 2, 5: the fold over qrv_pt_samples, clamped, reduced and packed by
    pt_adapt_view_frames, is oracle.render_pt(snapshot, n, order="kernel") -- frame and mean -- for the snapshot's own camera
    and one seeded camera at 67 x 45"""
    rm, base = rays_mod, _base(scene)
    w, h, ns = 67, 45, _ns(scene)
    lit = 0
    for what, v in (("own camera", rm.view_of(base)), ("seeded camera 1", _cams(rm, scene)[1])):
        snap = _view_snapshot(base, v, w, h)
        cols, rngs = _samples(snap, rm.pt_seeds(w, h, ns), 5)
        lit += int((cols != 0).any(axis=(1, 2)).sum())
        for n in (1, 2, 5):
            st = _fresh(rm, 1, w, h, ns)
            st[0], _, op = rm.pt_adapt_fold(st[0], cols[:, :n], rngs[:, :n], n, n, _tol2(0.5))
            f, m = rm.pt_adapt_view_frames(st, base, w, h)
            wf, wm = oracle.render_pt(snap, n, order="kernel", threads=16, want_mean=True)
            nf, nm = int((f[0] != wf).sum()), int((_bits(m[0]) != _bits(wm)).any(axis=2).sum())
            assert nf == 0 and nm == 0, f"{scene} {what}, {n} samples: {nf} pixels of the frame differ, {nm} of the mean"
            assert op == 0 and (st[0, 4] == n).all()
            assert (rm.pt_adapt_view_counts(st, ns) == n * ns).all()
    assert lit > 0, "no slot of either camera saw light"


def _rows(rm, scene, tol):
    """per seeded view at 64 x 64: fraction of slots stopped before MAX, fraction at MAX, distinct counts, footprints with every
    slot stopped early, footprints with both kinds, open, pixels whose heat differs from spp * MAX"""
    w, h = 64, 64
    ns = _ns(scene)
    fp, _ = _lanes(w, h, _fsaa(_base(scene)))
    rows = []
    for j in range(4):
        st, _, _, counts, op = _truth(rm, scene, [j], w, h, tol=tol)[0]
        m = st[0, 4]
        early = m < MAX
        n_early = np.bincount(fp, weights=early, minlength=fp.max() + 1)
        assert (np.bincount(fp) == 64).all()
        rows.append((float(early.mean()), float((m == MAX).mean()), len(np.unique(m)), int((n_early == 64).sum()),
                     int(((n_early > 0) & (n_early < 64)).sum()), op, int((counts != ns * MAX).sum())))
    return rows


@pytest.mark.parametrize("scene", SCENES)
def test_inputs_discriminate(rays_mod, scene):
    """A condition on the test inputs, checked with the truth alone, at 64 x 64, min 2, max 12, 12 candidates and the scene's TOL:
      - at least one seeded view has >= 15 % of the slots stopped before max and >= 15 % at max;
      - the counts of some view take >= 4 distinct values;
      - some footprint has every slot stopped early (the early wave exit) and some footprint has both kinds of slot;
      - tol2 doubled changes plane 4 on >= 5 % of that view's slots;
      - the heat map differs from spp * max somewhere.
    All six scenes meet this form as it stands; pt:test18_160_gf_aa4_pt meets it with its view 1 alone, as its ray twin
    (tests/test_pt_adaptive.py) documents: views 2 and 3 see no light and view 0's slots mostly stop at m = 2."""
    rows = _rows(rays_mod, scene, TOL[scene])
    print(f"{scene} tol {TOL[scene]}: early % / at max % / distinct counts / footprints all early / mixed / open / pixels off full heat, "
          "per view: " + "; ".join(f"{100 * e:.1f} {100 * f:.1f} {d} {a} {b} {o} {p}" for e, f, d, a, b, o, p in rows))
    ok = [e >= 0.15 and f >= 0.15 for e, f, *_ in rows]
    assert sum(ok) >= 1, rows
    assert max(r[2] for r in rows) >= 4, rows
    assert sum(r[3] for r in rows) >= 1 and sum(r[4] for r in rows) >= 1, rows
    assert all(r[5] == 0 for r in rows), "after 12 candidates at max 12 nothing is open"
    assert sum(r[6] for r in rows) >= 1, rows
    j = ok.index(True)
    a = _truth(rays_mod, scene, [j], 64, 64)[0][0]
    b = _truth(rays_mod, scene, [j], 64, 64, tol2=np.float32(2) * _tol2(TOL[scene]))[0][0]
    moved = float((a[0, 4] != b[0, 4]).mean())
    print(f"{scene} view {j}: tol2 doubled changes the count of {100 * moved:.1f} % of the slots")
    assert moved >= 0.05


def test_abi_and_constants(qr):
    """the library exports the three entry points, the header declares them, and its constants are the module's"""
    L = qr.lib()
    with open(os.path.join(ROOT, "include", "qrhip.h")) as f:
        hdr = f.read()
    for sym in ("qr_pt_adapt_views_state_bytes", "qr_pt_adapt_views_reset", "qr_pt_adapt_views_async"):
        assert hasattr(L, sym), sym
        assert sym in qr.ABI_SYMBOLS and f"int {sym}(" in hdr, sym
    assert f"#define QR_PT_ADAPT_VIEWS_MAX_SAMPLES {qr.PT_ADAPT_VIEWS_MAX_SAMPLES} " in hdr and qr.PT_ADAPT_VIEWS_MAX_SAMPLES == 512
    assert "uint32_t *frames_dev, float *mean_dev, int32_t *counts_dev, uint32_t *open_dev," in hdr
    assert hasattr(qr.Scene, "pt_adaptive_views") and hasattr(qr, "PtAdaptiveViews")
    for m in ("step", "reset", "clone", "open_list"):
        assert callable(getattr(qr.PtAdaptiveViews, m))
    assert isinstance(qr.PtAdaptiveViews.counts, property)
    rm = _rays_mod()
    assert callable(rm.pt_adapt_view_counts) and callable(rm.pt_adapt_view_frames)


def test_state_bytes_without_a_scene(qr):
    """the size query refuses a null scene and a null result, and leaves the caller's word alone (the sizes themselves need a
    resident scene: test_gpu_refusals)"""
    L = qr.lib()
    nb = ctypes.c_uint64(7)
    assert L.qr_pt_adapt_views_state_bytes(None, 2, 64, 64, ctypes.byref(nb)) == ARG and nb.value == 7
    assert "null scene" in L.qr_last_error().decode()
    assert L.qr_pt_adapt_views_reset(None, 2, 64, 64, None) == ARG


def test_kernel_in_resource_check():
    """the build's register check lists the kernel once, at the path-traced kernels' budget (168 VGPRs, nothing spilled, 2128 B
    of private segment), and the built assembly passes it"""
    import importlib.util
    path = os.path.join(ROOT, "tools", "check_kernel_resources.py")
    spec = importlib.util.spec_from_file_location("check_kernel_resources", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    frags = [f for f in m.LIMITS if "qr_pt_adapt_views_kernel" in f]
    assert frags == ["24qr_pt_adapt_views_kernel"]
    assert m.LIMITS[frags[0]] == (168, 0, 2128) == m.LIMITS["18qr_pt_adapt_kernel"]
    r = subprocess.run([sys.executable, path, ASM, "--print"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("qr_pt_adapt_views_kernel") == 1
    assert r.stdout.count("qr_pt_adapt_kernel") == 1 and r.stdout.count("qr_pt_views_kernel") == 1


def test_counts_and_frames_on_a_constructed_state(rays_mod):
    """pt_adapt_view_counts sums plane 4 over a pixel's slots; pt_adapt_view_frames is pack_colors (the frame's output step) on
    planes 1..3 -- clamp1 of values above 1 and of NaN, the 4x reduce, gamma, pack -- and its mean the reduce alone"""
    rm = rays_mod
    base = _base("pt:test18_160_gf_aa4_pt")
    w, h, ns = 3, 2, 4
    snap = _view_snapshot(base, rm.view_of(base), w, h)
    rng = np.random.default_rng(3)
    st = np.zeros((2, 8, w * h * ns), dtype=np.uint32)
    col = rng.uniform(0.0, 1.4, (2, 3, w * h * ns)).astype(np.float32)
    col[1, 2, 5] = np.nan
    col[0, 0, 0] = 0.0
    st[:, 1:4] = col.view(np.uint32)
    st[:, 4] = rng.integers(0, 40, (2, w * h * ns))
    st[1, 4, 7] = 0x00FFFFFF
    counts = rm.pt_adapt_view_counts(st, ns)
    assert counts.dtype == np.int32 and counts.shape == (2, w * h)
    assert (counts == st[:, 4].reshape(2, w * h, ns).astype(np.int64).sum(axis=2)).all()
    assert (rm.pt_adapt_view_counts(st[1], ns) == counts[1:2]).all() and (rm.pt_adapt_view_counts(st.view(np.int32), 1) == st[:, 4]).all()
    f, m = rm.pt_adapt_view_frames(st, base, w, h)
    assert f.dtype == np.uint32 and f.shape == (2, h, w) and m.dtype == np.float32 and m.shape == (2, h, w, 3)
    for j in range(2):
        rgb = np.ascontiguousarray(col[j].T.reshape(w * h, ns, 3).transpose(1, 0, 2))
        assert (f[j] == rm.pack_colors(rgb, snap)).all()
        assert (_bits(m[j].reshape(-1, 3)) == _bits(rm.reduce_colors(rgb, base))).all()
    assert (m <= 1.0).all() and m[1].reshape(-1, 3)[1, 2] > 0.25, "a NaN sample counts as 1 after clamp1"
    with pytest.raises(ValueError):
        rm.pt_adapt_view_frames(st, base, w + 1, h)
    with pytest.raises(ValueError):
        rm.pt_adapt_view_counts(st, 5)
    with pytest.raises(ValueError):
        rm.pt_adapt_view_counts(st[:, :4], ns)


# ---------------------------------------------------------------------------------------------------------------- GPU

_vt = TPV._vt


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def _dev_state(scn, st):
    import torch
    return torch.from_numpy(np.ascontiguousarray(st).view(np.int32).copy()).to(f"cuda:{scn.device}")


def _acc(scn, views, w, h, mn=MIN, mx=MAX, tol=None, state=None):
    return scn.pt_adaptive_views(_vt(scn, views), w, h, min_samples=mn, max_samples=mx, tol=tol,
                                 state=None if state is None else _dev_state(scn, state))


def _step(acc, samples):
    """one step with every output: (state uint32 [N, 8, slots], frames, mean, counts, open) on the host"""
    f, m, c, op = acc.step(samples, mean=True, counts=True, open=True)
    return (_host(acc.state).view(np.uint32), _host(f).view(np.uint32), _host(m), _host(c), int(_host(op).view(np.uint32)[0]))


def _run(scn, views, w, h, splits, mn=MIN, mx=MAX, tol=None, state=None):
    acc = _acc(scn, views, w, h, mn, mx, tol, state)
    return [_step(acc, s) for s in splits]


def _same(got, want, what):
    (gst, gf, gm, gc, gop), (wst, wf, wm, wc, wop) = got, want
    gst, wst = gst.view(np.uint32), np.ascontiguousarray(wst).view(np.uint32)
    assert gst.shape == wst.shape and gf.shape == wf.shape and gm.shape == wm.shape and gc.shape == wc.shape, what
    assert gm.dtype == np.float32 and gc.dtype == np.int32
    bad = [int((gst[:, p] != wst[:, p]).sum()) for p in range(8)]
    nf, nm, nc = int((gf != wf).sum()), int((_bits(gm) != _bits(wm)).any(axis=-1).sum()), int((gc != wc).sum())
    assert not any(bad) and nf == 0 and nm == 0 and nc == 0 and gop == wop, \
        (f"{what}: of {gst.shape[0]} x {gst.shape[2]} slots, per plane {bad} state words differ; {nf} pixels of the frames, {nm} of "
         f"the means, {nc} of the counts differ; open {gop}, want {wop}")


@pytest.mark.gpu
@pytest.mark.parametrize("scene", SCENES)
def test_gpu_views_equal_the_fold(qr, rays_mod, scene):
    """the four seeded views in one launch at the scene's size (CASE): all eight planes, frames, mean, counts and open are the
    fold's over the oracle's samples after EVERY call of 12 = 5 + 7 = 12 x 1 = 3 + 3 + 3 + 3"""
    w, h = CASE[scene]
    views = _cams(rays_mod, scene)
    splits = [(12,), (5, 7), (1,) * 12, (3, 3, 3, 3)]
    scn = qr.Scene(_base(scene), ray_queries=True)
    got = [_run(scn, views, w, h, s, tol=TOL[scene]) for s in splits]
    scn.close()
    for s, g in zip(splits, got):
        want = _truth(rays_mod, scene, [0, 1, 2, 3], w, h, s)
        for k in range(len(s)):
            _same(g[k], want[k], f"{scene} {w}x{h}: split {s}, call {k}")
        _same(g[-1], got[0][0], f"{scene} {w}x{h}: split {s} against 12 in one call")
    assert got[2][0][4] == 4 * w * h * _ns(scene) and got[0][0][4] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["patched:demo03_160", "pt:test18_160_gf_aa4_pt", "patched:demo02_160_gf_aa4"])
def test_gpu_min_equals_max_is_pt_views(qr, rays_mod, scene):
    """min = max = 5 (in 2 + 3, and 9 candidates in one call): planes 0..3, frames and mean are Scene.pt_views' on the same GPU
    after 5 samples, plane 4 is 5, counts 5 * spp and open 0; without FSAA and with 4x"""
    w, h = 67, 45
    views = _cams(rays_mod, scene)
    scn = qr.Scene(_base(scene), ray_queries=True)
    a = _run(scn, views, w, h, (2, 3), mn=5, mx=5, tol=TOL[scene])
    more = _run(scn, views, w, h, (9,), mn=5, mx=5, tol=0.0)[0]
    pv = scn.pt_views(_vt(scn, views), w, h)
    pf, pm = TPV._step(pv, 5)
    pst = TPV._state(pv).view(np.uint32)
    scn.close()
    st, f, m, c, op = a[1]
    assert (st[:, :4] == pst).all(), f"{scene}: {int((st[:, :4] != pst).any(axis=1).sum())} slots differ from pt_views"
    assert (f == pf).all() and (_bits(m) == _bits(pm)).all()
    assert (st[:, 4] == 5).all() and (c == 5 * _ns(scene)).all() and op == 0 and a[0][4] == st.shape[0] * st.shape[2]
    assert (st[:, 5:8] != 0).any() and (f != 0).any()
    _same(more, a[1], f"{scene}: 9 candidates at max 5")


@pytest.mark.gpu
@pytest.mark.parametrize("scene,j", [("pt:test18_160_gf_aa4_pt", 1), ("patched:demo01_160", 0)])
def test_gpu_a_slot_depends_on_its_own_column_alone(qr, rays_mod, scene, j):
    """Consequence (c) at 67 x 45 (partial footprints on both edges).  From a fresh state edited by the host so that every second
    slot -- and in a second run every slot but one per footprint -- holds m = max: the untouched slots end bit-identical to the
    unedited run, the closed slots keep all eight words, and every pixel of frames, mean and counts is still written
    (sentinel-filled outputs) with what the final state says.  The same view alone and as view 2 of 3 gives the same block."""
    import torch
    rm = rays_mod
    w, h = 67, 45
    fsaa, ns = _fsaa(_base(scene)), _ns(scene)
    cams = _cams(rm, scene)
    fp, lane = _lanes(w, h, fsaa)
    slots = w * h * ns
    every_second = (np.arange(slots) % 2) == 1
    one_per_fp = lane != (fp * 7 + 3) % 64
    # closed masks: True = the slot is closed.  A partial footprint whose chosen lane lies outside the frame is closed entirely
    scn = qr.Scene(_base(scene), ray_queries=True)
    dev = f"cuda:{scn.device}"
    plain = _run(scn, [cams[j]], w, h, (CAND,), tol=TOL[scene])[0]
    runs = []
    SI, SF = 0x5A5A5A5A, 12345.0
    for closed in (every_second, one_per_fp):
        st0 = _fresh(rm, 1, w, h, ns)
        st0[0, 4, closed] = MAX
        st0[0, 5:8, closed] = np.array([7.0], dtype=np.float32).view(np.uint32)[0]
        acc = _acc(scn, [cams[j]], w, h, tol=TOL[scene], state=st0)
        fr = torch.full((1, h, w), SI, dtype=torch.int32, device=dev)
        mn = torch.full((1, h, w, 3), SF, dtype=torch.float32, device=dev)
        cn = torch.full((1, h, w), -7, dtype=torch.int32, device=dev)
        _, _, _, op = acc.step(CAND, frames=fr, mean=mn, counts=cn, open=True)
        runs.append((closed, st0, (_host(acc.state).view(np.uint32), _host(fr).view(np.uint32), _host(mn), _host(cn),
                                   int(_host(op)[0]))))
    three = _run(scn, [cams[(j + 1) % 4], cams[(j + 2) % 4], cams[j]], w, h, (CAND,), tol=TOL[scene])[0]
    scn.close()
    assert 0 < (plain[0][0, 4] < MAX).mean() < 1 and (plain[0][0, 4] >= MIN).all()
    for closed, st0, got in runs:
        st = got[0]
        assert 0 < (~closed).sum() < slots
        assert (st[0][:, ~closed] == plain[0][0][:, ~closed]).all(), \
            f"{scene}: {int((st[0][:, ~closed] != plain[0][0][:, ~closed]).any(axis=0).sum())} open slots differ from the unedited run"
        assert (st[0][:, closed] == st0[0][:, closed]).all(), f"{scene}: a closed slot changed"
        _same(got, _outputs(rm, _base(scene), st, w, h, 0), f"{scene}: outputs of the edited run against its final state")
        assert (got[1] != SI).all() and (got[2] != SF).all() and (got[3] != -7).all(), f"{scene}: a pixel was not written"
    assert (three[0][2] == plain[0][0]).all(), f"{scene}: view {j} as view 2 of 3 differs from the view alone"
    assert (three[1][2] == plain[1][0]).all() and (_bits(three[2][2]) == _bits(plain[2][0])).all() and (three[3][2] == plain[3][0]).all()
    assert (three[0][0] != three[0][2]).any()


@pytest.mark.gpu
def test_gpu_all_slots_closed(qr, rays_mod):
    """a state in which every slot holds m >= max: the launch changes no state word, writes every output pixel with what the
    state says, and adds nothing to open (a preset word keeps its value)"""
    import torch
    rm = rays_mod
    scene, (w, h) = "patched:demo02_160_gf_aa4", (67, 45)
    ns = _ns(scene)
    views = _cams(rm, scene)[:2]
    st0 = _truth(rm, GUARD_CASE, [0, 1], 64, 64, (5,))[0][0][:, :, :w * h * ns].copy()     # any plausible means and M2
    st0[:, 4] = MAX
    st0[1, 4, ::3] = MAX + 5
    scn = qr.Scene(_base(scene), ray_queries=True)
    dev = f"cuda:{scn.device}"
    acc = _acc(scn, views, w, h, tol=TOL[scene], state=st0)
    SI, SF = 0x5A5A5A5A, 12345.0
    fr = torch.full((2, h, w), SI, dtype=torch.int32, device=dev)
    mn = torch.full((2, h, w, 3), SF, dtype=torch.float32, device=dev)
    cn = torch.full((2, h, w), -7, dtype=torch.int32, device=dev)
    op = torch.full((3,), 77, dtype=torch.int32, device=dev)
    vp = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)
    rc = qr.lib().qr_pt_adapt_views_async(scn._h, vp(acc.views), 2, w, h, vp(acc.state), 7, MIN, MAX, ctypes.c_float(float(acc.tol2)),
                                          vp(fr), vp(mn), vp(cn), vp(op, 4), 0, None)
    got = (_host(acc.state).view(np.uint32), _host(fr).view(np.uint32), _host(mn), _host(cn), 0)
    opw = _host(op).tolist()
    scn.close()
    assert rc == 0 and opw == [77, 77, 77]
    assert (got[0] == st0).all(), "a closed state changed"
    _same(got, _outputs(rm, _base(scene), st0, w, h, 0), f"{scene}: all slots closed")
    assert (got[1] != SI).all() and (got[2] != SF).all() and (got[3] != -7).all()


@pytest.mark.gpu
def test_gpu_loop_and_open_lists(qr, rays_mod):
    """3 candidates per call until open == 0: open after each call and the final state are the fold's; after the first (partial)
    call open_list(view) is np.flatnonzero(rays.pt_adapt_open(state[view])) for every view -- consequence (d) -- and after the
    last its count is 0 for every view"""
    rm = rays_mod
    scene = "patched:demo02_160_gf_aa4"
    w, h = CASE[scene]
    views = _cams(rm, scene)
    want = _truth(rm, scene, [0, 1, 2, 3], w, h, (3, 3, 3, 3))
    calls = [k for k, x in enumerate(want) if x[4] == 0][0] + 1
    t2 = _tol2(TOL[scene])
    scn = qr.Scene(_base(scene), ray_queries=True)
    acc = _acc(scn, views, w, h, tol=TOL[scene])
    got, lists = [], []
    while len(got) < 8:
        got.append(_step(acc, 3))
        if len(got) == 1 or got[-1][4] == 0:
            for v in range(4):
                idx, cnt = acc.open_list(v)
                n = int(_host(cnt)[0])
                lists.append((len(got), v, n, _host(idx)[:n].view(np.uint32)))
        if got[-1][4] == 0:
            break
    scn.close()
    assert len(got) == calls and [g[4] for g in got] == [x[4] for x in want[:calls]] and got[0][4] > 0
    _same(got[-1], want[calls - 1], f"{scene}: after {calls} calls of 3")
    assert len(lists) == 8
    for call, v, n, idx in lists:
        st = got[call - 1][0][v]
        ref = np.flatnonzero(rm.pt_adapt_open(st, MIN, MAX, t2))
        assert n == len(ref) and (idx == ref).all(), f"{scene}: open list of view {v} after call {call}"
    assert sum(n for call, _, n, _ in lists if call == 1) == got[0][4] > 0
    assert all(n == 0 for call, _, n, _ in lists if call == calls)


@pytest.mark.gpu
def test_gpu_edited_state(qr, rays_mod):
    """a state edited by the host: slots with m >= max (far above it too, unsigned) take nothing, slots with m = 0, 1 always
    take, a NaN in an M2 plane never converges and runs to max, a negative M2 is below every limit; and tol2 = 0 stops exactly
    the slots whose three M2 are <= 0"""
    rm = rays_mod
    scene = "patched:demo01_160"
    w, h = CASE[scene]
    blob = _base(scene)
    views = _cams(rm, scene)[:2]
    f32 = lambda v: np.array([v], dtype=np.float32).view(np.uint32)[0]
    st = _truth(rm, scene, [0, 1], w, h, (4,), tol=0.05)[0][0].copy()
    rng = np.random.default_rng(5)
    kind = rng.integers(0, 6, st.shape[2])
    st[:, 4, kind == 1] = MAX
    st[:, 4, kind == 2] = 0xFFFFFF00
    st[:, 4, kind == 3] = rng.integers(0, 2, int((kind == 3).sum()))
    st[:, 5:8, kind == 3] = 0
    st[:, 6, kind == 4] = f32(np.nan)
    st[:, 5:8, kind == 5] = f32(-1.0)
    scn = qr.Scene(blob, ray_queries=True)
    got = _run(scn, views, w, h, (CAND,), tol=0.05, state=st)[0]
    zero = _run(scn, views, w, h, (CAND,), tol=0.0)[0]
    scn.close()
    _same(got, _truth_call(rm, blob, views, w, h, st, CAND, MIN, MAX, 0.05), f"{scene}: edited state")
    gm = got[0][:, 4]
    shut = (kind == 1) | (kind == 2)
    assert (got[0][:, :, shut] == st[:, :, shut]).all()
    assert (gm[:, kind == 3] > st[:, 4, kind == 3]).all() and (gm[:, kind == 3] >= 2).all()
    assert (gm[:, kind == 4] == MAX).all() and np.isnan(got[0][:, 6, kind == 4].view(np.float32)).all()
    _same(zero, _truth(rm, scene, [0, 1], w, h, tol=0.0)[0], f"{scene}: tol2 = 0")
    quiet = (zero[0][:, 5:8].view(np.float32) <= 0).all(axis=1)
    assert (zero[0][:, 4][quiet] == 2).all() and (zero[0][:, 4][~quiet] == MAX).all() and 0 < quiet.mean() < 1 and zero[4] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["pt:test18_160_gf_aa4_pt", "patched:demo01_160"])
def test_gpu_bounds(qr, rays_mod, scene):
    """frame sizes whose last footprints are partial in both directions; state, frames, mean, counts and open carved out of
    larger sentinel-filled buffers: the fold's bits, and reset and launch leave the tails alone"""
    import torch
    rm = rays_mod
    w, h = CASE[scene]
    assert (w, h) != (64, 64)
    ns = _ns(scene)
    views = _cams(rm, scene)
    scn = qr.Scene(_base(scene), ray_queries=True)
    dev = f"cuda:{scn.device}"
    TAIL, SI, SF = 4096, 0x5A5A5A5A, 12345.0
    n_st, n_px = 4 * 8 * w * h * ns, 4 * w * h
    stb = torch.full((n_st + TAIL,), SI, dtype=torch.int32, device=dev)
    frb = torch.full((n_px + TAIL,), SI, dtype=torch.int32, device=dev)
    mnb = torch.full((3 * n_px + TAIL,), SF, dtype=torch.float32, device=dev)
    cnb = torch.full((n_px + TAIL,), SI, dtype=torch.int32, device=dev)
    opb = torch.full((4,), SI, dtype=torch.int32, device=dev)
    acc = scn.pt_adaptive_views(_vt(scn, views), w, h, min_samples=MIN, max_samples=MAX, tol=TOL[scene],
                                state=stb[:n_st].view(4, 8, w * h * ns))
    acc.reset()
    torch.cuda.synchronize()
    assert (stb[n_st:] == SI).all(), "reset wrote past the state"
    assert (_host(acc.state).view(np.uint32) == _fresh(rm, 4, w, h, ns)).all()
    f, m, c, op = acc.step(5, frames=frb[:n_px].view(4, h, w), mean=mnb[:3 * n_px].view(4, h, w, 3), counts=cnb[:n_px].view(4, h, w),
                           open=opb[1:2])
    assert f.data_ptr() == frb.data_ptr() and m.data_ptr() == mnb.data_ptr() and c.data_ptr() == cnb.data_ptr()
    got = (_host(acc.state).view(np.uint32), _host(f).view(np.uint32), _host(m), _host(c), int(_host(opb)[1]))
    only = acc.clone().step(1)
    tails_ok = bool((stb[n_st:] == SI).all()) and bool((frb[n_px:] == SI).all()) and bool((mnb[3 * n_px:] == SF).all()) \
        and bool((cnb[n_px:] == SI).all())
    op_ok = _host(opb)[[0, 2, 3]].tolist() == [SI] * 3
    counts = _host(acc.counts)
    scn.close()
    assert tuple(only.shape) == (4, h, w) and tails_ok and op_ok, f"{scene} {w}x{h}: a tail was written"
    want = _truth(rm, scene, [0, 1, 2, 3], w, h, (5,))[0]
    _same(got, want, f"{scene} {w}x{h}: into sentinel-tailed buffers")
    assert counts.shape == (4, w * h * ns) and (counts.view(np.uint32) == want[0][:, 4]).all()


@pytest.mark.gpu
def test_gpu_checkpoint_and_the_scenes_own_mode(qr, rays_mod):
    """clone() after 5 candidates: original and copy, each continued by 7, are equal and the fold's; reset() starts over; a
    state that left the device and came back continues like the clone; and the bits are the same with the scene inside its own
    path-tracer mode, which the call neither needs nor touches"""
    rm = rays_mod
    scene = "pt:test18_160_pt"
    w, h = CASE[scene]
    views = _cams(rm, scene)
    scn = qr.Scene(_base(scene), ray_queries=True)
    acc = _acc(scn, views, w, h, tol=TOL[scene])
    five = _step(acc, 5)
    cp = acc.clone()
    assert cp.state.data_ptr() != acc.state.data_ptr() and cp.tol2 == acc.tol2 and (cp.min_samples, cp.max_samples) == (MIN, MAX)
    back = _acc(scn, views, w, h, tol=TOL[scene], state=five[0])
    scn.set_pt(True)
    f = scn.new_frame()
    scn.render(f)
    a = _step(acc, 7)
    scn.render(f)
    scn.set_pt(False)
    b = _step(cp, 7)
    c = _step(back, 7)
    acc.reset()
    assert (_host(acc.state).view(np.uint32) == _fresh(rm, 4, w, h, 1)).all() and int(_host(acc.counts).sum()) == 0
    one = _step(acc, 1)
    scn.close()
    want = _truth(rm, scene, [0, 1, 2, 3], w, h, (5, 7))
    _same(five, want[0], f"{scene}: 5 candidates")
    _same(a, want[1], f"{scene}: 7 more inside the scene's path-tracer mode")
    _same(b, a, f"{scene}: the clone")
    _same(c, a, f"{scene}: a state restored from the host")
    _same(one, _truth(rm, scene, [0, 1, 2, 3], w, h, (1,))[0], f"{scene}: after reset()")
    assert acc.tol2.dtype == np.float32 and acc.tol2 == np.float32(TOL[scene]) * np.float32(TOL[scene])


@pytest.mark.gpu
def test_gpu_depth_sweep(qr, rays_mod):
    """depths 0, 1, 3 and 10 on the second seeded view of test18"""
    rm = rays_mod
    scene = "pt:test18_160_pt"
    w, h = CASE[scene]
    v = _cams(rm, scene)[1]
    scn = qr.Scene(_base(scene), ray_queries=True)
    got = {}
    for depth in (0, 1, 3, 10):
        scn.set_depth(depth)
        got[depth] = _run(scn, [v], w, h, (CAND,), tol=TOL[scene])[0]
    scn.close()
    for depth, g in got.items():
        _same(g, _truth(rm, scene, [1], w, h, depth=depth)[0], f"{scene} depth {depth}")
    assert all((got[0][0][0, 4] != got[d][0][0, 4]).any() for d in (3, 10)), "the depth does not show in the counts"


@pytest.mark.gpu
def test_gpu_crowd_scene(qr, rays_mod):
    """the crowd scene with a grid over a flat list (tests/_rayset.py crowd_flat_dda), emission patched on: two seeded views"""
    rm = rays_mod
    name, (w, h), tol = "crowd_flat_dda", (64, 64), TOL["patched:demo01_160"]
    blob = _ptpatch.pt_patch(RS.scene_blob(name))
    views = [rm.view_of(c) for c in _rayq.random_cameras(blob, seed=zlib.crc32(name.encode()), n=2)]
    with RS.upload_env(name):
        scn = qr.Scene(blob, ray_queries=True)
    got = _run(scn, views, w, h, (CAND,), tol=tol)[0]
    scn.close()
    want = _truth_call(rm, blob, views, w, h, _fresh(rm, 2, w, h, 1 << _fsaa(blob)), CAND, MIN, MAX, tol)
    _same(got, want, name)
    print(f"{name}: counts {np.bincount(want[0][:, 4].reshape(-1), minlength=MAX + 1).tolist()}")
    assert (want[2] != 0).any(), "no slot saw light"


@pytest.mark.gpu
def test_gpu_refusals(qr, rays_mod):
    """every refusal of the contract, each followed by a check that state, frames, mean, counts and open are unchanged"""
    import torch
    rm = rays_mod
    scene, (w, h) = "pt:test18_160_pt", (67, 45)
    blob = _base(scene)
    assert _fsaa(blob) == 0
    views = _cams(rm, scene)[:2]
    L = qr.lib()
    dev = "cuda:0"
    vt = torch.from_numpy(np.stack(views)).to(dev)
    SI, SF = 0x5A5A5A5A, 12345.0
    fr = torch.full((2, h, w), SI, dtype=torch.int32, device=dev)
    mn = torch.full((2, h, w, 3), SF, dtype=torch.float32, device=dev)
    cn = torch.full((2, h, w), SI, dtype=torch.int32, device=dev)
    op = torch.full((2,), SI, dtype=torch.int32, device=dev)
    vp = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)

    plain = qr.Scene(blob)
    scn = qr.Scene(blob, ray_queries=True)
    acc = scn.pt_adaptive_views(vt, w, h, min_samples=MIN, max_samples=MAX, tol=0.1)
    state = acc.state
    before = _host(state)
    t2 = float(acc.tol2)

    def call(s, views=vp(vt), n=2, w=w, h=h, state=vp(state), samples=1, mn_=MIN, mx=MAX, tol2=t2, frames=vp(fr), mean=vp(mn),
             counts=vp(cn), open=vp(op), flags=0):
        return L.qr_pt_adapt_views_async(s, views, n, w, h, state, samples, mn_, mx, ctypes.c_float(tol2), frames, mean, counts, open,
                                         flags, None)

    def untouched():
        torch.cuda.synchronize()
        return bool((fr == SI).all()) and bool((mn == SF).all()) and bool((cn == SI).all()) and bool((op == SI).all()) \
            and bool((_host(state) == before).all())

    def refused(rc, want, text):
        assert rc == want and text in L.qr_last_error().decode(), (rc, L.qr_last_error().decode())
        assert untouched(), "a refused call wrote something"

    refused(call(plain._h), UNSUP, "QR_UPLOAD_RAY_QUERIES")
    with pytest.raises(qr.QrError, match="QR_UPLOAD_RAY_QUERIES"):
        plain.pt_adaptive_views(vt, w, h, min_samples=MIN, max_samples=MAX, tol=0.1).step()
    plain.close()
    refused(call(None), ARG, "null scene")
    for kw in (dict(n=-1), dict(n=65536)):
        refused(call(scn._h, **kw), ARG, "view count")
    for kw in (dict(w=0), dict(h=0), dict(w=-5), dict(w=16385), dict(h=1 << 20)):
        refused(call(scn._h, **kw), ARG, "view frame size")
    refused(call(scn._h, n=65535, w=4096, h=4096), ARG, "QR_VIEW_MAX_WAVES")
    refused(call(scn._h, n=8, w=16384, h=16384), ARG, "2^30")                      # 2^31 slots in 2^25 footprints
    refused(call(scn._h, n=4, w=16384, h=16384), ARG, "2^29")                      # 2^30 slots: pt_views' most, twice this state's
    for kw in (dict(flags=1), dict(flags=0x80000000)):
        refused(call(scn._h, **kw), ARG, "flags")
    for kw in (dict(views=None), dict(state=None), dict(frames=None)):
        refused(call(scn._h, **kw), ARG, "null argument")
    for kw in (dict(views=vp(vt, 4)), dict(views=vp(vt, 8))):
        refused(call(scn._h, **kw), ARG, "16-byte aligned")
    for kw in (dict(state=vp(state, 2)), dict(frames=vp(fr, 1)), dict(mean=vp(mn, 2)), dict(counts=vp(cn, 2)), dict(open=vp(op, 1)),
               dict(open=vp(op, 2))):
        refused(call(scn._h, **kw), ARG, "4-byte aligned")
    for kw in (dict(samples=0), dict(samples=-1), dict(samples=513)):
        refused(call(scn._h, **kw), ARG, "samples must be")
    for kw in (dict(mn_=-1), dict(mx=0, mn_=0), dict(mx=-5, mn_=-7), dict(mn_=13), dict(mn_=3, mx=2), dict(mx=1 << 24),
               dict(mx=0x7FFFFFFF, mn_=0)):
        refused(call(scn._h, **kw), ARG, "min_samples and max_samples")
    for bad in (-1e-30, -1.0, float("nan"), float("inf"), float("-inf")):
        refused(call(scn._h, tol2=bad), ARG, "tol2")
    # the size query and the reset refuse the same sizes
    nb = ctypes.c_uint64(7)
    assert L.qr_pt_adapt_views_state_bytes(scn._h, 2, w, h, ctypes.byref(nb)) == 0 and nb.value == 2 * 8 * w * h * 4
    assert L.qr_pt_adapt_views_state_bytes(scn._h, 2, 0, h, ctypes.byref(nb)) == ARG and nb.value == 2 * 8 * w * h * 4
    assert L.qr_pt_adapt_views_state_bytes(scn._h, 4, 16384, 16384, ctypes.byref(nb)) == ARG
    assert L.qr_pt_adapt_views_state_bytes(scn._h, 2, 16384, 16384, ctypes.byref(nb)) == 0 and nb.value == 1 << 34
    assert L.qr_pt_adapt_views_state_bytes(scn._h, 2, w, h, None) == ARG
    assert L.qr_pt_adapt_views_reset(scn._h, 2, w, h, None) == ARG and L.qr_pt_adapt_views_reset(scn._h, 2, w, 16385, vp(state)) == ARG
    assert L.qr_pt_adapt_views_reset(scn._h, 2, w, h, vp(state, 2)) == ARG and L.qr_pt_adapt_views_reset(None, 2, w, h, vp(state)) == ARG
    assert L.qr_pt_adapt_views_reset(scn._h, 0, w, h, None) == 0
    # the empty call: no launch
    assert call(scn._h, n=0) == 0
    assert call(scn._h, n=0, views=None, state=None, frames=None, mean=None, counts=None, open=None) == 0
    assert untouched(), "an empty call wrote something"
    # the accepted edges: min = 0, max = 2^24 - 1, tol2 = 0, no mean, no counts, no open
    assert call(scn._h, mn_=0, mx=(1 << 24) - 1, tol2=0.0, mean=None, counts=None, open=None) == 0
    torch.cuda.synchronize()
    assert (mn == SF).all() and (cn == SI).all() and (op == SI).all() and (fr != SI).all() and (_host(state)[:, 4] == 1).all()
    acc.reset()

    # the Python object
    good = state.clone()
    for bad in (good[:1], good[:, :4], good.reshape(-1), good.float(), good.cpu(), good.cpu().numpy(), good[:, :, ::2]):
        with pytest.raises(qr.QrError, match="state must be"):
            scn.pt_adaptive_views(vt, w, h, min_samples=MIN, max_samples=MAX, tol=0.1, state=bad)
    with pytest.raises(qr.QrError, match="state must be"):
        scn.pt_adaptive_views(vt, w + 1, h, min_samples=MIN, max_samples=MAX, tol=0.1, state=good)
    for a, b in ((-1, 4), (5, 4), (0, 0), (0, 1 << 24), (1.0, 4), (1, None)):
        with pytest.raises(qr.QrError, match="min_samples and max_samples"):
            scn.pt_adaptive_views(vt, w, h, min_samples=a, max_samples=b, tol=0.1)
    for badt in (-0.1, float("nan"), float("inf"), 1e30, "x", None):
        with pytest.raises(qr.QrError, match="tol must be"):
            scn.pt_adaptive_views(vt, w, h, min_samples=MIN, max_samples=MAX, tol=badt)
    for bad in (vt.double(), vt[:, :15].contiguous(), vt.cpu(), vt.reshape(-1)):
        with pytest.raises(qr.QrError, match="views must be"):
            scn.pt_adaptive_views(bad, w, h, min_samples=MIN, max_samples=MAX, tol=0.1)
    for badf in (fr[:1], fr.float(), fr.cpu()):
        with pytest.raises(qr.QrError, match="frames must be"):
            acc.step(frames=badf)
    for badm in (mn[:1], mn.double(), mn.cpu()):
        with pytest.raises(qr.QrError, match="mean must be"):
            acc.step(mean=badm)
    for badc in (cn[:1], cn.float(), cn.cpu()):
        with pytest.raises(qr.QrError, match="counts must be"):
            acc.step(counts=badc)
    for bado in (op, op.float()[:1], op.cpu()[:1], 1):
        with pytest.raises(qr.QrError, match="open must be"):
            acc.step(open=bado)
    for bads in (0, 513, -2, 1.5):
        with pytest.raises(qr.QrError, match="samples must be"):
            acc.step(bads)
    for badv in (-1, 2, 0.5, None):
        with pytest.raises(qr.QrError, match="view must be"):
            acc.open_list(badv)
    torch.cuda.synchronize()
    assert (op == SI).all() and (_host(acc.state).view(np.uint32) == _fresh(rm, 2, w, h, 1)).all()

    got = _step(acc, 3)
    scn.close()
    want = _truth_call(rm, blob, views, w, h, _fresh(rm, 2, w, h, 1), 3, MIN, MAX, 0.1)
    _same(got, want, f"{scene}: after the refusals")


# One case once more through the guarded diagnostic build (make guard: QR_STATS + QR_GUARD), as the other feature files do.  The
# library is chosen when the package is imported, hence the child process: this file run as a script.

def _guard_child():
    from qr_loader import load_package
    qr = load_package()
    assert qr.LIB_PATH == GUARD_LIB, qr.LIB_PATH
    rm = _rays_mod()
    scene = GUARD_CASE
    w, h = CASE[scene]
    scn = qr.Scene(_base(scene), ray_queries=True)
    got = _run(scn, _cams(rm, scene), w, h, (CAND,), tol=TOL[scene])[0]
    scn.close()
    _same(got, _truth(rm, scene, [0, 1, 2, 3], w, h)[0], f"{scene}: guarded build")
    print(f"{scene} guard_ok 1", flush=True)
    return 0


@pytest.mark.gpu
def test_gpu_guarded_build_gives_the_same_adaptive_views():
    assert os.path.exists(GUARD_LIB), "libqrhip_guard.so is missing: build() makes it (make -C quadray-engine_amd/csrc guard)"
    env = dict(os.environ, QR_LIB=GUARD_LIB)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-child"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.count("guard_ok 1") == 1 and "QR_GUARD" not in out.stderr, out.stdout + out.stderr[-3000:]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.exit(_guard_child() if "--guard-child" in sys.argv else 2)
