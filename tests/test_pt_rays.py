"""Path-traced rays (include/qrhip.h qr_pt_rays_async, Scene.pt_rays): progressive path-tracer samples for caller-supplied rays, the
accumulation's state in an int32 [4, N] tensor the caller owns; and the host side of it in quadray-engine_amd/rays.py (pt_jitter,
spread_rays, pt_view_rays).

Every comparison is bit for bit.  The truth is tests/ptrays_oracle.c (qrp_pt_rays): the oracle's path tracer in the fast kernel's
order around the oracle's own list walk, set up from a caller's ray as tests/hitrec_oracle.c sets it up.  The CPU tests pin that
translation unit to oracle.render_pt (through pt_view_rays, the rays a path-traced frame's sample traces) and its spread path to
the numpy helpers, before any GPU is involved.

Scenes and cameras: SCENES and _cams of tests/test_pt_views.py.  Rays: view_rays(cam, 64, 64, base, 0), 4096 of them, with the
pinhole spread du, dv = the view's hor, ver, unless a test says otherwise.
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
import test_pt_views as TPV
from conftest import ROOT
from test_pt_views import SCENES, _base, _bits, _cams, _fsaa, _rays_mod, _size

ASM = TPV.ASM
GUARD_LIB = TPV.GUARD_LIB
GUARD_CASE = ("patched:demo02_160_gf_aa4", 2, 3)            # scene, view, samples
FAMILY_SCENES = ["demo01_160", "test05_160_j14", "synth_small", "crowd_hier"]
ARG, UNSUP = -1, -3
W = H = 64
# the seeded view the single-view tests use: one that test_inputs_discriminate shows to be lit and sensitive to the spread, the
# sample count and the depth (test18: the second view, the first sits inside an emitter)
VIEW = {"pt:test18_160_pt": 1, "pt:test18_160_gf_aa4_pt": 1, "patched:demo01_160": 2, "patched:demo02_160_gf_aa4": 2}


@pytest.fixture(scope="module")
def rays_mod():
    return _rays_mod()


# ------------------------------------------------------------------------------------------------- the truth (CPU)

_TU = None


def _tu():
    global _TU
    if _TU is None:
        import __graft_entry__ as g
        L = ctypes.CDLL(g.build_ptrays_oracle())
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.qrp_pt_rays.argtypes = [vp, ctypes.c_uint64, vp, vp, ctypes.c_int64, vp, ci, ci, ci, ci, vp, vp]
        L.qrp_pt_rays.restype = ci
        _TU = L
    return _TU


def _tu_run(blob, rays, spread, state, done, samples, depth=None):
    """qrp_pt_rays on a copy of `state` (uint32 or int32 [4, N]): (rgb float32 [N, 3], state uint32 [4, N], stats dict)"""
    import qr_oracle
    r = np.ascontiguousarray(rays, dtype=np.float32)
    n = r.shape[0]
    assert r.shape == (n, 8)
    sp = None if spread is None else np.ascontiguousarray(spread, dtype=np.float32)
    assert sp is None or sp.shape == (n, 8)
    st = np.ascontiguousarray(state).view(np.uint32).copy()
    assert st.shape == (4, n)
    rgb = np.zeros((n, 3), dtype=np.float32)
    stats = (ctypes.c_uint64 * 6)()
    buf = ctypes.create_string_buffer(blob, len(blob))
    rc = _tu().qrp_pt_rays(buf, len(blob), r.ctypes.data, None if sp is None else sp.ctypes.data, n, st.ctypes.data, int(done),
                           int(samples), -1 if depth is None else int(depth), 16, rgb.ctypes.data, stats)
    assert rc == 0, rc
    return rgb, st, dict(zip(qr_oracle.PT_STATS, (int(v) for v in stats)))


def _fresh(rm, n):
    """the state after a reset: plane 0 = pt_seeds(n, 1, 1), means 0"""
    st = np.zeros((4, n), dtype=np.uint32)
    st[0] = rm.pt_seeds(n, 1, 1)
    return st


def _depth(blob):
    return int(_rayq.frame_words(blob)[0][29])


def _spread_of(view, n):
    """the pinhole spread: du, dv = the view's hor, ver for every ray"""
    v = np.asarray(view, dtype=np.float32).reshape(16)
    sp = np.zeros((n, 8), dtype=np.float32)
    sp[:, 0:3] = v[8:11]
    sp[:, 4:7] = v[12:15]
    return sp


_RAYS, _TRUTH, _STATS = {}, {}, {}


def _view_rays(rm, scene, j):
    """(rays [4096, 8], spread [4096, 8]) of seeded view j of a scene; computed once, read-only"""
    if (scene, j) not in _RAYS:
        cam = _cams(rm, scene)[j]
        r = rm.view_rays(cam, W, H, _base(scene), 0)
        sp = _spread_of(cam, len(r))
        r.setflags(write=False); sp.setflags(write=False)
        _RAYS[scene, j] = (r, sp)
    return _RAYS[scene, j]


def _truth(rm, scene, j, spread, samples, depth=None):
    """(rgb, state) of the translation unit for view j's rays from a fresh state; computed once, read-only"""
    key = (scene, j, bool(spread), samples, depth)
    if key not in _TRUTH:
        r, sp = _view_rays(rm, scene, j)
        rgb, st, stats = _tu_run(_base(scene), r, sp if spread else None, _fresh(rm, len(r)), 0, samples, depth)
        rgb.setflags(write=False); st.setflags(write=False)
        _TRUTH[key] = (rgb, st)
        _STATS[key] = stats
    return _TRUTH[key]


def _differ(a, b):
    """fraction of rays whose rgb differs in some bit"""
    return float((_bits(a) != _bits(b)).any(axis=1).mean())


# ---------------------------------------------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("scene", ["pt:test18_160_pt", "pt:test18_160_gf_aa4_pt"])
def test_tu_through_pt_view_rays_is_render_pt(oracle, rays_mod, scene):
    """three frames of the snapshot's own camera sent through the translation unit as caller rays (pt_view_rays from pt_seeds,
    plane 0 overwritten by the states after the jitter draws, no spread), reduced as the frame reduces its samples: the mean and
    the packed frame of oracle.render_pt on the snapshot with one tile that holds the global list, on every pixel"""
    blob = _base(scene)
    w, h = _size(blob)
    ns = 1 << _fsaa(blob)
    assert int(_rayq.frame_words(blob)[0][33]) == w, "frm_row == frm_w: the seed slots are the ray order"
    slots = w * h * ns
    st = np.zeros((4, slots), dtype=np.uint32)
    st[0] = rays_mod.pt_seeds(w, h, ns)
    view = rays_mod.view_of(blob)
    for s in range(3):
        r, adv = rays_mod.pt_view_rays(view, w, h, blob, st[0])
        assert r.shape == (slots, 8) and r.dtype == np.float32 and adv.dtype == np.uint32
        st[0] = adv
        rgb, st, _ = _tu_run(blob, r, None, st, s, 1)
    per_sample = np.ascontiguousarray(rgb.reshape(w * h, ns, 3).transpose(1, 0, 2))
    f, m = oracle.render_pt(_rayq.one_tile(blob), 3, order="kernel", threads=16, want_mean=True)
    mean = rays_mod.reduce_colors(per_sample, blob)
    nm = int((_bits(mean) != _bits(m.reshape(w * h, 3))).any(axis=1).sum())
    nf = int((rays_mod.pack_colors(per_sample, blob) != f).sum())
    print(f"{scene}: {nm} of {w * h} pixels of the mean differ, {nf} of the frame")
    assert nm == 0 and nf == 0


@pytest.mark.parametrize("scene", ["pt:test18_160_pt", "patched:demo02_160_gf_aa4"])
def test_tu_spread_path_is_the_numpy_jitter(rays_mod, scene):
    """two samples with a spread in one call of the translation unit = per sample pt_jitter, spread_rays and its no-spread path
    on the advanced states: every rgb and state word"""
    r, sp = _view_rays(rays_mod, scene, VIEW[scene])
    n = len(r)
    rgb_a, st_a, _ = _tu_run(_base(scene), r, sp, _fresh(rays_mod, n), 0, 2)
    st = _fresh(rays_mod, n)
    moved = 0
    for s in range(2):
        adv, hh, vv = rays_mod.pt_jitter(st[0])
        assert hh.dtype == np.float32 and vv.dtype == np.float32 and adv.dtype == np.uint32
        assert (hh >= -0.5).all() and (hh <= 0.5).all() and (vv >= -0.5).all() and (vv <= 0.5).all()
        jr = rays_mod.spread_rays(r, sp, hh, vv)
        assert (jr[:, :4] == r[:, :4]).all() and (_bits(jr[:, 7]) == _bits(r[:, 7])).all()
        moved += int((jr[:, 4:7] != r[:, 4:7]).any(axis=1).sum())
        st[0] = adv
        rgb_b, st, _ = _tu_run(_base(scene), jr, None, st, s, 1)
    assert moved > n, "the jitter moves the directions"
    assert (_bits(rgb_a) == _bits(rgb_b)).all(), f"{scene}: {int((_bits(rgb_a) != _bits(rgb_b)).any(axis=1).sum())} of {n} rays differ"
    assert (st_a == st).all(), f"{scene}: {int((st_a != st).sum())} state words differ"


def test_pt_jitter_draws_are_the_oracles_first_two(oracle, rays_mod):
    """pt_jitter's h and v are the tent filter of the first two numbers oracle.pt_trace_sample lists for a sample, and its
    states the generator's after two steps; spread_rays keeps to the stated order of operations"""
    base = _base("pt:test18_160_gf_aa4_pt")
    w, h = _size(base)
    seeds = rays_mod.pt_seeds(w, h, 4)
    snap = TPV._view_snapshot(base, rays_mod.view_of(base), w, h)
    f32 = np.float32

    def tent(u):
        u = f32(u) + f32(u)
        a = f32(np.sqrt(u)) - f32(1) if u < f32(1) else f32(1) - f32(np.sqrt(f32(2) - u))
        return f32(a) * f32(0.5)

    for x, y, k in ((0, 0, 0), (5, 3, 2), (77, 60, 1), (159, 119, 3)):
        slot = (y * w + x) * 4 + k
        draws, _ = oracle.pt_trace_sample(snap, 1, x, y, k)
        assert [d[1] for d in draws[:2]] == ["jitter_h", "jitter_v"], draws[:2]
        s2, hh, vv = rays_mod.pt_jitter(seeds[slot:slot + 1])
        s1, _ = rays_mod.pt_random(seeds[slot])
        assert int(s2[0]) == int(rays_mod.pt_random(s1)[0])
        want = _bits(np.array([tent(draws[0][2]), tent(draws[1][2])], dtype=np.float32))
        assert (_bits(np.array([hh[0], vv[0]])) == want).all(), (x, y, k, float(hh[0]), float(vv[0]), draws[:2])
    # both branches of the filter and its ends
    s, hh, vv = rays_mod.pt_jitter(seeds)
    assert s.shape == hh.shape == vv.shape == seeds.shape and (hh < 0).any() and (hh > 0).any() and (vv < 0).any() and (vv > 0).any()
    # spread_rays, component by component in float32
    rng = np.random.default_rng(7)
    r = rng.normal(size=(33, 8)).astype(np.float32)
    sp = rng.normal(size=(33, 8)).astype(np.float32)
    a, b = rng.uniform(-0.5, 0.5, 33).astype(np.float32), rng.uniform(-0.5, 0.5, 33).astype(np.float32)
    out = rays_mod.spread_rays(r, sp, a, b)
    for i in (0, 7, 32):
        for c in range(3):
            t = f32(f32(sp[i, c] * a[i]) + f32(sp[i, 4 + c] * b[i]))
            assert _bits(out[i, 4 + c]) == _bits(f32(r[i, 4 + c] + t))
    assert (out[:, :4] == r[:, :4]).all() and (out[:, 7] == r[:, 7]).all() and out is not r
    with pytest.raises(ValueError):
        rays_mod.spread_rays(r, sp[:5], a, b)
    with pytest.raises(ValueError):
        rays_mod.pt_view_rays(rays_mod.view_of(base), w, h, base, seeds[:7])


def test_pt_rays_abi_and_constants(qr):
    """the library exports the three entry points, the header declares them, and its constants are the module's"""
    L = qr.lib()
    with open(os.path.join(ROOT, "include", "qrhip.h")) as f:
        hdr = f.read()
    for sym in ("qr_pt_rays_state_bytes", "qr_pt_rays_reset", "qr_pt_rays_async"):
        assert hasattr(L, sym), sym
        assert sym in qr.ABI_SYMBOLS and f"int {sym}(" in hdr, sym
    assert f"#define QR_PT_RAYS_MAX_SAMPLES {qr.PT_RAYS_MAX_SAMPLES} " in hdr and qr.PT_RAYS_MAX_SAMPLES == 512
    assert f"#define QR_PT_RAYS_STATE_WORDS {qr.PT_RAYS_STATE_WORDS} " in hdr and qr.PT_RAYS_STATE_WORDS == 4
    assert "typedef struct qr_ray_spread { float du[3], pad0, dv[3], pad1; } qr_ray_spread;" in hdr
    assert hasattr(qr.Scene, "pt_rays") and hasattr(qr, "PtRays")
    for m in ("step", "reset", "clone"):
        assert callable(getattr(qr.PtRays, m))


def test_pt_rays_kernel_in_resource_check():
    """the build's register check lists the kernel once, at the path-traced view kernel's budget (168 VGPRs, nothing spilled,
    2128 B of private segment), and the built assembly passes it"""
    import importlib.util
    path = os.path.join(ROOT, "tools", "check_kernel_resources.py")
    spec = importlib.util.spec_from_file_location("check_kernel_resources", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    frags = [f for f in m.LIMITS if "qr_pt_rays_kernel" in f]
    assert frags == ["17qr_pt_rays_kernel"]
    assert m.LIMITS[frags[0]] == (168, 0, 2128)
    r = subprocess.run([sys.executable, path, ASM, "--print"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("qr_pt_rays_kernel") == 1


@pytest.mark.parametrize("scene", SCENES)
def test_inputs_discriminate(rays_mod, scene):
    """A condition on the test inputs, checked with the translation unit alone: among the 3-sample results of the four views
    at least two meet all of: >= 15 % of the rays lit; spread against no spread differ on >= 25 % of the rays; 1 against 3
    samples on >= 15 %; depth 0 against the scene's depth on >= 15 %"""
    rows = []
    for j in range(4):
        s3 = _truth(rays_mod, scene, j, True, 3)[0]
        lit = float((s3 != 0).any(axis=1).mean())
        spr = _differ(s3, _truth(rays_mod, scene, j, False, 3)[0])
        conv = _differ(s3, _truth(rays_mod, scene, j, True, 1)[0])
        dep = _differ(s3, _truth(rays_mod, scene, j, True, 3, 0)[0])
        rows.append((lit, spr, conv, dep))
    print(f"{scene} (depth {_depth(_base(scene))}): lit / spread / 1 vs 3 / depth 0, % per view: "
          + "; ".join(" ".join(f"{100 * x:.1f}" for x in r) for r in rows))
    ok = [lit >= 0.15 and spr >= 0.25 and conv >= 0.15 and dep >= 0.15 for lit, spr, conv, dep in rows]
    assert sum(ok) >= 2, rows


def test_inputs_reach_every_branch_of_the_path_tracer(oracle, rays_mod):
    """over the six scenes' seeded views (3 samples, with the spread, at the scene's depth) every counter of oracle.PT_STATS,
    summed by the translation unit, is non-zero"""
    total = dict.fromkeys(oracle.PT_STATS, 0)
    for scene in SCENES:
        for j in range(4):
            _truth(rays_mod, scene, j, True, 3)
            for k, v in _STATS[scene, j, True, 3, None].items():
                total[k] += v
    print(total)
    assert all(total[k] > 0 for k in total), total


# ---------------------------------------------------------------------------------------------------------------- GPU

def _t(scn, a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).to(f"cuda:{scn.device}")     # a writable copy


def _host(x):
    import torch
    torch.cuda.synchronize()
    return x.cpu().numpy().copy()


def _state(acc):
    return _host(acc.state).view(np.uint32)


def _run(scn, rays, spread, splits, state=None):
    """a fresh accumulation (or one started from `state`, holding no samples) stepped by `splits`: (rgb, state) on the host"""
    import torch
    n = len(rays)
    if state is None:
        acc = scn.pt_rays(n)
    else:
        acc = scn.pt_rays(n, state=torch.from_numpy(np.ascontiguousarray(state).view(np.int32)).to(f"cuda:{scn.device}"), samples=0)
    rt, st = _t(scn, rays), None if spread is None else _t(scn, spread)
    for s in splits:
        rgb = acc.step(rt, s, spread=st)
    assert acc.samples == sum(splits) and tuple(rgb.shape) == (n, 3)
    return _host(rgb), _state(acc)


def _same(got, want, what):
    (grgb, gst), (wrgb, wst) = got, want
    assert grgb.shape == wrgb.shape and grgb.dtype == np.float32 and gst.shape == wst.shape
    nr = int((_bits(grgb) != _bits(wrgb)).any(axis=1).sum())
    ns = int((gst.view(np.uint32)[0] != wst.view(np.uint32)[0]).sum())
    nm = int((gst.view(np.uint32)[1:] != wst.view(np.uint32)[1:]).any(axis=0).sum())
    assert nr == 0 and ns == 0 and nm == 0, \
        f"{what}: of {len(grgb)} rays {nr} differ in rgb, {ns} in the generator state, {nm} in the state's means"
    assert (_bits(grgb) == gst.view(np.uint32)[1:].T).all(), f"{what}: rgb is not the state's means"


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["pt:test18_160_gf_aa4_pt", "patched:demo01_160"])
def test_gpu_frame_through_the_ray_path(qr, oracle, rays_mod, scene):
    """a 64 x 64 frame of one seeded view (VIEW), three samples, each sent as pt_view_rays with plane 0 overwritten by the
    states after the jitter draws: the reduced mean and packed frame are oracle.render_pt's of the view's snapshot and those of
    pt_views on the same GPU, whose state it shares word for word"""
    import torch
    base = _base(scene)
    ns = 1 << _fsaa(base)
    cam = _cams(rays_mod, scene)[VIEW[scene]]
    slots = W * H * ns
    scn = qr.Scene(base, ray_queries=True)
    acc = scn.pt_rays(slots)
    for s in range(3):
        r, adv = rays_mod.pt_view_rays(cam, W, H, base, _state(acc)[0])
        acc.state[0] = torch.from_numpy(adv.view(np.int32)).to(acc.state.device)
        rgb = acc.step(_t(scn, r), 1)
    rgb, st = _host(rgb), _state(acc)
    pv = scn.pt_views(_t(scn, cam[None]), W, H)
    fv, mv = pv.step(3, mean=True)
    fv, mv, sv = _host(fv).view(np.uint32)[0], _host(mv)[0], _host(pv.state).view(np.uint32)[0]
    scn.close()
    per_sample = np.ascontiguousarray(rgb.reshape(W * H, ns, 3).transpose(1, 0, 2))
    mean = rays_mod.reduce_colors(per_sample, base)
    frame = rays_mod.pack_linear(mean, base, W, H)
    wf, wm = TPV._truth(oracle, scene, cam, W, H, 3)
    nm, nf = int((_bits(mean) != _bits(wm.reshape(-1, 3))).any(axis=1).sum()), int((frame != wf).sum())
    assert nm == 0 and nf == 0, f"{scene}: {nm} of {W * H} pixels of the mean, {nf} of the frame differ from the oracle's"
    nm, nf = int((_bits(mean) != _bits(mv.reshape(-1, 3))).any(axis=1).sum()), int((frame != fv).sum())
    assert nm == 0 and nf == 0, f"{scene}: {nm} of {W * H} pixels of the mean, {nf} of the frame differ from pt_views'"
    assert (st == sv).all(), f"{scene}: {int((st != sv).sum())} state words differ from pt_views'"


@pytest.mark.gpu
@pytest.mark.parametrize("scene", SCENES)
def test_gpu_seeded_views_equal_the_tu(qr, rays_mod, scene):
    """the four seeded views' rays, with and without the spread, three samples in one call: rgb and state are the translation
    unit's"""
    scn = qr.Scene(_base(scene), ray_queries=True)
    got = {}
    for j in range(4):
        r, sp = _view_rays(rays_mod, scene, j)
        for spread in (True, False):
            got[j, spread] = _run(scn, r, sp if spread else None, (3,))
    scn.close()
    for (j, spread), g in got.items():
        _same(g, _truth(rays_mod, scene, j, spread, 3), f"{scene} view {j} spread={spread}")


def _family_spread(name, fam, n):
    """a seeded spread for rays that belong to no camera: components of a few hundredths"""
    rng = np.random.default_rng(zlib.crc32(f"{name}:{fam}:spread".encode()))
    sp = (rng.normal(size=(n, 8)) * 0.03).astype(np.float32)
    sp[:, 3] = np.float32(np.nan)           # the pad words are ignored
    sp[:, 7] = np.float32(1e30)
    return sp


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILY_SCENES)
def test_gpu_adversarial_families_equal_the_tu(qr, oracle, rays_mod, name, tmp_path):
    """the ray families of tests/_rayset.py (signed zeros, denormals, intervals at a hit's t, scaled directions, far origins,
    probes, all mixed) on fixtures with emission patched on, two samples, with and without a spread"""
    plain = RS.scene_blob(name)
    blob = _ptpatch.pt_patch(plain)
    off, img = RS.query_image(qr, name, tmp_path)
    g, reach = RS.dda_grid(off, img), RS.reach_of(img)
    scn = qr.Scene(blob, ray_queries=True)
    got, lit = [], 0
    for fam in RS.FAMILIES:
        r = RS.family(plain, name, fam, oracle, g, reach)
        if len(r) == 0:
            continue
        for sp in (_family_spread(name, fam, len(r)), None):
            got.append((fam, r, sp, _run(scn, r, sp, (2,))))
    scn.close()
    for fam, r, sp, res in got:
        rgb, st, _ = _tu_run(blob, r, sp, _fresh(rays_mod, len(r)), 0, 2)
        _same(res, (rgb, st), f"{name} family {fam} spread={sp is not None}")
        lit += int((rgb != 0).any(axis=1).sum())
    assert lit > 0, "no ray of any family saw light"


@pytest.mark.gpu
def test_gpu_depth_sweep(qr, rays_mod):
    """depths 0, 1, 3, 6 and 10 on the second seeded view of test18 (the first sits inside an emitter)"""
    scene = "pt:test18_160_pt"
    r, sp = _view_rays(rays_mod, scene, VIEW[scene])
    scn = qr.Scene(_base(scene), ray_queries=True)
    got = {}
    for depth in (0, 1, 3, 6, 10):
        scn.set_depth(depth)
        got[depth] = _run(scn, r, sp, (3,))
    scn.close()
    for depth, g in got.items():
        _same(g, _truth(rays_mod, scene, VIEW[scene], True, 3, depth), f"{scene} depth {depth}")
    assert all(_differ(got[0][0], got[d][0]) > 0 for d in (3, 6, 10)), "the depth does not show"


@pytest.mark.gpu
@pytest.mark.parametrize("scene,depth", [("pt:test18_160_pt", 10), ("patched:demo02_160_gf_aa4", None)])
def test_gpu_splits(qr, rays_mod, scene, depth):
    """1+1+1+1+1, 2+3 and 5 samples in one call give equal rgb and state words; 3+4 is the translation unit's 7 (sample numbers
    3, 5, 6 and 7: weights that are not exact in fp32)"""
    r, sp = _view_rays(rays_mod, scene, VIEW[scene])
    scn = qr.Scene(_base(scene), ray_queries=True)
    if depth is not None:
        scn.set_depth(depth)
    runs = [_run(scn, r, sp, split) for split in ((1, 1, 1, 1, 1), (2, 3), (5,))]
    seven = _run(scn, r, sp, (3, 4))
    scn.close()
    for got, how in zip(runs[:2], ("1+1+1+1+1", "2+3")):
        _same(got, runs[2], f"{scene}: {how} against 5 in one call")
    _same(seven, _truth(rays_mod, scene, VIEW[scene], True, 7, depth), f"{scene}: 3+4 samples")
    assert _differ(seven[0], runs[2][0]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 129])
def test_gpu_batch_sizes_and_bounds(qr, rays_mod, n):
    """partial and full waves, state and rgb carved out of larger sentinel-filled buffers: the translation unit's bits, and
    reset and launch leave the tails alone"""
    import torch
    scene = "patched:demo02_160_gf_aa4"
    r, sp = _view_rays(rays_mod, scene, VIEW[scene])
    r, sp = r[1000:1000 + n], sp[1000:1000 + n]
    TAIL, SI, SF = 4096, 0x5A5A5A5A, 12345.0
    scn = qr.Scene(_base(scene), ray_queries=True)
    dev = f"cuda:{scn.device}"
    stb = torch.full((4 * n + TAIL,), SI, dtype=torch.int32, device=dev)
    rgbb = torch.full((3 * n + TAIL,), SF, dtype=torch.float32, device=dev)
    acc = scn.pt_rays(n, state=stb[:4 * n].view(4, n), samples=0)
    acc.reset()
    torch.cuda.synchronize()
    assert (stb[4 * n:] == SI).all(), "reset wrote past the state"
    assert (_state(acc) == _fresh(rays_mod, n)).all()
    out = acc.step(_t(scn, r), 3, spread=_t(scn, sp), rgb=rgbb[:3 * n].view(n, 3))
    assert out.data_ptr() == rgbb.data_ptr()
    none = acc.clone().step(_t(scn, r), 1, spread=_t(scn, sp), rgb=False)
    got = (_host(out), _state(acc))
    tails_ok = bool((stb[4 * n:] == SI).all()) and bool((rgbb[3 * n:] == SF).all())
    scn.close()
    assert none is None
    assert tails_ok, f"n = {n}: a tail was written"
    rgb, st, _ = _tu_run(_base(scene), r, sp, _fresh(rays_mod, n), 0, 3)
    _same(got, (rgb, st), f"{scene} n = {n}")


@pytest.mark.gpu
def test_gpu_permutation_and_single_rays(qr, rays_mod):
    """rays permuted together with their state columns give permuted results; ray i of a batch is ray i alone"""
    scene = "pt:test18_160_pt"
    r, sp = _view_rays(rays_mod, scene, VIEW[scene])
    n = len(r)
    perm = np.random.default_rng(11).permutation(n)
    st0 = _fresh(rays_mod, n)
    scn = qr.Scene(_base(scene), ray_queries=True)
    a = _run(scn, r, sp, (3,))
    b = _run(scn, r[perm], sp[perm], (3,), state=st0[:, perm])
    picks = [0, 63, 64, 2077, n - 1]
    alone = [_run(scn, r[i:i + 1], sp[i:i + 1], (3,), state=st0[:, i:i + 1]) for i in picks]
    scn.close()
    _same(b, (a[0][perm], a[1][:, perm]), f"{scene}: permuted rays")
    assert _differ(a[0], b[0]) > 0.1, "the permutation moved nothing"
    for i, one in zip(picks, alone):
        _same(one, (a[0][i:i + 1], a[1][:, i:i + 1]), f"{scene}: ray {i} alone")


@pytest.mark.gpu
def test_gpu_checkpoint(qr, rays_mod):
    """clone() after 2 samples: original and copy, each continued by 2, are equal and the translation unit's 4; reset() starts
    over; a state that left the device and came back continues like the clone"""
    import torch
    scene = "pt:test18_160_gf_aa4_pt"
    r, sp = _view_rays(rays_mod, scene, VIEW[scene])
    scn = qr.Scene(_base(scene), ray_queries=True)
    rt, st = _t(scn, r), _t(scn, sp)
    acc = scn.pt_rays(len(r))
    acc.step(rt, 2, spread=st)
    cp = acc.clone()
    assert cp.samples == 2 and cp.state.data_ptr() != acc.state.data_ptr()
    a = (_host(acc.step(rt, 2, spread=st)), _state(acc))
    b = (_host(cp.step(rt, 2, spread=st)), _state(cp))
    acc.reset()
    assert acc.samples == 0
    one = (_host(acc.step(rt, 1, spread=st)), _state(acc))
    back = scn.pt_rays(len(r), state=torch.from_numpy(a[1].view(np.int32)).to(f"cuda:{scn.device}"), samples=4)
    five_a = (_host(back.step(rt, 1, spread=st)), _state(back))
    five_b = (_host(cp.step(rt, 1, spread=st)), _state(cp))
    assert back.samples == 5 and cp.samples == 5
    scn.close()
    _same(a, b, f"{scene}: original and clone after 2 + 2 samples")
    _same(a, _truth(rays_mod, scene, VIEW[scene], True, 4), f"{scene}: 2 + 2 samples")
    _same(one, _truth(rays_mod, scene, VIEW[scene], True, 1), f"{scene}: after reset()")
    _same(five_a, five_b, f"{scene}: a state restored from the host against the clone, fifth sample")
    _same(five_a, _truth(rays_mod, scene, VIEW[scene], True, 5), f"{scene}: the fifth sample")


@pytest.mark.gpu
def test_gpu_fresh_state_is_the_documented_layout(qr, rays_mod):
    scn = qr.Scene(_base("pt:test18_160_pt"), ray_queries=True)
    acc = scn.pt_rays(1000)
    st = _host(acc.state)
    empty = scn.pt_rays(0)
    shape0 = tuple(empty.state.shape)
    scn.close()
    assert st.shape == (4, 1000) and st.dtype == np.int32 and acc.samples == 0 and acc.n == 1000
    assert (st[0].view(np.uint32) == rays_mod.pt_seeds(1000, 1, 1)).all() and (st[1:] == 0).all()
    assert (st[0].view(np.uint32) == rays_mod.pt_seeds(50, 10, 2)).all(), "slot order: the seed plane of a 50 x 10 frame at 2x"
    assert shape0 == (4, 0)


@pytest.mark.gpu
def test_gpu_independent_of_the_scenes_own_mode(qr, oracle, rays_mod):
    """set_pt(True), render(), a pt_rays step, render(): the scene's second frame is the oracle's N = 2 of the snapshot (its
    planes and counter were left alone); the rays' bits are the same inside and outside the mode, where shade() works as before"""
    import torch
    scene = "pt:test18_160_pt"
    blob = _base(scene)
    r, sp = _view_rays(rays_mod, scene, VIEW[scene])
    scn = qr.Scene(blob, ray_queries=True)
    rt, st = _t(scn, r), _t(scn, sp)
    scn.set_pt(True)
    f = scn.new_frame()
    scn.render(f)
    acc = scn.pt_rays(len(r))
    on = (_host(acc.step(rt, 1, spread=st)), _state(acc))
    scn.render(f)
    torch.cuda.synchronize()
    second = f.cpu().numpy().view(np.uint32).copy()
    with pytest.raises(qr.QrError, match="path-tracer"):
        scn.shade(rt)
    scn.set_pt(False)
    shaded = _host(scn.shade(rt))
    off = (_host(acc.step(rt, 2, spread=st)), _state(acc))           # ... and the accumulation goes on with the mode off
    plain = _run(scn, r, sp, (1,))
    scn.close()
    _same(on, _truth(rays_mod, scene, VIEW[scene], True, 1), f"{scene}: with set_pt(True)")
    _same(plain, on, f"{scene}: outside against inside the mode")
    _same(off, _truth(rays_mod, scene, VIEW[scene], True, 3), f"{scene}: two more samples after set_pt(False)")
    nd = int((second != oracle.render_pt(blob, 2, order="kernel", threads=16)).sum())
    assert nd == 0, f"{scene}: the scene's own second frame differs from the oracle's N = 2 on {nd} pixels"
    want, _ = oracle.trace_rays(blob, r, "shade")
    assert (_bits(shaded) == _bits(want)).all(), "shade after set_pt(False) is not the ray-traced colour"


@pytest.mark.gpu
def test_gpu_refusals(qr, rays_mod):
    import torch
    scene = "pt:test18_160_pt"
    blob = _base(scene)
    r, sp = _view_rays(rays_mod, scene, VIEW[scene])
    n = 130
    r, sp = r[:n], sp[:n]
    L = qr.lib()
    dev = "cuda:0"
    SF = 12345.0
    rt, st = torch.from_numpy(r.copy()).to(dev), torch.from_numpy(sp.copy()).to(dev)
    rgb = torch.full((n, 3), SF, dtype=torch.float32, device=dev)
    vp = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)

    plain = qr.Scene(blob)
    scn = qr.Scene(blob, ray_queries=True)
    acc = scn.pt_rays(n)
    state = acc.state
    before = _state(acc)

    def call(s, rays=vp(rt), spread=vp(st), n=n, state=vp(state), done=0, samples=1, rgb=vp(rgb), flags=0):
        return L.qr_pt_rays_async(s, rays, spread, n, state, done, samples, rgb, flags, None)

    def refused(rc, want, text):
        assert rc == want and text in L.qr_last_error().decode(), (rc, L.qr_last_error().decode())

    refused(call(plain._h), UNSUP, "QR_UPLOAD_RAY_QUERIES")
    with pytest.raises(qr.QrError, match="QR_UPLOAD_RAY_QUERIES"):
        plain.pt_rays(n).step(rt)
    plain.close()
    refused(call(None), ARG, "null scene")
    for kw in (dict(n=-1), dict(n=1 << 31), dict(n=1 << 40)):
        refused(call(scn._h, **kw), ARG, "ray count")
    for kw in (dict(flags=1), dict(flags=2), dict(flags=0x80000000)):           # QR_TRACE_COHERENT is not a flag of this call
        refused(call(scn._h, **kw), ARG, "flags")
    for kw in (dict(rays=None), dict(state=None)):
        refused(call(scn._h, **kw), ARG, "null argument")
    for kw in (dict(rays=vp(rt, 4)), dict(rays=vp(rt, 8)), dict(spread=vp(st, 4)), dict(spread=vp(st, 8))):
        refused(call(scn._h, **kw), ARG, "16-byte aligned")
    for kw in (dict(state=vp(state, 2)), dict(rgb=vp(rgb, 1)), dict(rgb=vp(rgb, 2))):
        refused(call(scn._h, **kw), ARG, "4-byte aligned")
    for kw in (dict(samples=0), dict(samples=-1), dict(samples=513)):
        refused(call(scn._h, **kw), ARG, "samples must be")
    for kw in (dict(done=-1), dict(done=(1 << 24) - 1), dict(done=(1 << 24) - 512, samples=512), dict(done=1 << 30)):
        refused(call(scn._h, **kw), ARG, "done")
    # the size query and the reset refuse the same counts
    nb = ctypes.c_uint64(7)
    assert L.qr_pt_rays_state_bytes(scn._h, n, ctypes.byref(nb)) == 0 and nb.value == 4 * n * 4
    assert L.qr_pt_rays_state_bytes(scn._h, -1, ctypes.byref(nb)) == ARG and nb.value == 4 * n * 4
    assert L.qr_pt_rays_state_bytes(scn._h, 1 << 31, ctypes.byref(nb)) == ARG
    assert L.qr_pt_rays_state_bytes(scn._h, n, None) == ARG and L.qr_pt_rays_state_bytes(None, n, ctypes.byref(nb)) == ARG
    assert L.qr_pt_rays_reset(scn._h, n, None) == ARG and L.qr_pt_rays_reset(scn._h, -1, vp(state)) == ARG
    assert L.qr_pt_rays_reset(scn._h, n, vp(state, 2)) == ARG and L.qr_pt_rays_reset(None, n, vp(state)) == ARG
    assert L.qr_pt_rays_reset(scn._h, 0, None) == 0
    # the empty call: no launch
    assert call(scn._h, n=0) == 0 and call(scn._h, n=0, rays=None, spread=None, state=None, rgb=None) == 0
    torch.cuda.synchronize()
    assert (rgb == SF).all() and (_state(acc) == before).all(), "a refused or empty call wrote something"

    # the Python object: a state of the wrong size, type or device
    good = state.clone()
    for bad in (good[:3], good[:, :n - 1], good.reshape(-1), good.float(), good.cpu(), good.cpu().numpy(), good[:, ::2]):
        with pytest.raises(qr.QrError, match="state must be"):
            scn.pt_rays(n, state=bad, samples=0)
    with pytest.raises(qr.QrError, match="state must be"):
        scn.pt_rays(n + 1, state=good)
    with pytest.raises(qr.QrError, match="samples"):
        scn.pt_rays(n, state=good, samples=-1)
    with pytest.raises(qr.QrError, match="samples"):
        scn.pt_rays(n, samples=3)
    for badn in (-1, 1.5, None):
        with pytest.raises(qr.QrError, match="n must be"):
            scn.pt_rays(badn)
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
    for bads in (0, 513, -2):
        with pytest.raises(qr.QrError, match="samples must be"):
            acc.step(rt, bads)
    with pytest.raises(qr.QrError, match="samples must be"):
        acc.step(rt, 1.5)
    assert acc.samples == 0
    assert (_state(acc) == before).all()

    got = (_host(acc.step(rt, 1, spread=st)), _state(acc))
    scn.close()
    rgb_w, st_w, _ = _tu_run(blob, r, sp, _fresh(rays_mod, n), 0, 1)
    _same(got, (rgb_w, st_w), f"{scene}: after the refusals")


# One case once more through the guarded diagnostic build (make guard: QR_STATS + QR_GUARD), as the other feature files do.  The
# library is chosen when the package is imported, hence the child process: this file run as a script.

def _guard_child():
    from qr_loader import load_package
    qr = load_package()
    assert qr.LIB_PATH == GUARD_LIB, qr.LIB_PATH
    rm = _rays_mod()
    scene, j, n = GUARD_CASE
    r, sp = _view_rays(rm, scene, j)
    scn = qr.Scene(_base(scene), ray_queries=True)
    got = _run(scn, r, sp, (n,))
    bare = _run(scn, r, None, (n,))
    scn.close()
    _same(got, _truth(rm, scene, j, True, n), f"{scene}: guarded build")
    _same(bare, _truth(rm, scene, j, False, n), f"{scene}: guarded build, no spread")
    print(f"{scene} guard_ok 1", flush=True)
    return 0


@pytest.mark.gpu
def test_gpu_guarded_build_gives_the_same_path_traced_rays():
    assert os.path.exists(GUARD_LIB), "libqrhip_guard.so is missing: build() makes it (make -C quadray-engine_amd/csrc guard)"
    env = dict(os.environ, QR_LIB=GUARD_LIB)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-child"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.count("guard_ok 1") == 1 and "QR_GUARD" not in out.stderr, out.stdout + out.stderr[-3000:]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.exit(_guard_child() if "--guard-child" in sys.argv else 2)
