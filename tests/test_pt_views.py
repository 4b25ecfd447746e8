"""Path-traced views (include/qrhip.h qr_pt_views_async, Scene.pt_views): progressive path-traced frames from caller-supplied
cameras at any frame size, several per launch, the accumulation's state in a tensor the caller owns; and the host side of it in
quadray-engine_amd/rays.py (pt_seeds, pt_random).

Every comparison is bit for bit.  The truth of view j at w x h after N samples is always
    oracle.render_pt(_view_snapshot(base, view j, w, h), N, order="kernel", want_mean=True)       (depth= where a test sets one)
-- the oracle's path tracer in the fast kernel's order (tests/test_pt_oracle.py pins it) on the base snapshot rewritten to that
camera and size (tests/test_render_views.py): a fresh set_pt(True) followed by N render() calls on that snapshot.

Scenes: the two test18 path-tracer snapshots of tests/golden/pt and four ordinary fixtures with emission patched on
(tests/_ptpatch.py).  Cameras: _rayq.random_cameras(base, seed=crc32(tag), n=4).  test_inputs_discriminate checks on the oracle
alone that these inputs can tell a sample count, a draw order and a renderer apart.
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
import test_path_tracer as TPT
from conftest import ROOT
from test_render_views import _view_snapshot

SCENES = ["pt:test18_160_pt", "pt:test18_160_gf_aa4_pt", "patched:demo01_160", "patched:demo02_160_gf_aa4",
          "patched:demo03_160", "patched:test13_160_gf_aa4"]
SIZES = [(64, 64), (67, 45), (9, 130)]
ASM = os.path.join(ROOT, "quadray-engine_amd", "csrc", "qr_device-hip-amdgcn-amd-amdhsa-gfx950.s")
GUARD_LIB = os.path.join(ROOT, "quadray-engine_amd", "libqrhip_guard.so")
GUARD_CASE = ("patched:demo02_160_gf_aa4", 67, 45, 3)
ARG, UNSUP = -1, -3


def _rays_mod():
    import importlib
    from qr_loader import load_package
    load_package()
    return importlib.import_module("quadray_engine_amd.rays")


@pytest.fixture(scope="module")
def rays_mod():
    return _rays_mod()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _tag(scene):
    """the cameras' seed tag: the fixture name for the snapshots of tests/golden/pt, 'patched:<name>' for patched fixtures"""
    kind, n = scene.split(":")
    return n if kind == "pt" else scene


_BASE, _CAMS, _TRUTH, _STATS = {}, {}, {}, {}


def _base(scene):
    if scene not in _BASE:
        _BASE[scene] = TPT._scene_blob(scene)
    return _BASE[scene]


def _size(blob):
    fi, _ = _rayq.frame_words(blob)
    return int(fi[31]), int(fi[32])


def _fsaa(blob):
    return int(_rayq.frame_words(blob)[0][30])


def _cams(rm, scene):
    """the four seeded views of a scene, float32 [16] each"""
    if scene not in _CAMS:
        base = _base(scene)
        _CAMS[scene] = [rm.view_of(c) for c in _rayq.random_cameras(base, seed=zlib.crc32(_tag(scene).encode()), n=4)]
    return _CAMS[scene]


def _truth(oracle, scene, view, w, h, n, depth=None, order="kernel"):
    """(frame uint32 [h, w], mean float32 [h, w, 3]) of `view` after n samples by the oracle; computed once, read-only"""
    key = (scene, np.asarray(view, dtype=np.float32).tobytes(), w, h, n, depth, order)
    if key not in _TRUTH:
        snap = _view_snapshot(_base(scene), view, w, h)
        f, m, st = oracle.render_pt(snap, n, depth=-1 if depth is None else depth, order=order, threads=16, want_mean=True,
                                    want_stats=True)
        f.setflags(write=False); m.setflags(write=False)
        _TRUTH[key] = (f, m)
        _STATS[key] = st
    return _TRUTH[key]


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_pt_seeds_and_generator_give_the_oracles_first_draws(oracle, rays_mod):
    """rays.pt_seeds is the seed plane (slot (y * w + x) * 4 + k at 4x FSAA) and rays.pt_random the generator: the first two
    numbers they give for a sample are the jitter draws oracle.pt_trace_sample lists for it"""
    base = _base("pt:test18_160_gf_aa4_pt")
    w, h = _size(base)
    assert (w, h) == (160, 120) and _fsaa(base) == 2
    snap = _view_snapshot(base, rays_mod.view_of(base), w, h)
    seeds = rays_mod.pt_seeds(w, h, 4)
    assert seeds.dtype == np.uint32 and seeds.shape == (w * h * 4,)
    # the definition, slot by slot: a 48-bit LCG from 1, the low 32 bits of every state
    x, plain = 1, []
    for _ in range(3000):
        x = (x * 25214903917 + 11) & ((1 << 48) - 1)
        plain.append(x & 0xFFFFFFFF)
    assert (seeds[:3000] == np.array(plain, dtype=np.uint32)).all()
    assert (rays_mod.pt_seeds(67, 45, 1) == seeds[:67 * 45]).all() and (rays_mod.pt_seeds(9, 13, 2) == seeds[:9 * 13 * 2]).all()
    with pytest.raises(ValueError):
        rays_mod.pt_seeds(0, 4, 1)
    for x, y, k in ((0, 0, 0), (5, 3, 2), (159, 119, 3)):
        s0 = seeds[(y * w + x) * 4 + k]
        s1, v1 = rays_mod.pt_random(s0)
        s2, v2 = rays_mod.pt_random(s1)
        assert v1.dtype == np.float32 and s1.dtype == np.uint32
        assert int(s1) == (int(s0) * 214013 + 2531011) & 0xFFFFFFFF and int(s2) == (int(s1) * 214013 + 2531011) & 0xFFFFFFFF
        draws, _ = oracle.pt_trace_sample(snap, 1, x, y, k)
        assert [d[1] for d in draws[:2]] == ["jitter_h", "jitter_v"], draws[:2]
        got = _bits(np.array([v1, v2], dtype=np.float32))
        want = _bits(np.array([draws[0][2], draws[1][2]], dtype=np.float32))
        assert (got == want).all(), f"sample ({x}, {y}, {k}): {float(v1)}, {float(v2)} against the oracle's {draws[:2]}"
    # arrays of any shape
    s, v = rays_mod.pt_random(seeds[:24].reshape(2, 3, 4))
    assert s.shape == v.shape == (2, 3, 4) and (v >= 0).all() and (v < 1).all()


def test_pt_views_abi_and_constants(qr):
    """the library exports the three entry points, the header declares them, and its constants are the module's"""
    L = qr.lib()
    with open(os.path.join(ROOT, "include", "qrhip.h")) as f:
        hdr = f.read()
    for sym in ("qr_pt_views_state_bytes", "qr_pt_views_reset", "qr_pt_views_async"):
        assert hasattr(L, sym), sym
        assert sym in qr.ABI_SYMBOLS and f"int {sym}(" in hdr, sym
    assert f"#define QR_PT_VIEWS_MAX_SAMPLES {qr.PT_VIEWS_MAX_SAMPLES} " in hdr and qr.PT_VIEWS_MAX_SAMPLES == 512
    assert f"#define QR_PT_VIEWS_STATE_WORDS {qr.PT_VIEWS_STATE_WORDS} " in hdr and qr.PT_VIEWS_STATE_WORDS == 4
    assert hasattr(qr.Scene, "pt_views") and hasattr(qr, "PtViews")
    for m in ("step", "reset", "clone"):
        assert callable(getattr(qr.PtViews, m))


def test_pt_views_kernel_in_resource_check():
    """the build's register check lists the kernel at the path-tracer instance's budget (168 VGPRs: three waves per SIMD, its
    launch bound; nothing spilled) and the built assembly passes it"""
    import importlib.util
    path = os.path.join(ROOT, "tools", "check_kernel_resources.py")
    spec = importlib.util.spec_from_file_location("check_kernel_resources", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    frags = [f for f in m.LIMITS if "qr_pt_views_kernel" in f]
    assert len(frags) == 1
    vg, spill, scratch = m.LIMITS[frags[0]]
    assert vg == 168 and spill == 0 and scratch == 2128
    r = subprocess.run([sys.executable, path, ASM, "--print"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("qr_pt_views_kernel") == 1


@pytest.mark.parametrize("scene", SCENES)
def test_inputs_discriminate(oracle, rays_mod, scene):
    """A condition on the test inputs, checked with the oracle alone, at 64 x 64: for at least two of the four views each, the
    3-sample frame is non-black on >= 20 % of the pixels, the 1-sample and 3-sample frames differ on >= 3 %, the kernel order
    and the reference order differ on >= 3 %, and the ray-traced frame differs from the path-traced one on >= 50 %."""
    w, h = 64, 64
    lit, conv, order, rt = [], [], [], []
    for v in _cams(rays_mod, scene):
        f3 = _truth(oracle, scene, v, w, h, 3)[0]
        f1 = _truth(oracle, scene, v, w, h, 1)[0]
        r3 = _truth(oracle, scene, v, w, h, 3, order="reference")[0]
        ray, _, _ = oracle.render(_view_snapshot(_base(scene), v, w, h), threads=16)
        lit.append(float((f3 != 0).mean())); conv.append(float((f1 != f3).mean()))
        order.append(float((r3 != f3).mean())); rt.append(float((ray != f3).mean()))
    pc = lambda a: [round(100 * x, 1) for x in a]
    print(f"{scene}: non-black {pc(lit)} %, 1 vs 3 samples {pc(conv)} %, orders {pc(order)} %, ray-traced {pc(rt)} %")
    assert sum(x >= 0.20 for x in lit) >= 2, lit
    assert sum(x >= 0.03 for x in conv) >= 2, conv
    assert sum(x >= 0.03 for x in order) >= 2, order
    assert sum(x >= 0.50 for x in rt) >= 2, rt


def test_inputs_reach_every_branch_of_the_path_tracer(oracle, rays_mod):
    """over the six scenes' seeded views (64 x 64, 3 samples) every counter of oracle.PT_STATS is non-zero, and the scenes with
    glass split rays"""
    total = dict.fromkeys(oracle.PT_STATS, 0)
    glass = {}
    for scene in SCENES:
        for v in _cams(rays_mod, scene):
            _truth(oracle, scene, v, 64, 64, 3)
            st = _STATS[(scene, np.asarray(v, dtype=np.float32).tobytes(), 64, 64, 3, None, "kernel")]
            for k in total:
                total[k] += st[k]
            glass[scene] = glass.get(scene, 0) + st["split_reflect"] + st["split_refract"]
    print(total, glass)
    assert all(total[k] > 0 for k in total), total
    for scene in ("pt:test18_160_pt", "patched:demo02_160_gf_aa4", "patched:test13_160_gf_aa4"):
        assert glass[scene] > 0, scene


# ---------------------------------------------------------------------------------------------------------------- GPU

def _vt(scn, rows):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.stack(rows), dtype=np.float32)).to(f"cuda:{scn.device}")


def _step(acc, samples=1):
    """one launch; (frames uint32 [N, h, w], mean float32 [N, h, w, 3]) on the host"""
    import torch
    f, m = acc.step(samples, mean=True)
    torch.cuda.synchronize()
    return f.cpu().numpy().view(np.uint32), m.cpu().numpy()


def _state(acc):
    import torch
    torch.cuda.synchronize()
    return acc.state.cpu().numpy().copy()


def _same(got, wants, scene, w, h, what=""):
    """got: (frames, mean) of a launch; wants: per view (frame, mean)"""
    gf, gm = got
    assert gf.shape == (len(wants), h, w) and gm.shape == (len(wants), h, w, 3) and gm.dtype == np.float32
    bad = []
    for j, (wf, wm) in enumerate(wants):
        nf = int((gf[j] != wf).sum())
        nm = int((_bits(gm[j]) != _bits(wm)).any(axis=2).sum())
        if nf or nm:
            bad.append(f"{scene} view {j} at {w}x{h} {what}: {nf} of {w * h} pixels of the frame differ, {nm} of the mean")
    assert not bad, "; ".join(bad)


def _equal(a, b, what):
    (af, am), (bf, bm) = a, b
    nf, nm = int((af != bf).sum()), int((_bits(am) != _bits(bm)).any(axis=-1).sum())
    assert nf == 0 and nm == 0, f"{what}: {nf} pixels of the frames differ, {nm} of the means"


@pytest.mark.gpu
@pytest.mark.parametrize("scene,n", [("pt:test18_160_pt", 1), ("pt:test18_160_pt", 4), ("patched:demo02_160_gf_aa4", 3)])
def test_gpu_own_camera_own_size(qr, oracle, rays_mod, scene, n):
    """the snapshot's camera at the snapshot's size: the oracle's frame of the snapshot itself, and the frame set_pt(True)
    followed by n render() calls gives on the same GPU"""
    blob = _base(scene)
    w, h = _size(blob)
    scn = qr.Scene(blob, ray_queries=True)
    acc = scn.pt_views(_vt(scn, [rays_mod.view_of(blob)]))
    assert (acc.width, acc.height, acc.samples) == (w, h, 0)
    got = _step(acc, n)
    assert acc.samples == n
    f, m = oracle.render_pt(blob, n, order="kernel", threads=16, want_mean=True)
    _same(got, [(f, m)], scene, w, h, f"after {n} samples")
    own = TPT._gpu_frames(scn, n)
    scn.close()
    nd = int((got[0][0] != own).sum())
    assert nd == 0, f"{scene}: {nd} of {w * h} pixels differ from set_pt(True) + {n} x render()"


@pytest.mark.gpu
@pytest.mark.parametrize("scene", SCENES)
def test_gpu_seeded_views(qr, oracle, rays_mod, scene):
    """four seeded views in ONE launch per size, three samples in one call: frames and mean are the oracle's, view by view"""
    views = _cams(rays_mod, scene)
    scn = qr.Scene(_base(scene), ray_queries=True)
    got = {}
    for w, h in SIZES:
        got[w, h] = _step(scn.pt_views(_vt(scn, views), w, h), 3)
    scn.close()
    for w, h in SIZES:
        _same(got[w, h], [_truth(oracle, scene, v, w, h, 3) for v in views], scene, w, h)


@pytest.mark.gpu
@pytest.mark.parametrize("scene,depth", [("pt:test18_160_pt", 10), ("patched:demo02_160_gf_aa4", None)])
def test_gpu_splits(qr, oracle, rays_mod, scene, depth):
    """1+1+1+1+1, 2+3 and 5 samples in one call give equal frames, means and state bytes; 3+4 is the oracle's N = 7 (sample
    numbers 3, 5, 6 and 7: weights that are not exact in fp32)"""
    views = _cams(rays_mod, scene)
    scn = qr.Scene(_base(scene), ray_queries=True)
    if depth is not None:
        scn.set_depth(depth)
    vt = _vt(scn, views)
    res = {}
    for w, h in SIZES:
        runs = []
        for split in ((1, 1, 1, 1, 1), (2, 3), (5,)):
            acc = scn.pt_views(vt, w, h)
            for s in split:
                out = _step(acc, s)
            assert acc.samples == 5
            runs.append((out, _state(acc)))
        acc = scn.pt_views(vt, w, h)
        _step(acc, 3)
        res[w, h] = (runs, _step(acc, 4))
    scn.close()
    for w, h in SIZES:
        runs, seven = res[w, h]
        for (out, st), how in zip(runs[:2], ("1+1+1+1+1", "2+3")):
            _equal(out, runs[2][0], f"{scene} {w}x{h}: {how} against 5 in one call")
            nb = int((st != runs[2][1]).sum())
            assert nb == 0, f"{scene} {w}x{h}: {how} against 5 in one call: {nb} words of the state differ"
        _same(seven, [_truth(oracle, scene, v, w, h, 7, depth) for v in views], scene, w, h, "3+4 samples")


@pytest.mark.gpu
def test_gpu_depth_sweep(qr, oracle, rays_mod):
    """depths 0, 1, 3, 6 and 10 (the Fresnel split and the roulette switch on at levels 3 and 6) on the second seeded view: the
    first one sits inside an emitter and shows the same frame at every depth"""
    scene, (w, h) = "pt:test18_160_pt", (64, 64)
    v = _cams(rays_mod, scene)[1]
    scn = qr.Scene(_base(scene), ray_queries=True)
    got = {}
    for depth in (0, 1, 3, 6, 10):
        scn.set_depth(depth)
        got[depth] = _step(scn.pt_views(_vt(scn, [v]), w, h), 2)
    scn.close()
    for depth in got:
        _same(got[depth], [_truth(oracle, scene, v, w, h, 2, depth)], scene, w, h, f"depth {depth}")
    assert any((got[0][0] != got[d][0]).any() for d in (3, 6, 10)), "the depth does not show in the frames"


@pytest.mark.gpu
def test_gpu_checkpoint(qr, oracle, rays_mod):
    """clone() after 2 samples: original and copy, each continued by 2, are equal and the oracle's N = 4; reset() starts over"""
    scene, (w, h) = "pt:test18_160_gf_aa4_pt", (67, 45)
    views = _cams(rays_mod, scene)
    scn = qr.Scene(_base(scene), ray_queries=True)
    acc = scn.pt_views(_vt(scn, views), w, h)
    _step(acc, 2)
    cp = acc.clone()
    assert cp.samples == 2 and cp.state.data_ptr() != acc.state.data_ptr()
    a = _step(acc, 2)
    sa = _state(acc)
    b = _step(cp, 2)
    sb = _state(cp)
    # a state that left the device and came back, continued through Scene.pt_views(state=..., samples=...)
    import torch
    acc.reset()
    assert acc.samples == 0
    one = _step(acc, 1)
    back = scn.pt_views(_vt(scn, views), w, h, state=torch.from_numpy(sa).to("cuda:0"), samples=4)
    five_a = _step(back, 1)
    five_b = _step(cp, 1)
    scn.close()
    _equal(a, b, f"{scene}: original and clone after 2 + 2 samples")
    assert (sa == sb).all(), f"{scene}: {int((sa != sb).sum())} words of the two states differ"
    _same(a, [_truth(oracle, scene, v, w, h, 4) for v in views], scene, w, h, "2 + 2 samples")
    _same(one, [_truth(oracle, scene, v, w, h, 1) for v in views], scene, w, h, "after reset()")
    _equal(five_a, five_b, f"{scene}: a state restored from the host against the clone, fifth sample")
    assert sa.shape == (4, 4, w * h * 4)


@pytest.mark.gpu
def test_gpu_fresh_state_is_the_documented_layout(qr, rays_mod):
    scene, (w, h) = "pt:test18_160_gf_aa4_pt", (9, 130)
    views = _cams(rays_mod, scene)[:2]
    scn = qr.Scene(_base(scene), ray_queries=True)
    acc = scn.pt_views(_vt(scn, views), w, h)
    st = _state(acc)
    scn.close()
    seeds = rays_mod.pt_seeds(w, h, 4)
    assert st.shape == (2, 4, w * h * 4) and st.dtype == np.int32
    for j in range(2):
        assert (st[j, 0].view(np.uint32) == seeds).all(), "plane 0 of every view is the seed plane"
        assert (st[j, 1:] == 0).all()


@pytest.mark.gpu
def test_gpu_batch_independence(qr, rays_mod):
    """view j of a four-view launch is the same view launched alone (frames, mean, state), and views differ from each other"""
    scene, (w, h) = "patched:demo02_160_gf_aa4", (67, 45)
    views = _cams(rays_mod, scene)
    scn = qr.Scene(_base(scene), ray_queries=True)
    acc = scn.pt_views(_vt(scn, views), w, h)
    all4 = _step(acc, 3)
    st4 = _state(acc)
    for j, v in enumerate(views):
        alone = scn.pt_views(_vt(scn, [v]), w, h)
        one = _step(alone, 3)
        _equal((all4[0][j], all4[1][j]), (one[0][0], one[1][0]), f"{scene} view {j}: in a batch of four against alone")
        assert (st4[j] == _state(alone)[0]).all(), f"{scene} view {j}: the state differs"
    scn.close()
    ndiff = sum(bool((all4[0][i] != all4[0][j]).any()) for i in range(4) for j in range(i))
    assert ndiff >= 1, "all four views gave the same frame"


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["pt:test18_160_gf_aa4_pt", "pt:test18_160_pt"])
def test_gpu_bounds(qr, oracle, rays_mod, scene):
    """frames, mean and the state with sentinel-filled tails: reset and launch leave the tails alone (ragged sizes: partial
    footprints in both directions)"""
    import torch
    views = _cams(rays_mod, scene)
    ns = 1 << _fsaa(_base(scene))
    scn = qr.Scene(_base(scene), ray_queries=True)
    vt = _vt(scn, views)
    TAIL, SI, SF = 4096, 0x5A5A5A5A, 12345.0
    out = {}
    for w, h in SIZES[1:]:
        n_st, n_fr, n_mn = 4 * 4 * w * h * ns, 4 * w * h, 4 * w * h * 3
        st = torch.full((n_st + TAIL,), SI, dtype=torch.int32, device="cuda:0")
        fr = torch.full((n_fr + TAIL,), SI, dtype=torch.int32, device="cuda:0")
        mn = torch.full((n_mn + TAIL,), SF, dtype=torch.float32, device="cuda:0")
        acc = scn.pt_views(vt, w, h, state=st[:n_st].view(4, 4, w * h * ns), samples=0)
        acc.reset()
        f, m = acc.step(3, frames=fr[:n_fr].view(4, h, w), mean=mn[:n_mn].view(4, h, w, 3))
        torch.cuda.synchronize()
        assert f.data_ptr() == fr.data_ptr() and m.data_ptr() == mn.data_ptr()
        assert (st[n_st:] == SI).all() and (fr[n_fr:] == SI).all() and (mn[n_mn:] == SF).all(), f"{scene} {w}x{h}: a tail was written"
        assert not (st[:n_st].view(4, 4, -1)[:, 0] == SI).all()
        out[w, h] = (f.cpu().numpy().view(np.uint32), m.cpu().numpy())
    scn.close()
    for (w, h), got in out.items():
        _same(got, [_truth(oracle, scene, v, w, h, 3) for v in views], scene, w, h, "into sentinel-tailed buffers")


@pytest.mark.gpu
def test_gpu_independent_of_the_scenes_own_mode(qr, oracle, rays_mod):
    """set_pt(True), render(), a pt_views step, render(): the scene's second frame is the oracle's N = 2 of the snapshot (its
    planes and counter were left alone) and the view's frame the oracle's N = 1; with set_pt(False), render_views is as before"""
    import torch
    scene, (w, h) = "pt:test18_160_pt", (67, 45)
    blob = _base(scene)
    v = _cams(rays_mod, scene)[1]
    scn = qr.Scene(blob, ray_queries=True)
    vt = _vt(scn, [v])
    scn.set_pt(True)
    f = scn.new_frame()
    scn.render(f)
    acc = scn.pt_views(vt, w, h)
    got = _step(acc, 1)
    scn.render(f)
    torch.cuda.synchronize()
    second = f.cpu().numpy().view(np.uint32).copy()
    with pytest.raises(qr.QrError, match="path-tracer"):
        scn.render_views(vt, w, h)
    scn.set_pt(False)
    rv = scn.render_views(vt, w, h)
    off = _step(acc, 1)                                             # ... and the accumulation goes on with the mode off
    torch.cuda.synchronize()
    rv = rv.cpu().numpy().view(np.uint32)[0]
    scn.close()
    _same(got, [_truth(oracle, scene, v, w, h, 1)], scene, w, h, "with set_pt(True)")
    _same(off, [_truth(oracle, scene, v, w, h, 2)], scene, w, h, "second sample, after set_pt(False)")
    nd = int((second != oracle.render_pt(blob, 2, order="kernel", threads=16)).sum())
    assert nd == 0, f"{scene}: the scene's own second frame differs from the oracle's N = 2 on {nd} pixels"
    ray, _, _ = oracle.render(_view_snapshot(blob, v, w, h), threads=16)
    assert int((rv != ray).sum()) == 0, "render_views after set_pt(False) is not the ray-traced frame"


@pytest.mark.gpu
def test_gpu_scene_of_the_per_lane_instance(qr, oracle, rays_mod):
    """a scene whose ray-traced views the per-lane walk instance serves (long hierarchy): the path-traced view walks its lists
    with the packet instance, as set_pt(True) + render() does"""
    scene, (w, h) = "patched:synth_small", (64, 64)
    v = _cams(rays_mod, scene)[0]
    scn = qr.Scene(_base(scene), ray_queries=True)
    got = _step(scn.pt_views(_vt(scn, [v]), w, h), 2)
    scn.close()
    _same(got, [_truth(oracle, scene, v, w, h, 2)], scene, w, h)


@pytest.mark.gpu
def test_gpu_refusals(qr, oracle, rays_mod):
    import torch
    scene, (w, h) = "pt:test18_160_pt", (67, 45)
    blob = _base(scene)
    assert _fsaa(blob) == 0
    views = _cams(rays_mod, scene)[:2]
    L = qr.lib()
    dev = "cuda:0"
    vt = torch.from_numpy(np.stack(views)).to(dev)
    SI, SF = 0x5A5A5A5A, 12345.0
    fr = torch.full((2, h, w), SI, dtype=torch.int32, device=dev)
    mn = torch.full((2, h, w, 3), SF, dtype=torch.float32, device=dev)
    vp = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)

    plain = qr.Scene(blob)
    scn = qr.Scene(blob, ray_queries=True)
    acc = scn.pt_views(vt, w, h)
    st = acc.state
    before = _state(acc)

    def call(s, views=vp(vt), n=2, w=w, h=h, state=vp(st), done=0, samples=1, frames=vp(fr), mean=vp(mn), flags=0):
        return L.qr_pt_views_async(s, views, n, w, h, state, done, samples, frames, mean, flags, None)

    def refused(rc, want, text):
        assert rc == want and text in L.qr_last_error().decode(), (rc, L.qr_last_error().decode())

    refused(call(plain._h), UNSUP, "QR_UPLOAD_RAY_QUERIES")
    with pytest.raises(qr.QrError, match="QR_UPLOAD_RAY_QUERIES"):
        plain.pt_views(vt, w, h).step()
    plain.close()
    refused(call(None), ARG, "null scene")
    for kw in (dict(n=-1), dict(n=65536)):
        refused(call(scn._h, **kw), ARG, "view count")
    for kw in (dict(w=0), dict(h=0), dict(w=-5), dict(w=16385), dict(h=1 << 20)):
        refused(call(scn._h, **kw), ARG, "view frame size")
    refused(call(scn._h, n=65535, w=4096, h=4096), ARG, "QR_VIEW_MAX_WAVES")
    refused(call(scn._h, n=8, w=16384, h=16384), ARG, "2^30")                      # 2^31 slots in 2^25 footprints
    for kw in (dict(flags=1), dict(flags=0x80000000)):
        refused(call(scn._h, **kw), ARG, "flags")
    for kw in (dict(views=None), dict(state=None), dict(frames=None)):
        refused(call(scn._h, **kw), ARG, "null argument")
    for kw in (dict(views=vp(vt, 4)), dict(views=vp(vt, 8))):
        refused(call(scn._h, **kw), ARG, "16-byte aligned")
    for kw in (dict(state=vp(st, 2)), dict(frames=vp(fr, 1)), dict(mean=vp(mn, 2))):
        refused(call(scn._h, **kw), ARG, "4-byte aligned")
    for kw in (dict(samples=0), dict(samples=-1), dict(samples=513)):
        refused(call(scn._h, **kw), ARG, "samples must be")
    for kw in (dict(done=-1), dict(done=(1 << 24) - 1), dict(done=(1 << 24) - 512, samples=512), dict(done=1 << 30)):
        refused(call(scn._h, **kw), ARG, "done")
    # the size query and the reset refuse the same sizes
    nb = ctypes.c_uint64(7)
    assert L.qr_pt_views_state_bytes(scn._h, 2, w, h, ctypes.byref(nb)) == 0 and nb.value == 2 * 4 * w * h * 4
    assert L.qr_pt_views_state_bytes(scn._h, 2, 0, h, ctypes.byref(nb)) == ARG and nb.value == 2 * 4 * w * h * 4
    assert L.qr_pt_views_state_bytes(scn._h, 8, 16384, 16384, ctypes.byref(nb)) == ARG
    assert L.qr_pt_views_state_bytes(scn._h, 2, w, h, None) == ARG
    assert L.qr_pt_views_reset(scn._h, 2, w, h, None) == ARG and L.qr_pt_views_reset(scn._h, 2, w, 16385, vp(st)) == ARG
    assert L.qr_pt_views_reset(scn._h, 2, w, h, vp(st, 2)) == ARG and L.qr_pt_views_reset(None, 2, w, h, vp(st)) == ARG
    # the empty call: no launch
    assert call(scn._h, n=0) == 0 and call(scn._h, n=0, views=None, state=None, frames=None, mean=None) == 0
    torch.cuda.synchronize()
    assert (fr == SI).all() and (mn == SF).all() and (_state(acc) == before).all(), "a refused or empty call wrote something"

    # the Python object: a state of the wrong size, type or device
    good = st.clone()
    for bad in (good[:1], good[:, :3], good.reshape(-1), good.float(), good.cpu(), good.cpu().numpy(), good[:, :, ::2]):
        with pytest.raises(qr.QrError, match="state must be"):
            scn.pt_views(vt, w, h, state=bad, samples=0)
    with pytest.raises(qr.QrError, match="state must be"):
        scn.pt_views(vt, w + 1, h, state=good)
    with pytest.raises(qr.QrError, match="samples"):
        scn.pt_views(vt, w, h, state=good, samples=-1)
    with pytest.raises(qr.QrError, match="samples"):
        scn.pt_views(vt, w, h, samples=3)
    for bad in (vt.double(), vt[:, :15].contiguous(), vt.cpu(), vt.reshape(-1)):
        with pytest.raises(qr.QrError, match="views must be"):
            scn.pt_views(bad, w, h)
    for badf in (fr[:1], fr.float(), fr.cpu()):
        with pytest.raises(qr.QrError, match="frames must be"):
            acc.step(frames=badf)
    for badm in (mn[:1], mn.double(), mn.cpu()):
        with pytest.raises(qr.QrError, match="mean must be"):
            acc.step(mean=badm)
    for bads in (0, 513, -2):
        with pytest.raises(qr.QrError, match="samples must be"):
            acc.step(bads)
    with pytest.raises(qr.QrError, match="samples must be"):
        acc.step(1.5)
    assert acc.samples == 0
    torch.cuda.synchronize()
    assert (_state(acc) == before).all()

    got = _step(acc, 1)
    scn.close()
    _same(got, [_truth(oracle, scene, v, w, h, 1) for v in views], scene, w, h, "after the refusals")


# One case once more through the guarded diagnostic build (make guard: QR_STATS + QR_GUARD), as the other feature files do.  The
# library is chosen when the package is imported, hence the child process: this file run as a script.

def _guard_child():
    from qr_loader import load_package
    qr = load_package()
    assert qr.LIB_PATH == GUARD_LIB, qr.LIB_PATH
    import qr_oracle
    rm = _rays_mod()
    scene, w, h, n = GUARD_CASE
    views = _cams(rm, scene)
    scn = qr.Scene(_base(scene), ray_queries=True)
    got = _step(scn.pt_views(_vt(scn, views), w, h), n)
    scn.close()
    _same(got, [_truth(qr_oracle, scene, v, w, h, n) for v in views], scene, w, h, "guarded build")
    print(f"{scene} guard_ok 1", flush=True)
    return 0


@pytest.mark.gpu
def test_gpu_guarded_build_gives_the_same_path_traced_views():
    assert os.path.exists(GUARD_LIB), "libqrhip_guard.so is missing: build() makes it (make -C quadray-engine_amd/csrc guard)"
    env = dict(os.environ, QR_LIB=GUARD_LIB)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-child"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.count("guard_ok 1") == 1 and "QR_GUARD" not in out.stderr, out.stdout + out.stderr[-3000:]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.exit(_guard_child() if "--guard-child" in sys.argv else 2)
