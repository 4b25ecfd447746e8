"""View accumulation (include/qrhip.h qr_render_views_mean_async, Scene.render_views_mean): one frame that is the sum -- and,
scaled, the mean -- of many views, and the host side of it in quadray-engine_amd/rays.py (reduce_colors, pack_linear,
mean_of_views, jitter_view, thin_lens_views).

The truth of every GPU test is a composition of pieces that earlier tests pin one by one: rays.view_rays of every view and
sample -> oracle.trace_rays(..., "shade", depth) (the linear colour of a caller ray) -> rays.reduce_colors (clamp1 and the FSAA
reduce) -> rays.mean_of_views (the sum in view order and the output step on sum * scale).  Comparison is by bits: the sum as
uint32 words, the frame by value.

The views: five copies of one seeded camera (the first of _rayq.random_cameras(blob, SEED)) shifted by default_rng(SEED)
offsets within +-0.5 px.  test_inputs_discriminate checks on the oracle alone that they can tell a mean from a single view and
one summation order from another.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _rayq
import _rayset as RS
from conftest import ROOT, load_blob

SEED = 7
FSAA_CASES = ["demo01_160", "demo02_160_cam2_gf_aa2", "demo01_160_gf_aa4"]          # fsaa 0, 2x, 4x (the last two with gamma)
SIZES = [(64, 64), (67, 45), (9, 130)]
PER_LANE_CASES = ["synth_small", "swarm_demo01_240"]                                # scenes the per-lane walk instance serves
GUARD_CASES = ["synth_small", "synth_small_dda", "swarm_demo01_240"]
ASM = os.path.join(ROOT, "quadray-engine_amd", "csrc", "qr_device-hip-amdgcn-amd-amdhsa-gfx950.s")
GUARD_LIB = os.path.join(ROOT, "quadray-engine_amd", "libqrhip_guard.so")
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


def _scene_blob(name):
    return RS.scene_blob(name) if name in RS.SCENES else load_blob(name)


def _fsaa(blob):
    return int(_rayq.frame_words(blob)[0][30])


def _camera(rm, blob):
    """the seeded camera all view sets are built around"""
    return rm.view_of(_rayq.random_cameras(blob, seed=SEED, n=1)[0])


def _jittered(rm, blob, n=5):
    """n copies of the seeded camera shifted by seeded offsets within +-0.5 px"""
    cam = _camera(rm, blob)
    off = np.random.default_rng(SEED).uniform(-0.5, 0.5, (n, 2))
    return [rm.jitter_view(cam, dx, dy) for dx, dy in off]


_COL = {}


def _colour(oracle, rm, name, v, w, h, depth=None):
    """(reduced linear colour float32 [h*w, 3], sample 0's first-hit ids) of view v at w x h by the oracle; computed once"""
    key = (name, np.asarray(v, dtype=np.float32).tobytes(), w, h, depth)
    if key not in _COL:
        blob = _scene_blob(name)
        out = [oracle.trace_rays(blob, rm.view_rays(v, w, h, blob, k), "shade", depth, threads=16) for k in range(1 << _fsaa(blob))]
        c = rm.reduce_colors(np.stack([o[0] for o in out]), blob)
        c.setflags(write=False)
        _COL[key] = (c, out[0][1])
    return _COL[key]


def _truth(oracle, rm, name, views, w, h, scale, depth=None, start=None):
    """(frame, sum) of the composition"""
    cols = [_colour(oracle, rm, name, v, w, h, depth)[0] for v in views]
    return rm.mean_of_views(cols, _scene_blob(name), w, h, scale, start=start)


# ---------------------------------------------------------------------------------------------------------------- CPU

def _random_rgb(ns, n, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.5, 1.5, (ns, n, 3)).astype(np.float32)
    c[rng.uniform(size=c.shape) < 0.02] = np.nan
    c[rng.uniform(size=c.shape) < 0.02] = np.float32(7.5)
    c[rng.uniform(size=c.shape) < 0.02] = np.float32(-3.0)
    c[rng.uniform(size=c.shape) < 0.02] = np.float32(1.0)
    return c


@pytest.mark.parametrize("name", FSAA_CASES)
def test_reduce_then_pack_is_pack_colors(rays_mod, name):
    blob = load_blob(name)
    fi, _ = _rayq.frame_words(blob)
    fsaa, w, h = int(fi[30]), int(fi[31]), int(fi[32])
    assert fsaa == FSAA_CASES.index(name) and (fsaa == 0 or fi[28] & 0x40), "fixture: FSAA 0, 2x, 4x, the last two with gamma"
    rgb = _random_rgb(1 << fsaa, w * h, 3)
    assert np.isnan(rgb).any() and (rgb > 1).any() and (rgb < 0).any()
    with np.errstate(invalid="ignore"):
        want = rays_mod.pack_colors(rgb, blob)
    lin = rays_mod.reduce_colors(rgb, blob)
    assert lin.dtype == np.float32 and lin.shape == (w * h, 3)
    got = rays_mod.pack_linear(lin, blob, w, h)
    assert got.dtype == np.uint32 and got.shape == (h, w) and (got == want).all()
    if fsaa == 0:
        assert (_bits(rays_mod.reduce_colors(rgb[0], blob)) == _bits(lin)).all()      # [P, 3] is taken at fsaa 0
    # one view, scale 1: that packing, and the sum is the reduced colour
    f, s = rays_mod.mean_of_views([lin], blob, w, h, 1.0)
    assert (f == want).all() and s.shape == (h, w, 3) and (_bits(s).reshape(-1, 3) == _bits(lin)).all()
    with pytest.raises(ValueError):
        rays_mod.reduce_colors(rgb[:, :, :2], blob)
    with pytest.raises(ValueError):
        rays_mod.pack_linear(lin[:-1], blob, w, h)


def test_mean_of_views_split_with_start(rays_mod):
    """2 + 3 views with `start` = all 5 at once, bit for bit; and the sum is the in-order fp32 sum"""
    blob = load_blob("demo02_160_cam2_gf_aa2")
    w, h = 23, 11
    cols = [rays_mod.reduce_colors(np.abs(_random_rgb(2, w * h, 10 + j)), blob) for j in range(5)]
    scale = np.float32(1) / np.float32(5)
    f5, s5 = rays_mod.mean_of_views(cols, blob, w, h, scale)
    _, s2 = rays_mod.mean_of_views(cols[:2], blob, w, h, np.float32(0.5))
    f23, s23 = rays_mod.mean_of_views(cols[2:], blob, w, h, scale, start=s2)
    assert (_bits(s23) == _bits(s5)).all() and (f23 == f5).all()
    want = cols[0].copy()
    for c in cols[1:]:
        want = want + c
    assert (_bits(s5).reshape(-1, 3) == _bits(want)).all()
    assert (f5 == rays_mod.pack_linear(want * scale, blob, w, h)).all()
    rev = rays_mod.mean_of_views(cols[::-1], blob, w, h, scale)[1]
    assert (_bits(rev) != _bits(s5)).any(), "the order of the adds does not show: the inputs are too tame"
    with pytest.raises(ValueError):
        rays_mod.mean_of_views([], blob, w, h, 1.0)


def test_jitter_view(rays_mod):
    blob = load_blob("demo01_160")
    for cam in (rays_mod.view_of(blob), _camera(rays_mod, blob)):
        same = rays_mod.jitter_view(cam, 0.0, 0.0)
        assert same is not cam and same.dtype == np.float32 and (_bits(same) == _bits(cam)).all()
        w, h = 67, 45
        x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
        d, hor, ver = (cam[a:a + 3].astype(np.float64) for a in (4, 8, 12))
        for dx, dy in ((0.25, -0.4), (-0.5, 0.5), (0.0, 0.3)):
            j = rays_mod.jitter_view(cam, dx, dy)
            assert (_bits(j[[0, 1, 2, 3, 7, 8, 9, 10, 11, 12, 13, 14, 15]]) == _bits(cam[[0, 1, 2, 3, 7, 8, 9, 10, 11, 12, 13, 14, 15]])).all()
            got = rays_mod.view_rays(j, w, h, blob)[:, 4:7].astype(np.float64)
            want = d + hor * (x.reshape(-1, 1) + dx) + ver * (y.reshape(-1, 1) + dy)
            err = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
            assert err.max() < 1e-6, err.max()


def test_thin_lens_views(rays_mod):
    eye, target, up = (3.0, -2.0, 7.5), (-1.0, 4.0, 0.25), (0.0, 0.0, 1.0)
    w, h, fov = 67, 45, 50.0
    la = rays_mod.look_at(eye, target, up, fov, w, h)
    z = rays_mod.thin_lens_views(eye, target, up, fov, w, h, 0.0, 5.0, 4, seed=3)
    assert z.dtype == np.float32 and z.shape == (4, 16) and (_bits(z) == _bits(np.tile(la, (4, 1)))).all()
    aperture, focus, n = 0.8, 6.5, 12
    v = rays_mod.thin_lens_views(eye, target, up, fov, w, h, aperture, focus, n, seed=3)
    assert v.dtype == np.float32 and v.shape == (n, 16)
    assert (_bits(v) == _bits(rays_mod.thin_lens_views(eye, target, up, fov, w, h, aperture, focus, n, seed=3))).all()
    assert (_bits(v) != _bits(rays_mod.thin_lens_views(eye, target, up, fov, w, h, aperture, focus, n, seed=4))).any()
    fwd = np.subtract(target, eye, dtype=np.float64)
    fwd /= np.linalg.norm(fwd)
    off = v[:, 0:3].astype(np.float64) - np.float64(eye)
    r = np.linalg.norm(off, axis=1)
    assert (r <= aperture / 2 + 1e-6).all() and r.max() > aperture / 8 and len(np.unique(v[:, 0:3], axis=0)) == n
    assert np.abs(off @ fwd).max() < 1e-6
    assert (_bits(v[:, 8:16]) == _bits(la[8:16])).all() and (v[:, 3] == la[3]).all() and (v[:, 7] == la[7]).all()
    # through every pixel, the views' rays meet on the plane at distance `focus` along the viewing direction
    blob = load_blob("demo01_160")
    pts = []
    for row in v:
        rr = rays_mod.view_rays(row, w, h, blob).astype(np.float64)
        t = (focus - (rr[:, 0:3] - np.float64(eye)) @ fwd) / (rr[:, 4:7] @ fwd)
        pts.append(rr[:, 0:3] + rr[:, 4:7] * t[:, None])
    pts = np.stack(pts)
    assert np.linalg.norm(pts - pts[0], axis=2).max() < 1e-5 * focus
    # ... and nowhere else: at half the distance they are apart by about half the lens offsets
    assert np.linalg.norm((v[:, 0:3] + v[:, 4:7] * 0.5 * focus) - (v[0, 0:3] + v[0, 4:7] * 0.5 * focus), axis=1).max() > aperture / 16
    with pytest.raises(ValueError):
        rays_mod.thin_lens_views(eye, target, up, fov, w, h, aperture, 0.0, n, seed=3)


def test_mean_kernels_in_resource_check_and_abi(qr):
    """the build's register check holds the new instances to the view instances' budgets and the built assembly passes it; the
    header declares the entry point and the library exports it"""
    import importlib.util
    path = os.path.join(ROOT, "tools", "check_kernel_resources.py")
    spec = importlib.util.spec_from_file_location("check_kernel_resources", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    frags = sorted(f for f in m.LIMITS if "qr_views_mean_kernel" in f)
    views = sorted(f for f in m.LIMITS if "qr_render_views_kernel" in f)
    assert len(frags) == 2 and "ILb0ELi4EE" in frags[0] and "ILb1ELi3EE" in frags[1]
    assert [m.LIMITS[f] for f in frags] == [m.LIMITS[f] for f in views]
    assert m.LIMITS[frags[0]][0] == 128 and m.LIMITS[frags[1]][0] == 168
    r = subprocess.run([sys.executable, path, ASM, "--print"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("qr_views_mean_kernel") == 2
    with open(os.path.join(ROOT, "include", "qrhip.h")) as f:
        hdr = f.read()
    assert "int qr_render_views_mean_async(" in hdr and "#define QR_MEAN_RESUME 1u" in hdr
    assert "qr_render_views_mean_async" in qr.ABI_SYMBOLS and qr.MEAN_RESUME == 1
    assert hasattr(qr.lib(), "qr_render_views_mean_async") and hasattr(qr.Scene, "render_views_mean")


@pytest.mark.parametrize("name", FSAA_CASES)
def test_inputs_discriminate(oracle, rays_mod, name):
    """A condition on the test inputs, checked on the oracle alone: the mean frame of the five jittered views differs from every
    single view's frame on at least 1 % of the pixels (a kernel that returns one view, or drops one, cannot pass), and on the
    2x scene the reversed sum differs in bits from the forward one (a kernel that adds in another order cannot pass)."""
    blob = load_blob(name)
    w, h = 67, 45
    views = _jittered(rays_mod, blob)
    cols = [_colour(oracle, rays_mod, name, v, w, h)[0] for v in views]
    scale = np.float32(1) / np.float32(5)
    mean, s = rays_mod.mean_of_views(cols, blob, w, h, scale)
    frac = [float((rays_mod.pack_linear(c, blob, w, h) != mean).mean()) for c in cols]
    rev = rays_mod.mean_of_views(cols[::-1], blob, w, h, scale)[1]
    order = float((_bits(rev) != _bits(s)).any(axis=2).mean())
    print(f"{name}: mean differs from single views on {[round(100 * x, 1) for x in frac]} % of the pixels, "
          f"reversed sum on {100 * order:.1f} %")
    assert min(frac) >= 0.01, frac
    if name == "demo02_160_cam2_gf_aa2":
        assert order > 0, "forward and reversed sums agree everywhere"


# ---------------------------------------------------------------------------------------------------------------- GPU

def _vt(scn, rows):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.stack(rows), dtype=np.float32)).to(f"cuda:{scn.device}")


def _run(scn, rows, w, h, **kw):
    """(frame uint32 [h, w] or None, sum float32 [h, w, 3]) of one call, on the host"""
    import torch
    f, s = scn.render_views_mean(_vt(scn, rows), w, h, **kw)
    torch.cuda.synchronize()
    return (None if f is None else f.cpu().numpy().view(np.uint32)), s.cpu().numpy()


def _same(got, want, where):
    (gf, gs), (wf, ws) = got, want
    assert gs.shape == ws.shape and gs.dtype == np.float32
    nd = int((_bits(gs) != _bits(ws)).any(axis=2).sum())
    assert nd == 0, f"{where}: the sum differs on {nd} of {ws.shape[0] * ws.shape[1]} pixels"
    assert gf.shape == wf.shape and (gf == wf).all(), f"{where}: {int((gf != wf).sum())} of {wf.size} pixels of the frame differ"


def _scene(qr, name):
    if name in RS.SCENES:
        with RS.upload_env(name):
            return qr.Scene(RS.scene_blob(name), ray_queries=True)
    return qr.Scene(load_blob(name), ray_queries=True)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", FSAA_CASES)
def test_gpu_one_view(qr, oracle, rays_mod, name, size):
    """N = 1, scale 1: the frame is render_views' and the oracle's, the sum the reduced oracle colour"""
    import torch
    w, h = size
    v = _camera(rays_mod, load_blob(name))
    scn = _scene(qr, name)
    got = _run(scn, [v], w, h, scale=1.0)
    rv = scn.render_views(_vt(scn, [v]), w, h)
    torch.cuda.synchronize()
    scn.close()
    want = _truth(oracle, rays_mod, name, [v], w, h, 1.0)
    _same(got, want, f"{name} {w}x{h}")
    assert (_bits(want[1]).reshape(-1, 3) == _bits(_colour(oracle, rays_mod, name, v, w, h)[0])).all()
    assert (got[0] == rv.cpu().numpy().view(np.uint32)[0]).all(), "the frame of one view is not render_views' frame"


def _five_views(qr, oracle, rm, name, depth, sizes):
    blob = _scene_blob(name)
    views = _jittered(rm, blob)
    scn = _scene(qr, name)
    if depth is not None:
        scn.set_depth(depth)
    got = {s: _run(scn, views, *s) for s in sizes}                  # scale: float32(1) / float32(5) by default
    scn.close()
    hits = total = 0
    for (w, h) in sizes:
        _same(got[(w, h)], _truth(oracle, rm, name, views, w, h, np.float32(1) / np.float32(5), depth), f"{name} depth {depth} {w}x{h}")
        for v in views:
            ids = _colour(oracle, rm, name, v, w, h, depth)[1]
            hits += int((ids >= 0).sum()); total += ids.size
    # guards on the inputs: the views see scene and background, and the recursion contributes to some view's colour
    w, h = sizes[-1] if (67, 45) not in sizes else (67, 45)
    spawns = any((_bits(_colour(oracle, rm, name, v, w, h, depth)[0]) != _bits(_colour(oracle, rm, name, v, w, h, 0)[0])).any() for v in views)
    frac = hits / total
    print(f"{name} depth {depth}: hit fraction {frac:.3f}, secondary rays {spawns}")
    assert 0.05 <= frac <= 0.95, f"hit fraction {frac:.3f}: the views do not test much"
    assert spawns, "no view's colour depends on a reflection or refraction ray"


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [None, 3])
@pytest.mark.parametrize("name", FSAA_CASES)
def test_gpu_five_jittered_views(qr, oracle, rays_mod, name, depth):
    _five_views(qr, oracle, rays_mod, name, depth, SIZES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PER_LANE_CASES)
def test_gpu_five_jittered_views_per_lane_instance(qr, oracle, rays_mod, name):
    """scenes with long hierarchies: the instance with the per-lane walks (the three fixtures above take the packet instance)"""
    _five_views(qr, oracle, rays_mod, name, None, [(67, 45)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["demo02_160_cam2_gf_aa2", "demo01_160_gf_aa4"])
def test_gpu_resume(qr, oracle, rays_mod, name):
    """5 views as 5, as 2 + 3 and as 1 + 1 + 1 + 1 + 1: the same sum and the same final frame; the frame after 2 views with
    scale 1/2 is the composition of those 2"""
    import torch
    w, h = 67, 45
    views = _jittered(rays_mod, load_blob(name))
    fifth, half = np.float32(1) / np.float32(5), np.float32(0.5)
    want = _truth(oracle, rays_mod, name, views, w, h, fifth)
    scn = _scene(qr, name)
    vt = _vt(scn, views)
    _same(_run(scn, views, w, h), want, f"{name} 5")
    f2, s = scn.render_views_mean(vt[:2], w, h, scale=half)
    torch.cuda.synchronize()
    _same((f2.cpu().numpy().view(np.uint32), s.cpu().numpy()), _truth(oracle, rays_mod, name, views[:2], w, h, half), f"{name} 2")
    f, s2 = scn.render_views_mean(vt[2:], w, h, sum=s, scale=fifth, resume=True)
    torch.cuda.synchronize()
    assert s2.data_ptr() == s.data_ptr()
    _same((f.cpu().numpy().view(np.uint32), s.cpu().numpy()), want, f"{name} 2+3")
    f, s = scn.render_views_mean(vt[:1], w, h, frame=False)
    assert f is None
    for j in range(1, 5):
        f, s = scn.render_views_mean(vt[j:j + 1], w, h, sum=s, frame=(j == 4), scale=fifth, resume=True)
    torch.cuda.synchronize()
    scn.close()
    _same((f.cpu().numpy().view(np.uint32), s.cpu().numpy()), want, f"{name} 1+1+1+1+1")


@pytest.mark.gpu
def test_gpu_no_read_without_resume(qr, oracle, rays_mod):
    """a call without QR_MEAN_RESUME into a sum (and a frame) pre-filled with NaN (-1) shows no trace of the fill"""
    import torch
    name = "demo02_160_cam2_gf_aa2"
    w, h = 67, 45
    views = _jittered(rays_mod, load_blob(name))
    scn = _scene(qr, name)
    dev = f"cuda:{scn.device}"
    s = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device=dev)
    f = torch.full((h, w), -1, dtype=torch.int32, device=dev)
    f2, s2 = scn.render_views_mean(_vt(scn, views), w, h, sum=s, frame=f)
    torch.cuda.synchronize()
    scn.close()
    assert f2.data_ptr() == f.data_ptr() and s2.data_ptr() == s.data_ptr()
    got = (f.cpu().numpy().view(np.uint32), s.cpu().numpy())
    assert not np.isnan(got[1]).any()
    _same(got, _truth(oracle, rays_mod, name, views, w, h, np.float32(1) / np.float32(5)), name)


def _behind_and_far(rm, blob, w, h):
    """the seeded camera with t_min far below 0 (hits behind the origin count), and pulled back along its axis by 100 scene
    extents -- far beyond the image's reach -- and zoomed in by 50"""
    cam = _camera(rm, blob)
    lo, hi = _rayq.scene_box(blob)
    ext = max(float(np.max(hi - lo)), 1.0)
    behind = cam.copy()
    behind[3] = np.float32(-4.0 * ext)
    far = cam.copy()
    d, hor, ver = (cam[a:a + 3].astype(np.float64) for a in (4, 8, 12))
    fwd = d + hor * 32 + ver * 32                                   # random_cameras: unit axis, 64 x 64 frame
    hor, ver = hor / 50, ver / 50
    far[0:3] = cam[0:3].astype(np.float64) - fwd * (100.0 * ext)
    far[4:7], far[8:11], far[12:15] = fwd - hor * (w / 2) - ver * (h / 2), hor, ver
    return behind, far


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["demo01_160", "demo01_160_gf_aa4"])
def test_gpu_unlike_views_in_one_call(qr, oracle, rays_mod, name):
    """views that have nothing in common, one after the other in the same wave: three seeded cameras far apart; a view with
    t_min < 0 or a far origin first, and again last"""
    blob = load_blob(name)
    w, h = 67, 45
    cams = [rays_mod.view_of(c) for c in _rayq.random_cameras(blob, seed=SEED, n=3)]
    assert min(np.linalg.norm(cams[a][0:3] - cams[b][0:3]) for a, b in ((0, 1), (0, 2), (1, 2))) > 0.1
    behind, far = _behind_and_far(rays_mod, blob, w, h)
    assert (_colour(oracle, rays_mod, name, far, w, h)[1] >= 0).any(), "the far view sees nothing"
    sets = {"apart": cams, "behind first": [behind] + cams[:2], "behind last": cams[:2] + [behind],
            "far first": [far] + cams[1:], "far last": cams[1:] + [far]}
    scn = _scene(qr, name)
    got = {k: _run(scn, v, w, h) for k, v in sets.items()}
    scn.close()
    third = np.float32(1) / np.float32(3)
    for k, v in sets.items():
        _same(got[k], _truth(oracle, rays_mod, name, v, w, h, third), f"{name} {k}")
    assert (_bits(got["behind first"][1]) != _bits(got["apart"][1])).any()


@pytest.mark.gpu
def test_gpu_thin_lens_and_many_views(qr, oracle, rays_mod):
    """8 thin_lens_views at 64x64; 33 views at 16x16: more loop iterations than a wave has to give on a frame of four footprints"""
    name = "demo01_160"
    blob = load_blob(name)
    cam = _camera(rays_mod, blob)
    lo, hi = _rayq.scene_box(blob)
    eye, target = cam[0:3].astype(np.float64), (lo + hi) / 2
    focus = float(np.linalg.norm(target - eye))
    lens = list(rays_mod.thin_lens_views(eye, target, (0.0, 0.0, 1.0), 60.0, 64, 64, 0.05 * float(np.max(hi - lo)), focus, 8, seed=SEED))
    many = _jittered(rays_mod, blob, 33)
    scn = _scene(qr, name)
    got_lens = _run(scn, lens, 64, 64)
    got_many = _run(scn, many, 16, 16)
    scn.close()
    want_lens = _truth(oracle, rays_mod, name, lens, 64, 64, np.float32(1) / np.float32(8))
    one = rays_mod.pack_linear(_colour(oracle, rays_mod, name, lens[0], 64, 64)[0], blob, 64, 64)
    assert (want_lens[0] != one).mean() >= 0.01, "the lens does not blur: its mean is one view's frame"
    _same(got_lens, want_lens, "thin lens")
    _same(got_many, _truth(oracle, rays_mod, name, many, 16, 16, np.float32(1) / np.float32(33)), "33 views")


@pytest.mark.gpu
def test_gpu_determinism_and_side_effects(qr, oracle, rays_mod):
    import torch
    name = "demo02_160_cam2_gf_aa2"
    blob = load_blob(name)
    w, h = 67, 45
    views = _jittered(rays_mod, blob)
    other = [rays_mod.view_of(c) for c in _rayq.random_cameras(blob, seed=SEED, n=3)]
    fifth, third = np.float32(1) / np.float32(5), np.float32(1) / np.float32(3)
    scn = _scene(qr, name)
    dev = f"cuda:{scn.device}"
    vt, vo = _vt(scn, views), _vt(scn, other)
    before = (scn.render(), scn.render_views(vt, w, h))
    torch.cuda.synchronize()
    before = [t.cpu().numpy() for t in before]
    a = _run(scn, views, w, h)
    b = _run(scn, views, w, h)
    assert (a[0] == b[0]).all() and (_bits(a[1]) == _bits(b[1])).all()
    _same(a, _truth(oracle, rays_mod, name, views, w, h, fifth), name)
    # frame=False writes no frame: the only outputs are the returned sum
    f, s = scn.render_views_mean(vt, w, h, frame=False)
    torch.cuda.synchronize()
    assert f is None and (_bits(s.cpu().numpy()) == _bits(a[1])).all()
    # ... and through the C entry point a NULL frame leaves a sentinel-filled neighbour alone
    guard = torch.full((2, h, w, 3), 12345.0, dtype=torch.float32, device=dev)
    assert qr.lib().qr_render_views_mean_async(scn._h, ctypes.c_void_p(vt.data_ptr()), 5, w, h, ctypes.c_void_p(guard[0].data_ptr()), None,
                                               float("nan"), 0, scn._stream_ptr(None)) == 0        # scale is ignored without a frame
    torch.cuda.synchronize()
    g = guard.cpu().numpy()
    assert (_bits(g[0]) == _bits(a[1])).all() and (g[1] == 12345.0).all()
    # two streams, separate buffers
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    r1 = scn.render_views_mean(vt, w, h, stream=s1)
    r2 = scn.render_views_mean(vo, w, h, stream=s2)
    torch.cuda.synchronize()
    _same((r1[0].cpu().numpy().view(np.uint32), r1[1].cpu().numpy()), _truth(oracle, rays_mod, name, views, w, h, fifth), "stream 1")
    _same((r2[0].cpu().numpy().view(np.uint32), r2[1].cpu().numpy()), _truth(oracle, rays_mod, name, other, w, h, third), "stream 2")
    after = (scn.render(), scn.render_views(vt, w, h))
    torch.cuda.synchronize()
    scn.close()
    for x, y in zip(before, after):
        assert (x == y.cpu().numpy()).all(), "a view accumulation changed render() or render_views()"


@pytest.mark.gpu
def test_gpu_refusals(qr, oracle, rays_mod):
    import torch
    name = "demo01_160"
    blob = load_blob(name)
    L = qr.lib()
    w, h = 67, 45
    views = _jittered(rays_mod, blob, 2)
    dev = "cuda:0"
    vt = torch.from_numpy(np.stack(views)).to(dev)
    SENT = 12345.0
    sm = torch.full((h, w, 3), SENT, dtype=torch.float32, device=dev)
    fr = torch.full((h, w), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    vp = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)

    def call(s, views=vp(vt), n=2, w=w, h=h, sum=vp(sm), frame=vp(fr), scale=0.5, flags=0):
        return L.qr_render_views_mean_async(s, views, n, w, h, sum, frame, scale, flags, None)

    plain = qr.Scene(blob)
    with pytest.raises(qr.QrError, match="QR_UPLOAD_RAY_QUERIES"):
        plain.render_views_mean(vt, w, h)
    assert call(plain._h) == UNSUP
    plain.close()

    scn = qr.Scene(blob, ray_queries=True)
    assert call(None) == ARG
    assert call(scn._h, views=None) == ARG and call(scn._h, sum=None) == ARG
    assert call(scn._h, views=vp(vt, 4)) == ARG and call(scn._h, views=vp(vt, 8)) == ARG            # 16-byte alignment
    assert call(scn._h, sum=vp(sm, 2)) == ARG and call(scn._h, frame=vp(fr, 1)) == ARG              # 4-byte alignment
    assert call(scn._h, n=-1) == ARG and call(scn._h, n=65536) == ARG                               # QR_VIEW_MAX_VIEWS
    assert call(scn._h, w=0) == ARG and call(scn._h, h=0) == ARG and call(scn._h, w=-5) == ARG
    assert call(scn._h, w=16385) == ARG and call(scn._h, h=1 << 20) == ARG                          # QR_VIEW_MAX_DIM
    assert call(scn._h, flags=2) == ARG and call(scn._h, flags=3) == ARG and call(scn._h, flags=0x80000000) == ARG
    for bad in (0.0, -0.5, float("inf"), float("-inf"), float("nan")):
        assert call(scn._h, scale=bad) == ARG, bad
        assert call(scn._h, scale=bad, flags=1) == ARG, bad
    # the empty call: no launch, nothing written
    assert call(scn._h, n=0) == 0 and call(scn._h, n=0, views=None, sum=None, frame=None) == 0 and call(scn._h, n=0, flags=1) == 0
    torch.cuda.synchronize()
    assert (sm == SENT).all() and (fr == 0x5A5A5A5A).all(), "a refused or empty call wrote to its outputs"
    assert call(scn._h, frame=None, scale=float("nan")) == 0                                        # no frame: scale is ignored
    torch.cuda.synchronize()
    assert (fr == 0x5A5A5A5A).all() and not (sm == SENT).any()

    for bad in (vt.double(), vt[:, :15].contiguous(), vt.cpu(), vt[:, ::2], vt.reshape(-1), vt.cpu().numpy()):
        with pytest.raises(qr.QrError, match="views must be"):
            scn.render_views_mean(bad, w, h)
    for bw, bh in ((0, h), (w, -1), (w, 2.5), (16385, h)):
        with pytest.raises(qr.QrError):
            scn.render_views_mean(vt, bw, bh)
    for bads in (sm[:1], sm.double(), sm.cpu(), torch.zeros((w, h, 3), dtype=torch.float32, device=dev), sm[:, :, :2]):
        with pytest.raises(qr.QrError, match="sum must be"):
            scn.render_views_mean(vt, w, h, sum=bads)
    for badf in (fr[:1], fr.float(), fr.cpu(), torch.zeros((w, h), dtype=torch.int32, device=dev)):
        with pytest.raises(qr.QrError, match="frame must be"):
            scn.render_views_mean(vt, w, h, frame=badf)
    with pytest.raises(qr.QrError, match="resume"):
        scn.render_views_mean(vt, w, h, resume=True)                                                # no sum to resume from
    with pytest.raises(qr.QrError, match="scale"):
        scn.render_views_mean(vt, w, h, sum=sm, resume=True)                                        # a frame, but no scale
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(qr.QrError, match="scale"):
            scn.render_views_mean(vt, w, h, scale=bad)
    f, s = scn.render_views_mean(vt, w, h, sum=sm, frame=False, resume=True)                        # no frame: no scale needed
    assert f is None and s.data_ptr() == sm.data_ptr()
    f, s = scn.render_views_mean(vt[:0], w, h)
    assert tuple(f.shape) == (h, w) and tuple(s.shape) == (h, w, 3) and f.dtype == torch.int32 and s.dtype == torch.float32
    f, s = scn.render_views_mean(vt)                                                                # the snapshot's size by default
    assert tuple(f.shape) == (scn.height, scn.width) and tuple(s.shape) == (scn.height, scn.width, 3)
    torch.cuda.synchronize()

    scn.set_pt(True)
    with pytest.raises(qr.QrError, match="path-tracer"):
        scn.render_views_mean(vt, w, h)
    assert call(scn._h) == UNSUP
    scn.set_pt(False)
    _same(_run(scn, views, w, h), _truth(oracle, rays_mod, name, views, w, h, np.float32(0.5)), "after the refusals")
    scn.close()


# The five-view comparison once through the guarded diagnostic build (make guard: QR_STATS + QR_GUARD, every cell offset of the
# per-lane walks checked before it is loaded).  A guarded walk skips the cell it refuses, so a bad offset shows as a differing sum.
# The library is chosen when the package is imported, hence the child process: this file run as a script.

def _guard_child():
    from qr_loader import load_package
    qr = load_package()
    assert qr.LIB_PATH == GUARD_LIB, qr.LIB_PATH
    import qr_oracle
    rm = _rays_mod()
    done = 0
    for name in GUARD_CASES:
        blob = RS.scene_blob(name)
        views = _jittered(rm, blob)
        scn = _scene(qr, name)
        got = _run(scn, views, 67, 45)
        scn.close()
        _same(got, _truth(qr_oracle, rm, name, views, 67, 45, np.float32(1) / np.float32(5)), f"guard {name}")
        done += 1
        print(f"{name} guard_ok 1", flush=True)
    return 0 if done == len(GUARD_CASES) else 1


@pytest.mark.gpu
def test_gpu_guarded_build_gives_the_same_mean():
    assert os.path.exists(GUARD_LIB), "libqrhip_guard.so is missing: build() makes it (make -C quadray-engine_amd/csrc guard)"
    env = dict(os.environ, QR_LIB=GUARD_LIB)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-child"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.count("guard_ok 1") == len(GUARD_CASES) and "QR_GUARD" not in out.stderr, out.stdout + out.stderr[-3000:]


if __name__ == "__main__":
    sys.exit(_guard_child() if "--guard-child" in sys.argv else 2)
