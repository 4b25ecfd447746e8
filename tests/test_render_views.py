"""View rendering (include/qrhip.h qr_render_views_async, Scene.render_views): whole frames of the resident scene from
caller-supplied cameras at any frame size, and the host-side views of quadray-engine_amd/rays.py (view_of, look_at, view_rays).

The oracle of a view: the base snapshot with its frame record rewritten to the view's camera and the launch's size -- FSAA,
gamma and everything else kept -- and ONE tile holding the global list (_view_snapshot below, tests/_rayq.py one_tile),
rendered by oracle.render at the depth the scene is set to.  Its depth plane: oracle.trace_rays of sample 0's view_rays.
Every comparison is bit for bit.
"""
import ctypes
import os
import zlib

import numpy as np
import pytest

import _rayq
import _rayset as RS
from conftest import ROOT, load_blob, load_frame
from test_ray_query import NON_PT_SMALL, ORIGIN_CASES, _blob

ASM = os.path.join(ROOT, "quadray-engine_amd", "csrc", "qr_device-hip-amdgcn-amd-amdhsa-gfx950.s")
SIZES = [(64, 64), (67, 45), (9, 130), (200, 120)]
SEEDED = ORIGIN_CASES + ["demo01_160_gf_aa4", "demo02_160_cam2_gf_aa2", "demo01_160_aa2_t2500", "demo02_160_aa2_t2500"]
FSAA_CASES = ["demo01_160", "demo02_160_cam2_gf_aa2", "demo01_160_gf_aa4"]          # fsaa 0, 2x, 4x


@pytest.fixture(scope="module")
def rays_mod():
    import importlib
    from qr_loader import load_package
    load_package()
    return importlib.import_module("quadray_engine_amd.rays")


def _view_snapshot(base, view, w, h):
    """the base snapshot seen through `view` (a qr_view, float32 [16]) at w x h: camera and size rewritten, the whole frame in
    one call, everything else (FSAA, gamma, depth, t_max) kept; one tile with the global list"""
    b = bytearray(base)
    off = _rayq._hdr(b)[10]
    fi = np.frombuffer(b, dtype=np.int32, count=49, offset=off).copy()
    ff = fi.view(np.float32)
    v = np.asarray(view, dtype=np.float32)
    ff[25:28], ff[24], ff[1:4], ff[4:7], ff[7:10] = v[0:3], v[3], v[4:7], v[8:11], v[12:15]
    fi[31], fi[32], fi[33] = w, h, w                                # frm_w, frm_h, frm_row
    fi[39], fi[40] = 0, 1                                           # index, thnum
    b[off:off + 196] = fi.tobytes()
    return _rayq.one_tile(bytes(b))


def _size(blob):
    fi, _ = _rayq.frame_words(blob)
    return int(fi[31]), int(fi[32])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("name", FSAA_CASES)
def test_view_rays_of_own_camera_are_camera_rays(rays_mod, name):
    blob = load_blob(name)
    w, h = _size(blob)
    fsaa = int(_rayq.frame_words(blob)[0][30])
    assert fsaa == FSAA_CASES.index(name)
    v = rays_mod.view_of(blob)
    assert v.dtype == np.float32 and v.shape == (16,)
    for k in range(1 << fsaa):
        a, b = rays_mod.view_rays(v, w, h, blob, k), rays_mod.camera_rays(blob, k)
        assert a.dtype == np.float32 and a.shape == (w * h, 8)
        assert (a.view(np.uint32) == b.view(np.uint32)).all(), f"sample {k}"
    with pytest.raises(ValueError):
        rays_mod.view_rays(v, w, h, blob, 1 << fsaa)


def test_view_rays_other_size_and_offsets(rays_mod):
    """another size: pixel (x, y) of sample k is dir + hor * (x + hor_a) + ver * (y + ver_a) in the kernel's fp32 order, with
    the snapshot's sample offsets (2x: the offset index alternates with x)"""
    blob = load_blob("demo02_160_cam2_gf_aa2")
    _, ff = _rayq.frame_words(blob)
    v = rays_mod.view_of(load_blob("demo01_160"))
    r = rays_mod.view_rays(v, 7, 5, blob, 1)
    assert r.shape == (35, 8)
    for (x, y) in ((0, 0), (3, 2), (6, 4)):
        ai = (x & 1) * 2 + 1
        hs = np.float32(x) + ff[10 + ai]
        vs = np.float32(y) + ff[14 + ai]
        d = [(v[8 + c] * hs + v[12 + c] * vs) + v[4 + c] for c in range(3)]
        row = r[y * 7 + x]
        assert (_bits(row[4:7]) == _bits(d)).all() and (_bits(row[0:4]) == _bits(v[0:4])).all() and _bits(row[7:8]) == _bits(v[7:8])


@pytest.mark.parametrize("eye, target, up, fov, w, h", [
    ((0.0, 0.0, 0.0), (0.0, 0.0, -5.0), (0.0, 1.0, 0.0), 60.0, 64, 64),
    ((3.0, -2.0, 7.5), (-1.0, 4.0, 0.25), (0.0, 0.0, 1.0), 90.0, 1024, 1024),
    ((-12.0, 30.0, 4.0), (8.0, 1.0, -2.0), (0.3, 0.2, 1.0), 35.0, 200, 120),
    ((1.0, 1.0, 1.0), (1.5, 0.5, 40.0), (1.0, 0.0, 0.0), 40.0, 130, 10),
])
def test_look_at(rays_mod, eye, target, up, fov, w, h):
    """The frames stay below 2 in every component of the corner direction `dir`: the centre ray is then dir + hor * W/2 +
    ver * H/2 with five fp32 roundings of at most 2^-24 * 2 each per component, well inside the 1e-6 rad asked for (a very wide
    or very oblong frame has |dir| of 20 and more, and fp32 itself no longer resolves 1e-6 rad at its centre)."""
    v = rays_mod.look_at(eye, target, up, fov, w, h)
    assert v.dtype == np.float32 and v.shape == (16,)
    assert (v[0:3] == np.float32(eye)).all() and v[3] == 0.0 and v[7] == np.finfo(np.float32).max and v[11] == 0.0 and v[15] == 0.0
    d, hor, ver = (v[a:a + 3].astype(np.float64) for a in (4, 8, 12))
    fwd = np.subtract(target, eye, dtype=np.float64)
    fwd /= np.linalg.norm(fwd)
    # the ray through the centre of the frame (fsaa 0: no sample offset) points at the target
    blob = load_blob("demo01_160")
    c = rays_mod.view_rays(v, w, h, blob)[(h // 2) * w + w // 2, 4:7].astype(np.float64)
    ang = np.arctan2(np.linalg.norm(np.cross(c, fwd)), np.dot(c, fwd))
    assert ang < 1e-6, ang
    # orthogonal (as unit vectors), equal pixel pitch, the stated length, dir at the frame's corner
    uh, uv = hor / np.linalg.norm(hor), ver / np.linalg.norm(ver)
    assert abs(np.dot(uh, uv)) < 1e-6 and abs(np.dot(uh, fwd)) < 1e-6 and abs(np.dot(uv, fwd)) < 1e-6
    s = np.tan(np.radians(fov) / 2) / (w / 2)
    assert abs(np.linalg.norm(hor) / s - 1) < 1e-6 and abs(np.linalg.norm(ver) / s - 1) < 1e-6
    assert abs(np.linalg.norm(hor) / np.linalg.norm(ver) - 1) < 1e-6
    assert np.allclose(uv, np.cross(fwd, uh), atol=1e-6)
    want = fwd - hor * (w / 2) - ver * (h / 2)
    assert np.all(np.abs(d - want) <= 4 * np.spacing(np.float32(np.abs(want).max())))
    with pytest.raises(ValueError):
        rays_mod.look_at(eye, eye, up, fov, w, h)
    with pytest.raises(ValueError):
        rays_mod.look_at(eye, target, fwd, fov, w, h)


def test_view_kernels_in_resource_check():
    """the build's register check holds the view-rendering instances to the per-lane render instance's budget, and the build's
    assembly passes it"""
    import importlib.util
    import subprocess
    import sys
    path = os.path.join(ROOT, "tools", "check_kernel_resources.py")
    spec = importlib.util.spec_from_file_location("check_kernel_resources", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    divk = m.LIMITS["16qr_render_kernelILb0ELi3ELb1EE"]
    frags = sorted(f for f in m.LIMITS if "qr_render_views_kernel" in f)
    assert len(frags) == 2 and "ILb0ELi4EE" in frags[0] and "ILb1ELi3EE" in frags[1]
    assert m.LIMITS[frags[1]] == divk == (168, divk[1], 640)
    assert m.LIMITS[frags[0]] == (128, divk[1], 640)                # the packet-walk instance: 4 waves per SIMD
    r = subprocess.run([sys.executable, path, ASM, "--print"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("qr_render_views_kernel") == 2


@pytest.mark.parametrize("name", NON_PT_SMALL)
def test_view_snapshot_of_own_camera_is_the_golden_frame(oracle, rays_mod, name):
    """ties _view_snapshot, and with it every ground truth of the GPU tests, to the frames the reference rendered"""
    blob = load_blob(name)
    w, h = _size(blob)
    f, _, _ = oracle.render(_view_snapshot(blob, rays_mod.view_of(blob), w, h), threads=16)
    gold = load_frame(name)
    assert ((f & 0xFFFFFF) == (gold & 0xFFFFFF)).all(), f"{int(((f ^ gold) & 0xFFFFFF != 0).sum())} pixels differ"


# ---------------------------------------------------------------------------------------------------------------- GPU

def _views(scn, rows):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.stack(rows), dtype=np.float32)).to(f"cuda:{scn.device}")


def _render(scn, rows, w=None, h=None, **kw):
    """(frames uint32 [N, H, W], ids int32, depth float32) of one launch, on the host"""
    import torch
    f, i, d = scn.render_views(_views(scn, rows), w, h, ids=True, depth=True, **kw)
    torch.cuda.synchronize()
    return f.cpu().numpy().view(np.uint32), i.cpu().numpy(), d.cpu().numpy()


def _check_own_camera(qr, oracle, rays_mod, blob):
    w, h = _size(blob)
    v = rays_mod.view_of(blob)
    ref, ref_ids, _ = oracle.render(_view_snapshot(blob, v, w, h), threads=16, want_ids=True)
    scn = qr.Scene(blob, ray_queries=True)
    f, ids, _ = _render(scn, [v])
    scn.close()
    assert f.shape == (1, h, w)
    assert (f[0] == ref).all(), f"{int((f[0] != ref).sum())} of {ref.size} pixels differ"
    assert (ids[0] == ref_ids).all(), f"{int((ids[0] != ref_ids).sum())} ids differ"


@pytest.mark.gpu
@pytest.mark.parametrize("name", NON_PT_SMALL)
def test_gpu_own_camera_own_size(qr, oracle, rays_mod, name):
    _check_own_camera(qr, oracle, rays_mod, load_blob(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c2b_demo01_1080p", "c3_demo02_1080p_gf_d3"])
def test_gpu_own_camera_full_size(qr, oracle, rays_mod, name):
    _check_own_camera(qr, oracle, rays_mod, load_blob(name))


_SEEDED = {}
_DEPTHS = {}


def _seeded_views(rays_mod, name, n=8):
    base = RS.scene_blob(name) if name.startswith("crowd_") else _blob(name)      # a crowd of tests/_crowd.py, or a fixture
    return base, [rays_mod.view_of(c) for c in _rayq.random_cameras(base, seed=zlib.crc32(name.encode()), n=n)]


def _truth(oracle, rays_mod, name, depth, sizes=SIZES, n=8):
    """the seeded views of a fixture at every size, rendered by the oracle at `depth` (None: the snapshot's own):
    (base, views, {size: [(frame, ids, counts, depth plane) per view]})"""
    key = (name, depth, tuple(sizes), n)
    if key not in _SEEDED:
        base, views = _seeded_views(rays_mod, name, n)
        out = {}
        for (w, h) in sizes:
            per = []
            for j, v in enumerate(views):
                s = _view_snapshot(base, v, w, h)
                f, ids, cnt = oracle.render(s, depth=-1 if depth is None else depth, threads=16, want_ids=True)
                dk = (name, n, j, w, h)
                if dk not in _DEPTHS:                   # the first hit does not depend on the recursion depth
                    _DEPTHS[dk] = oracle.trace_rays(s, rays_mod.view_rays(v, w, h, base, 0), "trace", threads=16)[0].reshape(h, w)
                per.append((f, ids, cnt, _DEPTHS[dk]))
            out[(w, h)] = per
        _SEEDED[key] = (base, views, out)
    return _SEEDED[key]


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [None, 3])
@pytest.mark.parametrize("name", SEEDED)
def test_gpu_seeded_views_other_sizes(qr, oracle, rays_mod, name, depth):
    base, views, truth = _truth(oracle, rays_mod, name, depth)
    assert sum(1 for v in views if v[3] == 0.0) >= len(views) // 2
    scn = qr.Scene(base, ray_queries=True)
    if depth is not None:
        scn.set_depth(depth)
    got = {size: _render(scn, views, *size) for size in SIZES}         # all 8 views of one size in ONE launch
    scn.close()
    hits = total = 0
    spawns = False
    for (w, h) in SIZES:
        f, ids, dep = got[(w, h)]
        assert f.shape == ids.shape == dep.shape == (len(views), h, w)
        for j, (rf, ri, cnt, rd) in enumerate(truth[(w, h)]):
            where = f"{name} depth {depth} view {j} at {w}x{h}"
            assert (f[j] == rf).all(), f"{where}: {int((f[j] != rf).sum())} of {rf.size} pixels differ"
            assert (ids[j] == ri).all(), f"{where}: {int((ids[j] != ri).sum())} ids differ"
            assert (_bits(dep[j]) == _bits(rd)).all(), f"{where}: {int((_bits(dep[j]) != _bits(rd)).sum())} depths differ"
            hits += int((ri >= 0).sum()); total += ri.size
            spawns = spawns or cnt["reflect"] + cnt["refract"] > 0
    frac = hits / total
    print(f"{name} depth {depth}: hit fraction {frac:.3f}, secondary rays {spawns}")
    assert 0.05 <= frac <= 0.95, f"hit fraction {frac:.3f}: the views do not test much"
    assert spawns, "no view spawns a reflection or refraction ray"


def _behind_and_far(rays_mod, name, w, h):
    """views outside what the engine's cameras do: the first two seeded views with t_min far below 0 (hits behind the origin
    count), the next two pulled back along their axis by 100 scene extents -- far beyond the image's `reach` -- and zoomed in
    by 50, so that the scene still covers pixels"""
    base, views = _seeded_views(rays_mod, name)
    lo, hi = _rayq.scene_box(base)
    ext = max(float(np.max(hi - lo)), 1.0)
    out = []
    for j, v in enumerate(views[:4]):
        v = v.copy()
        if j < 2:
            v[3] = np.float32(-4.0 * ext)
        else:
            d, hor, ver = (v[a:a + 3].astype(np.float64) for a in (4, 8, 12))
            fwd = d + hor * 32 + ver * 32                               # random_cameras: unit axis, 64 x 64 frame
            hor, ver = hor / 50, ver / 50
            v[0:3] = v[0:3].astype(np.float64) - fwd * (100.0 * ext)
            v[4:7], v[8:11], v[12:15] = fwd - hor * (w / 2) - ver * (h / 2), hor, ver
        out.append(v)
    return base, out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["demo01_160", "synth_small", "swarm_demo01_240", "demo01_160_gf_aa4", "crowd_flat_dda"])
def test_gpu_views_behind_and_far_are_caller_rays(qr, oracle, rays_mod, name):
    """A view is caller input: with t_min < 0 or an origin beyond `reach` its rays behave as they do for shade -- the oracle's
    caller-ray restatement (oracle.trace_rays) of the view's rays, packed by the frame's output step, is the view's frame; its
    "trace" answers are the ids and the depth plane"""
    w, h = 67, 45
    base, views = _behind_and_far(rays_mod, name, w, h)
    ns = 1 << int(_rayq.frame_words(base)[0][30])
    if name in RS.SCENES:                       # crowd_flat_dda: engine-authored surfaces of every kind under a uniform grid
        with RS.upload_env(name):
            scn = qr.Scene(base, ray_queries=True)
    else:
        scn = qr.Scene(base, ray_queries=True)
    f, ids, dep = _render(scn, views, w, h)
    scn.close()
    hit = []
    for j, v in enumerate(views):
        s = _view_snapshot(base, v, w, h)
        rgb = np.stack([oracle.trace_rays(s, rays_mod.view_rays(v, w, h, base, k), "shade", threads=16)[0] for k in range(ns)])
        t, tid = oracle.trace_rays(s, rays_mod.view_rays(v, w, h, base, 0), "trace", threads=16)
        ref = rays_mod.pack_colors(rgb, s)
        assert (f[j] == ref).all(), f"{name} view {j}: {int((f[j] != ref).sum())} of {ref.size} pixels differ"
        assert (ids[j] == tid.reshape(h, w)).all() and (_bits(dep[j]) == _bits(t.reshape(h, w))).all(), f"{name} view {j}"
        hit.append(float((tid >= 0).mean()))
    print(f"{name}: hit fractions {hit}, negative depths {int((dep[:2] < 0).sum())}")
    assert all(x > 0 for x in hit), f"a view sees nothing: {hit}"
    assert (dep[:2] < 0).any(), "no hit behind an origin: the t_min < 0 views do not test that"


@pytest.mark.gpu
def test_gpu_batching_streams_and_bounds(qr, oracle, rays_mod):
    """N views in one launch = N launches of one view; two launches on two streams into disjoint frames = the sequential result;
    frames, ids and depth outside [0, N) of a larger buffer stay untouched"""
    import torch
    name = "demo02_160_cam2_gf_aa2"
    base, views = _seeded_views(rays_mod, name)
    w, h = 67, 45
    scn = qr.Scene(base, ray_queries=True)
    f, ids, dep = _render(scn, views, w, h)
    for j, v in enumerate(views):
        f1, i1, d1 = _render(scn, [v], w, h)
        assert (f1[0] == f[j]).all() and (i1[0] == ids[j]).all() and (_bits(d1[0]) == _bits(dep[j])).all(), f"view {j}"

    # a buffer of N + 2 frames, the launch writes frames 1 .. N through views of the tensors' storage
    n = len(views)
    SENT = 0x5A5A5A5A
    dev = f"cuda:{scn.device}"
    big = torch.full((n + 2, h, w), SENT, dtype=torch.int32, device=dev)
    vt = _views(scn, views)
    out = scn.render_views(vt, w, h, frames=big[1:n + 1])
    torch.cuda.synchronize()
    assert out.data_ptr() == big[1:n + 1].data_ptr()
    b = big.cpu().numpy().view(np.uint32)
    assert (b[0] == SENT).all() and (b[n + 1] == SENT).all() and (b[1:n + 1] == f).all()
    # ids and depth through the C entry point into sentinel-filled buffers
    L = qr.lib()
    bi = torch.full((n + 2, h, w), SENT, dtype=torch.int32, device=dev)
    bd = torch.full((n + 2, h, w), SENT, dtype=torch.int32, device=dev)
    bf = torch.full((n + 2, h, w), SENT, dtype=torch.int32, device=dev)
    step = h * w * 4
    assert L.qr_render_views_async(scn._h, ctypes.c_void_p(vt.data_ptr()), n, w, h, ctypes.c_void_p(bf.data_ptr() + step),
                                   ctypes.c_void_p(bi.data_ptr() + step), ctypes.c_void_p(bd.data_ptr() + step), 0,
                                   scn._stream_ptr(None)) == 0
    torch.cuda.synchronize()
    for t, ref in ((bf, f), (bi, ids.view(np.uint32)), (bd, _bits(dep))):
        a = t.cpu().numpy().view(np.uint32)
        assert (a[0] == SENT).all() and (a[n + 1] == SENT).all() and (a[1:n + 1] == ref).all()

    # two streams, disjoint halves of one buffer
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    both = torch.full((n, h, w), SENT, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    scn.render_views(vt[:n // 2], w, h, frames=both[:n // 2], stream=s1)
    scn.render_views(vt[n // 2:], w, h, frames=both[n // 2:], stream=s2)
    torch.cuda.synchronize()
    assert (both.cpu().numpy().view(np.uint32) == f).all()
    scn.close()


@pytest.mark.gpu
def test_gpu_agrees_with_ray_api(qr, oracle, rays_mod):
    """shade + pack_colors of the view's rays is the view's frame; trace of sample 0's rays its ids and depth"""
    import torch
    name = "demo01_160_gf_aa4"
    base, views = _seeded_views(rays_mod, name)
    w, h = 67, 45
    scn = qr.Scene(base, ray_queries=True)
    f, ids, dep = _render(scn, views[:3] + views[-1:], w, h)
    for j, v in enumerate(views[:3] + views[-1:]):
        rgb = []
        for k in range(4):
            r = torch.from_numpy(rays_mod.view_rays(v, w, h, base, k)).to(f"cuda:{scn.device}")
            rgb.append(scn.shade(r, coherent=True).cpu().numpy())
        packed = rays_mod.pack_colors(np.stack(rgb), _view_snapshot(base, v, w, h))
        assert (packed == f[j]).all(), f"view {j}: {int((packed != f[j]).sum())} pixels differ from shade + pack_colors"
        t, tid = scn.trace(torch.from_numpy(rays_mod.view_rays(v, w, h, base, 0)).to(f"cuda:{scn.device}"))
        torch.cuda.synchronize()
        assert (tid.cpu().numpy().reshape(h, w) == ids[j]).all()
        assert (_bits(t.cpu().numpy().reshape(h, w)) == _bits(dep[j])).all()
    scn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [0, 1, 2, 5, 10])
def test_gpu_view_depth_sweep(qr, oracle, rays_mod, depth):
    name = "demo02_160_cam2_gf_aa2"                                     # gamma, Fresnel, 2x FSAA
    size = (67, 45)
    base, views, truth = _truth(oracle, rays_mod, name, depth, sizes=[size], n=2)
    if depth > 0:
        assert any(c[2]["reflect"] > 0 for c in truth[size]) and any(c[2]["refract"] > 0 for c in truth[size])
    scn = qr.Scene(base, ray_queries=True)
    scn.set_depth(depth)
    f, ids, dep = _render(scn, views, *size)
    scn.close()
    for j, (rf, ri, _, rd) in enumerate(truth[size]):
        assert (f[j] == rf).all(), f"depth {depth} view {j}: {int((f[j] != rf).sum())} pixels differ"
        assert (ids[j] == ri).all() and (_bits(dep[j]) == _bits(rd)).all()


@pytest.mark.gpu
def test_gpu_refusals_and_no_side_effects(qr, oracle, rays_mod):
    import torch
    name = "demo01_160"
    blob = load_blob(name)
    L = qr.lib()
    w, h = 67, 45
    base, views, truth = _truth(oracle, rays_mod, name, None, sizes=[(w, h)], n=2)
    ref_render, _, _ = oracle.render(blob, threads=16)
    dev = "cuda:0"
    vt = torch.from_numpy(np.stack(views)).to(dev)
    fr = torch.zeros((2, h, w), dtype=torch.int32, device=dev)
    ids = torch.zeros((2, h, w), dtype=torch.int32, device=dev)
    dep = torch.zeros((2, h, w), dtype=torch.float32, device=dev)
    vp = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)
    ARG, UNSUP = -1, -3

    def call(s, views=vp(vt), n=2, w=w, h=h, frames=vp(fr), i=vp(ids), d=vp(dep), flags=0):
        return L.qr_render_views_async(s, views, n, w, h, frames, i, d, flags, None)

    plain = qr.Scene(blob)
    with pytest.raises(qr.QrError, match="QR_UPLOAD_RAY_QUERIES"):
        plain.render_views(vt, w, h)
    assert call(plain._h) == UNSUP
    plain.close()

    scn = qr.Scene(blob, ray_queries=True)

    def still_right():
        f, i, d = _render(scn, views, w, h)
        for j, (rf, ri, _, rd) in enumerate(truth[(w, h)]):
            assert (f[j] == rf).all() and (i[j] == ri).all() and (_bits(d[j]) == _bits(rd)).all()
        out = scn.render()
        torch.cuda.synchronize()
        assert (out.cpu().numpy().view(np.uint32) == ref_render).all()

    # ordinary results before any view launch
    rays = torch.from_numpy(rays_mod.camera_rays(blob)).to(dev)
    before = (scn.render(), *scn.trace(rays), scn.occluded(rays), scn.shade(rays))
    torch.cuda.synchronize()
    before = [t.cpu().numpy() for t in before]

    assert call(None) == ARG
    assert call(scn._h, views=None) == ARG
    assert call(scn._h, frames=None) == ARG
    assert call(scn._h, views=vp(vt, 4)) == ARG and call(scn._h, views=vp(vt, 8)) == ARG            # 16-byte alignment
    assert call(scn._h, frames=vp(fr, 2)) == ARG and call(scn._h, i=vp(ids, 1)) == ARG and call(scn._h, d=vp(dep, 2)) == ARG
    assert call(scn._h, n=-1) == ARG
    assert call(scn._h, w=0) == ARG and call(scn._h, h=0) == ARG and call(scn._h, w=-5) == ARG
    assert call(scn._h, w=16385) == ARG and call(scn._h, h=1 << 20) == ARG                          # QR_VIEW_MAX_DIM
    assert call(scn._h, n=65536) == ARG                                                             # QR_VIEW_MAX_VIEWS
    assert call(scn._h, n=65535, w=16384, h=16384) == ARG                                           # beyond one grid
    assert call(scn._h, flags=1) == ARG and call(scn._h, flags=0x80000000) == ARG
    assert call(scn._h, n=0) == 0 and call(scn._h, n=0, views=None, frames=None, i=None, d=None) == 0
    assert call(scn._h, i=None, d=None) == 0                                                        # the extras are optional
    torch.cuda.synchronize()
    for bad in (vt.double(), vt[:, :15].contiguous(), vt.cpu(), vt[:, ::2], vt.reshape(-1), vt.cpu().numpy()):
        with pytest.raises(qr.QrError, match="views must be"):
            scn.render_views(bad, w, h)
    for bw, bh in ((0, h), (w, -1), (w, 2.5), (16385, h)):
        with pytest.raises(qr.QrError):
            scn.render_views(vt, bw, bh)
    for badf in (fr[:1], fr.float(), fr.cpu(), torch.zeros((2, w, h), dtype=torch.int32, device=dev)):
        with pytest.raises(qr.QrError, match="frames must be"):
            scn.render_views(vt, w, h, frames=badf)
    e = scn.render_views(vt[:0], w, h)
    assert tuple(e.shape) == (0, h, w) and e.dtype == torch.int32
    d0 = scn.render_views(vt)                                           # the snapshot's size by default
    assert tuple(d0.shape) == (2, scn.height, scn.width)
    still_right()

    scn.set_pt(True)
    with pytest.raises(qr.QrError, match="path-tracer"):
        scn.render_views(vt, w, h)
    assert call(scn._h) == UNSUP
    scn.set_pt(False)
    still_right()

    after = (scn.render(), *scn.trace(rays), scn.occluded(rays), scn.shade(rays))
    torch.cuda.synchronize()
    for a, b in zip(before, after):
        b = b.cpu().numpy()
        assert a.dtype == b.dtype and (a.view(np.uint8) == b.view(np.uint8)).all(), "a view launch changed an ordinary result"
    scn.close()
