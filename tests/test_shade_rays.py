"""Ray shading (include/qrhip.h qr_shade_rays_async, Scene.shade): the renderer's colour for caller-supplied rays, and
rays.pack_colors, the frame's output step for those colours.

The oracle: shading the camera rays of every FSAA sample of a snapshot and packing the colours gives the frame that a walk of
the global list renders -- oracle.render of the snapshot with ONE tile holding that list (tests/_rayq.py one_tile), at the
snapshot's own FSAA, depth, Gamma and Fresnel.  Other cameras: _rayq.random_cameras / with_frame, rendered by the oracle at the
depth the scene is set to.
"""
import ctypes
import os
import zlib

import numpy as np
import pytest

import _rayq
from conftest import ROOT, load_blob
from test_ray_query import NON_PT_SMALL, ORIGIN_CASES, _blob

ASM = os.path.join(ROOT, "quadray-engine_amd", "csrc", "qr_device-hip-amdgcn-amd-amdhsa-gfx950.s")


@pytest.fixture(scope="module")
def rays_mod():
    import importlib
    from qr_loader import load_package
    load_package()
    return importlib.import_module("quadray_engine_amd.rays")


def _frame_blob(w, h, fsaa=0, gamma=False, clamp=255.0, cmask=0xFF):
    """a snapshot whose frame record is w x h with the given output-step fields (pack_colors reads nothing else)"""
    b = bytearray(_rayq.with_frame(load_blob("demo01_160"), w=w, h=h))
    off = _rayq._hdr(b)[10]
    fi = np.frombuffer(b, dtype=np.int32, count=49, offset=off).copy()
    ff = fi.view(np.float32)
    fi[30] = fsaa
    fi[28] = _rayq.frame_words(load_blob("demo01_160"))[0][28] & ~0x40 | (0x40 if gamma else 0)
    ff[18] = np.float32(clamp)
    fi[19] = cmask
    b[off:off + 196] = fi.tobytes()
    return bytes(b)


def _px(r, g, b):
    return (r << 16) | (g << 8) | b


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_pack_colors_no_fsaa(rays_mod):
    """clamp1 (values above 1 and NaN give 1, negatives pass), * clamp, round to nearest even, pack"""
    blob = _frame_blob(3, 2)
    rgb = np.float32([[0.0, 0.5, 1.0],                      # 127.5 rounds to even: 128
                      [2.0, 1e30, np.inf],                  # clamped
                      [np.nan, 0.25, 1.5 / 255],            # NaN -> 1; 63.75 -> 64; 1.5 -> 2
                      [2.5 / 255, 0.999, 0.1],              # 2.5 -> 2 (even); 254.745 -> 255; 25.5 -> 26 (25.500000372...)
                      [0.0, 0.0, 0.0],
                      [1.0, 1.0, 1.0]])
    f = rays_mod.pack_colors(rgb, blob)
    assert f.dtype == np.uint32 and f.shape == (2, 3)
    assert f.reshape(-1).tolist() == [_px(0, 128, 255), _px(255, 255, 255), _px(255, 64, 2), _px(2, 255, 26), 0, 0xFFFFFF]
    # the [ns, H*W, 3] form with ns = 1 is the same
    assert (rays_mod.pack_colors(rgb[None], blob) == f).all()


def test_pack_colors_gamma(rays_mod):
    """the square root comes after the clamp, before the scale"""
    rgb = np.float32([[0.25, 0.5, 4.0], [0.01, 0.0, 0.81]])
    on = rays_mod.pack_colors(rgb, _frame_blob(2, 1, gamma=True))
    off = rays_mod.pack_colors(rgb, _frame_blob(2, 1, gamma=False))
    # sqrt(0.25) * 255 = 127.5 -> 128; sqrt(0.5) * 255 = 180.31 -> 180; 4 -> 1 -> 255; sqrt(0.01) = 0.1 -> 25.5 -> 26 (float32
    # 0.1 * 255 = 25.500000...); sqrt(0.81) * 255 = 229.5 -> 230 (float32 rounding above .5)
    assert on.reshape(-1).tolist() == [_px(128, 180, 255), _px(26, 0, 230)]
    assert off.reshape(-1).tolist() == [_px(64, 128, 255), _px(3, 0, 207)]


def test_pack_colors_2x_reduce(rays_mod):
    """2x: each sample clamped first, then * 0.5 and added; gamma after the reduce"""
    s0 = np.float32([[1.5, 0.25, 0.3]])
    s1 = np.float32([[0.0, 1.0, 0.1]])
    rgb = np.stack([s0, s1])
    f = rays_mod.pack_colors(rgb, _frame_blob(1, 1, fsaa=1))
    # r: clamp(1.5) = 1 -> 0.5 + 0 = 0.5 -> 128 (a reduce before the clamp would give 0.75 -> 191)
    # g: 0.125 + 0.5 = 0.625 -> 159.375 -> 159; b: 0.15 + 0.05 = 0.2 -> 51
    assert f.reshape(-1).tolist() == [_px(128, 159, 51)]
    g = rays_mod.pack_colors(rgb, _frame_blob(1, 1, fsaa=1, gamma=True))
    # gamma after the reduce: sqrt(0.625) * 255 = 201.6 -> 202 (before it: (0.5 + 1) / 2 * 255 = 191)
    assert g.reshape(-1)[0] >> 8 & 0xFF == 202
    with pytest.raises(ValueError):
        rays_mod.pack_colors(s0, _frame_blob(1, 1, fsaa=1))           # one sample for a 2x frame


def test_pack_colors_4x_reduce_order(rays_mod):
    """4x: ((s0 / 2 + s1 / 2) / 2) + ((s2 / 2 + s3 / 2) / 2) in fp32.  The values are chosen so that the running sum
    (((s0 + s1) + s2) + s3) / 4 rounds to another byte: 185 against 186"""
    v = np.float32([0.70969146, 0.747002, 0.7821375, 0.67097276])
    h = np.float32(0.5)
    pairwise = ((v[0] * h + v[1] * h) * h) + ((v[2] * h + v[3] * h) * h)
    running = (((v[0] * h + v[1] * h) * h + v[2] * h * h) + v[3] * h * h)
    assert int(np.rint(pairwise * np.float32(255))) == 185 and int(np.rint(running * np.float32(255))) == 186
    rgb = np.zeros((4, 2, 3), dtype=np.float32)
    rgb[:, 0, 0] = v                                                  # pixel 0, red
    rgb[:, 1, 2] = v[::-1]                                            # pixel 1, blue: the pairs are (s3, s2), (s1, s0)
    rgb[:, 0, 1] = [4.0, 0.5, -1.0, 0.25]                             # clamp per sample: (0.5 + 0.25) / 2 + (-0.5 + 0.125) / 2 -> 0.1875
    f = rays_mod.pack_colors(rgb, _frame_blob(2, 1, fsaa=2))
    assert f.reshape(-1).tolist() == [_px(185, 48, 0), _px(0, 0, 185)]


def test_pack_colors_cmask_and_scale(rays_mod):
    """another scale and cmask: the mask applies to the rounded integer (negatives in two's complement)"""
    rgb = np.float32([[1.0, 0.5, -0.01], [0.2, 0.7, 0.0]])
    f = rays_mod.pack_colors(rgb, _frame_blob(2, 1, clamp=127.0, cmask=0x7E))
    # 127 & 0x7E = 126; 63.5 -> 64 & 0x7E = 64; -1.27 -> -1 & 0x7E = 126; 25.4 -> 25 & 0x7E = 24; 88.9 -> 89 & 0x7E = 88
    assert f.reshape(-1).tolist() == [_px(126, 64, 126), _px(24, 88, 0)]


def test_pack_colors_refuses_wrong_shapes(rays_mod):
    blob = _frame_blob(2, 2, fsaa=1)
    for bad in (np.zeros((4, 3), np.float32), np.zeros((2, 4, 3), np.float64), np.zeros((4, 4, 3), np.float32),
                np.zeros((2, 3, 3), np.float32)):
        with pytest.raises(ValueError):
            rays_mod.pack_colors(bad, blob)


def test_shade_kernels_in_resource_check():
    """the build's register check holds both ray-shading instances to the per-lane render instance's budget, and the
    build's assembly passes it"""
    import importlib.util
    import subprocess
    import sys
    path = os.path.join(ROOT, "tools", "check_kernel_resources.py")
    spec = importlib.util.spec_from_file_location("check_kernel_resources", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    divk = m.LIMITS["16qr_render_kernelILb0ELi3ELb1EE"]
    for frag in ("20qr_shade_rays_kernelILb0EE", "20qr_shade_rays_kernelILb1EE"):
        assert frag in m.LIMITS and m.LIMITS[frag] == divk, frag
    r = subprocess.run([sys.executable, path, ASM, "--print"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("qr_shade_rays_kernel") == 2


# ---------------------------------------------------------------------------------------------------------------- GPU

def _cuda(scn, rays_np):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rays_np, dtype=np.float32)).to(f"cuda:{scn.device}")


def _shade(scn, rays_np, coherent=False):
    import torch
    rgb, ids = scn.shade(_cuda(scn, rays_np), coherent=coherent, ids=True)
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), ids.cpu().numpy()


def _shaded_frame(rays_mod, scn, blob, coherent=False):
    """(packed frame of the camera rays of every FSAA sample, sample 0's first-hit ids, the raw colours [ns, H*W, 3])"""
    ns = 1 << int(_rayq.frame_words(blob)[0][30])
    rgb, ids = zip(*[_shade(scn, rays_mod.camera_rays(blob, sample=k), coherent) for k in range(ns)])
    rgb = np.stack(rgb)
    return rays_mod.pack_colors(rgb, blob), ids[0], rgb


def _check_camera_frame(qr, oracle, rays_mod, blob):
    ref, ref_ids, _ = oracle.render(_rayq.one_tile(blob), threads=16, want_ids=True)
    scn = qr.Scene(blob, ray_queries=True)
    f0, i0, c0 = _shaded_frame(rays_mod, scn, blob, coherent=False)
    f1, i1, c1 = _shaded_frame(rays_mod, scn, blob, coherent=True)
    scn.close()
    assert (f0 == ref).all(), f"{int((f0 != ref).sum())} of {ref.size} pixels differ"
    assert (i0 == ref_ids.reshape(-1)).all(), f"{int((i0 != ref_ids.reshape(-1)).sum())} ids differ"
    assert (c0.view(np.uint32) == c1.view(np.uint32)).all() and (i0 == i1).all(), "QR_TRACE_COHERENT changed a result"


@pytest.mark.gpu
@pytest.mark.parametrize("name", NON_PT_SMALL)
def test_gpu_camera_rays_shade_to_oracle_frame(qr, oracle, rays_mod, name):
    _check_camera_frame(qr, oracle, rays_mod, load_blob(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c2b_demo01_1080p", "c3_demo02_1080p_gf_d3"])
def test_gpu_camera_rays_shade_to_oracle_frame_full_size(qr, oracle, rays_mod, name):
    _check_camera_frame(qr, oracle, rays_mod, load_blob(name))


_CAMS = {}


def _cameras(oracle, rays_mod, name, depth):
    """the 8 seeded cameras of a fixture: [(camera snapshot, its rays, oracle frame, oracle ids, oracle counts)]"""
    key = (name, depth)
    if key not in _CAMS:
        base = _blob(name)
        out = []
        for cam in _rayq.random_cameras(base, seed=zlib.crc32(name.encode())):
            f, ids, cnt = oracle.render(cam, depth=depth, threads=16, want_ids=True)
            out.append((cam, rays_mod.camera_rays(cam), f, ids.reshape(-1), cnt))
        _CAMS[key] = (base, out)
    return _CAMS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [10, 3])
@pytest.mark.parametrize("name", ORIGIN_CASES)
def test_gpu_arbitrary_origins_shade_to_oracle(qr, oracle, rays_mod, name, depth):
    base, cams = _cameras(oracle, rays_mod, name, depth)
    scn = qr.Scene(base, ray_queries=True)
    scn.set_depth(depth)
    rgb, ids = _shade(scn, np.concatenate([c[1] for c in cams]))
    scn.close()
    at = 0
    for j, (cam, rays, ref, ref_ids, _) in enumerate(cams):
        n = len(rays)
        f = rays_mod.pack_colors(rgb[at:at + n], cam)
        assert (f == ref).all(), f"camera {j}: {int((f != ref).sum())} of {ref.size} pixels differ"
        assert (ids[at:at + n] == ref_ids).all(), f"camera {j}: ids differ"
        at += n
    frac = float(np.mean(np.concatenate([c[3] for c in cams]) >= 0))
    assert 0.05 <= frac <= 0.95, f"hit fraction {frac:.3f}: the cameras do not test much"
    assert any(c[4]["reflect"] + c[4]["refract"] > 0 for c in cams), "no camera spawns a reflection or refraction ray"


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [0, 1, 2, 5, 10])
def test_gpu_depth_sweep(qr, oracle, rays_mod, depth):
    blob = load_blob("demo02_160_gf_d5")
    ref, ref_ids, cnt = oracle.render(_rayq.one_tile(blob), depth=depth, threads=16, want_ids=True)
    if depth > 0:
        assert cnt["reflect"] > 0 and cnt["refract"] > 0
    scn = qr.Scene(blob, ray_queries=True)
    scn.set_depth(depth)
    f, ids, _ = _shaded_frame(rays_mod, scn, blob)
    scn.close()
    assert (f == ref).all(), f"depth {depth}: {int((f != ref).sum())} pixels differ"
    assert (ids == ref_ids.reshape(-1)).all()


@pytest.mark.gpu
def test_gpu_order_independence(qr, oracle, rays_mod):
    """a shuffled batch mixing the rays of several cameras (and a count that is no multiple of 64) gives identical rows"""
    rays = []
    for name in ("demo02_160", "synth_small"):
        base, cams = _cameras(oracle, rays_mod, name, 10)
        rays.append((base, np.concatenate([c[1] for c in cams])[:-13]))
    for base, r in rays:
        scn = qr.Scene(base, ray_queries=True)
        rgb, ids = _shade(scn, r)
        perm = np.random.default_rng(11).permutation(len(r))
        rgb2, ids2 = _shade(scn, r[perm])
        scn.close()
        assert (rgb2.view(np.uint32) == rgb[perm].view(np.uint32)).all() and (ids2 == ids[perm]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["demo01_160", "demo02_160_gf_d5", "synth_small"])
def test_gpu_ids_agree_with_trace(qr, oracle, rays_mod, name):
    """shade's ids are trace's on the same rays; rays that miss are exactly 0, 0, 0 (and the only ones that are not
    shaded: a hit always has an id)"""
    import torch
    base, cams = _cameras(oracle, rays_mod, name, 10)
    r = np.concatenate([c[1] for c in cams])
    scn = qr.Scene(base, ray_queries=True)
    rgb, ids = _shade(scn, r)
    _, tids = scn.trace(_cuda(scn, r))
    rgb_only = scn.shade(_cuda(scn, r))
    torch.cuda.synchronize()
    scn.close()
    assert (ids == tids.cpu().numpy()).all()
    assert (rgb_only.cpu().numpy().view(np.uint32) == rgb.view(np.uint32)).all(), "ids=True changed the colours"
    miss = ids == -1
    assert miss.any() and (~miss).any()
    assert (rgb[miss].view(np.uint32) == 0).all()


@pytest.mark.gpu
def test_gpu_refusals(qr):
    import torch
    blob = load_blob("demo01_160")
    L = qr.lib()
    rays = torch.zeros((65, 8), dtype=torch.float32, device="cuda:0")
    rgb = torch.empty((65, 3), dtype=torch.float32, device="cuda:0")
    ids = torch.empty(65, dtype=torch.int32, device="cuda:0")
    vp = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)

    plain = qr.Scene(blob)
    with pytest.raises(qr.QrError, match="QR_UPLOAD_RAY_QUERIES"):
        plain.shade(rays[:64])
    assert L.qr_shade_rays_async(plain._h, vp(rays), 64, vp(rgb), vp(ids), 0, None) == -3
    plain.close()

    scn = qr.Scene(blob, ray_queries=True)
    for bad in (rays.double(), rays[:, :7].contiguous(), rays.cpu(), rays[:, ::2], rays.reshape(-1)):
        with pytest.raises(qr.QrError):
            scn.shade(bad)
    e = scn.shade(rays[:0])
    e2, ei = scn.shade(rays[:0], ids=True)
    assert tuple(e.shape) == (0, 3) and e.dtype == torch.float32 and tuple(e2.shape) == (0, 3) and tuple(ei.shape) == (0,)
    assert L.qr_shade_rays_async(scn._h, vp(rays), 0, vp(rgb), None, 0, None) == 0
    assert L.qr_shade_rays_async(scn._h, vp(rays, 4), 64, vp(rgb), vp(ids), 0, None) == -1          # misaligned
    assert L.qr_shade_rays_async(scn._h, None, 64, vp(rgb), vp(ids), 0, None) == -1
    assert L.qr_shade_rays_async(scn._h, vp(rays), 64, None, vp(ids), 0, None) == -1
    assert L.qr_shade_rays_async(scn._h, vp(rays), 1 << 31, vp(rgb), vp(ids), 0, None) == -1        # n > INT32_MAX
    assert L.qr_shade_rays_async(scn._h, vp(rays), -1, vp(rgb), vp(ids), 0, None) == -1
    assert L.qr_shade_rays_async(scn._h, vp(rays), 64, vp(rgb), vp(ids), 2, None) == -1              # unknown flag
    assert L.qr_shade_rays_async(None, vp(rays), 64, vp(rgb), vp(ids), 0, None) == -1
    # path-tracer mode: caller rays carry no sample seeds
    scn.set_pt(True)
    with pytest.raises(qr.QrError, match="path-tracer"):
        scn.shade(rays[:64])
    scn.set_pt(False)
    # the scene still answers, without ids too (NULL id_out)
    out = scn.shade(rays[:64])
    torch.cuda.synchronize()
    assert tuple(out.shape) == (64, 3)
    scn.close()
