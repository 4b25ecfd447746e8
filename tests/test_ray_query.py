"""Ray queries (include/qrhip.h qr_trace_rays_async / qr_occluded_async, QR_UPLOAD_RAY_QUERIES): closest hit and occlusion of
caller-supplied rays against the snapshot's global list.

The oracle of a query: the snapshot rewritten so that a camera looks along the rays, at depth 0, with ONE tile holding the
global list (tests/_rayq.py with_frame).  Its primary-hit ids are what tracing rays.camera_rays of that snapshot must give.
"""
import ctypes
import os
import zlib

import numpy as np
import pytest

import _rayq
from conftest import MANIFEST, SMALL_CASES, load_blob

REBIN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rebin")
SYNTH_SMALL = dict(n_objects=300, width=320, height=240, depth=4, box=20.0)       # tests/test_synth.py SMALL
NON_PT_SMALL = [n for n in SMALL_CASES if _rayq.frame_words(load_blob(n))[0][41] == 0]
ORIGIN_CASES = ["demo01_160", "test05_160_j14", "test07_160_j3", "swarm_demo01_240", "synth_small"]


@pytest.fixture(scope="module")
def rays_mod():
    import importlib
    from qr_loader import load_package
    load_package()
    return importlib.import_module("quadray_engine_amd.rays")


def _synth(**kw):
    from qr_loader import load_package
    import importlib
    load_package()
    synth = importlib.import_module("quadray_engine_amd.synth")
    return synth.make_scene(**{**SYNTH_SMALL, **kw})


def _blob(name):
    return _synth() if name == "synth_small" else load_blob(name)


def _rebin_blobs():
    import gzip
    import json
    with open(os.path.join(REBIN_DIR, "manifest.json")) as f:
        cases = json.load(f)["cases"]
    for n in sorted(cases):
        with open(os.path.join(REBIN_DIR, cases[n]["snapshot"]), "rb") as f:
            yield n, gzip.decompress(f.read())


# ---------------------------------------------------------------------------------------------------------------- CPU

def _image(qr, monkeypatch, tmp_path, blob, flags):
    p = tmp_path / f"img{flags}.bin"
    monkeypatch.setenv("QR_DUMP_IMAGE", str(p))
    info = qr.program_stats(blob, flags)
    monkeypatch.delenv("QR_DUMP_IMAGE")
    return info, np.frombuffer(p.read_bytes(), dtype=np.uint32)


def test_program_stats_with_ray_queries(qr, monkeypatch, tmp_path):
    """every fixture, the rebin cases and the small synthetic scene compile and verify with the query list; the image without
    the flag is the one the flag extends: same words up to its tail padding but for the header's query-list offset"""
    blobs = [(n, load_blob(n)) for n in sorted(MANIFEST)] + list(_rebin_blobs()) + [("synth_small", _synth())]
    for name, blob in blobs:
        i0, img0 = _image(qr, monkeypatch, tmp_path, blob, 0)
        i1, img1 = _image(qr, monkeypatch, tmp_path, blob, qr.UPLOAD_RAY_QUERIES)
        plain = qr.program_stats(blob)
        assert bytes(plain) == bytes(i0), name
        assert i1.bytes >= i0.bytes and i1.n_lists >= i0.n_lists and i1.n_cells >= i0.n_cells, name
        assert (i1.n_sched, i1.n_clip_cells, i1.n_grids, i1.n_grid_lists) == (i0.n_sched, i0.n_clip_cells, i0.n_grids, i0.n_grid_lists), name
        # DevHeader: qr_frame (49 words), off_shade, off_tiles, off_order, n_blocks, img_flags, img_bytes (54), off_query (55)
        assert img0[55] == 0 and img1[55] != 0, name
        n = len(img0) - 16
        a, b = img0[:n].copy(), img1[:n].copy()
        a[54:56] = 0; b[54:56] = 0
        assert (a == b).all(), f"{name}: the query list changed the render part of the image"
    with pytest.raises(qr.QrError):
        qr.program_stats(blobs[0][1], qr.UPLOAD_REBIN_TILES)          # the binning pass needs the GPU


def test_camera_rays_pinned(rays_mod):
    """a hand-made frame record with integer camera vectors: every ray is exact"""
    fi, ff = _rayq.frame_words(load_blob("demo01_160"))
    blob = _rayq.with_frame(load_blob("demo01_160"), w=5, h=3, org=(1, 2, 3), dir=(-3, -4, 5), hor=(1, 0, 2), ver=(0, 2, -1), t_min=0.25)
    b = bytearray(blob)
    off = _rayq._hdr(b)[10]
    f = np.frombuffer(b, dtype=np.float32, count=49, offset=off).copy()
    f[10], f[14], f[0] = 0.5, 0.25, 1e30
    b[off:off + 196] = f.tobytes()
    r = rays_mod.camera_rays(bytes(b))
    assert r.shape == (15, 8) and r.dtype == np.float32
    for y in range(3):
        for x in range(5):
            hs, vs = x + 0.5, y + 0.25
            want = [1, 2, 3, 0.25, -3 + hs, -4 + 2 * vs, 5 + 2 * hs - vs, 1e30]
            assert r[y * 5 + x].tolist() == np.float32(want).tolist(), (x, y)


@pytest.mark.parametrize("name", NON_PT_SMALL)
def test_oracle_one_tile_clist_equals_tiled_ids(oracle, name):
    """the oracle harness the GPU tests rest on: a walk of the global list in one tile sees what the tiled frame sees"""
    blob = load_blob(name)
    _, ids_t, _ = oracle.render(blob, depth=0, threads=16, want_ids=True)
    _, ids_u, _ = oracle.render(_rayq.one_tile(blob), depth=0, threads=16, want_ids=True)
    assert (ids_t == ids_u).all()


# ---------------------------------------------------------------------------------------------------------------- GPU

def _trace(qr, scn, rays_np, coherent=False):
    import torch
    r = torch.from_numpy(np.ascontiguousarray(rays_np, dtype=np.float32)).to(f"cuda:{scn.device}")
    t, ids = scn.trace(r, coherent=coherent)
    torch.cuda.synchronize()
    return t.cpu().numpy(), ids.cpu().numpy()


def _occluded(qr, scn, rays_np):
    import torch
    r = torch.from_numpy(np.ascontiguousarray(rays_np, dtype=np.float32)).to(f"cuda:{scn.device}")
    o = scn.occluded(r)
    torch.cuda.synchronize()
    return o.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NON_PT_SMALL + ["c2b_demo01_1080p"])
def test_gpu_camera_rays_equal_oracle(qr, oracle, rays_mod, name):
    import torch
    blob = _rayq.with_frame(load_blob(name))
    _, ref, _ = oracle.render(blob, depth=0, threads=16, want_ids=True)
    ref = ref.reshape(-1)
    rays = rays_mod.camera_rays(blob)
    scn = qr.Scene(blob, ray_queries=True)
    for coherent in (False, True):
        _, ids = _trace(qr, scn, rays, coherent)
        assert (ids == ref).all(), f"coherent={coherent}: {int((ids != ref).sum())} rays differ"
    scn.close()
    rb = qr.Scene(blob, rebin_tiles=True)
    f = rb.new_frame(); i = torch.full_like(f, -2)
    rb.render(f, ids=i); torch.cuda.synchronize()
    assert (i.cpu().numpy().reshape(-1) == ref).all()
    rb.close()


_ORIGIN_CACHE = {}


def _origin_case(qr, oracle, rays_mod, name):
    """(scene with ray queries, rays of the 8 cameras concatenated, oracle ids, GPU t, GPU ids) of one fixture"""
    if name in _ORIGIN_CACHE:
        return _ORIGIN_CACHE[name]
    base = _blob(name)
    rays, ref = [], []
    for cam in (_rayq.random_cameras(base, seed=zlib.crc32(name.encode()))):
        _, ids, _ = oracle.render(cam, depth=0, threads=16, want_ids=True)
        rays.append(rays_mod.camera_rays(cam)); ref.append(ids.reshape(-1))
    rays, ref = np.concatenate(rays), np.concatenate(ref)
    scn = qr.Scene(base, ray_queries=True)
    t, ids = _trace(qr, scn, rays)
    _ORIGIN_CACHE[name] = (base, scn, rays, ref, t, ids)
    return _ORIGIN_CACHE[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ORIGIN_CASES)
def test_gpu_arbitrary_origins_equal_oracle(qr, oracle, rays_mod, name):
    base, scn, rays, ref, t, ids = _origin_case(qr, oracle, rays_mod, name)
    assert (ids == ref).all(), f"{int((ids != ref).sum())} of {len(ids)} rays differ"
    frac = float((ref >= 0).mean())
    assert 0.05 <= frac <= 0.95, f"hit fraction {frac:.3f}: the cameras do not test much"
    assert len(np.unique(ref[ref >= 0])) >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("name", ORIGIN_CASES)
def test_gpu_t_is_consistent(qr, oracle, rays_mod, name):
    base, scn, rays, ref, t, ids = _origin_case(qr, oracle, rays_mod, name)
    hit = ids >= 0
    assert hit.any()
    r = rays[hit].copy()
    r[:, 7] = t[hit]                                        # open interval: the hit itself is outside
    _, i2 = _trace(qr, scn, r)
    assert (i2 == -1).all(), f"{int((i2 != -1).sum())} rays still hit with tmax = t"
    r[:, 7] = np.nextafter(t[hit], np.float32(np.inf))
    t3, i3 = _trace(qr, scn, r)
    assert (i3 == ids[hit]).all() and (t3.view(np.uint32) == t[hit].view(np.uint32)).all()
    # +inf is FLT_MAX
    r = rays.copy(); r[:, 7] = np.float32(np.inf)
    t4, i4 = _trace(qr, scn, r)
    r[:, 7] = np.finfo(np.float32).max
    t5, i5 = _trace(qr, scn, r)
    assert (i4 == i5).all() and (t4.view(np.uint32) == t5.view(np.uint32)).all()
    assert not np.isnan(t4).any()


@pytest.mark.gpu
def test_gpu_t_matches_float64_intersection(qr, rays_mod):
    """untransformed surfaces without clippers in the flat synthetic scene: t agrees with a float64 intersection"""
    blob = _synth(hierarchy=False)
    s, f = _rayq.surfaces(blob)
    cams = _rayq.random_cameras(blob, seed=7)
    rays = np.concatenate([rays_mod.camera_rays(c) for c in cams])
    scn = qr.Scene(blob, ray_queries=True)
    t, ids = _trace(qr, scn, rays)
    scn.close()
    si = ids >> 1
    ok = (ids >= 0)
    ok[ok] &= (s[si[ok], 15] == 0) & (s[si[ok], 38] == -1) & np.isin(s[si[ok], 34], (1, 2))
    idx = np.nonzero(ok)[0]
    assert len(idx) > 100
    o = rays[idx, 0:3].astype(np.float64); d = rays[idx, 4:7].astype(np.float64)
    srf = si[idx]
    pos = f[srf, 0:3].astype(np.float64)
    df = o - pos
    n_checked = 0
    for j in range(len(idx)):
        q = srf[j]
        if s[q, 34] == 1:                                   # plane along axis k (axes bits 4-5)
            k = (s[q, 23] >> 4) & 3
            roots = [-df[j, k] / d[j, k]]
        else:                                               # quadric: sci . p^2 - 2 scj . p - sci3 = 0, p = df + t d
            sci = f[q, 24:28].astype(np.float64); scj = f[q, 28:31].astype(np.float64)
            a = np.sum(sci[:3] * d[j] * d[j])
            b = np.sum(d[j] * (sci[:3] * df[j] - scj))
            c = np.sum(df[j] * (sci[:3] * df[j] - 2 * scj)) - sci[3]
            disc = max(b * b - a * c, 0.0)
            roots = [(-b - np.sqrt(disc)) / a, (-b + np.sqrt(disc)) / a] if a != 0 else [-c / (2 * b)]
        err = min(abs(r - float(t[idx[j]])) / max(abs(r), 1e-30) for r in roots)
        # a grazing hit (the two roots close together) is ill-conditioned in any fp32 solver: the rounding of b^2 - ac is
        # magnified by 1 / sqrt(b^2 - ac) ~ t / (distance of the roots); 1e-5 where the roots lie at least a quarter of t apart,
        # 1e-3 on the others
        grazing = len(roots) == 2 and abs(roots[1] - roots[0]) < 0.25 * abs(float(t[idx[j]]))
        assert err <= (1e-3 if grazing else 1e-5), (j, int(q), float(t[idx[j]]), roots)
        n_checked += 0 if grazing else 1
    assert n_checked > 100


@pytest.mark.gpu
@pytest.mark.parametrize("name", ORIGIN_CASES)
def test_gpu_occlusion(qr, oracle, rays_mod, name):
    base, scn, rays, ref, t, ids = _origin_case(qr, oracle, rays_mod, name)
    cast = _rayq.casts(base)
    hit = ids >= 0
    r = rays[hit].copy()
    r[:, 7] = t[hit] * np.float32(0.5)
    assert not _occluded(qr, scn, r).any(), "nothing lies in front of the closest hit"
    r[:, 7] = t[hit] * np.float32(2.0)
    occ = _occluded(qr, scn, r)
    c = cast[ids[hit] >> 1, ids[hit] & 1]
    assert occ[c].all(), "a shadow-casting closest hit inside the interval occludes"
    miss = rays[~hit]
    assert not _occluded(qr, scn, miss).any(), "a ray that hits nothing is not occluded"
    if cast[_rayq.real_surfaces(base)].all():
        assert (_occluded(qr, scn, rays) == hit).all(), "all surfaces cast: occlusion is 'hits something'"


@pytest.mark.gpu
def test_gpu_occlusion_equals_hit_on_opaque_scene(qr, oracle, rays_mod):
    """every surface made to cast (props without light / transparency bits): the two queries are equivalent"""
    base, _, rays, _, _, _ = _origin_case(qr, oracle, rays_mod, "demo02_160")
    b = bytearray(base)
    h = _rayq._hdr(b)
    s = np.frombuffer(b, dtype=np.int32, count=h[4] * 64, offset=h[11]).reshape(h[4], 64).copy()
    s[:, 42:44] &= ~(_rayq.PROP_LIGHT | _rayq.PROP_TRANSP)
    b[h[11]:h[11] + s.nbytes] = s.tobytes()
    scn = qr.Scene(bytes(b), ray_queries=True)
    _, ids = _trace(qr, scn, rays)
    assert (_occluded(qr, scn, rays) == (ids >= 0)).all()
    scn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ORIGIN_CASES)
def test_gpu_order_invariance(qr, oracle, rays_mod, name):
    base, scn, rays, ref, t, ids = _origin_case(qr, oracle, rays_mod, name)
    perm = np.random.default_rng(5).permutation(len(rays))
    t2, i2 = _trace(qr, scn, rays[perm])
    assert (i2 == ids[perm]).all() and (t2.view(np.uint32) == t[perm].view(np.uint32)).all()
    o1 = _occluded(qr, scn, rays)
    assert (_occluded(qr, scn, rays[perm]) == o1[perm]).all()


@pytest.mark.gpu
def test_gpu_refusals(qr):
    import torch
    blob = load_blob("demo01_160")
    L = qr.lib()
    rays = torch.zeros((65, 8), dtype=torch.float32, device="cuda:0")
    t = torch.empty(65, dtype=torch.float32, device="cuda:0")
    ids = torch.empty(65, dtype=torch.int32, device="cuda:0")
    occ = torch.empty(65, dtype=torch.uint8, device="cuda:0")
    plain = qr.Scene(blob)
    with pytest.raises(qr.QrError, match="QR_UPLOAD_RAY_QUERIES"):
        plain.trace(rays[:64])
    assert L.qr_occluded_async(plain._h, ctypes.c_void_p(rays.data_ptr()), 64, ctypes.c_void_p(occ.data_ptr()), 0, None) == -3
    plain.close()
    scn = qr.Scene(blob, ray_queries=True)
    vp = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)
    assert L.qr_trace_rays_async(scn._h, vp(rays), 0, vp(t), vp(ids), 0, None) == 0
    assert L.qr_occluded_async(scn._h, vp(rays), 0, vp(occ), 0, None) == 0
    assert L.qr_trace_rays_async(scn._h, vp(rays, 4), 64, vp(t), vp(ids), 0, None) == -1         # misaligned
    assert L.qr_occluded_async(scn._h, vp(rays, 8), 64, vp(occ), 0, None) == -1
    assert L.qr_trace_rays_async(scn._h, vp(rays), 1 << 31, vp(t), vp(ids), 0, None) == -1       # n > INT32_MAX
    assert L.qr_trace_rays_async(scn._h, None, 64, vp(t), vp(ids), 0, None) == -1
    assert L.qr_trace_rays_async(None, vp(rays), 64, vp(t), vp(ids), 0, None) == -1
    torch.cuda.synchronize()
    # the scene still answers after the refusals
    tt, ii = scn.trace(rays[:64])
    torch.cuda.synchronize()
    assert ii.shape == (64,)
    scn.close()
