"""Hit records (include/qrhip.h qr_hit, qr_hit_rays_async / qr_hit_views_async; Scene.hits, Scene.view_hits): the closest hit of
a ray and the surface point the renderer would shade there -- position, normal, texture colour, material.

The truth is the oracle's own arithmetic, read out: tests/hitrec_oracle.c includes oracle/qr_oracle.c, runs the loop of
qro_trace_rays mode 0 (deferred: shade() is called once, for the closest hit) and writes the context's hit, nrm and tex fields
as qr_hit rows.  The oracle computes a normal only under QR_PROP_NORMAL, the kernel for every hit, so the helper sets the prop on
every side of a COPY of the snapshot.  The CPU tests pin that helper (its walk is qro_trace_rays' on the untouched snapshot, its
fields obey the rules the header states); the GPU tests then ask for all 48 bytes of every record.

The bounds and where they come from:
  | |nrm| - 1 | <= 1e-6   a normalised fp32 vector from one rsq and three products carries a few ulp (2^-23 = 1.2e-7 each).
                          Where the hit point rounds onto a quadric's centre or axis the gradient is zero and the normal NaN
                          (0 * inf), in the renderer too: only rays whose hit point fp32 cannot resolve get there (the `far`
                          family's origins, the `scale` family's directions of length 2^40), so every other family must give
                          finite normals; how many those two meet is printed.
  nrm . dir <= 0          nrm is the normal of the side the walk names (id & 1).  For planes and for quadrics without a conic
                          term -- spheres, ellipsoids, cylinders, paraboloids -- that is the side the ray arrives on, in front of
                          the origin and behind it (tmin < 0).  At grazing incidence the fp32 normal and the side come from
                          different roundings, so the dot product is allowed the error of its own inputs: 1e-5 * |dir| (|nrm| = 1;
                          hit point and normal carry a few ulp of a value of the scene's size, amplified by the surface's
                          curvature; the test prints the worst it meets).  Two families of tests/_rayset.py leave the rule's
                          domain by construction, and the header says so: on cones, hyperboloids and hyperbolic cylinders
                          (qr_surface.conic != 0) the solver names the side by the order of the roots, which on the second
                          sheet is the far side (`probe`, `interval`, `scale` meet such hits); and from origins hundreds of scene
                          sizes away (`far`) fp32 no longer resolves the point the normal is taken at.  So the rule is tested
                          on every hit of a surface with conic == 0 from an origin within two scene sizes of the scene's
                          middle -- camera rays and all families, 1.3 M hits, 40 000 of them behind the origin.
"""
import ctypes
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import _rayq
import _rayset as RS
from conftest import ROOT, load_blob
from test_ray_query import NON_PT_SMALL, ORIGIN_CASES, _blob

FLT_MAX = np.finfo(np.float32).max
CAMERA_CASES = NON_PT_SMALL + ["synth_small"]
VIEW_SIZES = [(64, 64), (67, 45), (9, 130)]
SEEDED = ORIGIN_CASES + ["demo01_160_gf_aa4", "demo02_160_cam2_gf_aa2"]
FAMILIES = [f for f in RS.FAMILIES if f != "grid"]          # the grid family needs a list that carries a uniform grid: test_gpu_hits_edge_families
ASM = os.path.join(ROOT, "quadray-engine_amd", "csrc", "qr_device-hip-amdgcn-amd-amdhsa-gfx950.s")
GUARD_LIB = os.path.join(ROOT, "quadray-engine_amd", "libqrhip_guard.so")


def _rays_mod():
    import importlib
    from qr_loader import load_package
    load_package()
    return importlib.import_module("quadray_engine_amd.rays")


@pytest.fixture(scope="module")
def rays_mod():
    return _rays_mod()


# ------------------------------------------------------------------------------------------------------------ the helper

_HELPER = None


def _helper():
    """hit_rays(blob, rays float32 [N, 8]) -> float32 [N, 12] from tests/_build/libqr_hitrec.so, compiled here when it is missing
    or older than its sources (the builder is build()'s own step: __graft_entry__.build_hitrec_oracle).  A compiler failure
    raises: the tests that need the helper fail, they do not skip."""
    global _HELPER
    if _HELPER is None:
        import __graft_entry__ as g
        L = ctypes.CDLL(g.build_hitrec_oracle())
        L.qrh_hit_rays.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
        L.qrh_hit_rays.restype = ctypes.c_int

        def hit_rays(blob, rays, threads=16):
            r = np.ascontiguousarray(rays, dtype=np.float32)
            assert r.ndim == 2 and r.shape[1] == 8
            out = np.full((len(r), 12), np.nan, dtype=np.float32)
            buf = ctypes.create_string_buffer(blob, len(blob))
            rc = L.qrh_hit_rays(buf, len(blob), r.ctypes.data, len(r), threads, out.ctypes.data)
            if rc != 0:
                raise RuntimeError(f"qrh_hit_rays rc={rc}")
            return out
        _HELPER = hit_rays
    return _HELPER


@pytest.fixture(scope="module")
def helper():
    return _helper()


def _fields(h):
    """(pos, t, nrm, id, alb, mat) of numpy records, the integer fields as int32"""
    i = h.view(np.int32)
    return h[..., 0:3], h[..., 3], h[..., 4:7], i[..., 7], h[..., 8:11], i[..., 11]


def _ray_sets(blob, name, oracle, rays_mod, g=None, reach=None):
    """[(label, rays)]: the camera's rays and the adversarial families of tests/_rayset.py"""
    out = [("camera", rays_mod.camera_rays(blob))]
    for fam in FAMILIES + (["grid"] if g is not None else []):
        r = RS.family(blob, name, fam, oracle, g, reach)
        if len(r):
            out.append((fam, r))
    return out


# ------------------------------------------------------------------------------------------------------------------- CPU

def test_helper_is_built_by_build():
    """build() compiles the helper (a tree built before it travels has the library) through the function the fixture uses"""
    import __graft_entry__ as g
    import inspect
    assert "build_hitrec_oracle()" in inspect.getsource(g.build)
    assert g.HITREC_LIB == os.path.join(ROOT, "tests", "_build", "libqr_hitrec.so")
    p = g.build_hitrec_oracle()
    assert os.path.exists(p) and os.path.getmtime(p) >= os.path.getmtime(g.HITREC_SRC)


@pytest.mark.parametrize("name", CAMERA_CASES)
def test_helper_pinned(oracle, rays_mod, helper, name):
    """the helper on camera rays and every family: its walk is qro_trace_rays' on the untouched snapshot, pos is fp32
    dir * t + org, mat the snapshot's, misses the stated defaults, normals unit length and on the ray's side"""
    blob = _blob(name)
    srf, _ = _rayq.surfaces(blob)
    lo, hi, ext = RS._box(blob)
    mid = (lo + hi) / 2
    worst_len, worst_face = 0.0, -1.0
    n_hits = n_faced = n_nan = 0
    mats = set()
    for label, rays in _ray_sets(blob, name, oracle, rays_mod):
        h = helper(blob, rays)
        pos, t, nrm, hid, alb, mat = _fields(h)
        t_w, id_w = oracle.trace_rays(blob, rays, "trace", threads=16)
        where = f"{name} {label}"
        assert (hid == id_w).all(), f"{where}: {int((hid != id_w).sum())} ids differ from qro_trace_rays"
        assert (t.view(np.uint32) == t_w.view(np.uint32)).all(), f"{where}: t differs from qro_trace_rays"
        hit = hid >= 0
        # misses, bit for bit
        tmax = np.where(rays[:, 7] > FLT_MAX, FLT_MAX, rays[:, 7]).astype(np.float32)
        miss = h[~hit].view(np.uint32)
        assert (miss[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]] == 0).all(), f"{where}: a miss holds something but +0.0"
        assert (miss[:, 3] == tmax[~hit].view(np.uint32)).all() and (mat[~hit] == -1).all(), where
        if not hit.any():
            continue
        r, t_h = rays[hit], t[hit]
        with np.errstate(over="ignore", invalid="ignore"):
            want = (r[:, 4:7] * t_h[:, None]).astype(np.float32) + r[:, 0:3]
        assert (pos[hit].view(np.uint32) == want.view(np.uint32)).all(), f"{where}: pos is not fp32 dir * t + org"
        assert (mat[hit] == srf[hid[hit] >> 1, 40 + (hid[hit] & 1)]).all(), f"{where}: mat is not qr_surface.mat[side]"
        mats.update(mat[hit].tolist())
        n64 = nrm[hit].astype(np.float64)
        fin = np.isfinite(n64).all(axis=1)
        # a hit point that fp32 rounds onto the surface's centre or axis has a zero gradient there: 0 * inf, NaN -- the far
        # family's origins and the scale family's directions of 2^40 make such points, no other family may
        assert fin.all() or label in ("far", "scale", "mixed"), f"{where}: {int((~fin).sum())} normals are not finite"
        n_nan += int((~fin).sum())
        ln = np.abs(np.linalg.norm(n64[fin], axis=1) - 1.0)
        worst_len = max(worst_len, float(ln.max()))
        assert (ln <= 1e-6).all(), f"{where}: |nrm| off by {ln.max():.3g}"
        d64 = r[:, 4:7].astype(np.float64)
        dl = np.linalg.norm(d64, axis=1)
        face = np.sum(n64 * d64, axis=1) / dl
        dom = (srf[hid[hit] >> 1, 11] == 0) & (np.abs(r[:, 0:3] - mid).max(axis=1) <= 2 * ext)     # the facing rule's domain
        n_faced += int(dom.sum())
        face = np.where(dom & fin, face, -1.0)
        worst_face = max(worst_face, float(face.max()))
        bad = face > 1e-5
        assert not bad.any(), (f"{where}: {int(bad.sum())} normals face away from the ray, worst {face.max():.3g}: "
                               f"ray {r[bad][0].tolist()} record {h[hit][bad][0].tolist()}")
        a = alb[hit]
        assert ((a >= 0) & (a <= 1)).all(), f"{where}: albedo outside [0, 1]"
        n_hits += int(hit.sum())
    print(f"{name}: {n_hits} hits, {len(mats)} materials, worst | |nrm| - 1 | {worst_len:.3g}, "
          f"worst nrm . dir / |dir| {worst_face:.3g} over {n_faced} hits, {n_nan} normals at a zero gradient")
    assert n_hits > 1000 and n_faced > 1000 and len(mats) >= 2


def test_helper_plane_without_transform_has_axis_normal(oracle, rays_mod, helper):
    """a plane whose surface has no transform: one component +-1, two +0.0, exactly"""
    seen = 0
    for name in ("demo01_160", "demo02_160_gf_d5", "test05_160_j14"):
        blob = load_blob(name)
        srf, _ = _rayq.surfaces(blob)
        h = helper(blob, rays_mod.camera_rays(blob))
        _, _, nrm, hid, _, _ = _fields(h)
        hit = hid >= 0
        si = hid[hit] >> 1
        plain = (srf[si, 35] == 1) & (srf[si, 15] == 0)            # srf_t[1]: plane normal; has_trm 0
        bits = np.sort(nrm[hit][plain].view(np.uint32) & 0x7FFFFFFF, axis=1)
        one = int(np.float32(1.0).view(np.uint32))
        assert (nrm[hit][plain].view(np.uint32)[np.abs(nrm[hit][plain]) == 0] == 0).all(), f"{name}: a zero component is -0.0"
        assert (bits == np.array([0, 0, one], dtype=np.uint32)).all(), name
        seen += int(plain.sum())
    assert seen > 1000


def test_hit_kernels_in_resource_check():
    """the build's register check knows the four hit-record instances, allows them no spill and no private segment, and the
    build's assembly passes it"""
    import importlib.util
    path = os.path.join(ROOT, "tools", "check_kernel_resources.py")
    spec = importlib.util.spec_from_file_location("check_kernel_resources", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    frags = sorted(f for f in m.LIMITS if "qr_hit_kernel" in f)
    assert len(frags) == 4
    for f in frags:
        assert m.LIMITS[f][1] == 0 and m.LIMITS[f][2] == 0 and m.LIMITS[f][0] <= 168, f
    r = subprocess.run([sys.executable, path, ASM, "--print"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("qr_hit_kernel") == 4


def _records():
    """four hand-made records: a hit with an axis normal, a hit with a tilted one, a miss, a hit"""
    h = np.zeros((4, 12), dtype=np.float32)
    i = h.view(np.int32)
    h[0, 0:3], h[0, 3], h[0, 4:7], h[0, 8:11] = (1, 2, 3), 5.0, (0, 0, 1), (0.5, 0.25, 1.0)
    i[0, 7], i[0, 11] = 7, 3
    s = np.float32(np.sqrt(0.5))
    h[1, 0:3], h[1, 3], h[1, 4:7], h[1, 8:11] = (-1, 0, 4), 2.5, (s, 0, s), (1, 1, 1)
    i[1, 7], i[1, 11] = (12 << 1) | 1, 0
    h[2, 3] = FLT_MAX
    i[2, 7], i[2, 11] = -1, -1
    h[3, 0:3], h[3, 3], h[3, 4:7] = (9, 9, 9), 1.0, (0, -1, 0)
    i[3, 7], i[3, 11] = 2, 1
    return h


def test_hit_fields_are_views(rays_mod):
    import torch
    for h in (_records(), torch.from_numpy(_records()), _records().reshape(2, 2, 12), torch.from_numpy(_records()).reshape(2, 2, 12)):
        pos, t, nrm, hid, alb, mat = rays_mod.hit_fields(h)
        flat = (lambda a: a.reshape(-1, a.shape[-1]) if a.ndim == h.ndim else a.reshape(-1))
        assert tuple(pos.shape) == tuple(h.shape[:-1]) + (3,) and tuple(t.shape) == tuple(h.shape[:-1])
        assert "int32" in str(hid.dtype) and "int32" in str(mat.dtype) and "float32" in str(t.dtype)
        assert [int(x) for x in flat(hid)] == [7, 25, -1, 2] and [int(x) for x in flat(mat)] == [3, 0, -1, 1]
        assert [float(x) for x in flat(t)][:2] == [5.0, 2.5] and [float(x) for x in flat(alb)[0]] == [0.5, 0.25, 1.0]
        assert [float(x) for x in flat(nrm)[3]] == [0.0, -1.0, 0.0]
        # views, not copies: writes through them land in the record
        flat(hid)[0] = 99
        flat(pos)[1, 2] = -8.0
        hh = h.reshape(-1, 12)
        assert int(hh.view(np.int32)[0, 7] if isinstance(hh, np.ndarray) else hh.view(torch.int32)[0, 7]) == 99
        assert float(hh[1, 2]) == -8.0
    for bad in (np.zeros((3, 11), dtype=np.float32), np.zeros((3, 12), dtype=np.float64), torch.zeros((3, 12), dtype=torch.int32)):
        with pytest.raises(ValueError):
            rays_mod.hit_fields(bad)


def test_offset_and_reflect_rays(rays_mod):
    import torch
    h = torch.from_numpy(_records())
    inc = torch.tensor([[0, 0, 10, 0, 0, 0, -2, np.inf], [0, 0, 0, 0, 1, 0, 0, np.inf],
                        [0, 0, 0, 0, 1, 1, 1, np.inf], [9, 10, 9, 0, 0, 1, 0, 5]], dtype=torch.float32)
    dirs = torch.tensor([[0, 0, 1], [1, 0, 0], [0, 1, 0], [0, -1, 0]], dtype=torch.float32)
    o = rays_mod.offset_rays(h, dirs, 1e-3)
    assert o.dtype == torch.float32 and tuple(o.shape) == (4, 8)
    assert torch.equal(o[:, 0:3], h[:, 0:3]) and torch.equal(o[:, 4:7], dirs)
    assert (o[:, 3] == float(np.float32(1e-3))).all()
    assert torch.isinf(o[[0, 1, 3], 7]).all() and o[2, 7] == o[2, 3], "a miss gets tmax = tmin: an empty interval"
    r = rays_mod.reflect_rays(inc, h, 1e-3)
    assert torch.equal(r[:, 0:3], h[:, 0:3]) and (r[:, 3] == float(np.float32(1e-3))).all()
    assert r[0, 4:7].tolist() == [0.0, 0.0, 2.0]                    # (0, 0, -2) mirrored at z
    assert np.allclose(r[1, 4:7].numpy(), [0.0, 0.0, -1.0], atol=1e-6)     # (1, 0, 0) at the 45 degree normal
    assert r[3, 4:7].tolist() == [0.0, -1.0, 0.0]
    assert r[2, 7] == r[2, 3] and torch.isinf(r[[0, 1, 3], 7]).all()
    for f in (rays_mod.offset_rays, rays_mod.reflect_rays):
        assert "bit-exact" in f.__doc__


# ------------------------------------------------------------------------------------------------------------------- GPU

NAMES = ("pos.x", "pos.y", "pos.z", "t", "nrm.x", "nrm.y", "nrm.z", "id", "alb.x", "alb.y", "alb.z", "mat")


def _nan_bits(h):
    """records as uint32 [N, 12]; a NaN in a float field becomes 0x7FC00000: which NaN an invalid operation (the 0 * inf of a
    normal at a zero gradient) delivers is the processor's choice -- x86 sets the sign bit, the GPU does not -- and no
    arithmetic of the record's"""
    f = np.ascontiguousarray(h, dtype=np.float32).reshape(-1, 12).copy()
    u = f.view(np.uint32)
    cols = [0, 1, 2, 3, 4, 5, 6, 8, 9, 10]
    nan = np.isnan(f[:, cols])
    sub = u[:, cols]
    sub[nan] = 0x7FC00000
    u[:, cols] = sub
    return u


def _same_records(where, rays, got, want):
    """all 48 bytes of every record"""
    g = _nan_bits(got)
    w = _nan_bits(want)
    assert g.shape == w.shape, f"{where}: {g.shape} records for {w.shape}"
    bad = (g != w).any(axis=1)
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        cols = [NAMES[c] for c in np.nonzero(g[i] != w[i])[0]]
        ray = rays[i].tolist() if rays is not None else None
        raise AssertionError(f"{where}: {int(bad.sum())} of {len(g)} records differ; first {i} in {cols}: ray {ray} "
                             f"got {g[i].view(np.float32).tolist()} ids {g[i].view(np.int32)[[7, 11]].tolist()} "
                             f"want {w[i].view(np.float32).tolist()} ids {w[i].view(np.int32)[[7, 11]].tolist()}")


def _cuda(scn, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(f"cuda:{scn.device}")


def _hits(scn, rays_np, **kw):
    import torch
    out = scn.hits(_cuda(scn, rays_np), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _view_hits(scn, views, w=None, h=None):
    import torch
    out = scn.view_hits(_cuda(scn, np.stack(views)), w, h)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_hits(scn, where, rays, want):
    """Scene.hits with and without `coherent` against the helper, and against Scene.trace"""
    import torch
    for coherent in (False, True):
        got = _hits(scn, rays, coherent=coherent)
        assert got.shape == (len(rays), 12) and got.dtype == np.float32
        _same_records(f"{where} coherent={coherent}", rays, got, want)
    t, ids = scn.trace(_cuda(scn, rays))
    torch.cuda.synchronize()
    _, t_h, _, id_h, _, _ = _fields(got)
    assert (ids.cpu().numpy() == id_h).all() and (t.cpu().numpy().view(np.uint32) == t_h.view(np.uint32)).all(), f"{where}: trace() disagrees"


@pytest.mark.gpu
@pytest.mark.parametrize("name", CAMERA_CASES)
def test_gpu_hits_camera_rays(qr, rays_mod, helper, name):
    blob = _blob(name)
    rays = rays_mod.camera_rays(blob)
    scn = qr.Scene(blob, ray_queries=True)
    try:
        _check_hits(scn, f"{name} camera", rays, helper(blob, rays))
    finally:
        scn.close()


def _rs_scene(qr, name):
    with RS.upload_env(name):
        return qr.Scene(RS.scene_blob(name), ray_queries=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ORIGIN_CASES + ["synth_small_dda", "crowd_flat_dda"])
def test_gpu_hits_edge_families(qr, oracle, rays_mod, helper, name, tmp_path):
    """the adversarial families of tests/_rayset.py (the grid family on the scenes whose query list carries a uniform grid;
    crowd_flat_dda: records on every surface kind, axis map and a textured plane of tests/_crowd.py)"""
    blob = RS.scene_blob(name)
    off, img = RS.query_image(qr, name, tmp_path)
    scn = _rs_scene(qr, name)
    try:
        for label, rays in _ray_sets(blob, name, oracle, rays_mod, RS.dda_grid(off, img), RS.reach_of(img))[1:]:
            _check_hits(scn, f"{name} {label}", rays, helper(blob, rays))
    finally:
        scn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_gpu_hits_batch_sizes(qr, oracle, rays_mod, helper, n):
    """partial waves: nothing is written past the batch's end"""
    import torch
    name = "synth_small"
    blob = RS.scene_blob(name)
    r = RS.mixed(blob, name, oracle)
    rays = np.concatenate([r] * (n // len(r) + 1))[:n]
    scn = _rs_scene(qr, name)
    try:
        _check_hits(scn, f"{name} n={n}", rays, helper(blob, rays))
        out = torch.full((n + 64, 12), 7.0, dtype=torch.float32, device="cuda:0")
        r_dev = _cuda(scn, rays)
        rc = qr.lib().qr_hit_rays_async(scn._h, ctypes.c_void_p(r_dev.data_ptr()), n, ctypes.c_void_p(out.data_ptr()), 0, None)
        torch.cuda.synchronize()
        assert rc == 0 and (out[n:] == 7.0).all().item(), "records written past the end of the batch"
    finally:
        scn.close()


def _check_views(scn, blob, rays_mod, helper, where, views, w, h):
    """view_hits of several views in one launch against the helper on view_rays(sample 0), and against render_views' ids / depth"""
    import torch
    got = _view_hits(scn, views, w, h)
    assert got.shape == (len(views), h, w, 12)
    for j, v in enumerate(views):
        rays = rays_mod.view_rays(v, w, h, blob, sample=0)
        _same_records(f"{where} view {j} at {w}x{h}", rays, got[j], helper(blob, rays))
    _, ids, dep = scn.render_views(_cuda(scn, np.stack(views)), w, h, ids=True, depth=True)
    torch.cuda.synchronize()
    _, t_h, _, id_h, _, _ = _fields(got)
    assert (ids.cpu().numpy() == id_h).all(), f"{where}: render_views ids disagree"
    assert (dep.cpu().numpy().view(np.uint32) == t_h.view(np.uint32)).all(), f"{where}: render_views depth disagrees"
    return int((id_h >= 0).sum()), id_h.size


@pytest.mark.gpu
@pytest.mark.parametrize("name", NON_PT_SMALL)
def test_gpu_view_hits_own_camera(qr, rays_mod, helper, name):
    blob = load_blob(name)
    fi, _ = _rayq.frame_words(blob)
    scn = qr.Scene(blob, ray_queries=True)
    try:
        _check_views(scn, blob, rays_mod, helper, name, [rays_mod.view_of(blob)], int(fi[31]), int(fi[32]))
    finally:
        scn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SEEDED)
def test_gpu_view_hits_seeded_cameras(qr, rays_mod, helper, name):
    """eight seeded cameras among the objects (half of them with t_min 0) in ONE launch per size, sizes that are no multiple
    of a footprint, FSAA fixtures included (sample 0's ray)"""
    blob = _blob(name)
    views = [rays_mod.view_of(c) for c in _rayq.random_cameras(blob, seed=zlib.crc32(name.encode()), n=8)]
    scn = qr.Scene(blob, ray_queries=True)
    hits = total = 0
    try:
        for (w, h) in VIEW_SIZES:
            a, b = _check_views(scn, blob, rays_mod, helper, name, views, w, h)
            hits += a; total += b
    finally:
        scn.close()
    assert 0.05 <= hits / total <= 0.95, f"hit fraction {hits / total:.3f}: the views do not test much"


@pytest.mark.gpu
def test_gpu_hits_ignore_path_tracer_mode_and_depth(qr, rays_mod, helper):
    """nothing is shaded: the records do not depend on the recursion depth or on path-tracer mode"""
    blob = load_blob("demo02_160_gf_d5")
    rays = rays_mod.camera_rays(blob)
    want = helper(blob, rays)
    scn = qr.Scene(blob, ray_queries=True)
    try:
        scn.set_depth(0)
        _same_records("depth 0", rays, _hits(scn, rays), want)
        scn.set_pt(True)
        _same_records("path-tracer mode", rays, _hits(scn, rays), want)
        fi, _ = _rayq.frame_words(blob)
        _same_records("path-tracer mode, view", rays, _view_hits(scn, [rays_mod.view_of(blob)])[0], want)
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_refusals(qr, rays_mod):
    import torch
    blob = load_blob("demo01_160")
    L = qr.lib()
    dev = "cuda:0"
    ARG, UNSUP = -1, -3
    rays = torch.from_numpy(rays_mod.camera_rays(blob)[:128]).to(dev)
    out = torch.zeros((128, 12), dtype=torch.float32, device=dev)
    w, h = 67, 45
    vt = torch.from_numpy(np.stack([rays_mod.view_of(blob)] * 2)).to(dev)
    vo = torch.zeros((2, h, w, 12), dtype=torch.float32, device=dev)
    vp = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)

    def views(s, views=vp(vt), n=2, w=w, h=h, hits=vp(vo), flags=0):
        return L.qr_hit_views_async(s, views, n, w, h, hits, flags, None)

    plain = qr.Scene(blob)
    with pytest.raises(qr.QrError, match="QR_UPLOAD_RAY_QUERIES"):
        plain.hits(rays)
    with pytest.raises(qr.QrError, match="QR_UPLOAD_RAY_QUERIES"):
        plain.view_hits(vt, w, h)
    assert L.qr_hit_rays_async(plain._h, vp(rays), 64, vp(out), 0, None) == UNSUP
    assert views(plain._h) == UNSUP
    plain.close()

    scn = qr.Scene(blob, ray_queries=True)
    # caller rays: as qr_trace_rays_async
    assert L.qr_hit_rays_async(scn._h, vp(rays), 0, vp(out), 0, None) == 0
    assert L.qr_hit_rays_async(scn._h, None, 0, None, 0, None) == 0
    assert L.qr_hit_rays_async(scn._h, vp(rays, 4), 64, vp(out), 0, None) == ARG            # misaligned
    assert L.qr_hit_rays_async(scn._h, vp(rays), 64, vp(out, 8), 0, None) == ARG
    assert L.qr_hit_rays_async(scn._h, None, 64, vp(out), 0, None) == ARG
    assert L.qr_hit_rays_async(scn._h, vp(rays), 64, None, 0, None) == ARG
    assert L.qr_hit_rays_async(scn._h, vp(rays), 1 << 31, vp(out), 0, None) == ARG          # n > INT32_MAX
    assert L.qr_hit_rays_async(scn._h, vp(rays), -1, vp(out), 0, None) == ARG
    assert L.qr_hit_rays_async(scn._h, vp(rays), 64, vp(out), 2, None) == ARG               # unknown flag
    assert L.qr_hit_rays_async(None, vp(rays), 64, vp(out), 0, None) == ARG
    assert L.qr_hit_rays_async(scn._h, vp(rays), 64, vp(out), 1, None) == 0                 # QR_TRACE_COHERENT
    for bad in (rays.double(), rays[:, :7].contiguous(), rays.cpu(), rays[:, ::2], rays.reshape(-1), rays.cpu().numpy()):
        with pytest.raises(qr.QrError, match="rays must be"):
            scn.hits(bad)
    e = scn.hits(rays[:0])
    assert tuple(e.shape) == (0, 12) and e.dtype == torch.float32
    # views: as qr_render_views_async
    assert views(None) == ARG
    assert views(scn._h, views=None) == ARG and views(scn._h, hits=None) == ARG
    assert views(scn._h, views=vp(vt, 4)) == ARG and views(scn._h, views=vp(vt, 8)) == ARG
    assert views(scn._h, hits=vp(vo, 4)) == ARG and views(scn._h, hits=vp(vo, 8)) == ARG
    assert views(scn._h, n=-1) == ARG
    assert views(scn._h, w=0) == ARG and views(scn._h, h=0) == ARG and views(scn._h, w=-5) == ARG
    assert views(scn._h, w=16385) == ARG and views(scn._h, h=1 << 20) == ARG                # QR_VIEW_MAX_DIM
    assert views(scn._h, n=65536) == ARG                                                    # QR_VIEW_MAX_VIEWS
    assert views(scn._h, n=65535, w=16384, h=16384) == ARG                                  # beyond one grid
    assert views(scn._h, flags=1) == ARG and views(scn._h, flags=0x80000000) == ARG
    assert views(scn._h, n=0) == 0 and views(scn._h, n=0, views=None, hits=None) == 0
    assert views(scn._h) == 0
    torch.cuda.synchronize()
    for bad in (vt.double(), vt[:, :15].contiguous(), vt.cpu(), vt[:, ::2], vt.reshape(-1), vt.cpu().numpy()):
        with pytest.raises(qr.QrError, match="views must be"):
            scn.view_hits(bad, w, h)
    for bw, bh in ((0, h), (w, -1), (w, 2.5), (16385, h)):
        with pytest.raises(qr.QrError):
            scn.view_hits(vt, bw, bh)
    e = scn.view_hits(vt[:0], w, h)
    assert tuple(e.shape) == (0, h, w, 12) and e.dtype == torch.float32
    assert tuple(scn.view_hits(vt).shape) == (2, scn.height, scn.width, 12)                 # the snapshot's size by default
    torch.cuda.synchronize()
    scn.close()


# the same comparisons once through the guarded diagnostic build (make guard: QR_STATS + QR_GUARD, every cell offset of the
# per-lane walks checked before it is loaded; it compiles every kernel of the device translation unit, these included).  A guarded
# walk skips the cell it refuses, so a bad offset shows as a differing record.  The library is chosen when the package is
# imported, hence the child process: this file run as a script.

def _guard_child():
    from qr_loader import load_package
    qr = load_package()
    assert qr.LIB_PATH == GUARD_LIB, qr.LIB_PATH
    import qr_oracle
    rays_mod, helper = _rays_mod(), _helper()
    done = 0
    for name in ("synth_small", "synth_small_dda", "swarm_demo01_240"):
        blob = RS.scene_blob(name)
        scn = _rs_scene(qr, name)
        for label, rays in (("camera", rays_mod.camera_rays(blob)), ("mixed", RS.mixed(blob, name, qr_oracle))):
            _check_hits(scn, f"guard {name} {label}", rays, helper(blob, rays))
        views = [rays_mod.view_of(blob)] + [rays_mod.view_of(c) for c in _rayq.random_cameras(blob, seed=11, n=2)]
        _check_views(scn, blob, rays_mod, helper, f"guard {name}", views, 67, 45)
        scn.close()
        done += 1
        print(f"{name} guard_ok 1", flush=True)
    return 0 if done == 3 else 1


@pytest.mark.gpu
def test_gpu_guarded_build_gives_the_same_records():
    assert os.path.exists(GUARD_LIB), "libqrhip_guard.so is missing: build() makes it (make -C quadray-engine_amd/csrc guard)"
    env = dict(os.environ, QR_LIB=GUARD_LIB)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-child"], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.count("guard_ok 1") == 3 and "QR_GUARD" not in out.stderr, out.stdout + out.stderr[-3000:]


if __name__ == "__main__":
    sys.exit(_guard_child() if "--guard-child" in sys.argv else 2)
