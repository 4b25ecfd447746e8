"""Ray queries and ray shading (include/qrhip.h qr_trace_rays_async, qr_occluded_async, qr_shade_rays_async) on adversarial
rays (tests/_rayset.py): axis-aligned and near-axis directions with +-0 and denormal components, origins on the cells of a
uniform grid, intervals at and around hits, negative tmin, directions scaled by 2^-60 .. 2^40, far origins, probe rays from
hit points -- against the oracle's restatement of the same contract (oracle/qr_oracle.c qro_trace_rays), bit for bit.

Every walk these rays start ends (checked by reading before the first GPU run):
  - walk_list (with or without its culls), walk_div and walk_pool only advance their cursor through the list program (resume offsets point forward);
    what a ray's numbers are changes which cells it solves, not how far the cursor goes.
  - walk_dda moves one cell index by +-1 per step, in a direction fixed per axis for the stretch; the march ends when an
    index leaves the grid or the next face lies beyond the stretch's end.  An inf or NaN increment can make the march
    visit the wrong cells (a wrong answer, which the comparison sees) but not go on for ever: at most nx + ny + nz steps.
The families stay inside the contract's domain: finite origins and directions, no zero-length direction, finite tmin.
"""
import os

import numpy as np
import pytest

import _rayq
import _rayset as RS
from conftest import load_blob
from test_ray_query import NON_PT_SMALL

NEEDED_FLAGS = [0, RS.LISTF_DIV | RS.LISTF_WORLD, RS.LISTF_DIV | RS.LISTF_LONG | RS.LISTF_WORLD]


@pytest.fixture(scope="module")
def rays_mod():
    import importlib
    from qr_loader import load_package
    load_package()
    return importlib.import_module("quadray_engine_amd.rays")


# ---------------------------------------------------------------------------------------------------------------- CPU:
# the oracle entry against the already pinned frames

@pytest.mark.parametrize("name", NON_PT_SMALL)
def test_oracle_trace_rays_gives_frame_ids(oracle, rays_mod, name):
    """camera rays traced by qro_trace_rays give the ids of the frame rendered from the same camera over the global list"""
    blob = _rayq.with_frame(load_blob(name))
    _, ref, _ = oracle.render(blob, depth=0, threads=16, want_ids=True)
    t, ids = oracle.trace_rays(blob, rays_mod.camera_rays(blob), "trace")
    assert (ids == ref.reshape(-1)).all(), f"{int((ids != ref.reshape(-1)).sum())} ids differ"
    f, _ = rays_mod.frame_record(blob)
    assert (t[ids < 0] == f[0]).all(), "a miss gives tmax"


@pytest.mark.parametrize("name", NON_PT_SMALL)
def test_oracle_shade_rays_gives_frame(oracle, rays_mod, name):
    """the shaded camera rays of every FSAA sample, packed by rays.pack_colors, give the oracle's one-tile frame (the
    fixture's own depth, FSAA, gamma and Fresnel); the first hit's ids are the frame's"""
    blob = load_blob(name)
    ref, ref_ids, _ = oracle.render(_rayq.one_tile(blob), threads=16, want_ids=True)
    ns = 1 << int(_rayq.frame_words(blob)[0][30])
    out = [oracle.trace_rays(blob, rays_mod.camera_rays(blob, sample=k), "shade") for k in range(ns)]
    frame = rays_mod.pack_colors(np.stack([c for c, _ in out]), blob)
    assert (frame == ref).all(), f"{int((frame != ref).sum())} pixels differ"
    assert (out[0][1] == ref_ids.reshape(-1)).all()


def _opaque(blob):
    b = bytearray(blob)
    h = _rayq._hdr(b)
    s = np.frombuffer(b, dtype=np.int32, count=h[4] * 64, offset=h[11]).reshape(h[4], 64).copy()
    s[:, 42:44] &= ~(_rayq.PROP_LIGHT | _rayq.PROP_TRANSP)
    b[h[11]:h[11] + s.nbytes] = s.tobytes()
    return bytes(b)


def test_oracle_occlusion_on_opaque_scene_is_hit(oracle, rays_mod):
    """every surface made to cast: occlusion is 'hits something', for camera rays and for every adversarial family"""
    blob = _opaque(load_blob("demo02_160"))
    rays = [rays_mod.camera_rays(_rayq.with_frame(blob))]
    rays += [RS.family(blob, "demo02_160", f, oracle) for f in RS.FAMILIES if f not in ("grid", "mixed")]
    rays = np.concatenate(rays)
    _, ids = oracle.trace_rays(blob, rays, "trace")
    occ = oracle.trace_rays(blob, rays, "occluded")
    assert (ids >= 0).any() and (ids < 0).any()
    assert (occ == (ids >= 0)).all()


# demo02_160's camera rays whose closest hits are on surfaces that cast no shadow (both sides of a transparent body), with a
# caster behind them: the oracle's answers, written down as (pixel index, closest id, first casting id behind it,
# occluded with tmax = +inf, occluded with tmax halfway between the last non-casting hit and the caster)
NONCAST_FIRST = [(7909, 10, 6, True, False), (8066, 16, 6, True, False)]


def test_oracle_occlusion_noncasting_surface_in_front(oracle, rays_mod):
    """a non-casting hit does not shorten the interval of the occlusion walk: the caster behind it occludes, and nothing
    does once tmax stops short of the caster.  The CHECK_SHAD rule is 'any hit in the interval on a surface that casts',
    whatever the list order"""
    blob = _rayq.with_frame(load_blob("demo02_160"))
    cast = _rayq.casts(blob)
    got = []
    for p, _, _, _, _ in NONCAST_FIRST:
        r = rays_mod.camera_rays(blob)[p:p + 1].copy()
        chain = []
        q = r.copy()
        while True:                                     # the hits along the ray, one by one: tmin = the previous t
            t, i = oracle.trace_rays(blob, q, "trace")
            assert i[0] >= 0 and len(chain) < 8
            chain.append((int(i[0]), float(t[0])))
            if cast[i[0] >> 1, i[0] & 1]:
                break
            q[0, 3] = t[0]
        short = r.copy()
        short[0, 7] = np.float32((chain[-2][1] + chain[-1][1]) / 2)
        got.append((p, chain[0][0], chain[-1][0], bool(oracle.trace_rays(blob, r, "occluded")[0]),
                    bool(oracle.trace_rays(blob, short, "occluded")[0])))
        assert len(chain) >= 2
    assert got == NONCAST_FIRST


# ---------------------------------------------------------------------------------------------------------------- CPU:
# the generators and the lists they run on

@pytest.fixture(scope="module")
def images(qr, tmp_path_factory):
    d = tmp_path_factory.mktemp("qimg")
    return {n: RS.query_image(qr, n, d) for n in RS.SCENES}


def test_query_lists_cover_the_walks(images):
    """the scenes' query lists carry the flags 0 (packet walk only), DIV|WORLD, DIV|LONG|WORLD and a uniform grid: a threshold
    that moves fails here instead of thinning out the GPU comparison"""
    flags = {n: off & 31 for n, (off, _) in images.items()}
    for want in NEEDED_FLAGS:
        assert want in flags.values(), (want, flags)
    assert any(f & RS.LISTF_DDA for f in flags.values()), flags
    assert flags["synth_small_dda"] & RS.LISTF_DDA and flags["synth_flat_dda"] & RS.LISTF_DDA
    assert flags["synth_dense_dda"] & RS.LISTF_DDA
    assert flags["synth_small"] == RS.LISTF_DIV | RS.LISTF_LONG | RS.LISTF_WORLD
    assert flags["synth_flat"] == RS.LISTF_DIV | RS.LISTF_WORLD
    assert flags["demo01_160"] == 0 and flags["swarm_demo01_240"] == 0
    # engine-authored surfaces of every kind (tests/_crowd.py) on the hand-over walk, and under a grid: a flat list with four
    # unbounded members, a dense one with built lists
    assert flags["crowd_hier"] == RS.LISTF_DIV | RS.LISTF_LONG | RS.LISTF_WORLD
    assert flags["crowd_flat_dda"] == RS.LISTF_DIV | RS.LISTF_WORLD | RS.LISTF_DDA
    assert flags["crowd_dense_dda"] == RS.LISTF_DIV | RS.LISTF_WORLD | RS.LISTF_DDA


@pytest.mark.parametrize("name", sorted(RS.SCENES))
def test_families_shapes(oracle, images, name):
    blob = RS.scene_blob(name)
    g = RS.dda_grid(*images[name])
    reach = RS.reach_of(images[name][1])
    sizes = {}
    for f in RS.FAMILIES:
        r = RS.family(blob, name, f, oracle, g, reach)
        assert r.dtype == np.float32 and r.ndim == 2 and r.shape[1] == 8, f
        assert np.isfinite(r[:, [0, 1, 2, 3, 4, 5, 6]]).all() or f in ("interval", "mixed"), f
        assert not np.isnan(r).any(), f
        assert (np.abs(r[:, 4:7]).max(axis=1) > 0).all(), f"{f}: zero-length direction"
        sizes[f] = len(r)
        if f == "grid" and g is None:
            assert len(r) == 0
        else:
            assert len(r) > 0, f
    assert sizes["mixed"] % 2 == 1
    again = RS.family(blob, name, "mixed", oracle, g, reach)
    assert again.tobytes() == RS.family(blob, name, "mixed", oracle, g, reach).tobytes(), "not deterministic"
    # the far family straddles the reach: origins whose largest coordinate lies just inside it and just outside
    o = np.abs(RS.far(blob, name, reach)[:, 0:3]).max(axis=1)
    assert ((o < reach) & (o > 0.9 * reach)).sum() >= 64 and ((o > reach) & (o < 1.1 * reach)).sum() >= 64


def test_reach_in_image_header(images):
    """DevHeader::reach: twice the largest coordinate of the camera origin and of the surfaces' bounds, written with and
    without the query list (the render kernels never read it)"""
    for name, (off, img) in images.items():
        reach = RS.reach_of(img)
        _, ff = _rayq.frame_words(RS.scene_blob(name))
        assert np.isfinite(reach) and reach > 0, name
        assert reach >= 2 * float(np.abs(ff[25:28]).max()), name
        _, f = _rayq.surfaces(RS.scene_blob(name))
        s, _ = _rayq.surfaces(RS.scene_blob(name))
        quad = _rayq.real_surfaces(RS.scene_blob(name))
        quad = quad[s[quad, 34] == 2]                    # quadrics: their centre lies inside their bounds
        if len(quad):
            assert reach >= 2 * float(np.abs(f[quad, 0:3]).max()) * (1 - 1e-6), name


def test_axis_families_hold_signed_zeros_and_denormals(oracle):
    blob = RS.scene_blob("demo01_160")
    d = RS.axis(blob, "demo01_160")[:, 4:7].view(np.uint32)
    assert (d == 0x00000000).any() and (d == 0x80000000).any()
    n = RS.near_axis(blob, "demo01_160")[:, 4:7]
    bits = set(np.unique(n.view(np.uint32) & 0x7FFFFFFF).tolist())
    for m in (1e-20, 1e-30, 1e-38, 1.4e-45):
        assert int(np.float32(m).view(np.uint32)) in bits, m
    assert (n.view(np.uint32) == 0x80000001).any() and (n.view(np.uint32) == 0x00000001).any()
    assert not (n == 0).any()


def test_grid_family_origins_on_cell_faces(oracle, images):
    name = "synth_dense_dda"
    org, dims, size = RS.dda_grid(*images[name])
    r = RS.grid(RS.scene_blob(name), name, (org, dims, size))
    on = np.zeros((len(r), 3), dtype=bool)
    for a in range(3):
        faces = (org[a] + np.arange(dims[a] + 1, dtype=np.float32) * size[a]).astype(np.float32)
        on[:, a] = np.isin(r[:, a], faces)
    assert on.any(axis=1).sum() >= 7 * 48, "faces, edges and corners"
    assert (on.sum(axis=1) >= 2).sum() >= 4 * 48 and (on.sum(axis=1) == 3).sum() >= 48
    in_plane = (r[:, 4:7] == 0) & on
    assert in_plane.any(axis=1).sum() >= 3 * 48, "rays inside a cell-face plane"


def test_interval_family_edges(oracle):
    name = "demo02_160_gf_d5"
    r = RS.interval(RS.scene_blob(name), name, oracle)
    assert (r[:, 3] == r[:, 7]).any() and (r[:, 3] > r[:, 7]).any()
    assert (r[:, 7] == 0).any() and (r[:, 7] == RS.DENORM_MIN).any()
    for tmn in (-1.0, -RS.FLT_MAX):
        assert (r[:, 3] == np.float32(tmn)).any()


# ---------------------------------------------------------------------------------------------------------------- GPU

_SCN = {}


def _scene(qr, name):
    if name not in _SCN:
        with RS.upload_env(name):
            _SCN[name] = qr.Scene(RS.scene_blob(name), ray_queries=True)
    return _SCN[name]


def _grid_of(qr, name, tmp_path):
    """(dda_grid, reach_of) of the scene's query image"""
    off, img = RS.query_image(qr, name, tmp_path)
    return RS.dda_grid(off, img), RS.reach_of(img)


def _first(rays, bad, got, want):
    idx = np.nonzero(bad)[0][:3]
    return "; ".join(f"ray {int(i)} {rays[i].tolist()} got {got[i]} want {want[i]}" for i in idx)


def _same_bits(what, fam, rays, got, want):
    g = np.ascontiguousarray(got).reshape(len(rays), -1).view(np.uint32)
    w = np.ascontiguousarray(want).reshape(len(rays), -1).view(np.uint32)
    bad = (g != w).any(axis=1)
    assert not bad.any(), f"{fam}: {what}: {int(bad.sum())} of {len(rays)} rays differ: " + _first(rays, bad, got, want)


def _gpu(scn, rays_np, call, **kw):
    import torch
    r = torch.from_numpy(np.ascontiguousarray(rays_np, dtype=np.float32)).to(f"cuda:{scn.device}")
    out = getattr(scn, call)(r, **kw)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out) if isinstance(out, tuple) else out.cpu().numpy()


def _check_families(qr, oracle, name, families, tmp_path):
    blob = RS.scene_blob(name)
    g, reach = _grid_of(qr, name, tmp_path)
    scn = _scene(qr, name)
    depth = int(_rayq.frame_words(blob)[0][29])
    try:
        for fam in families:
            _check_family(scn, oracle, blob, name, fam, RS.family(blob, name, fam, oracle, g, reach), depth)
    finally:
        scn.set_depth(depth)                # the scene is shared by the module's tests


def _check_family(scn, oracle, blob, name, fam, rays, depth):
    if len(rays) == 0:
        return
    t_w, id_w = oracle.trace_rays(blob, rays, "trace")
    for coherent in (False, True):
        t, ids = _gpu(scn, rays, "trace", coherent=coherent)
        _same_bits(f"trace ids coherent={coherent}", fam, rays, ids, id_w)
        _same_bits(f"trace t coherent={coherent}", fam, rays, t, t_w)
    occ = _gpu(scn, rays, "occluded").astype(np.uint8)
    _same_bits("occluded", fam, rays, occ.astype(np.uint32), oracle.trace_rays(blob, rays, "occluded").astype(np.uint32))
    for d in sorted({0, depth}):
        scn.set_depth(d)
        rgb, ids = _gpu(scn, rays, "shade", ids=True)
        rgb_w, ids_w = oracle.trace_rays(blob, rays, "shade", depth=d)
        _same_bits(f"shade ids depth {d}", fam, rays, ids, ids_w)
        _same_bits(f"shade rgb depth {d}", fam, rays, rgb, rgb_w)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RS.SCENES))
def test_gpu_edge_rays_equal_oracle(qr, oracle, name, tmp_path):
    """every family of the scene: trace (t as bits and ids, packet and per-lane walks), occlusion, and shade (rgb as bits and
    ids at depth 0 and at the scene's depth) equal the oracle's"""
    _check_families(qr, oracle, name, RS.FAMILIES, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 65])
def test_gpu_edge_rays_small_batches(qr, oracle, n, tmp_path):
    """n = 1 and n = 65 of the mixed family on the dense grid scene: a partial wave"""
    name = "synth_dense_dda"
    blob = RS.scene_blob(name)
    rays = RS.mixed(blob, name, oracle, *_grid_of(qr, name, tmp_path))[:n]
    scn = _scene(qr, name)
    t_w, id_w = oracle.trace_rays(blob, rays, "trace")
    t, ids = _gpu(scn, rays, "trace")
    _same_bits("trace ids", "mixed", rays, ids, id_w)
    _same_bits("trace t", "mixed", rays, t, t_w)
    rgb, ids = _gpu(scn, rays, "shade", ids=True)
    rgb_w, ids_w = oracle.trace_rays(blob, rays, "shade")
    _same_bits("shade rgb", "mixed", rays, rgb, rgb_w)
