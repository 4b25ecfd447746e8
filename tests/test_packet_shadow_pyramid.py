"""Packet shadow pyramids (csrc/qr_program.h: CGrid with QR_GRIDC_PYR; csrc/qr_builder.cpp compile_pgrid; the vote in
csrc/qr_shade.hpp): in an image the packet kernel instance serves, a large clipped plane's shadow chain is filtered per node of
a 2^L x 2^L pyramid over the plane's rectangle, and a wave walks the one node that covers the cells of all its shadow rays.

CPU: the records of the dumped image (tests/_pyramid.py on tests/_noshad.ShadowImage: a reader that shares nothing with the
compiler's verifier), on demo01_160 -- whose floor is the plane the work was done for -- and on a hand-made scene with a
trnode, a surface that casts no shadow, a low light and an occluder over the rectangle's centre lines; and, by the oracle alone,
that a node's list loses no occluder: shadow rays from a lattice over the node's patch see through the node's chain what they
see through the floor's whole chain.
GPU: frames, hit ids and ray counts equal the oracle's with the pyramids, without them (QR_PGRID=0) and through the per-lane
instance reading level 0 (QR_DIV=1); the packet view instance from cameras that graze the plane, look straight down at it and
straddle its edge; row-range launches compose."""

import numpy as np
import pytest

import _noshad
import _pyramid as P
from conftest import load_blob
from test_render_views import _view_snapshot

# program_stats of demo01_160 before the pyramids existed: QR_PGRID=0 must give that image
DEMO01_160_PLAIN = dict(bytes=333888, n_lists=90, n_cells=1141, n_dropped=31, n_clip_cells=52, n_sched=201, n_grids=0, n_grid_lists=0, n_dda=0)
UNTOUCHED = ("n_clip_cells", "n_sched", "n_grids", "n_grid_lists", "n_dda")


@pytest.fixture(scope="module")
def rays_mod():
    import importlib
    from qr_loader import load_package
    load_package()
    return importlib.import_module("quadray_engine_amd.rays")


def _blob(name):
    return P.scene()[0] if name == "handmade" else load_blob(name)


def _dump(qr, name, tmp_path, env=None):
    blob = _blob(name)
    st, img = _noshad.dump_image(qr, blob, str(tmp_path / "img.bin"), env)
    return blob, st, img


@pytest.mark.parametrize("name", ["demo01_160", "handmade"])
def test_structure(qr, tmp_path, name):
    blob, st, img = _dump(qr, name, tmp_path)
    im = _noshad.ShadowImage(blob, img)
    pyr, plain = P.pyramids(im)
    assert len({p.table for p, _ in pyr.values()}) == st.n_pgrids >= (2 if name == "handmade" else 1)
    # the packet instance is still chosen: nothing that needs the per-lane one
    assert (st.n_grids, st.n_grid_lists, st.n_dda) == (0, 0, 0)
    # level 0 is a CGrid table: the reader of the shadow grids takes it for one (sizes, every cell a sub-sequence of the chain),
    # and every plain shadow word is the chain's shadow program
    n = im.check()
    assert n["grids"] == st.n_pgrids and n["refs"] == sum(1 for e in plain if e[3] >= 0)
    nodes = 0
    seen = set()
    for (i, side, lgt), (p, head) in pyr.items():
        assert p.L == 4 and p.nx == p.ny == 16
        assert im.s[i, 37] == 0 and im.s[i, 15] == 0, "a pyramid on something else than an untransformed plane"
        if p.table not in seen:
            nodes += P.check_pyramid(im, p, head)
            seen.add(p.table)
    assert nodes == st.n_pgrid_nodes
    if name == "handmade":
        info = P.scene()[1]
        assert {k[0] for k in pyr} == {info["floor"]} and {k[2] for k in pyr} == {0, 1}
        # the trnode's members do show up below the top, behind their node's cell (check_pyramid), and the surface that casts
        # no shadow nowhere
        for p, _ in pyr.values():
            low = [c for l in range(p.L) for ij in p.nodes(l) if p.node(l, *ij) for c in P.cells(im, p.node(l, *ij))]
            assert any(t == P.OPT_TRNODE and s == info["node"] for t, s, _ in low)
            assert any(s in info["members"] and op & P.OPF_CACHED for _, s, op in low)
            assert not any(s == info["transparent"] for _, s, _ in low)


@pytest.mark.parametrize("name", ["demo01_160", "handmade"])
def test_image_does_not_depend_on_host_threads(qr, tmp_path, name):
    imgs = [_dump(qr, name, tmp_path, {"QR_HOST_THREADS": t})[2] for t in (1, 3, 8)]
    assert all(a.size == imgs[0].size and (a == imgs[0]).all() for a in imgs[1:])


@pytest.mark.parametrize("name", ["demo01_160", "handmade"])
def test_knob_off_is_the_plain_image(qr, tmp_path, name):
    blob, on, _ = _dump(qr, name, tmp_path)
    _, off, img = _dump(qr, name, tmp_path, {"QR_PGRID": 0})
    im = _noshad.ShadowImage(blob, img)
    pyr, plain = P.pyramids(im)
    assert not pyr and (off.n_pgrids, off.n_pgrid_nodes) == (0, 0)
    assert im.check()["grids"] == 0
    assert all(getattr(on, k) == getattr(off, k) for k in UNTOUCHED)
    assert on.n_pgrids > 0 and on.n_lists > off.n_lists
    if name == "demo01_160":
        assert {k: getattr(off, k) for k in DEMO01_160_PLAIN} == DEMO01_160_PLAIN


def test_long_lists_get_no_pyramid(qr):
    """an image that needs the per-lane instance (a crowd's long lists and shadow grids) is built without pyramids"""
    st = qr.program_stats(_noshad.scene_blob("flat_lights"))
    assert st.n_pgrids == 0 and st.n_pgrid_nodes == 0


# ---- conservativeness, by the oracle alone -------------------------------------------------------------------------

def _shadow_rays(p, geo, l, i, j, light):
    """the lattice over a node's patch (tests/_pyramid.py node_shadow_rays), on the plane whose a, b, pos and min / max `geo` holds"""
    return P.node_shadow_rays(p, geo, l, i, j, light)


@pytest.mark.parametrize("level", [0, 2])
def test_nodes_lose_no_occluder(qr, oracle, tmp_path, level):
    blob, st, img = _dump(qr, "handmade", tmp_path)
    info = P.scene()[1]
    im = _noshad.ShadowImage(blob, img)
    pyr, _ = P.pyramids(im)
    whole = P.scene(query=info["shadow_chain"])[0]
    n_rays = n_occ = n_short = 0
    for (srf, side, lgt), (p, head) in sorted(pyr.items()):
        assert p.comp == (0, 1) and p.org == (-P.HALF, -P.HALF)
        geo = P.plane_geometry(blob, srf)
        assert geo[:3] == (2, 0, 1) and (geo[3] == 0).all() and (geo[4][:2] == -P.HALF).all() and (geo[5][:2] == P.HALF).all()
        by_list = {}
        for (i, j) in p.nodes(level):
            w = p.node(level, i, j)
            kept = tuple(s for _, s, _ in P.cells(im, w)) if w else ()
            by_list.setdefault(kept, []).append(_shadow_rays(p, geo, level, i, j, P.LIGHTS[lgt]))
        for kept, rays in by_list.items():
            rays = np.concatenate(rays)
            want = oracle.trace_rays(whole, rays, "occluded", threads=8)
            got = oracle.trace_rays(P.scene(query=kept)[0], rays, "occluded", threads=8) if kept else np.zeros(len(rays), dtype=bool)
            assert (got == want).all(), f"light {lgt} level {level}: {int((got != want).sum())} of {len(rays)} rays lose their occluder with {kept}"
            n_rays += len(rays); n_occ += int(want.sum()); n_short += len(kept) < len(info["shadow_chain"]) - 1
    # the lattice is no empty exercise: rays in shadow and rays in the light, through lists that are shorter than the chain
    assert n_occ > 50 and n_rays - n_occ > 50 and n_short > 0


# ---- GPU ------------------------------------------------------------------------------------------------------------

ENVS = ({}, {"QR_PGRID": "0"}, {"QR_DIV": "1"})
_TRUTH = {}


def _oracle(oracle, name):
    if name not in _TRUTH:
        blob = _blob(name)
        f, ids, _ = oracle.render(blob, threads=8, want_ids=True)
        _, _, cnt = oracle.render(blob, threads=8, deferred=True)
        _TRUTH[name] = (f, ids, cnt)
    return _TRUTH[name]


def _scene(qr, blob, env, **kw):
    with _noshad.env(env):
        return qr.Scene(blob, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["demo01_160", "demo02_160", "handmade", "swarm_demo01_240_mix"])
def test_gpu_frames_ids_counts(qr, oracle, name):
    import torch
    blob = _blob(name)
    ref, ref_ids, ref_cnt = _oracle(oracle, name)
    for env in ENVS:
        scn = _scene(qr, blob, env)
        frame = scn.new_frame(); ids = torch.full_like(frame, -2)
        scn.render(frame, ids=ids)
        _, c = scn.render_count()
        torch.cuda.synchronize()
        out, got_ids, cnt = frame.cpu().numpy().view(np.uint32), ids.cpu().numpy(), c.as_dict()
        scn.close()
        assert int((out != ref).sum()) == 0, f"{name} {env}: {int((out != ref).sum())} pixels differ from the oracle"
        assert (got_ids == ref_ids).all(), f"{name} {env}: hit ids"
        assert cnt == {k: ref_cnt[k] for k in cnt}, f"{name} {env}: ray counts"


@pytest.mark.gpu
def test_gpu_packet_view_instance(qr, oracle, rays_mod):
    import torch
    blob = P.scene()[0]
    w, h = 160, 96
    views = [rays_mod.view_of(blob),
             rays_mod.look_at((-14.0, 0.5, 0.6), (6.0, 0.0, 0.0), (0, 0, 1), 50.0, w, h),       # grazing the plane
             rays_mod.look_at((0.0, 0.0, 12.0), (0.0, 0.0, 0.0), (0, 1, 0), 60.0, w, h),         # straight down at the centre
             rays_mod.look_at((9.0, -12.0, 5.0), (8.0, -8.0, 0.0), (0, 0, 1), 55.0, w, h)]       # the rectangle's corner mid-frame
    for env in ENVS[:2]:
        scn = _scene(qr, blob, env, ray_queries=True)
        v = torch.from_numpy(np.ascontiguousarray(np.stack(views), dtype=np.float32)).to(f"cuda:{scn.device}")
        f, ids = scn.render_views(v, w, h, ids=True)
        torch.cuda.synchronize()
        f, ids = f.cpu().numpy().view(np.uint32), ids.cpu().numpy()
        scn.close()
        floor = 0
        for j, view in enumerate(views):
            ref, ref_ids, _ = oracle.render(_view_snapshot(blob, view, w, h), threads=8, want_ids=True)
            assert (f[j] == ref).all(), f"view {j} {env}: {int((f[j] != ref).sum())} pixels differ"
            assert (ids[j] == ref_ids).all(), f"view {j} {env}: hit ids"
            on = (ref_ids >> 1) == P.scene()[1]["floor"]
            assert 200 < on.sum() < on.size, f"view {j}: the floor covers {int(on.sum())} pixels"
            floor += int(on.sum())
        assert floor > 4 * 2000


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["demo01_160", "handmade"])
def test_gpu_row_ranges_compose(qr, name):
    import torch
    scn = qr.Scene(_blob(name))
    whole = scn.new_frame(); scn.render(whole)
    acc = torch.zeros_like(whole)
    half = (scn.height // 2) & ~7
    for r0, r1 in ((0, half), (half, scn.height)):
        scn.set_rows(r0, r1)
        scn.render(acc)
    torch.cuda.synchronize()
    scn.close()
    assert (acc.cpu().numpy() == whole.cpu().numpy()).all()
