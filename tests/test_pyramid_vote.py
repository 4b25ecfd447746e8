"""The packet shadow pyramid's vote (csrc/qr_shade.hpp, the packet arm of the light loop) and its compiler (csrc/qr_builder.cpp
compile_pgrid) on every input they read, on a scene built for the purpose: the room of tests/_pyramid.py -- four clipped planes of
all three normal axes, two with the plane sign, every pos far from its rectangle, every rectangle two to four times as long as
wide with min != -max, a chain of its own content for every plane, three lights of which one stands behind a wall -- compiled
with QR_PGRID_LEVELS 1, 3, 4 and 6.

Who runs which arm.  The vote is the arm of the instances with packet walks: render, render_views, render_views_mean and the view
gathers of a scene the packet instance serves.  Scene.shade, Scene.gather and Scene.hit_gather on caller rays run the per-lane
instance (qr_shade_rays_kernel is render_wave<.., DIVK = true, ..>), which reads level 0 of the same record with the same comps,
org and inv, as QR_DIV=1 makes every launch do.  So a wave's 64 hits are placed through a CAMERA here (an 8 x 8 footprint is a
wave, lane 8 (y & 7) + (x & 7)): _pyramid.vote_views looks straight at each plane so that the pixels fall on an exact lattice
of the plane -- whole footprints in one cell, footprints over borders of every bit of ia and of ib, over corners of four cells,
over 4 x 4 cells, pixel rows ON every border and rim line, the four corners with misses beyond them -- and _pyramid.room_views
adds four perspective cameras, one along the edge two planes share, whose footprints hold lanes of two records.  The same rays,
as caller rays for Scene.shade, hold the per-lane arm.

CPU
  the room is a scene: the oracle's closest hits and occlusion agree with the float64 caster (tests/_f64xform.py) on 4 x 1 024
    camera rays and the `inside` rays, under the bounds and caps of tests/test_f64_caster.py;
  structure at levels 1, 3, 4, 6; the image does not depend on QR_HOST_THREADS; a census of the committed fixtures' pyramids;
  conservativeness of every node list of every (plane, light) pyramid, levels 0..4 of a 4-level pyramid and level 0 of a 6-level one;
  _pyramid.vote states the arm in numpy, and eight wrong votes (MUTANTS) are stated with it.  A witness of a mutant is a lane of
    a constructed wave whose shadow ray is occluded through the whole chain and not through the list of the node the mutant
    picks -- a lane that mutant would light.  Asserted: every mutant has at least 8 witnesses in at least 2 waves, swap_ab,
    swap_inv and world on planes of two different k, and the correct vote has none.
    Counted here (levels 4; levels4 at levels 6, where it differs from the vote; the correct vote: 0 at 1, 4 and 6):
      no_climb 1676 lanes in 93 waves, one_short 198 / 26, swap_ab 86573 / 1434, swap_inv 33974 / 757, world 54549 / 1072,
      first_record 290 / 20 (floor and back wall), levels4 89438 / 1410, no_clamp_hi 217 / 23 (profiles/r35_pyramid_vote.txt).
    no_clamp_hi differs from the vote only for a hit ON the rim line max[a], where the unclamped index is n: its witnesses are
    counted on those lanes (exact arithmetic on the room's numbers) and keep the border distance in b alone.  Every other
    witness lies 1e-3 of a level-0 cell away from every cell border.
GPU (bit for bit against the oracle, nothing left out)
  render_views of every constructed view and of the four cameras (160 x 96 and 67 x 45) at levels 1, 4 and 6, under {}, QR_PGRID=0
  and QR_DIV=1, depth 0 and depth 2 (secondary hits vote too); render with ids and ray counts, row ranges; render_views_mean;
  view_gather; Scene.shade on the same rays with and without `coherent`, reversed and shuffled; hit_gather on 1 024 of their hit records; the
  depth-0 views, one render and shade once more through the guarded build.  Every case under {}, QR_PGRID=0 and QR_DIV=1.
Not held: pyramids of the per-frame compile of qr_render0 (QR_DROPIN_PGRID=1), path-tracer modes (no shadow rays), planes under a
trnode (grid_plane refuses them), whether a lane that sends no ray is wrongly let into the vote (speed, not pixels), a wave
whose LEADER alone sits in one cell with the other 63 elsewhere (a camera cannot place that, and caller rays do not vote), and
the LOWER clamps ia < 0, ib < 0: a hit ON min[a] gives floor(0) = 0 and a hit below it is clipped away, so no lane reaches -1;
only the upper clamp (index n, a hit ON max[a]) is reached.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import _noshad
import _pyramid as P
import _rayq
import test_f64_caster as T
from conftest import MANIFEST, load_blob
from test_hit_records import GUARD_LIB, _helper, _rays_mod
from test_render_views import _view_snapshot

LEVELS = (1, 3, 4, 6)
GPU_LEVELS = (1, 4, 6)
GPU_CASES = [(1, 0), (4, 0), (6, 0), (4, 2)]                   # the depth-0 room at three pyramid sizes, the depth-2 room at 4
ENVS = ({}, {"QR_PGRID": "0"}, {"QR_DIV": "1"})
W, H = 160, 96


@pytest.fixture(scope="module")
def rays_mod():
    return _rays_mod()


@pytest.fixture(scope="module")
def helper():
    return _helper()


_IMAGES, _WAVES = {}, {}


def _image(qr, levels, extra=None):
    """(blob, info, program_stats, ShadowImage, {(surface, side, light): (Pyramid, head)}) of the room compiled with `levels`"""
    key = (levels, tuple(sorted((extra or {}).items())))
    if key not in _IMAGES:
        blob, info = P.room(levels=levels)
        with tempfile.TemporaryDirectory() as d:
            st, img = _noshad.dump_image(qr, blob, os.path.join(d, "img.bin"), dict(info["env"], **(extra or {})))
        im = _noshad.ShadowImage(blob, img)
        _IMAGES[key] = (blob, info, st, im, P.pyramids(im)[0])
    return _IMAGES[key]


def _tables(pyr):
    """one entry per record: {(surface, light): (Pyramid, head)} (a plane's two sides share their light list)"""
    out = {}
    for (srf, side, lgt), ph in sorted(pyr.items()):
        out.setdefault((srf, lgt), ph)
    return out


def _views(rays_mod, levels):
    """[(label, view, w, h)]: the lattices of `levels` and the four cameras at 160 x 96"""
    blob, info = P.room(levels=levels)
    return P.vote_views(blob, info, levels) + [(l, v, W, H) for l, v in P.room_views(rays_mod, blob, W, H)]


def _waves(rays_mod, helper, levels):
    """(rays [n, 8], records [n_waves, 64, 12], inside [n_waves, 64], label per wave) of the constructed views, footprint by footprint"""
    if levels not in _WAVES:
        blob = P.room()[0]
        rays, recs, ins, labels = [], [], [], []
        for label, v, w, h in _views(rays_mod, levels):
            r = rays_mod.view_rays(v, w, h, blob)
            idx, inside = P.footprints(w, h)
            rays.append(r); recs.append(helper(blob, r)[idx]); ins.append(inside); labels += [label] * len(idx)
        out = (np.concatenate(rays), np.concatenate(recs), np.concatenate(ins), labels)
        for a in out[:3]:
            a.setflags(write=False)
        _WAVES[levels] = out
    return _WAVES[levels]


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_room_is_a_scene(oracle, rays_mod):
    """before anything else: the oracle on the room against the float64 caster, bounds and caps of tests/test_f64_caster.py"""
    import _f64xform as X
    blob, info = P.room()
    s, f = _rayq.surfaces(blob)
    k_seen, signed = set(), 0
    for name, srf in info["planes"].items():
        k, a, b, pos, lo, hi, _ = P.plane_geometry(blob, srf)
        ea, eb = hi[a] - lo[a], hi[b] - lo[b]
        assert s[srf, 15] == 0 and s[srf, 19] == 0 and s[srf, 23] == P.ROOM_AXES[name][2]
        assert (pos != 0).all() and max(abs(pos[a]) / ea, abs(pos[b]) / eb) > 1, f"{name}: pos {pos}"
        assert max(ea / eb, eb / ea) >= 2 and lo[a] != -hi[a] and lo[b] != -hi[b], f"{name}: {ea} x {eb}"
        k_seen.add(k); signed += (int(s[srf, 23]) >> 10) & 1
    assert k_seen == {0, 1, 2} and signed >= 1 and len(info["planes"]) >= 4
    for srf, ch in info["shadow_chains"].items():
        assert len([x for x in ch if 0 <= s[x, 37] < 9 and 1 <= s[x, 34] <= 3]) >= 14
    assert len({tuple(ch) for ch in info["shadow_chains"].values()}) == len(info["planes"])
    dom = X.XDomain(blob)
    cams = _rayq.random_cameras(blob, seed=T._seed("pyramid_room", "camera")[0], n=4, size=32)
    sets = {"camera": np.concatenate([rays_mod.camera_rays(c) for c in cams]), "inside": T.inside_rays(blob, "pyramid_room")}
    assert len(sets["camera"]) == 4 * 1024
    for fam, rays in sets.items():
        c = dom.cast(rays, 1, T.margins("pyramid_room"))
        und, und_occ = 1 - c["decided"].mean(), 1 - c["occ_decided"].mean()
        print(f"room {fam}: {len(rays)} rays, undecided {und:.4f} closest hit, {und_occ:.4f} occlusion")
        assert und <= T.CAP_UNDECIDED and und_occ <= T.CAP_UNDECIDED
        t, ids = oracle.trace_rays(blob, rays, "trace", threads=16)
        hit = T.compare_trace(f"room {fam}", dom, rays, c, t, ids, tb=T.t_bound("pyramid_room"))
        assert hit.sum() >= 200
        T.compare_occluded(f"room {fam}", c, oracle.trace_rays(blob, rays, "occluded", threads=16))


@pytest.mark.parametrize("levels", LEVELS)
def test_room_structure(qr, levels):
    blob, info, st, im, pyr = _image(qr, levels)
    s, f = _rayq.surfaces(blob)
    n_lights = len(_noshad.lights(blob))
    # every plane has a pyramid for every light that enters it on a side
    assert set(pyr) == {(srf, side, l) for srf in info["planes"].values() for side in (0, 1) for l in range(n_lights)}
    assert (st.n_grids, st.n_grid_lists, st.n_dda) == (0, 0, 0)
    n = im.check()
    tables = _tables(pyr)
    assert len({p.table for p, _ in tables.values()}) == len(tables) == st.n_pgrids == n["grids"] == len(info["planes"]) * n_lights
    nodes = 0
    for (srf, lgt), (p, head) in tables.items():
        k, a, b, pos, lo, hi, _ = P.plane_geometry(blob, srf)
        assert p.comp == (a, b) and p.L == levels and p.nx == p.ny == 1 << levels
        assert p.org == (float(f[srf, 4 + a]), float(f[srf, 4 + b]))
        assert p.inv == (float(np.float32(p.nx / (hi[a] - lo[a]))), float(np.float32(p.nx / (hi[b] - lo[b]))))
        assert p.inv[0] != p.inv[1] and p.org[0] != p.org[1]
        assert s[srf, 37] == 0 and s[srf, 15] == 0 and s[srf, 19] == 0
        nodes += P.check_pyramid(im, p, head)
    assert nodes == st.n_pgrid_nodes
    assert {p.comp for p, _ in tables.values()} == {(1, 2), (0, 2), (0, 1)}


@pytest.mark.parametrize("levels", LEVELS)
def test_room_image_does_not_depend_on_host_threads(qr, levels):
    imgs = [_image(qr, levels, {"QR_HOST_THREADS": t})[3].img for t in (1, 3, 8)]
    assert all(a.size == imgs[0].size and (a == imgs[0]).all() for a in imgs[1:])


def census(qr):
    """[(scene, plane, k, pos, extents, lights)] of the pyramids in every committed snapshot load_blob knows"""
    rows = []
    for name in sorted(MANIFEST):
        blob = load_blob(name)
        st = qr.program_stats(blob)
        if st.n_pgrids == 0:
            continue
        with tempfile.TemporaryDirectory() as d:
            _, img = _noshad.dump_image(qr, blob, os.path.join(d, "img.bin"))
        im = _noshad.ShadowImage(blob, img)
        tables = _tables(P.pyramids(im)[0])
        assert len(tables) == st.n_pgrids
        for srf in sorted({k[0] for k in tables}):
            assert im.s[srf, 37] == 0 and im.s[srf, 15] == 0 and im.s[srf, 19] == 0, f"{name}: a pyramid on surface {srf}, no untransformed plane"
            k, a, b, pos, lo, hi, _ = P.plane_geometry(blob, srf)
            rows.append((name, srf, k, tuple(round(float(x), 4) for x in pos), (round(float(hi[a] - lo[a]), 4), round(float(hi[b] - lo[b]), 4)),
                         sorted(l for s_, l in tables if s_ == srf)))
    return rows


def test_census_of_the_fixtures(qr):
    rows = census(qr)
    for r in rows:
        print("%-28s plane %3d k %d pos %-24s extents %-16s lights %s" % (r[0], r[1], r[2], r[3], r[4], r[5]))
    per = {}
    for r in rows:
        per[r[0]] = per.get(r[0], 0) + len(r[5])
    assert per.get("demo01_160", 0) >= 1 and per.get("demo02_160", 0) >= 2
    # the table of profiles/r35_pyramid_vote.txt section 5 is this census, for the scenes it lists
    listed = _profile_census()
    names = {r[0] for r in listed}
    assert len(listed) >= 20 and {"demo01_160", "demo02_160"} <= names
    assert sorted(listed) == sorted((r[0], r[1], r[2], r[3], r[4], tuple(r[5])) for r in rows if r[0] in names), "the profile's census table is stale"


def _profile_census():
    """the rows of section 5 of profiles/r35_pyramid_vote.txt: (scene, plane, k, pos, extents, lights)"""
    import re
    from conftest import ROOT
    rows, on = [], False
    with open(os.path.join(ROOT, "profiles", "r35_pyramid_vote.txt")) as f:
        for line in f:
            if line.startswith("## "):
                on = line.startswith("## 5.")
            elif on and not line.startswith("#") and line.strip():
                m = re.match(r"\s*(\S+)\s+(\d+)\s+(\d)\s+\(([^)]*)\)\s+(\S+) x (\S+)\s+([\d ]+)$", line.rstrip())
                assert m, line
                rows.append((m.group(1), int(m.group(2)), int(m.group(3)), tuple(float(x) for x in m.group(4).split(",")),
                             (float(m.group(5)), float(m.group(6))), tuple(int(x) for x in m.group(7).split())))
    return rows


def _lose_no_occluder(oracle, qr, levels, node_levels):
    blob, info, st, im, pyr = _image(qr, levels)
    lights = _noshad.lights(blob)[:, 1:4]
    total = 0
    for srf in info["planes"].values():
        whole = P.room(query=info["shadow_chains"][srf])[0]
        geo = P.plane_geometry(blob, srf)
        n_rays = n_occ = n_short = 0
        for (s_, lgt), (p, head) in _tables(pyr).items():
            if s_ != srf:
                continue
            for level in node_levels:
                by_list = {}
                for (i, j) in p.nodes(level):
                    w = p.node(level, i, j)
                    kept = tuple(x for _, x, _ in P.cells(im, w)) if w else ()
                    by_list.setdefault(kept, []).append((i, j))
                for kept, nodes in by_list.items():
                    thin = len(nodes) * 14 * 14 > 64 * 64
                    rays = np.concatenate([P.node_shadow_rays(p, geo, level, i, j, lights[lgt], thin) for i, j in nodes])
                    want = oracle.trace_rays(whole, rays, "occluded", threads=16)
                    got = oracle.trace_rays(P.room(query=kept)[0], rays, "occluded", threads=16) if kept else np.zeros(len(rays), dtype=bool)
                    assert (got == want).all(), (f"plane {srf} light {lgt} level {level}: {int((got != want).sum())} of {len(rays)} rays lose "
                                                 f"their occluder with {kept}")
                    n_rays += len(rays); n_occ += int(want.sum()); n_short += len(kept) < len(info["shadow_chains"][srf]) - 1
        print(f"levels {levels} plane {srf}: {n_rays} rays, {n_occ} in shadow, {n_short} lists shorter than the chain")
        # the power condition, per plane
        assert n_occ > 50 and n_rays - n_occ > 50 and n_short > 0, f"plane {srf}: {n_occ} of {n_rays} rays in shadow, {n_short} short lists"
        total += n_rays
    return total


def test_room_nodes_lose_no_occluder(qr, oracle):
    """test_nodes_lose_no_occluder of tests/test_packet_shadow_pyramid.py for every (plane, light) pyramid of the room: a, b, pos
    and min / max of the plane's own record, every level of a 4-level pyramid"""
    _lose_no_occluder(oracle, qr, 4, range(5))


def test_room_cells_of_64_x_64_lose_no_occluder(qr, oracle):
    """level 0 of a 6-level pyramid: the smallest patches, whose padding is the largest share of the cell"""
    _lose_no_occluder(oracle, qr, 6, [0])


def _count(qr, oracle, rays_mod, helper, levels):
    blob, info, st, im, pyr = _image(qr, levels)
    rays, rec, inside, labels = _waves(rays_mod, helper, levels)
    lights = _noshad.lights(blob)[:, 1:4]
    whole = {srf: P.room(query=ch)[0] for srf, ch in info["shadow_chains"].items()}
    wit = P.witnesses(oracle, im, pyr, lights, rec, inside, whole, lambda kept: P.room(query=kept)[0])
    k_of = {srf: P.plane_geometry(blob, srf)[0] for srf in info["planes"].values()}
    for m, found in wit.items():
        print(f"levels {levels} {m}: {len(found)} witness lanes in {len({x[0] for x in found})} waves, planes {sorted({x[2] for x in found})}")
    return wit, k_of, rec, inside, (im, pyr, lights)


def test_vote_statement_meets_every_level_and_two_records(qr, rays_mod, helper):
    """the constructed waves do what they are built for: votes end at every level 0..L, some votes take two and some three turns
    of the loop (lanes of two and of three records vote at once), some waves hold voting lanes, lanes on a plane that do not vote
    and lanes that hit an occluder or miss"""
    blob, info, st, im, pyr = _image(qr, 4)
    rays, rec, inside, labels = _waves(rays_mod, helper, 4)
    lights = _noshad.lights(blob)[:, 1:4]
    levels, two, three, mixed, away = set(), 0, 0, 0, 0
    left = info["planes"]["left"]
    for w in range(len(rec)):
        ids = rec[w].view(np.int32)[:, 7]
        on_plane = inside[w] & (ids >= 0) & np.isin(ids >> 1, list(info["planes"].values()))
        for lgt, (votes, words, lv) in P.vote_wave(im, pyr, rec[w], lights, inside[w]).items():
            levels |= set(lv[votes].tolist())
            n_rec = len(set((ids[votes] >> 1).tolist()))             # a plane's two sides share one record
            two += n_rec >= 2
            three += n_rec >= 3
            mixed += votes.any() and (on_plane & ~votes).any() and (inside[w] & ~on_plane).any()
            away += lgt == 1 and (on_plane & ((ids >> 1) == left) & ~votes).any()
    print(f"levels met {sorted(levels)}, votes of two records {two}, of three {three}, with voting, silent and off-plane lanes {mixed}, left wall away from light 1 {away}")
    assert levels == set(range(5)) and two >= 8 and three >= 4 and mixed >= 8 and away >= 8
    fp = sum(len({int(i) >> 1 for i, o in zip(rec[w].view(np.int32)[:, 7], inside[w]) if o and i >= 0 and (i >> 1) in info["planes"].values()}) >= 2
             for w in range(len(rec)))
    assert fp >= 40, f"{fp} footprints hold pixels of two pyramid planes"


@pytest.mark.parametrize("levels", [4, 1, 6])
def test_mutants_have_witnesses_and_the_vote_has_none(qr, oracle, rays_mod, helper, levels):
    wit, k_of, rec, inside, _ = _count(qr, oracle, rays_mod, helper, levels)
    # the correct vote: a second conservativeness check, on the very rays the GPU renders
    assert wit[None] == [], f"the vote loses the occluder of {len(wit[None])} lanes, first {wit[None][:4]}"
    for m in P.MUTANTS:
        if (m == "levels4") != (levels == 6) or levels == 1:
            continue                                                # levels4 is the vote itself at 4; everything else is asserted at 4
        found = wit[m]
        assert len(found) >= 8 and len({x[0] for x in found}) >= 2, f"{m}: {len(found)} witnesses in {len({x[0] for x in found})} waves"
        if m in ("swap_ab", "swap_inv", "world"):
            assert len({k_of[x[2]] for x in found}) >= 2, f"{m}: witnesses on planes of one k only"


# ---------------------------------------------------------------------------------------------------------------- GPU

_TRUTH = {}


def _scene(qr, blob, env, **kw):
    with _noshad.env(env):
        return qr.Scene(blob, **kw)


def _view_truth(oracle, blob, view, w, h, depth):
    key = (np.asarray(view, dtype=np.float32).tobytes(), w, h, depth)
    if key not in _TRUTH:
        _TRUTH[key] = oracle.render(_view_snapshot(blob, view, w, h), depth=depth, threads=16, want_ids=True)[:2]
    return _TRUTH[key]


def _check_views(scn, oracle, blob, views, depth, where):
    """render_views of [(label, view, w, h)], one launch per frame size, every frame and id plane against the oracle"""
    import torch
    by_size = {}
    for label, v, w, h in views:
        by_size.setdefault((w, h), []).append((label, v))
    for (w, h), vs in by_size.items():
        vt = torch.from_numpy(np.ascontiguousarray(np.stack([v for _, v in vs]), dtype=np.float32)).to(f"cuda:{scn.device}")
        f, ids = scn.render_views(vt, w, h, ids=True)
        torch.cuda.synchronize()
        f, ids = f.cpu().numpy().view(np.uint32), ids.cpu().numpy()
        for j, (label, v) in enumerate(vs):
            ref, ref_ids = _view_truth(oracle, blob, v, w, h, depth)
            assert (f[j] == ref).all(), f"{where} {label} {w}x{h}: {int((f[j] != ref).sum())} pixels differ from the oracle"
            assert (ids[j] == ref_ids).all(), f"{where} {label} {w}x{h}: hit ids"


@pytest.mark.gpu
@pytest.mark.parametrize("levels, depth", GPU_CASES)
def test_gpu_constructed_views(qr, oracle, rays_mod, levels, depth):
    """the vote itself: every constructed wave is a footprint of these views (depth 2: secondary hits vote too)"""
    blob, info = P.room(levels=levels, depth=depth)
    views = _views(rays_mod, levels)
    for env in ENVS:
        scn = _scene(qr, blob, dict(info["env"], **env), ray_queries=True)
        try:
            _check_views(scn, oracle, blob, views, depth, f"levels {levels} depth {depth} {env}")
        finally:
            scn.close()


@pytest.mark.gpu
def test_gpu_four_cameras_at_an_odd_size(qr, oracle, rays_mod):
    """67 x 45: footprints cut by the frame's edge, lanes outside the frame next to voting lanes"""
    blob, info = P.room(levels=4, depth=2)
    views = [(l, v, 67, 45) for l, v in P.room_views(rays_mod, blob, 67, 45)]
    for env in ENVS:
        scn = _scene(qr, blob, dict(info["env"], **env), ray_queries=True)
        try:
            _check_views(scn, oracle, blob, views, 2, f"67x45 {env}")
        finally:
            scn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("levels", GPU_LEVELS)
def test_gpu_render_frames_ids_counts(qr, oracle, levels):
    import torch
    for depth in ((0, 2) if levels == 4 else (0,)):
        blob, info = P.room(levels=levels, depth=depth)
        ref, ref_ids, _ = oracle.render(blob, threads=16, want_ids=True)
        _, _, ref_cnt = oracle.render(blob, threads=16, deferred=True)
        for env in ENVS:
            scn = _scene(qr, blob, dict(info["env"], **env))
            frame = scn.new_frame(); ids = torch.full_like(frame, -2)
            scn.render(frame, ids=ids)
            _, c = scn.render_count()
            acc = torch.zeros_like(frame)
            half = (scn.height // 2) & ~7
            for r0, r1 in ((0, half), (half, scn.height)):
                scn.set_rows(r0, r1)
                scn.render(acc)
            torch.cuda.synchronize()
            out, got_ids, cnt, acc = frame.cpu().numpy().view(np.uint32), ids.cpu().numpy(), c.as_dict(), acc.cpu().numpy().view(np.uint32)
            scn.close()
            where = f"levels {levels} depth {depth} {env}"
            assert int((out != ref).sum()) == 0, f"{where}: {int((out != ref).sum())} pixels differ from the oracle"
            assert (got_ids == ref_ids).all(), f"{where}: hit ids"
            assert cnt == {k: ref_cnt[k] for k in cnt}, f"{where}: ray counts"
            assert (acc == out).all(), f"{where}: row ranges do not compose"


@pytest.mark.gpu
def test_gpu_views_mean(qr, oracle, rays_mod):
    """the mean instance over the four cameras: the composition of tests/test_views_mean.py (_truth) on the oracle's colours"""
    import torch
    blob, info = P.room(levels=4, depth=2)
    views = [v for _, v in P.room_views(rays_mod, blob, W, H)]
    cols = [rays_mod.reduce_colors(np.stack([oracle.trace_rays(blob, rays_mod.view_rays(v, W, H, blob), "shade", threads=16)[0]]), blob) for v in views]
    want_f, want_s = rays_mod.mean_of_views(cols, blob, W, H, 1.0 / len(views))
    for env in ENVS:
        scn = _scene(qr, blob, dict(info["env"], **env), ray_queries=True)
        vt = torch.from_numpy(np.ascontiguousarray(np.stack(views), dtype=np.float32)).to(f"cuda:{scn.device}")
        f, s = scn.render_views_mean(vt, W, H, scale=1.0 / len(views))
        torch.cuda.synchronize()
        f, s = f.cpu().numpy().view(np.uint32), s.cpu().numpy()
        scn.close()
        assert (s.view(np.uint32) == np.ascontiguousarray(want_s, dtype=np.float32).view(np.uint32)).all(), f"{env}: the sum differs"
        assert (f == want_f).all(), f"{env}: the frame differs"


def _shade(scn, rays, coherent=False):
    import torch
    rgb, ids = scn.shade(torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float32)).to(f"cuda:{scn.device}"), coherent=coherent, ids=True)
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), ids.cpu().numpy()


def _caller_rays(rays_mod, helper, levels):
    """the constructed views' rays as caller rays, every fifth ray of the four cameras' frames, the last wave partial"""
    rays = _waves(rays_mod, helper, levels)[0]
    n_cam = 4 * W * H
    return np.concatenate([rays[:-n_cam], rays[-n_cam::5]])[:-13]


@pytest.mark.gpu
@pytest.mark.parametrize("levels, depth", GPU_CASES)
def test_gpu_shade_constructed_rays(qr, oracle, rays_mod, helper, levels, depth):
    """the per-lane arm on the same hits: level 0 with the same comps, org, inv and clamps; colours and ids; a ray's colour does
    not depend on its wave (reversed and shuffled order)"""
    blob, info = P.room(levels=levels, depth=depth)
    rays = _caller_rays(rays_mod, helper, levels)
    assert len(rays) % 64 != 0
    want, want_ids = oracle.trace_rays(blob, rays, "shade", threads=16)
    perm = np.random.default_rng(35).permutation(len(rays))
    for env in ENVS:
        scn = _scene(qr, blob, dict(info["env"], **env), ray_queries=True)
        try:
            for coherent in (False, True):
                rgb, ids = _shade(scn, rays, coherent)
                bad = (rgb.view(np.uint32) != want.view(np.uint32)).any(axis=1)
                assert not bad.any(), f"levels {levels} depth {depth} {env} coherent={coherent}: {int(bad.sum())} of {len(rays)} colours differ, first ray {int(np.nonzero(bad)[0][0])}"
                assert (ids == want_ids).all()
            if not env:
                for order in (np.arange(len(rays))[::-1], perm):
                    rgb2, ids2 = _shade(scn, rays[order])
                    assert (rgb2.view(np.uint32) == rgb[order].view(np.uint32)).all() and (ids2 == ids[order]).all(), "a ray's colour depends on its wave"
        finally:
            scn.close()


@pytest.mark.gpu
def test_gpu_hit_gather_on_constructed_hits(qr, oracle, rays_mod, helper):
    """fans from 1 024 of the constructed hits with the 16-direction table and the truth of tests/test_gather_fans.py"""
    import torch
    from test_gather_fans import EPS, REACH, _same, _table, _truth
    blob, info = P.room(levels=4, depth=0)
    rays = _caller_rays(rays_mod, helper, 4)
    hits = helper(blob, rays[np.linspace(0, len(rays) - 1, 1024).astype(int)])
    dirs = _table(rays_mod)
    scn = _scene(qr, blob, info["env"], ray_queries=True)
    try:
        for flip, cosine in ((False, False), (False, True)):
            want = _truth(oracle, rays_mod, blob, hits, dirs, EPS, REACH, flip, cosine)
            dev = f"cuda:{scn.device}"
            g, c = scn.hit_gather(torch.from_numpy(hits).to(dev), torch.from_numpy(dirs).to(dev), EPS, REACH, flip=flip, cosine=cosine)
            torch.cuda.synchronize()
            _same(f"room flip={flip} cosine={cosine}", g, c, *want)
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_view_gather(qr, oracle, rays_mod, helper):
    """the view gather runs the scene's instance, the packet one: the fan rays' hits on the planes vote.  The four cameras at
    67 x 45 in one launch, with the pyramids, without and through the per-lane instance; _check_view_gather of tests/test_gather_fans.py"""
    from test_gather_fans import _check_view_gather, _table
    blob, info = P.room(levels=4, depth=0)
    views = [v for _, v in P.room_views(rays_mod, blob, 67, 45)]
    for env in ENVS:
        scn = _scene(qr, blob, dict(info["env"], **env), ray_queries=True)
        try:
            _check_view_gather(scn, oracle, rays_mod, helper, blob, f"room {env}", views, 67, 45, _table(rays_mod), combos=[(False, True), (True, False)])
        finally:
            scn.close()


# the depth-0 views, one render and the shaded rays once more through the guarded diagnostic build (make guard): the library is chosen when
# the package is imported, hence the child process: this file run as a script

def _guard_child():
    from qr_loader import load_package
    qr = load_package()
    assert qr.LIB_PATH == GUARD_LIB, qr.LIB_PATH
    import qr_oracle
    rays_mod, helper = _rays_mod(), _helper()
    blob, info = P.room(levels=4, depth=0)
    scn = _scene(qr, blob, info["env"], ray_queries=True)
    _check_views(scn, qr_oracle, blob, _views(rays_mod, 4), 0, "guard")
    import torch
    ref, ref_ids, _ = qr_oracle.render(blob, threads=16, want_ids=True)
    frm = _scene(qr, blob, info["env"])                             # the frame's own kernel: tile schedule, pixel_of
    frame = frm.new_frame(); fids = torch.full_like(frame, -2)
    frm.render(frame, ids=fids)
    torch.cuda.synchronize()
    out, got_ids = frame.cpu().numpy().view(np.uint32), fids.cpu().numpy()
    frm.close()
    assert (out == ref).all() and (got_ids == ref_ids).all(), "guard: render of the room"
    rays = _caller_rays(rays_mod, helper, 4)
    want, want_ids = qr_oracle.trace_rays(blob, rays, "shade", threads=16)
    rgb, ids = _shade(scn, rays)
    assert (rgb.view(np.uint32) == want.view(np.uint32)).all() and (ids == want_ids).all()
    scn.close()
    print("room guard_ok 1", flush=True)
    return 0


@pytest.mark.gpu
def test_gpu_guarded_build_gives_the_same_room():
    assert os.path.exists(GUARD_LIB), "libqrhip_guard.so is missing: build() makes it (make -C quadray-engine_amd/csrc guard)"
    env = dict(os.environ, QR_LIB=GUARD_LIB)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-child"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.count("guard_ok 1") == 1 and "QR_GUARD" not in out.stderr, out.stdout + out.stderr[-3000:]


if __name__ == "__main__":
    sys.exit(_guard_child() if "--guard-child" in sys.argv else 2)
