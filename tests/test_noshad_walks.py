"""The large-scene shadow walks on surfaces that cast no shadow (tests/_noshad.py; csrc/qr_builder.cpp compile_list(head,
as_shadow) leaves QR_OPF_NOSHAD cells out of the programs CLight::shadow points to, QR_SHADOWLESS=0 keeps them).

tests/test_own_surface_roots.py holds that on fixtures of at most 240 objects; no large scene of the tree has a surface that
casts no shadow (synth.py and _crowd.py write plain, metal and glass, and glass refracts: it casts).  Here every third member of
the crowds and of the synthetic scene is plainly transparent and every third casts on its outer side only, so that the per-lane
walks (walk_div, walk_pool with its length word and hand-over), the shadow lists by hit position and the batched shadow rounds
of incoherent hits meet a shadow program with cells left out, and a QR_OPF_SIDESHAD cell.

CPU: the patched scenes send the shadow rays the tests are about (counted with the oracle), the shadow program of the long
hierarchy changes its kind, an independent reader of the dumped image finds every shadow program to be the snapshot's chain
without its non-casters, a program of shadow rays alone gets no uniform grid, the image under QR_SHADOWLESS=0 is what it was
before that change, and the difference between the raw and the built lists of the patched crowds is pinned (_crowd.py's text).
GPU: frames, hit ids and ray counts, Scene.shade of incoherent rays and render_views equal the oracle's bit for bit with the
setting on and off; the guarded build renders the same frames and reports no bad cell offset.
"""
import hashlib
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import _crowd as C
import _noshad as N
import _rayq
import _rayset as RS
from conftest import ROOT

OFF = {"QR_SHADOWLESS": "0"}
LOW = {"QR_DDA": "64", "QR_GRID": "64"}


@pytest.fixture(scope="module")
def rays_mod():
    from qr_loader import load_package
    load_package()
    return importlib.import_module("quadray_engine_amd.rays")


def _image(qr, name, tmp_path, e=None, flags=0):
    return N.dump_image(qr, N.scene_blob(name), os.path.join(str(tmp_path), "noshad_image.bin"), e, flags)


# ---------------------------------------------------------------------------------------------------------------- CPU

# scene -> (shadow rays; the four conditions as the oracle counted them when the test was written: only non-casters in the way,
# nearest hit a non-caster yet occluded, nearest hit on a one-sided surface's non-casting side, ... casting side)
COVERAGE = {
    "mid_own": (193048, (43542, 20701, 20429, 20985)),
    "hier_raw": (25096, (4132, 655, 1357, 1087)),
    "dense_built": (43960, (9692, 7378, 5636, 6249)),
    "open_raw": (14320, (2109, 587, 802, 722)),
}


@pytest.mark.parametrize("name", sorted(COVERAGE))
def test_patched_scenes_send_the_shadow_rays(qr, oracle, rays_mod, name, capsys):
    """camera rays of sample 0, a shadow ray from every hit point to every light (tmin 1e-3, tmax 1): each condition is met by
    at least half as many rays as when the table was measured (a floor for the scene's content, the oracle alone decides it),
    and the patch changes at least 5 % of the oracle's frame"""
    blob = N.scene_blob(name)
    casts = _rayq.casts(blob)
    cam = rays_mod.camera_rays(blob, sample=0)
    t, ids = oracle.trace_rays(blob, cam, "trace", threads=16)
    hit = ids >= 0
    p = (cam[hit, 0:3] + cam[hit, 4:7] * t[hit, None]).astype(np.float32)
    rows = []
    for lp in N.lights(blob)[:, 1:4]:
        q = np.zeros((len(p), 8), dtype=np.float32)
        q[:, 0:3], q[:, 3], q[:, 4:7], q[:, 7] = p, 1e-3, lp - p, 1.0
        rows.append(q)
    sh = np.concatenate(rows)
    _, near = oracle.trace_rays(blob, sh, "trace", threads=16)
    occ = oracle.trace_rays(blob, sh, "occluded", threads=16)
    h = near >= 0
    srf, side = near >> 1, near & 1
    near_casts = np.zeros(len(sh), dtype=bool)
    near_casts[h] = casts[srf[h], side[h]]
    one_sided = np.zeros(len(sh), dtype=bool)
    one_sided[h] = casts[srf[h], 0] != casts[srf[h], 1]
    got = (int((h & ~occ).sum()), int((h & ~near_casts & occ).sum()), int((one_sided & ~near_casts).sum()),
           int((one_sided & near_casts).sum()))
    frame, _, _ = oracle.render(blob, threads=16)
    base = N.base_blob(name)
    plain, _, _ = oracle.render(bytes(qr.build_lists(base)) if name.endswith("_built") else base, threads=16)
    changed = float((frame != plain).mean())
    with capsys.disabled():
        print(f"\n{name}: {len(sh)} shadow rays, conditions {got}, {100 * changed:.1f} % of the frame changed by the patch")
    n_rays, want = COVERAGE[name]
    assert len(sh) >= n_rays // 2
    for g, w in zip(got, want):
        assert 2 * g >= w, (got, want)
    assert changed >= 0.05


def _f(st):
    return dict(lists=st.n_lists, cells=st.n_cells, dropped=st.n_dropped, grids=st.n_grids, dda=st.n_dda, bytes=st.bytes)


@pytest.mark.parametrize("name", N.SCENES)
def test_program_stats_with_the_setting_on_and_off(qr, name, capsys):
    blob = N.scene_blob(name)
    with N.env({}):
        on = qr.program_stats(blob)
    with N.env(OFF):
        off = qr.program_stats(blob)
    with capsys.disabled():
        print(f"\n{name}: on {_f(on)} off {_f(off)}")
    assert on.n_dropped > off.n_dropped
    assert on.n_grids == off.n_grids
    if name == "hier_raw":
        assert (on.n_lists, on.n_cells, on.n_dropped) == (2, 430, 74) and (off.n_lists, off.n_cells, off.n_dropped) == (1, 252, 0)
    if name == "flat_lights":
        assert (on.n_lists, on.n_cells, on.n_dropped) == (2, 365, 77) and (off.n_lists, off.n_cells, off.n_dropped) == (1, 221, 0)
    if name == "dense_built":
        assert on.n_grids >= 1, "the ground plane's shadow grids at default thresholds"


def test_shadow_program_of_the_long_hierarchy_changes_its_kind(qr, tmp_path):
    """HIER with raw lists: the full program is a long hierarchy (the ground plane's side lists: DIV | LONG | WORLD); its shadow
    program, 178 cells under QR_LONG_CELLS = 192, is not: shadow rays take another branch of traverse than before"""
    blob = N.scene_blob("hier_raw")
    ground = int(_rayq.real_surfaces(blob)[0])
    _, img = _image(qr, "hier_raw", tmp_path)
    im = N.ShadowImage(blob, img)
    words = im.shadow_words(ground, 0)
    assert len(words) == len(N.lights(blob)) and len(set(words)) == 1
    assert words[0] & 31 == N.LISTF_DIV | N.LISTF_WORLD
    assert len(im.program(words[0])) == 147                     # 221 solver surfaces, 74 of them plainly transparent
    for side in (0, 1):
        assert im.side_list_word(ground, side) & 31 == N.LISTF_DIV | N.LISTF_LONG | N.LISTF_WORLD
    _, img = _image(qr, "hier_raw", tmp_path, OFF)
    im = N.ShadowImage(blob, img)
    assert set(im.shadow_words(ground, 0)) == {im.side_list_word(ground, 0)}


READER_CASES = [(n, {}) for n in N.SCENES] + [("hier_built", LOW)]


@pytest.mark.parametrize("name,e", READER_CASES, ids=[n + ("_low" if e else "") for n, e in READER_CASES])
def test_image_reader_finds_the_chains_without_their_non_casters(qr, name, e, tmp_path, capsys):
    """every CLight::shadow of every real surface: a list program holds the solver surfaces of the snapshot's shadow chain that
    cast on some side, in chain order (all of them under QR_SHADOWLESS=0); a CGrid's cells hold subsequences of the chain;
    every array's end and hand-over offset lie on cell boundaries inside it, arrays nest, the length word is the program's"""
    blob = N.scene_blob(name)
    st, img = _image(qr, name, tmp_path, e)
    on = N.ShadowImage(blob, img).check(shadowless=True)
    _, img = _image(qr, name, tmp_path, dict(e, **OFF))
    off = N.ShadowImage(blob, img).check(shadowless=False)
    with capsys.disabled():
        print(f"\n{name} {e}: {on}; QR_SHADOWLESS=0 {off}")
    assert on["refs"] == off["refs"] > 0 and on["left_out"] > 0 and off["left_out"] == 0
    assert on["grids"] == off["grids"] == st.n_grids
    if e or name in ("dense_built", "mid_own", "mid_built"):
        assert on["grids"] >= 1 and on["grid_lists"] > 0


def test_image_reader_has_teeth(qr, tmp_path):
    """an image that kept the non-casters fails the reader when it is told they were left out, and the reverse"""
    for name in ("hier_raw", "dense_built"):
        blob = N.scene_blob(name)
        _, img = _image(qr, name, tmp_path, OFF)
        with pytest.raises(N.ImageError, match="solver cells"):
            N.ShadowImage(blob, img).check(shadowless=True)
        _, img = _image(qr, name, tmp_path)
        with pytest.raises(N.ImageError, match="solver cells"):
            N.ShadowImage(blob, img).check(shadowless=False)
    # a hand-over offset or an array end moved by one cell, a length word off by one cell
    blob = N.scene_blob("hier_raw")
    _, img = _image(qr, "hier_raw", tmp_path)
    im = N.ShadowImage(blob, img)
    word = im.shadow_words(int(_rayq.real_surfaces(blob)[0]))[0]
    off = word & ~31
    bv = next(p for p in range(off, off + 32 * 64, 32) if im.word(p) & 31 == N.OPT_BV)
    for at, why in ((bv + 8, "array end"), (off - 4, "length word")):
        bad = img.copy()
        bad[at // 4] += 32
        with pytest.raises(N.ImageError, match=why):
            N.ShadowImage(blob, bad).program(word)


def test_program_of_shadow_rays_alone_gets_no_uniform_grid(qr):
    """traverse enters walk_dda only for nearest-hit rays: the shadow program with cells left out carries no CDda"""
    blob = N.scene_blob("hier_raw")
    with N.env({"QR_DDA": "64"}):
        on = qr.program_stats(blob)
    with N.env(dict(OFF, QR_DDA="64")):
        off = qr.program_stats(blob)
    assert on.n_lists == 2 and off.n_lists == 1
    assert on.n_dda == off.n_dda == 1


# sha1 of the image under QR_SHADOWLESS=0 at default thresholds, recorded with the library of the commit before the shadow
# programs lost their uniform grids (profiles/r26_noshad_walks.txt)
IMAGE_SHA1 = {
    "hier_raw": "5a84692f77b145388c121b6388609660a44be140",
    "hier_built": "3f464509f3c14e15316223bc5dcea706df6e4357",
    "dense_built": "bb319b06ce5c5b105624cbfedde4a216ab91c245",
    "open_raw": "ba923738c06776829b41e124a89593a998e4fa88",
    "flat_lights": "4a758e7a8041e0c0c640db660d2bf6c19e3e38c6",
    "mid_own": "edc9cf8c60bfc830f0b273e8cd05d17d2a9fe14f",
    "mid_built": "567ab6a7937908a5e13e65afa15aa0922268db3f",
}


@pytest.mark.parametrize("name", N.SCENES)
def test_image_with_the_setting_off_is_what_it_was(qr, name, tmp_path):
    _, img = _image(qr, name, tmp_path, OFF)
    assert hashlib.sha1(img.tobytes()).hexdigest() == IMAGE_SHA1[name]


# --- the list finding (_crowd.py's module text): pixels of the oracle's frame that differ between a patched crowd
# with the generator's lists (the global list is every shadow list) and with the lists the product's pass builds (the engine's
# placement per side, which takes every wall for a caster)
LIST_PIXELS = {"hier": 8, "dense": 75, "open": 1, "mid": 0}
SINGLES = {250: (0, 1), 271: (2, 2), 310: (30, 31)}             # surface of the DENSE crowd -> pixels at depth 0, at its own depth


def _raw(name):
    if name == "mid":
        from test_synth import MID
        return N.patched(C.synth().make_scene(shadow_lists=False, **MID))
    return N.patched(C.make_crowd(**{"hier": C.HIER, "dense": C.DENSE, "open": C.OPEN}[name]))


@pytest.mark.parametrize("name", sorted(LIST_PIXELS))
def test_list_finding_patched_crowds(qr, oracle, name):
    raw = _raw(name)
    built = bytes(qr.build_lists(raw))
    a, ia, _ = oracle.render(raw, threads=16, want_ids=True)
    b, ib, _ = oracle.render(built, threads=16, want_ids=True)
    assert int((a != b).sum()) == LIST_PIXELS[name]
    assert (ia == ib).all(), "first hits do not depend on the lists"
    # the generator and the product's pass enter the same lights on the same sides of every surface
    (sr, _), (sb, _), Er, Eb = _rayq.surfaces(raw), _rayq.surfaces(built), N.elems(raw), N.elems(built)
    for i in _rayq.real_surfaces(raw):
        for k in (N.S_LST, N.S_LST + 2):
            assert [int(Er[e, 0]) for e in N.chain(Er, int(sr[i, k]))] == [int(Eb[e, 0]) for e in N.chain(Eb, int(sb[i, k]))], (i, k)


def _one_surface(base, i, fn):
    s, _ = _rayq.surfaces(base)
    for k in (0, 1):
        s[i, N.S_PROPS + k] = fn(int(s[i, N.S_PROPS + k]))
    return N._with_surfaces(base, s)


@pytest.mark.parametrize("i", sorted(SINGLES))
def test_list_finding_single_surfaces(qr, oracle, i):
    """one open shape of the DENSE crowd made plainly transparent: the light lists of both sides are the same in the generator's
    and in the built snapshot (synth._sides and qr_sides.cpp clip_side agree); the built shadow lists hold what the engine places
    on that side, a few of the 401 -- without what stands behind the shape's own wall, which a wall that casts no shadow no
    longer hides.  With the global list as this surface's shadow lists the built snapshot gives the generator's frame; so does a
    surface that refracts, which casts."""
    base = C.make_crowd(**C.DENSE)
    glist = int(_rayq.frame_words(base)[0][38])
    raw = _one_surface(base, i, lambda p: (p | N.P_TRANSP) & ~(N.P_REFRACT | N.P_OPAQUE))
    built = bytes(qr.build_lists(raw))
    for depth, want in zip((0, -1), SINGLES[i]):
        a, _, _ = oracle.render(raw, depth=depth, threads=16)
        b, _, _ = oracle.render(built, depth=depth, threads=16)
        assert int((a != b).sum()) == want, depth
    sr, _ = _rayq.surfaces(raw)
    sb, _ = _rayq.surfaces(built)
    Er, Eb = N.elems(raw), N.elems(built)
    E2 = Eb.copy()
    for side in (0, 1):
        mine, theirs = N.chain(Eb, int(sb[i, N.S_LST + 2 * side])), N.chain(Er, int(sr[i, N.S_LST + 2 * side]))
        assert [int(Eb[e, 0]) for e in mine] == [int(Er[e, 0]) for e in theirs], "light lists"
        assert all(int(Er[e, 1]) == glist for e in theirs)
        for e in mine:
            assert len(N.chain(Eb, int(Eb[e, 1]))) < 32 < len(N.chain(Eb, glist))
            E2[e, 1] = glist
    if i == 310:
        assert [int(Eb[e, 0]) for e in N.chain(Eb, int(sb[i, N.S_LST + 2]))] == [0, 1], "two of the four lights reach its inner side"
    bb = bytearray(built)
    at = _rayq._hdr(bb)[14]
    bb[at:at + E2.nbytes] = E2.tobytes()
    a, _, _ = oracle.render(raw, threads=16)
    c, _, _ = oracle.render(bytes(bb), threads=16)
    assert int((a != c).sum()) == 0
    glass = _one_surface(base, i, lambda p: (p | N.P_TRANSP | N.P_REFRACT) & ~N.P_OPAQUE)
    a, _, _ = oracle.render(glass, threads=16)
    b, _, _ = oracle.render(bytes(qr.build_lists(glass)), threads=16)
    assert int((a != b).sum()) == 0


def test_light_bodies_and_patch_rule(oracle):
    """the rule as _noshad.py states it: the ground plane stays, every third member casts nothing, every third on its outer side
    only; the light bodies of the flat HIER crowd are surfaces 3, 12, 19 and 26 and change the oracle's frame"""
    flat = N.patched(C.make_crowd(**dict(C.HIER, hierarchy=False)))
    casts = _rayq.casts(flat)
    real = _rayq.real_surfaces(flat)
    assert casts[real[0]].all()
    m = casts[real[1:]]
    assert not m[0::3].any() and m[1::3, 0].all() and not m[1::3, 1].any() and m[2::3].all()
    lit, which = N.light_bodies(flat)
    assert which == [3, 12, 19, 26]
    _, f = _rayq.surfaces(lit)
    assert (f[which, 0:3] == N.lights(lit)[:, 1:4]).all() and not _rayq.casts(lit)[which].any()
    a, _, _ = oracle.render(flat, threads=16)
    b, _, _ = oracle.render(lit, threads=16)
    assert int((a != b).sum()) == 89
    with pytest.raises(AssertionError):
        N.light_bodies(N.scene_blob("hier_raw"))


# ---------------------------------------------------------------------------------------------------------------- GPU

# case -> (scene, environment at upload, GPU tile binning)
FRAME_CASES = {
    "hier_raw": ("hier_raw", {}, False),
    "hier_raw_div1": ("hier_raw", {"QR_DIV": "1"}, False),
    "hier_built": ("hier_built", {}, False),
    "hier_built_low": ("hier_built", LOW, False),
    "dense_built": ("dense_built", {}, False),          # not under QR_DDA=64: a 55 MB image
    "open_raw": ("open_raw", {}, False),
    "flat_lights": ("flat_lights", {}, False),
    "mid_own": ("mid_own", {}, False),
    "mid_built_rebin": ("mid_built", {}, True),
}
_TRUTH = {}
_GPU_HASH = {}


def _truth(oracle, name):
    if name not in _TRUTH:
        blob = N.scene_blob(name)
        frame, ids, _ = oracle.render(blob, threads=16, want_ids=True)
        _, _, counts = oracle.render(blob, threads=16, deferred=True)
        _TRUTH[name] = (blob, frame, ids, counts)
    return _TRUTH[name]


def _render(qr, blob, e, rebin):
    import torch
    with N.env(e):
        scn = qr.Scene(blob, rebin_tiles=rebin)
    frame = scn.new_frame(); ids = torch.full_like(frame, -2)
    scn.render(frame, ids=ids)
    _, c = scn.render_count()
    torch.cuda.synchronize()
    out = frame.cpu().numpy().view(np.uint32), ids.cpu().numpy(), c.as_dict()
    scn.close()
    return out


def _gpu_frames(qr, oracle, case):
    scene, e, rebin = FRAME_CASES[case]
    blob, o_frame, o_ids, o_counts = _truth(oracle, scene)
    frames = []
    for se in ({}, OFF):
        out, ids, cnt = _render(qr, blob, dict(e, **se), rebin)
        what = f"{case} {se}"
        assert int((out != o_frame).sum()) == 0, f"{what}: {int((out != o_frame).sum())} pixels differ"
        assert (ids == o_ids).all(), f"{what}: hit ids"
        assert cnt == {k: o_counts[k] for k in cnt}, f"{what}: ray counts {cnt}"
        frames.append(out)
    assert (frames[0] == frames[1]).all()
    _GPU_HASH[case] = "%016x" % qr.frame_hash(frames[0])
    return _GPU_HASH[case]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(FRAME_CASES))
def test_gpu_frames(qr, oracle, case):
    """frame, hit ids and ray counts equal the oracle's bit for bit, with the setting on and under QR_SHADOWLESS=0"""
    _gpu_frames(qr, oracle, case)


# scene of the ray API -> (snapshot, environment at upload)
def _ray_scene(name):
    if name == "noshad_hier":
        return N.scene_blob("hier_raw"), {}
    key = "noshad_open_flat"
    if key not in N._BLOBS:
        N._BLOBS[key] = N.patched(C.make_crowd(**dict(C.OPEN, hierarchy=False)))
    return N._BLOBS[key], {"QR_DDA": "64"}


def _gpu(scn, rays_np, call, **kw):
    import torch
    r = torch.from_numpy(np.ascontiguousarray(rays_np, dtype=np.float32)).to(f"cuda:{scn.device}")
    out = getattr(scn, call)(r, **kw)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out) if isinstance(out, tuple) else out.cpu().numpy()


def _same_bits(what, rays, got, want):
    g = np.ascontiguousarray(got).reshape(len(rays), -1).view(np.uint32)
    w = np.ascontiguousarray(want).reshape(len(rays), -1).view(np.uint32)
    bad = (g != w).any(axis=1)
    first = "; ".join(f"ray {int(i)} {rays[i].tolist()} got {got[i]} want {want[i]}" for i in np.nonzero(bad)[0][:3])
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(rays)} rays differ: {first}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["noshad_hier", "noshad_open_flat"])
def test_gpu_shade_of_incoherent_rays(qr, oracle, name, tmp_path):
    """Scene.shade of the grid, probe and mixed families (tests/_rayset.py): rgb as bits and ids equal oracle.trace_rays at the
    scene's depth and at depth 0, with the setting on and off -- the batched (hit, light) shadow rounds of qr_shade.hpp"""
    blob, e = _ray_scene(name)
    _, img = N.dump_image(qr, blob, os.path.join(str(tmp_path), "noshad_query.bin"), e, qr.UPLOAD_RAY_QUERIES)
    g, reach = RS.dda_grid(int(img[55]), img), RS.reach_of(img)
    assert (g is not None) == bool(e)
    depth = int(_rayq.frame_words(blob)[0][29])
    fams = {f: RS.family(blob, name, f, oracle, g, reach) for f in ("grid", "probe", "mixed")}
    want = {(f, d): oracle.trace_rays(blob, r, "shade", depth=d, threads=16) for f, r in fams.items() if len(r) for d in (0, depth)}
    assert len(fams["probe"]) > 64 and len(fams["mixed"]) > 1000 and (len(fams["grid"]) > 0) == bool(e)
    for se in ({}, OFF):
        with N.env(dict(e, **se)):
            scn = qr.Scene(blob, ray_queries=True)
        for (f, d), (rgb_w, ids_w) in want.items():
            scn.set_depth(d)
            rgb, ids = _gpu(scn, fams[f], "shade", ids=True)
            _same_bits(f"{name} {se} {f} depth {d}: ids", fams[f], ids, ids_w)
            _same_bits(f"{name} {se} {f} depth {d}: rgb", fams[f], rgb, rgb_w)
        scn.close()


@pytest.mark.gpu
def test_gpu_render_views(qr, oracle, rays_mod):
    """four seeded cameras among the members of the patched HIER crowd at 64 x 64, one launch: frames and ids equal the oracle's
    frames of the rewritten snapshot, with the setting on and off"""
    import torch
    from test_render_views import _view_snapshot
    blob = N.scene_blob("hier_raw")
    views = [rays_mod.view_of(c) for c in _rayq.random_cameras(blob, seed=26, n=4, size=64)]
    want = [oracle.render(_view_snapshot(blob, v, 64, 64), threads=16, want_ids=True)[:2] for v in views]
    assert sum(int((i >= 0).sum()) for _, i in want) > 0.05 * 4 * 64 * 64
    for se in ({}, OFF):
        with N.env(se):
            scn = qr.Scene(blob, ray_queries=True)
        v = torch.from_numpy(np.ascontiguousarray(np.stack(views), dtype=np.float32)).to(f"cuda:{scn.device}")
        f, ids = scn.render_views(v, 64, 64, ids=True)
        torch.cuda.synchronize()
        f, ids = f.cpu().numpy().view(np.uint32), ids.cpu().numpy()
        scn.close()
        for j, (rf, ri) in enumerate(want):
            assert (f[j] == rf).all(), f"{se} view {j}: {int((f[j] != rf).sum())} pixels differ"
            assert (ids[j] == ri).all(), f"{se} view {j}: ids"


@pytest.mark.gpu
def test_gpu_guarded_build_renders_the_same_frames(qr, oracle):
    """the QR_GUARD build checks every cell offset of the per-lane walks before it is loaded: a wrong length word or hand-over
    offset in a program with cells left out shows as `bad cell offsets`.  Every case of test_gpu_frames, in a child process."""
    lib = os.path.join(ROOT, "quadray-engine_amd", "libqrhip_guard.so")
    assert os.path.exists(lib), "libqrhip_guard.so not built (make -C quadray-engine_amd/csrc guard)"
    want = {case: _GPU_HASH.get(case) or _gpu_frames(qr, oracle, case) for case in FRAME_CASES}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_noshad_guard.py")] + list(FRAME_CASES), capture_output=True,
                         text=True, timeout=300, env=dict(os.environ, QR_LIB=lib))
    assert out.returncode == 0, out.stderr[-2000:]
    got = dict(l.split() for l in out.stdout.splitlines() if len(l.split()) == 2 and l.split()[0] in FRAME_CASES)
    assert got == want
    assert "bad cell offsets" not in out.stderr, out.stderr[-2000:]
