"""Temporal reprojection for animated scenes (include/qrhip.h qr_reproject_moving_async; Scene.reproject(motion=),
Temporal.step(motion=, scene=), hierarchy_motion; rays.reproject_pass(motion=), rays.move_hits).

The motion table is held to the oracle (a point moved by its row lies on the same surface of the previous snapshot), the numpy
specification to a scalar restatement of the header's text and to a case worked by hand, and the GPU to the specification:
every word of every output, two NaNs equal.  The helpers are those of tests/test_reproject.py, tests/test_hierarchy.py and
tests/test_hit_records.py."""
import ctypes
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import _tree
import test_atrous as TA
import test_hierarchy as TH
import test_hit_records as THR
import test_reproject as TR
from conftest import ROOT, load_blob
from test_atrous import SENTINEL, _bits, _dev, _host
from test_pt_views import _rays_mod
from test_reproject import ARG, ASM, F, FIELDS, GUARD_LIB, H16, QNAN, S, W16, _dyadic_view, _history, _plane, _same

IDENT = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=F)
NAN = np.array([QNAN], dtype=np.uint32).view(F)[0]
FLAGS = None                                                # qr.HIER_RESET_TILES | qr.HIER_BOUNDS, set with the package
SIZES = [(64, 64), (67, 45), (9, 130)]                      # (w, h)
SYNTH_SIZES = [(1, 1), (9, 130), (67, 45), (33, 9)]
# the animated cases of the record and GPU tests: an object array of a demo scene turned by the same step three times
ANIMATED = {"demo02_160": (8, dict(rot=(25.0, 0.0, 30.0))),            # tilt: about x and z
            "demo01_160": (33, dict(rot=(35.0, 8.0, 0.0)))}            # rot
# the seeded camera's framing per frame width: (fit, aside) -- the object's radius times `fit` spans half the frame's longer
# side, and the camera aims `aside` radii to the right of the object's centre.  The 9-pixel strip looks at the object's edge from
# further away, so that its silhouette and the background it uncovers lie inside the strip
FRAMING = {64: (1.2, 0.0), 67: (1.2, 0.0), 9: (3.5, -0.25)}
KERNELS = ("23qr_reproj_moving_kernelILi3EE", "23qr_reproj_moving_kernelILi4EE")


@pytest.fixture(scope="module")
def rays_mod():
    return _rays_mod()


def _is_identity(rows):
    return (_bits(rows) == _bits(IDENT)).all(-1)


# ------------------------------------------------------------------------------------------------- names and sizes

def test_symbols_sizes_and_header(qr, rays_mod):
    hdr = open(os.path.join(ROOT, "include", "qrhip.h")).read()
    assert "qr_reproject_moving_async" in qr.ABI_SYMBOLS and "int qr_reproject_moving_async(" in hdr
    assert hasattr(qr.lib(), "qr_reproject_moving_async") and len(qr.lib().qr_reproject_moving_async.argtypes) == 18
    assert "typedef struct qr_motion { float row[3][4]; } qr_motion;" in hdr and ctypes.sizeof(qr.Motion) == 48
    for text in ("move     only with a table.  s = id_p >> 1.  s >= n_motion: a fresh entry, coords NaN (id_p < 0 is the miss rule as before).",
                 "r0, r1, r2 = the three quads of motion[s];",
                 "pos'.k = ((rk.x * pos.x + rk.y * pos.y) + rk.z * pos.z) + rk.w",
                 "nrm'.k =  (rk.x * nrm.x + rk.y * nrm.y) + rk.z * nrm.z          (not renormalised)",
                 "project  as before with e = pos' - org",
                 "taps     as before with nrm' in the normal test and nrm' . (pos_q - pos') in the plane test; id_q == id_p unchanged",
                 "What this does NOT do", "the one documented difference"):
        assert text in hdr, text
    assert callable(qr.hierarchy_motion) and callable(rays_mod.move_hits)
    import inspect
    for fn in (qr.Scene.reproject, qr.Temporal.step, rays_mod.reproject_pass, rays_mod.Temporal.step):
        assert inspect.signature(fn).parameters["motion"].default is None
    assert inspect.signature(qr.Temporal.step).parameters["scene"].default is None


def test_kernels_in_resource_check():
    """both new instances are held to the static instance's budget plus the 12 row words by the build's own check, and the
    build's assembly, where there is one, meets it; the static pair is still a pair"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import check_kernel_resources as ck
    finally:
        sys.path.pop(0)
    for frag, vgprs in zip(KERNELS, (108, 92)):
        assert ck.LIMITS[frag] == (vgprs, 0, 0) and ck.LDS_LIMITS[frag] == 0
    assert ck.LIMITS["19qr_reproject_kernelILi3EE"][0] + 12 == 108 and ck.LIMITS["19qr_reproject_kernelILi4EE"][0] + 12 == 92
    if os.path.exists(ASM):
        mine = [k for k in ck.kernels(ASM) if "qr_reproj_moving_kernel" in k["name"]]
        assert len(mine) == 2 and not any("qr_reproject_kernel" in k["name"] for k in mine)
        for k in mine:
            frag = next(f for f in KERNELS if f in k["name"])
            assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] == 0
            assert k["vgpr_count"] <= ck.LIMITS[frag][0]


# ------------------------------------------------------------------------------------------------- the motion table

def _patch(qr, raw, table, opts, camera, node, move):
    """one animation step: (patched snapshot, the same with its lists built, the node table after it, the motion table)"""
    nxt = table.copy()
    for f, d in move.items():
        nxt[node][f] += np.asarray(d, dtype=F)
    patched = qr.hierarchy_apply(raw, nxt, opts, camera=camera, base=table, flags=qr.HIER_RESET_TILES | qr.HIER_BOUNDS)
    after = qr.hierarchy_records_after_apply(raw, nxt, opts)
    n_srf = struct.unpack_from("<I", patched, 16)[0]
    return patched, qr.build_lists(patched), after, qr.hierarchy_motion(table, after, opts, n_srf)


MOVES = {"rot": dict(rot=(0.0, 0.0, 7.0)), "pos": dict(pos=(0.3, -0.2, 0.1)), "both": dict(rot=(3.0, 0.0, 7.0), pos=(0.3, -0.2, 0.1))}
# object arrays with at least 80 hits in their scene's own frame
ORACLE_CASES = [("demo02_160", 1), ("demo02_160", 8), ("demo01_160", 33), ("demo03_160", 12), ("demo03_160", 24)]


@pytest.mark.parametrize("move", sorted(MOVES))
@pytest.mark.parametrize("base_name,node", ORACLE_CASES)
def test_motion_table_against_the_oracle(qr, oracle, rays_mod, base_name, node, move):
    """One object array of a demo scene moved, the snapshot patched and its lists rebuilt; the oracle's hits of the patched
    snapshot's camera rays are taken through their rows, and a ray traced back from 0.01 before the mapped point in the
    PREVIOUS snapshot finds the same surface at |t - 0.01| < 2e-3: on at least 99 % of the moved hits (the reference alone gave
    99.08 % at worst here: demo02_160 node 1, both; silhouettes and contact lines), and on all unmoved hits but 0.1 % (at
    most 5 of 18 978 here).  The cases include those where the array newly becomes a transform node and the snapshot grows
    by a record."""
    rm = rays_mod
    t, base = TH.load_tree(qr, base_name)
    prev = load_blob(base_name)
    _, cur, after, m = _patch(qr, prev, base, t["opts"], t["camera"], node, MOVES[move])
    n_prev, n_cur = (struct.unpack_from("<I", b, 16)[0] for b in (prev, cur))
    assert m.shape == (n_cur, 12) and m.dtype == F and n_cur in (n_prev, n_prev + 1)
    rays = rm.camera_rays(cur)
    tt, ids = oracle.trace_rays(cur, rays, "trace")
    hit = ids >= 0
    s = np.where(hit, ids >> 1, 0)
    assert not np.isnan(m[s[hit]]).any(), "every surface a ray can hit has a row"
    pos = rays[:, 0:3].astype(np.float64) + rays[:, 4:7].astype(np.float64) * tt[:, None].astype(np.float64)
    r = m[s].reshape(-1, 3, 4).astype(np.float64)
    was = (r[:, :, :3] * pos[:, None, :]).sum(-1) + r[:, :, 3]
    d = (r[:, :, :3] * rays[:, None, 4:7].astype(np.float64)).sum(-1)
    back = rays.copy()
    back[hit, 0:3], back[hit, 4:7] = (was - 0.01 * d)[hit], d[hit]
    back[:, 3], back[:, 7] = 0.0, np.finfo(F).max
    tb, ib = oracle.trace_rays(prev, back, "trace")
    good = hit & (ib >= 0) & ((ib >> 1) == s) & (np.abs(tb - F(0.01)) < 2e-3)
    moved = hit & ~_is_identity(m[s])
    print(f"{base_name} node {node} {move}: {int((good & moved).sum())} of {int(moved.sum())} moved hits, "
          f"{int((hit & ~moved & ~good).sum())} of {int((hit & ~moved).sum())} unmoved hits astray")
    assert moved.sum() >= 80
    assert (good & moved).sum() >= 0.99 * moved.sum(), (int((good & moved).sum()), int(moved.sum()))
    assert (hit & ~moved & ~good).sum() <= 0.001 * (hit & ~moved).sum(), int((hit & ~moved & ~good).sum())


def test_tree_reader_is_test_hierarchys(qr):
    """tests/_tree.py, which the GPU tool of this call loads its scene with, reads what tests/test_hierarchy.py reads"""
    for name in sorted(ANIMATED) + ["demo03_160"]:
        (ta, na), (tb, nb) = _tree.load_tree(qr, name), TH.load_tree(qr, name)
        assert ta == tb and na.dtype == nb.dtype and na.tobytes() == nb.tobytes(), name


def test_motion_table_rows(qr):
    """unmoved surfaces have the exact identity row, as bits; arrays and appended transform-node records have NaN rows; a node
    whose scaler changed has a NaN row; the table is as long as the grown snapshot; mismatched tables are refused"""
    t, base = TH.load_tree(qr, "demo02_160")
    raw = load_blob("demo02_160")
    n0 = struct.unpack_from("<I", raw, 16)[0]
    node = 1
    patched, _, after, m = _patch(qr, raw, base, t["opts"], t["camera"], node, MOVES["rot"])
    assert len(m) == n0 + 1 == struct.unpack_from("<I", patched, 16)[0], "the array became a transform node: one more record"
    assert int(after[node]["srf"]) == n0 and (_bits(m[n0]) == QNAN).all(), "the appended record names no surface"
    st0, st1 = qr.hierarchy_update(base, t["opts"]), qr.hierarchy_update(after, t["opts"])

    def world(st, i):
        tr = int(st[i]["trnode"])
        own = st[i]["mtx"].reshape(4, 4).astype(np.float64)
        return own if tr < 0 or tr == i else own @ st[tr]["mtx"].reshape(4, 4).astype(np.float64)
    named, still, turned = set(), 0, 0
    for i in range(len(after)):
        srf = int(after[i]["srf"])
        if not (0 <= after[i]["tag"] < 9 and srf >= 0):
            continue
        named.add(srf)
        if np.array_equal(world(st0, i), world(st1, i)):
            assert (_bits(m[srf]) == _bits(IDENT)).all(), i
            still += 1
        else:
            a = m[srf].reshape(3, 4)[:, :3].astype(np.float64)
            assert np.abs(a @ a.T - np.eye(3)).max() < 1e-5 and not _is_identity(m[srf]), i
            x = np.linalg.inv(world(st1, i)) @ world(st0, i)
            assert (_bits(m[srf]) == _bits(np.concatenate([x[:3, :3].T, x[3, :3, None]], axis=1).reshape(12).astype(F))).all(), i
            turned += 1
    assert still > 0 and turned > 0
    for srf in range(len(m)):
        assert (srf in named) or (_bits(m[srf]) == QNAN).all(), srf
    assert any(after[i]["tag"] == -1 and after[i]["srf"] >= 0 for i in range(len(after))), "arrays with records are among them"
    # a scaler that changed: no history
    scaled = after.copy()
    leaf = next(i for i in range(len(base)) if 0 <= base[i]["tag"] < 9 and base[i]["srf"] >= 0)
    scaled[leaf]["scl"] *= F(1.25)
    ms = qr.hierarchy_motion(after, scaled, t["opts"], len(m))
    assert (_bits(ms[int(base[leaf]["srf"])]) == QNAN).all()
    assert _is_identity(ms[[s for s in named if s != int(base[leaf]["srf"])]]).sum() > 0
    # the same table twice: identity everywhere a surface is named
    same = qr.hierarchy_motion(after, after, t["opts"], len(m))
    assert all(_is_identity(same[s]) for s in named)
    assert qr.hierarchy_motion(base, after, t["opts"], 0).shape == (0, 12)
    other = after.copy()
    other[3]["tag"] = 5 if after[3]["tag"] != 5 else 4
    parent = after.copy()
    parent[5]["parent"] = 0 if after[5]["parent"] != 0 else 1
    for a, b, n in ((base[:-1], after, len(m)), (base, other, len(m)), (base, parent, len(m)), (base, after, -1), (base, after, 2.5),
                    (base, after, True)):
        with pytest.raises(ValueError):
            qr.hierarchy_motion(a, b, t["opts"], n)


# ------------------------------------------------------------------------------------------------- the move step

def _moved_records(rec, motion):
    """the header's move step in scalar float32, pixel by pixel, written a second time: a copy of one view's records with pos
    and nrm replaced by pos' and nrm' -- NaN beyond the table, which the projection turns into a fresh entry --; misses are
    left alone (the miss rule)"""
    f = F
    out = rec.copy()
    h, w = rec.shape[:2]
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                pid = int(rec[y, x].view(np.int32)[7])
                if pid < 0:
                    continue
                s = pid >> 1
                if s >= len(motion):
                    out[y, x, 0:3], out[y, x, 4:7] = NAN, NAN
                    continue
                pos, nrm, r = rec[y, x, 0:3], rec[y, x, 4:7], motion[s].reshape(3, 4)
                for k in range(3):
                    out[y, x, k] = ((r[k, 0] * pos[0] + r[k, 1] * pos[1]) + r[k, 2] * pos[2]) + r[k, 3]
                    out[y, x, 4 + k] = (r[k, 0] * nrm[0] + r[k, 1] * nrm[1]) + r[k, 2] * nrm[2]
                assert all(type(v) is f or isinstance(v, f) for v in (out[y, x, 0], out[y, x, 4]))
    return out


def _against_scalar(rm, p, col, rec, var, prev, motion, where):
    """reproject_pass(motion=) on one view against the scalar move step followed by test_reproject's scalar pixel"""
    got = rm.reproject_pass(col, rec, var, prev, motion=motion, **p)
    moved = _moved_records(rec, motion)
    h, w, ch = col.shape
    for y in range(h):
        for x in range(w):
            e, v, xy = TR._pixel(rm, p, col, moved, var, prev, x, y)
            _same(got[0][y, x], e, f"{where} entry ({x}, {y})")
            _same(got[1][y, x], e[:ch], f"{where} colour ({x}, {y})")
            _same(got[2][y, x], v, f"{where} variance ({x}, {y})")
            _same(got[3][y, x], xy, f"{where} coords ({x}, {y})")
    return got


def _rigid(rng, angle, shift):
    """a rotation about a random axis through the origin by `angle` radians and a translation of up to `shift`: a row"""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    a = np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)
    return np.concatenate([a, rng.uniform(-shift, shift, (3, 1))], axis=1).reshape(12).astype(F)


def _about_z(angle, tx, ty):
    """the plane z = 1 stays the plane z = 1 and its normal its normal: points slide inside the previous frame"""
    c, s = np.cos(angle), np.sin(angle)
    return np.array([c, -s, 0, tx, s, c, 0, ty, 0, 0, 1, 0], dtype=F)


def _tables(seed):
    """motion tables for test_reproject's synthetic frames (ids 2 and 5: surfaces 1 and 2; misses): rows that slide the plane by
    a few pixels, a random rigid row, and rows with NaN, Inf, huge values and -0.0"""
    rng = np.random.default_rng(seed)
    slide = np.stack([_rigid(rng, 0.3, 0.2), _about_z(0.02, 3.25 * S, -1.5 * S), _about_z(-0.05, -0.75 * S, 2.0 * S), _rigid(rng, 0.1, 0.05)])
    odd = slide.copy()
    odd[1, [1, 2, 6]] = -0.0                                 # -0.0 among the zeros of the matrix
    odd[1, 3] = F(3.0e38)
    odd[2, 5] = np.inf
    nan = slide.copy()
    nan[2] = NAN
    nan[1, 7] = np.nan
    ident = np.tile(IDENT, (3, 1))
    ident[2, [1, 4, 11]] = -0.0
    return [("slide", slide), ("odd", odd), ("nan", nan), ("identity", ident), ("one row", slide[:1]), ("two rows", slide[:2])]


def _with_far_ids(rec, seed):
    """ids beyond any table among the records: surfaces 7, 2^30 - 1 and 2^30"""
    rng = np.random.default_rng(seed)
    out = rec.copy()
    ids = out.view(np.int32)[..., 7]
    for val in (15, 0x7FFFFFFE, 0x7FFFFFFF, 14):
        ids[rng.uniform(size=ids.shape) < 0.03] = val
    return out


def test_move_step_against_the_scalar_text(rays_mod):
    """reproject_pass(motion=) against a scalar restatement of the header's move step, pixel by pixel, on frames with NaN, Inf
    and -0.0 records and tables with NaN, Inf, huge and -0.0 rows; ids beyond the table, a table of one row, negative ids;
    motion=None is the call without the argument, as bits; move_hits is the same step"""
    rm = rays_mod
    w, h = 13, 11
    taken = 0
    for ch in (3, 4):
        col, rec, var, prev = TR._synthetic(w, h, 40 + ch, ch)
        rec = _with_far_ids(rec, 50 + ch)
        ids = rec.view(np.int32)[..., 7]
        assert (ids < 0).any() and (ids == 15).any() and (ids == 0x7FFFFFFF).any() and (ids == 5).any()
        for name, m in _tables(60 + ch):
            for kw in (dict(plane_max=2.0 ** -5), dict(plane_max=2.0 ** -5, demodulate=True, var_min_len=1, normal_min=-1.0, off=(0.5, -0.25))):
                p = rm.reproject_stops(**kw)
                for j in range(2):
                    pj = tuple(a[j] for a in prev)
                    taps = []
                    rm.reproject_pass(col[j], rec[j], var[j], pj, motion=m, taps=taps, **p)
                    taken += sum(int(t[0].sum()) for t in taps) if name == "slide" else 0
                    _against_scalar(rm, p, col[j], rec[j], var[j], pj, m, f"{name} ch {ch} view {j} {kw}")
            both = rm.reproject_pass(col, rec, var, prev, motion=m, plane_max=F(2.0 ** -5))
            for j in range(2):
                one = rm.reproject_pass(col[j], rec[j], var[j], tuple(a[j] for a in prev), motion=m, plane_max=F(2.0 ** -5))
                for a, b in zip(both, one):
                    _same(a[j], b, f"{name}: a view alone and in a batch")
            pos, nrm, listed = rm.move_hits(rec[0], m)
            want = _moved_records(rec[0], m)
            on = ids[0] >= 0
            _same(pos[on], want[..., 0:3][on], f"{name} move_hits pos"), _same(nrm[on], want[..., 4:7][on], f"{name} move_hits nrm")
            assert (listed == (on & ((ids[0] >> 1) < len(m)))).all() and np.isnan(pos[~listed]).all()
        first = rm.reproject_pass(col, rec, var, None, motion=_tables(1)[0][1])
        for a, b in zip(first, rm.reproject_pass(col, rec, var, None)):
            _same(a, b, "a first frame with a table is a first frame")
        for a, b in zip(rm.reproject_pass(col, rec, var, prev, motion=None, plane_max=F(2.0 ** -5)),
                        rm.reproject_pass(col, rec, var, prev, plane_max=F(2.0 ** -5))):
            assert (_bits(a) == _bits(b)).all(), "motion=None is the call without the argument"
    assert taken > 50, "the sliding rows keep history"


def test_identity_table_on_real_records(rays_mod):
    """the exact identity table against motion=None on the oracle's records of two real scenes (test_reproject's cameras A and
    B).  The header says: on finite records every word of history, colour and variance is the same, and coords are the same but
    for the sign of a zero.  Observed here: every word of all four outputs is the same, zeros included -- no -0.0 coordinate
    meets a +0.0 camera origin in these records"""
    rm = rays_mod
    for scene in TR.REAL_SCENES:
        w = h = 64
        cams, off, plane_max = TR._pair(rm, scene, w, h)
        ra, rb = TR._oracle_records(rm, scene, w, h)
        ids = rb.view(np.int32)[..., 7]
        assert np.isfinite(rb[ids >= 0][:, [0, 1, 2, 4, 5, 6]]).all()
        p = rm.reproject_stops(plane_max=plane_max, off=off, demodulate=True)
        col = np.random.default_rng(2).uniform(0.0, 1.0, (h, w, 3)).astype(F)
        h0 = rm.reproject_pass(col, ra, None, None, **p)[0]
        table = np.tile(IDENT, (int(ids.max() >> 1) + 1, 1))
        plain = rm.reproject_pass(col, rb, None, (cams[0], ra, h0), **p)
        moved = rm.reproject_pass(col, rb, None, (cams[0], ra, h0), motion=table, **p)
        assert (plain[0][..., 6] > 1).sum() > 100
        for k in range(3):
            assert (_bits(plain[k]) == _bits(moved[k])).all(), f"{scene} output {k}"
        both_nan = np.isnan(plain[3]) & np.isnan(moved[3])
        assert ((plain[3] == moved[3]) | both_nan).all(), f"{scene}: coords differ by more than the sign of a zero"
        assert ((_bits(plain[3]) == _bits(moved[3])) | both_nan).all(), f"{scene}: observed: not even a zero's sign differs"
    # the difference the header documents, made by hand: a -0.0 coordinate, a +0.0 origin, three zero products in nu
    view = _dyadic_view()
    view[4:7] = (0.0, -H16 / 2 * S, 1.0)                    # B.z = ver.x * dir.y - ver.y * dir.x = -S * 0 = -0.0
    rec = _plane()
    rec[..., 0] = -0.0
    out = [rm.reproject_pass(np.zeros((H16, W16, 3), dtype=F), rec, None, (view, _plane(), _history(H16, W16, 3)), motion=m, plane_max=F(1.0))
           for m in (None, np.tile(IDENT, (2, 1)))]
    for k in range(3):
        assert (_bits(out[0][k]) == _bits(out[1][k])).all()
    minus = _bits(out[0][3][..., 0]) == 0x80000000             # the rows above the axis: e.y * B.y is -0.0 too
    assert (out[0][3] == out[1][3]).all() and minus[:H16 // 2].all() and (_bits(out[1][3][..., 0]) == 0).all()
    assert (_bits(out[0][3][..., 1]) == _bits(out[1][3][..., 1])).all()


# ------------------------------------------------------------------------------------------------- a case worked by hand

def _hand_case(ch=3, seed=9):
    """a static dyadic camera on the plane z = 1; a patch of it (surface 1, x = 2..9 in the previous frame) moved by exactly 2.25
    pixel footprints to the right, the rest (surface 2) stands still: (colour, records, prev, table)"""
    rng = np.random.default_rng(seed)
    col = rng.uniform(0.0, 1.0, (H16, W16, ch)).astype(F)
    old, cur = _plane(sid=4), _plane(sid=4)
    old.view(np.int32)[:, 2:10, 7] = 2
    cur.view(np.int32)[:, 5:12, 7] = 2                      # x - 2.25 in 2..9
    table = np.stack([np.full(12, NAN, dtype=F), IDENT.copy(), IDENT.copy()])
    table[1, 3] = F(-2.25 * S)
    return col, cur, (_dyadic_view(), old, _history(H16, W16, seed + 1, ch)), table


@pytest.mark.parametrize("ch", [3, 4])
def test_patch_moved_by_two_and_a_quarter_pixels(rays_mod, ch):
    """With the table the patch's pixels fall at exactly x - 2.25: wx = 0.75, wy = 0, the two taps of the row weigh 1/4 and 3/4,
    sum to exactly 1, and the entry is the blend written out by hand, bit for bit.  With motion=None on the same inputs every
    pixel of the patch projects onto itself and is fresh or takes the history of the material two and a quarter pixels away:
    the inputs tell the feature from its absence"""
    rm = rays_mod
    col, rec, prev, table = _hand_case(ch)
    p = rm.reproject_stops(plane_max=2.0 ** -4)
    taps = []
    hist, out, var, xy = rm.reproject_pass(col, rec, None, prev, motion=table, taps=taps, **p)
    _against_scalar(rm, p, col, rec, None, prev, table, "the hand case")
    ys, xs = np.mgrid[0:H16, 0:W16]
    patch = rec.view(np.int32)[..., 7] == 2
    assert patch.sum() == 7 * H16
    assert (xy[..., 0][patch] == (xs - F(2.25))[patch]).all() and (xy[..., 1] == ys).all() and (xy[..., 0][~patch] == xs[~patch]).all()
    assert (hist[..., 6][patch] > 1).all(), "every pixel of the patch keeps its history"
    assert [bool(t[0].reshape(H16, W16)[3, 7]) for t in taps] == [True, True, False, False]
    hq = prev[2]
    b = [F(0.25) * F(1.0), F(0.75) * F(1.0)]
    tp = [hq[3, 4], hq[3, 5]]                                # pixel (7, 3) fell at (4.75, 3)
    sw = (F(0) + b[0]) + b[1]
    assert sw == 1.0 and xy[3, 7, 0] == 4.75
    sl = (F(0) + tp[0][6] * b[0]) + tp[1][6] * b[1]
    ln = sl / sw + F(1.0)
    assert 2.0 <= ln <= 9.0 and _bits(hist[3, 7, 6]) == _bits(ln)
    a = F(1.0) / ln
    ac, am = max(a, F(0.05)), max(a, F(0.2))
    for k in range(ch):
        sc = (F(0) + tp[0][k] * b[0]) + tp[1][k] * b[1]
        assert _bits(hist[3, 7, k]) == _bits((sc / sw) * (F(1.0) - ac) + col[3, 7, k] * ac)
        assert _bits(out[3, 7, k]) == _bits(hist[3, 7, k])
    lum = (col[3, 7, 0] * F(0.2126) + col[3, 7, 1] * F(0.7152)) + col[3, 7, 2] * F(0.0722)
    s1 = (F(0) + tp[0][4] * b[0]) + tp[1][4] * b[1]
    s2 = (F(0) + tp[0][5] * b[0]) + tp[1][5] * b[1]
    assert _bits(hist[3, 7, 4]) == _bits((s1 / sw) * (F(1.0) - am) + lum * am)
    assert _bits(hist[3, 7, 5]) == _bits((s2 / sw) * (F(1.0) - am) + (lum * lum) * am)
    assert _bits(hist[3, 7, 7]) == 0 and (ch == 4 or _bits(hist[3, 7, 3]) == 0)
    v = hist[3, 7, 5] - hist[3, 7, 4] * hist[3, 7, 4]
    assert _bits(var[3, 7]) == _bits((v if 0 < v else F(0.0)) if F(4.0) <= ln else F(1.0))
    # the rest of the plane: uncovered pixels (x = 2..4 were the patch) are fresh, the others keep their own pixel's history
    still = hist[..., 6][~patch].reshape(H16, -1)
    assert (still[:, 2:5] == 1).all() and (still[:, :2] > 1).all() and (still[:, 5:] > 1).all()
    # without the table
    taps0 = []
    hist0, _, _, xy0 = rm.reproject_pass(col, rec, None, prev, taps=taps0, **p)
    assert (xy0[..., 0] == xs).all() and (xy0[..., 1] == ys).all(), "every pixel projects onto itself"
    assert (hist0[:, 10:12, 6] == 1).all(), "where the patch is new the static call starts afresh"
    wrong = patch & (hist0[..., 6] > 1)
    took = [t[0].reshape(H16, W16) for t in taps0]
    assert wrong.sum() == 5 * H16 and took[0][wrong].all() and not any(t[wrong].any() for t in took[1:])
    for k in range(ch):                                      # ... the history of the pixel itself: other material
        a0 = np.maximum(F(1.0) / hist0[..., 6], F(0.05))
        assert (_bits(hist0[..., k][wrong]) == _bits((hq[..., k] * (F(1.0) - a0) + col[..., k] * a0)[wrong])).all()
    assert not (_bits(hist0[..., :ch][patch]) == _bits(hist[..., :ch][patch])).all(-1).any(), "no pixel of the patch agrees"
    _same(hist0[~patch], hist[~patch], "the plane that stands still does not notice the table")


# ------------------------------------------------------------------------------------------------- real animated records

_FRAMES, _VIEWS, _RECORDS = {}, {}, {}


def _frames(qr, base_name, n=3):
    """the animated case of a scene: [(snapshot with its lists built, motion table from the frame before or None)] * (n + 1),
    every frame the patch of the one before (node tables carried on with hierarchy_records_after_apply)"""
    if (base_name, n) not in _FRAMES:
        node, move = ANIMATED[base_name]
        t, table = TH.load_tree(qr, base_name)
        raw = load_blob(base_name)
        out = [(raw, None)]
        for _ in range(n):
            raw, listed, table, m = _patch(qr, raw, table, t["opts"], t["camera"], node, move)
            out.append((listed, m))
        _FRAMES[base_name, n] = out
    return _FRAMES[base_name, n]


def _view(qr, rm, base_name, w, h):
    """(camera, off, plane_max): a seeded camera near the scene's own that looks at the moved object of frame 1 and holds it
    across the frame's longer side; plane_max is one pixel's footprint at the object"""
    if (base_name, w, h) not in _VIEWS:
        blob, m = _frames(qr, base_name)[1]
        own = rm.view_of(blob)
        fw, fh = TR.TPV._size(blob)
        rec = THR._helper()(blob, rm.view_rays(own, fw, fh, blob, 0))
        ids = rec.view(np.int32)[:, 7]
        moved = (ids >= 0) & ~_is_identity(m[np.where(ids >= 0, ids >> 1, 0)])
        assert moved.sum() >= 80
        at = rec[moved, 0:3].astype(np.float64)
        centre = at.mean(0)
        radius = np.linalg.norm(at - centre, axis=1).max()
        org, _, up, right = TR._frame_of(own, fw, fh)
        fit, aside = FRAMING[w]
        rng = np.random.default_rng(zlib.crc32(base_name.encode()) + w)
        eye = org + rng.uniform(-0.05, 0.05, 3) * np.linalg.norm(centre - org)
        dist = np.linalg.norm(centre - eye)
        fov = np.degrees(2 * np.arctan(fit * radius / dist * w / max(w, h)))
        v = rm.look_at(eye, centre + right * (aside * radius), up, fov, w, h)
        _VIEWS[base_name, w, h] = (v, TR._offsets(rm, blob), float(F(dist * np.linalg.norm(v[8:11]))))
    return _VIEWS[base_name, w, h]


def _records(qr, rm, base_name, w, h, n=3):
    """the oracle's hit records of every frame from the seeded camera, [n + 1, h, w, 12]"""
    if (base_name, w, h, n) not in _RECORDS:
        v = _view(qr, rm, base_name, w, h)[0]
        _RECORDS[base_name, w, h, n] = np.stack([THR._helper()(b, rm.view_rays(v, w, h, b, 0)).reshape(h, w, 12)
                                                 for b, _ in _frames(qr, base_name, n)])
    return _RECORDS[base_name, w, h, n]


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("base_name", sorted(ANIMATED))
def test_animated_records_have_work_for_every_branch(qr, rays_mod, base_name, size):
    """The oracle's hit records of three frames of a turning object (demo02 node 8 tilted by (25, 0, 30) degrees a frame, demo01
    node 33 turned by (35, 8, 0)) from a seeded camera that sees it: over the two steps, pixels of the moved surfaces keep
    history, some through fewer than four taps; some fall inside the previous frame and are disoccluded
    all the same; unmoved pixels have the static pass's entries, as bits.  With motion=None the moved surfaces keep fewer than
    a tenth as many pixels, and both counts are non-zero.  All of it is asserted at every size; the 9 x 130 strip looks at the
    object from further away and a quarter of a radius aside (FRAMING), so that the object's edge and the background it
    uncovers lie inside it.  Over both steps, kept with the table / without / through fewer than four taps / disoccluded:
    demo01 251 / 5 / 158 / 196 at 64 x 64, 294 / 2 / 180 / 232 at 67 x 45, 43 / 2 / 37 / 32 at 9 x 130;
    demo02 2360 / 12 / 646 / 7, 2560 / 20 / 555 / 41, 276 / 5 / 103 / 33.  These records are the GPU tests' inputs."""
    rm = rays_mod
    w, h = size
    v, off, plane_max = _view(qr, rm, base_name, w, h)
    recs = _records(qr, rm, base_name, w, h)
    p = rm.reproject_stops(plane_max=plane_max, off=off)
    col = np.random.default_rng(1).uniform(0.0, 1.0, (h, w, 3)).astype(F)
    hist = rm.reproject_pass(col, recs[0], None, None, **p)[0]
    kept_with = kept_without = few = disoccluded = 0
    for k in (1, 2):
        m = _frames(qr, base_name)[k][1]
        taps = []
        prev = (v, recs[k - 1], hist)
        hist, _, _, xy = rm.reproject_pass(col, recs[k], None, prev, motion=m, taps=taps, **p)
        static = rm.reproject_pass(col, recs[k], None, prev, **p)[0]
        ids = recs[k].view(np.int32)[..., 7]
        hit = ids >= 0
        moved = hit & ~_is_identity(m[np.where(hit, ids >> 1, 0)])
        assert moved.any() and (hit & ~moved).any() and not np.isnan(m[ids[hit] >> 1]).any()
        kept = hist[..., 6] > 1
        ntaps = sum(t[0].astype(np.int32) for t in taps)
        with np.errstate(invalid="ignore"):
            inside = (xy[..., 0] > -1) & (xy[..., 0] < w) & (xy[..., 1] > -1) & (xy[..., 1] < h)
        kept_with += int((moved & kept).sum())
        kept_without += int((moved & (static[..., 6] > 1)).sum())
        few += int((moved & kept & (ntaps < 4)).sum())
        disoccluded += int((moved & inside & ~kept).sum())
        assert (_bits(hist[hit & ~moved]) == _bits(static[hit & ~moved])).all(), "an unmoved pixel does not notice the table"
        assert (hit & ~moved & kept).sum() > 0
    print(f"{base_name} {w}x{h}: kept {kept_with} with the table, {kept_without} without, {few} through fewer than four taps, "
          f"{disoccluded} disoccluded")
    assert kept_with > 0 and few > 0 and disoccluded > 0, (kept_with, few, disoccluded)
    assert 0 < kept_without and 10 * kept_without < kept_with, (kept_with, kept_without)


# ------------------------------------------------------------------------------------------------- chain and refusals

def test_temporal_with_motion_is_its_chained_passes(rays_mod):
    """rays.temporal(...).step(motion=) over 4 frames of two views against reproject_pass(motion=) chained by hand"""
    rm = rays_mod
    rng = np.random.default_rng(14)
    n = 4
    cols = rng.uniform(0.0, 1.0, (n, 2, H16, W16, 4)).astype(F)
    var = rng.uniform(0.01, 0.1, (n, 2, H16, W16)).astype(F)
    shifts = [(0.0, 0.0), (0.25, 0.75), (0.5, 0.125), (-0.375, 0.25)]
    recs = [np.stack([_plane(dx=dx, dy=dy), _plane(dx=-dy, dy=dx, sid=4)]) for dx, dy in shifts]
    views = np.stack([_dyadic_view(), _dyadic_view()])
    kw = dict(plane_max=2.0 ** -4, demodulate=True, var_min_len=2)
    acc, p = rm.temporal(2, W16, H16, 4, **kw), rm.reproject_stops(**kw)
    prev = None
    for k in range(n):
        m = None if k == 0 else np.stack([np.full(12, NAN, dtype=F), _about_z(0.0, (k - 2.5) * S, 0.5 * S), _about_z(0.01 * k, 0.0, -S)])
        want = rm.reproject_pass(cols[k], recs[k], var[k], prev, motion=m, **p)
        out, v = acc.step(cols[k], recs[k], views, var[k], motion=m)
        _same(out, want[1], f"step {k} colour"), _same(v, want[2], f"step {k} variance"), _same(acc.history, want[0], f"step {k} history")
        if k:
            plain = rm.reproject_pass(cols[k], recs[k], var[k], prev, **p)
            assert (_bits(plain[0]) != _bits(want[0])).any(), "the table matters"
        prev = (views, recs[k], want[0])
    assert (acc.length > 2).any()


def test_refusals_without_a_gpu(qr, rays_mod):
    """what needs no device: the specification's ValueError for a table that is none, Scene.reproject's and Temporal.step's
    ValueError for a motion argument that is no float32 [n, 12] tensor on the scene's device, QrError for a scene on another
    device"""
    import torch
    rm = rays_mod
    col, rec, prev, table = _hand_case()
    for bad in (table.astype(np.float64), table[:, :11], table[0], table[:0], table.reshape(3, 3, 4), "table", 5):
        with pytest.raises(ValueError, match="motion must be"):
            rm.reproject_pass(col, rec, None, prev, motion=bad)
        with pytest.raises(ValueError, match="motion must be"):
            rm.move_hits(rec, bad)
    with pytest.raises(ValueError):
        rm.temporal(1, W16, H16).step(col[None], rec[None], prev[0][None], motion=table[:, :5])
    me = object.__new__(qr.Scene)
    me._h, me.device = ctypes.c_void_p(), 0
    n, h, w = 2, 5, 6
    tc, th = torch.zeros((n, h, w, 3)), torch.zeros((n, h, w, 12))
    good = torch.zeros((4, 12))
    for bad in (good, good.numpy(), good.double(), torch.zeros((4, 11)), torch.zeros((12,)), torch.zeros((0, 12)), good.t(), "m", 7):
        with pytest.raises(ValueError, match="motion must be"):
            me.reproject(tc, th, motion=bad)
    with pytest.raises(qr.QrError, match="on cuda:0"):
        me.reproject(tc, th, motion=None)
    acc = object.__new__(qr.Temporal)
    acc.scene, acc.shape, acc.channels = me, (n, h, w), 3
    elsewhere = object.__new__(qr.Scene)
    elsewhere._h, elsewhere.device = ctypes.c_void_p(), 1
    for bad in (elsewhere, "scene", 0):
        with pytest.raises(qr.QrError, match="accumulator's device"):
            acc.step(tc, th, torch.zeros((n, 16)), scene=bad)
    with pytest.raises(ValueError, match="motion must be"):
        acc.step(tc, th, torch.zeros((n, 16)), motion=good, scene=me)


# ---------------------------------------------------------------------------------------------------------------- GPU

def _call_moving(qr, rm, scn, col, rec, var, prev, motion, p, where, outs=(True, True, True), stream=None, n_motion=None):
    """one qr_reproject_moving_async call through ctypes into filled, sentinel-guarded buffers -- colour, variance and coords 4
    bytes off a 16-byte boundary, the table aligned --, compared with reproject_pass(motion=) on the same host arrays: every
    word of every output that is given, the guards intact.  motion=None: a null table and n_motion 0.  Returns the history"""
    import torch
    n, h, w, ch = col.shape
    cd, hd = _dev(scn, col), _dev(scn, rec)
    vd = None if var is None else _dev(scn, var)
    pd = [None] * 3 if prev is None else [_dev(scn, a) for a in prev]
    md = None if motion is None else _dev(scn, motion)
    assert md is None or md.data_ptr() % 16 == 0
    shapes = [(n, h, w, 8), (n, h, w, ch), (n, h, w), (n, h, w, 2)]
    bufs = [TR._buffer(scn, s, 777.0 if k == 3 else float("nan"), min(k, 1)) if k == 0 or outs[k - 1] else (None, None)
            for k, s in enumerate(shapes)]
    vp = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())
    cp = TR._params(qr, ch, p)
    st = torch.cuda.current_stream() if stream is None else stream
    rc = qr.lib().qr_reproject_moving_async(scn._h, vp(cd), vp(hd), vp(vd), vp(pd[0]), vp(pd[1]), vp(pd[2]), vp(md),
                                            (0 if motion is None else len(motion)) if n_motion is None else n_motion,
                                            n, w, h, ctypes.byref(cp), *(vp(b[1]) for b in bufs), ctypes.c_void_p(st.cuda_stream))
    assert rc == 0, f"{where}: {qr.lib().qr_last_error().decode()}"
    st.synchronize()
    want = rm.reproject_pass(col, rec, var, prev, motion=motion, **p)
    got_hist = None
    for k, (whole, body) in enumerate(bufs):
        if whole is None:
            continue
        g = _host(whole)
        size, lead = int(np.prod(shapes[k])), min(k, 1)
        assert (g[lead + size:] == SENTINEL).all() and (g[:lead] == SENTINEL).all(), f"{where}: output {k} was written outside"
        got = g[lead:lead + size].reshape(shapes[k])
        _same(got, want[k], f"{where} output {k}")
        if k == 0:
            got_hist = got
        if k == 3:
            ids = rec.view(np.int32)[..., 7]
            far = (ids < 0) if motion is None or prev is None else (ids < 0) | ((ids >> 1) >= len(motion))
            assert (_bits(got[far]) == QNAN).all(), f"{where}: coords of a miss and of a surface beyond the table are the NaN the text writes"
    return got_hist


_CHAIN = {}


def _chain_inputs(qr, rm, base_name, w, h):
    """(stops, inputs) of an animated case, computed once: frames A, B, A' each rendered from its OWN Scene object -- view_hits
    and a spun 4-direction gather for the colour (four channels) --, the scenes closed again; a seeded variance"""
    import torch
    if (base_name, w, h) not in _CHAIN:
        v, off, plane_max = _view(qr, rm, base_name, w, h)
        frames = _frames(qr, base_name)[:3]
        hits, gathers = [], []
        for blob, _ in frames:
            scn = qr.Scene(blob, ray_queries=True)
            vt = TR.TPV._vt(scn, [v])
            ht = scn.view_hits(vt, w, h)
            spin = torch.from_numpy(rm.spins((1, h, w), 7)).to(vt.device)
            dirs = torch.from_numpy(rm.cosine_dirs(4)).to(vt.device)
            gat, _ = scn.view_gather(vt, dirs, w, h, eps=TA.EPS, reach=TA.REACH, frame=True, spin=spin)
            hits.append(_host(ht)[0]), gathers.append(_host(gat)[0])
            scn.close()
        x = dict(hits=np.stack(hits), gather=np.stack(gathers), view=v, motion=[m for _, m in frames],
                 var=np.random.default_rng(w * h).uniform(0.0, 0.1, (3, h, w)).astype(F))
        assert np.isfinite(x["gather"]).all() and x["gather"].shape[-1] == 4
        want = _records(qr, rm, base_name, w, h).view(np.int32)[:3, ..., 7]
        assert (x["hits"].view(np.int32)[..., 7] == want).all(), "the device's records are the ones the CPU test judged"
        _CHAIN[base_name, w, h] = (dict(plane_max=plane_max, off=off), x)
    return _CHAIN[base_name, w, h]


def _run_chain(qr, rm, scn, x, stops, where, combos):
    """A -> B -> A', each step's history the input of the next, with the step's motion table"""
    for ch, with_var, demod, outs in combos:
        p = rm.reproject_stops(demodulate=demod, **stops)
        prev, kept = None, 0
        for k in range(3):
            col = np.ascontiguousarray(x["gather"][k:k + 1, ..., :ch])
            var = x["var"][k:k + 1] if with_var else None
            hist = _call_moving(qr, rm, scn, col, x["hits"][k:k + 1], var, prev, x["motion"][k], p,
                                f"{where} ch {ch} var {with_var} demod {demod} outs {outs} step {k}", outs)
            prev = (x["view"][None], x["hits"][k:k + 1], hist)
            if k:
                ids = x["hits"][k].view(np.int32)[..., 7]
                moved = (ids >= 0) & ~_is_identity(x["motion"][k][np.where(ids >= 0, ids >> 1, 0)])
                kept += int((moved & (hist[0, ..., 6] > 1)).sum())
        assert kept > 0, f"{where}: no pixel of the moved object kept history"


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("base_name", sorted(ANIMATED))
def test_gpu_animated_chain(qr, rays_mod, base_name, size):
    """three frames of a turning object, each rendered from its own Scene; three steps A -> B -> A' with the frames' motion
    tables, launched on yet another scene (the call reads nothing of it but its device), in 3 and 4 channels, with and
    without var_in, DEMODULATE and each optional output"""
    w, h = size
    stops, x = _chain_inputs(qr, rays_mod, base_name, w, h)
    scn = qr.Scene(load_blob("demo01_160"))
    try:
        _run_chain(qr, rays_mod, scn, x, stops, f"{base_name} {w}x{h}", TR.COMBOS)
    finally:
        scn.close()


def _synthetic_ids(rec, prev, seed):
    out = _with_far_ids(rec, seed)
    return out, (prev[0], _with_far_ids(prev[1], seed + 1), prev[2])


@pytest.mark.gpu
@pytest.mark.parametrize("size", SYNTH_SIZES)
def test_gpu_synthetic_inputs(qr, rays_mod, size):
    """test_reproject's hand-made records (NaN, Inf, -0.0, misses) with ids beyond the table, under tables with rigid, NaN, Inf,
    huge and -0.0 rows and tables of one and two rows, at 1x1, 9x130, 67x45 and 33x9 in 3 and 4 channels"""
    w, h = size
    rm = rays_mod
    scn = qr.Scene(load_blob("demo01_160"))
    try:
        for ch in (3, 4):
            col, rec, var, prev = TR._synthetic(w, h, 11 * w + ch, ch)
            rec, prev = _synthetic_ids(rec, prev, 13 * w + ch)
            kws = (dict(plane_max=2.0 ** -5), dict(plane_max=2.0 ** -5, demodulate=True, var_min_len=1, max_len=8, unknown=np.nan),
                   dict(normal_min=-1.0, min_weight=0.3, alpha_min=1.0, alpha_mom_min=0.0, off=(0.5, -0.25)))
            for t, (name, m) in enumerate(_tables(17 * w + ch)):
                p = rm.reproject_stops(**kws[t % 3])
                _call_moving(qr, rm, scn, col, rec, var, prev, m, p, f"synthetic {w}x{h} ch {ch} {name}")
                _call_moving(qr, rm, scn, col, rec, None, prev, m, p, f"synthetic {w}x{h} ch {ch} {name} no variance", (True, False, True))
            _call_moving(qr, rm, scn, col, rec, var, None, _tables(1)[0][1], rm.reproject_stops(demodulate=True), f"synthetic {w}x{h} ch {ch} first frame")
    finally:
        scn.close()


def _wave_frame(kind, ch, seed):
    """a 64 x 2 frame, one workgroup's first wave per 32 x 8 tile: `distinct` -- every pixel its own surface, so all 64 lanes of
    a wave hold different rows --, `but one` -- one surface everywhere but at one pixel.  Every row slides its pixel by its own
    fraction of a pixel, so each keeps history through the taps of its own surface"""
    w, h = 64, 2
    rng = np.random.default_rng(seed)
    cur, old = _plane(w, h), _plane(w, h)
    ys, xs = np.mgrid[0:h, 0:w]
    srf = (xs + w * ys + 1) if kind == "distinct" else np.where((xs == 37) & (ys == 1), 9, 3)
    for r in (cur, old):
        r.view(np.int32)[..., 7] = srf * 2 + (xs & 1 if kind == "distinct" else 0)
    table = np.stack([_about_z(0.0, rng.integers(-7, 8) / 16.0 * S, rng.integers(-7, 8) / 16.0 * S) for _ in range(int(srf.max()) + 1)])
    table[0] = NAN
    col = rng.uniform(0.0, 1.0, (1, h, w, ch)).astype(F)
    return col, cur[None], (_dyadic_view(w, h)[None], old[None], _history(h, w, seed + 1, ch)[None]), table


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["distinct", "but one"])
def test_gpu_waves_of_many_surfaces_and_of_one(qr, rays_mod, kind):
    """the smallest shapes at which a wave-uniform row path could go wrong: all 64 lanes of a wave on different surfaces, and all
    lanes but one on the same"""
    rm = rays_mod
    scn = qr.Scene(load_blob("demo01_160"))
    try:
        for ch in (3, 4):
            col, rec, prev, table = _wave_frame(kind, ch, 70 + ch)
            hist = _call_moving(qr, rm, scn, col, rec, None, prev, table, rm.reproject_stops(plane_max=2.0 ** -4), f"{kind} ch {ch}")
            assert (hist[..., 6] > 1).sum() >= 64, "most pixels keep history through their own surface's taps"
            static = rm.reproject_pass(col, rec, None, prev, plane_max=F(2.0 ** -4))[0]
            assert (_bits(static) != _bits(hist)).any()
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_null_table_is_the_static_call(qr, rays_mod):
    """motion_dev = NULL, n_motion = 0 against qr_reproject_views_async on the same GPU and the same device buffers: every
    word of every output, in 3 and 4 channels, with and without a previous frame"""
    import torch
    rm = rays_mod
    w, h = 67, 45
    scn = qr.Scene(load_blob("demo01_160"))
    L = qr.lib()
    vp = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())
    try:
        for ch in (3, 4):
            col, rec, var, prev = TR._synthetic(w, h, 5 + ch, ch)
            d = [_dev(scn, a) for a in (col, rec, var)]
            pd = [_dev(scn, a) for a in prev]
            for first in (False, True):
                pv = [None] * 3 if first else pd
                cp = TR._params(qr, ch, rm.reproject_stops(plane_max=2.0 ** -5, demodulate=True))
                outs = [[torch.full(s, 7.5, dtype=torch.float32, device=d[0].device) for s in ((2, h, w, 8), (2, h, w, ch), (2, h, w), (2, h, w, 2))]
                        for _ in range(2)]
                assert L.qr_reproject_views_async(scn._h, vp(d[0]), vp(d[1]), vp(d[2]), vp(pv[0]), vp(pv[1]), vp(pv[2]), 2, w, h,
                                                  ctypes.byref(cp), *(vp(o) for o in outs[0]), None) == 0
                assert L.qr_reproject_moving_async(scn._h, vp(d[0]), vp(d[1]), vp(d[2]), vp(pv[0]), vp(pv[1]), vp(pv[2]), None, 0, 2, w, h,
                                                   ctypes.byref(cp), *(vp(o) for o in outs[1]), None) == 0
                torch.cuda.synchronize()
                for a, b in zip(*outs):
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"ch {ch} first {first}"
                assert not (outs[1][0] == 7.5).any().item()
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_views_streams_and_python(qr, rays_mod):
    """three views with three previous cameras and one table in one launch; view 1 alone gives the same bits; Scene.reproject
    (motion=) is the C call; the same call twice and a call on a side stream give the same bytes; what Python refuses"""
    import torch
    rm = rays_mod
    base_name, (w, h) = "demo02_160", SIZES[1]
    stops, x = _chain_inputs(qr, rm, base_name, w, h)
    p = rm.reproject_stops(**stops)
    scn = qr.Scene(load_blob("demo01_160"))
    try:
        va, vb, vc = x["view"], rm.jitter_view(x["view"], 0.5, -0.25), rm.jitter_view(x["view"], -0.25, 0.375)
        views = np.stack([va, vb, vc])
        # views 0 and 2: B against A; view 1: A' against B; the previous cameras of views 1 and 2 stand a fraction of a pixel
        # aside.  The table of A' serves as B's too (the same step every frame)
        cur, old = [1, 2, 1], [0, 1, 0]
        col, rec, var = np.ascontiguousarray(x["gather"][cur][..., :3]), x["hits"][cur], x["var"][cur]
        first = rm.reproject_pass(np.ascontiguousarray(x["gather"][old][..., :3]), x["hits"][old], None, None, **p)[0]
        prev = (views, x["hits"][old], first)
        m = x["motion"][2]
        hist = _call_moving(qr, rm, scn, col, rec, var, prev, m, p, "three views")
        assert all((hist[j, ..., 6] > 1).any() for j in range(3))
        alone = _call_moving(qr, rm, scn, col[1:2], rec[1:2], var[1:2], tuple(a[1:2] for a in prev), m, p, "view 1 alone")
        _same(alone[0], hist[1], "a view alone and as view 2 of 3")
        dev = [_dev(scn, a) for a in (col, rec, var)]
        pd = tuple(_dev(scn, a) for a in prev)
        md = _dev(scn, m)
        a = scn.reproject(dev[0], dev[1], pd, dev[2], coords=True, motion=md, **stops)
        b = scn.reproject(dev[0], dev[1], pd, dev[2], coords=True, motion=md, **stops)
        assert len(a) == 4 and tuple(a[0].shape) == (3, h, w, 8)
        _same(_host(a[0]), hist, "Scene.reproject(motion=) is the C call")
        for s, t in zip(a, b):
            assert torch.equal(s.view(torch.int32), t.view(torch.int32)), "the same call twice"
        plain = scn.reproject(dev[0], dev[1], pd, dev[2], coords=True, **stops)
        assert not torch.equal(plain[0].view(torch.int32), a[0].view(torch.int32)), "the table matters"
        side, ready, done = torch.cuda.Stream(), torch.cuda.Event(), torch.cuda.Event()
        c2 = dev[0].clone()
        ready.record()
        side.wait_event(ready)
        s = scn.reproject(c2, dev[1], pd, dev[2], coords=True, stream=side, motion=md, **stops)
        done.record(side)
        torch.cuda.current_stream().wait_event(done)
        for u, t in zip(s, a):
            assert torch.equal(u.view(torch.int32), t.view(torch.int32)), "a side stream"
        side.synchronize()
        for bad in (md.cpu(), md.double(), md[:, :11], md.t(), m, md[:0]):
            with pytest.raises(ValueError, match="motion must"):
                scn.reproject(dev[0], dev[1], pd, dev[2], motion=bad, **stops)
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_temporal_accumulator_on_animated_frames(qr, rays_mod):
    """Temporal.step(motion=, scene=) over 4 animated frames of two views, a fresh Scene per frame and the earlier ones closed
    -- the scene the accumulator was made with among them -- against rays.temporal; its output through Scene.denoise equals
    rays.denoise of the same input"""
    import torch
    rm = rays_mod
    base_name, (w, h) = "demo02_160", SIZES[0]
    v, off, plane_max = _view(qr, rm, base_name, w, h)
    views = np.stack([v, rm.jitter_view(v, 0.5, -0.25)])
    frames = _frames(qr, base_name, 3)
    kw = dict(plane_max=plane_max, off=off, demodulate=True, var_min_len=2)
    ref = rm.temporal(2, w, h, 3, **kw)
    acc, before, kept = None, None, 0
    for k, (blob, m) in enumerate(frames):
        scn = qr.Scene(blob, ray_queries=True)
        if acc is None:
            acc = scn.temporal(2, w, h, 3, **kw)
        vt = _dev(scn, views)
        hits = scn.view_hits(vt, w, h)
        spin = torch.from_numpy(rm.spins((2, h, w), 7 + k)).to(vt.device)
        gat, _ = scn.view_gather(vt, torch.from_numpy(rm.cosine_dirs(4)).to(vt.device), w, h, eps=TA.EPS, reach=TA.REACH, frame=True, spin=spin)
        col = gat[..., :3].contiguous()
        var = _dev(scn, np.random.default_rng(k).uniform(0.0, 0.1, (2, h, w)).astype(F))
        got = acc.step(col, hits, vt, var, motion=None if m is None else _dev(scn, m), scene=scn)
        want = ref.step(_host(col), _host(hits), views, _host(var), motion=m)
        _same(_host(got[0]), want[0], f"frame {k} colour"), _same(_host(got[1]), want[1], f"frame {k} variance")
        _same(_host(acc.history), ref.history, f"frame {k} history")
        assert acc.frames == k + 1
        if m is not None:
            ids = _host(hits).view(np.int32)[..., 7]
            moved = (ids >= 0) & ~_is_identity(m[np.where(ids >= 0, ids >> 1, 0)])
            kept += int((moved & (ref.length > 1)).sum())
        if k == len(frames) - 1:
            dkw = dict(passes=2, plane=plane_max, luma=4.0, normal_power=8)
            clean, cvar = scn.denoise(got[0], hits, got[1], **dkw)
            wc, wv = rm.denoise(want[0], want[1], _host(hits), **dkw)
            _same(_host(clean), wc, "denoise of the accumulated colour"), _same(_host(cvar), wv, "denoise of the accumulated variance")
            with pytest.raises(qr.QrError):
                acc.step(col, hits, vt, var)                 # the accumulator's own scene is closed: scene= is needed
        if before is not None:
            before.close()
        before = scn
    before.close()
    assert kept > 0 and (ref.length > 2).any(), "the moved object keeps history, some of it three frames long"


@pytest.mark.gpu
def test_gpu_refusals(qr, rays_mod):
    """every new QR_ERR_ARG and the static call's through the new entry point, the sentinel-filled outputs untouched after all
    of them; n_views = 0 is QR_OK; then calls that are served"""
    import torch
    rm = rays_mod
    L = qr.lib()
    scn = qr.Scene(load_blob("demo01_160"))
    dev = f"cuda:{scn.device}"
    n, w, h = 2, 9, 7
    z = lambda m: torch.zeros((m + 16,), dtype=torch.float32, device=dev)
    s75 = lambda m: torch.full((m + 16,), 7.5, dtype=torch.float32, device=dev)
    px = n * h * w
    col, hits, var, views, hprev, hin, table = z(px * 4), z(px * 12), z(px), z(n * 16), z(px * 12), z(px * 8), z(4 * 12)
    hout, cout, vout, xout = s75(px * 8), s75(px * 4), s75(px), s75(px * 2)
    vp = lambda x, off=0: ctypes.c_void_p(None if x is None else x.data_ptr() + off)
    nan, inf = float("nan"), float("inf")
    base = rm.reproject_stops(plane_max=0.5)

    def call(s=scn._h, ci=vp(col), hi=vp(hits), vi=vp(var), pv=vp(views), ph=vp(hprev), pi=vp(hin), mt=vp(table), nm=4, n=n, w=w, h=h,
             ho=vp(hout), co=vp(cout), vo=vp(vout), xo=vp(xout), null_p=False, channels=3, reserved=(0, 0, 0), **pk):
        p = TR._params(qr, channels, dict(base, **pk), reserved)
        return L.qr_reproject_moving_async(s, ci, hi, vi, pv, ph, pi, mt, nm, n, w, h, None if null_p else ctypes.byref(p), ho, co, vo, xo, None)

    none = vp(None)
    # the table
    assert call(mt=none) == ARG and call(mt=none, nm=1) == ARG, "a null table with rows"
    assert call(nm=0) == ARG, "a table without rows"
    assert call(nm=-1) == ARG and call(nm=(1 << 30) + 1) == ARG and call(nm=-(1 << 31)) == ARG and call(mt=none, nm=-1) == ARG
    for off in (4, 8, 12):
        assert call(mt=vp(table, off), nm=3) == ARG, "the table is 16-byte aligned"
    assert call(n=0, mt=none, nm=2) == ARG, "the table's checks come before the empty launch"
    # the static call's
    assert call(s=None) == ARG and call(null_p=True) == ARG
    assert call(ci=none) == ARG and call(hi=none) == ARG and call(ho=none) == ARG
    for name, buf in (("hi", hits), ("pv", views), ("ph", hprev), ("pi", hin), ("ho", hout)):
        for off in (4, 8, 12):
            assert call(**{name: vp(buf, off)}) == ARG, f"{name} is 16-byte aligned"
    for name, buf in (("ci", col), ("vi", var), ("co", cout), ("vo", vout), ("xo", xout)):
        for off in (1, 2, 3):
            assert call(**{name: vp(buf, off)}) == ARG, f"{name} is 4-byte aligned"
    for some in ((none, None, None), (None, none, None), (None, None, none), (none, none, None), (none, None, none), (None, none, none)):
        kw = {k: v for k, v in zip(("pv", "ph", "pi"), some) if v is not None}
        assert call(**kw) == ARG, "the previous triple goes together"
    assert call(ho=vp(hin)) == ARG, "hist_out == hist_in"
    assert call(channels=2) == ARG and call(channels=5) == ARG and call(channels=0) == ARG
    assert call(flags=2) == ARG and call(flags=0x80000000) == ARG and call(flags=3) == ARG
    assert call(reserved=(1, 0, 0)) == ARG and call(reserved=(0, 1, 0)) == ARG and call(reserved=(0, 0, 0x80000000)) == ARG
    for name in ("plane_max", "max_len", "alb_floor"):
        for bad in (0.0, -1.0, nan, -0.0):
            assert call(**{name: bad}) == ARG, (name, bad)
    assert call(min_weight=-1e-6) == ARG and call(min_weight=nan) == ARG
    for name in ("alpha_min", "alpha_mom_min"):
        for bad in (-0.01, 1.01, nan, inf):
            assert call(**{name: bad}) == ARG, (name, bad)
    for name in ("max_len", "var_min_len"):
        for bad in (0.5, 0.0, nan, -inf):
            assert call(**{name: bad}) == ARG, (name, bad)
    assert call(normal_min=nan) == ARG
    for name in ("off_x", "off_y"):
        for bad in (inf, -inf, nan):
            assert call(**{name: bad}) == ARG, (name, bad)
    assert call(w=0) == ARG and call(h=0) == ARG and call(w=16385) == ARG and call(h=16385) == ARG and call(w=-3) == ARG
    assert call(n=-1) == ARG and call(n=65536) == ARG
    assert call(n=0) == 0 and call(n=0, ci=none, hi=none, ho=none) == 0 and call(n=0, mt=none, nm=0) == 0
    torch.cuda.synchronize()
    for t in (hout, cout, vout, xout):
        assert (t == 7.5).all().item(), "a refused call wrote something"
    # served: a table at an offset that keeps the alignment, one row, no table, the first frame, no optional output, four channels
    assert call() == 0 and call(mt=vp(table, 48), nm=3) == 0 and call(nm=1) == 0 and call(mt=none, nm=0) == 0
    assert call(pv=none, ph=none, pi=none) == 0 and call(vi=none, co=none, vo=none, xo=none) == 0
    assert call(channels=4, flags=1, unknown=nan, min_weight=-0.0, alpha_min=0.0, alpha_mom_min=1.0, max_len=inf, var_min_len=1.0,
                plane_max=inf, normal_min=-inf) == 0
    torch.cuda.synchronize()
    assert (hout[:px * 8] != 7.5).all().item() and (hout[px * 8:] == 7.5).all().item()
    scn.close()


# once more through the guarded diagnostic build (make guard), as tests/test_reproject.py does it: the library is chosen when
# the package is imported, hence the child process: this file run as a script.

def _guard_child():
    from qr_loader import load_package
    qr = load_package()
    assert qr.LIB_PATH == GUARD_LIB, qr.LIB_PATH
    rm = _rays_mod()
    base_name, (w, h) = "demo02_160", SIZES[1]
    stops, x = _chain_inputs(qr, rm, base_name, w, h)
    scn = qr.Scene(load_blob("demo01_160"))
    _run_chain(qr, rm, scn, x, stops, f"guard {base_name}", TR.COMBOS[:3])
    scn.close()
    print(f"{base_name} guard_ok 1", flush=True)
    return 0


@pytest.mark.gpu
def test_gpu_guarded_build_gives_the_same_history():
    assert os.path.exists(GUARD_LIB), "libqrhip_guard.so is missing: build() makes it (make -C quadray-engine_amd/csrc guard)"
    env = dict(os.environ, QR_LIB=GUARD_LIB)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-child"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.count("guard_ok 1") == 1 and "QR_GUARD" not in out.stderr, out.stdout + out.stderr[-3000:]


if __name__ == "__main__":
    sys.exit(_guard_child() if "--guard-child" in sys.argv else 2)
