"""Guided upsampling (include/qrhip.h qr_upsample_views_async; Scene.upsample; rays.upsample_pass, rays.upsample_stops,
rays.coarse_size, rays.coarse_hits, rays.coarse_view).

The call is a pure function of its inputs and its arithmetic is pinned to the operation, so there is no oracle: the CPU tests
check the numpy statement against cases worked out by hand (one tap, a dyadic blend, a scalar restatement of the header's text,
each stage next to its nearest neighbour case) and on real hit records of the oracle; the GPU tests check every word the kernel
writes against the numpy statement on the inputs copied back from the device.  Every comparison is bit for bit, except that two
NaNs count as equal."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import test_atrous as TA
import test_hit_records as THR
import test_pt_views as TPV
import test_reproject as TR
from conftest import ROOT
from test_atrous import SENTINEL, _bits, _dev, _flat, _host
from test_pt_views import _base, _cams, _rays_mod
from test_reproject import _buffer, _same

F = np.float32
ARG = -1
GUARD_LIB = TPV.GUARD_LIB
ASM = TPV.ASM
NORMAL, PLANE, SAME_ID, DEMOD, MOD = 1, 2, 4, 8, 16
GUIDE_SCENE, VIEW_SCENE = "patched:demo02_160_gf_aa4", "pt:test18_160_pt"
REAL_INPUTS = [(GUIDE_SCENE, 0), (GUIDE_SCENE, 1), (VIEW_SCENE, 1)]                 # (scene, seeded camera)
REAL_SIZES = [(64, 64), (67, 45), (9, 130)]                                         # (w, h)
SYNTH_SIZES = [(1, 1), (9, 130), (67, 45), (33, 9)]                                 # 33 x 9: one tile plus one pixel each way
FACTORS = [1, 2, 3, 4, 8, 16]
FRAGS = ("18qr_upsample_kernelILi3EE", "18qr_upsample_kernelILi4EE")


@pytest.fixture(scope="module")
def rays_mod():
    return _rays_mod()


def _phases(s, w, h):
    """(0, 0), (1, 1) and (s - 1, 0), without repeats, of those the lattice has and that lie inside the frame"""
    out = []
    for ph in ((0, 0), (1, 1), (s - 1, 0)):
        if ph not in out and max(ph) < s and ph[0] < w and ph[1] < h:
            out.append(ph)
    return out


def _stage_counts(weight):
    return int((weight > 0).sum()), int((weight == 0).sum()), int((weight < 0).sum())


# ------------------------------------------------------------------------------------------------- names and sizes

def test_symbols_constants_and_header(qr, rays_mod):
    hdr = open(os.path.join(ROOT, "include", "qrhip.h")).read()
    assert "qr_upsample_views_async" in qr.ABI_SYMBOLS and "qr_upsample_views_async(" in hdr
    assert hasattr(qr.lib(), "qr_upsample_views_async") and len(qr.lib().qr_upsample_views_async.argtypes) == 12
    assert ctypes.sizeof(qr.UpsampleParams) == 32 and "typedef struct qr_upsample_params" in hdr
    assert [n for n, _ in qr.UpsampleParams._fields_] == ["factor", "phase_x", "phase_y", "channels", "normal_sq", "flags", "sigma_z",
                                                          "alb_floor"]
    for name, val in (("NORMAL", 1), ("PLANE", 2), ("SAME_ID", 4), ("DEMODULATE", 8), ("MODULATE", 16), ("MAX_FACTOR", 16)):
        assert getattr(qr, "UPSAMPLE_" + name) == val == getattr(rays_mod, "UPSAMPLE_" + name)
        assert f"#define QR_UPSAMPLE_{name} " in hdr
    for text in ("w = b * g", "2 * rx >= s", "X0 = floor_div(x - px, s)", "wx = (float)rx / (float)s", "sv += var_Q * (w * w)",
                 "b = (i ? wx : 1.0f - wx) * (j ? wy : 1.0f - wy)", "weight = -1.0f", "weight = +0.0f", "t = fabsf(d) / sigma_z"):
        assert text in hdr, text
    assert callable(qr.Scene.upsample)
    for m in ("upsample_pass", "upsample_stops", "coarse_size", "coarse_hits", "coarse_view"):
        assert callable(getattr(rays_mod, m))


def test_kernels_in_resource_check():
    """both instances are held to a budget by the build's own check, and the build's assembly meets it"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import check_kernel_resources as ck
    finally:
        sys.path.pop(0)
    for frag in FRAGS:
        vg, spill, scratch = ck.LIMITS[frag]
        assert vg <= 64 and spill == 0 and scratch == 0 and 0 < ck.LDS_LIMITS[frag] <= 34 * 10 * 12 * 4
    if os.path.exists(ASM):
        mine = [k for k in ck.kernels(ASM) if "qr_upsample_kernel" in k["name"]]
        assert len(mine) == 2
        for k in mine:
            frag = next(f for f in FRAGS if f in k["name"])
            assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0
            assert k["vgpr_count"] <= ck.LIMITS[frag][0] and 0 < k["group_segment_fixed_size"] <= ck.LDS_LIMITS[frag]


# ------------------------------------------------------------------------------------------------- the lattice and the camera

def test_coarse_size_and_hits(rays_mod):
    rm = rays_mod
    for w, h in ((1, 1), (9, 130), (67, 45), (64, 64), (33, 9)):
        for s in FACTORS:
            for px in range(min(s, w)):
                for py in (0, min(s, h) - 1):
                    wl, hl = rm.coarse_size(w, h, s, (px, py))
                    assert wl == len(range(px, w, s)) >= 1 and hl == len(range(py, h, s)) >= 1
                    assert s * (wl - 1) + px <= w - 1 < s * wl + px and s * (hl - 1) + py <= h - 1 < s * hl + py
    hits = np.arange(2 * 7 * 9 * 12, dtype=F).reshape(2, 7, 9, 12)
    c = rm.coarse_hits(hits, 3, (2, 1))
    assert c.shape == (2, 2, 3, 12) and c.flags["C_CONTIGUOUS"] and (c == hits[:, 1::3, 2::3]).all()
    assert (rm.coarse_hits(hits[0], 3, (2, 1)) == c[0]).all()
    import torch
    t = rm.coarse_hits(torch.from_numpy(hits), 3, (2, 1))
    assert t.is_contiguous() and (t.numpy() == c).all()
    for bad in (dict(factor=0), dict(factor=17), dict(factor=2.0), dict(factor=True), dict(phase=(2, 0)), dict(phase=(0, -1)),
                dict(phase=(0, 0, 0)), dict(phase=1), dict(phase=(0.0, 0)), dict(width=0), dict(height=0), dict(width=2.5)):
        with pytest.raises(ValueError):
            rm.coarse_size(**dict(dict(width=8, height=8, factor=2, phase=(0, 0)), **bad))
    for w, h, s, ph in ((3, 8, 4, (3, 0)), (8, 2, 4, (0, 2)), (1, 1, 2, (1, 1))):
        with pytest.raises(ValueError, match="empty"):
            rm.coarse_size(w, h, s, ph)
    with pytest.raises(ValueError):
        rm.coarse_hits(hits[..., :11], 2)


def _look_at(rm, w, h):
    """a look_at camera where the scene's seeded camera 1 stands, at w x h"""
    return TR._cameras(rm, VIEW_SCENE, w, h, 1.0)[0]


@pytest.mark.parametrize("size", REAL_SIZES)
def test_coarse_view(rays_mod, size):
    """at phase (0, 0) and a power of two the coarse view's rays ARE the strided full rays, and so are the oracle's records; at
    every other factor and phase the directions agree to 4 * 2^-24 of the frame's largest direction component: the two texts --
    (hor * s) * X + ... + (dir + hor * px + ...) and hor * (s * X + px) + ... + dir -- differ by that many roundings"""
    rm = rays_mod
    w, h = size
    blob = _base(VIEW_SCENE)
    assert TPV._fsaa(blob) == 0
    v = _look_at(rm, w, h)
    full = rm.view_rays(v, w, h, blob).reshape(h, w, 8)
    helper = THR._helper()
    full_rec = helper(blob, full.reshape(-1, 8)).reshape(h, w, 12)
    assert (full_rec.view(np.int32)[..., 7] >= 0).any()
    for s in (2, 4, 8):
        cv = rm.coarse_view(v, s)
        wl, hl = rm.coarse_size(w, h, s)
        assert (cv[0:4] == v[0:4]).all() and cv[7] == v[7] and (cv[4:7] == v[4:7]).all() and cv.dtype == np.float32
        got = rm.view_rays(cv, wl, hl, blob)
        _same(got.reshape(hl, wl, 8), full[::s, ::s], f"{w}x{h} factor {s}")
        _same(helper(blob, got).reshape(hl, wl, 12), full_rec[::s, ::s], f"{w}x{h} factor {s}: the oracle's records")
    scale = float(np.abs(full[..., 4:7]).max())
    worst = 0.0
    for s, ph in ((3, (0, 0)), (3, (1, 1)), (3, (2, 0)), (2, (1, 1)), (2, (1, 0)), (4, (1, 1)), (4, (3, 0)), (8, (1, 1)), (8, (7, 0))):
        cv = rm.coarse_view(v, s, ph)
        wl, hl = rm.coarse_size(w, h, s, ph)
        got = rm.view_rays(cv, wl, hl, blob).reshape(hl, wl, 8)
        want = full[ph[1]::s, ph[0]::s]
        assert (got[..., 0:4] == want[..., 0:4]).all() and (got[..., 7] == want[..., 7]).all()
        err = float(np.abs(got[..., 4:7].astype(np.float64) - want[..., 4:7]).max()) / (2.0 ** -24 * scale)
        print(f"{w}x{h} factor {s} phase {ph}: {err:.2f} x 2^-24 of the largest component")
        worst = max(worst, err)
    assert worst <= 4.0, worst


# ------------------------------------------------------------------------------------------------- the numpy statement by hand

def _alb(a, floor):
    return a if a > floor else floor


def _pixel(col_lo, var_lo, rec, s, ph, x, y, flags=0, normal_sq=0, sigma_z=1.0, alb_floor=1 / 256):
    """the header's text for ONE full pixel in scalar float32, written a second time: (colour [C], variance, weight)"""
    f = F
    px, py = ph
    h, w = rec.shape[:2]
    hl, wl, ch = col_lo.shape
    sigma_z, alb_floor = f(sigma_z), f(alb_floor)
    ids = rec.view(np.int32)[..., 7]

    def read(qx, qy):
        g = rec[s * qy + py, s * qx + px]
        c = [f(col_lo[qy, qx, k]) for k in range(ch)]
        if flags & DEMOD and ids[s * qy + py, s * qx + px] >= 0:
            for k in range(3):
                c[k] = c[k] / _alb(g[8 + k], alb_floor)
        return c, (f(0) if var_lo is None else var_lo[qy, qx])

    with np.errstate(all="ignore"):
        x0, y0 = (x - px) // s, (y - py) // s
        rx, ry = (x - px) - x0 * s, (y - py) - y0 * s
        wx, wy = f(rx) / f(s), f(ry) / f(s)
        p = rec[y, x]
        idp = int(ids[y, x])
        taps = []
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                b = (wx if i else f(1) - wx) * (wy if j else f(1) - wy)
                if not (0 <= qx < wl and 0 <= qy < hl):
                    continue
                g_rec = rec[s * qy + py, s * qx + px]
                idg = int(ids[s * qy + py, s * qx + px])
                if idp < 0:
                    if idg >= 0:
                        continue
                    g = f(1)
                else:
                    if idg < 0 or (flags & SAME_ID and idg != idp):
                        continue
                    g = f(1)
                    if flags & NORMAL:
                        d = (p[4] * g_rec[4] + p[5] * g_rec[5]) + p[6] * g_rec[6]
                        d = d if 0 < d else f(0)
                        for _ in range(normal_sq):
                            d = d * d
                        g = g * d
                    if flags & PLANE:
                        e = [g_rec[k] - p[k] for k in range(3)]
                        d = (p[4] * e[0] + p[5] * e[1]) + p[6] * e[2]
                        t = np.abs(d) / sigma_z
                        g = g * (f(1) / (f(1) + t * t))
                taps.append((qx, qy, b, g))
        out = None
        for stage in (1, 2):
            sc, sw, sv, took = [f(0)] * ch, f(0), f(0), False
            for qx, qy, b, g in taps:
                wt = b * g if stage == 1 else g
                if 0 < wt:
                    c, v = read(qx, qy)
                    sc = [sc[k] + c[k] * wt for k in range(ch)]
                    sw, sv, took = sw + wt, sv + v * (wt * wt), True
            if took:
                out = [sc[k] / sw for k in range(ch)], sv / (sw * sw), (sw if stage == 1 else f(0.0))
                break
        if out is None:
            qx = min(max(x0 + (1 if 2 * rx >= s else 0), 0), wl - 1)
            qy = min(max(y0 + (1 if 2 * ry >= s else 0), 0), hl - 1)
            c, v = read(qx, qy)
            out = c, v, f(-1.0)
        c, v, wgt = out
        if flags & MOD and idp >= 0:
            c = [c[k] * _alb(p[8 + k], alb_floor) if k < 3 else c[k] for k in range(ch)]
    return np.array(c, dtype=F), F(v), F(wgt)


def _against_scalar(rm, col_lo, var_lo, rec, s, ph, where, **kw):
    got = rm.upsample_pass(col_lo, var_lo, rec, s, ph, **kw)
    h, w = rec.shape[:2]
    for y in range(h):
        for x in range(w):
            c, v, wgt = _pixel(col_lo, var_lo, rec, s, ph, x, y, **kw)
            _same(got[0][y, x], c, f"{where} colour ({x}, {y})")
            if var_lo is not None:
                _same(got[1][y, x], v, f"{where} variance ({x}, {y})")
            _same(got[2][y, x], wgt, f"{where} weight ({x}, {y})")
            assert _bits(got[2][y, x]) in (0, 0xBF800000) or got[2][y, x] > 0, "the weight is positive, +0.0 or -1.0"
    assert got[1] is None or var_lo is not None
    return got


def _coarse(rm, h, w, s, ph, seed, ch=3):
    rng = np.random.default_rng(seed)
    wl, hl = rm.coarse_size(w, h, s, ph)
    return rng.uniform(0.0, 1.0, (hl, wl, ch)).astype(F), rng.uniform(0.001, 0.05, (hl, wl)).astype(F)


@pytest.mark.parametrize("ch", [3, 4])
def test_factor_one_is_one_tap(rays_mod, ch):
    """factor 1: rx = 0, the pixel's own tap has b = 1 and g = 1, the other three b = 0: (c * 1) / 1, the variance (v * 1) / 1"""
    rm = rays_mod
    col, var, rec = TA._random_frame(11, 13, 3, ch)
    taps = []
    out, vo, wgt = rm.upsample_pass(col, var, rec, 1, flags=PLANE | SAME_ID, sigma_z=0.01, taps=taps)
    _same(out, col, "factor 1 colour"), _same(vo, var, "factor 1 variance")
    assert (wgt == 1).all() and len(taps) == 4 and (taps[0][1] == 1).all() and all((t[1] == 0).all() for t in taps[1:])
    ids = rec.view(np.int32)[..., 7]
    assert (ids < 0).any(), "a miss pixel takes its own miss tap"
    # with the normal stop the one weight is (n . n)^128 of a normal that is a unit vector only to rounding: (c * w) / w
    out, vo, wgt = rm.upsample_pass(col, var, rec, 1, flags=NORMAL | PLANE | SAME_ID, normal_sq=7, sigma_z=0.01)
    assert (np.abs(wgt - 1) < 1e-4).all() and (wgt[ids < 0] == 1).all()
    _same(out, (F(0) + col * wgt[..., None]) / wgt[..., None], "one tap with its weight")
    _same(vo, (F(0) + var * (wgt * wgt)) / (wgt * wgt), "one tap's variance")


def test_dyadic_blend_by_hand(rays_mod):
    """factor 4, phase (0, 0), pixel (1, 3) on a flat guide: rx = 1, ry = 3, the weights are 3/16, 1/16, 9/16, 3/16 and sum to
    exactly 1; the blend written out matches bit for bit; the whole frame agrees with the scalar restatement"""
    rm = rays_mod
    h, w, s = 10, 11, 4
    rec = _flat(h, w)
    col, var = _coarse(rm, h, w, s, (0, 0), 5)
    out, vo, wgt = _against_scalar(rm, col, var, rec, s, (0, 0), "dyadic")
    b = [F(0.75) * F(0.25), F(0.25) * F(0.25), F(0.75) * F(0.75), F(0.25) * F(0.75)]
    assert [float(x) for x in b] == [3 / 16, 1 / 16, 9 / 16, 3 / 16]
    taps = [(0, 0), (0, 1), (1, 0), (1, 1)]                 # (row, column) of the coarse taps of full pixel (1, 3)
    sw = ((F(0) + b[0] + b[1]) + b[2]) + b[3]
    assert sw == 1.0 and wgt[3, 1] == 1.0
    for k in range(3):
        sc = F(0)
        for t, bb in zip(taps, b):
            sc = sc + col[t][k] * bb
        assert _bits(out[3, 1, k]) == _bits(sc / sw)
    sv = F(0)
    for t, bb in zip(taps, b):
        sv = sv + var[t] * (bb * bb)
    assert _bits(vo[3, 1]) == _bits(sv / (sw * sw))
    # the last lattice column is 8, the last row 8: pixels right of and below them lose the taps off the coarse frame
    assert wgt[3, 10] == F(0.5) * F(0.25) + F(0.5) * F(0.75) and wgt[9, 9] == F(0.75) * F(0.75)


@pytest.mark.parametrize("s,ph", [(1, (0, 0)), (2, (0, 0)), (2, (1, 1)), (3, (2, 0)), (4, (1, 1)), (5, (4, 0)), (16, (1, 1)), (16, (15, 0))])
def test_scalar_restatement_on_a_synthetic_frame(rays_mod, s, ph):
    """two tilted surfaces, a strip of misses, NaN, Inf, -0.0 and denormal guides: every pixel against the scalar text, with all
    stops and de/modulation in four channels, and without any in three"""
    rm = rays_mod
    h, w = 19, 23
    _, _, rec = TA._random_frame(h, w, 100 + s)
    rng = np.random.default_rng(s)
    for word in (0, 1, 2, 4, 5, 6, 8, 9, 10):
        for val in (np.nan, np.inf, -np.inf, -0.0, 1e-42):
            rec[..., word] = np.where(rng.uniform(size=(h, w)) < 0.02, F(val), rec[..., word])
    col, var = _coarse(rm, h, w, s, ph, 7, 4)
    full = dict(flags=NORMAL | PLANE | DEMOD | MOD, normal_sq=3, sigma_z=0.5, alb_floor=1 / 64)
    got = _against_scalar(rm, col, var, rec, s, ph, f"factor {s} phase {ph}", **full)
    _against_scalar(rm, col, var, rec, s, ph, f"factor {s} phase {ph} same id", **dict(full, flags=31, normal_sq=0))
    _against_scalar(rm, col[..., :3].copy(), None, rec, s, ph, f"factor {s} phase {ph} plain")
    if s in (2, 3, 4):
        assert min(_stage_counts(got[2])) > 0, _stage_counts(got[2])
    # a [H, W] call is the [1, H, W] call
    many = rm.upsample_pass(col[None], var[None], rec[None], s, ph, **full)
    for a, b in zip(got, many):
        _same(a, b[0], "single view")


def test_each_stage_next_to_its_neighbour(rays_mod):
    rm = rays_mod
    h, w, s, ph = 13, 14, 4, (1, 2)
    col, var = _coarse(rm, h, w, s, ph, 11)
    kw = dict(flags=NORMAL | PLANE, normal_sq=2, sigma_z=0.5)
    nan = F(np.nan)

    def run(edit=None):
        rec = _flat(h, w)
        if edit:
            edit(rec)
        return rec, _against_scalar(rm, col, var, rec, s, ph, "stages", **kw)

    # a lattice pixel whose own tap is open: stage 1, weight exactly 1, its own coarse colour
    rec, (out, vo, wgt) = run()
    assert (wgt > 0).all()
    x, y = 1 + 4 * 2, 2 + 4 * 1                                             # coarse (2, 1)
    assert wgt[y, x] == 1.0
    _same(out[y, x], col[1, 2], "own tap"), _same(vo[y, x], var[1, 2], "own tap variance")
    # the same pixel with a NaN normal: every g is NaN, nothing is eligible at any weight: stage 3, the nearest is itself
    rec, (out, vo, wgt) = run(lambda r: r[y, x].__setitem__(4, nan))
    assert _bits(wgt[y, x]) == 0xBF800000
    _same(out[y, x], col[1, 2], "stage 3 takes the nearest"), _same(vo[y, x], var[1, 2], "stage 3 variance")
    # the pixel next to it: its own normal is fine but the lattice point's normal is NaN: that tap is closed (b = 3/4), the
    # others stay open: stage 1 with less weight
    assert 0 < wgt[y, x + 1] < 1 and wgt[y, x + 1] == F(0.25)
    # stage 2: a pixel on a lattice ROW (wy = 0) between two lattice columns whose two row taps are closed (another id under
    # SAME_ID) while the row below (b = 0) is open
    def other_id(r):
        r.view(np.int32)[y, x, 7] = 6
        r.view(np.int32)[y, x + 4, 7] = 6
    rec = _flat(h, w)
    other_id(rec)
    k2 = dict(kw, flags=NORMAL | PLANE | SAME_ID)
    out, vo, wgt = _against_scalar(rm, col, var, rec, s, ph, "stage 2", **k2)
    for dx in (1, 2, 3):
        assert _bits(wgt[y, x + dx]) == 0, "stage 2 writes +0.0"
    # ... and is the plain mean of the two open taps below, g = 1 each on the flat guide
    want = (F(0) + col[2, 2] * F(1) + col[2, 3] * F(1)) / (F(0) + F(1) + F(1))
    _same(out[y, x + 1], want, "stage 2 colour")
    _same(vo[y, x + 1], (F(0) + var[2, 2] + var[2, 3]) / F(4), "stage 2 variance")
    assert wgt[y + 1, x + 1] > 0, "one row further down the taps below have weight: stage 1"
    # without SAME_ID the same pixel is served by stage 1: the stop closes what NORMAL alone leaves open
    out1, _, wgt1 = rm.upsample_pass(col, var, rec, s, ph, **kw)
    assert wgt1[y, x + 1] == 1.0 and (wgt1 > 0).all()
    # stage 3 clamps at each of the four borders: a frame of hits whose lattice points are all misses is served by nothing
    rec = _flat(h, w)
    rec.view(np.int32)[ph[1]::s, ph[0]::s, 7] = -1
    out, vo, wgt = _against_scalar(rm, col, var, rec, s, ph, "all lattice points miss", **kw)
    hit = rec.view(np.int32)[..., 7] >= 0
    assert (wgt[hit] == -1).all() and (wgt[~hit] == 1).all()
    wl, hl = rm.coarse_size(w, h, s, ph)
    assert (wl, hl) == (4, 3)
    _same(out[0, 0], col[0, 0], "left and above the lattice: clamped to coarse (0, 0)")
    _same(out[h - 1, w - 1], col[hl - 1, wl - 1], "right and below")
    _same(out[0, w - 1], col[0, wl - 1], "above, right"), _same(out[h - 1, 0], col[hl - 1, 0], "below, left")
    _same(out[5, 4], col[1, 1], "2 * rx >= s rounds up: rx = 3 of 4"), _same(out[5, 3], col[1, 1], "rx = 2 of 4 rounds up")
    _same(out[5, 2], col[1, 0], "rx = 1 of 4 stays")


def test_a_miss_pixel_takes_only_miss_taps(rays_mod):
    rm = rays_mod
    h, w, s = 9, 9, 4
    col, var = _coarse(rm, h, w, s, (0, 0), 13)
    rec = _flat(h, w)
    ids = rec.view(np.int32)[..., 7]
    ids[:, 7:] = -1                                         # lattice columns 0, 4 hit; column 8 miss
    rec[:, 7:, 4:7] = np.nan                                # a miss's normal is never looked at
    out, vo, wgt = _against_scalar(rm, col, var, rec, s, (0, 0), "misses", flags=NORMAL | PLANE | DEMOD | MOD, normal_sq=7, sigma_z=0.1)
    _same(out[0, 8], col[0, 2], "a miss lattice pixel is its own coarse colour, never divided")
    assert wgt[0, 8] == 1 and wgt[0, 7] == F(0.75), "a miss pixel: only the miss column counts"
    _same(out[0, 7], (F(0) + col[0, 2] * F(0.75)) / F(0.75), "one miss tap")
    assert wgt[0, 5] == F(0.75) and wgt[0, 6] == F(0.5) and wgt[0, 4] == 1 and wgt[0, 3] == 1, "a hit pixel takes only hit taps"
    alb = F(0.5)
    _same(out[0, 6], ((F(0) + (col[0, 1] / alb) * F(0.5)) / F(0.5)) * alb, "one hit tap, divided and multiplied back")


@pytest.mark.parametrize("ch", [3, 4])
def test_demodulate_then_modulate_keeps_textures(rays_mod, ch):
    """a coarse colour alb_G * L with a textured albedo and constant L: the demodulated lattice holds (alb_G * L) / alb_G, the
    blend of those is within the pinned arithmetic's own bits of L, and the output is that times alb_p: the full pixel's texture,
    not a blur of the lattice's.  The fourth channel is neither divided nor multiplied"""
    rm = rays_mod
    h, w, s, ph = 17, 18, 4, (1, 1)
    rng = np.random.default_rng(21)
    rec = _flat(h, w)
    rec[..., 8:11] = rng.uniform(0.1, 1.0, (h, w, 3)).astype(F)
    L = np.array([0.75, 0.5, 1.5, 0.3], dtype=F)[:ch]
    wl, hl = rm.coarse_size(w, h, s, ph)
    col = np.empty((hl, wl, ch), dtype=F)
    col[..., 0:3] = rec[ph[1]::s, ph[0]::s, 8:11] * L[0:3]
    if ch == 4:
        col[..., 3] = L[3]
    out, _, wgt = _against_scalar(rm, col, None, rec, s, ph, "textured", flags=DEMOD | MOD)
    assert (wgt > 0).all()
    # roundings, each at most 2^-24 relative: a * L and the division by a 2, c * w 1, three adds into sc (sw is exact: the weights
    # are sixteenths), the division by sw 1, the product with alb_p 1, and the reference's own product 1: 9; 10 covers their
    # second-order terms
    want = rec[..., 8:11] * L[0:3]
    assert np.abs(out[..., 0:3] / want - 1).max() <= 10 * 2.0 ** -24
    blur = rm.upsample_pass(col, None, rec, s, ph)[0]
    assert np.abs(blur[..., 0:3] / want - 1).max() > 0.1, "without de/modulation the lattice's texture is smeared"
    if ch == 4:
        assert np.abs(out[..., 3] / L[3] - 1).max() <= 6 * 2.0 ** -24       # c * w, three adds, the division: 5
    # the floor and the NaN rule, on both sides
    rec[5, 5, 8:11] = (0.0, np.nan, -1.0)                   # the lattice point (1, 1) and the pixel itself
    out = _against_scalar(rm, col, None, rec, s, ph, "floor", flags=DEMOD | MOD, alb_floor=1 / 64)[0]
    _same(out[5, 5, 0:3], (F(0) + (col[1, 1, 0:3] / F(1 / 64)) * F(1)) / F(1) * F(1 / 64), "zero, NaN and negative albedo give the floor")


def test_variance_factor_on_a_flat_guide(rays_mod):
    """constant variance v on a flat guide without stops: a lattice pixel keeps v, a pixel half way between two lattice points
    gets v / 2, one in the middle of four v / 4: sum(w^2) / sum(w)^2"""
    rm = rays_mod
    h, w, s = 9, 9, 2
    col, _ = _coarse(rm, h, w, s, (0, 0), 2)
    var = np.full(col.shape[:2], F(0.5))
    _, vo, wgt = rm.upsample_pass(col, var, _flat(h, w), s)
    assert (wgt == 1).all()
    assert vo[2, 2] == 0.5 and vo[2, 3] == 0.25 and vo[3, 2] == 0.25 and vo[3, 3] == 0.125
    assert rm.upsample_pass(col, None, _flat(h, w), s)[1] is None


def test_float64_evaluation_agrees(rays_mod):
    """|fp32 - fp64| <= 16 * 2^-24 * (sum |c_Q| w / sum w) per channel, with the fp32 run's taken / not taken decisions and
    stages.  The cap counts roundings, each at most 2^-24 relative, on the longest path of a term c_Q w / sw: the weight -- the
    dot 3, three squarings, the plane stop's 5 on top of its dot, g * d and b * g 2 more, of which the dominant ones are shared
    by sum_c and sum_w and cancel --, c * w 1, at most 4 adds into sc and 4 into sw, the division 1: 16 covers the count.  The
    differences inside the plane stop cancel and could amplify; positions within a few units of each other with sigma_z = 0.5
    keep that small.  A derived cap, not a measurement"""
    rm = rays_mod
    h, w = 23, 29
    _, _, rec = TA._random_frame(h, w, 77)
    d64 = np.float64
    worst = 0.0
    for s, ph in ((2, (1, 0)), (3, (1, 1)), (4, (0, 0))):
        col, var = _coarse(rm, h, w, s, ph, 5)
        kw = dict(flags=NORMAL | PLANE, normal_sq=3, sigma_z=0.5)
        taps = []
        out, _, wgt = rm.upsample_pass(col, var, rec, s, ph, taps=taps, **kw)
        pos, nrm = rec[..., 0:3].astype(d64), rec[..., 4:7].astype(d64)
        g = rec[ph[1]::s, ph[0]::s]
        hit = rec.view(np.int32)[..., 7] >= 0
        ys, xs = np.mgrid[0:h, 0:w]
        wx = ((xs - ph[0]) % s) / s
        wy = ((ys - ph[1]) % s) / s
        acc = {}
        for stage in (1, 2):
            sc, sa, sw = np.zeros((h, w, 3)), np.zeros((h, w, 3)), np.zeros((h, w))
            for t, (elig, b32, g32, qy, qx) in enumerate(taps):
                i, j = t & 1, t >> 1
                b = (wx if i else 1 - wx) * (wy if j else 1 - wy)
                d = np.maximum((nrm * g[qy, qx, 4:7].astype(d64)).sum(-1), 0.0) ** 8
                x = np.abs((nrm * (g[qy, qx, 0:3].astype(d64) - pos)).sum(-1)) / d64(F(0.5))
                gw = np.where(hit, d / (1 + x * x), 1.0)
                w32 = b32 * g32[0] if stage == 1 else g32[0]
                wt = np.where(elig[0] & (0 < w32), b * gw if stage == 1 else gw, 0.0)
                sc += col[qy, qx].astype(d64) * wt[..., None]
                sa += np.abs(col[qy, qx].astype(d64)) * wt[..., None]
                sw += wt
            acc[stage] = (sc, sa, sw)
        for stage, sel in ((1, wgt > 0), (2, wgt == 0)):
            sc, sa, sw = acc[stage]
            if sel.any():
                err = np.abs(out[sel].astype(d64) - sc[sel] / sw[sel][:, None]) / (sa[sel] / sw[sel][:, None])
                worst = max(worst, float(err.max()) / 2.0 ** -24)
        assert (wgt > 0).sum() > h * w / 2
    print(f"worst fp32 - fp64 difference: {worst:.2f} x 2^-24 relative")
    assert worst <= 16.0


# ------------------------------------------------------------------------------------------------- real guides

_GUIDES = {}


def _guides(rm, scene, cam, w, h):
    """(the oracle's hit records [h, w, 12] of a seeded camera at w x h, the camera, the median depth of its hits)"""
    if (scene, cam, w, h) not in _GUIDES:
        blob = _base(scene)
        v = _cams(rm, scene)[cam]
        rec = THR._helper()(blob, rm.view_rays(v, w, h, blob, 0)).reshape(h, w, 12)
        t = rec[..., 3][rec.view(np.int32)[..., 7] >= 0]
        _GUIDES[scene, cam, w, h] = (rec, v, float(np.median(t)))
    return _GUIDES[scene, cam, w, h]


def _sigma_z(v, depth, s):
    """two coarse footprints at the median depth"""
    return float(F(2.0 * s * float(np.linalg.norm(v[8:11].astype(np.float64))) * depth))


@pytest.mark.parametrize("size", REAL_SIZES[:2])
def test_real_guides_reach_every_stage(rays_mod, size):
    """the oracle's hit records of seeded camera 0 of demo02 at 64x64 and 67x45, factors 2, 3 and 4, NORMAL at normal_sq 7 and
    PLANE at two coarse footprints, with and without SAME_ID: stage 1, stage 2 and stage 3 each occur in every configuration
    (these cameras are the GPU tests' inputs); one configuration against the scalar text at every pixel.  Camera 1 supplies
    real miss / hit borders: some hundreds of miss pixels, and pixels on either side that lose the taps across the border"""
    rm = rays_mod
    w, h = size
    rec, v, depth = _guides(rm, GUIDE_SCENE, 0, w, h)
    for s in (2, 3, 4):
        col, var = _coarse(rm, h, w, s, (0, 0), s)
        for same in (False, True):
            kw = dict(flags=NORMAL | PLANE | (SAME_ID if same else 0), normal_sq=7, sigma_z=_sigma_z(v, depth, s))
            _, _, wgt = rm.upsample_pass(col, var, rec, s, **kw)
            n = _stage_counts(wgt)
            print(f"{w}x{h} factor {s} same_id {same}: stages {n}")
            assert min(n) > 0 and sum(n) == w * h, n
            if s == 3 and same:
                _against_scalar(rm, col, var, rec, s, (0, 0), f"{w}x{h} real guides", **kw)
    rec1, v1, d1 = _guides(rm, GUIDE_SCENE, 1, w, h)
    miss = rec1.view(np.int32)[..., 7] < 0
    assert 100 <= miss.sum() <= 2000, int(miss.sum())
    col, var = _coarse(rm, h, w, 4, (1, 1), 9)
    _, _, wgt = rm.upsample_pass(col, var, rec1, 4, (1, 1), flags=NORMAL | PLANE, normal_sq=7, sigma_z=_sigma_z(v1, d1, 4))
    hit_lattice = ~miss[1::4, 1::4]
    assert hit_lattice.any() and (~hit_lattice).any(), "lattice points on both sides of the border"
    assert (wgt[miss] == 1).any() and ((wgt[miss] > 0) & (wgt[miss] < 1)).any(), "misses served by miss taps alone, some by fewer than four"
    assert ((wgt[~miss] > 0) & (wgt[~miss] < 0.5)).any(), "hits beside the border lose their miss taps"


# ------------------------------------------------------------------------------------------------- refusals without a device

def test_specification_refuses(rays_mod):
    rm = rays_mod
    h, w, s = 6, 7, 2
    col, var = _coarse(rm, h, w, s, (0, 0), 1)
    rec = _flat(h, w)
    ok = rm.upsample_pass
    ok(col, var, rec, s)
    for bad in (dict(factor=0), dict(factor=17), dict(phase=(2, 0)), dict(phase=(0, -1)), dict(normal_sq=8), dict(normal_sq=-1),
                dict(flags=32), dict(sigma_z=0.0), dict(sigma_z=np.nan), dict(alb_floor=0.0), dict(alb_floor=-1.0)):
        with pytest.raises(ValueError):
            ok(col, var, rec, **dict(dict(factor=s), **bad))
    for c, v, r in ((col.astype(np.float64), var, rec), (col[..., :2], var, rec), (col[:-1], var, rec), (col, var[:-1], rec),
                    (col, var.astype(np.float64), rec), (col, var, rec[..., :11]), (col, var, rec.astype(np.float64)),
                    (np.zeros((h, w, 3), dtype=F), None, rec)):
        with pytest.raises(ValueError):
            ok(c, v, r, s)
    S = rm.upsample_stops
    assert S() == (NORMAL, 7, F(1), F(1 / 256))
    assert S(normal_power=None, plane=0.25, same_id=True, demodulate=True, modulate=True, albedo_floor=0.5) == (PLANE | SAME_ID | DEMOD | MOD, 0, F(0.25), F(0.5))
    assert [S(normal_power=p)[1] for p in (1, 2, 4, 8, 16, 32, 64, 128)] == list(range(8))
    assert all(isinstance(x, np.float32) for x in S(plane=2)[2:])
    for bad in (dict(normal_power=0), dict(normal_power=3), dict(normal_power=256), dict(normal_power=2.0), dict(normal_power=True),
                dict(plane=0), dict(plane=-1.0), dict(plane=np.nan), dict(plane=np.inf), dict(plane="x"), dict(albedo_floor=0.0),
                dict(albedo_floor=-1), dict(albedo_floor=np.nan), dict(albedo_floor=None), dict(same_id=1), dict(demodulate="yes"),
                dict(modulate=None)):
        with pytest.raises(ValueError):
            S(**bad)
    with pytest.raises(TypeError):
        S(luma=1.0)


def test_python_refusals_without_a_gpu(qr):
    """what Scene.upsample refuses before anything reaches the library or the device: ValueError.  The scene is a shell without a
    handle; every tensor is on the CPU, which is 'another device' and the last thing checked"""
    import torch
    me = object.__new__(qr.Scene)
    me._h, me.device = ctypes.c_void_p(), 0
    n, h, w, s = 2, 5, 6, 2
    hits, col, var = torch.zeros((n, h, w, 12)), torch.zeros((n, 3, 3, 3)), torch.zeros((n, 3, 3))
    with pytest.raises(ValueError, match="on cuda:0"):
        me.upsample(col, hits, s, variance=var)
    with pytest.raises(ValueError, match="on cuda:0"):
        me.upsample(torch.zeros((n, 2, 3, 4)), hits, s, (1, 1))
    for kw in (dict(normal_power=3), dict(normal_power=256), dict(normal_power=1.0), dict(plane=0.0), dict(plane=float("nan")),
               dict(albedo_floor=0.0), dict(albedo_floor="a"), dict(same_id=2), dict(demodulate=None), dict(modulate="x")):
        with pytest.raises(ValueError, match="must be"):
            me.upsample(col, hits, s, **kw)
    for factor in (0, 17, 1.5, True, None):
        with pytest.raises(ValueError, match="factor must be"):
            me.upsample(col, hits, factor)
    for phase in ((2, 0), (0, 2), (-1, 0), (0, 0, 0), 1, (0.5, 0), None):
        with pytest.raises(ValueError, match="phase must be"):
            me.upsample(col, hits, s, phase)
    with pytest.raises(ValueError, match="empty"):
        me.upsample(col, torch.zeros((n, 1, 6, 12)), 2, (0, 1))
    for bad in (hits.double(), hits[..., :11], hits[0], hits.numpy(), torch.zeros((0, h, w, 12)), None):
        with pytest.raises(ValueError, match="hits must be"):
            me.upsample(col, bad, s)
    for bad in (col.double(), col[..., :2], torch.zeros((n, 3, 3, 5)), col[0], col.numpy(), torch.zeros((n, 2, 3, 3)),
                torch.zeros((n, h, w, 3)), col[:1], None):
        with pytest.raises(ValueError, match="colour_lo must be"):
            me.upsample(bad, hits, s)
    with pytest.raises(ValueError, match="colour_lo must be"):
        me.upsample(col, hits, s, (1, 1))                   # the coarse frame of phase (1, 1) is 2 x 3
    for bad in (var.double(), var[:1], var[..., None], var.numpy(), torch.zeros((n, h, w))):
        with pytest.raises(ValueError, match="variance must be"):
            me.upsample(col, hits, s, variance=bad)
    for bad in (col, torch.zeros((n, h, w, 4)), torch.zeros((n, h, w, 3)).double(), torch.zeros((1, h, w, 3))):
        with pytest.raises(ValueError, match="out must be"):
            me.upsample(col, hits, s, out=bad)
    with pytest.raises(ValueError, match="variance_out needs a variance"):
        me.upsample(col, hits, s, variance_out=torch.zeros((n, h, w)))
    for bad in (var, torch.zeros((n, h, w)).double()):
        with pytest.raises(ValueError, match="variance_out must be"):
            me.upsample(col, hits, s, variance=var, variance_out=bad)
    for bad in (var, torch.zeros((n, h, w)).double(), 1, "yes"):
        with pytest.raises(ValueError, match="weight must be"):
            me.upsample(col, hits, s, weight=bad)
    with pytest.raises(ValueError, match="contiguous"):
        me.upsample(torch.zeros((n, 3, 3, 6))[..., ::2], hits, s)


# ---------------------------------------------------------------------------------------------------------------- GPU

def _params(qr, s, ph, ch, kw):
    return qr.UpsampleParams(s, ph[0], ph[1], ch, kw.get("normal_sq", 0), kw.get("flags", 0), kw.get("sigma_z", 1.0),
                             kw.get("alb_floor", 1 / 256))


def _off16(scn, a):
    """a device copy of a float array that sits 4 bytes off a 16-byte boundary"""
    import torch
    a = np.ascontiguousarray(a)
    whole = torch.empty((a.size + 1,), dtype=torch.float32, device=f"cuda:{scn.device}")
    assert whole.data_ptr() % 16 == 0
    body = whole[1:].view(a.shape)
    body.copy_(torch.from_numpy(a))
    return body


def _call_gpu(qr, rm, scn, col, var, rec, s, ph, kw, where, weight=True, stream=None):
    """one qr_upsample_views_async call through ctypes -- the float inputs and outputs 4 bytes off a 16-byte boundary, the outputs
    NaN-filled between sentinels -- compared with upsample_pass on the same host arrays: every word of every output that is
    given, the sentinels intact.  Returns (colour, variance or None, weight or None) as numpy"""
    import torch
    n, h, w = rec.shape[:3]
    ch = col.shape[-1]
    cd, hd = _off16(scn, col), _dev(scn, rec)
    vd = None if var is None else _off16(scn, var)
    shapes = [(n, h, w, ch), (n, h, w), (n, h, w)]
    given = [True, var is not None, weight]
    bufs = [_buffer(scn, sh, float("nan"), 1) if g else (None, None) for sh, g in zip(shapes, given)]
    vp = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())
    cp = _params(qr, s, ph, ch, kw)
    st = torch.cuda.current_stream() if stream is None else stream
    rc = qr.lib().qr_upsample_views_async(scn._h, vp(cd), vp(vd), vp(hd), n, w, h, ctypes.byref(cp), *(vp(b[1]) for b in bufs),
                                          ctypes.c_void_p(st.cuda_stream))
    assert rc == 0, f"{where}: {qr.lib().qr_last_error().decode()}"
    st.synchronize()
    want = rm.upsample_pass(col, var, rec, s, ph, **kw)
    got = []
    for k, (whole, body) in enumerate(bufs):
        if whole is None:
            got.append(None)
            continue
        g = _host(whole)
        size = int(np.prod(shapes[k]))
        assert (g[1 + size:] == SENTINEL).all() and (g[:1] == SENTINEL).all(), f"{where}: output {k} was written outside"
        got.append(g[1:1 + size].reshape(shapes[k]))
        _same(got[k], want[k], f"{where} output {k}")
    return got


def _configs(sigma_z):
    """each stop alone, all stops and none; normal_sq 0, 3 and 7; with and without de/modulation"""
    full = dict(normal_sq=3, sigma_z=sigma_z, alb_floor=1 / 64)
    return [dict(full, flags=31), dict(full, flags=NORMAL), dict(full, flags=PLANE), dict(full, flags=SAME_ID), dict(flags=0),
            dict(full, flags=NORMAL | PLANE | SAME_ID, normal_sq=0), dict(full, flags=NORMAL | PLANE | DEMOD, normal_sq=7),
            dict(full, flags=NORMAL | MOD, normal_sq=7)]


_REAL = {}


def _real(qr, rm, scene, cam, w, h):
    """(scene, view, hits on the device, hits on the host, the median depth): view_hits of a seeded camera, computed once"""
    if (scene, cam, w, h) not in _REAL:
        scn = qr.Scene(_base(scene), ray_queries=True)
        scn.set_pt(False)
        v = np.array(_cams(rm, scene)[cam], dtype=F)
        hd = scn.view_hits(TPV._vt(scn, [v]), w, h)
        hits = _host(hd)
        ids = hits.view(np.int32)[..., 7]
        assert (ids >= 0).any()
        _REAL[scene, cam, w, h] = (scn, v, hd, hits, float(np.median(hits[..., 3][ids >= 0])))
    return _REAL[scene, cam, w, h]


def _coarse_light(rm, scn, v, hd, s, ph, w, h):
    """the coarse light of one lattice, made the two ways the feature is for: a spun framed 4-direction gather on coarse_hits (4
    channels) and 6 adaptive path-traced samples on coarse_view with variance() (3 channels); host arrays"""
    import torch
    wl, hl = rm.coarse_size(w, h, s, ph)
    ch_d = rm.coarse_hits(hd, s, ph)
    assert tuple(ch_d.shape) == (1, hl, wl, 12) and ch_d.is_contiguous()
    spin = torch.from_numpy(rm.spins((1, hl, wl), 7)).to(hd.device)
    dirs = torch.from_numpy(rm.cosine_dirs(4)).to(hd.device)
    gat, _ = scn.hit_gather(ch_d, dirs, eps=TA.EPS, reach=TA.REACH, frame=True, spin=spin)
    acc = scn.pt_adaptive_views(TPV._vt(scn, [rm.coarse_view(v, s, ph)]), wl, hl, min_samples=2, max_samples=64, tol=0.05)
    _, mean = acc.step(6, mean=True)
    var = acc.variance()
    gat, mean, var = _host(gat), _host(mean), _host(var)
    assert gat.shape == (1, hl, wl, 4) and mean.shape == (1, hl, wl, 3) and var.shape == (1, hl, wl)
    assert np.isfinite(gat).all() and np.isfinite(mean).all()
    return gat, mean, var


@pytest.mark.gpu
@pytest.mark.parametrize("size", REAL_SIZES)
@pytest.mark.parametrize("scene,cam", REAL_INPUTS)
def test_gpu_real_inputs(qr, rays_mod, scene, cam, size):
    """view_hits of a seeded camera; per factor (1, 2, 3, 4, 8, 16; at 16, 9x130 has a coarse frame one pixel wide) and phase
    ((0, 0), (1, 1), (s - 1, 0)) the coarse light from hit_gather on coarse_hits and from pt_adaptive_views on coarse_view; every
    lattice with all flags in both channel counts with variance and weight, and with two more of the stop sets, so that each
    stop alone, all, none, normal_sq 0, 3, 7, with and without variance, weight and de/modulation all occur at every size"""
    rm = rays_mod
    w, h = size
    scn, v, hd, hits, depth = _real(qr, rm, scene, cam, w, h)
    if (scene, cam) == REAL_INPUTS[0] and size != (9, 130):
        want = _guides(rm, scene, cam, w, h)[0].view(np.int32)[..., 7]
        assert (hits[0].view(np.int32)[..., 7] == want).all(), "the device's records are the ones the CPU test judged"
    k, stages = 0, np.zeros(3, dtype=np.int64)
    for s in FACTORS:
        cfgs = _configs(_sigma_z(v, depth, s))
        for ph in _phases(s, w, h):
            gat, mean, var = _coarse_light(rm, scn, v, hd, s, ph, w, h)
            where = f"{scene} camera {cam} {w}x{h} factor {s} phase {ph}"
            got = _call_gpu(qr, rm, scn, mean, var, hits, s, ph, cfgs[0], where + " all flags, 3 channels")
            _call_gpu(qr, rm, scn, gat, var, hits, s, ph, dict(cfgs[0], normal_sq=7), where + " all flags, 4 channels")
            stages += _stage_counts(rm.upsample_pass(mean, var, hits, s, ph, **dict(cfgs[0], flags=NORMAL | PLANE, normal_sq=7))[2])
            for j in (1 + k % 7, 1 + (k + 3) % 7):
                four, with_var, with_w = (k + j) % 2 == 0, (k + j) % 3 != 0, j % 2 == 1
                _call_gpu(qr, rm, scn, gat if four else mean, var if with_var else None, hits, s, ph, cfgs[j],
                          where + f" {cfgs[j]} four {four} variance {with_var} weight {with_w}", with_w)
            k += 1
    if (scene, cam) == REAL_INPUTS[0] and size != (9, 130):
        assert (stages > 0).all(), stages.tolist()


def _synthetic(w, h, seed):
    """two views of random records: two tilted surfaces, random ids among 2, 5, 6 and misses, NaN, Inf and -0.0 in pos, nrm and
    alb"""
    rng = np.random.default_rng(seed)
    recs = []
    for j in range(2):
        _, _, r = TA._random_frame(h, w, seed + j)
        ids = r.view(np.int32)[..., 7]
        pick = rng.uniform(size=(h, w)) < 0.3
        ids[pick] = rng.choice(np.array([2, 5, 6, -1], dtype=np.int32), (h, w))[pick]
        for word in (0, 1, 2, 4, 5, 6, 8, 9, 10):
            for val in (np.nan, np.inf, -np.inf, -0.0):
                r[..., word] = np.where(rng.uniform(size=(h, w)) < 0.01, F(val), r[..., word])
        recs.append(r)
    return np.stack(recs)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SYNTH_SIZES)
def test_gpu_synthetic_inputs(qr, rays_mod, size):
    """hand-made records with NaN, Inf, -0.0 and random ids at 1x1, 9x130, 67x45 and 33x9 (one tile plus one pixel each way:
    every tile-edge case of the staging), every factor and phase the frame has, two views, 3 and 4 channels; NaN-filled,
    sentinel-tailed buffers whose float planes sit 4 bytes off a 16-byte boundary"""
    w, h = size
    rm = rays_mod
    scn = qr.Scene(_base("patched:demo01_160"))          # any scene, any mode, no ray-query list
    try:
        rec = _synthetic(w, h, 17 * w + h)
        stages, k = np.zeros(3, dtype=np.int64), 0
        for s in FACTORS:
            phases = _phases(s, w, h) + ([(s // 2, s - 1)] if s > 2 and s // 2 < w and s - 1 < h else [])
            for ph in phases:
                wl, hl = rm.coarse_size(w, h, s, ph)
                rng = np.random.default_rng(k)
                cfgs = _configs(0.5)
                for ch in (3, 4):
                    col = rng.uniform(0.0, 1.0, (2, hl, wl, ch)).astype(F)
                    var = rng.uniform(0.0, 0.1, (2, hl, wl)).astype(F)
                    where = f"synthetic {w}x{h} factor {s} phase {ph} ch {ch}"
                    got = _call_gpu(qr, rm, scn, col, var, rec, s, ph, cfgs[0], where + " all flags")
                    stages += _stage_counts(got[2])
                    j = 1 + (k + ch) % 7
                    _call_gpu(qr, rm, scn, col, var if ch == 3 else None, rec, s, ph, cfgs[j], where + f" {cfgs[j]}", weight=ch == 4)
                k += 1
        assert (stages > 0).all() or w * h == 1, stages.tolist()
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_views_are_independent(qr, rays_mod):
    """a view alone and as view 2 of 3 give the same bits; the same call twice and a call on a side stream behind an event give
    the same bytes; Scene.upsample is the C call, with out= tensors and each combination of optional outputs"""
    import torch
    rm = rays_mod
    w, h, s, ph = 67, 45, 3, (1, 1)
    scn, v, hd, hits, depth = _real(qr, rm, GUIDE_SCENE, 0, w, h)
    gat, mean, var = _coarse_light(rm, scn, v, hd, s, ph, w, h)
    rec3 = np.concatenate([_synthetic(w, h, 5)[:1], hits, _synthetic(w, h, 6)[:1]])
    rng = np.random.default_rng(3)
    col3 = np.concatenate([rng.uniform(0, 1, mean.shape).astype(F), mean, rng.uniform(0, 1, mean.shape).astype(F)])
    var3 = np.concatenate([var * F(2), var, var * F(0.5)])
    sz = _sigma_z(v, depth, s)
    kw = dict(flags=NORMAL | PLANE | DEMOD | MOD, normal_sq=7, sigma_z=sz, alb_floor=1 / 256)
    three = _call_gpu(qr, rm, scn, col3, var3, rec3, s, ph, kw, "three views")
    alone = _call_gpu(qr, rm, scn, mean, var, hits, s, ph, kw, "view 1 alone")
    for a, b in zip(alone, three):
        _same(a[0], b[1], "a view alone and as view 2 of 3")
    cd, vd, rd = _dev(scn, col3), _dev(scn, var3), _dev(scn, rec3)
    args = dict(normal_power=128, plane=sz, demodulate=True, modulate=True)
    a = scn.upsample(cd, rd, s, ph, variance=vd, weight=True, **args)
    b = scn.upsample(cd, rd, s, ph, variance=vd, weight=True, **args)
    assert len(a) == 3 and tuple(a[0].shape) == (3, h, w, 3) and tuple(a[1].shape) == tuple(a[2].shape) == (3, h, w)
    for k in range(3):
        _same(_host(a[k]), three[k], "Scene.upsample is the C call")
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), "the same call twice"
    only = scn.upsample(cd, rd, s, ph, **args)
    assert isinstance(only, torch.Tensor) and torch.equal(only.view(torch.int32), a[0].view(torch.int32))
    two = scn.upsample(cd, rd, s, ph, weight=True, **args)
    assert len(two) == 2 and torch.equal(two[1].view(torch.int32), a[2].view(torch.int32))
    two = scn.upsample(cd, rd, s, ph, variance=vd, **args)
    assert len(two) == 2 and torch.equal(two[1].view(torch.int32), a[1].view(torch.int32))
    out, vout, wout = torch.empty_like(a[0]), torch.empty_like(a[1]), torch.empty_like(a[2])
    got = scn.upsample(cd, rd, s, ph, variance=vd, out=out, variance_out=vout, weight=wout, **args)
    assert got[0] is out and got[1] is vout and got[2] is wout
    for k in range(3):
        assert torch.equal(got[k].view(torch.int32), a[k].view(torch.int32)), "out= tensors"
    side, ready, done = torch.cuda.Stream(), torch.cuda.Event(), torch.cuda.Event()
    c2 = cd.clone()
    ready.record()
    side.wait_event(ready)
    u = scn.upsample(c2, rd, s, ph, variance=vd, weight=True, stream=side, **args)
    done.record(side)
    torch.cuda.current_stream().wait_event(done)
    for k in range(3):
        assert torch.equal(u[k].view(torch.int32), a[k].view(torch.int32)), "a side stream"
    side.synchronize()
    with pytest.raises(ValueError, match="out must be"):
        scn.upsample(cd, rd, s, ph, out=out[:1], **args)
    with pytest.raises(qr.QrError, match="cannot be an input"):
        scn.upsample(cd, rd, s, ph, weight=rd.view(-1)[:3 * h * w].view(3, h, w))        # the weight plane is the records' memory


@pytest.mark.gpu
def test_gpu_refusals(qr, rays_mod):
    """every QR_ERR_ARG through ctypes, the filled outputs untouched after all of them; n_views = 0 is QR_OK; calls at the edge
    of what is allowed are served"""
    import torch
    L = qr.lib()
    scn = qr.Scene(_base("patched:demo01_160"))             # no ray-query list: the call needs none
    dev = f"cuda:{scn.device}"
    n, w, h, s = 2, 9, 7, 2
    z = lambda m: torch.zeros((m + 16,), dtype=torch.float32, device=dev)
    s75 = lambda m: torch.full((m + 16,), 7.5, dtype=torch.float32, device=dev)
    px = n * h * w
    col, var, hits = z(px * 4), z(px), z(px * 12)               # large enough for the coarse frame of factor 1
    cout, vout, wout = s75(px * 4), s75(px), s75(px)
    vp = lambda x, off=0: ctypes.c_void_p(None if x is None else x.data_ptr() + off)
    nan = float("nan")

    def call(sc=scn._h, ci=vp(col), vi=vp(var), hi=vp(hits), n=n, w=w, h=h, co=vp(cout), vo=vp(vout), wo=vp(wout), null_p=False,
             factor=s, phase=(0, 0), channels=3, **kw):
        p = _params(qr, factor, phase, channels, kw)
        return L.qr_upsample_views_async(sc, ci, vi, hi, n, w, h, None if null_p else ctypes.byref(p), co, vo, wo, None)

    none = vp(None)
    assert call(sc=None) == ARG and call(null_p=True) == ARG
    assert call(ci=none) == ARG and call(hi=none) == ARG and call(co=none) == ARG
    for off in (4, 8, 12):
        assert call(hi=vp(hits, off)) == ARG, "hits are 16-byte aligned"
    for name, buf in (("ci", col), ("vi", var), ("co", cout), ("vo", vout), ("wo", wout)):
        for off in (1, 2, 3):
            assert call(**{name: vp(buf, off)}) == ARG, f"{name} is 4-byte aligned"
    assert call(vi=none) == ARG and call(vo=none) == ARG, "var_lo and var_out go together"
    for o in ("co", "vo", "wo"):
        for i in (col, var, hits):
            assert call(**{o: vp(i)}) == ARG, "an output equal to an input"
    for bad in (0, -1, 17, 1 << 20):
        assert call(factor=bad) == ARG
    for bad in ((2, 0), (0, 2), (-1, 0), (0, -1)):
        assert call(phase=bad) == ARG
    assert call(factor=16, phase=(9, 0)) == ARG and call(factor=16, phase=(0, 7)) == ARG, "a phase beyond the frame"
    assert call(w=1, phase=(1, 0)) == ARG and call(h=1, phase=(0, 1)) == ARG
    assert call(channels=2) == ARG and call(channels=5) == ARG and call(channels=0) == ARG
    assert call(normal_sq=-1) == ARG and call(normal_sq=8) == ARG
    assert call(flags=32) == ARG and call(flags=0x80000000) == ARG and call(flags=63) == ARG
    for name in ("sigma_z", "alb_floor"):
        for bad in (0.0, -1.0, nan, -0.0):
            assert call(**{name: bad}) == ARG, (name, bad)
    assert call(w=0) == ARG and call(h=0) == ARG and call(w=16385) == ARG and call(h=16385) == ARG and call(w=-3) == ARG
    assert call(n=-1) == ARG and call(n=65536) == ARG
    assert call(n=0) == 0 and call(n=0, ci=none, hi=none, co=none) == 0
    torch.cuda.synchronize()
    for t in (cout, vout, wout):
        assert (t == 7.5).all().item(), "a refused call wrote something"
    # served: offsets that keep the alignment, no optional output, four channels, every flag, the limits of the lattice
    assert call() == 0 and call(ci=vp(col, 4), vi=vp(var, 8), co=vp(cout, 12), vo=vp(vout, 4), wo=vp(wout, 4), hi=vp(hits, 48)) == 0
    assert call(vi=none, vo=none, wo=none) == 0 and call(vi=none, vo=none) == 0
    assert call(channels=4, flags=31, normal_sq=7, sigma_z=float("inf"), alb_floor=float("inf")) == 0
    assert call(factor=16, phase=(8, 6)) == 0 and call(factor=1) == 0 and call(factor=2, phase=(1, 1)) == 0
    torch.cuda.synchronize()
    assert (cout[:px * 3] != 7.5).all().item() and (cout[px * 4:] == 7.5).all().item()
    assert (vout[:px] != 7.5).all().item() and (vout[px + 1:] == 7.5).all().item() and (wout[px + 1:] == 7.5).all().item()
    scn.close()


@pytest.mark.gpu
def test_gpu_pipeline_end_to_end(qr, rays_mod):
    """the pipeline the feature exists for, on one scene at 64x64, two frames: view_hits -> hit_gather on coarse_hits at factor 2 ->
    upsample -> Temporal.step -> denoise, against the numpy chain fed the device's hits and coarse gather"""
    import torch
    rm = rays_mod
    w = h = 64
    s, ph = 2, (0, 0)
    cams, off, plane_max = TR._pair(rm, GUIDE_SCENE, w, h)
    scn = qr.Scene(_base(GUIDE_SCENE), ray_queries=True)
    try:
        scn.set_pt(False)
        kw = dict(plane_max=plane_max, off=off, var_min_len=2)
        acc, ref = scn.temporal(1, w, h, 4, **kw), rm.temporal(1, w, h, 4, **kw)
        dirs = torch.from_numpy(rm.cosine_dirs(4)).to(f"cuda:{scn.device}")
        wl, hl = rm.coarse_size(w, h, s, ph)
        flags, nsq, sz, af = rm.upsample_stops(plane=2 * plane_max)
        for k in range(2):
            vt = TPV._vt(scn, [cams[k]])
            hd = scn.view_hits(vt, w, h)
            spin = torch.from_numpy(rm.spins((1, hl, wl), 7 + k)).to(hd.device)
            lo, _ = scn.hit_gather(rm.coarse_hits(hd, s, ph), dirs, eps=TA.EPS, reach=TA.REACH, frame=True, spin=spin, cosine=True)
            up, wgt = scn.upsample(lo, hd, s, ph, plane=2 * plane_max, weight=True)
            col, var = acc.step(up, hd, vt)
            clean, _ = scn.denoise(col, hd, var, passes=2, plane=plane_max, luma=4.0, normal_power=8)
            hits, lo_h = _host(hd), _host(lo)
            want_up, _, want_w = rm.upsample_pass(lo_h, None, hits, s, ph, flags=flags, normal_sq=nsq, sigma_z=sz, alb_floor=af)
            _same(_host(up), want_up, f"frame {k} upsampled"), _same(_host(wgt), want_w, f"frame {k} weight")
            wc, wv = ref.step(want_up, hits, np.stack([cams[k]]))
            _same(_host(col), wc, f"frame {k} accumulated"), _same(_host(var), wv, f"frame {k} variance")
            want_clean, _ = rm.denoise(wc, wv, hits, passes=2, plane=plane_max, luma=4.0, normal_power=8)
            _same(_host(clean), want_clean, f"frame {k} denoised")
        assert (ref.length > 1).any() and (want_w > 0).sum() > w * h / 2
    finally:
        scn.close()


# once more through the guarded diagnostic build (make guard), as tests/test_reproject.py does it: the library is chosen when the
# package is imported, hence the child process: this file run as a script.

def _guard_child():
    from qr_loader import load_package
    qr = load_package()
    assert qr.LIB_PATH == GUARD_LIB, qr.LIB_PATH
    rm = _rays_mod()
    w, h = REAL_SIZES[1]
    scn, v, hd, hits, depth = _real(qr, rm, GUIDE_SCENE, 0, w, h)
    for s, ph in ((1, (0, 0)), (2, (1, 1)), (3, (2, 0)), (16, (1, 1))):
        gat, mean, var = _coarse_light(rm, scn, v, hd, s, ph, w, h)
        cfgs = _configs(_sigma_z(v, depth, s))
        _call_gpu(qr, rm, scn, mean, var, hits, s, ph, cfgs[0], f"guard factor {s} 3 channels")
        _call_gpu(qr, rm, scn, gat, None, hits, s, ph, cfgs[6], f"guard factor {s} 4 channels", weight=False)
    scn.close()
    print(f"{GUIDE_SCENE} guard_ok 1", flush=True)
    return 0


@pytest.mark.gpu
def test_gpu_guarded_build_gives_the_same_frames():
    assert os.path.exists(GUARD_LIB), "libqrhip_guard.so is missing: build() makes it (make -C quadray-engine_amd/csrc guard)"
    env = dict(os.environ, QR_LIB=GUARD_LIB)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-child"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.count("guard_ok 1") == 1 and "QR_GUARD" not in out.stderr, out.stdout + out.stderr[-3000:]


if __name__ == "__main__":
    sys.exit(_guard_child() if "--guard-child" in sys.argv else 2)
