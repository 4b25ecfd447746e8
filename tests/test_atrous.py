"""The guided a-trous filter (include/qrhip.h qr_atrous_views_async, qr_pt_adapt_views_variance_async; Scene.atrous,
Scene.denoise, PtAdaptiveViews.variance; rays.atrous_pass, rays.denoise, rays.pt_adapt_view_variance).

The filter is a pure function of its inputs and its arithmetic is pinned to the operation, so there is no oracle: the CPU tests
check the numpy statement against properties worked out by hand (the exact variance factor of the kernel, misses, what each
stop closes, non-finite guides, a float64 evaluation), the GPU tests check every word the kernel writes against the numpy
statement on the inputs copied back from the device.  Every comparison is bit for bit unless it says otherwise."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import test_pt_views as TPV
from conftest import ROOT
from test_pt_views import _base, _cams, _rays_mod

F = np.float32
ARG = -1
GUARD_LIB = TPV.GUARD_LIB
ASM = TPV.ASM
NORMAL, PLANE, LUMA, DEMOD, MOD = 1, 2, 4, 8, 16
REAL_SCENES = ["patched:demo02_160_gf_aa4", "pt:test18_160_pt"]
STEPS = [1, 2, 4, 8, 16, 64]
SIZES = [(1, 1), (9, 130), (67, 45)]                    # (w, h)
EPS, REACH = 1e-3, 2.0                                  # of the 4-channel input's gather fan
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def rays_mod():
    return _rays_mod()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _flat(h, w, nrm=(0.0, 0.0, 1.0), sid=2, alb=0.5):
    """records of a flat guide: pos = (x, y, 0), one normal, one id"""
    r = np.zeros((h, w, 12), dtype=F)
    ys, xs = np.mgrid[0:h, 0:w]
    r[..., 0], r[..., 1] = xs, ys
    r[..., 3] = 1.0
    r[..., 4:7] = nrm
    r[..., 8:11] = alb
    r.view(np.int32)[..., 7] = sid
    r.view(np.int32)[..., 11] = 0
    return r


def _random_frame(h, w, seed, ch=3):
    """a random frame with everything a stop looks at: two tilted surfaces and a strip of misses, noisy colour, a variance"""
    rng = np.random.default_rng(seed)
    r = _flat(h, w)
    n = rng.normal(0.0, 0.15, (h, w, 3)).astype(F) + np.array([0, 0, 1], dtype=F)
    n[:, w // 2:] = rng.normal(0.0, 0.15, (h, w - w // 2, 3)).astype(F) + np.array([0.6, 0, 0.8], dtype=F)
    r[..., 4:7] = n / np.sqrt((n * n).sum(-1, keepdims=True)).astype(F)
    r[..., 2] = rng.normal(0.0, 0.3, (h, w)).astype(F)
    r[..., 8:11] = rng.uniform(0.0, 1.0, (h, w, 3)).astype(F)
    ids = r.view(np.int32)[..., 7]
    ids[:, w // 2:] = 5
    ids[rng.uniform(size=(h, w)) < 0.08] = -1
    col = rng.uniform(0.0, 1.0, (h, w, ch)).astype(F)
    var = rng.uniform(0.001, 0.05, (h, w)).astype(F)
    return col, var, r


ALL_STOPS = dict(flags=NORMAL | PLANE | LUMA, normal_sq=3, sigma_z=0.5, sigma_l2=4.0, eps_l=1e-6)


# ------------------------------------------------------------------------------------------------- names and constants

def test_symbols_constants_and_header(qr, rays_mod):
    hdr = open(os.path.join(ROOT, "include", "qrhip.h")).read()
    for sym in ("qr_atrous_views_async", "qr_pt_adapt_views_variance_async"):
        assert sym in qr.ABI_SYMBOLS and sym + "(" in hdr
        assert hasattr(qr.lib(), sym)
    assert ctypes.sizeof(qr.AtrousParams) == 32
    for name, val in (("NORMAL", 1), ("PLANE", 2), ("LUMA", 4), ("DEMODULATE", 8), ("MODULATE", 16), ("MAX_STEP", 64)):
        assert getattr(qr, "ATROUS_" + name) == val == getattr(rays_mod, "ATROUS_" + name)
        assert f"QR_ATROUS_{name}" in hdr
    assert rays_mod.ATROUS_H.dtype == np.float32 and float(rays_mod.ATROUS_H.sum()) == 1.0
    for m in ("atrous", "denoise"):
        assert callable(getattr(qr.Scene, m))
    assert callable(qr.PtAdaptiveViews.variance)


def test_kernels_in_resource_check():
    """the three new kernels are held to a budget by the build's own check, and the build's assembly meets it"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import check_kernel_resources as ck
    finally:
        sys.path.pop(0)
    for frag in ("16qr_atrous_kernelILi3EE", "16qr_atrous_kernelILi4EE", "22qr_pt_adapt_var_kernel"):
        assert ck.LIMITS[frag] == (64, 0, 0)
    if os.path.exists(ASM):
        ks = {k["name"]: k for k in ck.kernels(ASM)}
        mine = [k for n, k in ks.items() if "qr_atrous_kernel" in n or "qr_pt_adapt_var_kernel" in n]
        assert len(mine) == 3
        for k in mine:
            assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0 and k["vgpr_count"] <= 64
            assert k["group_segment_fixed_size"] <= 22464


# ------------------------------------------------------------------------------------------------- the numpy statement

@pytest.mark.parametrize("step", [1, 3])
def test_variance_factor_on_a_flat_guide(rays_mod, step):
    """no stops, a flat guide, a constant variance that is a power of two (every product and sum below is then exact): an
    interior pixel's variance falls by exactly float32((70/256)^2) per pass, a corner pixel's by the surviving 3 x 3 taps"""
    h, w = 8 * step + 5, 9 * step + 5
    rng = np.random.default_rng(3)
    col = rng.uniform(0, 1, (h, w, 3)).astype(F)
    var = np.full((h, w), 0.25, dtype=F)
    out, vout = rays_mod.atrous_pass(col, var, _flat(h, w), step)
    assert out.dtype == np.float32 and vout.dtype == np.float32 and out.shape == col.shape and vout.shape == var.shape
    factor = F((70 / 256) ** 2)
    assert float(factor) == (70 / 256) ** 2, "4900 / 65536 is a float32"
    inner = vout[2 * step:h - 2 * step, 2 * step:w - 2 * step]
    assert inner.size > 0 and (_bits(inner) == _bits(F(0.25) * factor)).all()
    H = rays_mod.ATROUS_H
    sw, sv = F(0), F(0)
    for dy in range(0, 3):
        for dx in range(0, 3):
            wt = H[dy + 2] * H[dx + 2]
            sw, sv = sw + wt, sv + F(0.25) * (wt * wt)
    want = sv / (sw * sw)
    assert abs(float(want) / 0.25 - (53 / 256) ** 2 / (11 / 16) ** 4) < 1e-7
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        assert _bits(vout[y, x]) == _bits(want), (y, x)
    # a second pass divides the interior again
    out2, vout2 = rays_mod.atrous_pass(out, vout, _flat(h, w), step)
    deep = vout2[4 * step:h - 4 * step, 4 * step:w - 4 * step]
    assert deep.size > 0 and (_bits(deep) == _bits(F(0.25) * factor * factor)).all()
    # and a constant colour stays what it was: the weights sum to 1 exactly in the interior
    flat, _ = rays_mod.atrous_pass(np.full((h, w, 3), 0.3, dtype=F), var, _flat(h, w), step)
    assert (_bits(flat[2 * step:h - 2 * step, 2 * step:w - 2 * step]) == _bits(F(0.3))).all()


@pytest.mark.parametrize("stops", [dict(), ALL_STOPS])
@pytest.mark.parametrize("ch", [3, 4])
def test_a_miss_passes_through_and_is_never_a_tap(rays_mod, stops, ch):
    col, var, rec = _random_frame(21, 19, 5, ch)
    miss = rec.view(np.int32)[..., 7] < 0
    assert 5 < miss.sum() < miss.size // 2
    for step in (1, 2):
        out, vout = rays_mod.atrous_pass(col, var, rec, step, **stops)
        assert (_bits(out[miss]) == _bits(col[miss])).all() and (_bits(vout[miss]) == _bits(var[miss])).all()
        col2, var2 = col.copy(), var.copy()
        col2[miss] += 7.0
        var2[miss] = 3.0
        out2, vout2 = rays_mod.atrous_pass(col2, var2, rec, step, **stops)
        assert (_bits(out2[~miss]) == _bits(out[~miss])).all() and (_bits(vout2[~miss]) == _bits(vout[~miss])).all()
        assert (out[~miss] != col[~miss]).any()
        # without a variance plane nothing comes back for it, and the colours are those of v = 1
        o3, v3 = rays_mod.atrous_pass(col, None, rec, step, **stops)
        o4, _ = rays_mod.atrous_pass(col, np.ones_like(var), rec, step, **stops)
        assert v3 is None and (_bits(o3) == _bits(o4)).all()


def _halves(stop, h=12, w=80, split=40, seed=9):
    """two half-frames that the stop separates: (colour, variance, records, pass arguments).  NORMAL: perpendicular normals.
    PLANE: two parallel planes 10 sigma_z apart.  LUMA: a step edge of 100 standard deviations"""
    rng = np.random.default_rng(seed)
    rec = _flat(h, w)
    sd = F(0.01)
    col = (F(0.5) + rng.normal(0, float(sd), (h, w, 3))).astype(F)
    var = np.full((h, w), sd * sd, dtype=F)
    if stop == NORMAL:
        rec[:, split:, 4:7] = (1.0, 0.0, 0.0)
        kw = dict(flags=NORMAL, normal_sq=7)
    elif stop == PLANE:
        rec[:, split:, 2] = 5.0                         # the planes z = 0 and z = 5 = 10 * sigma_z, normal +z
        kw = dict(flags=PLANE, sigma_z=0.5)
    else:
        col[:, split:] += F(100) * sd
        kw = dict(flags=LUMA, sigma_l2=1.0, eps_l=1e-12)
    return col, var, rec, kw


@pytest.mark.parametrize("step", [1, 2, 16])
def test_the_normal_stop_separates_two_half_frames_bit_for_bit(rays_mod, step):
    """perpendicular normals: the dot is 0, the weight is 0 and the tap is not taken, so changing one side's colours leaves every
    bit of the other side; without the stop the other side does change"""
    col, var, rec, kw = _halves(NORMAL)
    col2 = col.copy()
    col2[:, 40:] += 5.0
    a, av = rays_mod.atrous_pass(col, var, rec, step, **kw)
    b, bv = rays_mod.atrous_pass(col2, var, rec, step, **kw)
    assert (_bits(a[:, :40]) == _bits(b[:, :40])).all() and (_bits(av) == _bits(bv)).all()
    assert (a[:, 40:] != b[:, 40:]).all()
    c, _ = rays_mod.atrous_pass(col, var, rec, step)
    d, _ = rays_mod.atrous_pass(col2, var, rec, step)
    near = slice(max(0, 40 - 2 * step), 40)
    assert (c[:, near] != d[:, near]).all(), "without the stop the neighbours across the edge are read"
    assert (_bits(c[:, :near.start]) == _bits(d[:, :near.start])).all(), "... and nothing further than two taps"


@pytest.mark.parametrize("step", [1, 2, 16])
@pytest.mark.parametrize("stop", [PLANE, LUMA])
def test_the_rational_stops_hold_the_other_side_below_a_hundredth(rays_mod, stop, step):
    """PLANE with two parallel planes 10 sigma_z apart, LUMA with a step edge of 100 standard deviations.  A rational stop is never
    0 at a finite distance, so the other side's bits do move; what the stop guarantees is the weight: 1 / (1 + 10^2) < 1/100 of
    the tap's kernel weight (LUMA: 1 / (1 + 100^2 / ~1), far below).  Asserted on the weights themselves, and on the effect: a
    change of D on one side moves the other side by at most D * (weight across the edge / weight taken) -- against nearly
    D * 5/16 without the stop.  At an infinite distance the plane stop is 0 and the sides' bits are independent."""
    col, var, rec, kw = _halves(stop)
    D = F(0.25)
    col2 = col.copy()
    col2[:, 40:] += D
    ws = []
    a, _ = rays_mod.atrous_pass(col, var, rec, step, weights=ws, **kw)
    b, _ = rays_mod.atrous_pass(col2, var, rec, step, **kw)
    assert len(ws) == 25
    H = rays_mod.ATROUS_H
    cross = np.zeros(col.shape[:2], dtype=np.float64)
    total = np.zeros(col.shape[:2], dtype=np.float64)
    k = 0
    xs = np.arange(col.shape[1])[None, :]
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            take, wt = ws[k]
            take, wt = take[0], wt[0]
            k += 1
            over = take & (xs < 40) & (xs + dx * step >= 40)
            assert (wt[over] < H[dy + 2] * H[dx + 2] / F(100)).all()
            cross += np.where(over, wt, 0)
            total += wt
    left = slice(max(0, 40 - 2 * step), 40)
    assert (cross[:, left] > 0).any(), "the taps across the edge are open, only weak"
    moved = np.abs(b.astype(np.float64) - a)[:, :40]
    bound = (float(D) * cross / total * (1 + 1e-3) + 4 * 2.0 ** -24)[:, :40]
    assert (moved <= bound[..., None]).all() and moved.max() < float(D) / 100
    c, _ = rays_mod.atrous_pass(col, var, rec, step)
    d, _ = rays_mod.atrous_pass(col2, var, rec, step)
    assert np.abs(d - c)[:, left].max() > float(D) / 20, "without the stop the edge bleeds"
    if stop == PLANE:
        rec[:, 40:, 2] = np.inf
        a, _ = rays_mod.atrous_pass(col, var, rec, step, **kw)
        b, _ = rays_mod.atrous_pass(col2, var, rec, step, **kw)
        assert (_bits(a[:, :40]) == _bits(b[:, :40])).all() and np.isfinite(a).all()


def _hand_made(h=14, w=13):
    """finite colours on records and variances made to break a filter: NaN and zero normals, infinite positions, negative, NaN
    and zero variances, normals at a dot of 0.3, zero and NaN albedo, misses"""
    rng = np.random.default_rng(21)
    rec = _flat(h, w)
    col = rng.uniform(0.05, 1.0, (h, w, 3)).astype(F)
    var = np.full((h, w), 0.01, dtype=F)
    rec[1, 1, 4:7] = np.nan
    rec[1, 5, 4] = np.nan
    rec[2, 8, 4:7] = 0.0
    rec[3, 3, 0:3] = np.inf
    rec[3, 9, 2] = -np.inf
    rec[5, 5, 0] = np.nan
    var[6, 2] = -0.5
    var[6, 9] = np.nan
    var[8, 4] = 0.0
    var[8, 5] = 0.0
    col[8, 5] = col[8, 4]                               # a tap at distance 0 in luminance from a pixel of variance 0
    th = np.arccos(F(0.3))
    rec[10:, :, 4:7] = (np.sin(th), 0.0, np.cos(th))    # the bottom rows: n . n' = 0.3 against the rest
    rec[4, 11, 8:11] = 0.0
    rec[5, 11, 8:11] = np.nan
    rec[6, 11, 8:11] = (-1.0, 2.0, 1e-30)
    rec.view(np.int32)[0, 7:9, 7] = -1
    rec.view(np.int32)[12, 0, 7] = -1
    return col, var, rec


HAND_CASES = [dict(flags=NORMAL | PLANE | LUMA, normal_sq=7, sigma_z=0.5, sigma_l2=4.0, eps_l=1e-30),
              dict(flags=NORMAL, normal_sq=6), dict(flags=NORMAL, normal_sq=0), dict(flags=PLANE, sigma_z=1e-3),
              dict(flags=LUMA, sigma_l2=1.0, eps_l=1e-30), dict(flags=LUMA | DEMOD | MOD, sigma_l2=4.0, alb_floor=1 / 256),
              dict(flags=NORMAL | PLANE | LUMA | DEMOD, normal_sq=7, sigma_z=0.5, sigma_l2=4.0, alb_floor=1e-3),
              dict(flags=MOD, alb_floor=1 / 256)]


@pytest.mark.parametrize("case", range(len(HAND_CASES)))
@pytest.mark.parametrize("step", [1, 2, 5])
def test_hand_made_records_give_finite_colours(rays_mod, case, step):
    """wherever the centre colour is finite (here: everywhere) the output colour is finite: a NaN, zero or negative weight
    closes the tap.  The variance is finite where no NaN variance lies among the pixel's taps (a tap's weight does not look at
    the tap's own variance, so a NaN there is summed: the arithmetic as pinned)."""
    col, var, rec = _hand_made()
    kw = HAND_CASES[case]
    out, vout = rays_mod.atrous_pass(col, var, rec, step, **kw)
    assert np.isfinite(out).all(), np.argwhere(~np.isfinite(out))[:5]
    h, w = var.shape
    near = np.zeros((h, w), dtype=bool)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            y, x = 6 + dy * step, 9 + dx * step
            if 0 <= y < h and 0 <= x < w:
                near[y, x] = True
    assert np.isfinite(vout[~near]).all()
    if kw["flags"] & NORMAL and kw["normal_sq"] == 7:
        # 0.3^128 underflows to 0: the bottom rows and the rest do not read each other
        col2 = col.copy()
        col2[10:] += 3.0
        out2, _ = rays_mod.atrous_pass(col2, var, rec, step, **kw)
        assert (_bits(out2[:10]) == _bits(out[:10])).all()
    if kw == dict(flags=NORMAL, normal_sq=6):
        ws = []
        rays_mod.atrous_pass(col, var, rec, 1, weights=ws, **kw)
        tiny = np.concatenate([w_[t_] for t_, w_ in ws])
        assert ((tiny > 0) & (tiny < 1e-30)).any(), "0.3^64 * h: taps open with weights 36 orders below the centre's"


@pytest.mark.parametrize("ch", [3, 4])
def test_modulate_after_demodulate_in_one_pass_is_c_over_a_times_a(rays_mod, ch):
    """a 1 x 1 frame has no neighbours: the pass gives (c / a) * a per channel -- NOT c -- through the one tap there is: the
    centre's weight is h = 9/64, not a power of two, so by the pinned arithmetic the value is (((c / a) * h) / h) * a, four
    roundings, which is within 2 ulp of (c / a) * a and is what is asserted bit for bit.  a = alb above the floor, the floor
    below it or for a NaN; a fourth channel is neither divided nor multiplied (it too passes through * h / h)"""
    floor, hc = F(1 / 256), F(9 / 64)
    for alb in ((0.3, 0.7, 0.9), (0.0, 1e-3, np.nan), (-1.0, 1 / 256, 2.0)):
        rec = _flat(1, 1)
        rec[0, 0, 8:11] = alb
        col = np.array([[[0.123, 0.777, 0.451, 0.9][:ch]]], dtype=F)
        out, vout = rays_mod.atrous_pass(col, np.full((1, 1), 0.5, dtype=F), rec, 1, flags=DEMOD | MOD, alb_floor=floor)
        a = np.array([x if x > floor else floor for x in np.array(alb, dtype=F)], dtype=F)
        want = (((col[0, 0, :3] / a) * hc) / hc) * a
        plain = (col[0, 0, :3] / a) * a
        assert (_bits(out[0, 0, :3]) == _bits(want)).all()
        assert (np.abs(_bits(want).astype(np.int64) - _bits(plain).astype(np.int64)) <= 2).all()
        assert _bits(vout[0, 0]) == _bits((F(0.5) * (hc * hc)) / (hc * hc))
        if ch == 4:
            assert _bits(out[0, 0, 3]) == _bits((col[0, 0, 3] * hc) / hc)
        only, _ = rays_mod.atrous_pass(col, None, rec, 1, flags=DEMOD, alb_floor=floor)
        assert (_bits(only[0, 0, :3]) == _bits(((col[0, 0, :3] / a) * hc) / hc)).all()
    rec.view(np.int32)[0, 0, 7] = -1                     # a miss is neither divided nor multiplied, nor filtered
    out, _ = rays_mod.atrous_pass(col, None, rec, 1, flags=DEMOD | MOD, alb_floor=floor)
    assert (_bits(out) == _bits(col)).all()


def _atrous64(col, var, rec, step, takes, flags=0, normal_sq=0, sigma_z=1.0, sigma_l2=1.0, eps_l=1e-6):
    """the same formula in float64 on the float32 inputs, with the taken / not taken decisions of the float32 run; returns
    (colour, sum |c_q| w_q / sum w_q) per channel"""
    d64 = np.float64
    h, w, ch = col.shape
    pos, nrm = rec[..., 0:3].astype(d64), rec[..., 4:7].astype(d64)
    c = col.astype(d64)
    lum = c[..., 0] * d64(F(0.2126)) + c[..., 1] * d64(F(0.7152)) + c[..., 2] * d64(F(0.0722))
    v = var.astype(d64)
    H = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
    ys, xs = np.mgrid[0:h, 0:w]
    sc, sa, sw = np.zeros((h, w, ch)), np.zeros((h, w, ch)), np.zeros((h, w))
    k = 0
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            take = takes[k][0][0]
            k += 1
            qy, qx = np.clip(ys + dy * step, 0, h - 1), np.clip(xs + dx * step, 0, w - 1)
            wt = np.full((h, w), H[dy + 2] * H[dx + 2])
            if dx or dy:
                if flags & NORMAL:
                    d = np.maximum((nrm * nrm[qy, qx]).sum(-1), 0.0)
                    wt = wt * d ** (2 ** normal_sq)
                if flags & PLANE:
                    x = np.abs((nrm * (pos[qy, qx] - pos)).sum(-1)) / d64(F(sigma_z))
                    wt = wt / (1 + x * x)
                if flags & LUMA:
                    dl = lum - lum[qy, qx]
                    wt = wt / (1 + dl * dl / (d64(F(sigma_l2)) * v + d64(F(eps_l))))
            wt = np.where(take, wt, 0.0)
            sc += c[qy, qx] * wt[..., None]
            sa += np.abs(c[qy, qx]) * wt[..., None]
            sw += wt
    return sc / sw[..., None], sa / sw[..., None]


@pytest.mark.parametrize("step", [1, 2, 7])
def test_float64_evaluation_agrees(rays_mod, step):
    """|fp32 - fp64| <= 64 * 2^-24 * (sum |c_q| w_q / sum w_q) per channel, the decisions taken as the fp32 run took them.
    The cap counts the roundings (each at most 2^-24 relative) on the longest path of a term c_q w_q / sum_w: the weight -- the
    dot 3, up to 7 squarings, h * d 1, the plane stop 6 (dot 3, division, x * x, the sum and the reciprocal folded into 2, the
    product 1 shared with the next), the luma stop 6 likewise -- about 24; c_q * w 1; at most 25 adds each into sum_c and into
    sum_w, of which a term sees on average half: 25; the division 1; the rest is slack for the luminances and den.  It is a
    count of roundings, not a condition number: the differences inside the stops (dl, n . e) cancel, and where a stop is steep
    their absolute error is amplified -- for the luma stop by at most 1 / (2 sqrt(den)).  The inputs keep that small: colours
    in [0, 1), variances of 0.001 and more with sigma_l2 = 4 (den >= 0.004, amplification <= 8), positions within 30 of each
    other with sigma_z = 0.5.  A derived cap, not a measurement (the inputs here reach about 9 * 2^-24)."""
    col, var, rec = _random_frame(23, 29, 40 + step)
    rec.view(np.int32)[..., 7][rec.view(np.int32)[..., 7] < 0] = 2          # every pixel filtered
    ws = []
    out, _ = rays_mod.atrous_pass(col, var, rec, step, weights=ws, **ALL_STOPS)
    kw = {k: v for k, v in ALL_STOPS.items()}
    ref, scale = _atrous64(col, var, rec, step, ws, **kw)
    err = np.abs(out.astype(np.float64) - ref)
    assert (err <= 64 * 2.0 ** -24 * scale).all(), float((err / scale).max() / 2.0 ** -24)
    assert sum(int(t.sum()) for t, _ in ws) > 10 * col.shape[0] * col.shape[1], "most pixels take many taps"


@pytest.mark.parametrize("albedo", [False, True])
def test_denoise_is_its_passes(rays_mod, albedo):
    col, var, rec = _random_frame(19, 17, 77)
    stops = dict(normal_power=8, plane=0.5, luma=2.0, luma_eps=1e-6)
    c, v = rays_mod.denoise(col, var, rec, passes=3, albedo=albedo, **stops)
    a, av = col, var
    for k, step in enumerate((1, 2, 4)):
        flags = NORMAL | PLANE | LUMA | (DEMOD if albedo and k == 0 else 0) | (MOD if albedo and k == 2 else 0)
        a, av = rays_mod.atrous_pass(a, av, rec, step, flags, 3, F(0.5), F(2.0) * F(2.0), F(1e-6), F(1 / 256))
    assert (_bits(c) == _bits(a)).all() and (_bits(v) == _bits(av)).all()
    one, _ = rays_mod.denoise(col, var, rec, passes=1, albedo=True, **stops)
    both, _ = rays_mod.atrous_pass(col, var, rec, 1, NORMAL | PLANE | LUMA | DEMOD | MOD, 3, 0.5, 4.0, 1e-6, 1 / 256)
    assert (_bits(one) == _bits(both)).all(), "one pass is first and last"
    c5, v5 = rays_mod.denoise(col, None, rec, passes=5, normal_power=None)
    assert v5 is None and np.isfinite(c5).all()
    # batches: a frame alone and as frame 1 of 2
    two, twov = rays_mod.denoise(np.stack([col[::-1], col]), np.stack([var, var]), np.stack([rec, rec]), passes=3, albedo=albedo, **stops)
    assert (_bits(two[1]) == _bits(c)).all() and (_bits(twov[1]) == _bits(v)).all()
    for bad in (dict(passes=0), dict(passes=8), dict(demodulate=True), dict(normal_power=3), dict(plane=0.0), dict(luma=-1.0)):
        with pytest.raises(ValueError):
            rays_mod.denoise(col, var, rec, **bad)


def test_noise_falls_and_stays_finite(rays_mod):
    """five passes take noise of standard deviation 0.1 on a flat guide below 0.01 (the variance factors alone give 0.1 *
    (70/256)^5 at the centre of an infinite frame; edges and the luma stop keep it above that)"""
    rng = np.random.default_rng(1)
    h, w = 45, 67
    col = rng.normal(0.5, 0.1, (h, w, 3)).astype(F)
    var = np.full((h, w), 0.01, dtype=F)
    c, v = rays_mod.denoise(col, var, _flat(h, w), passes=5, plane=0.5, luma=4.0)
    assert np.isfinite(c).all() and np.isfinite(v).all() and c.std() < 0.01 < col.std() and v.max() < 0.01 * 0.08


def _rule_state():
    """the constructed columns of tests/test_pt_adaptive.py's rule test: counts 0, 1, 2, 3, at and above max, M2 NaN, negative, inf"""
    f = lambda *v: np.array(v, dtype=np.float32).view(np.uint32)
    cases = [(0, 0.0, 0.0, 0.0), (1, 0.0, 0.0, 0.0), (2, 0.5, 0.5, 0.5), (2, 0.5, F(0.5) + F(2.0 ** -24), 0.5),
             (2, 0.0, 0.0, 0.50001), (3, 1.5, 1.5, 1.5), (3, np.nan, 0.0, 0.0), (5, -1.0, -np.inf, 0.0), (11, np.inf, 0.0, 0.0),
             (12, np.inf, np.nan, 9e9), (13, np.inf, 0.0, 0.0), (0xFFFFFFFF, np.nan, 0.0, 0.0),
             (4, -3.0, 1.0, 1.0), (7, 0.25, 0.5, 0.125), (2, -0.0, 0.0, -0.0), (1, 9.0, 9.0, 9.0)]
    st = np.zeros((8, len(cases)), dtype=np.uint32)
    st[0] = 0xDEADBEEF
    st[1:4] = f(0.1, 0.2, 0.3)[:, None]
    for i, (m, a, b, c) in enumerate(cases):
        st[4, i] = m
        st[5:8, i] = f(a, b, c)
    return st


def _variance_scalar(st, spp, unknown):
    n = st.shape[1]
    v = np.empty(n, dtype=F)
    m2 = st[5:8].view(F)
    with np.errstate(all="ignore"):
        for i in range(n):
            m = int(st[4, i])
            if m >= 2:
                s = (m2[0, i] + m2[1, i]) + m2[2, i]
                s = s if 0 < s else F(0)
                v[i] = s / ((F(m) * F(m - 1)) * F(3))
            else:
                v[i] = F(unknown)
        out = np.empty(n // spp, dtype=F)
        for p in range(n // spp):
            acc = v[p * spp]
            for k in range(1, spp):
                acc = acc + v[p * spp + k]
            out[p] = acc * (F(1) / F(spp * spp))
    return out


@pytest.mark.parametrize("spp", [1, 2, 4])
def test_variance_of_a_constructed_state(rays_mod, spp):
    st = _rule_state()
    for unknown in (1.0, 0.0, np.inf, 0.125):
        got = rays_mod.pt_adapt_view_variance(st, spp, unknown)
        assert got.dtype == np.float32 and got.shape == (1, st.shape[1] // spp)
        want = _variance_scalar(st, spp, unknown)
        assert (_bits(got[0]) == _bits(want)).all()
        two = rays_mod.pt_adapt_view_variance(np.stack([st, st[:, ::-1]]).view(np.int32), spp, unknown)
        assert (_bits(two[0]) == _bits(want)).all()
    v1 = rays_mod.pt_adapt_view_variance(st, 1, 7.0)[0]
    assert v1[0] == 7.0 and v1[1] == 7.0 and v1[15] == 7.0, "m < 2: unknown"
    assert v1[2] == F(1.5) / F(6) and v1[7] == 0.0 and v1[12] == 0.0, "a negative sum is taken as 0"
    assert v1[6] == 0.0 and np.isinf(v1[8]) and v1[9] == 0.0 and _bits(v1[14]) == 0, "a NaN sum fails 0 < s and is taken as 0"
    for bad in (3, 0, 5):
        with pytest.raises(ValueError):
            rays_mod.pt_adapt_view_variance(st, bad)
    with pytest.raises(ValueError):
        rays_mod.pt_adapt_view_variance(st[:, :15], 2)


@pytest.mark.parametrize("spp", [1, 2, 4])
def test_variance_against_recorded_samples_in_float64(rays_mod, spp):
    """ordinary columns: states folded by pt_adapt_fold from recorded samples in [0, 1), m = 2 .. 12 per slot, against the float64
    two-pass variance of the same samples: per slot sum over channels of sum (x - mean)^2 / (m - 1), / 3 for the channel mean,
    / m for the mean's variance; per pixel the sum / spp^2.  Bound per slot: Welford's M2 in fp32 adds m terms d1 * d2 >= 0, each
    with |d| <= 1 known to 4 * 2^-24 absolutely (a subtraction of numbers below 1 and the mean's own error), so each term is off
    by at most 10 * 2^-24 and the m roundings of the running sum by m * 2^-24 * M2 <= m * 2^-24 * m: |M2 err| <= (10 m + m^2)
    2^-24 per channel; the division adds 3 roundings relative.  So |v err| <= (10 m + m^2) 2^-24 / (m (m - 1)) + 4 * 2^-24 v."""
    rng = np.random.default_rng(spp)
    n, S = 32 * spp, 12
    ms = rng.integers(2, S + 1, n)
    cols = rng.uniform(0, 1, (n, S, 3)).astype(F)
    st = np.zeros((8, n), dtype=np.uint32)
    for m in np.unique(ms):
        sel = np.flatnonzero(ms == m)
        sub, _, _ = rays_mod.pt_adapt_fold(st[:, sel], cols[sel], np.zeros((len(sel), S), dtype=np.uint32), int(m), int(m), 0.0)
        st[:, sel] = sub
    assert (st[4] == ms).all()
    got = rays_mod.pt_adapt_view_variance(st, spp)[0].astype(np.float64)
    v64, bound = np.empty(n), np.empty(n)
    for i in range(n):
        x = cols[i, :ms[i]].astype(np.float64)
        m = int(ms[i])
        v64[i] = ((x - x.mean(0)) ** 2).sum() / (m - 1) / 3 / m
        bound[i] = (10 * m + m * m) * 2.0 ** -24 / (m * (m - 1)) + 4 * 2.0 ** -24 * v64[i]
    want = v64.reshape(-1, spp).sum(1) / spp ** 2
    cap = bound.reshape(-1, spp).sum(1) / spp ** 2 + 4 * 2.0 ** -24 * want
    assert (np.abs(got - want) <= cap).all(), float((np.abs(got - want) / cap).max())


def test_specification_refuses(rays_mod):
    col, var, rec = _random_frame(6, 7, 1)
    ok = rays_mod.atrous_pass
    for bad in (dict(step=0), dict(step=65), dict(normal_sq=8), dict(normal_sq=-1), dict(flags=32), dict(sigma_z=0.0), dict(sigma_l2=-1.0),
                dict(eps_l=np.nan), dict(alb_floor=0.0)):
        kw = dict(step=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            ok(col, var, rec, **kw)
    for c, v, r in ((col.astype(np.float64), var, rec), (col[..., :2], var, rec), (col, var[:-1], rec), (col, var, rec[..., :11]),
                    (col, var.astype(np.float64), rec), (col[0], var, rec), (col, var, rec[:-1])):
        with pytest.raises(ValueError):
            ok(c, v, r, 1)
    S = rays_mod.atrous_stops
    assert S() == (NORMAL, 7, F(1), F(1), F(1e-6), F(1 / 256))
    assert S(normal_power=None, plane=0.25, luma=3.0, demodulate=True, modulate=True)[:4] == (PLANE | LUMA | DEMOD | MOD, 0, F(0.25), F(9))
    assert [S(normal_power=p)[1] for p in (1, 2, 4, 8, 16, 32, 64, 128)] == list(range(8))
    for bad in (dict(normal_power=0), dict(normal_power=3), dict(normal_power=256), dict(normal_power=2.0), dict(normal_power=True),
                dict(plane=0), dict(plane=-1.0), dict(plane=np.nan), dict(plane=np.inf), dict(plane="x"), dict(luma=0.0),
                dict(luma=np.nan), dict(luma=1e30), dict(luma=1e-30), dict(luma_eps=0.0), dict(luma_eps=None), dict(albedo_floor=0.0),
                dict(albedo_floor=-1)):
        with pytest.raises(ValueError):
            S(**bad)


def test_python_refusals_without_a_gpu(qr):
    """what Scene.atrous and Scene.denoise refuse before anything reaches the library or the device: QrError.  The scene is a
    shell without a handle; every tensor is on the CPU, which is 'another device' and the last thing checked"""
    import torch
    me = object.__new__(qr.Scene)
    me._h, me.device = ctypes.c_void_p(), 0
    n, h, w = 2, 5, 6
    col, hits, var = torch.zeros((n, h, w, 3)), torch.zeros((n, h, w, 12)), torch.zeros((n, h, w))
    with pytest.raises(qr.QrError, match="on cuda:0"):
        me.atrous(col, hits, var)
    with pytest.raises(qr.QrError, match="on cuda:0"):
        me.denoise(col, hits)
    for kw in (dict(normal_power=3), dict(normal_power=256), dict(normal_power=1.0), dict(plane=0.0), dict(plane=float("nan")),
               dict(luma=-2.0), dict(luma=1e30), dict(luma_eps=0.0), dict(albedo_floor=0.0), dict(albedo_floor="a")):
        with pytest.raises(qr.QrError, match="must be"):
            me.atrous(col, hits, var, **kw)
        with pytest.raises(qr.QrError, match="must be"):
            me.denoise(col, hits, var, **kw)
    for step in (0, 65, -1, 1.5, True, None):
        with pytest.raises(qr.QrError, match="step must be"):
            me.atrous(col, hits, var, step=step)
    for passes in (0, 8, 2.0, True):
        with pytest.raises(qr.QrError, match="passes must be"):
            me.denoise(col, hits, var, passes=passes)
    for kw in (dict(demodulate=True), dict(modulate=False)):
        with pytest.raises(qr.QrError, match="albedo=True"):
            me.denoise(col, hits, var, **kw)
    with pytest.raises(qr.QrError, match="nonsense"):
        me.denoise(col, hits, var, nonsense=1)
    for bad in (col.double(), col[..., :2], torch.zeros((n, h, w, 5)), col[0], col.numpy(), torch.zeros((0, h, w, 3)), None):
        with pytest.raises(qr.QrError, match="colour must be"):
            me.atrous(bad, hits, var)
        with pytest.raises(qr.QrError, match="colour must be"):
            me.denoise(bad, hits, var)
    for bad in (hits.double(), hits[..., :11], hits[:1], hits.reshape(n, h * w, 12), None):
        with pytest.raises(qr.QrError, match="hits must be"):
            me.atrous(col, bad, var)
    for bad in (var.double(), var[:1], var[..., None], var.numpy()):
        with pytest.raises(qr.QrError, match="variance must be"):
            me.atrous(col, hits, bad)
    for bad in (col.double(), torch.zeros((n, h, w, 4)), col[:1]):
        with pytest.raises(qr.QrError, match="out must be"):
            me.atrous(col, hits, var, out=bad)
    with pytest.raises(qr.QrError, match="variance_out needs a variance"):
        me.atrous(col, hits, variance_out=var)
    for bad in (var.double(), var[:1]):
        with pytest.raises(qr.QrError, match="variance_out must be"):
            me.atrous(col, hits, var, variance_out=bad)
    with pytest.raises(qr.QrError, match="contiguous"):
        me.atrous(torch.zeros((n, h, w, 6))[..., ::2], hits, var)


# ---------------------------------------------------------------------------------------------------------------- GPU

def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def _dev(scn, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(f"cuda:{scn.device}")


def _tailed(scn, shape):
    """an output buffer filled with NaN and one extra row of SENTINEL behind it: (whole, body)"""
    import torch
    n, h, w = shape[:3]
    rest = tuple(shape[3:])
    whole = torch.full((n * h + 1, w) + rest, float("nan"), dtype=torch.float32, device=f"cuda:{scn.device}")
    whole[n * h:] = SENTINEL
    return whole, whole[:n * h].view(shape)


def _pass_gpu(scn, col, var, hits, step, kw, where):
    """one qr_atrous_views_async call through ctypes into NaN-filled, sentinel-tailed buffers, compared with atrous_pass on the
    same host arrays: every word of the body, the tail intact"""
    import torch
    qr = sys.modules["quadray_engine_amd"]
    rm = _rays_mod()
    n, h, w, ch = col.shape
    cd, hd = _dev(scn, col), _dev(scn, hits)
    vd = None if var is None else _dev(scn, var)
    cw, cb = _tailed(scn, (n, h, w, ch))
    vw, vb = _tailed(scn, (n, h, w)) if var is not None else (None, None)
    p = qr.AtrousParams(step, ch, kw.get("normal_sq", 0), kw.get("flags", 0), kw.get("sigma_z", 1.0), kw.get("sigma_l2", 1.0),
                        kw.get("eps_l", 1e-6), kw.get("alb_floor", 1 / 256))
    vp = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())
    rc = qr.lib().qr_atrous_views_async(scn._h, vp(cd), vp(vd), vp(hd), n, w, h, ctypes.byref(p), vp(cb), vp(vb),
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, f"{where}: {qr.lib().qr_last_error().decode()}"
    want, wantv = rm.atrous_pass(col, var, hits, step, **kw)
    got = _host(cw)
    assert (got[n * h:] == SENTINEL).all(), f"{where}: the row behind the colour was written"
    bad = _bits(got[:n * h].reshape(n, h, w, ch)) != _bits(want)
    assert not bad.any(), f"{where}: {int(bad.any(-1).sum())} of {n * h * w} pixels differ, first {np.argwhere(bad)[:4].tolist()}"
    if var is not None:
        gv = _host(vw)
        assert (gv[n * h:] == SENTINEL).all(), f"{where}: the row behind the variance was written"
        badv = _bits(gv[:n * h].reshape(n, h, w)) != _bits(wantv)
        assert not badv.any(), f"{where}: {int(badv.sum())} of {n * h * w} variances differ, first {np.argwhere(badv)[:4].tolist()}"
    return got[:n * h].reshape(n, h, w, ch)


_REAL = {}


def _real(qr, rm, scene):
    """(scene, views tensor, inputs) of a real case, computed once: 6 adaptive candidates on 2 seeded cameras at 64 x 64 in one
    launch: mean, variance(), view_hits, and a 4-channel input: the view_gather of a spun cosine_dirs(4) fan"""
    import torch
    if scene not in _REAL:
        w = h = 64
        scn = qr.Scene(_base(scene), ray_queries=True)
        scn.set_pt(False)
        views = [np.array(v, dtype=F) for v in _cams(rm, scene)[:2]]
        t = _host(scn.view_hits(TPV._vt(scn, views), w, h))[..., 3]
        for j, v in enumerate(views):
            if (t[j] < v[7]).all():                     # a camera inside a closed room: end its rays at the median depth, so
                v[7] = np.median(t[j])                  # that the far half of the frame are misses, for every call below alike
        vt = TPV._vt(scn, views)
        acc = scn.pt_adaptive_views(vt, w, h, min_samples=2, max_samples=64, tol=0.05)
        _, mean = acc.step(6, mean=True)
        var = acc.variance()
        hits = scn.view_hits(vt, w, h)
        spin = torch.from_numpy(rm.spins((2, h, w), 7)).to(vt.device)
        dirs = torch.from_numpy(rm.cosine_dirs(4)).to(vt.device)
        gat, _ = scn.view_gather(vt, dirs, w, h, eps=EPS, reach=REACH, frame=True, spin=spin)
        _REAL[scene] = (scn, vt, acc, dict(mean=_host(mean), var=_host(var), hits=_host(hits), gather=_host(gat),
                                          state=_host(acc.state)))
    return _REAL[scene]


def _stop_sets(sigma_z):
    full = dict(normal_sq=3, sigma_z=sigma_z, sigma_l2=4.0, eps_l=1e-6)
    return [dict(full, flags=NORMAL | PLANE | LUMA), dict(full, flags=NORMAL), dict(full, flags=PLANE), dict(full, flags=LUMA),
            dict(flags=0), dict(full, flags=NORMAL | PLANE | LUMA, normal_sq=0), dict(full, flags=NORMAL | LUMA, normal_sq=7)]


@pytest.mark.gpu
@pytest.mark.parametrize("scene", REAL_SCENES)
def test_gpu_real_inputs(qr, rays_mod, scene):
    """each step with all stops, each stop alone and none, normal_sq 0, 3 and 7, with a variance plane; at steps 1 and 16 also
    without one, and the 4-channel gather input with and without; the variance() input itself against the numpy statement"""
    scn, vt, acc, x = _real(qr, rays_mod, scene)
    ids = x["hits"].view(np.int32)[..., 7]
    assert (ids < 0).any() and len(np.unique(ids[ids >= 0])) > 1, "misses and more than one surface: the stops have work"
    assert np.isfinite(x["mean"]).all() and (x["var"] > 0).any()
    spp = 1 << TPV._fsaa(_base(scene))
    want = rays_mod.pt_adapt_view_variance(x["state"], spp, 1.0).reshape(x["var"].shape)
    assert (_bits(x["var"]) == _bits(want)).all(), "variance() against pt_adapt_view_variance"
    pos = x["hits"][..., 0:3][ids >= 0]
    sigma_z = float(np.abs(pos - pos.mean(0)).max()) / 64
    for step in STEPS:
        for kw in _stop_sets(sigma_z):
            _pass_gpu(scn, x["mean"], x["var"], x["hits"], step, kw, f"{scene} step {step} {kw}")
        if step in (1, 16):
            for kw in _stop_sets(sigma_z)[:5]:
                _pass_gpu(scn, x["mean"], None, x["hits"], step, kw, f"{scene} step {step} no variance {kw}")
                _pass_gpu(scn, x["gather"], None, x["hits"], step, kw, f"{scene} step {step} 4 channels {kw}")
            _pass_gpu(scn, x["gather"], x["var"], x["hits"], step, dict(_stop_sets(sigma_z)[0], flags=31), f"{scene} step {step} 4 channels, all flags")


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["patched:demo02_160_gf_aa4", "patched:demo01_160"])
def test_gpu_variance_of_edited_states(qr, rays_mod, scene):
    """variance() on a scene with 4x FSAA and on one without, at 67 x 45 and 9 x 130, on the state as stepped and on host-edited
    states (m set to 0, 1 and max, M2 set to NaN and negative, the constructed rule columns), `unknown` 1 and 0.25, into a
    sentinel-tailed buffer"""
    import torch
    blob = _base(scene)
    spp = 1 << TPV._fsaa(blob)
    assert spp == (4 if "aa4" in scene else 1)
    scn = qr.Scene(blob, ray_queries=True)
    try:
        for (w, h) in ((67, 45), (9, 130)):
            vt = TPV._vt(scn, _cams(rays_mod, scene)[:2])
            acc = scn.pt_adaptive_views(vt, w, h, min_samples=2, max_samples=16, tol=0.05)
            acc.step(4)
            st = _host(acc.state).view(np.uint32)
            rng = np.random.default_rng(w)
            ed = st.copy()
            slots = ed.shape[2]
            pick = lambda: rng.integers(0, slots, slots // 7)
            ed[0, 4, pick()] = 0
            ed[1, 4, pick()] = 1
            ed[0, 4, pick()] = 16
            ed[1, 4, pick()] = 0xFFFFFFFF
            ed[0, 5, pick()] = np.array([np.nan], dtype=F).view(np.uint32)[0]
            ed[1, 6, pick()] = np.array([-2.5], dtype=F).view(np.uint32)[0]
            ed[1, 7, pick()] = np.array([np.inf], dtype=F).view(np.uint32)[0]
            rule = _rule_state()
            ed[0, :, :rule.shape[1]] = rule
            for state in (st, ed):
                acc.state.copy_(torch.from_numpy(state.view(np.int32)).to(vt.device))
                for unknown in (1.0, 0.25):
                    whole, body = _tailed(scn, (2, h, w))
                    assert acc.variance(out=body, unknown=unknown) is body
                    got = _host(whole)
                    assert (got[2 * h:] == SENTINEL).all()
                    want = rays_mod.pt_adapt_view_variance(state, spp, unknown).reshape(2, h, w)
                    bad = _bits(got[:2 * h].reshape(2, h, w)) != _bits(want)
                    assert not bad.any(), f"{scene} {w}x{h} unknown {unknown}: {int(bad.sum())} pixels differ"
                    assert (_host(acc.state).view(np.uint32) == state).all(), "the state is only read"
            fresh = acc.variance(unknown=0.25)
            assert tuple(fresh.shape) == (2, h, w) and torch.equal(fresh.view(torch.int32), body.view(torch.int32))
    finally:
        scn.close()


def _synthetic(w, h):
    """the CPU tests' inputs at a frame size: [(name, colour [1, h, w, C], variance, records, stop sets)]"""
    out = []
    col, var, rec = _random_frame(h, w, 100 + w)
    out.append(("random", col, var, rec, [ALL_STOPS, dict(flags=0), dict(ALL_STOPS, flags=31, alb_floor=1 / 64)]))
    col4, _, _ = _random_frame(h, w, 200 + w, ch=4)
    out.append(("random4", col4, var, rec, [dict(ALL_STOPS, flags=NORMAL | LUMA | DEMOD), dict(flags=MOD)]))
    if w >= 9 and h >= 9:
        hc, hv, hr = _hand_made(h, w) if (h >= 14 and w >= 13) else _hand_made()
        out.append(("hand-made", hc, hv, hr, HAND_CASES))
        for stop in (NORMAL, PLANE, LUMA):
            c, v, r, kw = _halves(stop, h, w, w // 2, seed=stop)
            out.append((f"halves {stop}", c, v, r, [kw]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_gpu_synthetic_inputs(qr, rays_mod, size):
    """the CPU tests' inputs uploaded -- a random frame in 3 and 4 channels, the hand-made records, the half-frames -- at 1 x 1,
    9 x 130 and 67 x 45 with steps up to 64: most taps fall off the frame, most tiles are partial, every phase has its own
    length.  NaN-filled, sentinel-tailed outputs"""
    w, h = size
    scn = qr.Scene(_base("patched:demo01_160"))          # any scene, any mode, no ray-query list
    try:
        for name, col, var, rec, sets in _synthetic(w, h):
            for step in (1, 2, 3, 7, 16, 33, 64):
                for kw in sets:
                    _pass_gpu(scn, col[None], var[None], rec[None], step, kw, f"{name} {w}x{h} step {step} {kw}")
                _pass_gpu(scn, col[None], None, rec[None], step, sets[0], f"{name} {w}x{h} step {step} no variance")
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_views_are_independent_and_denoise(qr, rays_mod):
    """view j alone and as view 2 of 3 gives the same bits; Scene.atrous is the C call; Scene.denoise equals rays.denoise, with
    and without albedo and variance, and leaves the caller's tensors as they were; the same call twice gives the same bytes; a
    call on a side stream behind an event gives the bytes of the current stream"""
    import torch
    scene = REAL_SCENES[0]
    scn, vt, acc, x = _real(qr, rays_mod, scene)
    col, var, hits = _dev(scn, x["mean"]), _dev(scn, x["var"]), _dev(scn, x["hits"])
    kw = dict(normal_power=8, plane=0.05, luma=2.0)
    for step in (1, 4):
        both, bothv = scn.atrous(col, hits, var, step=step, **kw)
        want, wantv = rays_mod.atrous_pass(x["mean"], x["var"], x["hits"], step, *rays_mod.atrous_stops(**kw))
        assert (_bits(_host(both)) == _bits(want)).all() and (_bits(_host(bothv)) == _bits(wantv)).all()
        three = torch.cat([col[1:], col[:1], col[1:]]), torch.cat([hits[1:], hits[:1], hits[1:]]), torch.cat([var[1:], var[:1], var[1:]])
        o3, v3 = scn.atrous(three[0], three[1], three[2], step=step, **kw)
        o1, v1 = scn.atrous(col[1:].contiguous(), hits[1:].contiguous(), var[1:].contiguous(), step=step, **kw)
        for t in (o3[2], o3[0], o1[0]):
            assert torch.equal(t.view(torch.int32), both[1].view(torch.int32))
        assert torch.equal(o3[1].view(torch.int32), both[0].view(torch.int32)) and torch.equal(v3[2].view(torch.int32), v1[0].view(torch.int32))
        only = scn.atrous(col, hits, step=step, **kw)
        assert isinstance(only, torch.Tensor) and tuple(only.shape) == tuple(col.shape)
        out, vout = torch.empty_like(col), torch.empty_like(var)
        r = scn.atrous(col, hits, var, step=step, out=out, variance_out=vout, **kw)
        assert r[0] is out and r[1] is vout and torch.equal(out.view(torch.int32), both.view(torch.int32))
    for albedo, v in ((False, var), (True, var), (True, None)):
        c0, h0 = col.clone(), hits.clone()
        got, gotv = scn.denoise(col, hits, v, passes=5, albedo=albedo, **kw)
        again, againv = scn.denoise(col, hits, v, passes=5, albedo=albedo, **kw)
        want, wantv = rays_mod.denoise(x["mean"], None if v is None else x["var"], x["hits"], passes=5, albedo=albedo, **kw)
        assert (_bits(_host(got)) == _bits(want)).all(), f"denoise albedo={albedo} variance={v is not None}"
        assert (gotv is None) == (v is None) and (v is None or (_bits(_host(gotv)) == _bits(wantv)).all())
        assert torch.equal(again.view(torch.int32), got.view(torch.int32)), "the same call twice"
        assert torch.equal(col.view(torch.int32), c0.view(torch.int32)) and torch.equal(hits.view(torch.int32), h0.view(torch.int32))
        assert torch.equal(var.view(torch.int32), _dev(scn, x["var"]).view(torch.int32)), "the caller's tensors are only read"
        assert got.data_ptr() not in (col.data_ptr(),) and np.isfinite(want).all()
    one, _ = scn.denoise(col, hits, var, passes=1, albedo=True, **kw)
    assert (_bits(_host(one)) == _bits(rays_mod.denoise(x["mean"], x["var"], x["hits"], passes=1, albedo=True, **kw)[0])).all()
    # a side stream: its work waits for an event recorded after the inputs were made, the current stream for its event
    ref, refv = scn.denoise(col, hits, var, passes=3, **kw)
    side = torch.cuda.Stream()
    ready = torch.cuda.Event()
    c2 = col.clone()
    ready.record()
    side.wait_event(ready)
    s_out, s_var = scn.denoise(c2, hits, var, passes=3, stream=side, **kw)
    p_out = scn.atrous(c2, hits, step=2, stream=side, **kw)
    done = torch.cuda.Event()
    done.record(side)
    torch.cuda.current_stream().wait_event(done)
    assert torch.equal(s_out.view(torch.int32), ref.view(torch.int32)) and torch.equal(s_var.view(torch.int32), refv.view(torch.int32))
    assert torch.equal(p_out.view(torch.int32), scn.atrous(col, hits, step=2, **kw).view(torch.int32))
    side.synchronize()
    with pytest.raises(qr.QrError, match="in place"):
        scn.atrous(col, hits, var, out=col)
    with pytest.raises(qr.QrError, match="in place"):
        scn.atrous(col, hits, var, variance_out=var)
    with pytest.raises(qr.QrError, match="out must be"):
        acc.variance(out=var[:1])


@pytest.mark.gpu
def test_gpu_refusals(qr, rays_mod):
    """every QR_ERR_ARG of the two entry points through ctypes, the outputs untouched after all of them; n_views = 0 is QR_OK"""
    import torch
    L = qr.lib()
    scn = qr.Scene(_base("patched:demo02_160_gf_aa4"))
    dev = f"cuda:{scn.device}"
    n, w, h = 2, 9, 7
    col = torch.zeros((n * h * w * 3 + 8,), dtype=torch.float32, device=dev)
    var = torch.zeros((n * h * w + 8,), dtype=torch.float32, device=dev)
    hits = torch.zeros((n * h * w + 1, 12), dtype=torch.float32, device=dev)
    out = torch.full((n * h * w * 4 + 8,), 7.5, dtype=torch.float32, device=dev)
    vout = torch.full((n * h * w + 8,), 7.5, dtype=torch.float32, device=dev)
    vp = lambda x, off=0: ctypes.c_void_p(None if x is None else x.data_ptr() + off)
    nan = float("nan")

    def call(s=scn._h, ci=vp(col), vi=vp(var), hi=vp(hits), n=n, w=w, h=h, co=vp(out), vo=vp(vout), null_p=False, **pk):
        f = dict(step=1, channels=3, normal_sq=3, flags=7, sigma_z=1.0, sigma_l2=1.0, eps_l=1e-6, alb_floor=1 / 256)
        f.update(pk)
        p = qr.AtrousParams(f["step"], f["channels"], f["normal_sq"], f["flags"], f["sigma_z"], f["sigma_l2"], f["eps_l"], f["alb_floor"])
        return L.qr_atrous_views_async(s, ci, vi, hi, n, w, h, None if null_p else ctypes.byref(p), co, vo, None)

    assert call(s=None) == ARG and call(null_p=True) == ARG
    assert call(ci=vp(None)) == ARG and call(hi=vp(None)) == ARG and call(co=vp(None)) == ARG
    assert call(ci=vp(col, 2)) == ARG and call(co=vp(out, 1)) == ARG and call(vi=vp(var, 2)) == ARG and call(vo=vp(vout, 3)) == ARG
    assert call(hi=vp(hits, 4)) == ARG and call(hi=vp(hits, 8)) == ARG, "hits are 16-byte aligned"
    assert call(co=vp(col)) == ARG and call(vo=vp(var)) == ARG, "in place"
    assert call(vi=vp(None)) == ARG and call(vo=vp(None)) == ARG, "var_in and var_out go together"
    assert call(step=0) == ARG and call(step=65) == ARG and call(step=-1) == ARG
    assert call(channels=2) == ARG and call(channels=5) == ARG and call(channels=0) == ARG
    assert call(normal_sq=8) == ARG and call(normal_sq=-1) == ARG
    for name in ("sigma_z", "sigma_l2", "eps_l", "alb_floor"):
        for bad in (0.0, -1.0, nan, -0.0):
            assert call(**{name: bad}) == ARG, (name, bad)
    assert call(flags=32) == ARG and call(flags=0x80000000) == ARG and call(flags=7 | 64) == ARG
    assert call(w=0) == ARG and call(h=0) == ARG and call(w=16385) == ARG and call(h=16385) == ARG and call(w=-3) == ARG
    assert call(n=-1) == ARG and call(n=65536) == ARG
    assert call(n=0) == 0 and call(n=0, ci=vp(None), co=vp(None), hi=vp(None)) == 0
    torch.cuda.synchronize()
    assert (out == 7.5).all().item() and (vout == 7.5).all().item(), "a refused call wrote something"
    # served: offsets that keep the alignment, no variance, four channels, every flag, the widest step
    assert call() == 0 and call(ci=vp(col, 4), co=vp(out, 12), vi=vp(var, 4), vo=vp(vout, 8), hi=vp(hits, 48)) == 0
    assert call(vi=vp(None), vo=vp(None)) == 0 and call(channels=4, n=1, flags=31, step=64) == 0
    torch.cuda.synchronize()
    scn.close()

    scn = qr.Scene(_base("patched:demo02_160_gf_aa4"), ray_queries=True)
    state = torch.zeros((n * 8 * h * w * 4 + 4,), dtype=torch.int32, device=dev)
    vv = torch.full((n * h * w + 4,), 7.5, dtype=torch.float32, device=dev)

    def vcall(s=scn._h, st=vp(state), n=n, w=w, h=h, unknown=1.0, v=vp(vv), flags=0):
        return L.qr_pt_adapt_views_variance_async(s, st, n, w, h, unknown, v, flags, None)

    assert vcall(s=None) == ARG and vcall(st=vp(None)) == ARG and vcall(v=vp(None)) == ARG
    assert vcall(st=vp(state, 2)) == ARG and vcall(v=vp(vv, 1)) == ARG
    assert vcall(flags=1) == ARG and vcall(flags=0x80000000) == ARG
    assert vcall(w=0) == ARG and vcall(h=0) == ARG and vcall(w=16385) == ARG and vcall(h=16385) == ARG
    assert vcall(n=-1) == ARG and vcall(n=65536) == ARG
    assert vcall(n=0) == 0 and vcall(n=0, st=vp(None), v=vp(None)) == 0
    torch.cuda.synchronize()
    assert (vv == 7.5).all().item(), "a refused call wrote something"
    assert vcall() == 0 and vcall(st=vp(state, 4), v=vp(vv, 4), unknown=nan) == 0
    torch.cuda.synchronize()
    scn.close()
    plain = qr.Scene(_base("patched:demo02_160_gf_aa4"))                # no ray-query list: the variance needs none
    assert L.qr_pt_adapt_views_variance_async(plain._h, vp(state), n, w, h, 1.0, vp(vv), 0, None) == 0
    torch.cuda.synchronize()
    assert (vv[:n * h * w] == 0.25).all().item(), "a zero state holds no samples: four slots of unknown 1.0, over 16"
    plain.close()


# once more through the guarded diagnostic build (make guard), as tests/test_framed_fans.py does it: the library is chosen when
# the package is imported, hence the child process: this file run as a script.

def _guard_child():
    from qr_loader import load_package
    qr = load_package()
    assert qr.LIB_PATH == GUARD_LIB, qr.LIB_PATH
    rm = _rays_mod()
    scene = REAL_SCENES[0]
    scn, vt, acc, x = _real(qr, rm, scene)
    kw = dict(flags=NORMAL | PLANE | LUMA, normal_sq=3, sigma_z=0.05, sigma_l2=4.0, eps_l=1e-6)
    for step in (1, 4):
        _pass_gpu(scn, x["mean"], x["var"], x["hits"], step, kw, f"guard {scene} step {step}")
    scn.close()
    print(f"{scene} guard_ok 1", flush=True)
    return 0


@pytest.mark.gpu
def test_gpu_guarded_build_gives_the_same_filter():
    assert os.path.exists(GUARD_LIB), "libqrhip_guard.so is missing: build() makes it (make -C quadray-engine_amd/csrc guard)"
    env = dict(os.environ, QR_LIB=GUARD_LIB)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-child"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.count("guard_ok 1") == 1 and "QR_GUARD" not in out.stderr, out.stdout + out.stderr[-3000:]


if __name__ == "__main__":
    sys.exit(_guard_child() if "--guard-child" in sys.argv else 2)
