"""Temporal reprojection with a clamp (include/qrhip.h qr_reproject_clamped_async; rays.reproject_pass(clamp=, moved=);
Scene.reproject(clamp=, moved=), Scene.temporal(clamp=)): the fetched history colour held to a box of this frame's colours around
the pixel before it is blended.  On the CPU the numpy specification is held to the header's text -- a step change by hand, a
scalar restatement at every pixel of synthetic frames, the pinned order as bits, properties, the oracle's records and shading of
animated scenes --; on the GPU every word of every output is held to the specification.  The helpers of tests/test_reproject.py
and tests/test_reproject_moving.py are imported, not copied."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import test_atrous as TA
import test_reproject as TR
import test_reproject_moving as TM
from conftest import ROOT, load_blob
from test_atrous import SENTINEL, _bits, _dev, _host
from test_pt_views import _rays_mod
from test_reproject import ARG, ASM, F, GUARD_LIB, H16, S, W16, _dyadic_view, _history, _plane, _same
from test_reproject_moving import SIZES, _chain_inputs, _frames, _is_identity, _records, _view

KERNELS = ("22qr_reproj_clamp_kernelILi3ELb0EE", "22qr_reproj_clamp_kernelILi3ELb1EE",
           "22qr_reproj_clamp_kernelILi4ELb0EE", "22qr_reproj_clamp_kernelILi4ELb1EE")
LDS = {3: 4 * 38 * 14 * 4, 4: 5 * 38 * 14 * 4}             # (CH + 1) planes of (32 + 6) x (8 + 6) words
SCALAR_SIZES = [(1, 1), (2, 3), (9, 130), (67, 45)]         # (w, h)
SYNTH_SIZES = [(1, 1), (9, 130), (67, 45), (33, 9)]
INF = F(np.inf)


@pytest.fixture(scope="module")
def rays_mod():
    return _rays_mod()


# ------------------------------------------------------------------------------------------------- names and sizes

def test_symbols_sizes_and_header(qr, rays_mod):
    rm = rays_mod
    hdr = open(os.path.join(ROOT, "include", "qrhip.h")).read()
    assert "qr_reproject_clamped_async" in qr.ABI_SYMBOLS and "int qr_reproject_clamped_async(" in hdr
    assert hasattr(qr.lib(), "qr_reproject_clamped_async") and len(qr.lib().qr_reproject_clamped_async.argtypes) == 20
    assert ctypes.sizeof(qr.ClampParams) == 32 and "typedef struct qr_clamp_params {       /* 32 bytes, 8 words */" in hdr
    assert [n for n, _ in qr.ClampParams._fields_] == ["flags", "radius", "gamma", "short_len", "reserved"]
    assert (qr.CLAMP_MINMAX, qr.CLAMP_VARIANCE, qr.CLAMP_SHORTEN, qr.CLAMP_MAX_RADIUS) == (1, 2, 4, 3)
    assert (rm.CLAMP_MINMAX, rm.CLAMP_VARIANCE, rm.CLAMP_SHORTEN, rm.CLAMP_MAX_RADIUS) == (1, 2, 4, 3)
    for text in ("#define QR_CLAMP_MINMAX    1u", "#define QR_CLAMP_VARIANCE  2u", "#define QR_CLAMP_SHORTEN   4u",
                 "#define QR_CLAMP_MAX_RADIUS 3", "h1 = hc < lo ? lo : hc", "h2 = hi < h1 ? hi : h1", "d = fabsf(h2 - hc)",
                 "moved = d > moved ? d : moved", "lo = v < lo ? v : lo", "hi = hi < v ? v : hi", "nf = (float)n",
                 "v = t2[k] / nf - mu * mu", "w = gamma * sd", "lo = mu - w", "hi = mu + w", "len = len < short_len ? len : short_len",
                 "no sum here can be -0.0", "a NaN bound clamps", "qr_reproject_clamped_async below is this call with the clamp step"):
        assert text in hdr, text
    assert "a follow-up, not" not in hdr
    # the structures and calls that stay: test_reproject.py pins them, this only says that the new call did not touch them
    assert ctypes.sizeof(qr.ReprojectParams) == 64 and len(qr.lib().qr_reproject_moving_async.argtypes) == 18
    for fn in (qr.Scene.reproject, rm.reproject_pass):
        sig = inspect.signature(fn).parameters
        assert sig["clamp"].default is None and sig["moved"].default is False
    for fn in (qr.Scene.temporal, qr.Temporal.__init__, rm.temporal, rm.Temporal.__init__):
        assert inspect.signature(fn).parameters["clamp"].default is None
    c = rm.clamp_stops()
    assert c == dict(flags=2, radius=1, gamma=F(1.0), short_len=F(1.0)) and sorted(c) == ["flags", "gamma", "radius", "short_len"]
    assert rm.clamp_stops("minmax", 3, short_len=2)["flags"] == 5 and rm.clamp_stops("variance", 2, 0.5, 1.5)["flags"] == 6


def test_kernels_in_resource_check():
    """the four new instances are in the build's own check -- nothing spilled, no private segment, the staged planes as the LDS
    limit, the VGPRs of the next occupancy step -- and the build's assembly, where there is one, meets it; their names do not
    contain the static kernels' name"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import check_kernel_resources as ck
    finally:
        sys.path.pop(0)
    for frag in KERNELS:
        ch = 3 if "ILi3" in frag else 4
        assert ck.LIMITS[frag] == ({3: 96, 4: 80}[ch], 0, 0) and ck.LDS_LIMITS[frag] == LDS[ch]
        assert "qr_reproject_kernel" not in frag
    assert LDS == {3: 8512, 4: 10640}
    if os.path.exists(ASM):
        mine = [k for k in ck.kernels(ASM) if "qr_reproj_clamp_kernel" in k["name"]]
        assert len(mine) == 4 and len([k for k in ck.kernels(ASM) if "qr_reproject_kernel" in k["name"]]) == 2
        for k in mine:
            frag = next(f for f in KERNELS if f in k["name"])
            assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0
            assert k["group_segment_fixed_size"] <= ck.LDS_LIMITS[frag] and k["vgpr_count"] <= ck.LIMITS[frag][0]


# ------------------------------------------------------------------------------------------------- a step change by hand

def _step_case(ch):
    """a 9 x 9 patch of the plane z = 1 under the fixed dyadic camera: every pixel projects onto itself and takes one tap of
    weight 1"""
    w = h = 9
    a = np.array([0.25, 0.5, 0.125, 0.75][:ch], dtype=F)
    b = np.array([0.875, 0.0625, 0.5, 0.25][:ch], dtype=F)
    rec, views = _plane(w, h)[None], _dyadic_view(w, h)[None]
    return w, h, a, b, rec, views


@pytest.mark.parametrize("ch", [3, 4])
def test_step_change_by_hand(rays_mod, ch):
    """constant colour A for 6 frames, then constant B, alpha_min 0: unclamped the first B frame is A * (1 - 1/7) + B * (1/7),
    written out; clamped -- min/max and variance, any radius, any gamma -- it is B in every bit, with moved = the largest
    |B - A| of the channels; with SHORTEN and short_len 1 the length is 1 and the variance the fresh rule's; moved is -1.0
    on the first frame"""
    rm = rays_mod
    w, h, a, b, rec, views = _step_case(ch)
    var_in = np.full((1, h, w), 0.375, dtype=F)
    p = rm.reproject_stops(plane_max=2.0 ** -4, alpha_min=0.0, alpha_mom_min=0.0, var_min_len=1)
    blocks = [rm.clamp_stops(m, r, g) for m in ("minmax", "variance") for r in (1, 2, 3) for g in (0.0, 1.0, 7.5)]
    ca, cb = np.broadcast_to(a, (1, h, w, ch)).copy(), np.broadcast_to(b, (1, h, w, ch)).copy()
    prev = None
    for k in range(6):
        got = rm.reproject_pass(ca, rec, var_in, prev, clamp=blocks[k], moved=True, **p)
        assert len(got) == 5 and got[4].dtype == F and got[4].shape == (1, h, w)
        assert (got[4] == (-1.0 if k == 0 else 0.0)).all() and (_bits(got[4]) == _bits(F(-1.0 if k == 0 else 0.0))).all()
        assert (got[0][..., 6] == k + 1).all() and (_bits(got[1]) == _bits(ca)).all(), "a constant stays what it is"
        prev = (views, rec, got[0])
    seventh = F(1.0) / F(7.0)
    plain = rm.reproject_pass(cb, rec, var_in, prev, **p)
    assert len(plain) == 4
    assert (_bits(plain[1]) == _bits(a * (F(1.0) - seventh) + b * seventh)).all() and (plain[0][..., 6] == 7).all()
    dist = np.abs(b - a).max()
    for c in blocks:
        hist, col, var, _, mv = rm.reproject_pass(cb, rec, var_in, prev, clamp=c, moved=True, **p)
        assert (_bits(col) == _bits(cb)).all(), c
        assert (_bits(mv) == _bits(dist)).all() and (hist[..., 6] == 7).all()
        _same(hist[..., 4:6], plain[0][..., 4:6], "the moments are blended unchanged")
        _same(var, plain[2], "... and so is the variance without SHORTEN")
        short = dict(c, flags=c["flags"] | rm.CLAMP_SHORTEN, short_len=F(1.0))
        hist, col, var, _, mv = rm.reproject_pass(cb, rec, var_in, prev, clamp=short, moved=True, **dict(p, var_min_len=F(2.0)))
        assert (_bits(col) == _bits(cb)).all() and (hist[..., 6] == 1).all() and (_bits(var) == _bits(F(0.375))).all()
        assert (_bits(mv) == _bits(dist)).all()


# ------------------------------------------------------------------------------------------------- the scalar restatement

def _scalar_box(col, ok, x, y, flags, r, gamma):
    """the header's box for ONE pixel in scalar float32, written a second time: (lo [ch], hi [ch], n)"""
    h, w, ch = col.shape
    zero = F(0.0)
    with np.errstate(all="ignore"):
        if flags & 2:
            n, t1, t2 = 0, [zero] * ch, [zero] * ch
            for j in range(-r, r + 1):
                rn, r1, r2 = 0, [zero] * ch, [zero] * ch
                for i in range(-r, r + 1):
                    qx, qy = x + i, y + j
                    if 0 <= qx < w and 0 <= qy < h and ok[qy, qx]:
                        rn += 1
                        v = col[qy, qx]
                        r1 = [r1[k] + v[k] for k in range(ch)]
                        r2 = [r2[k] + v[k] * v[k] for k in range(ch)]
                n += rn
                t1 = [t1[k] + r1[k] for k in range(ch)]
                t2 = [t2[k] + r2[k] for k in range(ch)]
            lo, hi = [], []
            for k in range(ch):
                nf = F(n)
                mu = t1[k] / nf
                v = t2[k] / nf - mu * mu
                v = v if 0 < v else zero
                wd = F(gamma) * np.sqrt(v)
                lo.append(mu - wd), hi.append(mu + wd)
            return lo, hi, n
        n, lo, hi = 0, [INF] * ch, [-INF] * ch
        for j in range(-r, r + 1):
            rl, rh = [INF] * ch, [-INF] * ch
            for i in range(-r, r + 1):
                qx, qy = x + i, y + j
                if 0 <= qx < w and 0 <= qy < h and ok[qy, qx]:
                    n += 1
                    v = col[qy, qx]
                    rl = [v[k] if v[k] < rl[k] else rl[k] for k in range(ch)]
                    rh = [v[k] if rh[k] < v[k] else rh[k] for k in range(ch)]
            lo = [rl[k] if rl[k] < lo[k] else lo[k] for k in range(ch)]
            hi = [rh[k] if hi[k] < rh[k] else hi[k] for k in range(ch)]
        return lo, hi, n


def _read_step(col, rec, demod, alb_floor):
    """every pixel's colour after the read step, in the test's own words"""
    out = col.copy()
    ids = rec.view(np.int32)[..., 7]
    if demod:
        with np.errstate(all="ignore"):
            alb = rec[..., 8:11]
            out[..., 0:3] = np.where((ids >= 0)[..., None], out[..., 0:3] / np.where(alb > F(alb_floor), alb, F(alb_floor)), out[..., 0:3])
    return out, ids >= 0


def _scalar_frame(w, h, ch, seed):
    """one view under the fixed dyadic camera: every hit projects onto itself and takes its own pixel's history through one tap
    of weight 1.  Colours and history with NaN, Inf, -0.0 and denormals; misses scattered, and around three pixels everything
    within radius 3 but the centre is a miss; a textured albedo, some of it below the floor"""
    rng = np.random.default_rng(seed)
    rec = _plane(w, h)
    ids = rec.view(np.int32)[..., 7]
    ids[rng.uniform(size=(h, w)) < 0.3] = 5
    ids[rng.uniform(size=(h, w)) < 0.2] = -1
    for _ in range(3):
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        ids[max(0, y - 3):y + 4, max(0, x - 3):x + 4] = -1
        ids[y, x] = 2
    ids[h // 2, w // 2] = 2
    rec[..., 8:11] = rng.choice(np.array([0.001, 0.25, 0.5, 0.9, 1.0], dtype=F), (h, w, 3))
    col = rng.uniform(0.0, 1.0, (h, w, ch)).astype(F)
    hist = _history(h, w, seed + 1, ch)
    hist[..., 0:ch] = rng.uniform(-0.5, 1.5, (h, w, ch)).astype(F)
    for a, share in ((col, 0.02), (hist[..., 0:ch], 0.01)):
        for val in (np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-41, -3e-45):
            a[...] = np.where(rng.uniform(size=a.shape) < share, F(val), a)
    return col, rec, (_dyadic_view(w, h), rec.copy(), hist)


def _covering(w, h):
    """(ch, radius, mode, demodulate, shorten): every combination on the small frames; on the large ones every radius with
    every mode, the channels, the flag and SHORTEN alternating so that each value meets each radius or mode"""
    if w * h <= 6:
        return [(ch, r, m, d, s) for ch in (3, 4) for r in (1, 2, 3) for m in (1, 2) for d in (False, True) for s in (False, True)]
    return [(3 + (r + m + (w > 9)) % 2, r, m, bool((r + (w > 9)) % 2), bool(m % 2) ^ bool(r % 2)) for r in (1, 2, 3) for m in (1, 2)]


@pytest.mark.parametrize("size", SCALAR_SIZES)
def test_clamp_step_against_the_scalar_text(rays_mod, size):
    """the header's clamp step, written a second time in scalar float32 (one rounding per operation), at EVERY pixel of
    synthetic frames of 1x1, 2x3, 9x130 and 67x45: the box (lo, hi, n) of rays.clamp_box, and the entry, the variance and the
    moved plane of reproject_pass(clamp=, moved=True)"""
    rm = rays_mod
    w, h = size
    seen = 0
    for ch, r, mode, demod, shorten in _covering(w, h):
        col, rec, prev = _scalar_frame(w, h, ch, 100 * w + 10 * r + ch)
        gamma = F([0.0, 0.75, 1.5][r - 1])
        c = dict(flags=mode | (4 if shorten else 0), radius=r, gamma=gamma, short_len=F(2.0))
        p = rm.reproject_stops(plane_max=2.0 ** -4, demodulate=demod, max_len=6, var_min_len=3, alpha_min=0.125)
        where = f"{w}x{h} ch {ch} r {r} mode {mode} demod {demod} shorten {shorten}"
        read, ok = _read_step(col, rec, demod, p["alb_floor"])
        lo, hi, n = rm.clamp_box(read[None], ok[None], c["flags"], r, gamma)
        hist, out, var, _, mv = rm.reproject_pass(col, rec, None, prev, clamp=c, moved=True, **p)
        plain = rm.reproject_pass(col, rec, None, prev, **p)
        one = F(1.0)
        for y in range(h):
            for x in range(w):
                slo, shi, sn = _scalar_box(read, ok, x, y, c["flags"], r, gamma)
                if not ok[y, x]:
                    assert mv[y, x] == -1 and hist[y, x, 6] == 1, where
                    continue
                assert sn == n[0, y, x] and sn >= 1
                _same(lo[0, y, x], np.array(slo, dtype=F), f"{where} lo ({x}, {y})")
                _same(hi[0, y, x], np.array(shi, dtype=F), f"{where} hi ({x}, {y})")
                g = prev[2][y, x]
                with np.errstate(all="ignore"):
                    sw = F(0.0) + one
                    moved, h2 = F(0.0), []
                    for k in range(ch):
                        hc = (F(0.0) + g[k] * one) / sw
                        h1 = slo[k] if hc < slo[k] else hc
                        h2.append(shi[k] if shi[k] < h1 else h1)
                        d = np.abs(h2[k] - hc)
                        moved = d if d > moved else moved
                    ln = (F(0.0) + g[6] * one) / sw + one
                    ln = ln if ln < p["max_len"] else p["max_len"]
                    if shorten and 0 < moved:
                        ln = ln if ln < c["short_len"] else c["short_len"]
                    a = one / ln
                    ac = a if a > p["alpha_min"] else p["alpha_min"]
                    want = [h2[k] * (one - ac) + read[y, x, k] * ac for k in range(ch)]
                _same(hist[y, x, :ch], np.array(want, dtype=F), f"{where} colour ({x}, {y})")
                _same(out[y, x], np.array(want, dtype=F), f"{where} colour_out ({x}, {y})")
                _same(hist[y, x, 6], ln, f"{where} len ({x}, {y})")
                _same(mv[y, x], moved, f"{where} moved ({x}, {y})")
                if not shorten or not 0 < moved:
                    _same(hist[y, x, 4:], plain[0][y, x, 4:], f"{where} moments and length ({x}, {y})")
                    _same(var[y, x], plain[2][y, x], f"{where} variance ({x}, {y})")
                elif ln < p["var_min_len"]:
                    _same(var[y, x], p["unknown"], f"{where} the fresh rule's variance ({x}, {y})")
                seen += 1
    assert seen >= 1


# ------------------------------------------------------------------------------------------------- the order, as bits

def _separable_box(rm, col, ok, flags, r, gamma, columns_first=False):
    """the box by a row pass into planes of its own, then a column pass over those planes (columns_first: the other order)"""
    if columns_first:
        out = _separable_box(rm, col.transpose(0, 2, 1, 3), ok.transpose(0, 2, 1), flags, r, gamma)
        return tuple(a.transpose(0, 2, 1, 3) for a in out)
    n, h, w, ch = col.shape
    with np.errstate(all="ignore"):
        colp = np.zeros((n, h, w + 2 * r, ch), dtype=F)
        colp[:, :, r:r + w] = col
        okp = np.zeros((n, h, w + 2 * r), dtype=bool)
        okp[:, :, r:r + w] = ok
        if flags & 2:
            rn, r1, r2 = np.zeros((n, h, w), dtype=np.int64), np.zeros((n, h, w, ch), dtype=F), np.zeros((n, h, w, ch), dtype=F)
            for i in range(2 * r + 1):
                v, o = colp[:, :, i:i + w], okp[:, :, i:i + w]
                rn += o
                r1, r2 = np.where(o[..., None], r1 + v, r1), np.where(o[..., None], r2 + v * v, r2)
            planes = [np.zeros((n, h + 2 * r, w) + a.shape[3:], dtype=a.dtype) for a in (rn, r1, r2)]
            for pl, a in zip(planes, (rn, r1, r2)):
                pl[:, r:r + h] = a
            cnt, t1, t2 = np.zeros((n, h, w), dtype=np.int64), np.zeros((n, h, w, ch), dtype=F), np.zeros((n, h, w, ch), dtype=F)
            for j in range(2 * r + 1):
                cnt, t1, t2 = cnt + planes[0][:, j:j + h], t1 + planes[1][:, j:j + h], t2 + planes[2][:, j:j + h]
            nf = cnt.astype(F)[..., None]
            mu = t1 / nf
            var = t2 / nf - mu * mu
            var = np.where(0 < var, var, F(0.0))
            wd = F(gamma) * np.sqrt(var)
            return (mu - wd).astype(F), (mu + wd).astype(F)
        rl, rh = np.full((n, h, w, ch), np.inf, dtype=F), np.full((n, h, w, ch), -np.inf, dtype=F)
        for i in range(2 * r + 1):
            v, o = colp[:, :, i:i + w], okp[:, :, i:i + w]
            rl, rh = np.where(o[..., None] & (v < rl), v, rl), np.where(o[..., None] & (rh < v), v, rh)
        pl, ph = np.full((n, h + 2 * r, w, ch), np.inf, dtype=F), np.full((n, h + 2 * r, w, ch), -np.inf, dtype=F)
        pl[:, r:r + h], ph[:, r:r + h] = rl, rh
        lo, hi = np.full((n, h, w, ch), np.inf, dtype=F), np.full((n, h, w, ch), -np.inf, dtype=F)
        for j in range(2 * r + 1):
            lo, hi = np.where(pl[:, j:j + h] < lo, pl[:, j:j + h], lo), np.where(hi < ph[:, j:j + h], ph[:, j:j + h], hi)
        return lo, hi


def test_direct_and_separable_orders_agree_and_another_order_does_not(rays_mod):
    """the pinned order -- a row's partials, then the rows folded -- evaluated directly (rays.clamp_box) and separably (a row
    pass into planes, a column pass over them) gives the same bits on the scalar test's frames in both modes at every radius;
    columns first differs in variance mode on at least one of them, so the comparison can tell an order from another"""
    rm = rays_mod
    differs = 0
    for w, h in SCALAR_SIZES:
        for ch in (3, 4):
            col, rec, _ = _scalar_frame(w, h, ch, 7 * w + ch)
            for demod in (False, True):
                read, ok = _read_step(col, rec, demod, 1 / 256)
                for r in (1, 2, 3):
                    for flags in (1, 2):
                        lo, hi, n = rm.clamp_box(read[None], ok[None], flags, r, 1.25)
                        slo, shi = _separable_box(rm, read[None], ok[None], flags, r, 1.25)
                        at = ok[None]
                        _same(slo[at], lo[at], f"{w}x{h} r {r} flags {flags} lo"), _same(shi[at], hi[at], f"{w}x{h} r {r} flags {flags} hi")
                        clo, chi = _separable_box(rm, read[None], ok[None], flags, r, 1.25, columns_first=True)
                        both = at[..., None] & ~(np.isnan(lo) | np.isnan(clo))
                        differs += int(((_bits(clo) != _bits(lo)) & both).sum()) if flags == 2 else 0
    assert differs > 0


def test_counts_at_corner_and_edge_and_views_apart(rays_mod):
    """radius 1 counts 4 neighbours in a frame's corner, 6 on its edge, 9 inside; in a stack of three views of different
    constant colours the middle view's boxes hold its own colour alone, in both modes"""
    rm = rays_mod
    w, h = 7, 5
    col = np.random.default_rng(2).uniform(0.0, 1.0, (1, h, w, 3)).astype(F)
    _, _, n = rm.clamp_box(col, np.ones((1, h, w), dtype=bool), 2, 1)
    assert n[0, 0, 0] == n[0, 0, -1] == n[0, -1, 0] == n[0, -1, -1] == 4
    assert (n[0, 0, 1:-1] == 6).all() and (n[0, -1, 1:-1] == 6).all() and (n[0, 1:-1, 0] == 6).all() and (n[0, 1:-1, -1] == 6).all()
    assert (n[0, 1:-1, 1:-1] == 9).all()
    consts = np.array([0.25, 0.5, 0.75], dtype=F)
    stack = np.broadcast_to(consts[:, None, None, None], (3, h, w, 4)).copy()
    for flags in (1, 2):
        for r in (1, 2, 3):
            lo, hi, n = rm.clamp_box(stack, np.ones((3, h, w), dtype=bool), flags, r, 3.0)
            assert (_bits(lo[1]) == _bits(F(0.5))).all() and (_bits(hi[1]) == _bits(F(0.5))).all(), (flags, r)
            assert n[1].max() == min(2 * r + 1, w) * min(2 * r + 1, h)


# ------------------------------------------------------------------------------------------------- properties

def _property_case(rm, ch, seed, finite=False):
    w, h = 23, 17
    col, rec, prev = _scalar_frame(w, h, ch, seed)
    if finite:
        col = np.random.default_rng(seed).uniform(0.25, 0.75, col.shape).astype(F)
    return col, rec, prev, rm.reproject_stops(plane_max=2.0 ** -4)


def test_properties(rays_mod):
    """min/max: lo <= h2 <= hi wherever the bounds are no NaN (and the box is not the empty (+inf, -inf) of a neighbourhood
    whose valid colours are all NaN, which the comparison form leaves: the header says so); gamma = 0: h2 == mu wherever hc is
    no NaN and the box has none; a box that contains hc leaves every word of the unclamped result and moved == +0.0;
    clamp=None is the old 4-tuple on the old bits"""
    rm = rays_mod
    for ch in (3, 4):
        col, rec, prev, p = _property_case(rm, ch, 40 + ch)
        read, ok = _read_step(col, rec, False, p["alb_floor"])
        hc = prev[2][..., :ch]                               # one tap of weight 1: sc / sw is the tap's colour (-0.0 as +0.0)
        keeps = ok & (prev[2][..., 6] >= 1)
        for r in (1, 2, 3):
            lo, hi, _ = rm.clamp_box(read[None], ok[None], 1, r)
            alpha1 = dict(p, alpha_min=F(0.0), max_len=F(np.inf))
            # with a history of length inf the blend weight is 0 and the entry is h2 itself
            inf_hist = prev[2].copy()
            inf_hist[..., 6] = np.inf
            for flags, gamma in ((1, 1.0), (2, 0.0)):
                c = dict(flags=flags, radius=r, gamma=F(gamma), short_len=F(1.0))
                out = rm.reproject_pass(col, rec, None, (prev[0], prev[1], inf_hist), clamp=c, moved=True, **alpha1)
                h2 = out[0][..., :ch]
                finite_col = np.isfinite(read).all(-1, keepdims=True)      # 0 * Inf in the blend is no statement about h2
                if flags == 1:
                    at = keeps[..., None] & ~np.isnan(lo[0]) & ~np.isnan(hi[0]) & (lo[0] <= hi[0]) & finite_col & ~np.isnan(hc)
                    assert at.sum() > 100 and (lo[0][at] <= h2[at]).all() and (h2[at] <= hi[0][at]).all()
                else:
                    mlo, mhi, _ = rm.clamp_box(read[None], ok[None], 2, r, 0.0)
                    at = keeps[..., None] & ~np.isnan(mlo[0]) & ~np.isnan(hc) & finite_col & np.isfinite(mlo[0])
                    assert at.sum() > 100 and (_bits(mlo[0]) == _bits(mhi[0]))[at].all()
                    assert (h2[at] == mlo[0][at]).all(), "gamma 0: the mean"
        # a box that contains hc
        col, rec, prev, p = _property_case(rm, ch, 50 + ch, finite=True)
        prev[2][..., :ch] = col                                # the history is the frame: inside every box of it
        plain = rm.reproject_pass(col, rec, None, prev, **p)
        assert len(plain) == 4
        for c in (rm.clamp_stops("minmax", 1), rm.clamp_stops("minmax", 3, short_len=1), rm.clamp_stops("variance", 2, 1e9, short_len=1)):
            got = rm.reproject_pass(col, rec, None, prev, clamp=c, moved=True, **p)
            for a, b in zip(got[:4], plain):
                _same(a, b, "a box that contains hc")
            ids = rec.view(np.int32)[..., 7]
            assert (_bits(got[4][ids >= 0]) == 0).all() and (got[4][ids < 0] == -1).all()
        again = rm.reproject_pass(col, rec, None, prev, clamp=None, moved=False, **p)
        assert len(again) == 4 and all((_bits(a) == _bits(b)).all() for a, b in zip(again, plain))


# ------------------------------------------------------------------------------------------------- real records

REAL = [(b, s) for b in sorted(TM.ANIMATED) for s in SIZES]
_SHADED = {}


def _shaded(qr, oracle, rm, base_name, w, h):
    """the oracle's shade of frames 0 and 1 of an animated case from the seeded camera: noise-free colour [2, h, w, 3]"""
    if (base_name, w, h) not in _SHADED:
        v = _view(qr, rm, base_name, w, h)[0]
        _SHADED[base_name, w, h] = np.stack([oracle.trace_rays(b, rm.view_rays(v, w, h, b, 0), "shade")[0].reshape(h, w, 3)
                                             for b, _ in _frames(qr, base_name)[:2]]).astype(F)
    return _SHADED[base_name, w, h]


@pytest.mark.parametrize("base_name,size", REAL)
def test_real_records_lose_the_moved_shadow(qr, oracle, rays_mod, base_name, size):
    """The tilting (demo02) and the turning (demo01) array at 64x64, 67x45 and 9x130, A -> B with the motion table, the colour
    the oracle's noise-free shade of each frame's own view rays: over the pixels that keep history the sum of |colour_out -
    colour of B| is strictly smaller with the min/max clamp at radius 1 than without it, and at least one pixel of a surface
    that did not move has 0 < moved: the light on it changed, not the surface.  No (fixture, size) pair had to be dropped.
    Measured, sum without / with the clamp, pixels that keep history, static pixels with 0 < moved:
    demo01 34.0686 / 26.0543, 2424, 165 at 64 x 64;  34.9729 / 23.7438, 2156, 101 at 67 x 45;  3.0352 / 2.8538, 241, 10 at 9 x 130;
    demo02 110.2553 / 83.4756, 4050, 329;  83.7173 / 68.4501, 2920, 206;  18.9432 / 13.3792, 1075, 79."""
    rm = rays_mod
    w, h = size
    v, off, plane_max = _view(qr, rm, base_name, w, h)
    recs = _records(qr, rm, base_name, w, h)
    col = _shaded(qr, oracle, rm, base_name, w, h)
    m = _frames(qr, base_name)[1][1]
    p = rm.reproject_stops(plane_max=plane_max, off=off)
    first = rm.reproject_pass(col[0], recs[0], None, None, **p)[0]
    prev = (v, recs[0], first)
    plain = rm.reproject_pass(col[1], recs[1], None, prev, motion=m, **p)
    got = rm.reproject_pass(col[1], recs[1], None, prev, motion=m, clamp=rm.clamp_stops("minmax", 1), moved=True, **p)
    keeps = plain[0][..., 6] > 1
    assert (keeps == (got[4] >= 0)).all()
    ids = recs[1].view(np.int32)[..., 7]
    static = (ids >= 0) & _is_identity(m[np.where(ids >= 0, ids >> 1, 0)])
    e0 = float(np.abs(plain[1].astype(np.float64) - col[1])[keeps].sum())
    e1 = float(np.abs(got[1].astype(np.float64) - col[1])[keeps].sum())
    lit = int((static & (got[4] > 0)).sum())
    print(f"{base_name} {w}x{h}: {e0:.4f} without, {e1:.4f} with the clamp over {int(keeps.sum())} pixels; {lit} static pixels moved")
    assert keeps.sum() > 0 and e1 < e0, (e0, e1)
    assert lit >= 1


def test_temporal_with_a_clamp_is_its_chained_passes(rays_mod):
    """rays.temporal(clamp=).step over 4 frames of two views against reproject_pass(clamp=) chained by hand; the clone carries
    the block; the block matters"""
    rm = rays_mod
    rng = np.random.default_rng(21)
    n = 4
    cols = rng.uniform(0.0, 1.0, (n, 2, H16, W16, 4)).astype(F)
    var = rng.uniform(0.01, 0.1, (n, 2, H16, W16)).astype(F)
    shifts = [(0.0, 0.0), (0.25, 0.75), (0.5, 0.125), (-0.375, 0.25)]
    recs = [np.stack([_plane(dx=dx, dy=dy), _plane(dx=-dy, dy=dx, sid=4)]) for dx, dy in shifts]
    views = np.stack([_dyadic_view(), _dyadic_view()])
    kw = dict(plane_max=2.0 ** -4, demodulate=True, var_min_len=2)
    c = rm.clamp_stops("variance", 2, 0.5, short_len=1.5)
    acc, p = rm.temporal(2, W16, H16, 4, clamp=c, **kw), rm.reproject_stops(**kw)
    assert acc.clamp == c and acc.clone().clamp == c and rm.temporal(2, W16, H16, 4, **kw).clamp is None
    prev, differs = None, 0
    for k in range(n):
        if k == 2:
            acc = acc.clone()
        want = rm.reproject_pass(cols[k], recs[k], var[k], prev, clamp=c, **p)
        assert len(want) == 4
        out, v = acc.step(cols[k], recs[k], views, var[k])
        _same(out, want[1], f"step {k} colour"), _same(v, want[2], f"step {k} variance"), _same(acc.history, want[0], f"step {k} history")
        if k:
            differs += int((_bits(rm.reproject_pass(cols[k], recs[k], var[k], prev, **p)[0]) != _bits(want[0])).sum())
        prev = (views, recs[k], want[0])
    assert differs > 0


# ------------------------------------------------------------------------------------------------- refusals without a device

BAD_BLOCKS = [(dict(flags=0), "exactly one of the two"), (dict(flags=3), "exactly one of the two"), (dict(flags=7), "exactly one of the two"),
              (dict(flags=8 | 2), "clamp flags must be of CLAMP_"), (dict(flags=0x80000001), "clamp flags must be of CLAMP_"),
              (dict(radius=0), "radius must be 1..3"), (dict(radius=4), "radius must be 1..3"), (dict(radius=-1), "radius must be 1..3"),
              (dict(gamma=-0.5), "gamma must be 0 or more"), (dict(gamma=float("nan")), "gamma must be 0 or more"),
              (dict(flags=1, gamma=float("nan")), "gamma must be 0 or more"),
              (dict(short_len=float("nan")), "short_len must not be NaN"), (dict(flags=6, short_len=0.5), "short_len must not be NaN, and 1 or more"),
              (dict(flags=5, short_len=-1.0), "short_len must not be NaN, and 1 or more")]


def test_refusals_without_a_gpu(qr, rays_mod):
    """the specification's and the binding's ValueError for a bad block, text and all, before any tensor is looked at; moved
    without a clamp; what clamp_stops refuses; served: short_len below 1 without SHORTEN"""
    import torch
    rm = rays_mod
    good = rm.clamp_stops()
    w, h, a, b, rec, views = _step_case(3)
    col = np.zeros((1, h, w, 3), dtype=F)
    me = object.__new__(qr.Scene)
    me._h, me.device = ctypes.c_void_p(), 0
    tc, th = torch.zeros((1, h, w, 3)), torch.zeros((1, h, w, 12))
    shape = "clamp must be None or a dict of flags, radius, gamma and short_len"
    blocks = [(dict(good, **kw), text) for kw, text in BAD_BLOCKS]
    blocks += [("variance", shape), (5, shape), (dict(flags=1), shape), (dict(good, more=1), shape), (dict(good, radius="x"), shape)]
    for bad, text in blocks:
        with pytest.raises(ValueError, match=text):
            rm.reproject_pass(col, rec, None, None, clamp=bad)
        with pytest.raises(ValueError, match=text):
            rm.temporal(1, w, h, clamp=bad)
        with pytest.raises(ValueError, match=text):
            me.reproject(tc, th, clamp=bad)
        with pytest.raises(ValueError, match=text):
            me.temporal(1, w, h, clamp=bad)
    with pytest.raises(ValueError, match="moved needs a clamp"):
        rm.reproject_pass(col, rec, None, None, moved=True)
    for moved in (True, torch.zeros((1, h, w))):
        with pytest.raises(ValueError, match="moved needs a clamp"):
            me.reproject(tc, th, moved=moved)
    with pytest.raises(qr.QrError, match="on cuda:0"):
        me.reproject(tc, th, clamp=good, moved=True)         # the block passes; the tensors are not on the device
    for kw, text in ((dict(mode="mean"), 'mode must be "variance" or "minmax"'), (dict(mode=2), "mode must be"),
                     (dict(radius=1.5), "radius must be an integer, 1..3"), (dict(radius=True), "radius must be an integer"),
                     (dict(radius=0), "radius must be 1..3"), (dict(radius=4), "radius must be 1..3"),
                     (dict(gamma="1"), "gamma must be a number"), (dict(gamma=-1), "gamma must be 0 or more"),
                     (dict(gamma=float("nan")), "gamma must be 0 or more"), (dict(short_len=0.5), "short_len must not be NaN, and 1 or more"),
                     (dict(short_len=float("nan")), "short_len must not be NaN"), (dict(short_len="2"), "short_len must be a number")):
        with pytest.raises(ValueError, match=text):
            rm.clamp_stops(**kw)
    assert len(rm.reproject_pass(col, rec, None, None, clamp=dict(good, short_len=F(0.25)), moved=True)) == 5
    assert len(rm.reproject_pass(col, rec, None, None, clamp=dict(good, short_len=F(-np.inf), gamma=F(np.inf)))) == 4
    # the unknown-keyword message of reproject_stops is what it was: clamp is no stop
    with pytest.raises(TypeError, match=r"reproject_stops\(\) got an unexpected keyword argument 'clamp'"):
        rm.reproject_stops(clamp=good)


# ---------------------------------------------------------------------------------------------------------------- GPU

def _block(qr, c, reserved=(0, 0, 0, 0)):
    return qr.ClampParams(int(c["flags"]), int(c["radius"]), float(c["gamma"]), float(c["short_len"]), (ctypes.c_uint32 * 4)(*reserved))


def _call_clamped(qr, rm, scn, col, rec, var, prev, motion, p, c, where, outs=(True, True, True, True), stream=None):
    """one qr_reproject_clamped_async call through ctypes into filled, sentinel-guarded buffers -- colour, variance, coords and
    moved 4 bytes off a 16-byte boundary --, compared with reproject_pass(clamp=, moved=True) on the same host arrays: every word
    of every output that is given, the guards intact.  Returns the history"""
    import torch
    n, h, w, ch = col.shape
    cd, hd = _dev(scn, col), _dev(scn, rec)
    vd = None if var is None else _dev(scn, var)
    pd = [None] * 3 if prev is None else [_dev(scn, a) for a in prev]
    md = None if motion is None else _dev(scn, motion)
    shapes = [(n, h, w, 8), (n, h, w, ch), (n, h, w), (n, h, w, 2), (n, h, w)]
    bufs = [TR._buffer(scn, s, 777.0 if k == 3 else float("nan"), min(k, 1)) if k == 0 or outs[k - 1] else (None, None)
            for k, s in enumerate(shapes)]
    vp = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())
    cp, cc = TR._params(qr, ch, p), _block(qr, c)
    st = torch.cuda.current_stream() if stream is None else stream
    rc = qr.lib().qr_reproject_clamped_async(scn._h, vp(cd), vp(hd), vp(vd), vp(pd[0]), vp(pd[1]), vp(pd[2]), vp(md),
                                             0 if motion is None else len(motion), n, w, h, ctypes.byref(cp), ctypes.byref(cc),
                                             *(vp(b[1]) for b in bufs), ctypes.c_void_p(st.cuda_stream))
    assert rc == 0, f"{where}: {qr.lib().qr_last_error().decode()}"
    st.synchronize()
    want = rm.reproject_pass(col, rec, var, prev, motion=motion, clamp=c, moved=True, **p)
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
    return got_hist


BLOCKS = [("minmax", 1, 1.0, None), ("variance", 1, 1.0, None), ("minmax", 2, 1.0, 1.0), ("variance", 2, 0.5, 2.0),
          ("minmax", 3, 1.0, None), ("variance", 3, 2.0, 1.5)]
# (channels, var_in, DEMODULATE, table, (colour_out, var_out, coords_out, moved_out)): every block meets every line
COMBOS = [(3, True, False, True, (True, True, True, True)), (4, False, True, True, (False, True, False, True)),
          (4, True, True, False, (True, False, True, False)), (3, False, False, True, (False, False, False, False)),
          (3, True, True, True, (True, True, False, True)), (4, True, False, True, (True, True, True, True))]


def _run_clamped_chain(qr, rm, scn, x, stops, where, lines):
    """A -> B -> A', each step's history the input of the next; without the table (the static instance) the moved object is
    fresh, which is fine: the clamp is what is looked at"""
    for (mode, r, gamma, short), (ch, with_var, demod, table, outs) in lines:
        c = rm.clamp_stops(mode, r, gamma, short)
        p = rm.reproject_stops(demodulate=demod, **stops)
        prev, clamped = None, 0
        for k in range(3):
            col = np.ascontiguousarray(x["gather"][k:k + 1, ..., :ch])
            var = x["var"][k:k + 1] if with_var else None
            m = x["motion"][k] if table else None
            tag = f"{where} {mode} r {r} ch {ch} var {with_var} demod {demod} table {table} outs {outs} step {k}"
            hist = _call_clamped(qr, rm, scn, col, x["hits"][k:k + 1], var, prev, m if prev is not None else None, p, c, tag, outs)
            if k:
                clamped += int((rm.reproject_pass(col, x["hits"][k:k + 1], var, prev, motion=m, clamp=c, moved=True, **p)[4] > 0).sum())
            prev = (x["view"][None], x["hits"][k:k + 1], hist)
        assert clamped > 0, f"{where}: the clamp moved no pixel's history"


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("base_name", sorted(TM.ANIMATED))
def test_gpu_animated_chain(qr, rays_mod, base_name, size):
    """three frames of a turning object, each rendered from its own Scene (test_reproject_moving's inputs); three steps A -> B
    -> A' with both modes at radii 1 to 3, in 3 and 4 channels, with and without var_in, DEMODULATE, SHORTEN, the table and
    each optional output, moved_out among them"""
    w, h = size
    stops, x = _chain_inputs(qr, rays_mod, base_name, w, h)
    scn = qr.Scene(load_blob("demo01_160"))
    try:
        _run_clamped_chain(qr, rays_mod, scn, x, stops, f"{base_name} {w}x{h}", list(zip(BLOCKS, COMBOS)))
    finally:
        scn.close()


def _synthetic_colours(col, prev, seed):
    """NaN, Inf, -0.0 and denormals in this frame's colours, which the boxes are made of"""
    rng = np.random.default_rng(seed)
    col = col.copy()
    for val in (np.nan, np.inf, -np.inf, -0.0, 1e-41):
        col[...] = np.where(rng.uniform(size=col.shape) < 0.01, F(val), col)
    return col


@pytest.mark.gpu
@pytest.mark.parametrize("size", SYNTH_SIZES)
def test_gpu_synthetic_inputs(qr, rays_mod, size):
    """test_reproject's hand-made records (NaN, Inf, -0.0, scattered misses, a random history) with such colours, at 1x1, 9x130,
    67x45 and 33x9 in 3 and 4 channels, every block, with and without a table"""
    w, h = size
    rm = rays_mod
    scn = qr.Scene(load_blob("demo01_160"))
    try:
        for ch in (3, 4):
            col, rec, var, prev = TR._synthetic(w, h, 11 * w + ch, ch)
            col = _synthetic_colours(col, prev, 3 * w + ch)
            rec2, prev2 = TM._synthetic_ids(rec, prev, 13 * w + ch)
            tables = TM._tables(17 * w + ch)
            kws = (dict(plane_max=2.0 ** -5), dict(plane_max=2.0 ** -5, demodulate=True, var_min_len=1, max_len=8, unknown=np.nan),
                   dict(normal_min=-1.0, min_weight=0.3, alpha_min=1.0, alpha_mom_min=0.0, off=(0.5, -0.25)))
            for t, blk in enumerate(BLOCKS):
                p, c = rm.reproject_stops(**kws[t % 3]), rm.clamp_stops(*blk)
                _call_clamped(qr, rm, scn, col, rec, var, prev, None, p, c, f"synthetic {w}x{h} ch {ch} block {blk}")
                name, m = tables[t % len(tables)]
                _call_clamped(qr, rm, scn, col, rec2, None, prev2, m, p, c, f"synthetic {w}x{h} ch {ch} block {blk} table {name}",
                              (True, False, True, True))
            _call_clamped(qr, rm, scn, col, rec, var, None, None, rm.reproject_stops(demodulate=True), rm.clamp_stops(),
                          f"synthetic {w}x{h} ch {ch} first frame")
    finally:
        scn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(64, 2), (2, 64)])
def test_gpu_halo_wider_than_the_frame(qr, rays_mod, size):
    """64x2 and 2x64: the halo of radius 3 is wider than the frame; two tiles beside or below each other"""
    rm = rays_mod
    w, h = size
    scn = qr.Scene(load_blob("demo01_160"))
    try:
        for ch in (3, 4):
            col, rec, prev = _scalar_frame(w, h, ch, 5 * w + ch)
            p = rm.reproject_stops(plane_max=2.0 ** -4)
            assert (rm.reproject_pass(col, rec, None, prev, **p)[0][..., 6] > 1).sum() > 20, "pixels that keep history: the clamp's work"
            for blk in BLOCKS:
                _call_clamped(qr, rm, scn, col[None], rec[None], None, tuple(a[None] for a in prev), None, p, rm.clamp_stops(*blk),
                              f"{w}x{h} ch {ch} {blk}")
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_views_and_rows_do_not_leak(qr, rays_mod):
    """a view alone and as the middle of three whose neighbours hold other colours gives the same bits; the frame is 35 wide, so
    that the second tile's halo would find the next row's pixels in flat memory"""
    rm = rays_mod
    w, h, ch = 35, 11, 3
    scn = qr.Scene(load_blob("demo01_160"))
    try:
        frames = [_scalar_frame(w, h, ch, 300 + j) for j in range(3)]
        for j in (0, 2):
            frames[j][0][...] = frames[j][0] * F(8.0) + F(100.0)
        col, rec = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
        prev = tuple(np.stack([f[2][k] for f in frames]) for k in range(3))
        p = rm.reproject_stops(plane_max=2.0 ** -4)
        for blk in BLOCKS:
            c = rm.clamp_stops(*blk)
            three = _call_clamped(qr, rm, scn, col, rec, None, prev, None, p, c, f"three views {blk}")
            alone = _call_clamped(qr, rm, scn, col[1:2], rec[1:2], None, tuple(a[1:2] for a in prev), None, p, c, f"view 1 alone {blk}")
            _same(alone[0], three[1], "a view alone and as the middle of three")
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_null_block_is_the_moving_call(qr, rays_mod):
    """clamp = NULL, moved_out = NULL against qr_reproject_moving_async on the same GPU and the same device buffers: every word
    of every output, in 3 and 4 channels, with and without a table"""
    import torch
    rm = rays_mod
    w, h = 67, 45
    scn = qr.Scene(load_blob("demo01_160"))
    L = qr.lib()
    vp = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())
    try:
        for ch in (3, 4):
            col, rec, var, prev = TR._synthetic(w, h, 5 + ch, ch)
            rec, prev = TM._synthetic_ids(rec, prev, 9 + ch)
            d = [_dev(scn, a) for a in (col, rec, var)]
            pd = [_dev(scn, a) for a in prev]
            m = TM._tables(3 + ch)[0][1]
            md = _dev(scn, m)
            for table in (False, True):
                mt, nm = (vp(md), len(m)) if table else (None, 0)
                cp = TR._params(qr, ch, rm.reproject_stops(plane_max=2.0 ** -5, demodulate=True))
                outs = [[torch.full(s, 7.5, dtype=torch.float32, device=d[0].device) for s in ((2, h, w, 8), (2, h, w, ch), (2, h, w), (2, h, w, 2))]
                        for _ in range(2)]
                assert L.qr_reproject_moving_async(scn._h, vp(d[0]), vp(d[1]), vp(d[2]), vp(pd[0]), vp(pd[1]), vp(pd[2]), mt, nm, 2, w, h,
                                                   ctypes.byref(cp), *(vp(o) for o in outs[0]), None) == 0
                assert L.qr_reproject_clamped_async(scn._h, vp(d[0]), vp(d[1]), vp(d[2]), vp(pd[0]), vp(pd[1]), vp(pd[2]), mt, nm, 2, w, h,
                                                    ctypes.byref(cp), None, *(vp(o) for o in outs[1]), None, None) == 0
                torch.cuda.synchronize()
                for a, b in zip(*outs):
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"ch {ch} table {table}"
                assert not (outs[1][0] == 7.5).any().item()
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_streams_and_python(qr, rays_mod):
    """Scene.reproject(clamp=, moved=) is the C call; the same call twice and a call on a side stream give the same bytes; a
    tensor to fill; what Python refuses on the device"""
    import torch
    rm = rays_mod
    base_name, (w, h) = "demo02_160", SIZES[1]
    stops, x = _chain_inputs(qr, rm, base_name, w, h)
    p, c = rm.reproject_stops(**stops), rm.clamp_stops("variance", 2, 0.75, short_len=2)
    scn = qr.Scene(load_blob("demo01_160"))
    try:
        col, rec, var = np.ascontiguousarray(x["gather"][1:2, ..., :3]), x["hits"][1:2], x["var"][1:2]
        first = rm.reproject_pass(np.ascontiguousarray(x["gather"][0:1, ..., :3]), x["hits"][0:1], None, None, **p)[0]
        prev, m = (x["view"][None], x["hits"][0:1], first), x["motion"][1]
        hist = _call_clamped(qr, rm, scn, col, rec, var, prev, m, p, c, "B against A")
        want = rm.reproject_pass(col, rec, var, prev, motion=m, clamp=c, moved=True, **p)
        assert (want[4] > 0).any()
        dev = [_dev(scn, a) for a in (col, rec, var)]
        pd, md = tuple(_dev(scn, a) for a in prev), _dev(scn, m)
        a = scn.reproject(dev[0], dev[1], pd, dev[2], coords=True, motion=md, clamp=c, moved=True, **stops)
        b = scn.reproject(dev[0], dev[1], pd, dev[2], coords=True, motion=md, clamp=c, moved=True, **stops)
        assert len(a) == 5 and tuple(a[4].shape) == (1, h, w) and a[4].dtype == torch.float32
        for k in range(5):
            _same(_host(a[k]), want[k], f"Scene.reproject(clamp=, moved=True) output {k}")
        _same(_host(a[0]), hist, "... is the C call")
        for s, t in zip(a, b):
            assert torch.equal(s.view(torch.int32), t.view(torch.int32)), "the same call twice"
        fill = torch.full((1, h, w), 7.5, device=dev[0].device)
        short = scn.reproject(dev[0], dev[1], pd, dev[2], motion=md, clamp=c, moved=fill, **stops)
        assert len(short) == 4 and short[3] is fill and torch.equal(fill.view(torch.int32), a[4].view(torch.int32))
        quiet = scn.reproject(dev[0], dev[1], pd, dev[2], motion=md, clamp=c, **stops)
        assert len(quiet) == 3 and torch.equal(quiet[0].view(torch.int32), a[0].view(torch.int32))
        plain = scn.reproject(dev[0], dev[1], pd, dev[2], motion=md, **stops)
        assert len(plain) == 3 and not torch.equal(plain[0].view(torch.int32), a[0].view(torch.int32)), "the block matters"
        side, ready, done = torch.cuda.Stream(), torch.cuda.Event(), torch.cuda.Event()
        c2 = dev[0].clone()
        ready.record()
        side.wait_event(ready)
        s = scn.reproject(c2, dev[1], pd, dev[2], coords=True, stream=side, motion=md, clamp=c, moved=True, **stops)
        done.record(side)
        torch.cuda.current_stream().wait_event(done)
        for u, t in zip(s, a):
            assert torch.equal(u.view(torch.int32), t.view(torch.int32)), "a side stream"
        side.synchronize()
        for bad in (fill.cpu(), fill.double(), fill[0], fill[:, :, :5], "m", 3):
            with pytest.raises(ValueError, match="moved must be"):
                scn.reproject(dev[0], dev[1], pd, dev[2], clamp=c, moved=bad, **stops)
        with pytest.raises(ValueError, match="radius must be"):
            scn.reproject(dev[0], dev[1], pd, dev[2], clamp=dict(c, radius=9), **stops)
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_temporal_accumulator_with_a_clamp(qr, rays_mod):
    """Temporal(clamp=).step(motion=, scene=) over 4 animated frames of two views, a fresh Scene per frame and the earlier ones
    closed, against rays.temporal(clamp=); a clone taken midway goes on alike; Scene.denoise of its output equals rays.denoise"""
    import torch
    rm = rays_mod
    base_name, (w, h) = "demo02_160", SIZES[0]
    v, off, plane_max = _view(qr, rm, base_name, w, h)
    views = np.stack([v, rm.jitter_view(v, 0.5, -0.25)])
    frames = _frames(qr, base_name, 3)
    kw = dict(plane_max=plane_max, off=off, demodulate=True, var_min_len=2)
    c = rm.clamp_stops("variance", 1, 1.0, short_len=1)
    ref = rm.temporal(2, w, h, 3, clamp=c, **kw)
    plain = rm.temporal(2, w, h, 3, **kw)
    acc, before, differs = None, None, 0
    for k, (blob, m) in enumerate(frames):
        scn = qr.Scene(blob, ray_queries=True)
        if acc is None:
            acc = scn.temporal(2, w, h, 3, clamp=c, **kw)
            assert acc.clamp == c
        if k == 2:
            acc = acc.clone()
            assert acc.clamp == c
        vt = _dev(scn, views)
        hits = scn.view_hits(vt, w, h)
        spin = torch.from_numpy(rm.spins((2, h, w), 7 + k)).to(vt.device)
        gat, _ = scn.view_gather(vt, torch.from_numpy(rm.cosine_dirs(4)).to(vt.device), w, h, eps=TA.EPS, reach=TA.REACH, frame=True, spin=spin)
        col = gat[..., :3].contiguous()
        var = _dev(scn, np.random.default_rng(k).uniform(0.0, 0.1, (2, h, w)).astype(F))
        got = acc.step(col, hits, vt, var, motion=None if m is None else _dev(scn, m), scene=scn)
        want = ref.step(_host(col), _host(hits), views, _host(var), motion=m)
        other = plain.step(_host(col), _host(hits), views, _host(var), motion=m)
        _same(_host(got[0]), want[0], f"frame {k} colour"), _same(_host(got[1]), want[1], f"frame {k} variance")
        _same(_host(acc.history), ref.history, f"frame {k} history")
        differs += int((_bits(other[0]) != _bits(want[0])).sum())
        if k == len(frames) - 1:
            dkw = dict(passes=2, plane=plane_max, luma=4.0, normal_power=8)
            clean, cvar = scn.denoise(got[0], hits, got[1], **dkw)
            wc, wv = rm.denoise(want[0], want[1], _host(hits), **dkw)
            _same(_host(clean), wc, "denoise of the accumulated colour"), _same(_host(cvar), wv, "denoise of the accumulated variance")
        if before is not None:
            before.close()
        before = scn
    before.close()
    assert differs > 0, "the block matters"


@pytest.mark.gpu
def test_gpu_refusals(qr, rays_mod):
    """every QR_ERR_ARG of the block with its text, the shared checks through the new entry point (they come first), the
    sentinel-filled outputs untouched after all of them; n_views = 0 is QR_OK; then calls that are served"""
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
    hout, cout, vout, xout, mout = s75(px * 8), s75(px * 4), s75(px), s75(px * 2), s75(px)
    vp = lambda x, off=0: ctypes.c_void_p(None if x is None else x.data_ptr() + off)
    nan, inf = float("nan"), float("inf")
    base, good = rm.reproject_stops(plane_max=0.5), dict(flags=2, radius=1, gamma=1.0, short_len=1.0)

    def call(s=scn._h, ci=vp(col), hi=vp(hits), mt=vp(table), nm=4, n=n, w=w, ho=vp(hout), mo=vp(mout), null_c=False, channels=3,
             reserved=(0, 0, 0, 0), text=None, **ck):
        p = TR._params(qr, channels, dict(base, **{k: ck.pop(k) for k in list(ck) if k in base and k != "flags"}))
        c = _block(qr, dict(good, **ck), reserved)
        rc = L.qr_reproject_clamped_async(s, ci, hi, vp(var), vp(views), vp(hprev), vp(hin), mt, nm, n, w, h, ctypes.byref(p),
                                          None if null_c else ctypes.byref(c), ho, vp(cout), vp(vout), vp(xout), mo, None)
        if text is not None:
            assert rc == ARG and text in L.qr_last_error().decode(), (rc, L.qr_last_error().decode(), text)
        return rc

    none = vp(None)
    one_of = "exactly one of the two"
    call(flags=0, text=one_of), call(flags=3, text=one_of), call(flags=4, text=one_of), call(flags=7, text=one_of)
    call(flags=8 | 1, text="unknown clamp flags"), call(flags=0x80000002, text="unknown clamp flags")
    for k in range(4):
        call(reserved=tuple(int(j == k) for j in range(4)), text="the reserved words of the clamp block must be 0")
    for bad in (0, 4, -1, 1 << 30):
        call(radius=bad, text="radius must be 1..3")
    for flags in (1, 2):
        for bad in (-0.5, nan, -inf):
            call(flags=flags, gamma=bad, text="gamma must be 0 or more")
    call(short_len=nan, text="short_len must not be NaN"), call(flags=1, short_len=nan, text="short_len must not be NaN")
    for bad in (0.5, 0.0, -1.0, -inf, nan):
        call(flags=6, short_len=bad, text="short_len must not be NaN, and 1 or more with QR_CLAMP_SHORTEN")
    for off in (1, 2, 3):
        call(mo=vp(mout, off), text="moved_out must be 4-byte aligned")
    call(null_c=True, text="moved_out needs a clamp block")
    # the shared checks, first and in their order
    call(s=None, flags=0, text="null"), call(ci=none, radius=0, text="null argument"), call(channels=5, flags=0, text="channels must be 3 or 4")
    call(mt=none, flags=0, text="motion_dev and n_motion go together"), call(ho=vp(hin), radius=9, text="hist_out cannot be hist_in")
    call(plane_max=-1.0, gamma=nan, text="plane_max and alb_floor must be above 0")
    for off in (4, 8, 12):
        assert call(hi=vp(hits, off)) == ARG and call(mt=vp(table, off), nm=3) == ARG
    assert call(w=0) == ARG and call(n=-1) == ARG
    assert call(n=0) == 0 and call(n=0, ci=none, hi=none, ho=none) == 0
    torch.cuda.synchronize()
    for t in (hout, cout, vout, xout, mout):
        assert (t == 7.5).all().item(), "a refused call wrote something"
    # served: without moved_out, without a table, both modes, every radius, SHORTEN, short_len below 1 without it, no block at all
    assert call() == 0 and call(mo=none) == 0 and call(mt=none, nm=0) == 0 and call(null_c=True, mo=none) == 0
    for r in (1, 2, 3):
        assert call(flags=1, radius=r) == 0 and call(flags=6, radius=r, short_len=1.0, gamma=0.0) == 0
    assert call(short_len=-inf, gamma=inf) == 0 and call(channels=4, flags=5, short_len=inf) == 0
    torch.cuda.synchronize()
    assert (hout[:px * 8] != 7.5).all().item() and (hout[px * 8:] == 7.5).all().item()
    assert (mout[:px] != 7.5).all().item() and (mout[px:] == 7.5).all().item()
    scn.close()


# once more through the guarded diagnostic build (make guard), as tests/test_reproject_moving.py does it: the library is chosen
# when the package is imported, hence the child process: this file run as a script.

def _guard_child():
    from qr_loader import load_package
    qr = load_package()
    assert qr.LIB_PATH == GUARD_LIB, qr.LIB_PATH
    rm = _rays_mod()
    base_name, (w, h) = "demo02_160", SIZES[1]
    stops, x = _chain_inputs(qr, rm, base_name, w, h)
    scn = qr.Scene(load_blob("demo01_160"))
    _run_clamped_chain(qr, rm, scn, x, stops, f"guard {base_name}", list(zip(BLOCKS, COMBOS))[:4])
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
