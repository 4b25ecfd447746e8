"""Temporal reprojection (include/qrhip.h qr_reproject_views_async; Scene.reproject, Scene.temporal; rays.project_to_view,
rays.reproject_pass, rays.reproject_stops, rays.temporal).

The call is a pure function of its inputs and its arithmetic is pinned to the operation, so there is no oracle: the CPU tests
check the numpy statement against cases worked out by hand (a dyadic camera on which every weight is exact, a scalar restatement
of the header's text, the running mean, each way an entry starts afresh) and against real hit records of the oracle; the GPU
tests check every word the kernel writes against the numpy statement on the inputs copied back from the device.  Every
comparison is bit for bit, except that two NaNs count as equal whatever their sign and payload: a NaN the text WRITES is
0x7FC00000 and is checked as such, a NaN an operation computes is the processor's."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import test_atrous as TA
import test_hit_records as THR
import test_pt_views as TPV
from conftest import ROOT
from test_atrous import SENTINEL, _bits, _dev, _flat, _host
from test_pt_views import _base, _cams, _rays_mod

F = np.float32
ARG = -1
GUARD_LIB = TPV.GUARD_LIB
ASM = TPV.ASM
REAL_SCENES = ["patched:demo02_160_gf_aa4", "pt:test18_160_pt"]
REAL_CAMERA = {"patched:demo02_160_gf_aa4": -1, "pt:test18_160_pt": 1}      # the scene's own camera / the seeded camera 1
REAL_SIZES = [(64, 64), (67, 45), (9, 130)]                                   # (w, h)
SYNTH_SIZES = [(1, 1), (9, 130), (67, 45)]
QNAN = 0x7FC00000
FIELDS = ("flags", "off_x", "off_y", "normal_min", "plane_max", "min_weight", "alpha_min", "alpha_mom_min", "max_len", "var_min_len",
          "unknown", "alb_floor")


@pytest.fixture(scope="module")
def rays_mod():
    return _rays_mod()


def _same(got, want, where):
    """every word equal, two NaNs equal"""
    got, want = np.asarray(got, dtype=F), np.asarray(want, dtype=F)
    assert got.shape == want.shape, f"{where}: shape {got.shape} against {want.shape}"
    bad = (_bits(got) != _bits(want)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), f"{where}: {int(bad.sum())} of {bad.size} words differ, first {np.argwhere(bad)[:4].tolist()}"


# ------------------------------------------------------------------------------------------------- names and sizes

def test_symbols_constants_and_header(qr, rays_mod):
    hdr = open(os.path.join(ROOT, "include", "qrhip.h")).read()
    assert "qr_reproject_views_async" in qr.ABI_SYMBOLS and "qr_reproject_views_async(" in hdr
    assert hasattr(qr.lib(), "qr_reproject_views_async") and len(qr.lib().qr_reproject_views_async.argtypes) == 16
    assert ctypes.sizeof(qr.ReprojectParams) == 64 and "typedef struct qr_reproject_params" in hdr
    assert [n for n, _ in qr.ReprojectParams._fields_] == ["channels"] + list(FIELDS) + ["reserved"]
    assert qr.REPROJ_DEMODULATE == 1 == rays_mod.REPROJ_DEMODULATE and "#define QR_REPROJ_DEMODULATE  1u" in hdr
    assert _bits(rays_mod.REPROJ_NAN) == QNAN
    for text in ("sw += b", "len = sl / sw + 1.0f", "front = (0 < den && 0 < det) || (den < 0 && det < 0)", "1.0f <= len_q"):
        assert text in hdr, text
    for m in ("reproject", "temporal"):
        assert callable(getattr(qr.Scene, m))
    for m in ("step", "reset", "clone"):
        assert callable(getattr(qr.Temporal, m)) and callable(getattr(rays_mod.Temporal, m))
    for m in ("history", "length"):
        assert isinstance(getattr(qr.Temporal, m), property) and isinstance(getattr(rays_mod.Temporal, m), property)
    for m in ("reproject_stops", "project_to_view", "reproject_pass", "temporal"):
        assert callable(getattr(rays_mod, m))


def test_kernels_in_resource_check():
    """both instances are held to a budget by the build's own check, and the build's assembly meets it"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import check_kernel_resources as ck
    finally:
        sys.path.pop(0)
    for frag in ("19qr_reproject_kernelILi3EE", "19qr_reproject_kernelILi4EE"):
        vg, spill, scratch = ck.LIMITS[frag]
        assert vg <= 128 and spill == 0 and scratch == 0 and ck.LDS_LIMITS[frag] == 0
    if os.path.exists(ASM):
        mine = [k for k in ck.kernels(ASM) if "qr_reproject_kernel" in k["name"]]
        assert len(mine) == 2
        for k in mine:
            frag = next(f for f in ck.LIMITS if f in k["name"])
            assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] == 0
            assert k["vgpr_count"] <= ck.LIMITS[frag][0]


# ------------------------------------------------------------------------------------------------- the projection

def _projection_cases(rm):
    """[(view, w, h, points float32 [N, 3], pixel coordinates [N, 2], in front)]: points along the cameras' own rays at several
    t, and the same rays followed backwards, behind the eye"""
    blob = _base(REAL_SCENES[1])
    assert TPV._fsaa(blob) == 0
    out = []
    for (w, h) in ((67, 45), (9, 130)):
        for eye, target, up, fov in (((0.5, -2.0, 1.25), (3.0, 4.0, -1.0), (0.0, 0.0, 1.0), 60.0),
                                    ((-40.0, 11.0, 7.0), (-41.0, 10.0, 7.5), (0.1, 1.0, 0.0), 35.0),
                                    ((1e3, 2e3, -5e2), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 100.0)):
            v = rm.look_at(eye, target, up, fov, w, h)
            r = rm.view_rays(v, w, h, blob)
            ys, xs = np.mgrid[0:h, 0:w]
            px = np.stack([xs.ravel(), ys.ravel()], -1).astype(np.float64)
            for t in (0.5, 1.0, 7.3, 1e2, -0.5, -7.3):
                out.append((v, w, h, (r[:, 0:3] + r[:, 4:7] * F(t)).astype(F), px, t > 0))
    return out


PROJECTION_WORST = 1.533e-4     # pixels: the measured worst case of the test below (see its docstring)


def test_projection_against_float64(rays_mod):
    """project_to_view in float32 against the same text evaluated in float64, on look_at cameras at 67x45 and 9x130, for points
    along the cameras' own view_rays at t = 0.5, 1, 7.3, 100 and behind the eye: `front` is right everywhere, the float64
    evaluation recovers the pixel coordinates of the float32 points, and the float32 one stays within 4x the worst case this
    comparison measured when the test was written.  Measured: 1.533e-4 pixel, on the camera 2 000 units from the origin at
    9x130 (its very oblique rows; pos - org cancels three digits); 5.3e-5 at 9x130 on the cameras near the origin and 2.0e-5 at
    67x45 on the far one.  PROJECTION_WORST is the first figure."""
    worst = 0.0
    for v, w, h, pts, px, front in _projection_cases(rays_mod):
        xy32, f32 = rays_mod.project_to_view(v, pts)
        xy64, f64 = rays_mod.project_to_view(v, pts, dtype=np.float64)
        assert xy32.dtype == np.float32 and xy64.dtype == np.float64
        assert (f32 == front).all() and (f64 == front).all()
        if np.abs(v[0:3]).max() < 100:                   # points the float32 grid resolves to a small part of a pixel
            assert np.abs(xy64 - px).max() < 5e-3, "the float64 text recovers the pixels of the float32 points"
        err = float(np.abs(xy32.astype(np.float64) - xy64).max())
        print(f"{w}x{h} org {v[0:3].tolist()}: {err:.3e}")
        worst = max(worst, err)
    print(f"worst float32 - float64 projection error: {worst:.3e} pixel")
    assert worst <= 4 * PROJECTION_WORST
    # the offset of the records' rays is taken off
    v, w, h, pts, px, _ = _projection_cases(rays_mod)[1]
    xy, _ = rays_mod.project_to_view(v, pts, off=(0.25, -0.5), dtype=np.float64)
    assert np.abs(xy - (px - np.array([0.25, -0.5]))).max() < 1e-3


# ------------------------------------------------------------------------------------------------- the dyadic camera

S = 2.0 ** -6
W16 = H16 = 16


def _dyadic_view(w=W16, h=H16):
    """org = 0, hor = (s, 0, 0), ver = (0, s, 0), dir = (-w/2 s, -h/2 s, 1), s = 2^-6: the point ((fx - w/2) s, (fy - h/2) s, 1)
    projects to (fx, fy) exactly"""
    v = np.zeros(16, dtype=F)
    v[4:7], v[7] = (-w / 2 * S, -h / 2 * S, 1.0), np.finfo(F).max
    v[8], v[13] = S, S
    return v


def _plane(w=W16, h=H16, dx=0.0, dy=0.0, sid=2, alb=0.5):
    """records of the plane z = 1 seen by the dyadic camera: pixel (x, y) holds the point that projects to (x + dx, y + dy)"""
    r = _flat(h, w, nrm=(0.0, 0.0, -1.0), sid=sid, alb=alb)
    ys, xs = np.mgrid[0:h, 0:w]
    r[..., 0], r[..., 1], r[..., 2] = (xs + dx - w / 2) * S, (ys + dy - h / 2) * S, 1.0
    return r


def _history(h, w, seed, ch=3):
    rng = np.random.default_rng(seed)
    hist = rng.uniform(0.0, 1.0, (h, w, 8)).astype(F)
    hist[..., 6] = rng.integers(1, 9, (h, w)).astype(F)
    hist[..., 7] = 0.0
    if ch == 3:
        hist[..., 3] = 0.0
    return hist


def _pixel(rm, p, col, rec, var, prev, x, y):
    """the header's text for ONE pixel in scalar float32, written a second time: (entry [8], variance, coords [2])"""
    f = F
    h, w, ch = col.shape
    par = {k: f(p[k]) for k in FIELDS if k != "flags"}
    c = [f(col[y, x, k]) for k in range(ch)] + [f(0.0)] * (4 - ch)
    pid = int(rec[y, x].view(np.int32)[7])
    pos, nrm, alb = rec[y, x, 0:3], rec[y, x, 4:7], rec[y, x, 8:11]
    with np.errstate(all="ignore"):
        if int(p["flags"]) & 1 and pid >= 0:
            for k in range(3):
                c[k] = c[k] / (alb[k] if alb[k] > par["alb_floor"] else par["alb_floor"])
        lum = (c[0] * f(0.2126) + c[1] * f(0.7152)) + c[2] * f(0.0722)
        vfresh = par["unknown"] if var is None else var[y, x]
        nan = np.array([QNAN], dtype=np.uint32).view(F)[0]
        fresh = (np.array(c + [lum, lum * lum, f(1.0), f(0.0)], dtype=F), vfresh)
        if prev is None or pid < 0:
            return fresh + (np.array([nan, nan], dtype=F),)
        view, rq, hq = prev
        org, d, hor, ver = view[0:3], view[4:7], view[8:11], view[12:15]
        cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
        dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
        A, B, C = cross(hor, ver), cross(ver, d), cross(d, hor)
        det = dot(d, A)
        e = [pos[k] - org[k] for k in range(3)]
        den, nu, nv = dot(e, A), dot(e, B), dot(e, C)
        fx, fy = nu / den - par["off_x"], nv / den - par["off_y"]
        if not ((0 < den and 0 < det) or (den < 0 and det < 0)):
            return fresh + (np.array([nan, nan], dtype=F),)
        coords = np.array([fx, fy], dtype=F)
        if not (f(-1.0) < fx and fx < f(w) and f(-1.0) < fy and fy < f(h)):
            return fresh + (coords,)
        x0, y0 = np.floor(fx), np.floor(fy)
        wx, wy = fx - x0, fy - y0
        sw, sc, s1, s2, sl = f(0), [f(0)] * 4, f(0), f(0), f(0)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = int(x0) + i, int(y0) + j
                b = (wx if i else f(1.0) - wx) * (wy if j else f(1.0) - wy)
                if not (0 <= qx < w and 0 <= qy < h):
                    continue
                r, g = rq[qy, qx], hq[qy, qx]
                dd = [r[k] - pos[k] for k in range(3)]
                if (int(r.view(np.int32)[7]) == pid and f(1.0) <= g[6] and par["normal_min"] < dot(nrm, r[4:7])
                        and np.abs(dot(nrm, dd)) <= par["plane_max"] and 0 < b):
                    sw = sw + b
                    sc = [sc[k] + g[k] * b for k in range(4)]
                    s1, s2, sl = s1 + g[4] * b, s2 + g[5] * b, sl + g[6] * b
        if not par["min_weight"] < sw:
            return fresh + (coords,)
        ln = sl / sw + f(1.0)
        ln = ln if ln < par["max_len"] else par["max_len"]
        a = f(1.0) / ln
        ac = a if a > par["alpha_min"] else par["alpha_min"]
        am = a if a > par["alpha_mom_min"] else par["alpha_mom_min"]
        out = [(sc[k] / sw) * (f(1.0) - ac) + c[k] * ac for k in range(ch)] + [f(0.0)] * (4 - ch)
        m1 = (s1 / sw) * (f(1.0) - am) + lum * am
        m2 = (s2 / sw) * (f(1.0) - am) + (lum * lum) * am
        v = vfresh
        if par["var_min_len"] <= ln:
            v = m2 - m1 * m1
            v = v if 0 < v else f(0.0)
        return np.array(out + [m1, m2, ln, f(0.0)], dtype=F), v, coords


def _against_scalar(rm, p, col, rec, var, prev, where):
    """reproject_pass on one view against _pixel at every pixel"""
    got = rm.reproject_pass(col, rec, var, prev, **p)
    h, w, ch = col.shape
    for y in range(h):
        for x in range(w):
            e, v, xy = _pixel(rm, p, col, rec, var, prev, x, y)
            _same(got[0][y, x], e, f"{where} entry ({x}, {y})")
            _same(got[1][y, x], e[:ch], f"{where} colour ({x}, {y})")
            _same(got[2][y, x], v, f"{where} variance ({x}, {y})")
            _same(got[3][y, x], xy, f"{where} coords ({x}, {y})")
    return got


def _dyadic_case(rm, dx, dy, ch=3, seed=5, **stops):
    rng = np.random.default_rng(seed)
    col = rng.uniform(0.0, 1.0, (H16, W16, ch)).astype(F)
    p = rm.reproject_stops(plane_max=2.0 ** -4, **stops)
    prev = (_dyadic_view(), _plane(), _history(H16, W16, seed + 1, ch))
    return p, col, _plane(dx=dx, dy=dy), prev


@pytest.mark.parametrize("ch", [3, 4])
def test_exact_bilinear_blend(rays_mod, ch):
    """records made so that (fx, fy) is exactly (x + 0.25, y + 0.75): the four weights are 3/16, 1/16, 9/16, 3/16, they sum to
    exactly 1, and the entry is the blend written out by hand; the whole frame agrees with the scalar restatement, edges with
    two taps off the frame included"""
    rm = rays_mod
    p, col, rec, prev = _dyadic_case(rm, 0.25, 0.75, ch)
    hist, out, var, xy = _against_scalar(rm, p, col, rec, None, prev, "shift (0.25, 0.75)")
    ys, xs = np.mgrid[0:H16, 0:W16]
    assert (xy[..., 0] == xs + F(0.25)).all() and (xy[..., 1] == ys + F(0.75)).all(), "the camera is exact"
    assert xy[3, 5, 0] == 5.25 and xy[3, 5, 1] == 3.75
    hq = prev[2]
    b = [F(0.75) * F(0.25), F(0.25) * F(0.25), F(0.75) * F(0.75), F(0.25) * F(0.75)]
    taps = [hq[3, 5], hq[3, 6], hq[4, 5], hq[4, 6]]
    sw = ((b[0] + b[1]) + b[2]) + b[3]
    assert sw == 1.0
    sl = ((taps[0][6] * b[0] + taps[1][6] * b[1]) + taps[2][6] * b[2]) + taps[3][6] * b[3]
    ln = sl / sw + F(1.0)
    assert 2.0 <= ln <= 9.0 and hist[3, 5, 6] == ln
    a = F(1.0) / ln
    ac, am = max(a, F(0.05)), max(a, F(0.2))
    for k in range(ch):
        sc = ((F(0) + taps[0][k] * b[0] + taps[1][k] * b[1]) + taps[2][k] * b[2]) + taps[3][k] * b[3]
        assert _bits(hist[3, 5, k]) == _bits((sc / sw) * (F(1.0) - ac) + col[3, 5, k] * ac)
        assert _bits(out[3, 5, k]) == _bits(hist[3, 5, k])
    lum = (col[3, 5, 0] * F(0.2126) + col[3, 5, 1] * F(0.7152)) + col[3, 5, 2] * F(0.0722)
    s1 = ((taps[0][4] * b[0] + taps[1][4] * b[1]) + taps[2][4] * b[2]) + taps[3][4] * b[3]
    assert _bits(hist[3, 5, 4]) == _bits((s1 / sw) * (F(1.0) - am) + lum * am)
    assert _bits(hist[3, 5, 7]) == 0 and (ch == 4 or _bits(hist[3, 5, 3]) == 0)
    assert (hist[H16 - 1, :, 6] > 1).all(), "the last row keeps history through its two taps inside the frame"


def test_zero_shift_takes_one_tap(rays_mod):
    """a shift of exactly 0: wx == wy == 0, only the i == 0, j == 0 tap counts, and sc / sw is the tap's entry itself"""
    rm = rays_mod
    p, col, rec, prev = _dyadic_case(rm, 0.0, 0.0, alpha_min=0.0, alpha_mom_min=0.0)
    taps = []
    hist, _, _, xy = rm.reproject_pass(col, rec, None, prev, taps=taps, **p)
    assert len(taps) == 4 and taps[0][0].all() and not any(t[0].any() for t in taps[1:])
    assert (taps[0][1] == 1.0).all() and (hist[..., 6] == prev[2][..., 6] + 1).all()
    a = F(1.0) / hist[..., 6]
    _same(hist[..., 0:3], prev[2][..., 0:3] * (F(1.0) - a)[..., None] + col * a[..., None], "one tap")
    _against_scalar(rm, p, col, rec, None, prev, "zero shift")


def test_running_mean(rays_mod):
    """zero shift, N frames, alpha_min = alpha_mom_min = 0 and a large max_len: len == N and the colour is the running mean in
    the pinned form m * (1 - 1/k) + c * (1/k); from var_min_len on the variance is max(0, m2 - m1^2), before it `unknown`; with
    max_len = 4 the length stops at 4 and the blend is exponential with 1/4 from there"""
    rm = rays_mod
    rng = np.random.default_rng(9)
    n = 7
    cols = rng.uniform(0.0, 1.0, (n, 1, H16, W16, 3)).astype(F)
    rec, view = _plane()[None], _dyadic_view()[None]
    for max_len in (1e9, 4.0):
        acc = rm.temporal(1, W16, H16, 3, plane_max=2.0 ** -4, alpha_min=0.0, alpha_mom_min=0.0, max_len=max_len, var_min_len=3,
                          unknown=0.125)
        mean = m1 = m2 = None
        for k in range(1, n + 1):
            c = cols[k - 1]
            lum = (c[..., 0] * F(0.2126) + c[..., 1] * F(0.7152)) + c[..., 2] * F(0.0722)
            out, var = acc.step(c, rec, view)
            ln = F(min(k, max_len))
            a = F(1.0) / ln
            if k == 1:
                mean, m1, m2 = c, lum, lum * lum
            else:
                mean = mean * (F(1.0) - a) + c * a
                m1, m2 = m1 * (F(1.0) - a) + lum * a, m2 * (F(1.0) - a) + (lum * lum) * a
            assert (acc.length == ln).all(), (k, max_len)
            _same(out, mean, f"running mean after {k} frames, max_len {max_len}")
            _same(acc.history[..., 4], m1, "first moment")
            _same(acc.history[..., 5], m2, "second moment")
            if k < 3:
                assert (var == F(0.125)).all()
            else:
                v = m2 - m1 * m1
                _same(var, np.where(0 < v, v, F(0.0)), f"variance after {k} frames")
                assert (var >= 0).all()
        assert acc.frames == n


def _fresh_at(rm, p, col, rec, prev, x, y, keeps=False, where=""):
    hist, out, var, xy = rm.reproject_pass(col, rec, None, prev, **p)
    e, v, c = _pixel(rm, p, col, rec, None, prev, x, y)
    _same(hist[y, x], e, where + " against the scalar text")
    _same(xy[y, x], c, where + " coords")
    if keeps:
        assert hist[y, x, 6] > 1, where + ": history should be kept"
    else:
        lum = (col[y, x, 0] * F(0.2126) + col[y, x, 1] * F(0.7152)) + col[y, x, 2] * F(0.0722)
        _same(hist[y, x], np.array(list(col[y, x]) + [0.0] * (4 - col.shape[2]) + [lum, lum * lum, 1.0, 0.0], dtype=F), where + ": a fresh entry")
        _same(out[y, x], col[y, x], where + ": the colour as read")
        assert var[y, x] == p["unknown"]
    return xy[y, x]


def test_fresh_entries(rays_mod):
    """each reason alone makes pixel (5, 3) start afresh (len == 1, the colour as read, bit for bit), and its nearest
    counterpart keeps history"""
    rm = rays_mod
    x, y = 5, 3
    taps = [(3, 5), (3, 6), (4, 5), (4, 6)]                 # (row, column) of the four taps of (5.25, 3.75)
    nan, inf = F(np.nan), F(np.inf)

    def case(where, keeps=False, cur=None, old=None, hist=None, **stops):
        p, col, rec, prev = _dyadic_case(rm, 0.25, 0.75, **stops)
        view, rq, hq = prev[0], prev[1].copy(), prev[2].copy()
        if cur:
            cur(rec)
        for t in taps:
            if old:
                old(rq[t])
            if hist:
                hist(hq[t])
        return _fresh_at(rm, p, col, rec, (view, rq, hq), x, y, keeps, where)

    def set_id(r, v):
        r.view(np.int32)[..., 7] = v

    case("untouched", keeps=True)
    case("another id", cur=lambda r: set_id(r[y, x], 4))
    case("another id in the previous frame", old=lambda r: set_id(r, 4))
    case("a previous miss", old=lambda r: set_id(r, -1))
    case("a flipped normal", cur=lambda r: r[y, x].__setitem__(slice(4, 7), (0.0, 0.0, 1.0)))
    case("a normal at a dot of 0.9", old=lambda r: r.__setitem__(slice(4, 7), (0.0, F(np.sqrt(1 - 0.81)), F(-0.9))))
    case("a normal at a dot of 0.9, normal_min below it", keeps=True, normal_min=0.89,
         old=lambda r: r.__setitem__(slice(4, 7), (0.0, F(np.sqrt(1 - 0.81)), F(-0.9))))
    above = np.nextafter(F(1.0625), F(2.0))
    assert above - F(1.0) > F(2.0 ** -4) and F(1.0625) - F(1.0) == F(2.0 ** -4)
    case("a plane offset just above plane_max", old=lambda r: r.__setitem__(2, above))
    case("a plane offset at plane_max", keeps=True, old=lambda r: r.__setitem__(2, F(1.0625)))
    case("a plane offset just below plane_max", keeps=True, old=lambda r: r.__setitem__(2, np.nextafter(F(1.0625), F(0.0))))
    case("a plane offset below, just above plane_max", old=lambda r: r.__setitem__(2, np.nextafter(F(0.9375), F(0.0))))
    for name, fx, fy, inside in (("left", -1.0, 3.75, -0.5), ("right", 16.0, 3.75, 15.5), ("above", 5.25, -1.0, -0.5), ("below", 5.25, 16.0, 15.5)):
        def move(r, fx=fx, fy=fy):
            r[y, x, 0], r[y, x, 1] = (fx - W16 / 2) * S, (fy - H16 / 2) * S
        xy = case(f"a projection outside the frame, {name}", cur=move)
        assert (xy == (fx, fy)).all(), "coords are given in front of the camera, whether inside the frame or not"
        fx2, fy2 = (inside, fy) if name in ("left", "right") else (fx, inside)
        # half a pixel inside the window: the two taps off the frame are skipped, the two on it keep history
        p, col, rec, prev = _dyadic_case(rm, 0.25, 0.75)
        move(rec, fx2, fy2)
        _fresh_at(rm, p, col, rec, prev, x, y, True, f"half a pixel inside, {name}")

    def behind(r):
        r[y, x, 2] = -1.0
    xy = case("a point behind the previous camera", cur=behind)
    assert (_bits(xy) == QNAN).all()
    case("len_q == 0", hist=lambda g: g.__setitem__(6, 0.0))
    case("len_q just below 1", hist=lambda g: g.__setitem__(6, np.nextafter(F(1.0), F(0.0))))
    for k in (0, 1, 2, 4, 5, 6):
        xy = case(f"NaN in word {k} of this frame's record", cur=lambda r, k=k: r[y, x].__setitem__(k, nan))
        assert (_bits(xy) == QNAN).all() == (k < 3), "a NaN position is not in front of anything"
        case(f"NaN in word {k} of the previous records", old=lambda r, k=k: r.__setitem__(k, nan))
    case("an infinite position", cur=lambda r: r[y, x].__setitem__(0, inf))
    case("an infinite previous position", old=lambda r: r.__setitem__(2, inf))
    # the weight: three taps closed by their id leave b = 1/16
    p, col, rec, prev = _dyadic_case(rm, 0.25, 0.75, min_weight=0.0625)
    rq = prev[1].copy()
    for t in (taps[0], taps[2], taps[3]):
        set_id(rq[t], 7)
    _fresh_at(rm, p, col, rec, (prev[0], rq, prev[2]), x, y, False, "sw == min_weight")
    p = rm.reproject_stops(plane_max=2.0 ** -4, min_weight=np.nextafter(F(0.0625), F(0.0)))
    _fresh_at(rm, p, col, rec, (prev[0], rq, prev[2]), x, y, True, "sw just above min_weight")
    # ... and the one open tap's history is kept exactly: s / sw with one term
    hist = rm.reproject_pass(col, rec, None, (prev[0], rq, prev[2]), **p)[0]
    g = prev[2][taps[1]]
    a = F(1.0) / (g[6] + F(1.0))
    ac, am = max(a, F(0.05)), max(a, F(0.2))
    _same(hist[y, x, 0:3], g[0:3] * (F(1.0) - ac) + col[y, x] * ac, "one open tap")
    assert hist[y, x, 6] == g[6] + 1
    lum = (col[y, x, 0] * F(0.2126) + col[y, x, 1] * F(0.7152)) + col[y, x, 2] * F(0.0722)
    _same(hist[y, x, 4:6], np.array([g[4] * (F(1.0) - am) + lum * am, g[5] * (F(1.0) - am) + (lum * lum) * am]), "one open tap's moments")


def test_miss_demodulate_and_first_frame(rays_mod):
    """a miss passes through undivided with NaN coords; DEMODULATE divides by the pixel's OWN albedo with the floor and the NaN
    rule and never the fourth channel; the first frame is the fresh rule everywhere, with var_in handed out"""
    rm = rays_mod
    p, col, rec, prev = _dyadic_case(rm, 0.25, 0.75, ch=4, demodulate=True, albedo_floor=1 / 64)
    rec.view(np.int32)[2, 2, 7] = -1
    rec[4, 4, 8:11] = (0.0, 1e-3, np.nan)
    rec[6, 6, 8:11] = (0.25, 2.0, -1.0)
    prev[1][...] = _plane(alb=0.125)                      # the previous frame's albedo is never looked at
    var = np.random.default_rng(2).uniform(0.01, 0.1, (H16, W16)).astype(F)
    for pv in (None, prev):
        hist, out, v, xy = _against_scalar(rm, p, col, rec, var, pv, f"demodulate, prev {pv is not None}")
        _same(out[2, 2], col[2, 2], "a miss is not divided")
        assert (_bits(xy[2, 2]) == QNAN).all() and hist[2, 2, 6] == 1 and v[2, 2] == var[2, 2]
    hist, out, v, xy = rm.reproject_pass(col, rec, var, None, **p)
    want = col.copy()
    a = np.where(rec[..., 8:11] > F(1 / 64), rec[..., 8:11], F(1 / 64))
    want[..., 0:3] = col[..., 0:3] / a
    want[2, 2] = col[2, 2]
    _same(out, want, "the first frame's colour")
    _same(out[4, 4, 0:3], col[4, 4, 0:3] / F(1 / 64), "zero, small and NaN albedo give the floor")
    _same(out[6, 6, 0:3], col[6, 6, 0:3] / np.array([0.25, 2.0, 1 / 64], dtype=F), "a negative albedo gives the floor")
    assert (out[..., 3] == col[..., 3]).all(), "the fourth channel is never divided"
    assert (hist[..., 6] == 1).all() and (hist[..., 7] == 0).all() and (_bits(xy) == QNAN).all()
    _same(v, var, "the first frame hands var_in out")
    lum = (want[..., 0] * F(0.2126) + want[..., 1] * F(0.7152)) + want[..., 2] * F(0.0722)
    _same(hist[..., 4], lum, "m1")
    _same(hist[..., 5], lum * lum, "m2")
    plain = rm.reproject_pass(col[..., :3].copy(), rec, None, None, **dict(p, unknown=F(0.5)))
    assert (_bits(plain[0][..., 3]) == 0).all() and (plain[2] == 0.5).all()
    # a [H, W, C] call is the [1, H, W, C] call
    one = rm.reproject_pass(col, rec, var, prev, **p)
    many = rm.reproject_pass(col[None], rec[None], var[None], tuple(a[None] for a in prev), **p)
    for a, b in zip(one, many):
        _same(a, b[0], "single view")


# ------------------------------------------------------------------------------------------------- real inputs

_PAIRS, _RECORDS = {}, {}


def _frame_of(v, fw, fh):
    org, d, hor, ver = (v[k:k + 3].astype(np.float64) for k in (0, 4, 8, 12))
    fwd = d + hor * (fw / 2) + ver * (fh / 2)
    return org, fwd / np.linalg.norm(fwd), -ver / np.linalg.norm(ver), hor / np.linalg.norm(hor)


def _cameras(rm, scene, w, h, depth):
    """four look_at cameras A, B, A', B' of a scene at w x h: A stands where the scene's chosen camera stands, B is 3 degrees
    to its right and 3 % of `depth` (the median hit distance of A) to the side and up -- at 64 pixels across 60 degrees about
    three pixels of turn and one to two of parallax, never a whole number --, A' and B' half a degree and 0.7 % further"""
    blob = _base(scene)
    fw, fh = TPV._size(blob)
    cam = REAL_CAMERA[scene]
    org, fwd, up, right = _frame_of(rm.view_of(blob) if cam < 0 else _cams(rm, scene)[cam], fw, fh)
    out = []
    for deg, frac in ((0.0, 0.0), (3.0, 0.03), (0.5, 0.007), (3.5, 0.037)):
        a = np.radians(deg)
        eye = org + (right + 0.5 * up) * (frac * depth)
        out.append(rm.look_at(eye, eye + fwd * np.cos(a) + right * np.sin(a), up, 60.0, w, h))
    return out


def _offsets(rm, blob):
    """the sub-pixel offset of the records' rays: the frame's hor_a[0], ver_a[0] under FSAA"""
    f, i = rm.frame_record(blob)
    return (float(f[10]), float(f[14])) if i[30] else (0.0, 0.0)


def _pair(rm, scene, w, h):
    """(cameras [4], off, plane_max): plane_max is one pixel's footprint at the median depth"""
    if (scene, w, h) not in _PAIRS:
        blob = _base(scene)
        helper = THR._helper()
        a = _cameras(rm, scene, 64, 64, 1.0)[0]
        rec = helper(blob, rm.view_rays(a, 64, 64, blob, 0))
        t = rec[:, 3][rec.view(np.int32)[:, 7] >= 0]
        depth = float(np.median(t))
        cams = _cameras(rm, scene, w, h, depth)
        _PAIRS[scene, w, h] = (cams, _offsets(rm, blob), float(F(depth * np.linalg.norm(cams[0][8:11]))))
    return _PAIRS[scene, w, h]


def _oracle_records(rm, scene, w, h):
    if (scene, w, h) not in _RECORDS:
        blob = _base(scene)
        cams = _pair(rm, scene, w, h)[0]
        _RECORDS[scene, w, h] = [THR._helper()(blob, rm.view_rays(v, w, h, blob, 0)).reshape(h, w, 12) for v in cams[:2]]
    return _RECORDS[scene, w, h]


@pytest.mark.parametrize("scene", REAL_SCENES)
def test_real_records_have_work_for_every_branch(rays_mod, scene):
    """the oracle's hit records of cameras A and B at 64x64: at least a quarter of B's hit pixels keep A's history, at least 16
    fall inside A's frame and are disoccluded all the same, at least 16 keep history through fewer than four taps; A's own
    records project onto A's own pixels.  These cameras are the GPU tests' inputs"""
    rm = rays_mod
    w = h = 64
    cams, off, plane_max = _pair(rm, scene, w, h)
    ra, rb = _oracle_records(rm, scene, w, h)
    p = rm.reproject_stops(plane_max=plane_max, off=off)
    col = np.random.default_rng(1).uniform(0.0, 1.0, (h, w, 3)).astype(F)
    h0 = rm.reproject_pass(col, ra, None, None, **p)[0]
    taps = []
    h1, _, _, xy = rm.reproject_pass(col, rb, None, (cams[0], ra, h0), taps=taps, **p)
    hit = rb.view(np.int32)[..., 7] >= 0
    kept = h1[..., 6] > 1
    ntaps = sum(t[0].astype(np.int32) for t in taps)
    with np.errstate(invalid="ignore"):
        inside = (xy[..., 0] > -1) & (xy[..., 0] < w) & (xy[..., 1] > -1) & (xy[..., 1] < h)
    assert not (kept & ~hit).any() and (h1[..., 6] <= 2).all()
    assert kept.sum() >= hit.sum() / 4, (int(kept.sum()), int(hit.sum()))
    assert (hit & inside & ~kept).sum() >= 16, int((hit & inside & ~kept).sum())
    assert (kept & (ntaps < 4)).sum() >= 16, int((kept & (ntaps < 4)).sum())
    assert len(np.unique(rb.view(np.int32)[..., 7][hit])) > 1
    own, front = rm.project_to_view(cams[0], ra[..., 0:3], off)
    hit_a = ra.view(np.int32)[..., 7] >= 0
    ys, xs = np.mgrid[0:h, 0:w]
    assert front[hit_a].all() and np.abs(own[hit_a] - np.stack([xs, ys], -1)[hit_a]).max() < 1e-3, "the offset is the records' rays'"


# ------------------------------------------------------------------------------------------------- accumulator, refusals

def test_temporal_is_its_chained_passes(rays_mod):
    """rays.temporal against reproject_pass chained by hand over two views with different cameras; reset() makes the next step
    a first frame; a clone continues on its own"""
    rm = rays_mod
    rng = np.random.default_rng(4)
    n = 5
    cols = rng.uniform(0.0, 1.0, (n, 2, H16, W16, 4)).astype(F)
    var = rng.uniform(0.01, 0.1, (n, 2, H16, W16)).astype(F)
    shifts = [(0.0, 0.0), (0.25, 0.75), (0.5, 0.125), (-0.375, 0.25), (3.0, -2.5)]
    recs = [np.stack([_plane(dx=dx, dy=dy), _plane(dx=-dy, dy=dx, sid=4)]) for dx, dy in shifts]
    views = np.stack([_dyadic_view(), _dyadic_view()])
    kw = dict(plane_max=2.0 ** -4, demodulate=True, var_min_len=2)
    acc = rm.temporal(2, W16, H16, 4, **kw)
    assert acc.history is None and acc.length is None and acc.frames == 0
    p = rm.reproject_stops(**kw)
    assert acc.params == p
    prev, twin = None, None
    for k in range(n):
        want = rm.reproject_pass(cols[k], recs[k], var[k], prev, **p)
        out, v = acc.step(cols[k], recs[k], views, var[k])
        _same(out, want[1], f"step {k} colour"), _same(v, want[2], f"step {k} variance")
        _same(acc.history, want[0], f"step {k} history")
        assert acc.length.base is not None and (acc.length == want[0][..., 6]).all() and acc.frames == k + 1
        prev = (views, recs[k], want[0])
        if k == 2:
            twin = acc.clone()
    assert (acc.length > 1).any()
    for k in (3, 4):
        out, v = twin.step(cols[k], recs[k], views, var[k])
    _same(out, want[1], "the clone, continued, arrives where the original did")
    assert twin.history is not acc.history and twin.frames == acc.frames
    before = acc.history.copy()
    twin.step(cols[0], recs[0], views)
    _same(acc.history, before, "a clone's step leaves the original alone")
    acc.reset()
    assert acc.history is None and acc.frames == 0
    out, v = acc.step(cols[1], recs[1], views, var[1])
    want = rm.reproject_pass(cols[1], recs[1], var[1], None, **p)
    _same(out, want[1], "after reset: a first frame"), _same(acc.history, want[0], "after reset")
    with pytest.raises(ValueError):
        acc.step(cols[1][..., :3], recs[1], views)
    with pytest.raises(ValueError):
        acc.step(cols[1], recs[1], views[:1])
    for bad in (dict(channels=5), dict(n_views=0), dict(width=0)):
        with pytest.raises(ValueError):
            rm.temporal(**dict(dict(n_views=1, width=4, height=4, channels=3), **bad))


def test_specification_refuses(rays_mod):
    rm = rays_mod
    p, col, rec, prev = _dyadic_case(rm, 0.25, 0.75)
    S_ = rm.reproject_stops
    d = S_()
    assert tuple(d) == FIELDS and d["flags"] == 0 and d["plane_max"] == np.inf and d["normal_min"] == F(0.9)
    assert (d["min_weight"], d["alpha_min"], d["alpha_mom_min"], d["max_len"], d["var_min_len"]) == (F(0.01), F(0.05), F(0.2), F(32), F(4))
    assert all(isinstance(d[k], np.float32) for k in FIELDS[1:])
    assert S_(demodulate=True, off=(0.25, -0.5))["flags"] == 1 and S_(off=(0.25, -0.5))["off_y"] == F(-0.5)
    assert S_(unknown=np.nan, min_weight=-0.0, normal_min=-np.inf, plane_max=np.inf, max_len=np.inf, alpha_min=0, alpha_mom_min=1)
    nan, inf = np.nan, np.inf
    bad = [dict(plane_max=0.0), dict(plane_max=-1.0), dict(plane_max=nan), dict(plane_max="x"), dict(max_len=0.0), dict(max_len=0.5),
           dict(max_len=nan), dict(albedo_floor=0.0), dict(albedo_floor=-1), dict(albedo_floor=nan), dict(min_weight=-1e-9), dict(min_weight=nan),
           dict(alpha_min=-0.1), dict(alpha_min=1.5), dict(alpha_min=nan), dict(alpha_mom_min=-0.1), dict(alpha_mom_min=1.5),
           dict(alpha_mom_min=nan), dict(var_min_len=0.5), dict(var_min_len=nan), dict(normal_min=nan), dict(normal_min=None),
           dict(off=(inf, 0)), dict(off=(0, -inf)), dict(off=(nan, 0)), dict(off=1.0), dict(off=(1, 2, 3)), dict(unknown="a"),
           dict(max_len=True)]
    for kw in bad:
        with pytest.raises(ValueError):
            S_(**kw)
    with pytest.raises(TypeError):
        S_(nonsense=1)
    ok = rm.reproject_pass
    for kw in (dict(flags=2), dict(flags=3), dict(plane_max=0.0), dict(max_len=0.5), dict(alb_floor=0.0), dict(min_weight=-1.0),
               dict(alpha_min=2.0), dict(alpha_mom_min=nan), dict(var_min_len=0.0), dict(normal_min=nan), dict(off_x=inf), dict(off_y=nan)):
        with pytest.raises(ValueError):
            ok(col, rec, None, prev, **dict(p, **kw))
    var = np.zeros((H16, W16), dtype=F)
    for c, r, v, pv in ((col.astype(np.float64), rec, None, prev), (col[..., :2], rec, None, prev), (col, rec[..., :11], None, prev),
                        (col, rec[:-1], None, prev), (col, rec, var[:-1], prev), (col, rec, var.astype(np.float64), prev),
                        (col, rec, None, prev[:2]), (col, rec, None, (prev[0][:15], prev[1], prev[2])),
                        (col, rec, None, (prev[0], prev[1][:-1], prev[2])), (col, rec, None, (prev[0], prev[1], prev[2][..., :7])),
                        (col, rec, None, (prev[0], prev[1], prev[2].astype(np.float64))), (col, rec, None, 5)):
        with pytest.raises(ValueError):
            ok(c, r, v, pv, **p)


def test_python_refusals_without_a_gpu(qr):
    """what Scene.reproject and Scene.temporal refuse before anything reaches the library or the device: QrError.  The scene is a
    shell without a handle; every tensor is on the CPU, which is 'another device' and the last thing checked"""
    import torch
    me = object.__new__(qr.Scene)
    me._h, me.device = ctypes.c_void_p(), 0
    n, h, w = 2, 5, 6
    col, hits, var = torch.zeros((n, h, w, 3)), torch.zeros((n, h, w, 12)), torch.zeros((n, h, w))
    prev = (torch.zeros((n, 16)), hits.clone(), torch.zeros((n, h, w, 8)))
    with pytest.raises(qr.QrError, match="on cuda:0"):
        me.reproject(col, hits, prev, var)
    for kw in (dict(plane_max=0.0), dict(max_len=0.5), dict(alpha_min=2.0), dict(min_weight=-1.0), dict(albedo_floor="a"),
               dict(normal_min=float("nan")), dict(off=(float("inf"), 0)), dict(var_min_len=0)):
        with pytest.raises(qr.QrError, match="must be"):
            me.reproject(col, hits, prev, var, **kw)
        with pytest.raises(qr.QrError, match="must be"):
            me.temporal(n, w, h, **kw)
    with pytest.raises(qr.QrError, match="nonsense"):
        me.reproject(col, hits, nonsense=1)
    for bad in (col.double(), col[..., :2], torch.zeros((n, h, w, 5)), col[0], col.numpy(), torch.zeros((0, h, w, 3)), None):
        with pytest.raises(qr.QrError, match="colour must be"):
            me.reproject(bad, hits)
    for bad in (hits.double(), hits[..., :11], hits[:1], None):
        with pytest.raises(qr.QrError, match="hits must be"):
            me.reproject(col, bad)
    for bad in (var.double(), var[:1], var[..., None], var.numpy()):
        with pytest.raises(qr.QrError, match="variance must be"):
            me.reproject(col, hits, variance=bad)
    for bad in (prev[:2], (prev[0][:1], prev[1], prev[2]), (prev[0], prev[1], prev[2][..., :7]), (prev[0], None, prev[2]),
                (prev[0].double(), prev[1], prev[2]), 5):
        with pytest.raises(qr.QrError, match="prev must be"):
            me.reproject(col, hits, bad)
    for bad in (dict(n_views=0), dict(width=0), dict(height=2.5), dict(channels=5), dict(n_views=True)):
        with pytest.raises(qr.QrError, match="positive integers"):
            me.temporal(**dict(dict(n_views=1, width=4, height=4), **bad))


# ---------------------------------------------------------------------------------------------------------------- GPU

def _buffer(scn, shape, fill=float("nan"), lead=0):
    """an output buffer of `fill` (NaN: the call leaves none where the statement has none) between `lead` floats and 64 floats
    of SENTINEL -- lead = 1 puts it 4 bytes off a 16-byte boundary --: (whole, body)"""
    import torch
    n = int(np.prod(shape))
    whole = torch.full((lead + n + 64,), SENTINEL, dtype=torch.float32, device=f"cuda:{scn.device}")
    whole[lead:lead + n] = fill
    return whole, whole[lead:lead + n].view(shape)


def _params(qr, ch, p, reserved=(0, 0, 0)):
    return qr.ReprojectParams(ch, int(p["flags"]), *(float(p[k]) for k in FIELDS[1:]), (ctypes.c_uint32 * 3)(*reserved))


def _call_gpu(qr, rm, scn, col, rec, var, prev, p, where, outs=(True, True, True), stream=None):
    """one qr_reproject_views_async call through ctypes into filled, sentinel-tailed buffers, compared with reproject_pass on the
    same host arrays: every word of every output that is given, the tails intact.  Returns the history (numpy)"""
    import torch
    n, h, w, ch = col.shape
    cd, hd = _dev(scn, col), _dev(scn, rec)
    vd = None if var is None else _dev(scn, var)
    pd = [None] * 3 if prev is None else [_dev(scn, a) for a in prev]
    shapes = [(n, h, w, 8), (n, h, w, ch), (n, h, w), (n, h, w, 2)]
    bufs = [_buffer(scn, s, 777.0 if k == 3 else float("nan"), min(k, 1)) if k == 0 or outs[k - 1] else (None, None)
            for k, s in enumerate(shapes)]
    vp = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())
    cp = _params(qr, ch, p)
    st = torch.cuda.current_stream() if stream is None else stream
    rc = qr.lib().qr_reproject_views_async(scn._h, vp(cd), vp(hd), vp(vd), vp(pd[0]), vp(pd[1]), vp(pd[2]), n, w, h, ctypes.byref(cp),
                                           *(vp(b[1]) for b in bufs), ctypes.c_void_p(st.cuda_stream))
    assert rc == 0, f"{where}: {qr.lib().qr_last_error().decode()}"
    st.synchronize()
    want = rm.reproject_pass(col, rec, var, prev, **p)
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
            assert (_bits(got[ids < 0]) == QNAN).all(), f"{where}: a miss's coords are the NaN the text writes"
    return got_hist


_CHAIN = {}


def _chain_inputs(qr, rm, scene, w, h):
    """(scene, cameras [4], stops, inputs) of a real case, computed once: the four cameras of _pair in ONE launch each of
    view_hits, two adaptive path-traced samples (mean and variance()) and a spun 4-direction gather (four channels)"""
    import torch
    if (scene, w, h) not in _CHAIN:
        cams, off, plane_max = _pair(rm, scene, w, h)
        scn = qr.Scene(_base(scene), ray_queries=True)
        scn.set_pt(False)
        vt = TPV._vt(scn, cams)
        hits = scn.view_hits(vt, w, h)
        acc = scn.pt_adaptive_views(vt, w, h, min_samples=2, max_samples=64, tol=0.05)
        _, mean = acc.step(2, mean=True)
        var = acc.variance()
        spin = torch.from_numpy(rm.spins((4, h, w), 7)).to(vt.device)
        dirs = torch.from_numpy(rm.cosine_dirs(4)).to(vt.device)
        gat, _ = scn.view_gather(vt, dirs, w, h, eps=TA.EPS, reach=TA.REACH, frame=True, spin=spin)
        x = dict(hits=_host(hits), mean=_host(mean), var=_host(var), gather=_host(gat), views=np.stack(cams))
        assert np.isfinite(x["mean"]).all() and np.isfinite(x["gather"]).all() and x["gather"].shape[-1] == 4
        _CHAIN[scene, w, h] = (scn, cams, dict(plane_max=plane_max, off=off), x)
    return _CHAIN[scene, w, h]


def _run_chain(qr, rm, scn, x, stops, where, combos):
    """A -> B -> A' one view at a time: each step's history goes into the next"""
    for ch, with_var, demod, outs in combos:
        p = rm.reproject_stops(demodulate=demod, **stops)
        prev, kept = None, 0
        for k in range(3):
            col = (x["mean"] if ch == 3 else x["gather"])[k:k + 1]
            var = x["var"][k:k + 1] if with_var else None
            hist = _call_gpu(qr, rm, scn, col, x["hits"][k:k + 1], var, prev, p, f"{where} ch {ch} var {with_var} demod {demod} outs {outs} step {k}", outs)
            prev = (x["views"][k:k + 1], x["hits"][k:k + 1], hist)
            kept += int((hist[..., 6] > 1).sum())
        assert kept > 0, f"{where}: no pixel kept history"


COMBOS = [(3, True, False, (True, True, True)), (3, False, True, (False, True, False)), (4, True, True, (True, True, True)),
          (4, False, False, (False, False, True)), (3, True, True, (True, False, False))]


@pytest.mark.gpu
@pytest.mark.parametrize("size", REAL_SIZES)
@pytest.mark.parametrize("scene", REAL_SCENES)
def test_gpu_chain_of_three_cameras(qr, rays_mod, scene, size):
    """view_hits, path-traced means with their variance and a spun gather of cameras A, B, A'; three steps A -> B -> A', the
    history of each the input of the next, in 3 and 4 channels, with and without var_in, DEMODULATE and each optional output"""
    w, h = size
    scn, cams, stops, x = _chain_inputs(qr, rays_mod, scene, w, h)
    if (w, h) == (64, 64):
        ids = x["hits"].view(np.int32)[..., 7]
        want = np.stack(_oracle_records(rays_mod, scene, w, h)).view(np.int32)[..., 7]
        assert (ids[:2] == want).all(), "the device's records are the ones the CPU test judged"
    _run_chain(qr, rays_mod, scn, x, stops, f"{scene} {w}x{h}", COMBOS)


def _synthetic(w, h, seed, ch):
    """two views of hand-made inputs: a dyadic camera each (the second turned), previous records on the plane z = 1 with ids 2,
    5 and misses and tilted normals, this frame's points scattered over and around the previous frame, and in both frames
    records with NaN, Inf and -0.0 in pos, nrm and alb; a random history with lengths 0, below 1, 1 and up to 40"""
    rng = np.random.default_rng(seed)
    views = np.stack([_dyadic_view(w, h), _dyadic_view(w, h)])
    views[1, 8:11], views[1, 12:15] = (0.0, S, 0.0), (-S, 0.0, 0.0)
    views[1, 4:7] = (h / 2 * S, -w / 2 * S, 1.0)
    recs, olds = [], []
    for j in range(2):
        old = _plane(w, h)
        cur = _plane(w, h)
        fx = rng.uniform(-2.0, w + 1.0, (h, w))
        fy = rng.uniform(-2.0, h + 1.0, (h, w))
        near = rng.uniform(size=(h, w)) < 0.6                       # most pixels move by less than two pixels
        ys, xs = np.mgrid[0:h, 0:w]
        fx = np.where(near, xs + rng.uniform(-2, 2, (h, w)), fx)
        fy = np.where(near, ys + rng.uniform(-2, 2, (h, w)), fy)
        whole = rng.uniform(size=(h, w)) < 0.15                     # some land exactly on a pixel: wx == 0
        fx, fy = np.where(whole, np.round(fx), fx), np.where(whole, np.round(fy), fy)
        if j == 0:
            cur[..., 0], cur[..., 1] = (fx - w / 2) * S, (fy - h / 2) * S
        else:                                                       # the turned camera: fx = Y / s + w/2, fy = h/2 - X / s
            cur[..., 0], cur[..., 1] = (h / 2 - fy) * S, (fx - w / 2) * S
            old[..., 0], old[..., 1] = (h / 2 - ys) * S, (xs - w / 2) * S
        cur[..., 2] = np.where(rng.uniform(size=(h, w)) < 0.1, rng.choice([-1.0, 1.03, 1.07, 0.0], (h, w)), 1.0)
        for r in (cur, old):
            ids = r.view(np.int32)[..., 7]
            ids[rng.uniform(size=(h, w)) < 0.3] = 5
            ids[rng.uniform(size=(h, w)) < 0.08] = -1
            tilt = rng.uniform(size=(h, w)) < 0.2
            nn = rng.normal(0.0, 0.4, (h, w, 3)) + np.array([0.0, 0.0, -1.0])
            nn = (nn / np.sqrt((nn * nn).sum(-1, keepdims=True))).astype(F)
            r[..., 4:7] = np.where(tilt[..., None], nn, r[..., 4:7])
            r[..., 8:11] = rng.uniform(0.0, 1.0, (h, w, 3)).astype(F)
            for word in (0, 1, 2, 4, 5, 6, 8, 9, 10):
                for val in (np.nan, np.inf, -np.inf, -0.0):
                    r[..., word] = np.where(rng.uniform(size=(h, w)) < 0.01, F(val), r[..., word])
        recs.append(cur), olds.append(old)
    hist = rng.uniform(-1.0, 2.0, (2, h, w, 8)).astype(F)
    hist[..., 6] = rng.choice(np.array([0.0, 0.5, 1.0, 1.0, 2.5, 7.0, 31.0, 40.0], dtype=F), (2, h, w))
    hist[..., 7] = 0.0
    col = rng.uniform(0.0, 1.0, (2, h, w, ch)).astype(F)
    var = rng.uniform(0.0, 0.1, (2, h, w)).astype(F)
    return col, np.stack(recs), var, (views, np.stack(olds), hist)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SYNTH_SIZES)
def test_gpu_synthetic_inputs(qr, rays_mod, size):
    """hand-made records with NaN, Inf and -0.0, a random history, points that fall all over and around the previous frame, at
    1x1, 9x130 and 67x45 in 3 and 4 channels: most tiles are partial.  Filled, sentinel-tailed outputs, 4 bytes off a 16-byte
    boundary where 4-byte alignment is all the call asks for"""
    w, h = size
    rm = rays_mod
    scn = qr.Scene(_base("patched:demo01_160"))          # any scene, any mode, no ray-query list
    try:
        taken = 0
        for ch in (3, 4):
            col, rec, var, prev = _synthetic(w, h, 11 * w + ch, ch)
            taps = []
            rm.reproject_pass(col, rec, var, prev, plane_max=F(2.0 ** -5), taps=taps)
            taken += sum(int(t[0].sum()) for t in taps)
            for kw in (dict(plane_max=2.0 ** -5), dict(plane_max=2.0 ** -5, demodulate=True, var_min_len=1, max_len=8, unknown=np.nan),
                       dict(normal_min=-1.0, min_weight=0.3, alpha_min=1.0, alpha_mom_min=0.0, off=(0.5, -0.25))):
                p = rm.reproject_stops(**kw)
                _call_gpu(qr, rm, scn, col, rec, var, prev, p, f"synthetic {w}x{h} ch {ch} {kw}")
                _call_gpu(qr, rm, scn, col, rec, None, prev, p, f"synthetic {w}x{h} ch {ch} {kw} no variance", (True, False, True))
            _call_gpu(qr, rm, scn, col, rec, var, None, rm.reproject_stops(demodulate=True), f"synthetic {w}x{h} ch {ch} first frame")
        assert taken > 0 or w * h == 1, "the inputs take taps"
    finally:
        scn.close()


@pytest.mark.gpu
def test_gpu_views_are_independent(qr, rays_mod):
    """three views with three different previous cameras in one launch; view 1 alone gives the same bits; the same call twice
    and a call on a side stream behind an event give the same bytes; Scene.reproject is the C call"""
    import torch
    rm = rays_mod
    scene, (w, h) = REAL_SCENES[0], REAL_SIZES[1]
    scn, cams, stops, x = _chain_inputs(qr, rm, scene, w, h)
    p = rm.reproject_stops(**stops)
    first = rm.reproject_pass(x["mean"][:3], x["hits"][:3], x["var"][:3], None, **p)[0]
    cur = [1, 2, 3]                                          # B, A', B' against A, B, A'
    col, rec, var = x["mean"][cur], x["hits"][cur], x["var"][cur]
    prev = (x["views"][:3], x["hits"][:3], first)
    hist = _call_gpu(qr, rm, scn, col, rec, var, prev, p, "three views")
    assert all((hist[j, ..., 6] > 1).any() for j in range(3))
    alone = _call_gpu(qr, rm, scn, col[1:2], rec[1:2], var[1:2], tuple(a[1:2] for a in prev), p, "view 1 alone")
    _same(alone[0], hist[1], "a view alone and as view 2 of 3")
    dev = [_dev(scn, a) for a in (col, rec, var)]
    pd = tuple(_dev(scn, a) for a in prev)
    a = scn.reproject(dev[0], dev[1], pd, dev[2], coords=True, **stops)
    b = scn.reproject(dev[0], dev[1], pd, dev[2], coords=True, **stops)
    assert len(a) == 4 and tuple(a[0].shape) == (3, h, w, 8) and tuple(a[3].shape) == (3, h, w, 2)
    _same(_host(a[0]), hist, "Scene.reproject is the C call")
    for s, t in zip(a, b):
        assert torch.equal(s.view(torch.int32), t.view(torch.int32)), "the same call twice"
    three = scn.reproject(dev[0], dev[1], pd, dev[2], colour_out=False, variance_out=False, **stops)
    assert len(three) == 3 and three[1] is None and three[2] is None
    out = torch.empty_like(a[0])
    assert scn.reproject(dev[0], dev[1], pd, dev[2], out=out, **stops)[0] is out and torch.equal(out.view(torch.int32), a[0].view(torch.int32))
    side, ready, done = torch.cuda.Stream(), torch.cuda.Event(), torch.cuda.Event()
    c2 = dev[0].clone()
    ready.record()
    side.wait_event(ready)
    s = scn.reproject(c2, dev[1], pd, dev[2], coords=True, stream=side, **stops)
    done.record(side)
    torch.cuda.current_stream().wait_event(done)
    for u, t in zip(s, a):
        assert torch.equal(u.view(torch.int32), t.view(torch.int32)), "a side stream"
    side.synchronize()
    with pytest.raises(qr.QrError, match="previous history"):
        scn.reproject(dev[0], dev[1], pd, dev[2], out=pd[2], **stops)
    with pytest.raises(qr.QrError, match="out must be"):
        scn.reproject(dev[0], dev[1], pd, dev[2], out=out[:1], **stops)
    with pytest.raises(qr.QrError, match="coords must be"):
        scn.reproject(dev[0], dev[1], pd, dev[2], coords=out, **stops)


@pytest.mark.gpu
def test_gpu_temporal_accumulator(qr, rays_mod):
    """Temporal over 4 moving frames of two views (A B A' B' and B A' B' A) against rays.temporal, with demodulation; its
    output fed to Scene.denoise equals rays.denoise of the same input; clone and reset as in numpy"""
    import torch
    rm = rays_mod
    scene, (w, h) = REAL_SCENES[0], REAL_SIZES[0]
    scn, cams, stops, x = _chain_inputs(qr, rm, scene, w, h)
    order = [[0, 1], [1, 2], [2, 3], [3, 0]]
    kw = dict(stops, demodulate=True, var_min_len=2)
    acc, ref = scn.temporal(2, w, h, 3, **kw), rm.temporal(2, w, h, 3, **kw)
    assert acc.history is None and acc.length is None and acc.frames == 0 and acc.params == ref.params
    twin = None
    for k, o in enumerate(order):
        col, rec, var, vw = x["mean"][o], x["hits"][o], x["var"][o], x["views"][o]
        hd = _dev(scn, rec)
        got = acc.step(_dev(scn, col), hd, _dev(scn, vw), _dev(scn, var))
        want = ref.step(col, rec, vw, var)
        _same(_host(got[0]), want[0], f"frame {k} colour"), _same(_host(got[1]), want[1], f"frame {k} variance")
        _same(_host(acc.history), ref.history, f"frame {k} history"), _same(_host(acc.length), ref.length, f"frame {k} length")
        assert acc.frames == k + 1
        if k == 1:
            twin = acc.clone()
    assert (ref.length > 2).any(), "some history is three frames long"
    dkw = dict(passes=2, plane=stops["plane_max"], luma=4.0, normal_power=8)
    clean, cvar = scn.denoise(got[0], hd, got[1], **dkw)
    wc, wv = rm.denoise(want[0], want[1], rec, **dkw)
    _same(_host(clean), wc, "denoise of the accumulated colour"), _same(_host(cvar), wv, "denoise of the accumulated variance")
    for k in (2, 3):
        o = order[k]
        tg = twin.step(_dev(scn, x["mean"][o]), _dev(scn, x["hits"][o]), _dev(scn, x["views"][o]), _dev(scn, x["var"][o]))
    assert torch.equal(tg[0].view(torch.int32), got[0].view(torch.int32)) and twin.history.data_ptr() != acc.history.data_ptr()
    acc.reset()
    assert acc.history is None and acc.frames == 0
    o = order[1]
    got = acc.step(_dev(scn, x["mean"][o]), _dev(scn, x["hits"][o]), _dev(scn, x["views"][o]))
    want = rm.reproject_pass(x["mean"][o], x["hits"][o], None, None, **ref.params)
    _same(_host(got[0]), want[1], "after reset: a first frame"), _same(_host(got[1]), want[2], "after reset: unknown")
    with pytest.raises(qr.QrError, match="this accumulation holds"):
        acc.step(_dev(scn, x["gather"][o]), _dev(scn, x["hits"][o]), _dev(scn, x["views"][o]))


@pytest.mark.gpu
def test_gpu_refusals(qr, rays_mod):
    """every QR_ERR_ARG through ctypes, the sentinel-filled outputs untouched after all of them; n_views = 0 is QR_OK; the scene
    then still traces 64 rays as the oracle's helper does"""
    import torch
    rm = rays_mod
    L = qr.lib()
    blob = _base(REAL_SCENES[0])
    scn = qr.Scene(blob, ray_queries=True)
    dev = f"cuda:{scn.device}"
    n, w, h = 2, 9, 7
    z = lambda m: torch.zeros((m + 16,), dtype=torch.float32, device=dev)
    s75 = lambda m: torch.full((m + 16,), 7.5, dtype=torch.float32, device=dev)
    px = n * h * w
    col, hits, var, views, hprev, hin = z(px * 4), z(px * 12), z(px), z(n * 16), z(px * 12), z(px * 8)
    hout, cout, vout, xout = s75(px * 8), s75(px * 4), s75(px), s75(px * 2)
    vp = lambda x, off=0: ctypes.c_void_p(None if x is None else x.data_ptr() + off)
    nan, inf = float("nan"), float("inf")
    base = rm.reproject_stops(plane_max=0.5)

    def call(s=scn._h, ci=vp(col), hi=vp(hits), vi=vp(var), pv=vp(views), ph=vp(hprev), pi=vp(hin), n=n, w=w, h=h, ho=vp(hout),
             co=vp(cout), vo=vp(vout), xo=vp(xout), null_p=False, channels=3, reserved=(0, 0, 0), **pk):
        p = _params(qr, channels, dict(base, **pk), reserved)
        return L.qr_reproject_views_async(s, ci, hi, vi, pv, ph, pi, n, w, h, None if null_p else ctypes.byref(p), ho, co, vo, xo, None)

    none = vp(None)
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
    assert call(n=0) == 0 and call(n=0, ci=none, hi=none, ho=none) == 0
    torch.cuda.synchronize()
    for t in (hout, cout, vout, xout):
        assert (t == 7.5).all().item(), "a refused call wrote something"
    # served: offsets that keep the alignment, the first frame, no optional output, four channels, the limits of the stops
    assert call() == 0 and call(ci=vp(col, 4), vi=vp(var, 8), co=vp(cout, 12), vo=vp(vout, 4), xo=vp(xout, 4), hi=vp(hits, 48), pi=vp(hin, 16)) == 0
    assert call(pv=none, ph=none, pi=none) == 0 and call(vi=none, co=none, vo=none, xo=none) == 0
    assert call(channels=4, flags=1, unknown=nan, min_weight=-0.0, alpha_min=0.0, alpha_mom_min=1.0, max_len=inf, var_min_len=1.0,
                plane_max=inf, normal_min=-inf) == 0
    torch.cuda.synchronize()
    assert (hout[:px * 8] != 7.5).all().item() and (hout[px * 8:] == 7.5).all().item()
    rays = rm.camera_rays(blob)
    rays = rays[:: max(1, len(rays) // 64)][:64]
    t, ids = scn.trace(_dev(scn, rays))
    want = THR._helper()(blob, rays)
    assert (_host(ids) == want.view(np.int32)[:, 7]).all() and (_bits(_host(t)) == _bits(want[:, 3])).all(), "the scene still traces"
    scn.close()
    plain = qr.Scene(_base("patched:demo01_160"))           # no ray-query list: the call needs none
    assert L.qr_reproject_views_async(plain._h, vp(col), vp(hits), none, none, none, none, n, w, h, ctypes.byref(_params(qr, 3, base)),
                                      vp(hout), none, none, none, None) == 0
    torch.cuda.synchronize()
    plain.close()


# once more through the guarded diagnostic build (make guard), as tests/test_atrous.py does it: the library is chosen when the
# package is imported, hence the child process: this file run as a script.

def _guard_child():
    from qr_loader import load_package
    qr = load_package()
    assert qr.LIB_PATH == GUARD_LIB, qr.LIB_PATH
    rm = _rays_mod()
    scene, (w, h) = REAL_SCENES[0], REAL_SIZES[1]
    scn, cams, stops, x = _chain_inputs(qr, rm, scene, w, h)
    _run_chain(qr, rm, scn, x, stops, f"guard {scene}", COMBOS[:3])
    scn.close()
    print(f"{scene} guard_ok 1", flush=True)
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
