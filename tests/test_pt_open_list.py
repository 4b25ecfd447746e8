"""Open lists and indexed adaptive steps (include/qrhip.h qr_pt_adapt_open_list_async, qr_pt_adapt_list_rays_async;
PtAdaptive.open_list, PtAdaptive.step(index=, count=, cap=)): the indices of the rays an adaptive state's stop rule leaves open,
written on chip in ascending order, and the adaptive step on the rays of such a list, 64 listed rays per wave; and the host side
in quadray-engine_amd/rays.py (pt_adapt_open_list, pt_adapt_fold_list).

Every comparison is bit for bit.  The truth of a step is tests/test_pt_adaptive.py's: rays.pt_adapt_fold over the raw samples of
tests/ptadapt_oracle.c; a ray's result depends on nothing but its own column, ray and spread, so the state after "list, then
indexed step" is the state after the plain step, and the tests ask for exactly that.  The truth of a list is
np.flatnonzero(rays.pt_adapt_open(state)).  Unwritten memory is shown by sentinels: SI in index, count and state tails, SF in rgb.

Settings of the seeded-view tests: test_pt_adaptive's (min 2, max 12, the scene's tolerance), 6 plain candidates, then 6 listed.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _ptpatch
import _rayset as RS
import test_pt_adaptive as TPA
import test_pt_rays as TPR
from conftest import ROOT
from test_pt_adaptive import MAX, MIN, TOL, _fresh, _run, _same, _samples, _seq, _step, _tol2, _truth, _truth_call, _view_rays, _window
from test_pt_views import _base, _bits, _rays_mod

ASM, GUARD_LIB, VIEW = TPA.ASM, TPA.GUARD_LIB, TPA.VIEW
ARG, UNSUP = -1, -3
SI, SF = 0x5A5A5A5A, 12345.0
STEP_SCENES = ["patched:demo02_160_gf_aa4", "pt:test18_160_pt"]
_t, _host = TPR._t, TPR._host


@pytest.fixture(scope="module")
def rays_mod():
    return _rays_mod()


def _f(*v):
    return np.array(v, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- CPU

def _rule_cases():
    """the constructed state of test_pt_adaptive.test_rule_on_a_constructed_state: (m, M2r, M2g, M2b) per column"""
    return [(0, 0.0, 0.0, 0.0), (1, 0.0, 0.0, 0.0), (2, 0.5, 0.5, 0.5), (2, 0.5, np.float32(0.5) + np.float32(2.0 ** -24), 0.5),
            (2, 0.0, 0.0, 0.50001), (3, 1.5, 1.5, 1.5), (3, np.nan, 0.0, 0.0), (5, -1.0, -np.inf, 0.0), (11, np.inf, 0.0, 0.0),
            (12, np.inf, np.nan, 9e9), (13, np.inf, 0.0, 0.0), (0xFFFFFFFF, np.nan, 0.0, 0.0)]


def _rule_state():
    cases = _rule_cases()
    st = np.zeros((8, len(cases)), dtype=np.uint32)
    for i, (m, a, b, c) in enumerate(cases):
        st[4, i] = m
        st[5:8, i] = _f(a, b, c)
    return st


def test_open_list_is_flatnonzero_of_the_rule(rays_mod):
    """pt_adapt_open_list on the constructed state of test_rule_on_a_constructed_state -- counts around min, max, 0 and 1, M2 at,
    above and below the limit, NaN -- at several min, max and tol2, tol2 = 0 among them"""
    st = _rule_state()
    seen = set()
    for mn, mx, t2 in ((0, 12, 0.25), (12, 12, 0.25), (3, 12, 0.25), (0, 12, 0.0), (2, 3, 0.25), (0, 1 << 20, 0.25)):
        got = rays_mod.pt_adapt_open_list(st, mn, mx, np.float32(t2))
        want = np.flatnonzero(rays_mod.pt_adapt_open(st, mn, mx, np.float32(t2)))
        assert got.dtype == np.uint32 and got.ndim == 1 and got.tolist() == want.tolist()
        assert (np.diff(got.astype(np.int64)) > 0).all()
        assert rays_mod.pt_adapt_open_list(st.view(np.int32), mn, mx, np.float32(t2)).tolist() == got.tolist()
        seen.add(tuple(got.tolist()))
    assert rays_mod.pt_adapt_open_list(st, 0, 12, np.float32(0.25)).tolist() == [0, 1, 3, 4, 6, 8]
    assert len(seen) >= 5, "the settings do not tell the lists apart"


@pytest.mark.parametrize("scene", STEP_SCENES)
def test_fold_list_is_the_fold_on_listed_columns(rays_mod, scene):
    """after 6 candidates between 10 % and 90 % of the rays are open; pt_adapt_fold_list with the full open list gives
    pt_adapt_fold's state and open and its rgb on the listed rows; with a sub-list, with count or cap below its length, and with
    entries >= N, it changes the served columns only -- and those as the fold does"""
    rm, j = rays_mod, VIEW[scene]
    t2 = _tol2(TOL[scene])
    seq = _seq(rm, scene, j, True)
    first = _truth(rm, scene, j, True, (6, 6))
    s6 = first[0][0]
    n = s6.shape[1]
    L = rm.pt_adapt_open_list(s6, MIN, MAX, t2)
    print(f"{scene}: {len(L)} of {n} rays open after 6 candidates")
    assert 0.1 * n <= len(L) <= 0.9 * n and len(L) == first[0][2]
    c, g = _window(seq, s6, 6)
    st, rgb, op = rm.pt_adapt_fold_list(s6, L, len(L), c, g, MIN, MAX, t2)
    wst, wrgb, wop = first[1]
    assert (st == wst).all() and op == wop and (_bits(rgb[L]) == _bits(wrgb[L])).all()
    rest = np.ones(n, dtype=bool); rest[L] = False
    assert np.isnan(rgb[rest]).all() and (st[:, rest] == s6[:, rest]).all()
    assert (st[4, L] > s6[4, L]).all(), "a listed ray took nothing"
    perm = np.random.default_rng(3).permutation(L[::2])
    for lst, count, cap in ((perm, len(perm), None), (L, len(L) // 2, None), (L, len(L), len(L) // 3), (L[::-1].copy(), len(L), None),
                            (np.concatenate([L[:5], [n, n + 3], L[5:9]]).astype(np.uint32), 11, None)):
        served = np.asarray(lst[:min(count, len(lst) if cap is None else cap)], dtype=np.int64)
        served = served[served < n]
        st2, rgb2, op2 = rm.pt_adapt_fold_list(s6, lst, count, c, g, MIN, MAX, t2, cap=cap)
        out = np.ones(n, dtype=bool); out[served] = False
        assert (st2[:, served] == wst[:, served]).all() and (st2[:, out] == s6[:, out]).all()
        assert (_bits(rgb2[served]) == _bits(wrgb[served])).all() and np.isnan(rgb2[out]).all()
        assert op2 == int(rm.pt_adapt_open(wst[:, served], MIN, MAX, t2).sum())
    with pytest.raises(ValueError):
        rm.pt_adapt_fold_list(s6, np.array([1, 2, 1]), 3, c, g, MIN, MAX, t2)


def test_open_list_abi_and_constants(qr):
    """the library exports the three entry points, the header declares them, and its two constants are the module's"""
    L = qr.lib()
    with open(os.path.join(ROOT, "include", "qrhip.h")) as f:
        hdr = f.read()
    for sym in ("qr_pt_adapt_list_work_bytes", "qr_pt_adapt_open_list_async", "qr_pt_adapt_list_rays_async"):
        assert hasattr(L, sym), sym
        assert sym in qr.ABI_SYMBOLS and f"int {sym}(" in hdr, sym
    assert f"#define QR_PT_OPEN_BLOCK {qr.PT_OPEN_BLOCK} " in hdr and qr.PT_OPEN_BLOCK % 64 == 0 and qr.PT_OPEN_BLOCK > 0
    assert f"#define QR_PT_OPEN_CHUNK {qr.PT_OPEN_CHUNK} " in hdr and qr.PT_OPEN_CHUNK > 0
    assert "const uint32_t *index_dev, const uint32_t *count_dev, int64_t cap," in hdr
    assert callable(qr.PtAdaptive.open_list)
    import inspect
    assert {"index", "count", "cap"} <= set(inspect.signature(qr.PtAdaptive.step).parameters)
    assert "NOT written" in qr.PtAdaptive.step.__doc__
    rm = _rays_mod()
    assert callable(rm.pt_adapt_open_list) and callable(rm.pt_adapt_fold_list)


def test_list_kernels_in_resource_check():
    """the build's register check lists the four new kernels once each -- the indexed step at the adaptive kernel's budget, the
    three list kernels with nothing spilled and no private segment -- and the built assembly passes it"""
    import importlib.util
    path = os.path.join(ROOT, "tools", "check_kernel_resources.py")
    spec = importlib.util.spec_from_file_location("check_kernel_resources", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    r = subprocess.run([sys.executable, path, ASM, "--print"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for name in ("qr_pt_list_kernel", "qr_open_count_kernel", "qr_open_scan_kernel", "qr_open_scatter_kernel"):
        frags = [f for f in m.LIMITS if name in f]
        assert len(frags) == 1, (name, frags)
        vg, sp, scr = m.LIMITS[frags[0]]
        if name == "qr_pt_list_kernel":
            assert (vg, sp, scr) == (168, 0, 2128) == m.LIMITS["18qr_pt_adapt_kernel"]
        else:
            assert sp == 0 and scr == 0
        assert r.stdout.count(name) == 1, name


# ---------------------------------------------------------------------------------------------------------------- GPU

PATTERNS = ("all", "none", "third", "last", "first", "half")


def _pattern_state(n, pattern):
    """(state uint32 [8, n], open bool [n]) at min 2, max 12, tol2 0.25: open columns hold m = 0, (5, one M2 above the limit) or
    (3, NaN); closed ones m = max, (5, M2 = 0) or (5, M2 == the limit 5 * 4 * 0.25 = 5); plane 0..3 arbitrary words"""
    i = np.arange(n)
    if pattern == "all": op = np.ones(n, dtype=bool)
    elif pattern == "none": op = np.zeros(n, dtype=bool)
    elif pattern == "third": op = i % 3 == 0
    elif pattern == "last": op = i == n - 1
    elif pattern == "first": op = i == 0
    else: op = np.random.default_rng(n).random(n) < 0.5
    kind = (i * 7 + i // 64) % 3
    st = np.zeros((8, n), dtype=np.uint32)
    st[0] = i * 2654435761 & 0xFFFFFFFF
    st[1:4] = _f(0.25)[0]
    m_open, m_closed = np.array([0, 5, 3], dtype=np.uint32), np.array([MAX, 5, 5], dtype=np.uint32)
    st[4] = np.where(op, m_open[kind], m_closed[kind])
    g_open = np.array([_f(0.0)[0], _f(5.000001)[0], _f(np.nan)[0]], dtype=np.uint32)
    g_closed = np.array([_f(np.inf)[0], _f(0.0)[0], _f(5.0)[0]], dtype=np.uint32)
    st[6] = np.where(op, g_open[kind], g_closed[kind])
    return st, op


def _list_case(qr_mod, rm, scn, n, pattern):
    import torch
    dev = f"cuda:{scn.device}"
    st, op = _pattern_state(n, pattern)
    t2 = np.float32(0.5) * np.float32(0.5)
    want = rm.pt_adapt_open_list(st, MIN, MAX, t2)
    assert want.tolist() == np.flatnonzero(op).tolist(), "the constructed state does not show the pattern"
    dst = torch.from_numpy(st.view(np.int32)).to(dev)
    acc = scn.pt_adaptive(n, MIN, MAX, 0.5, state=dst.clone())
    a = torch.full((n,), SI, dtype=torch.int32, device=dev)
    b = torch.full((n,), SI, dtype=torch.int32, device=dev)
    ca = torch.full((3,), SI, dtype=torch.int32, device=dev)
    cb = torch.full((3,), SI, dtype=torch.int32, device=dev)
    ia, cnt = acc.open_list(a, ca[1:2])
    assert ia.data_ptr() == a.data_ptr() and cnt.data_ptr() == ca[1:2].data_ptr()
    acc.open_list(b, cb[1:2])
    torch.cuda.synchronize()
    what = f"n = {n}, {pattern}"
    assert ca.tolist() == [SI, len(want), SI], f"{what}: count {ca.tolist()}, want {len(want)}"
    ha = a.cpu().numpy().view(np.uint32)
    assert (ha[:len(want)] == want).all(), f"{what}: the list differs"
    assert (ha[len(want):] == SI).all(), f"{what}: entries past count were written"
    assert torch.equal(a, b) and torch.equal(ca, cb), f"{what}: a second call gave other bytes"
    assert torch.equal(acc.state, dst), f"{what}: the state changed"


def _list_sizes(qr_mod):
    B, C = qr_mod.PT_OPEN_BLOCK, qr_mod.PT_OPEN_CHUNK
    return [1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1, B * C + B + 1]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(9))
def test_gpu_lists_on_constructed_states(qr, rays_mod, k):
    """n = 1, 63, 64, 65, B - 1, B, B + 1, 2 B + 1 and B C + B + 1 (past one pass of the scan), every pattern: index[:count] is
    pt_adapt_open_list, count is exact, index[count:] and the words around count keep their sentinel, the state is unchanged and
    a second call writes the same bytes"""
    n = _list_sizes(qr)[k]
    scn = qr.Scene(_base("patched:demo01_160"), ray_queries=True)
    try:
        for pattern in PATTERNS:
            _list_case(qr, rays_mod, scn, n, pattern)
        # the accumulator's own tensors: allocated once, returned again
        acc = scn.pt_adaptive(n, MIN, MAX, 0.5)
        i1, c1 = acc.open_list()
        i2, c2 = acc.open_list()
        assert i1.data_ptr() == i2.data_ptr() and c1.data_ptr() == c2.data_ptr() and tuple(i1.shape) == (n,) and tuple(c1.shape) == (1,)
        assert int(_host(c1)[0]) == n and (_host(i1) == np.arange(n)).all(), "a fresh state is all open"
    finally:
        scn.close()


def _listed(acc, rt, st, samples, index, count, cap=None):
    """one indexed step with rgb prefilled with SF and open: (state uint32 [8, N], rgb, open) on the host"""
    import torch
    rgb = torch.full((acc.n, 3), SF, dtype=torch.float32, device=rt.device)
    out, op = acc.step(rt, samples, spread=st, rgb=rgb, open=True, index=index, count=count, cap=cap)
    assert out.data_ptr() == rgb.data_ptr()
    return _host(acc.state).view(np.uint32), _host(rgb), int(_host(op).view(np.uint32)[0])


def _dev_list(scn, lst, count=None):
    import torch
    dev = f"cuda:{scn.device}"
    ix = torch.from_numpy(np.ascontiguousarray(lst, dtype=np.uint32).view(np.int32).copy()).to(dev)
    return ix, torch.tensor([len(lst) if count is None else count], dtype=torch.int32, device=dev)


def _same_listed(got, want, served, n, what):
    """state and open as `want` (state, rgb, open); rgb as want's on the served rows, SF on every other"""
    (gst, grgb, gop), (wst, wrgb, wop) = got, want
    served = np.asarray(served, dtype=np.int64)
    served = served[served < n]
    bad = [int((gst[p] != wst.view(np.uint32)[p]).sum()) for p in range(8)]
    out = np.ones(n, dtype=bool); out[served] = False
    nr = int((_bits(grgb[served]) != _bits(wrgb[served])).any(axis=1).sum())
    ns = int((grgb[out] != np.float32(SF)).any(axis=1).sum())
    assert not any(bad) and nr == 0 and ns == 0 and gop == wop, \
        f"{what}: of {n} rays, per plane {bad} state words differ, {nr} listed rays differ in rgb, {ns} unlisted rgb rows written; open {gop}, want {wop}"
    assert (_bits(grgb[served]) == gst[1:4, served].T).all(), f"{what}: rgb is not the state's means"


@pytest.mark.gpu
@pytest.mark.parametrize("scene", STEP_SCENES)
def test_gpu_indexed_step_equals_the_plain_step(qr, rays_mod, scene):
    """6 plain candidates, the open list, 6 more through the list: all eight planes and open are those of a plain second step on
    the same GPU and of the truth's second call; rgb is the truth's on the listed rows and untouched on the others"""
    rm, j = rays_mod, VIEW[scene]
    r, sp = _view_rays(rm, scene, j)
    n = len(r)
    want = _truth(rm, scene, j, True, (6, 6))
    L = rm.pt_adapt_open_list(want[0][0], MIN, MAX, _tol2(TOL[scene]))
    scn = qr.Scene(_base(scene), ray_queries=True)
    plain = _run(scn, r, sp, (6, 6), tol=TOL[scene])
    acc = TPA._acc(scn, n, tol=TOL[scene])
    rt, st = _t(scn, r), _t(scn, sp)
    first = _step(acc, rt, 6, st)
    index, count = acc.open_list()
    hl, hc = _host(index).view(np.uint32), int(_host(count)[0])
    got = _listed(acc, rt, st, 6, index, count)
    c2 = int(_host(acc.open_list()[1])[0])
    scn.close()
    _same(first, want[0], f"{scene}: the first 6")
    assert hc == len(L) == want[0][2] and (hl[:hc] == L).all() and 0.1 * n <= hc <= 0.9 * n
    assert (got[0] == plain[1][0]).all() and got[2] == plain[1][2], f"{scene}: the indexed step differs from the plain step on this GPU"
    _same_listed(got, want[1], L, n, f"{scene}: 6 listed after 6 plain")
    assert c2 == want[1][2], "the next list's length is the step's open"


@pytest.mark.gpu
def test_gpu_loop_of_lists_until_nothing_is_open(qr, rays_mod):
    """open_list, then step(3, index, count, cap = the open read back) until the count is 0: the final state is the truth's
    after (3, 3, 3, 3) and every round's count is the truth's open of the round before"""
    scene = "pt:test18_160_gf_aa4_pt"
    rm, j = rays_mod, VIEW[scene]
    r, sp = _view_rays(rm, scene, j)
    n = len(r)
    want = _truth(rm, scene, j, True, (3, 3, 3, 3))
    scn = qr.Scene(_base(scene), ray_queries=True)
    acc = TPA._acc(scn, n, tol=TOL[scene])
    rt, st = _t(scn, r), _t(scn, sp)
    counts, opens, cap = [], [], n
    while len(counts) < 8:
        index, count = acc.open_list()
        counts.append(int(_host(count)[0]))
        if counts[-1] == 0:
            break
        assert counts[-1] == cap
        _, op = acc.step(rt, 3, spread=st, rgb=False, open=True, index=index, count=count, cap=cap)
        cap = int(_host(op)[0])
        opens.append(cap)
    final = _host(acc.state).view(np.uint32)
    scn.close()
    assert opens == [w[2] for w in want][:len(opens)] and counts == [n] + opens, (counts, opens, [w[2] for w in want])
    assert opens[-1] == 0 and opens[0] > 0 and (final == want[len(opens) - 1][0]).all() and (final == want[-1][0]).all()


@pytest.mark.gpu
def test_gpu_caller_made_lists(qr, rays_mod):
    """a reversed list, a seeded permutation of a sub-list, a single entry, count below the list's length and cap below count,
    each from the state after 6 plain candidates: the served columns are the plain step's, every other column keeps all eight
    planes, rgb is written on the served rows only"""
    scene = "patched:demo02_160_gf_aa4"
    rm, j = rays_mod, VIEW[scene]
    r, sp = _view_rays(rm, scene, j)
    n = len(r)
    t2 = _tol2(TOL[scene])
    s6 = _truth(rm, scene, j, True, (6,))[0][0]
    L = rm.pt_adapt_open_list(s6, MIN, MAX, t2)
    c, g = _window(_seq(rm, scene, j, True), s6, 6)
    perm = np.random.default_rng(3).permutation(L[::2]).astype(np.uint32)
    mixed = np.random.default_rng(4).permutation(n)[:1000].astype(np.uint32)         # open and closed rays: any list is a list
    cases = [("ascending", L, len(L), None), ("reversed", L[::-1].copy(), len(L), None), ("permuted sub-list", perm, len(perm), None),
             ("one entry", L[77:78], 1, None), ("count below the length", L, len(L) // 2, None),
             ("cap below count", L, len(L), len(L) // 3), ("cap 1", L, len(L), 1), ("count 0", L, 0, None),
             ("open and closed rays", mixed, len(mixed), None)]
    scn = qr.Scene(_base(scene), ray_queries=True)
    rt, st = _t(scn, r), _t(scn, sp)
    got = {}
    for name, lst, count, cap in cases:
        acc = TPA._acc(scn, n, tol=TOL[scene], state=s6)
        ix, ct = _dev_list(scn, lst, count)
        got[name] = _listed(acc, rt, st, 6, ix, ct, cap)
    scn.close()
    for name, lst, count, cap in cases:
        served = lst[:min(count, len(lst) if cap is None else cap)]
        want = rm.pt_adapt_fold_list(s6, lst, count, c, g, MIN, MAX, t2, cap=cap)
        _same_listed(got[name], want, served, n, f"{scene}: {name}")
        out = np.ones(n, dtype=bool); out[served.astype(np.int64)] = False
        assert (got[name][0][:, out] == s6[:, out]).all(), f"{name}: an unlisted column changed"
    assert (got["reversed"][0] == got["ascending"][0]).all() and got["reversed"][2] == got["ascending"][2]
    assert (got["ascending"][0][4, L] > s6[4, L]).all() and (got["count 0"][0] == s6).all()
    assert (got["permuted sub-list"][0][:, perm] == got["ascending"][0][:, perm]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 63, 64, 65, 129])
def test_gpu_list_lengths_and_bounds(qr, rays_mod, k):
    """lists of 1, 63, 64, 65 and 129 entries over n = 200, entries n and n + 3 among them (alone in the list for k = 1, too);
    rays, spread, state and rgb are views into larger sentinel-filled tensors: the served columns are the fold's, every other
    word of every buffer keeps its bytes"""
    import torch
    scene = "patched:demo02_160_gf_aa4"
    rm = rays_mod
    r, sp = _view_rays(rm, scene, VIEW[scene])
    n, TAIL = 200, 4096
    r, sp = r[1000:1000 + n], sp[1000:1000 + n]
    lst = (np.random.default_rng(k).permutation(n - 4)[:k] + 4).astype(np.uint32)        # columns 0..3 stay unlisted
    if k > 1:
        lst[1], lst[k - 2] = n, n + 3
    lists = [lst] + ([np.array([n], dtype=np.uint32), np.array([n + 3], dtype=np.uint32)] if k == 1 else [])
    fresh = _fresh(rm, n)
    scn = qr.Scene(_base(scene), ray_queries=True)
    dev = f"cuda:{scn.device}"
    got = []
    for l in lists:
        stb = torch.full((8 * n + TAIL,), SI, dtype=torch.int32, device=dev)
        rgbb = torch.full((3 * n + TAIL,), SF, dtype=torch.float32, device=dev)
        rb = torch.full((8 * n + TAIL,), float("nan"), dtype=torch.float32, device=dev)
        sb = torch.full((8 * n + TAIL,), float("nan"), dtype=torch.float32, device=dev)
        opb = torch.full((3,), SI, dtype=torch.int32, device=dev)
        stb[:8 * n] = torch.from_numpy(fresh.view(np.int32).reshape(-1).copy()).to(dev)
        rb[:8 * n] = _t(scn, r).reshape(-1)
        sb[:8 * n] = _t(scn, sp).reshape(-1)
        acc = scn.pt_adaptive(n, MIN, MAX, TOL[scene], state=stb[:8 * n].view(8, n))
        ix, ct = _dev_list(scn, np.concatenate([l, np.full(64, 7, dtype=np.uint32)]), len(l))     # a tail past count: never read as a ray
        acc.step(rb[:8 * n].view(n, 8), 7, spread=sb[:8 * n].view(n, 8), rgb=rgbb[:3 * n].view(n, 3), open=opb[1:2], index=ix, count=ct)
        torch.cuda.synchronize()
        tails = bool((stb[8 * n:] == SI).all()) and bool((rgbb[3 * n:] == SF).all()) and bool(torch.isnan(rb[8 * n:]).all()) \
            and bool(torch.isnan(sb[8 * n:]).all()) and _host(opb)[[0, 2]].tolist() == [SI, SI]
        got.append((tails, (_host(acc.state).view(np.uint32), _host(rgbb[:3 * n].view(n, 3)), int(_host(opb)[1]))))
    scn.close()
    c, g = _samples(_base(scene), r, sp, fresh[0], 7)
    for l, (tails, gk) in zip(lists, got):
        assert tails, f"k = {k}, list {l[:4].tolist()}..: a tail was written"
        want = rm.pt_adapt_fold_list(fresh, l, len(l), c, g, MIN, MAX, _tol2(TOL[scene]))
        _same_listed(gk, want, l, n, f"{scene}: {len(l)} entries over {n}")
        assert (gk[0][:, :4] == fresh[:, :4]).all()
    assert (got[0][1][0][4] > 0).sum() == (lst < n).sum()


@pytest.mark.gpu
def test_gpu_splits_and_min_equals_max_through_the_list(qr, rays_mod):
    """through the full list 0 .. n - 1: 5 + 7 candidates give the bits of 12 and the truth's; and with min = max = 7, 3 + 4 give
    pt_rays' four planes after 7 samples, plane 4 = 7 and open 0"""
    scene = "pt:test18_160_pt"
    rm, j = rays_mod, VIEW[scene]
    r, sp = _view_rays(rm, scene, j)
    n = len(r)
    scn = qr.Scene(_base(scene), ray_queries=True)
    rt, st = _t(scn, r), _t(scn, sp)
    ix, ct = _dev_list(scn, np.arange(n))
    a = TPA._acc(scn, n, tol=TOL[scene])
    five = _listed(a, rt, st, 5, ix, ct)
    twelve_a = _listed(a, rt, st, 7, ix, ct)
    b = TPA._acc(scn, n, tol=TOL[scene])
    twelve_b = _listed(b, rt, st, 12, ix, ct)
    m = TPA._acc(scn, n, mn=7, mx=7, tol=TOL[scene])
    three = _listed(m, rt, st, 3, ix, ct)
    seven = _listed(m, rt, st, 4, ix, ct)
    prgb, pst = TPR._run(scn, r, sp, (7,))
    scn.close()
    want = _truth(rm, scene, j, True, (5, 7))
    _same(five, want[0], f"{scene}: 5 through the full list")
    _same(twelve_a, want[1], f"{scene}: 5 + 7 through the full list")
    _same(twelve_b, twelve_a, f"{scene}: 12 against 5 + 7")
    _same(twelve_b, _truth(rm, scene, j, True, (12,))[0], f"{scene}: 12 through the full list")
    assert (seven[0][:4] == pst.view(np.uint32)).all() and (_bits(seven[1]) == _bits(prgb)).all()
    assert (seven[0][4] == 7).all() and seven[2] == 0 and three[2] == n and (seven[0][5:8] != 0).any()


@pytest.mark.gpu
def test_gpu_depths_through_the_list(qr, rays_mod):
    """depth 0 and the scene's own depth: 6 plain, the list, 6 listed are the truth's two calls.  At depth 0 the samples of a
    ray differ only where the spread's jitter crosses an edge: 42 of the 4096 rays are open, a sparse list in one wave"""
    scene = "patched:demo02_160_gf_aa4"
    rm, j = rays_mod, VIEW[scene]
    r, sp = _view_rays(rm, scene, j)
    n = len(r)
    scn = qr.Scene(_base(scene), ray_queries=True)
    rt, st = _t(scn, r), _t(scn, sp)
    got = {}
    for depth in (None, 0):
        if depth is not None:
            scn.set_depth(depth)
        acc = TPA._acc(scn, n, tol=TOL[scene])
        first = _step(acc, rt, 6, st)
        index, count = acc.open_list()
        got[depth] = (first, _host(index).view(np.uint32)[:int(_host(count)[0])], _listed(acc, rt, st, 6, index, count))
    scn.close()
    for depth, (first, hl, second) in got.items():
        want = _truth(rm, scene, j, True, (6, 6), depth=depth)
        L = rm.pt_adapt_open_list(want[0][0], MIN, MAX, _tol2(TOL[scene]))
        _same(first, want[0], f"{scene} depth {depth}: 6 plain")
        assert hl.tolist() == L.tolist() and len(L) > 0
        _same_listed(second, want[1], L, n, f"{scene} depth {depth}: 6 listed")
    assert (got[0][2][0][4] != got[None][2][0][4]).any(), "the depth does not show in the counts"


@pytest.mark.gpu
def test_gpu_crowd_scene_through_the_list(qr, oracle, rays_mod, tmp_path):
    """the crowd scene with a grid over a flat list (crowd_flat_dda), the adversarial family "mixed" with a seeded spread: 6
    plain, the list, 6 listed"""
    name, tol, rm = "crowd_flat_dda", TOL["patched:demo01_160"], rays_mod
    plain = RS.scene_blob(name)
    blob = _ptpatch.pt_patch(plain)
    off, img = RS.query_image(qr, name, tmp_path)
    r = RS.family(plain, name, "mixed", oracle, RS.dda_grid(off, img), RS.reach_of(img))
    n = len(r)
    assert n > 64
    sp = TPR._family_spread(name, "mixed", n)
    with RS.upload_env(name):
        scn = qr.Scene(blob, ray_queries=True)
    rt, st = _t(scn, r), _t(scn, sp)
    acc = TPA._acc(scn, n, tol=tol)
    first = _step(acc, rt, 6, st)
    index, count = acc.open_list()
    hl = _host(index).view(np.uint32)[:int(_host(count)[0])]
    second = _listed(acc, rt, st, 6, index, count)
    scn.close()
    w1 = _truth_call(rm, blob, r, sp, _fresh(rm, n), 6, MIN, MAX, tol)
    w2 = _truth_call(rm, blob, r, sp, w1[0], 6, MIN, MAX, tol)
    L = rm.pt_adapt_open_list(w1[0], MIN, MAX, _tol2(tol))
    print(f"{name}: {n} rays, {len(L)} open after 6 candidates, {w2[2]} after 12")
    _same(first, w1, f"{name}: 6 plain")
    assert hl.tolist() == L.tolist() and 0 < len(L) < n
    _same_listed(second, w2, L, n, f"{name}: 6 listed")


@pytest.mark.gpu
def test_gpu_list_refusals(qr, rays_mod):
    """every refusal of the two calls, each followed by a check that state, index, count, rgb and open are unchanged; then the
    empty calls; then a step that works"""
    import torch
    scene = "pt:test18_160_pt"
    blob, rm = _base(scene), rays_mod
    r, sp = _view_rays(rm, scene, VIEW[scene])
    n = 130
    r, sp = r[:n], sp[:n]
    L = qr.lib()
    dev = "cuda:0"
    rt, st = torch.from_numpy(r.copy()).to(dev), torch.from_numpy(sp.copy()).to(dev)
    rgb = torch.full((n, 3), SF, dtype=torch.float32, device=dev)
    op = torch.full((2,), SI, dtype=torch.int32, device=dev)
    index = torch.arange(n + 2, dtype=torch.int32, device=dev)
    count = torch.tensor([n, SI], dtype=torch.int32, device=dev)
    work = torch.full((16,), SI, dtype=torch.int32, device=dev)
    vp = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)
    plain = qr.Scene(blob)
    scn = qr.Scene(blob, ray_queries=True)
    acc = scn.pt_adaptive(n, MIN, MAX, 0.1)
    state = acc.state
    before = _host(state).copy()
    t2 = float(acc.tol2)

    def step(s, rays=vp(rt), spread=vp(st), n=n, state=vp(state), index=vp(index), count=vp(count), cap=n, samples=1, mn=MIN, mx=MAX,
             tol2=t2, rgb=vp(rgb), open=vp(op), flags=0):
        return L.qr_pt_adapt_list_rays_async(s, rays, spread, n, state, index, count, cap, samples, mn, mx, ctypes.c_float(tol2), rgb,
                                             open, flags, None)

    def lst(s, state=vp(state), n=n, mn=MIN, mx=MAX, tol2=t2, index=vp(index), count=vp(count), work=vp(work), flags=0):
        return L.qr_pt_adapt_open_list_async(s, state, n, mn, mx, ctypes.c_float(tol2), index, count, work, flags, None)

    def refused(rc, want, text):
        assert rc == want and text in L.qr_last_error().decode(), (rc, L.qr_last_error().decode())
        torch.cuda.synchronize()
        assert bool((rgb == SF).all()) and bool((op == SI).all()) and (_host(state) == before).all() and bool((work == SI).all()) \
            and count.tolist() == [n, SI] and index.tolist() == list(range(n + 2)), "a refused call wrote something"

    for call in (step, lst):
        refused(call(plain._h), UNSUP, "QR_UPLOAD_RAY_QUERIES")
        refused(call(None), ARG, "null scene")
        for kw in (dict(n=-1), dict(n=1 << 31), dict(n=1 << 40)):
            refused(call(scn._h, **kw), ARG, "ray count")
        for kw in (dict(flags=1), dict(flags=2), dict(flags=0x80000000)):
            refused(call(scn._h, **kw), ARG, "flags")
        for kw in (dict(state=None), dict(index=None), dict(count=None)):
            refused(call(scn._h, **kw), ARG, "null argument")
        for kw in (dict(state=vp(state, 2)), dict(index=vp(index, 1)), dict(index=vp(index, 2)), dict(count=vp(count, 1)), dict(count=vp(count, 2))):
            refused(call(scn._h, **kw), ARG, "4-byte aligned")
        for kw in (dict(mn=-1), dict(mx=0, mn=0), dict(mx=-5, mn=-7), dict(mn=13), dict(mn=3, mx=2), dict(mx=1 << 24), dict(mx=0x7FFFFFFF, mn=0)):
            refused(call(scn._h, **kw), ARG, "min_samples and max_samples")
        for bad in (-1e-30, -1.0, float("nan"), float("inf"), float("-inf")):
            refused(call(scn._h, tol2=bad), ARG, "tol2")
    plain.close()
    refused(lst(scn._h, work=None), ARG, "null argument")
    for off in (1, 2):
        refused(lst(scn._h, work=vp(work, off)), ARG, "4-byte aligned")
    refused(step(scn._h, rays=None), ARG, "null argument")
    for kw in (dict(rays=vp(rt, 4)), dict(rays=vp(rt, 8)), dict(spread=vp(st, 4)), dict(spread=vp(st, 8))):
        refused(step(scn._h, **kw), ARG, "16-byte aligned")
    for kw in (dict(rgb=vp(rgb, 1)), dict(rgb=vp(rgb, 2)), dict(open=vp(op, 1)), dict(open=vp(op, 2))):
        refused(step(scn._h, **kw), ARG, "4-byte aligned")
    for kw in (dict(samples=0), dict(samples=-1), dict(samples=513)):
        refused(step(scn._h, **kw), ARG, "samples must be")
    for kw in (dict(cap=-1), dict(cap=-(1 << 40))):
        refused(step(scn._h, **kw), ARG, "cap must be")
    # the size query
    nb = ctypes.c_uint64(7)
    B = qr.PT_OPEN_BLOCK
    for k, words in ((1, 1), (B, 1), (B + 1, 2), (B * qr.PT_OPEN_CHUNK + B + 1, qr.PT_OPEN_CHUNK + 2)):
        assert L.qr_pt_adapt_list_work_bytes(scn._h, k, ctypes.byref(nb)) == 0 and nb.value == 4 * words, (k, nb.value)
    assert L.qr_pt_adapt_list_work_bytes(scn._h, -1, ctypes.byref(nb)) == ARG and L.qr_pt_adapt_list_work_bytes(scn._h, 1 << 31, ctypes.byref(nb)) == ARG
    assert L.qr_pt_adapt_list_work_bytes(scn._h, n, None) == ARG and L.qr_pt_adapt_list_work_bytes(None, n, ctypes.byref(nb)) == ARG
    # the empty calls: no launch
    assert step(scn._h, n=0) == 0 and step(scn._h, cap=0) == 0 and lst(scn._h, n=0) == 0
    assert step(scn._h, n=0, rays=None, spread=None, state=None, index=None, count=None, rgb=None, open=None) == 0
    assert lst(scn._h, n=0, state=None, index=None, count=None, work=None) == 0
    torch.cuda.synchronize()
    assert (rgb == SF).all() and (op == SI).all() and (_host(state) == before).all() and count.tolist() == [n, SI] and (work == SI).all()

    # the Python object
    for kw in (dict(index=index[:n]), dict(count=count[:1]), dict(cap=3)):
        with pytest.raises(qr.QrError, match="index needs count|belong to a list"):
            acc.step(rt, **kw)
    for bad in (index.float(), index.cpu(), index[::2], index.reshape(2, -1), [1, 2]):
        with pytest.raises(qr.QrError, match="index must be"):
            acc.step(rt, index=bad, count=count[:1])
    for bad in (count, count.float()[:1], count.cpu()[:1], 3):
        with pytest.raises(qr.QrError, match="count must be"):
            acc.step(rt, index=index, count=bad)
    for bad in (-1, n + 3, 1.5):
        with pytest.raises(qr.QrError, match="cap must be"):
            acc.step(rt, index=index, count=count[:1], cap=bad)
    for bad in (index, index[:n].float(), index[:n].cpu()):
        with pytest.raises(qr.QrError, match="index must be"):
            acc.open_list(index=bad)
    with pytest.raises(qr.QrError, match="count must be"):
        acc.open_list(count=count)
    torch.cuda.synchronize()
    assert (op == SI).all() and (_host(acc.state).view(np.uint32) == _fresh(rm, n)).all() and count.tolist() == [n, SI]

    got = _listed(acc, rt, st, 3, index, count[:1])                # entries n and n + 1 lie past count
    scn.close()
    want = _truth_call(rm, blob, r, sp, _fresh(rm, n), 3, MIN, MAX, 0.1)
    _same_listed(got, want, np.arange(n), n, f"{scene}: after the refusals")


# Once more through the guarded diagnostic build (make guard: QR_STATS + QR_GUARD), as the other feature files do: the small list
# shapes and one indexed step.  The library is chosen when the package is imported, hence the child process.

def _guard_child():
    from qr_loader import load_package
    qr = load_package()
    assert qr.LIB_PATH == GUARD_LIB, qr.LIB_PATH
    rm = _rays_mod()
    scene, j = TPA.GUARD_CASE
    r, sp = _view_rays(rm, scene, j)
    n = len(r)
    scn = qr.Scene(_base(scene), ray_queries=True)
    for k in _list_sizes(qr)[:8]:
        for pattern in PATTERNS:
            _list_case(qr, rm, scn, k, pattern)
    acc = TPA._acc(scn, n, tol=TOL[scene])
    rt, st = _t(scn, r), _t(scn, sp)
    first = _step(acc, rt, 6, st)
    index, count = acc.open_list()
    hl = _host(index).view(np.uint32)[:int(_host(count)[0])]
    second = _listed(acc, rt, st, 6, index, count)
    scn.close()
    want = _truth(rm, scene, j, True, (6, 6))
    L = rm.pt_adapt_open_list(want[0][0], MIN, MAX, _tol2(TOL[scene]))
    _same(first, want[0], f"{scene}: guarded build, 6 plain")
    assert hl.tolist() == L.tolist()
    _same_listed(second, want[1], L, n, f"{scene}: guarded build, 6 listed")
    print(f"{scene} guard_ok 1", flush=True)
    return 0


@pytest.mark.gpu
def test_gpu_guarded_build_gives_the_same_lists_and_steps():
    assert os.path.exists(GUARD_LIB), "libqrhip_guard.so is missing: build() makes it (make -C quadray-engine_amd/csrc guard)"
    env = dict(os.environ, QR_LIB=GUARD_LIB)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-child"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.count("guard_ok 1") == 1 and "QR_GUARD" not in out.stderr, out.stdout + out.stderr[-3000:]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.exit(_guard_child() if "--guard-child" in sys.argv else 2)
