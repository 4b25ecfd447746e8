"""The oracle's path tracer (oracle/qr_oracle.c qro_render_pt) is the reference's: CPU tests.

The chain this file holds up (tests/test_path_tracer.py holds the GPU end):

    the reference's PT frames (tests/golden/pt, made by make_pt_golden.py from oracle/_ref)
        == oracle PT, order="reference"      (here: every frame, pixel for pixel)
    oracle PT, order="kernel"                (same formulas, the fast kernel's order of draws: DESIGN.md 4)
        == Scene.set_pt(True) frames         (tests/test_path_tracer.py, on the GPU)

Reference order pins the FORMULAS (generator, seeding, tent jitter, emission, roulette, cosine-hemisphere bounce with the
power-series sin / cos, Fresnel split, running mean); the kernel order adds only the order in which a sample consumes its
stream.  Power conditions keep the pins from passing vacuously: every kind of draw must actually happen.
"""
import gzip
import os

import numpy as np
import pytest

import _ptpatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT = os.path.join(ROOT, "tests", "golden", "pt")
THREADS = 16


def _blob(name):
    return gzip.decompress(open(os.path.join(PT, name + ".qrs.gz"), "rb").read())


def _ref(name, w=160, h=120):
    return np.frombuffer(gzip.decompress(open(os.path.join(PT, name + ".raw.gz"), "rb").read()), dtype=np.uint32).reshape(h, w)


def _aa4_of_plain():
    """test18_160_pt with the 4x FSAA sample offsets of the aa4 snapshot (as tests/test_path_tracer.py builds it)."""
    import struct
    a, b = _blob("test18_160_gf_aa4_pt"), bytearray(_blob("test18_160_pt"))
    oa, ob = struct.unpack_from("<I", a, 40)[0], struct.unpack_from("<I", b, 40)[0]
    fa = np.frombuffer(a, dtype=np.uint32, count=49, offset=oa)
    fb = np.frombuffer(bytes(b), dtype=np.uint32, count=49, offset=ob).copy()
    fb[10:18] = fa[10:18]; fb[30] = fa[30]                     # hor_a / ver_a, fsaa
    b[ob:ob + 196] = fb.tobytes()
    return bytes(b)


# (snapshot, reference frame, depth or -1 for the snapshot's, accumulated frames): EVERY frame under tests/golden/pt
PINS = [
    ("test18_160_pt", "test18_160_pt_d0_n1", 0, 1),
    ("aa4", "test18_160_aa4_pt_d0_n1", 0, 1),
    ("test18_160_pt", "test18_160_pt_d2_n2", 2, 2),
    ("test18_160_pt", "test18_160_pt_d6_n2", 6, 2),
    ("test18_160_pt", "test18_160_pt_d8_n2", 8, 2),
    ("test18_160_pt", "test18_160_pt_d8_n1", 8, 1),
    ("test18_160_pt", "test18_160_pt_d10_n1", 10, 1),
    ("test18_160_pt", "test18_160_pt_d10_n2", 10, 2),
    ("test18_160_pt", "test18_160_pt_d10_n4", 10, 4),
    ("test18_160_pt", "test18_160_pt_n64", -1, 64),
    ("test18_160_pt", "test18_160_pt_n512", -1, 512),
    ("test18_160_gf_aa4_pt", "test18_160_gf_aa4_pt_n3", -1, 3),
    ("test18_160_gf_aa4_pt", "test18_160_gf_aa4_pt_n128", -1, 128),
]


def _snap(name):
    return _aa4_of_plain() if name == "aa4" else _blob(name)


def test_every_golden_pt_frame_is_pinned_here():
    have = sorted(f[:-len(".raw.gz")] for f in os.listdir(PT) if f.endswith(".raw.gz"))
    assert have == sorted(p[1] for p in PINS)


@pytest.mark.parametrize("snap,ref,depth,frames", PINS, ids=[p[1] for p in PINS])
def test_reference_order_reproduces_the_references_frames(oracle, snap, ref, depth, frames):
    """allowed = 0: after N accumulated frames every one of the N x samples streams is still the reference's (frame k's
    jitter depends on every number frames 1..k-1 drew).  512 frames of test18 take about six seconds on 16 threads."""
    want = _ref(ref)
    assert int((want != 0).sum()) > 100
    got = oracle.render_pt(_snap(snap), frames, depth=depth, order="reference", threads=THREADS)
    assert int((got != want).sum()) == 0


@pytest.mark.parametrize("snap,ref", [("test18_160_pt", "test18_160_pt_d0_n1"), ("aa4", "test18_160_aa4_pt_d0_n1")])
def test_kernel_order_at_depth_0_is_the_references_frame(oracle, snap, ref):
    """No order exists without recursion: one hit per sample, its draws, no child."""
    got = oracle.render_pt(_snap(snap), 1, depth=0, order="kernel", threads=THREADS)
    assert int((got != _ref(ref)).sum()) == 0


def test_every_kind_of_draw_happens_on_test18(oracle):
    _, st = oracle.render_pt(_blob("test18_160_pt"), 1, depth=10, order="reference", threads=THREADS, want_stats=True)
    print(st)
    assert set(st) == set(oracle.PT_STATS)
    for k in oracle.PT_STATS:
        assert st[k] > 0, k
    assert st["roulette_deaths"] < st["roulette_draws"]
    # above the roulette's level nothing is drawn for it, and above the split's level nothing is split
    _, st4 = oracle.render_pt(_blob("test18_160_pt"), 1, depth=4, order="reference", threads=THREADS, want_stats=True)
    assert st4["roulette_draws"] > 0                           # inf_DEPTH <= 5 at once: the roulette counts from RT_STACK_DEPTH
    _, st1 = oracle.render_pt(_blob("test18_160_pt"), 1, depth=1, order="kernel", threads=THREADS, want_stats=True)
    assert st1["bounces"] > 0 and st1["split_reflect"] > 0 and st1["split_refract"] > 0


def test_both_split_directions_and_the_tir_skip_on_the_fresnel_snapshot(oracle):
    for order in ("reference", "kernel"):
        _, st = oracle.render_pt(_blob("test18_160_gf_aa4_pt"), 1, order=order, threads=THREADS, want_stats=True)
        print(order, st)
        assert st["split_reflect"] > 0 and st["split_refract"] > 0 and st["split_tir_skipped"] > 0, order


def test_the_two_orders_differ_at_depth_10(oracle):
    """The known "distribution, not bits" fact: the reference shades every depth-test winner of a walk and
    lets the bounce's subtree draw before the split; the kernel draws for final hits only, bounce last.  Same image in the
    mean, other numbers per sample."""
    b = _blob("test18_160_pt")
    ref = oracle.render_pt(b, 2, depth=10, order="reference", threads=THREADS)
    ker = oracle.render_pt(b, 2, depth=10, order="kernel", threads=THREADS)
    n = int((ref != ker).sum())
    print("pixels that differ between the orders:", n)
    assert n > 0
    # and yet the same image: channel means of two 2-sample estimates of it
    rgb = lambda a: np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], -1).astype(np.float64)
    assert np.abs(rgb(ref).mean((0, 1)) - rgb(ker).mean((0, 1))).max() < 4.0


@pytest.mark.parametrize("order", ["reference", "kernel"])
def test_result_does_not_depend_on_threads(oracle, order):
    b = _blob("test18_160_gf_aa4_pt")
    one, m1, s1 = oracle.render_pt(b, 2, order=order, threads=1, want_mean=True, want_stats=True)
    many, m16, s16 = oracle.render_pt(b, 2, order=order, threads=16, want_mean=True, want_stats=True)
    assert (one == many).all() and (m1.view(np.uint32) == m16.view(np.uint32)).all() and s1 == s16


def test_trace_of_one_sample_is_its_stream(oracle):
    """qro_pt_trace_sample, the aid for telling an ordering choice from a wrong formula: the draws of one sample in order.
    Every sample starts with its two jitter numbers at level 0; a roulette is drawn only from the sixth level on; the split
    only from the third; the two orders draw the same jitter and then part ways somewhere in the frame."""
    b = _blob("test18_160_pt")
    parted = 0
    for x, y in ((80, 60), (40, 100), (120, 30), (20, 20)):
        seqs = {}
        for order in ("reference", "kernel"):
            seq, col = oracle.pt_trace_sample(b, 1, x, y, depth=10, order=order)
            assert [s for _, s, _ in seq[:2]] == ["jitter_h", "jitter_v"] and seq[0][0] == 0
            assert all(0.0 <= v < 1.0 for _, _, v in seq)
            assert all(l >= 5 for l, s, _ in seq if s == "roulette")
            assert all(l >= 2 for l, s, _ in seq if s == "split")
            assert np.isfinite(col).all()
            seqs[order] = seq
        assert seqs["reference"][:2] == seqs["kernel"][:2]
        parted += seqs["reference"] != seqs["kernel"]
    assert parted > 0


def test_existing_entry_points_ignore_the_path_tracer(oracle):
    """qro_render on a path-tracer snapshot is the ray tracer (pt_on and the emission change nothing there)."""
    plain = gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "test18_160.qrs.gz"), "rb").read())
    a, _, _ = oracle.render(_blob("test18_160_pt"), threads=4)
    b, _, _ = oracle.render(plain, threads=4)
    assert (a == b).all()


# ---- a second family of scenes: emission patched onto fixtures with CSG, trnode arrays, textures, every quadric kind ----

def test_patch_sets_the_flag_and_the_emission_only():
    import struct
    for name in _ptpatch.PATCHED_SCENES:
        a, b = _ptpatch.golden_blob(name), _ptpatch.patched(name)
        assert len(a) == len(b)
        h = struct.unpack_from("<26I", a, 0)
        wa, wb = np.frombuffer(a, dtype=np.uint32), np.frombuffer(b, dtype=np.uint32)
        changed = np.nonzero(wa != wb)[0]
        mats = _ptpatch.emitters(a)
        assert len(mats) >= 4
        allowed = {h[10] // 4 + 41} | {h[12] // 4 + 32 * m + k for m in mats for k in (21, 22, 23)}
        assert set(changed.tolist()) == allowed
        fr = np.frombuffer(b, dtype=np.int32, count=49, offset=h[10])
        assert fr[41] == 1


@pytest.mark.parametrize("order", ["reference", "kernel"])
@pytest.mark.parametrize("name", _ptpatch.PATCHED_SCENES)
def test_patched_scenes_are_lit_and_draw(oracle, name, order):
    """No frame of the reference exists for these (it cannot light them): here only that they are not black and that the
    counters fire; their use is on the GPU, against these very frames."""
    b = _ptpatch.patched(name)
    f, st = oracle.render_pt(b, 2, order=order, threads=THREADS, want_stats=True)
    print(name, order, int((f != 0).sum()), st)
    assert int((f != 0).sum()) > f.size // 5
    assert st["roulette_draws"] > 0 and st["roulette_deaths"] > 0 and st["bounces"] > 0
    if "_gf_" in name:                                          # the Fresnel captures
        assert st["split_reflect"] > 0 and st["split_refract"] > 0 and st["split_tir_skipped"] > 0
    # unpatched, the path tracer sees no emitter: black, as make_pt_golden.py notes for the demos
    if name == "demo01_160":
        assert int((oracle.render_pt(_ptpatch.golden_blob(name), 1, order=order, threads=THREADS) != 0).sum()) == 0
