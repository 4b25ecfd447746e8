"""Path-tracer mode (the reference's RT_FEAT_PT).

Two modes.  The reference's own frames (tests/golden/pt/, made by tests/golden/make_pt_golden.py from oracle/_ref with the
smallpt Cornell box, test18) pin the eager mode directly and the oracle's path tracer on the CPU (tests/test_pt_oracle.py);
the oracle then pins the fast mode on any scene:

* EAGER (set_pt(True, eager=True)): the reference's frames, bit-exact.  The reference shades eagerly -- every hit that
  passes the depth test while a list is walked is shaded at once, and in path-tracer mode that shading draws random numbers
  -- so a sample's stream depends on that order.  The eager machine (csrc/qr_pt_eager.hpp) follows it and reproduces the
  reference's frames pixel for pixel: recursion depths 0..10, 1 to 512 accumulated frames, 4x FSAA, Gamma, Fresnel.  On
  scenes the reference cannot light (emission patched onto CSG / trnode / textured fixtures, tests/_ptpatch.py) it equals
  the oracle's reference order: two independent statements of that order.
* FAST (set_pt(True)): the fast kernel with deferred shading: same generator, per-sample seeds (rt_Scene::reset_pseed),
  sampling formulas (tent-filter jitter, cosine hemisphere with the reference's power series, Russian roulette, Fresnel
  split) and running-mean accumulation, numbers drawn for the final hit of a walk only, children in the order DESIGN.md 4
  "Path-tracer instance" numbers.  Its frames are THE ORACLE'S (oracle.render_pt(order="kernel")) BIT FOR BIT, on any scene,
  depth and frame count; the reference's in distribution (the statistical tests below: the only link to the reference's own
  images that does not pass through this project's reading of the order), and in bits wherever the orders coincide (depth 0).
"""
import gzip
import os
import struct

import subprocess
import sys

import numpy as np
import pytest

import _ptpatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT = os.path.join(ROOT, "tests", "golden", "pt")


def _blob(name):
    return gzip.decompress(open(os.path.join(PT, name + ".qrs.gz"), "rb").read())


def _ref(name, w, h):
    return np.frombuffer(gzip.decompress(open(os.path.join(PT, name + ".raw.gz"), "rb").read()), dtype=np.uint32).reshape(h, w)


def _rgb(a):
    return np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], -1).astype(np.float64)


def _blocks(a, b=8):
    h, w, _ = a.shape
    return a.reshape(h // b, b, w // b, b, 3).mean((1, 3))


def test_pt_snapshot_carries_the_flag_and_the_emission():
    """The walker captures path-tracer snapshots (qr_frame.pt_on, qr_material.emis = mat_COL_R/G/B); ordinary snapshots
    keep zeros there, so every older fixture is unchanged."""
    b = _blob("test18_160_pt")
    hdr = struct.unpack_from("<32I", b, 0)
    n_mat, off_frame, off_mat = hdr[5], hdr[10], hdr[12]
    fr = np.frombuffer(b, dtype=np.int32, count=49, offset=off_frame)
    assert fr[41] == 1                                        # qr_frame.pt_on
    m = np.frombuffer(b, dtype=np.float32, count=n_mat * 32, offset=off_mat).reshape(n_mat, 32)
    emis = m[:, 21:24]
    assert (emis == 12.0).all(axis=1).sum() >= 1              # smallpt's light: emission (12, 12, 12)
    assert (emis == 0.0).all(axis=1).sum() >= n_mat - 2
    plain = gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "test18_160.qrs.gz"), "rb").read())
    h2 = struct.unpack_from("<32I", plain, 0)
    m2 = np.frombuffer(plain, dtype=np.float32, count=h2[5] * 32, offset=h2[12]).reshape(h2[5], 32)
    assert (m2[:, 21:24] == 0.0).all()
    assert np.frombuffer(plain, dtype=np.int32, count=49, offset=h2[10])[41] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("snap,ref,n,mean_tol,block_tol", [
    ("test18_160_pt", "test18_160_pt_n64", 64, 1.0, 8.0),
    ("test18_160_pt", "test18_160_pt_n512", 512, 0.6, 3.0),
    ("test18_160_gf_aa4_pt", "test18_160_gf_aa4_pt_n128", 128, 0.8, 3.0),
])
def test_gpu_path_tracer_has_the_references_distribution(qr, snap, ref, n, mean_tol, block_tol):
    """N accumulated frames against N accumulated frames of the reference: channel means of the whole frame and the
    means of 8x8 pixel blocks.  Measured on MI355X: channel means within 0.2 of 255, block means 5.1 / 1.8 / 1.7 apart
    on average (two independent estimates of the same image: the distance shrinks with sqrt(N))."""
    import torch
    scn = qr.Scene(_blob(snap))
    want = _rgb(_ref(ref, scn.width, scn.height))
    plain = _rgb(scn.render().cpu().numpy().view(np.uint32))         # ray-traced frame of the same snapshot
    scn.set_pt(True)
    f = scn.new_frame()
    for _ in range(n):
        scn.render(f)
    torch.cuda.synchronize()
    got = _rgb(f.cpu().numpy().view(np.uint32))
    assert np.abs(got.mean((0, 1)) - want.mean((0, 1))).max() < mean_tol
    assert np.abs(_blocks(got) - _blocks(want)).mean() < block_tol
    # the statistic can tell images apart: the ray-traced frame of the same scene is far away from the reference's
    assert np.abs(plain.mean((0, 1)) - want.mean((0, 1))).max() > 20.0
    assert np.abs(_blocks(plain) - _blocks(want)).mean() > 4 * block_tol


@pytest.mark.gpu
def test_gpu_path_tracer_is_deterministic_and_restartable(qr, oracle):
    """Same seeds, same frames: two accumulations of 16 frames are bit-identical; set_pt(True) restarts the mean;
    set_pt(False) gives the ray-traced frame again, which is the oracle's (emission and the flag change nothing there)."""
    import torch
    blob = _blob("test18_160_pt")
    scn = qr.Scene(blob)
    runs = []
    for _ in range(2):
        scn.set_pt(True)
        f = scn.new_frame()
        for _ in range(16):
            scn.render(f)
        torch.cuda.synchronize()
        runs.append(f.cpu().numpy().copy())
    assert (runs[0] == runs[1]).all()
    one = scn.new_frame()
    scn.set_pt(True); scn.render(one); torch.cuda.synchronize()
    assert (one.cpu().numpy() != runs[0]).any()                       # one sample is not the mean of sixteen
    scn.set_pt(False)
    rt = scn.render(); torch.cuda.synchronize()
    o_frame, _, _ = oracle.render(blob, threads=4)
    assert (rt.cpu().numpy().view(np.uint32) == o_frame).all()
    scn.set_pt(True)
    with pytest.raises(qr.QrError):
        scn.render_count()                                            # counting renders are refused in this mode
    with pytest.raises(qr.QrError):
        qr.MultiRender([(scn, scn.new_frame(), 0, scn.height)])()    # and so are multi-target launches
    # a path-traced frame is one more sample of EVERY pixel: cut into row-range launches the sample count would advance
    # once per launch and weigh the later ranges wrongly -- refused, and nothing is counted by the refused call
    two = scn.new_frame(); scn.render(two); torch.cuda.synchronize()
    for sel in ((scn.set_rows, (0, scn.height // 2)), (scn.set_rows, (0, scn.height, 1, 2)), (scn.set_tile_rows, (1, 2))):
        sel[0](*sel[1])
        with pytest.raises(qr.QrError):
            scn.render(two)
        with pytest.raises(qr.QrError):
            scn.render_host()
    scn.set_rows(0, scn.height)
    scn.set_pt(True)
    again = scn.new_frame(); scn.render(again); torch.cuda.synchronize()
    assert (again.cpu().numpy() == one.cpu().numpy()).all()           # whole frames work as before


@pytest.mark.gpu
@pytest.mark.parametrize("ref,fsaa", [("test18_160_pt_d0_n1", 0), ("test18_160_aa4_pt_d0_n1", 2)])
def test_gpu_path_tracer_first_frame_depth0_is_bit_exact(qr, ref, fsaa):
    """qr_ref --scene test18 --depth 0 --pt 1 [--fsaa 4]: the reference's first path-traced frame without recursion."""
    import torch
    b = bytearray(_blob("test18_160_pt"))
    if fsaa:
        # same scene with 4x FSAA: the engine's sample offsets (engine.cpp:3525-3546 pattern, as in the aa4 snapshot)
        a = _blob("test18_160_gf_aa4_pt")
        oa, ob = struct.unpack_from("<I", a, 40)[0], struct.unpack_from("<I", b, 40)[0]
        fa = np.frombuffer(a, dtype=np.uint32, count=49, offset=oa)
        fb = np.frombuffer(bytes(b), dtype=np.uint32, count=49, offset=ob).copy()
        fb[10:18] = fa[10:18]; fb[30] = fa[30]                 # hor_a / ver_a, fsaa
        b[ob:ob + 196] = fb.tobytes()
    scn = qr.Scene(bytes(b))
    scn.set_depth(0)
    scn.set_pt(True)
    f = scn.render(); torch.cuda.synchronize()
    want = _ref(ref, scn.width, scn.height)
    assert int((want != 0).sum()) > 100
    assert int((f.cpu().numpy().view(np.uint32) != want).sum()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("depth,frames,allowed", [(2, 2, 0), (6, 2, 0), (8, 1, 0), (8, 2, 0), (10, 1, 0), (10, 2, 0), (10, 4, 0)])
def test_gpu_eager_path_tracer_reproduces_the_references_frames(qr, depth, frames, allowed):
    """set_pt(True, eager=True): shading in the reference's order (csrc/qr_pt_eager.hpp) -- every hit that passes the
    depth test is shaded at once, bounce subtree first, then the Fresnel split, refraction, reflection -- so a sample
    consumes the reference's numbers.  Pixel for pixel the reference's frames (qr_ref --pt N) at every recursion depth up
    to the default 10, first frame and accumulated ones (frame k's jitter depends on every number frames 1..k-1 drew)."""
    import torch
    scn = qr.Scene(_blob("test18_160_pt"))
    scn.set_depth(depth)
    scn.set_pt(True, eager=True)
    f = scn.new_frame()
    for _ in range(frames):
        scn.render(f)
    torch.cuda.synchronize()
    want = _ref("test18_160_pt_d%d_n%d" % (depth, frames), scn.width, scn.height)
    assert int((f.cpu().numpy().view(np.uint32) != want).sum()) <= allowed


@pytest.mark.gpu
@pytest.mark.parametrize("frames", [64, 512])
def test_gpu_eager_path_tracer_accumulates_the_references_image(qr, frames):
    """N accumulated frames at the default depth: every one of the N x 19 200 streams stays the reference's to the end."""
    import torch
    scn = qr.Scene(_blob("test18_160_pt"))
    scn.set_pt(True, eager=True)
    f = scn.new_frame()
    for _ in range(frames):
        scn.render(f)
    torch.cuda.synchronize()
    want = _ref("test18_160_pt_n%d" % frames, scn.width, scn.height)
    assert int((f.cpu().numpy().view(np.uint32) != want).sum()) == 0


@pytest.mark.gpu
def test_gpu_eager_path_tracer_with_fsaa_gamma_fresnel(qr):
    """4x FSAA (four samples per pixel, each with its own stream), Gamma, Fresnel (the split of Fresnel surfaces between
    reflection and refraction draws numbers): the reference's first three accumulated frames, pixel for pixel."""
    import torch
    scn = qr.Scene(_blob("test18_160_gf_aa4_pt"))
    scn.set_pt(True, eager=True)
    f = scn.new_frame()
    for _ in range(3):
        scn.render(f)
    torch.cuda.synchronize()
    want = _ref("test18_160_gf_aa4_pt_n3", scn.width, scn.height)
    assert int((want != 0).sum()) > 1000
    assert int((f.cpu().numpy().view(np.uint32) != want).sum()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["test18_160", "demo01_160", "demo02_160", "demo03_160", "test09_160", "test13_160", "test16_160",
                                  "swarm_demo01_240_mix", "test11_160_j7"])
def test_gpu_eager_machine_with_ray_tracer_shading_is_the_ray_tracer(qr, name):
    """Self-test of the eager machine: with the ray tracer's shading (lights, shadows, no random numbers) shading every
    provisional hit cannot change a pixel, so its frame is the deferred kernel's, at every depth -- also on the scenes
    whose surfaces carry clipper programs (CSG), which the machine's walk runs per lane."""
    import torch
    blob = gzip.decompress(open(os.path.join(ROOT, "tests", "golden", name + ".qrs.gz"), "rb").read())
    scn = qr.Scene(blob)
    for depth in (10, 3, 0):
        scn.set_depth(depth)
        rt = scn.render(); torch.cuda.synchronize()
        qr._check(qr.lib().qr_scene_set_pt(scn._h, 3))
        f = scn.render(); torch.cuda.synchronize()
        qr._check(qr.lib().qr_scene_set_pt(scn._h, 0))
        assert int((f != rt).sum().item()) == 0


# ---- the fast kernel is the oracle's kernel order, bit for bit (DESIGN.md 4 "Path-tracer instance", order of draws) ----

GUARD_LIB = os.path.join(ROOT, "quadray-engine_amd", "libqrhip_guard.so")
_ORACLE_FRAMES = {}


def _scene_blob(name):
    """'pt:<snapshot under tests/golden/pt>' or 'patched:<fixture with emission patched on>' (tests/_ptpatch.py)"""
    kind, n = name.split(":")
    if kind == "pt":
        return _blob(n)
    if n == "synth_small":
        import _rayset
        return _ptpatch.pt_patch(_rayset.scene_blob(n))
    return _ptpatch.patched(n)


def _want(oracle, name, frames, depth, order="kernel"):
    """the oracle's frame, computed once per module"""
    key = (name, frames, depth, order)
    if key not in _ORACLE_FRAMES:
        _ORACLE_FRAMES[key] = oracle.render_pt(_scene_blob(name), frames, depth=-1 if depth is None else depth, order=order, threads=16)
    return _ORACLE_FRAMES[key]


def _gpu_frames(scn, frames, depth=None, eager=False, keep=()):
    """`frames` accumulated frames; returns the last one (and those after the frame counts in `keep`)"""
    import torch
    if depth is not None:
        scn.set_depth(depth)
    scn.set_pt(True, eager=eager)
    f = scn.new_frame()
    kept = {}
    for i in range(1, frames + 1):
        scn.render(f)
        if i in keep:
            torch.cuda.synchronize()
            kept[i] = f.cpu().numpy().view(np.uint32).copy()
    torch.cuda.synchronize()
    out = f.cpu().numpy().view(np.uint32).copy()
    return (out, kept) if keep else out


def _same(got, want, what):
    d = got != want
    if d.any():
        ys, xs = np.nonzero(d)
        print("%s: %d of %d pixels differ, first at x=%d y=%d: kernel %06x oracle %06x"
              % (what, int(d.sum()), d.size, xs[0], ys[0], got[ys[0], xs[0]], want[ys[0], xs[0]]))
    assert int(d.sum()) == 0, what


PATCHED_DEPTHS = [(n, d) for n in _ptpatch.PATCHED_SCENES for d in (None, 6)]


@pytest.mark.gpu
@pytest.mark.parametrize("frames", [1, 4])
@pytest.mark.parametrize("depth", [0, 1, 2, 3, 5, 6, 7, 10])
def test_gpu_fast_path_tracer_is_the_oracles_kernel_order_on_test18(qr, oracle, depth, frames):
    """Levels 3 and 6 are where the Fresnel split and the roulette switch on at the default depth; at a smaller depth they
    come sooner (both compare inf_DEPTH with RT_STACK_DEPTH, tracer.cpp:2354, 3433)."""
    got = _gpu_frames(qr.Scene(_blob("test18_160_pt")), frames, depth)
    _same(got, _want(oracle, "pt:test18_160_pt", frames, depth), "test18 depth %d, %d frames" % (depth, frames))


@pytest.mark.gpu
@pytest.mark.parametrize("frames", [3, 16])
def test_gpu_fast_path_tracer_is_the_oracles_with_fsaa_gamma_fresnel(qr, oracle, frames):
    got = _gpu_frames(qr.Scene(_blob("test18_160_gf_aa4_pt")), frames)
    _same(got, _want(oracle, "pt:test18_160_gf_aa4_pt", frames, None), "test18 gf aa4, %d frames" % frames)


@pytest.mark.gpu
@pytest.mark.parametrize("name,depth", PATCHED_DEPTHS)
def test_gpu_fast_path_tracer_is_the_oracles_on_patched_scenes(qr, oracle, name, depth):
    """Bounces on clipped (CSG) surfaces, through trnode arrays, on every quadric kind, off textures; ragged frames
    (33x17 with 4x FSAA, 157x93): partial footprints, seed slots on a frame that is no multiple of anything."""
    got = _gpu_frames(qr.Scene(_ptpatch.patched(name)), 4, depth)
    _same(got, _want(oracle, "patched:" + name, 4, depth), "%s depth %s" % (name, depth))


@pytest.mark.gpu
@pytest.mark.parametrize("name", _ptpatch.PATCHED_SCENES)
def test_gpu_eager_path_tracer_is_the_oracles_reference_order_on_patched_scenes(qr, oracle, name):
    """Two independent statements of the reference's order (csrc/qr_pt_eager.hpp and the oracle's, the latter pinned to the
    reference's frames on the CPU) on content the reference's own frames cannot reach."""
    got = _gpu_frames(qr.Scene(_ptpatch.patched(name)), 2, eager=True)
    _same(got, _want(oracle, "patched:" + name, 2, None, "reference"), name)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["rebin_tiles", "QR_CULL=0", "QR_REBIN=1,QR_BIN_TILE=8x8"])
@pytest.mark.parametrize("name", ["pt:test18_160_pt", "patched:demo02_160_gf_aa4"])
def test_gpu_fast_path_tracer_does_not_depend_on_the_lists_walked(qr, oracle, name, variant):
    """Numbers are drawn at final hits only, so tile lists rebuilt on the GPU, other tile sizes and walks without cull
    cells leave every stream alone: the same oracle frame."""
    blob = _scene_blob(name)
    if variant == "rebin_tiles":
        scn = qr.Scene(blob, rebin_tiles=True)
    else:
        env = dict(kv.split("=") for kv in variant.split(","))
        os.environ.update(env)
        try:
            scn = qr.Scene(blob)
        finally:
            for k in env:
                del os.environ[k]
    _same(_gpu_frames(scn, 4), _want(oracle, name, 4, None), "%s %s" % (name, variant))


@pytest.mark.gpu
def test_gpu_fast_path_tracer_accumulates_and_restarts_like_the_oracle(qr, oracle):
    """Eight frames as eight calls: after frames 1, 2, 5 and 8 the frame is the oracle's for that count (running mean and
    seed carry-over frame by frame, not only at the end); set_pt(True) again starts over."""
    scn = qr.Scene(_blob("test18_160_pt"))
    last, kept = _gpu_frames(scn, 8, keep=(1, 2, 5, 8))
    for n in (1, 2, 5, 8):
        _same(kept[n], _want(oracle, "pt:test18_160_pt", n, None), "after %d frames" % n)
    assert (last == kept[8]).all()
    _same(_gpu_frames(scn, 1), _want(oracle, "pt:test18_160_pt", 1, None), "after the restart")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["synth_small", "swarm_demo01_240"])
def test_gpu_fast_path_tracer_on_scenes_of_the_per_lane_instance(qr, oracle, name):
    """set_pt(True) is accepted on the scenes whose ray-traced frames the per-lane walk instance serves (long hierarchies,
    grids): the path-tracer launch walks their lists with the packet instance.  Emission patched on; the oracle's frame."""
    got = _gpu_frames(qr.Scene(_scene_blob("patched:" + name)), 2)
    want = _want(oracle, "patched:" + name, 2, None)
    assert int((want != 0).sum()) > want.size // 20
    _same(got, want, name)


# one representative case once more through the guarded diagnostic build (make guard), as the other feature tests do: the
# library is chosen when the package is imported, hence the child process: this file run as a script.

def _guard_child():
    from qr_loader import load_package
    qr = load_package()
    assert qr.LIB_PATH == GUARD_LIB, qr.LIB_PATH
    import qr_oracle
    name = "patched:demo02_160_gf_aa4"
    got = _gpu_frames(qr.Scene(_scene_blob(name)), 4)
    _same(got, _want(qr_oracle, name, 4, None), "guard " + name)
    print("%s guard_ok 1" % name, flush=True)
    return 0


@pytest.mark.gpu
def test_gpu_guarded_build_gives_the_same_path_traced_frame():
    if not os.path.exists(GUARD_LIB):
        pytest.skip("libqrhip_guard.so is absent (build() makes it: make -C quadray-engine_amd/csrc guard)")
    env = dict(os.environ, QR_LIB=GUARD_LIB)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-child"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.count("guard_ok 1") == 1 and "QR_GUARD" not in out.stderr, out.stdout + out.stderr[-3000:]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.exit(_guard_child() if "--guard-child" in sys.argv else 2)
