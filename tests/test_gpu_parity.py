"""GPU suite: the HIP backend (through the C ABI) against the oracle and the reference's golden frames.

Bar: bit-exact 0x00RRGGBB pixels, bit-exact primary hit-id buffers, equal ray counts.
"""
import numpy as np
import pytest

from conftest import MANIFEST, SMALL_CASES, BIG_CASES, load_blob, load_frame

pytestmark = pytest.mark.gpu


def _gpu_frame(qr, blob, **kw):
    import torch
    scn = qr.Scene(blob)
    for k, v in kw.items():
        getattr(scn, k)(*v)
    frame = scn.new_frame()
    ids = torch.full_like(frame, -2)
    scn.render(frame, ids=ids)
    torch.cuda.synchronize()
    out = frame.cpu().numpy().view(np.uint32)
    return scn, out, ids.cpu().numpy()


@pytest.mark.parametrize("name", SMALL_CASES)
def test_gpu_matches_reference_frame_and_oracle(qr, oracle, name):
    blob = load_blob(name)
    ref = load_frame(name) & 0xFFFFFF
    scn, out, ids = _gpu_frame(qr, blob)
    diff = int((out != ref).sum())
    assert diff == 0, f"{name}: {diff} pixels differ from the reference frame"
    o_frame, o_ids, _ = oracle.render(blob, threads=8, want_ids=True)
    assert (out == o_frame).all()
    assert (ids == o_ids).all(), "primary hit-id buffer differs from the oracle"
    # ray counts: the backend shades only final hits, compare with the oracle in the same mode
    _, _, o_counts = oracle.render(blob, threads=8, deferred=True)
    _, c = scn.render_count()
    assert c.as_dict() == {k: o_counts[k] for k in c.as_dict()}


@pytest.mark.parametrize("name", BIG_CASES)
def test_gpu_full_size_hash_and_oracle(qr, oracle, name):
    """BASELINE.json configs at full size: reference frame hash + pixel equality with the oracle."""
    blob = load_blob(name)
    scn, out, ids = _gpu_frame(qr, blob)
    assert oracle.frame_hash(out) == int(MANIFEST[name]["hash"], 16)
    o_frame, o_ids, _ = oracle.render(blob, threads=16, want_ids=True)
    assert (out == o_frame).all()
    assert (ids == o_ids).all()
    _, _, o_counts = oracle.render(blob, threads=16, deferred=True)
    _, c = scn.render_count()
    assert c.as_dict() == {k: o_counts[k] for k in c.as_dict()}


def test_gpu_depth_override_matches_oracle(qr, oracle):
    blob = load_blob("demo02_160_gf_aa4")
    for depth in (0, 1, 2, 5):
        scn, out, _ = _gpu_frame(qr, blob, set_depth=(depth,))
        o_frame, _, _ = oracle.render(blob, depth=depth, threads=8)
        assert (out == o_frame).all(), f"depth {depth}"


def test_gpu_row_interleave_and_tile_row_sharding_compose(qr):
    """index/thnum slices and round-robin tile-row shards each compose to the whole frame
    (idempotence of the partition; this is the multi-GPU decomposition)."""
    import torch
    blob = load_blob("c1_demo01_640x480")
    scn, whole, _ = _gpu_frame(qr, blob)
    acc = torch.zeros((scn.height, scn.width), dtype=torch.int32, device="cuda")
    for idx in range(3):
        scn.set_rows(0, scn.height, idx, 3)
        scn.render(acc)
    torch.cuda.synchronize()
    assert (acc.cpu().numpy().view(np.uint32) == whole).all()
    acc.zero_()
    for r in range(4):
        scn.set_tile_rows(r, 4)
        scn.render(acc)
    torch.cuda.synchronize()
    assert (acc.cpu().numpy().view(np.uint32) == whole).all()


def test_gpu_render_host_matches_device_path(qr):
    blob = load_blob("demo03_160")
    scn, out, _ = _gpu_frame(qr, blob)
    assert (scn.render_host() == out).all()


def test_gpu_is_deterministic(qr):
    blob = load_blob("demo02_160_gf_t5000")
    _, a, _ = _gpu_frame(qr, blob)
    _, b, _ = _gpu_frame(qr, blob)
    assert (a == b).all()


def test_gpu_drop_in_through_reference_engine():
    """The UNMODIFIED reference engine (prebuilt oracle/_ref/qr_ref_shim), linked with the shim TU in
    place of tracer_128v8.cpp, renders once with its own CPU SIMD backend and once through
    qr_render0 -> HIP; the driver compares the two frames."""
    import os
    import subprocess
    import tempfile
    from conftest import ROOT
    exe = os.path.join(ROOT, "oracle", "_ref", "qr_ref_shim")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/qr_ref_shim was not built (needs /root/reference at build time)")
    tmp = tempfile.mkdtemp(prefix="qrdrop_")
    os.makedirs(os.path.join(tmp, "dump"), exist_ok=True)
    for args in (["--scene", "demo01", "-w", "640", "-h", "480"],
                 ["--scene", "demo02", "-w", "320", "-h", "240", "--gamma", "--fresnel", "--fsaa", "4", "-t", "3000"],
                 ["--scene", "test13", "-w", "200", "-h", "150", "--opts", "none"],
                 # the engine's own thread pool: qr_render0 entered concurrently from 4 threads, each
                 # owning every fourth row (index / thnum, tracer.cpp:1144-1145)
                 ["--scene", "demo03", "-w", "333", "-h", "211", "--threads", "4", "--fsaa", "2"]):
        out = subprocess.run([exe] + args + ["--gpu"], cwd=tmp, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "MATCH" in out.stdout and "MISMATCH" not in out.stdout, out.stdout


@pytest.mark.parametrize("args", [["-w", "160", "-h", "120", "--pt", "3"],
                                  ["-w", "200", "-h", "150", "--pt", "4", "--fsaa", "4", "--gamma", "--fresnel"],
                                  ["-w", "160", "-h", "120", "--pt", "3", "--threads", "4"],
                                  ["-w", "96", "-h", "64", "--pt", "2", "--depth", "4"],
                                  # path tracer on -> a frame -> off -> a ray-traced frame -> on again: the ray-traced frame must
                                  # zero the sample count in s_inf (FF_ini, tracer.cpp:1128-1132) or the restarted accumulation
                                  # weighs its first frame as the second
                                  ["-w", "128", "-h", "96", "--pt", "3", "--pt-warm"],
                                  ["-w", "128", "-h", "96", "--pt", "2", "--pt-warm", "--threads", "4", "--fsaa", "2"]])
def test_gpu_drop_in_path_tracer_through_reference_engine(args):
    """Path-tracer mode through the drop-in boundary: the unmodified engine accumulates N frames with its own CPU SIMD
    backend in one process and, in another, with EVERY frame going through ref_shim.cpp -> qr_render0 (--shim): the
    engine's seed and colour planes travel to the GPU and back each frame, the eager path-tracer kernel draws the
    reference's numbers.  The N-th frames must be equal (the driver prints the frame hash)."""
    import os
    import subprocess
    import tempfile
    from conftest import ROOT
    exe = os.path.join(ROOT, "oracle", "_ref", "qr_ref_shim")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/qr_ref_shim was not built (needs /root/reference at build time)")
    tmp = tempfile.mkdtemp(prefix="qrdroppt_")
    os.makedirs(os.path.join(tmp, "dump"), exist_ok=True)
    hashes = []
    for extra in ([], ["--shim"]):
        out = subprocess.run([exe, "--scene", "test18"] + args + extra, cwd=tmp, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        hashes.append([l.split()[1] for l in out.stdout.splitlines() if l.startswith("hash ")][0])
        if extra:
            assert "simd 128x1v8" in out.stdout, out.stdout       # the shim's target was the one rendering
    assert hashes[0] == hashes[1], hashes


@pytest.mark.parametrize("ranks,mode", [(2, []), (2, ["--gather"]), (4, []), (3, ["--gather"]), (2, ["--split-frame"]), (3, ["--split-frame"])])
def test_gpu_two_rank_bench_path_on_one_gpu(ranks, mode):
    """The N > 1 code path of bench.py -- MultiRender (one multi-target launch per step), the buffer rotation and
    the grouped exchange / gather -- with the HIP renderer, all ranks on this one GPU (gloo carries the exchange:
    RCCL refuses two ranks on one device).  The assembled frames must equal the reference-checked frame.
    2, 3 and 4 ranks: 135 tile rows do not divide by 4, and with 3 every rank's blocks sit elsewhere."""
    import json
    import os
    import socket
    import subprocess
    import sys
    from conftest import ROOT
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, QR_BENCH_SAME_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(ranks), "--steps", "7", "--warmup", "2",
           "--workload", "demo2_1080p_gf_d3", "--full", "--no-cpu-baseline"] + mode
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    j = json.loads(line)
    assert j["n_gpus"] == ranks and j["config"]["frame_check"]["ok"] is True
    assert j["config"]["frame_check"]["timed_frames_match"] is True and j["config"]["assembled_frame_matches"] is True
    assert j["collective"]["ranks"] == ranks and j["collective"]["backend"] == "gloo"
    assert j["collective"]["exchange_groups"] >= 1 and j["collective"]["exchange_ms_per_step"] >= 0.0
    assert j["scaling"] == ("strong" if "--split-frame" in mode else "weak")
    assert j["config"]["frames_per_step"] == (1 if "--split-frame" in mode else ranks)


def test_gpu_rccl_communicator_beside_the_hip_library():
    """RCCL itself, as far as one GPU can take it: the `nccl` backend of torch.distributed with world size 1 in a process
    that has libqrhip.so's HIP kernels loaded -- a communicator is created, a rendered frame goes through an all_gather, an
    all_reduce and the sharding module's exchange / gather / split-frame paths on the backend bench.py uses with N > 1
    (two HIP runtimes in one process would fail here: quadray-engine_amd/__init__.py loads torch's first).  What this does
    NOT show is traffic between two devices: no such box exists in this pipeline."""
    import os
    import socket
    import subprocess
    import sys
    from conftest import ROOT
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_nccl_world1.py")], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "rccl ok" in out.stdout, out.stdout


def test_gpu_drop_in_bench_1080p_matches_and_reports_split(capsys):
    """BASELINE's headline configuration through the actual boundary: the unmodified engine renders demo scene 1 at
    1920x1080 with its own backend and through qr_render0, frozen and animated (33 ms per frame: the engine
    rebuilds every list, nothing can be reused); frames must match; the per-call split is printed."""
    import os
    import re
    import subprocess
    import tempfile
    from conftest import ROOT
    exe = os.path.join(ROOT, "oracle", "_ref", "qr_ref_shim")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/qr_ref_shim was not built (needs /root/reference at build time)")
    tmp = tempfile.mkdtemp(prefix="qrdropb_")
    os.makedirs(os.path.join(tmp, "dump"), exist_ok=True)
    report = []
    for extra in ([], ["--animate", "33"], ["--pin-frame"], ["--animate", "33", "--pin-frame"]):
        out = subprocess.run([exe, "--scene", "demo01", "-w", "1920", "-h", "1080", "--gpu", "--bench", "50"] + extra,
                             cwd=tmp, capture_output=True, text=True, timeout=600, env=dict(os.environ, QR_VERBOSE="1"))
        assert out.returncode == 0, out.stdout + out.stderr
        assert "MATCH" in out.stdout and "MISMATCH" not in out.stdout, out.stdout
        if "--animate" in extra:
            assert "ANIM_MATCH" in out.stdout, out.stdout
        line = [l for l in out.stdout.splitlines() if l.startswith("gpu_bench")][0]
        cpu = [l for l in out.stdout.splitlines() if l.startswith("bench ")][0]
        # the split of a frame of the timed loop (the last two calls of an animated run re-render one scene time)
        split = [l for l in out.stderr.splitlines() if l.startswith("qr_render0:")][-3 if "--animate" in extra else -1]
        report += [" ".join(extra) or "(frozen)", cpu, line, split]
        # rt_Scene::render through the HIP backend, median of 50 frames: 0.66-0.80 ms frozen, 1.18-1.26 ms animated on the rounds'
        # boxes (DESIGN.md 5 "Drop-in"); the bounds catch a regression of 1.5x without tripping on a slower host
        med = float(re.search(r"median_ms ([0-9.]+)", line).group(1))
        assert med < (2.0 if "--animate" in extra else 1.2), (extra, line, split)
    with capsys.disabled():
        print("\n" + "\n".join(report))


@pytest.mark.parametrize("name", SMALL_CASES + BIG_CASES)
def test_gpu_tile_binning_keeps_frames(qr, name):
    """QR_UPLOAD_REBIN_TILES: tile lists rebuilt on the GPU from the camera list (replaces the engine's
    host tiling, engine.cpp:1956-2128) give the reference's pixels, hit ids and ray counts."""
    import torch
    blob = load_blob(name)
    scn = qr.Scene(blob, rebin_tiles=True)
    frame = scn.new_frame(); ids = torch.full_like(frame, -2)
    scn.render(frame, ids=ids); torch.cuda.synchronize()
    out = frame.cpu().numpy().view(np.uint32)
    if name in BIG_CASES:
        assert _hash(out) == int(MANIFEST[name]["hash"], 16)
    else:
        assert (out == (load_frame(name) & 0xFFFFFF)).all()
    base = qr.Scene(blob)
    f0 = base.new_frame(); i0 = torch.full_like(f0, -2)
    base.render(f0, ids=i0); torch.cuda.synchronize()
    assert bool((f0 == frame).all()) and bool((i0 == ids).all())
    _, c0 = base.render_count(); _, c1 = scn.render_count()
    assert c0.as_dict() == c1.as_dict()


VARIANT_CASES = ["demo01_160", "demo02_160_gf_aa4", "demo03_160_aa2_t2500", "test13_160", "test16_160_noopt"]


@pytest.mark.parametrize("env", [{"QR_CULL": "0"}, {"QR_CULL": "2"}, {"QR_REBIN": "1"}, {"QR_REBIN": "1", "QR_BIN_TILE": "8x8"},
                                 {"QR_DIV": "1"}, {"QR_DIV": "1", "QR_CULL": "0"}])
@pytest.mark.parametrize("name", VARIANT_CASES)
def test_gpu_build_variants_match_reference(qr, name, env):
    """The knobs that change what the upload pass builds (cull cells off / on open shapes only, tile lists from
    the binning pass at two tile sizes) and the kernel instance with the per-lane walk (QR_DIV=1: the reference's
    scenes have no long hierarchies and get the instance without it by default) leave the reference's pixels,
    hit ids and ray counts untouched."""
    import os
    import torch
    blob = load_blob(name)
    base = qr.Scene(blob)
    f0 = base.new_frame(); i0 = torch.full_like(f0, -2)
    base.render(f0, ids=i0); _, c0 = base.render_count()
    os.environ.update(env)
    try:
        scn = qr.Scene(blob)
    finally:
        for k in env:
            del os.environ[k]
    frame = scn.new_frame(); ids = torch.full_like(frame, -2)
    scn.render(frame, ids=ids); torch.cuda.synchronize()
    assert (frame.cpu().numpy().view(np.uint32) == (load_frame(name) & 0xFFFFFF)).all()
    assert bool((i0 == ids).all())
    _, c1 = scn.render_count()
    assert c0.as_dict() == c1.as_dict()


def _hash(frame):
    """FNV-1a-64 over pixel & 0xFFFFFF, row-major (tests/golden/manifest.json 'hash'): the oracle's C helper."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import qr_oracle
    return qr_oracle.frame_hash(frame)


def test_gpu_multi_target_launch_matches_separate_launches(qr):
    """qr_render_multi_async: row blocks of the same scene and of two different scenes (different sizes,
    FSAA, options) rendered by ONE launch equal what separate launches give."""
    import torch
    a = qr.Scene(load_blob("demo01_160"))
    b = qr.Scene(load_blob("demo02_160_gf_aa4"))
    whole_a = a.render(); whole_b = b.render(); torch.cuda.synchronize()
    fa = [torch.full_like(whole_a, 0x55) for _ in range(3)]
    fb = torch.full_like(whole_b, 0x55)
    ha, hb = a.height, b.height
    cuts = [0, 40, 48, ha]
    targets = [(a, fa[i], cuts[i], cuts[i + 1]) for i in range(3)] + [(b, fb, 17, hb - 9)]
    qr.MultiRender(targets)()
    torch.cuda.synchronize()
    for i in range(3):
        assert bool((fa[i][cuts[i]:cuts[i + 1]] == whole_a[cuts[i]:cuts[i + 1]]).all())
        outside = torch.cat([fa[i][:cuts[i]], fa[i][cuts[i + 1]:]])
        assert bool((outside == 0x55).all()), "rows outside the range must stay untouched"
    assert bool((fb[17:hb - 9] == whole_b[17:hb - 9]).all())
    assert bool((fb[:17] == 0x55).all()) and bool((fb[hb - 9:] == 0x55).all())


def test_gpu_multi_target_launch_follows_depth_changes(qr):
    """Nothing of a scene's launch state is cached by the multi-target path: after qr_scene_set_depth the next
    multi-target launch renders with the new depth, exactly like a single-target launch."""
    import torch
    a = qr.Scene(load_blob("demo02_160_gf_d5"))
    h = a.height
    tg = [torch.zeros((h, a.width), dtype=torch.int32, device="cuda") for _ in range(2)]
    m = qr.MultiRender([(a, tg[0], 0, h // 2), (a, tg[1], h // 2, h)])
    for depth in (5, 0, 2):
        a.set_depth(depth)
        whole = a.render(); m(); torch.cuda.synchronize()
        assert bool((tg[0][:h // 2] == whole[:h // 2]).all()) and bool((tg[1][h // 2:] == whole[h // 2:]).all()), f"depth {depth}"
    d5 = a.render(); a.set_depth(0); d0 = a.render(); torch.cuda.synchronize()
    assert not bool((d5 == d0).all()), "the fixture must depend on the recursion depth"


def test_gpu_frame_hash_matches_manifest(qr):
    """qr_frame_hash (product helper used by bench.py's gate) has the manifest's definition."""
    import torch
    scn = qr.Scene(load_blob("c1_demo01_640x480"))
    f = scn.render(); torch.cuda.synchronize()
    assert qr.frame_hash(f) == int(MANIFEST["c1_demo01_640x480"]["hash"], 16) == _hash(f.cpu().numpy().view(np.uint32))


def _recamera(blob, seed):
    """The snapshot with its tile lists dropped (one whole-frame tile -> camera list) and the camera moved and
    turned at random (same rotation for the view, horizontal and vertical vectors): views the reference never
    rendered, including from inside objects and from below the floor."""
    import struct
    rng = np.random.default_rng(seed)
    b = bytearray(blob)
    off_frame = struct.unpack_from("<I", b, 4 * 10)[0]
    fr = np.frombuffer(b, dtype=np.float32, count=49, offset=off_frame).copy()
    fi = fr.view(np.int32)
    a = rng.normal(size=3); a /= np.linalg.norm(a)
    th = rng.uniform(0.0, 1.2)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K).astype(np.float32)
    for o in (1, 4, 7):
        fr[o:o + 3] = R @ fr[o:o + 3]
    fr[25:28] += rng.uniform(-4.0, 4.0, size=3).astype(np.float32)
    fi[29] = int(rng.integers(0, 11))                               # recursion depth 0..10
    fr[24] = np.float32(rng.choice([0.0, 0.5, 1.0, 2.0]))           # near clip t_min
    fi[34], fi[35], fi[36], fi[37] = fi[31], fi[32], 1, 1          # tile = frame
    b[off_frame:off_frame + 196] = fr.tobytes()
    struct.pack_into("<I", b, 4 * 8, 1)                             # n_tiles
    off_tiles = struct.unpack_from("<I", b, 4 * 15)[0]
    struct.pack_into("<i", b, off_tiles, int(fi[38]))               # tiles[0] = clist
    return bytes(b)


@pytest.mark.parametrize("name", ["demo01_160", "demo02_160_gf_aa4", "demo03_160", "test13_160_gf_aa4"])
def test_gpu_random_cameras_match_oracle(qr, oracle, name):
    """Parity away from the reference's own cameras: GPU (tile lists rebuilt by the binning pass) == oracle
    (camera list for every pixel) for random camera poses."""
    import torch
    base = load_blob(name)
    for seed in range(6):
        blob = _recamera(base, 1000 * seed + 7)
        o_frame, o_ids, _ = oracle.render(blob, threads=8, want_ids=True)
        scn = qr.Scene(blob, rebin_tiles=True)
        frame = scn.new_frame(); ids = torch.full_like(frame, -2)
        scn.render(frame, ids=ids); torch.cuda.synchronize()
        out = frame.cpu().numpy().view(np.uint32)
        assert int((out != o_frame).sum()) == 0, f"{name} seed {seed}"
        assert (ids.cpu().numpy() == o_ids).all(), f"{name} seed {seed}"


def _jitter_scene(blob, seed):
    """Random geometry: every real, untransformed surface is moved by up to 0.4 and quadrics are rescaled by up
    to 15 % (the engine's lists are kept, so this is not a scene the engine would build -- it is a stress of the
    solvers, clippers and culls on configurations no fixture has: the oracle and the GPU get the same blob)."""
    import struct
    rng = np.random.default_rng(seed)
    b = bytearray(blob)
    n_srf = struct.unpack_from("<I", b, 4 * 4)[0]
    off_srf = struct.unpack_from("<I", b, 4 * 11)[0]
    s = np.frombuffer(b, dtype=np.float32, count=n_srf * 64, offset=off_srf).reshape(n_srf, 64).copy()
    si = s.view(np.int32)
    for i in range(n_srf):
        tag, trm = si[i, 37], si[i, 15]
        if tag < 0 or tag >= 9 or trm != 0:
            continue
        s[i, 0:3] += rng.uniform(-0.4, 0.4, size=3).astype(np.float32)
        if si[i, 34] != 1:
            s[i, 27] *= np.float32(rng.uniform(0.85, 1.15))
    # every transformed array gets an extra random rotation and a little shear; its members carry a copy of
    # the array's matrix rows (tci/tcj/tck), so they receive the same new rows
    for t in range(n_srf):
        if si[t, 37] >= 0 or si[t, 15] < 2:
            continue
        a = rng.normal(size=3); a /= np.linalg.norm(a)
        th = rng.uniform(-0.5, 0.5)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K + rng.uniform(-0.05, 0.05, size=(3, 3))
        M = np.stack([s[t, 12:15], s[t, 16:19], s[t, 20:23]]).astype(np.float64)
        M2 = (M @ R).astype(np.float32)
        for i in range(n_srf):
            if si[i, 39] == t and si[i, 15] >= 2:
                s[i, 12:15], s[i, 16:19], s[i, 20:23] = M2[0], M2[1], M2[2]
    b[off_srf:off_srf + s.nbytes] = s.tobytes()
    return bytes(b)


@pytest.mark.parametrize("name", ["demo01_160", "demo02_160_gf_aa4", "test13_160_gf_aa4"])
def test_gpu_jittered_geometry_matches_oracle(qr, oracle, name):
    import torch
    base = load_blob(name)
    for seed in range(5):
        blob = _recamera(_jitter_scene(base, 77 + seed), 31 * seed + 3)
        o_frame, o_ids, _ = oracle.render(blob, threads=8, want_ids=True)
        scn = qr.Scene(blob, rebin_tiles=True)
        frame = scn.new_frame(); ids = torch.full_like(frame, -2)
        scn.render(frame, ids=ids); torch.cuda.synchronize()
        assert int((frame.cpu().numpy().view(np.uint32) != o_frame).sum()) == 0, f"{name} seed {seed}"
        assert (ids.cpu().numpy() == o_ids).all(), f"{name} seed {seed}"
