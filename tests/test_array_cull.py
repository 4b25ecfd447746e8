"""Bounding-volume arrays in the packet walk's cull run (cull_run and walk_list, csrc/qr_walk.hpp): an array whose cull sphere every ray that
is on misses sideways is skipped inside the run, and a ray that misses it stays out of the volume test.  Frames must keep every
bit, so each snapshot below is rendered by the oracle on the CPU and by the kernel -- the packet instance, the per-lane instance
(QR_DIV=1), and both with the culls off (QR_CULL=0): equal pixels, first-hit ids and ray counts.  160 x 120 throughout.

The snapshots are the fixtures that carry arrays (the engine's own tile and light lists: demo scenes 1-3, the swarms, test13) and
patches of them that bring about what the stock cameras rarely do:

  own        the fixture as it is: primary walks over the engine's tile lists, arrays nested in arrays, arrays that end their list;
  turned     the camera moved and turned (test_gpu_parity._recamera, one tile with the global list): most arrays of the light
             lists and of the secondary rays' lists lie beside the footprints;
  inside     the camera at the centre of the largest array sphere of the image, one tile with the global list.  (No camera list of
             any fixture holds an array -- the counters below show that no primary walk meets one -- so where the camera stands
             reaches the arrays only through the shadow and secondary rays of what it sees; those start inside the spheres.)
  jitter     test_gpu_parity._jitter_scene: transformed arrays get a rotation and a shear (full matrices; volumes in a node's space);
  open       every plane's clip box opened: arrays with an unbounded member carry no sphere and must walk as before;
  own volumes  every bounding volume given a full-matrix transform of its own (QR_OPF_OWN | QR_OPF_FULLM cells).

The same snapshots once more through the guarded diagnostic build (make guard: the hand-written run with the cursor checked where
it is handed out, so a bad jump target shows), whose QR_STATS lines count, apart for shadow, primary and secondary walks (the
last two told by whether the rays start on a surface), on the jump side as well as where a cell is handed out: arrays jumped in
the run; of them jumped while rays wait at an enclosing array's end; of them jumped onto the list's END cell; arrays that leave
the run because every ray that is on starts inside the sphere; arrays split between rays that are ruled out and rays that go on;
arrays reached with rays already occluded.  The test asserts each for the snapshot made for it.  A ray that starts on a member
of an array has its origin inside the array's sphere, so "secondary and shadow rays that start on a member" show as all-inside
exits of shadow and secondary walks (depth 10, metal and glass members); the counter cannot tell such a ray from another that
starts inside the sphere.
The `_noopt` fixtures and all jittered `_jN` ones but test17_160_j18 compile to images without a bounding-volume cell, and
tests/_crowd.py's crowds are built for the per-lane walks, which this cut leaves alone; so the cases come from the fixtures whose
images hold arrays by the hundred.
"""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD_LIB = os.path.join(ROOT, "quadray-engine_amd", "libqrhip_guard.so")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _rayq                                                        # noqa: E402
from conftest import load_blob                                      # noqa: E402
from test_gpu_parity import _jitter_scene, _recamera                # noqa: E402

OPT_BV, OPF_CULL, OPF_CACHED, OPF_OWN, OPF_FULLM = 8, 32, 64, 128, 256   # csrc/qr_program.h


def _image(qr, blob, tmp):
    """the compiled device image as uint32 words (QR_DUMP_IMAGE)"""
    p = os.path.join(str(tmp), "img.bin")
    os.environ["QR_DUMP_IMAGE"] = p
    try:
        qr.program_stats(blob)
    finally:
        del os.environ["QR_DUMP_IMAGE"]
    img = np.fromfile(p, dtype=np.uint32)
    os.remove(p)
    return img


def _arrays(img):
    """bounding-volume cells of an image: [n, 8] words and their byte offsets.  A cell is taken for one when its words fit: type
    bits BV alone, the surface record and the end offset aligned and inside the image, the end behind the cell's two slots."""
    n = len(img) // 8
    c = img[:n * 8].reshape(n, 8)
    pos = np.arange(n, dtype=np.int64) * 32
    ok = ((c[:, 0] & 31) == OPT_BV) & (c[:, 0] < (1 << 20)) & (c[:, 2] % 32 == 0) & (c[:, 2] > pos + 32) & (c[:, 2] < len(img) * 4) \
        & (c[:, 1] % 16 == 0) & (c[:, 1] < len(img) * 4)
    return c[ok], pos[ok]


def _inside(qr, blob, tmp):
    """the camera moved to the centre of the largest array sphere, one tile with the global list"""
    c, _ = _arrays(_image(qr, blob, tmp))
    c = c[(c[:, 0] & OPF_CULL) != 0]
    f = c.view(np.float32)
    k = int(np.argmax(f[:, 7]))
    b = bytearray(blob)
    off = struct.unpack_from("<I", b, 40)[0]
    struct.pack_into("<3f", b, off + 4 * 25, *(float(x) for x in f[k, 4:7]))
    return _rayq.one_tile(bytes(b))


def _open_planes(blob):
    """every plane's clip box opened on both of its in-plane axes: an array that holds one has an unbounded member"""
    b = bytearray(blob)
    h = struct.unpack_from("<26I", b, 0)
    s = np.frombuffer(b, dtype=np.int32, count=h[4] * 64, offset=h[11]).reshape(h[4], 64).copy()
    f = s.view(np.float32)
    for i in np.nonzero(s[:, 37] == 0)[0]:
        s[i, 7] &= ~63
        f[i, 4:7] = -np.inf
        f[i, 8:11] = np.inf
    b[h[11]:h[11] + s.nbytes] = s.tobytes()
    return bytes(b)


def _own_volumes(blob, seed):
    """every untransformed bounding volume gets a transform of its own: a rotation with a little shear as its matrix rows,
    has_trm = 2 (full matrix), shift = 1 (the volume test reads the transformed diff and ray) and itself as its trnode -- outside
    a node's range such a volume compiles to QR_OPF_OWN | QR_OPF_FULLM.  The volume's quadric then stands rotated and sheared in
    the world; the oracle and the kernel read the same record."""
    rng = np.random.default_rng(seed)
    b = bytearray(blob)
    h = struct.unpack_from("<26I", b, 0)
    s = np.frombuffer(b, dtype=np.int32, count=h[4] * 64, offset=h[11]).reshape(h[4], 64).copy()
    f = s.view(np.float32)
    e = np.frombuffer(b, dtype=np.int32, count=h[7] * 4, offset=h[14]).reshape(h[7], 4)
    vols = sorted(set(int(i) for i in e[(e[:, 3] & 3) == 1, 0] if i >= 0 and s[i, 15] == 0 and s[i, 39] < 0))
    assert vols, "no untransformed bounding volume"
    for i in vols:
        a = rng.normal(size=3); a /= np.linalg.norm(a)
        th = rng.uniform(-0.6, 0.6)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        M = (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K + rng.uniform(-0.05, 0.05, size=(3, 3))).astype(np.float32)
        f[i, 12:15], f[i, 16:19], f[i, 20:23] = M[0], M[1], M[2]
        s[i, 15], s[i, 19], s[i, 39] = 2, 1, i
    b[h[11]:h[11] + s.nbytes] = s.tobytes()
    return bytes(b)


def _shallow(blob, depth):
    b = bytearray(blob)
    off = struct.unpack_from("<I", b, 40)[0]
    struct.pack_into("<i", b, off + 4 * 29, depth)
    return bytes(b)


# name -> (fixture, patch).  Depth is kept at the fixture's (10 for the demo scenes and swarms: secondary and shadow rays that start
# on members of arrays, reflecting and refracting ones among them) unless the patch draws its own.
CASES = {
    "demo01 own": ("demo01_160", None),
    "demo02 own": ("demo02_160_gf_d3", None),
    "demo03 own": ("demo03_160", None),
    "swarm mix own": ("swarm_demo01_240_mix", None),
    "swarm demo03 own": ("swarm_demo03_200_t3000", None),
    "swarm mix turned 1": ("swarm_demo01_240_mix", ("turned", 1007)),
    "swarm mix turned 2": ("swarm_demo01_240_mix", ("turned", 2007)),
    "demo02 turned": ("demo02_160_gf_d3", ("turned", 3007)),
    "swarm mix inside": ("swarm_demo01_240_mix", ("inside",)),
    "demo01 inside": ("demo01_160", ("inside",)),
    "test13 jitter": ("test13_160", ("jitter", 1)),
    "swarm demo03 jitter": ("swarm_demo03_200_t3000", ("jitter", 2)),
    "demo01 open": ("demo01_160", ("open",)),
    "demo01 own volumes": ("demo01_160", ("ownvol", 5)),
    "swarm mix own volumes": ("swarm_demo01_240_mix", ("ownvol", 6)),
}
_BLOBS = {}


def _blob(qr, case, tmp):
    if case not in _BLOBS:
        name, patch = CASES[case]
        blob = load_blob(name)
        if patch is not None:
            if patch[0] == "turned":
                blob = _recamera(blob, patch[1])
            elif patch[0] == "inside":
                blob = _inside(qr, blob, tmp)
            elif patch[0] == "jitter":
                blob = _jitter_scene(blob, patch[1])
            elif patch[0] == "open":
                blob = _open_planes(blob)
            elif patch[0] == "ownvol":
                blob = _own_volumes(blob, patch[1])
        _BLOBS[case] = blob
    return _BLOBS[case]


def _render(qr, blob, env):
    import torch
    os.environ.update(env)
    try:
        scn = qr.Scene(blob)
    finally:
        for k in env:
            del os.environ[k]
    frame = scn.new_frame(); ids = torch.full_like(frame, -2)
    scn.render(frame, ids=ids)
    _, c = scn.render_count()
    torch.cuda.synchronize()
    out = frame.cpu().numpy().view(np.uint32), ids.cpu().numpy(), c.as_dict()
    scn.close()
    return out


def _oracle(oracle, blob):
    f, ids, _ = oracle.render(blob, threads=8, want_ids=True)
    _, _, cnt = oracle.render(blob, threads=8, deferred=True)
    return f, ids, cnt


ENVS = ({}, {"QR_DIV": "1"}, {"QR_CULL": "0"}, {"QR_CULL": "0", "QR_DIV": "1"})


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_gpu_arrays_keep_every_bit(qr, oracle, tmp_path, case):
    blob = _blob(qr, case, tmp_path)
    ref, ref_ids, ref_cnt = _oracle(oracle, blob)
    for env in ENVS:
        out, ids, cnt = _render(qr, blob, env)
        assert int((out != ref).sum()) == 0, f"{case} {env}: {int((out != ref).sum())} pixels differ from the oracle"
        assert (ids == ref_ids).all(), f"{case} {env}: hit ids"
        assert cnt == {k: ref_cnt[k] for k in cnt}, f"{case} {env}: ray counts"


def test_patches_make_their_cases(qr, tmp_path):
    """what the patches are for, read off the compiled images (needs no GPU)"""
    for case in ("swarm mix inside", "demo01 inside"):
        blob = _blob(qr, case, tmp_path)
        c, _ = _arrays(_image(qr, blob, tmp_path))
        f = c[(c[:, 0] & OPF_CULL) != 0].view(np.float32)
        org = _rayq.frame_words(blob)[1][25:28]
        d = np.linalg.norm(f[:, 4:7].astype(np.float64) - org.astype(np.float64), axis=1)
        assert (d < f[:, 7]).any(), f"{case}: the camera lies in no array sphere"
    for case in ("demo01 own", "swarm mix own"):
        img = _image(qr, _blob(qr, case, tmp_path), tmp_path)
        c, pos = _arrays(img)
        assert (img[c[:, 2].astype(np.int64) // 4] == 0).any(), f"{case}: no array ends its list"
        starts = set(int(p) for p in pos)
        assert any(any(q in starts for q in range(int(p) + 64, int(e), 32)) for p, e in zip(pos, c[:, 2])), f"{case}: no nested array"
    c, _ = _arrays(_image(qr, _blob(qr, "demo01 open", tmp_path), tmp_path))
    assert ((c[:, 0] & OPF_CULL) == 0).any(), "open: every array still has a sphere"
    c, _ = _arrays(_image(qr, _blob(qr, "test13 jitter", tmp_path), tmp_path))
    assert ((c[:, 0] & OPF_CACHED) != 0).any(), "jitter: no volume in a node's space"
    want = OPF_CULL | OPF_OWN | OPF_FULLM
    for case in ("demo01 own volumes", "swarm mix own volumes"):
        c, _ = _arrays(_image(qr, _blob(qr, case, tmp_path), tmp_path))
        assert len(c) and ((c[:, 0] & want) == want).all(), f"{case}: arrays without QR_OPF_CULL | QR_OPF_OWN | QR_OPF_FULLM"


# ------------------------------------------------------------------------------------------------ the guarded build and its counters
# The library is chosen when the package is imported, hence the child process: this file run as a script.

_LINE = re.compile(r"QR_STATS arrays (shadow|primary|secondary): handed out (\d+) jumped in the run (\d+) jumped past waiting rays (\d+) "
                   r"jumped onto END (\d+) left all inside (\d+) split (\d+) rays ruled out (\d+) with occluded rays (\d+) "
                   r"with waiting rays (\d+)")
FIELDS = ("handed", "jumped", "jumped_waiting", "jumped_end", "inside", "split", "ruled_out", "occluded", "waiting")


def _guard_child(tmp):
    from qr_loader import load_package
    qr = load_package()
    assert qr.LIB_PATH == GUARD_LIB, qr.LIB_PATH
    import qr_oracle
    for case in sorted(CASES):
        blob = _blob(qr, case, tmp)
        ref, ref_ids, ref_cnt = _oracle(qr_oracle, blob)
        print(f"case {case}", file=sys.stderr, flush=True)
        out, ids, cnt = _render(qr, blob, {})
        ok = int((out != ref).sum()) == 0 and bool((ids == ref_ids).all()) and cnt == {k: ref_cnt[k] for k in cnt}
        print(f"{case} guard_ok {int(ok)}", flush=True)
    return 0


@pytest.mark.gpu
def test_gpu_guarded_build_and_counters(tmp_path):
    assert os.path.exists(GUARD_LIB), "libqrhip_guard.so is missing: build() makes it (make -C quadray-engine_amd/csrc guard)"
    env = dict(os.environ, QR_LIB=GUARD_LIB)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-child", str(tmp_path)], env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.count("guard_ok 1") == len(CASES) and "QR_GUARD" not in out.stderr, out.stdout + out.stderr[-3000:]
    # the counter lines of each case's render_count (the last pair after its "case" line)
    st, case = {}, None
    for line in out.stderr.splitlines():
        if line.startswith("case "):
            case = line[5:]
        m = _LINE.search(line)
        if m and case is not None:
            st.setdefault(case, {})[m.group(1)] = dict(zip(FIELDS, (int(v) for v in m.groups()[1:])))
    for k, v in sorted(st.items()):
        print(k, {kind: {f: x for f, x in c.items() if x} for kind, c in v.items()})
    assert sorted(st) == sorted(CASES), sorted(st)

    def n(case, field, *kinds):
        return sum(v[field] for k, v in st[case].items() if not kinds or k in kinds)

    for case in CASES:
        if case != "demo01 open":
            assert n(case, "jumped") > 0, f"{case}: no array was jumped inside the run"
    # every ray of a footprint misses an array sideways, in both kinds of walk, where the camera was turned away
    for case in ("swarm mix turned 1", "swarm mix turned 2"):
        assert n(case, "jumped", "shadow") > 0 and n(case, "jumped", "secondary") > 0, f"{case}: jumps in shadow and nearest-hit walks"
    # some rays miss and some enter: arrays split, in both kinds of walk
    for kind in ("shadow", "secondary"):
        assert n("swarm mix own", "split", kind) > 0 and n("swarm mix own", "ruled_out", kind) > 0, kind
    # no tile list of any fixture holds an array (the engine's camera lists are flat), so a primary walk never meets one: the camera
    # reaches the arrays through the rays its hits send out, which is what the inside snapshots move
    assert all(n(case, f, "primary") == 0 for case in CASES for f in ("handed", "jumped")), "a primary walk met an array: assert its cases too"
    # rays that start on a member of an array (depth 10, reflecting and refracting members): all-inside exits of shadow and secondary walks
    assert n("swarm mix own", "inside", "shadow") > 0 and n("swarm mix own", "inside", "secondary") > 0
    assert n("swarm mix inside", "inside") > 0 and n("demo01 inside", "inside") > 0
    # an array nested in an array, the inner one jumped while a ray waits at the outer's end
    for case in ("demo01 own", "swarm mix own"):
        assert n(case, "jumped_waiting") > 0, f"{case}: no array was jumped while rays waited at an enclosing array's end"
        assert n(case, "jumped_end") > 0, f"{case}: no jump landed on the END cell"
    # a shadow walk in which some rays are already occluded when the array is reached
    assert n("swarm mix own", "occluded", "shadow") > 0 and n("demo02 own", "occluded", "shadow") > 0
    # volumes with a transform of their own: handed out (their volume test runs) as well as jumped
    for case in ("demo01 own volumes", "swarm mix own volumes"):
        assert n(case, "handed") > 0 and n(case, "jumped") > 0 and n(case, "split") > 0, case
    # an array with an unbounded member is no array of the run: fewer arrays take part than in the fixture as it is
    assert n("demo01 open", "jumped") + n("demo01 open", "handed") < n("demo01 own", "jumped") + n("demo01 own", "handed")


if __name__ == "__main__":
    sys.exit(_guard_child(sys.argv[sys.argv.index("--guard-child") + 1]) if "--guard-child" in sys.argv else 2)
