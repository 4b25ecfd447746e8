"""Shadow lists without the cells that cast no shadow (csrc/qr_builder.cpp compile_list(head, as_shadow), QR_SHADOWLESS=0 keeps
them; profiles/r25_own_surface_roots.txt).

The count that was asked for before anything was cut found a ray's own surface in few of the packet walks' solves, and a cell that
casts no shadow -- the light's own body, which every shadow ray aims at -- in every shadow walk; so this is what was built, and the
root pre-test and the own-plane cells were not (the profile has the figures).

CPU: the image is smaller with the setting on, both images pass the compiler's verification (program_stats runs it), a chain that is
a shadow list and a side list keeps its full program, chains without such a cell have one program.
GPU: the frames of the fixtures equal the golden frames, ids and ray counts the oracle's, with the setting on and off, on the packet
and the per-lane instance, and in the guarded build; snapshots patched so that the dropped cell is the last member of every
bounding-volume array, or ends every trnode's range, or sits in a chain that is shadow list and side list at once, equal the oracle.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import _rayq
from conftest import ROOT, load_blob, load_frame

FIXTURES = ["demo01_160", "demo02_160_gf_d5", "demo03_160_gf_aa4", "demo01_odd_157x93",
            "test01_160", "test02_160", "test03_160", "test04_160", "test15_160", "test16_160"]
OFF = {"QR_SHADOWLESS": "0"}
P_OPAQUE, P_TRANSP, P_REFRACT, P_LIGHT = 0x200, 0x400, 0x2000, 0x10
S_SOLVER, S_TAG, S_PROPS, S_LST = 34, 37, 42, 44                # qr_surface words (include/qr_scene.h)


class env:
    def __init__(self, e):
        self.e = e

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.e}
        os.environ.update(self.e)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _stats(qr, blob, e):
    with env(e):
        return qr.program_stats(blob)


# ------------------------------------------------------------------------------------------------ snapshots

def _elems(blob):
    h = _rayq._hdr(blob)
    return np.frombuffer(blob, dtype=np.int32, count=h[7] * 4, offset=h[14]).reshape(h[7], 4).copy()      # simd, data, next, kind


def _chain(E, head):
    out = []
    while head >= 0:
        out.append(head)
        head = int(E[head, 2])
    return out


def _shadow_heads(blob):
    """heads of the shadow lists: `data` of the elements of every surface's two light lists"""
    s, _ = _rayq.surfaces(blob)
    E = _elems(blob)
    heads = set()
    for i in _rayq.real_surfaces(blob):
        for k in (0, 2):
            for e in _chain(E, int(s[i, S_LST + k])):
                if E[e, 1] >= 0:
                    heads.add(int(E[e, 1]))
    return sorted(heads)


def _is_solver(s, i):
    return 0 <= s[i, S_TAG] < 9 and 1 <= s[i, S_SOLVER] <= 3


def _shadowless(blob, which):
    """both sides of the surfaces `which` made plainly transparent: they cast no shadow (CHECK_SHAD)"""
    b = bytearray(blob)
    h = _rayq._hdr(b)
    s, _ = _rayq.surfaces(blob)
    for i in which:
        for k in (0, 1):
            s[i, S_PROPS + k] = (int(s[i, S_PROPS + k]) | P_TRANSP) & ~(P_REFRACT | P_OPAQUE)
    b[h[11]:h[11] + s.nbytes] = s.tobytes()
    return bytes(b)


def _range_ends(blob, arrays):
    """surfaces of the shadow lists' elements that end a bounding-volume array (arrays) or a trnode's range (not arrays)"""
    s, _ = _rayq.surfaces(blob)
    E = _elems(blob)
    out = set()
    for head in _shadow_heads(blob):
        for e in _chain(E, head):
            si, last = int(E[e, 0]), int(E[e, 1])
            if last < 0 or si < 0:
                continue
            is_bv = (int(E[e, 3]) & 3) == 1
            is_trnode = s[si, S_TAG] < 0 and not is_bv
            if (is_bv if arrays else is_trnode) and E[last, 0] >= 0 and _is_solver(s, int(E[last, 0])):
                out.add(int(E[last, 0]))
    return sorted(out)


def _small(blob):
    from test_shade_solve_cuts import _resized
    return _resized(blob, 64, 48)


def _patched(kind):
    if kind == "array_end":                     # the dropped cell is the last member of every bounding-volume array
        blob = _small(load_blob("swarm_demo01_240_mix"))
        which = _range_ends(blob, arrays=True)
    elif kind == "trnode_end":                  # ... ends every trnode's range
        blob = _small(load_blob("demo01_160"))
        which = _range_ends(blob, arrays=False)
    else:                                       # shadow chains with the elements of tile and side chains (one program for all of
        blob = load_blob("test02_160")          # them until now): the light's body is the cell that goes, as the snapshot has it
        return blob, []                         # (with its own tiles: the tile chains are the ones they shared with)
    assert len(which) > 0, kind
    return _shadowless(blob, which), which


KINDS = ["array_end", "trnode_end", "shared_chain"]


# ------------------------------------------------------------------------------------------------ CPU

def test_image_is_smaller_and_verified(qr):
    for name in FIXTURES:                       # (a chain that shared its program with a tile or side chain gets one of its own:
        on, off = _stats(qr, load_blob(name), {}), _stats(qr, load_blob(name), OFF)     # the sum of all cells may grow by that)
        assert on.n_dropped > off.n_dropped and on.n_lists >= off.n_lists, name
    blob = load_blob("demo01_160")
    on, off = _stats(qr, blob, {}), _stats(qr, blob, OFF)
    assert on.n_cells < off.n_cells and on.bytes < off.bytes
    assert on.n_dropped > off.n_dropped


def test_scene_without_shadowless_surface_keeps_its_image(qr):
    """no surface casts none: one program per chain, the image byte for byte what it was"""
    blob = load_blob("demo01_160")
    b = bytearray(blob)
    h = _rayq._hdr(b)
    s, _ = _rayq.surfaces(blob)
    s[:, S_PROPS:S_PROPS + 2] &= ~(P_LIGHT | P_TRANSP)
    b[h[11]:h[11] + s.nbytes] = s.tobytes()
    on, off = _stats(qr, bytes(b), {}), _stats(qr, bytes(b), OFF)
    assert (on.bytes, on.n_lists, on.n_cells, on.n_dropped) == (off.bytes, off.n_lists, off.n_cells, off.n_dropped)


@pytest.mark.parametrize("kind", KINDS)
def test_patched_snapshots_drop_cells(qr, kind):
    blob, which = _patched(kind)
    on, off = _stats(qr, blob, {}), _stats(qr, blob, OFF)
    assert on.n_dropped > off.n_dropped, kind
    if kind == "shared_chain":
        assert on.n_lists > off.n_lists         # the chains' full program stays beside their shadow programs
    else:
        assert on.n_cells < off.n_cells and on.n_lists == off.n_lists


# ------------------------------------------------------------------------------------------------ GPU

def _render(qr, blob, e):
    import torch
    with env(e):
        scn = qr.Scene(blob)
    frame = scn.new_frame(); ids = torch.full_like(frame, -2)
    scn.render(frame, ids=ids)
    _, c = scn.render_count()
    torch.cuda.synchronize()
    out = frame.cpu().numpy().view(np.uint32), ids.cpu().numpy(), c.as_dict()
    scn.close()
    return out


def _against_oracle(qr, oracle, blob, what, golden=None):
    ref, ref_ids, _ = oracle.render(blob, threads=8, want_ids=True)
    _, _, ref_cnt = oracle.render(blob, threads=8, deferred=True)
    if golden is not None:
        assert (ref == golden).all(), f"{what}: the oracle's frame is not the golden frame"
    frames = []
    for e in ({}, OFF, {"QR_DIV": "1"}, dict(OFF, QR_DIV="1")):
        out, ids, cnt = _render(qr, blob, e)
        assert int((out != ref).sum()) == 0, f"{what} {e}: {int((out != ref).sum())} pixels differ"
        assert (ids == ref_ids).all(), f"{what} {e}: hit ids"
        assert cnt == {k: ref_cnt[k] for k in cnt}, f"{what} {e}: ray counts {cnt}"
        frames.append(out)
    assert all((f == frames[0]).all() for f in frames)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_gpu_fixture_frames(qr, oracle, name):
    _against_oracle(qr, oracle, load_blob(name), name, golden=load_frame(name).view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_patched_snapshots(qr, oracle, kind):
    blob, _ = _patched(kind)
    _against_oracle(qr, oracle, blob, kind)


@pytest.mark.gpu
def test_gpu_guarded_build_renders_the_golden_frames(qr):
    lib = os.path.join(ROOT, "quadray-engine_amd", "libqrhip_guard.so")
    assert os.path.exists(lib), "libqrhip_guard.so not built (make -C quadray-engine_amd/csrc guard)"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_guard_frames.py")] + FIXTURES, capture_output=True, text=True,
                         timeout=300, env=dict(os.environ, QR_LIB=lib))
    assert out.returncode == 0, out.stderr[-2000:]
    got = dict(l.split() for l in out.stdout.splitlines() if len(l.split()) == 2 and l.split()[0] in FIXTURES)
    want = {n: "%016x" % qr.frame_hash(load_frame(n).view(np.uint32)) for n in FIXTURES}
    assert got == want
    assert "bad cell offsets" not in out.stderr, out.stderr[-2000:]
