"""The hot-path cuts of shade() and solve_cell() (csrc/qr_shade.hpp and csrc/qr_walk.hpp, profiles/r05_shade_solve_cuts.txt)
against the oracle, on snapshots patched so that every cut's branches run -- the stock fixtures take few of them:

  texel colour   every material a one-texel colour of its own (the colour comes finished from the image), masks of 7 / 8 / 10
                 bits, gamma on and off (the squaring stays in the kernel);
  texel table    the textures kept, with those masks: table loads, and the arithmetic for the 10-bit mask;
  shared rsq     specular powers with and without fraction bits, diffuse off with specular on (the shared rsq then comes from
                 the specular block alone), metal and plain blends;
  shared ray     surfaces that refract AND reflect with Fresnel on, and total inner reflection;
  xform2         scaled, rotated and sheared arrays: full matrices, own and cached transforms;
  quadric roots  quadrics with a raised d_eps: silhouette lanes with 0 <= d < d_eps beside lanes without.

Each patched snapshot is rendered by the oracle on the CPU and by the kernel -- the packet instance, the per-lane instance
(QR_DIV=1) and qr_shade_rays on the camera's rays: pixels, first-hit ids and ray counts must be equal.  160 x 120 throughout.
"""
import os
import struct

import numpy as np
import pytest

import _rayq
from conftest import load_blob
from test_material_colours import patch_materials
from test_gpu_parity import _jitter_scene
from test_shade_rays import _check_camera_frame, rays_mod          # noqa: F401  (rays_mod: a fixture)

pytestmark = pytest.mark.gpu

P_METAL, P_GAMMA, P_FRESNEL, P_OPAQUE, P_TRANSP, P_REFLECT, P_REFRACT, P_DIFFUSE, P_SPECULAR = \
    0x20, 0x40, 0x80, 0x200, 0x400, 0x1000, 0x2000, 0x4000, 0x8000
S_DEPS, S_SOLVER, S_TAG, S_MAT, S_PROPS = 32, 34, 37, 40, 42        # qr_surface words (include/qr_scene.h)
M_LPOW, M_CRFL, M_CTRN, M_CRFR, M_RFR2 = 12, 13, 14, 15, 16         # qr_material words
F_FLAGS = 28                                                       # qr_frame.ctx_flags

_ORACLE = {}


def _oracle(oracle, blob):
    """(frame, ids, ray counts in the backend's shading mode) of a patched snapshot: computed once per blob"""
    k = hash(blob)
    if k not in _ORACLE:
        f, ids, _ = oracle.render(blob, threads=8, want_ids=True)
        _, _, cnt = oracle.render(blob, threads=8, deferred=True)
        _ORACLE.clear()                                             # one blob at a time is all the callers need
        _ORACLE[k] = (f, ids, cnt)
    return _ORACLE[k]


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


def _check(qr, oracle, rays_mod, blob, what):
    ref, ref_ids, ref_cnt = _oracle(oracle, blob)
    for env in ({}, {"QR_DIV": "1"}):
        out, ids, cnt = _render(qr, blob, env)
        assert int((out != ref).sum()) == 0, f"{what} {env}: {int((out != ref).sum())} pixels differ from the oracle"
        assert (ids == ref_ids).all(), f"{what} {env}: hit ids"
        assert cnt == {k: ref_cnt[k] for k in cnt}, f"{what} {env}: ray counts"
    _check_camera_frame(qr, oracle, rays_mod, blob)


def _surfaces(b):
    h = struct.unpack_from("<26I", b, 0)
    s = np.frombuffer(b, dtype=np.int32, count=h[4] * 64, offset=h[11]).reshape(h[4], 64).copy()
    return h, s


def _put_surfaces(b, h, s):
    b[h[11]:h[11] + s.nbytes] = s.tobytes()


def _real(s):
    return np.nonzero((s[:, S_TAG] >= 0) & (s[:, S_TAG] < 9))[0]


def _props(blob, set_bits=0, clear_bits=0, only=None):
    """props of both sides of every real surface (`only`: of those whose side passes the predicate)"""
    b = bytearray(blob)
    h, s = _surfaces(b)
    for i in _real(s):
        for k in (0, 1):
            p = int(s[i, S_PROPS + k])
            if only is None or only(p):
                s[i, S_PROPS + k] = (p | set_bits) & ~clear_bits
    _put_surfaces(b, h, s)
    return bytes(b)


def _materials(blob, **words):
    """float / int words of every material record: name=(word index, format, value)"""
    b = bytearray(blob)
    h = struct.unpack_from("<26I", b, 0)
    for i in range(h[5]):
        for at, fmt, val in words.values():
            struct.pack_into(fmt, b, h[12] + 128 * i + 4 * at, val)
    return bytes(b)


def _frame_gamma(blob, on):
    b = bytearray(blob)
    off = struct.unpack_from("<I", b, 40)[0] + 4 * F_FLAGS
    fl = struct.unpack_from("<i", b, off)[0]
    struct.pack_into("<i", b, off, (fl | P_GAMMA) if on else (fl & ~P_GAMMA))
    return bytes(b)


def _resized(blob, w=160, h=120):
    """the snapshot at w x h with one tile that holds the global list (its tile lists belong to the old size)"""
    b = bytearray(blob)
    off = struct.unpack_from("<I", b, 40)[0]
    fi = np.frombuffer(b, dtype=np.int32, count=49, offset=off).copy()
    fi[31], fi[32], fi[33] = w, h, w
    b[off:off + 196] = fi.tobytes()
    return _rayq.one_tile(bytes(b))


# ------------------------------------------------------------------------------------------------ colours at upload

@pytest.mark.parametrize("gamma", [False, True])
@pytest.mark.parametrize("cmask,clamp", [(0xFF, 255.0), (0x7F, 127.0), (0x3FF, 1023.0)])
def test_one_texel_colours(qr, oracle, rays_mod, cmask, clamp, gamma):
    blob = patch_materials(load_blob("demo01_160"), cmask, clamp, one_texel=True)
    blob = _props(blob, set_bits=P_GAMMA) if gamma else _props(blob, clear_bits=P_GAMMA)
    blob = _frame_gamma(blob, gamma)
    _check(qr, oracle, rays_mod, blob, f"one texel, cmask {cmask:#x}, gamma {gamma}")


@pytest.mark.parametrize("name", ["demo01_160", "demo03_160_gf_aa4"])
@pytest.mark.parametrize("cmask,clamp", [(0xFF, 255.0), (0x7F, 127.0), (0x3FF, 1023.0), (0xFF, 3.0)])
def test_textured_colour_tables(qr, oracle, rays_mod, name, cmask, clamp):
    """the textures kept: channels through the image's 256-entry tables (masks of at most 8 bits) or the arithmetic (10 bits)"""
    _check(qr, oracle, rays_mod, patch_materials(load_blob(name), cmask, clamp), f"{name} textured, cmask {cmask:#x} clamp {clamp}")


def test_one_texel_black_and_white(qr, oracle, rays_mod):
    blob = patch_materials(load_blob("demo01_160"), one_texel=True, colours=[0x000000, 0xFFFFFF, 0xFFFFFFFF])
    _check(qr, oracle, rays_mod, blob, "black and white")


# ------------------------------------------------------------------------------------------------ one rsq per light

@pytest.mark.parametrize("l_pow", [0x00, 0x08, 0x1F, 0x123])
@pytest.mark.parametrize("name", ["demo01_160", "test07_160_gf"])
def test_light_terms(qr, oracle, rays_mod, name, l_pow):
    base = _materials(load_blob(name), l_pow=(M_LPOW, "<I", l_pow))
    for diffuse in (True, False):
        for metal in (True, False):
            blob = _props(base, set_bits=P_SPECULAR | (P_DIFFUSE if diffuse else 0) | (P_METAL if metal else 0),
                          clear_bits=(0 if diffuse else P_DIFFUSE) | (0 if metal else P_METAL))
            _check(qr, oracle, rays_mod, blob, f"{name} l_pow {l_pow:#x} diffuse {diffuse} metal {metal}")


# ------------------------------------------------------------------------------------------------ one normalised ray

@pytest.mark.parametrize("rfr_2", [None, 1.5, 4.0])
@pytest.mark.parametrize("name", ["demo02_160_gf_d3", "demo03_160_gf_aa4"])
def test_refract_and_reflect(qr, oracle, rays_mod, name, rfr_2):
    """every side that is not opaque refracts, reflects and splits by Fresnel; opaque sides reflect with Fresnel too (metal
    and plain as they come); a raised rfr_2 turns shallow hits into total inner reflection"""
    blob = load_blob(name)
    blob = _props(blob, set_bits=P_REFRACT | P_REFLECT | P_FRESNEL, only=lambda p: not (p & P_OPAQUE))
    blob = _props(blob, set_bits=P_REFLECT | P_FRESNEL, only=lambda p: bool(p & P_OPAQUE))
    words = dict(c_rfl=(M_CRFL, "<f", 0.25), c_trn=(M_CTRN, "<f", 0.5))
    if rfr_2 is not None:
        words["rfr_2"] = (M_RFR2, "<f", rfr_2)
    blob = _materials(blob, **words)
    _check(qr, oracle, rays_mod, blob, f"{name} rfr_2 {rfr_2}")


# ------------------------------------------------------------------------------------------------ transforms and roots

def _grazing(blob, factor):
    """d_eps of every quadric raised: 0 <= d < d_eps along the silhouettes"""
    b = bytearray(blob)
    h, s = _surfaces(b)
    f = s.view(np.float32)
    for i in _real(s):
        if s[i, S_SOLVER] != 1:
            f[i, S_DEPS] *= np.float32(factor)
    _put_surfaces(b, h, s)
    return bytes(b)


@pytest.mark.parametrize("patch", ["plain", "jitter1", "jitter2", "graze", "jitter+graze"])
@pytest.mark.parametrize("name", ["test15_160", "test16_160", "swarm_demo01_240_mix"])
def test_transforms_and_roots(qr, oracle, rays_mod, name, patch):
    blob = _resized(load_blob(name))
    if "jitter" in patch:
        blob = _jitter_scene(blob, 2 if patch == "jitter2" else 1)
    if "graze" in patch:
        blob = _grazing(blob, 3.0e4)
    _check(qr, oracle, rays_mod, blob, f"{name} {patch}")
