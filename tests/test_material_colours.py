"""Colours at upload (csrc/qr_program.h QR_MATX_*, qr_compile.hpp material_colour): the image's copy of a material record whose
texture is ONE texel carries the finished colour, so that shade() skips the texel load, the three conversions and the three
IEEE divisions by `clamp`.  The kernel takes the stored words as they are: they must be the bits its own arithmetic gives,

    numpy.float32(numpy.int32((texel >> s) & cmask)) / numpy.float32(clamp)        s = 16, 8, 0

and the flag must be set exactly when both index masks are 0.  A textured material whose channels have at most 8 bits
(cmask <= 0xFF) points at a 256-entry table, one per distinct (cmask, clamp) of the image, entry i the same expression for
the channel byte i; with a wider mask the kernel keeps its arithmetic and the record's image-only words are 0.
"""
import glob
import gzip
import hashlib
import os
import struct

import numpy as np
import pytest

from conftest import GOLDEN

SNAPSHOTS = sorted(os.path.basename(p)[:-len(".qrs.gz")] for p in glob.glob(os.path.join(GOLDEN, "*.qrs.gz")))
MATF_COLOUR, MATF_LUT = 1, 2
# DevHeader (csrc/qr_program.h): the 49 words of qr_frame, then off_shade, off_tiles, off_order, n_blocks, img_flags, img_bytes,
# off_query, reach, off_mat, n_mat
HDR_OFF_MAT, HDR_N_MAT = 57, 58
# qr_material (include/qr_scene.h), 32 words
M_XMASK, M_YMASK, M_TEX, M_CLAMP, M_CMASK, M_PAD = 4, 5, 7, 19, 20, 24


def _blob(name):
    return gzip.decompress(open(os.path.join(GOLDEN, name + ".qrs.gz"), "rb").read())


def _image(qr, blob, tmp_path, threads=None):
    p = os.path.join(str(tmp_path), "image.bin")
    old = {k: os.environ.get(k) for k in ("QR_DUMP_IMAGE", "QR_HOST_THREADS")}
    os.environ["QR_DUMP_IMAGE"] = p
    if threads is not None:
        os.environ["QR_HOST_THREADS"] = str(threads)
    try:
        qr.program_stats(blob)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    raw = open(p, "rb").read()
    os.remove(p)
    return raw


def _expected(texel, cmask, clamp):
    """the three channels with the kernel's operations, as uint32 bit patterns"""
    with np.errstate(all="ignore"):
        return [int((np.float32(np.int32((int(texel) >> s) & int(cmask))) / np.float32(clamp)).view(np.uint32)) for s in (16, 8, 0)]


def _check_image(blob, raw):
    """every material record of the image, the zero record behind the last one included; returns (one-texel, textured) counts"""
    img = np.frombuffer(raw, dtype=np.uint32)
    h = struct.unpack_from("<26I", blob, 0)
    n_mat, off_mat_s, off_tex_s = h[5], h[12], h[16]
    off_mat = int(img[HDR_OFF_MAT])
    assert int(img[HDR_N_MAT]) == n_mat and off_mat % 128 == 0 and off_mat + (n_mat + 1) * 128 <= len(raw)
    snap = np.frombuffer(blob, dtype=np.uint32, count=n_mat * 32, offset=off_mat_s).reshape(n_mat, 32)
    texels = np.frombuffer(blob, dtype=np.uint32, count=h[9], offset=off_tex_s)
    plain = textured = 0
    tables = {}
    for i in range(n_mat + 1):
        m = img[off_mat // 4 + 32 * i: off_mat // 4 + 32 * (i + 1)]
        one = int(m[M_XMASK]) == 0 and int(m[M_YMASK]) == 0
        assert bool(int(m[M_PAD]) & MATF_COLOUR) == one, f"material {i}: flag {int(m[M_PAD])}, one texel {one}"
        assert not m[M_PAD + 5:].any()
        if not one:
            textured += 1
            assert not m[M_PAD + 1:M_PAD + 4].any(), f"material {i}: colour words of a textured material"
            lut = int(m[M_PAD + 4])
            if int(m[M_CMASK]) > 0xFF:
                assert int(m[M_PAD]) == 0 and lut == 0, f"material {i}: a table for a mask of more than 8 bits"
                continue
            assert int(m[M_PAD]) == MATF_LUT and lut % 64 == 0 and 0 < lut and lut + 1024 <= len(raw), f"material {i}: table offset"
            clamp = m[M_CLAMP:M_CLAMP + 1].view(np.float32)[0]
            tables.setdefault(lut, (int(m[M_CMASK]), int(m[M_CLAMP])))
            assert tables[lut] == (int(m[M_CMASK]), int(m[M_CLAMP])), "one table, two (cmask, clamp) pairs"
            want = [_expected(k, m[M_CMASK], clamp)[2] for k in range(256)]
            assert [int(x) for x in img[lut // 4:lut // 4 + 256]] == want, f"material {i}: table"
            continue
        assert int(m[M_PAD]) == MATF_COLOUR and int(m[M_PAD + 4]) == 0, f"material {i}: flag {int(m[M_PAD])} of a one-texel material"
        plain += 1
        texel = int(img[int(m[M_TEX]) // 4])
        clamp = m[M_CLAMP:M_CLAMP + 1].view(np.float32)[0]
        assert [int(x) for x in m[M_PAD + 1:M_PAD + 4]] == _expected(texel, m[M_CMASK], clamp), f"material {i}"
        if i < n_mat:
            # ... which are the snapshot's own texel, mask and clamp: the documented fields travel unchanged
            s = snap[i]
            assert int(s[M_CMASK]) == int(m[M_CMASK]) and int(s[M_CLAMP]) == int(m[M_CLAMP]) and int(texels[int(s[M_TEX])]) == texel
            assert not s[M_PAD:].any(), "the snapshot's pad words stay 0: the colour is no part of its format"
    assert len(set(tables.values())) == len(tables), "two tables for one (cmask, clamp) pair"
    return plain, textured


@pytest.mark.parametrize("name", SNAPSHOTS)
def test_image_materials_carry_their_colour(qr, tmp_path, name):
    blob = _blob(name)
    plain, textured = _check_image(blob, _image(qr, blob, tmp_path))
    assert plain >= 1           # the zero record at least


def test_fixtures_hold_both_kinds_of_material(qr, tmp_path):
    """the sweep above is not vacuous: plain colours and real textures both occur"""
    blob = _blob("demo01_160")
    plain, textured = _check_image(blob, _image(qr, blob, tmp_path))
    assert plain >= 2 and textured >= 1


def patch_materials(blob, cmask=None, clamp=None, one_texel=False, colours=None):
    """The snapshot with every material's `cmask` / `clamp` replaced, and -- one_texel -- every texture cut down to one texel
    of its own: material i reads texel i (modulo the pool) which holds colours[i] (default: a distinct value per material)."""
    b = bytearray(blob)
    h = struct.unpack_from("<26I", b, 0)
    n_mat, n_tex, off_mat, off_tex = h[5], h[9], h[12], h[16]
    for i in range(n_mat):
        o = off_mat + 128 * i
        if cmask is not None:
            struct.pack_into("<I", b, o + 4 * M_CMASK, cmask)
        if clamp is not None:
            struct.pack_into("<f", b, o + 4 * M_CLAMP, clamp)
        if one_texel:
            struct.pack_into("<3I", b, o + 4 * M_XMASK, 0, 0, 0)               # xmask, ymask, yshft
            struct.pack_into("<i", b, o + 4 * M_TEX, i % n_tex)
    if one_texel:
        for i in range(min(n_mat, n_tex)):
            c = colours[i % len(colours)] if colours is not None else (0x3F5A91 * (i + 1) + 0x1B0D07 * (i * i)) & 0xFFFFFFFF
            struct.pack_into("<I", b, off_tex + 4 * i, c)
    return bytes(b)


@pytest.mark.parametrize("cmask,clamp", [(0xFF, 255.0), (0x7F, 127.0), (0x3FF, 1023.0), (0xFF, 3.0)])
@pytest.mark.parametrize("colours", [None, [0x000000], [0xFFFFFF], [0xFFFFFFFF, 0x00800001, 0x7F00FF]])
def test_patched_materials(qr, tmp_path, cmask, clamp, colours):
    """masks of 7, 8 and 10 bits (a 10-bit mask reads across the channel boundaries of the texel), a clamp that is no power of
    two minus one, black, white and texels with the unused top byte set -- all one-texel, all finished at upload"""
    blob = patch_materials(_blob("demo01_160"), cmask, clamp, one_texel=True, colours=colours)
    plain, textured = _check_image(blob, _image(qr, blob, tmp_path))
    assert textured == 0 and plain == struct.unpack_from("<26I", blob, 0)[5] + 1


def test_patched_masks_on_textured_materials(qr, tmp_path):
    """cmask / clamp replaced on a scene that keeps its textures: the flags follow the texture sizes, a table exists for the
    7-bit mask and none for the 10-bit one (the arithmetic path); two pairs in one image get a table each"""
    base = _blob("demo01_160")
    want = _check_image(base, _image(qr, base, tmp_path))
    for cmask, clamp in ((0x7F, 127.0), (0x3FF, 1023.0), (0xFF, 3.0)):
        blob = patch_materials(base, cmask, clamp)
        assert _check_image(blob, _image(qr, blob, tmp_path)) == want
    b = bytearray(base)
    h = struct.unpack_from("<26I", b, 0)
    for i in range(0, h[5], 2):
        struct.pack_into("<fI", b, h[12] + 128 * i + 4 * M_CLAMP, 127.0, 0x7F)
    assert _check_image(bytes(b), _image(qr, bytes(b), tmp_path)) == want


@pytest.mark.parametrize("name", ["demo01_160", "demo02_160_gf_aa4", "test16_160", "swarm_demo01_240_mix", "c2b_demo01_1080p"])
def test_image_does_not_depend_on_host_threads(qr, tmp_path, name):
    blob = _blob(name)
    digests = {thr: hashlib.sha1(_image(qr, blob, tmp_path, threads=thr)).hexdigest() for thr in (1, 3, 8)}
    assert digests[1] == digests[3] == digests[8]
