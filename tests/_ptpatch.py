"""Helper of tests/test_pt_oracle.py and tests/test_path_tracer.py: snapshot rewrites that turn an ordinary (ray-traced)
fixture into a path-tracer one.  Pure data rewriting, in the style of tests/_rayq.py: qr_frame.pt_on = 1 (frame word 41) and
qr_material.emis (floats 21..23 of the 32-word record) set on the materials of chosen surfaces.  The reference cannot light
these scenes (tests/golden/make_pt_golden.py: the demos stay black under its path tracer, their lights are not emitters), so
there is no frame of the reference for them; they carry what test18 lacks: clipper programs (CSG), trnode arrays, textures,
every quadric kind, and frames that are no multiple of any footprint."""
import gzip
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PROP_LIGHT = 0x10
EMISSION = (6.0, 4.5, 3.0)          # three different channels: a swapped plane shows

PATCHED_SCENES = ["demo01_160", "demo02_160_gf_aa4", "demo03_160", "test13_160_gf_aa4", "demo02_odd_33x17_aa4", "demo01_odd_157x93"]


def golden_blob(name):
    return gzip.decompress(open(os.path.join(GOLDEN, name + ".qrs.gz"), "rb").read())


def emitters(blob, every=3):
    """Indices of the materials that get the emission: both sides' materials of every real surface that shows as a light
    (QR_PROP_LIGHT on either side) and of every `every`-th real surface, so that planes, quadrics, clipped and array members
    all glow somewhere."""
    h = struct.unpack_from("<26I", blob, 0)
    s = np.frombuffer(blob, dtype=np.int32, count=h[4] * 64, offset=h[11]).reshape(h[4], 64)
    real = np.nonzero((s[:, 37] >= 0) & (s[:, 37] < 9))[0]         # srf_t[3]: tag of a real surface
    pick = [int(i) for n, i in enumerate(real) if n % every == 0 or ((s[i, 42] | s[i, 43]) & PROP_LIGHT)]
    mats = sorted({int(m) for i in pick for m in s[i, 40:42] if 0 <= m < h[5]})
    return mats


def pt_patch(blob, every=3, emission=EMISSION):
    """The snapshot as the walker would have captured it in path-tracer mode, with `emission` on emitters(blob, every)."""
    b = bytearray(blob)
    h = struct.unpack_from("<26I", b, 0)
    off_frame, off_mat = h[10], h[12]
    struct.pack_into("<i", b, off_frame + 4 * 41, 1)                # qr_frame.pt_on
    for m in emitters(blob, every):
        struct.pack_into("<3f", b, off_mat + 128 * m + 4 * 21, *emission)
    return bytes(b)


def patched(name):
    return pt_patch(golden_blob(name))
