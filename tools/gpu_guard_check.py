#!/usr/bin/env python3
"""The QR_STATS + QR_GUARD build (every cell offset of the per-lane walks checked before it is loaded, csrc/qr_walk.hpp
QR_GUARD_POS) on scenes that drive walk_div / walk_pool / walk_dda hard: synthetic crowds with built lists, the 10 000-object
scene at a small size, a swarm fixture, a dense crowd of engine-authored surfaces (tests/_crowd.py).  Prints one line per case: "<case> guard_bad 0 frame_ok 1"; exit code 1 on any bad
offset or frame.  Build: make -C quadray-engine_amd/csrc guard.  (GPU box; run by tests/test_synth.py in a child process.)"""
import gzip, importlib.util, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "quadray-engine_amd", "libqrhip_guard.so")
if os.environ.get("QR_LIB") != LIB:
    # the library is chosen at import time: run ourselves again with it selected, collect stderr (QR_GUARD lines)
    env = dict(os.environ, QR_LIB=LIB)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True)
    bad = [l for l in p.stderr.splitlines() if l.startswith("QR_GUARD")]
    sys.stdout.write(p.stdout)
    for l in bad:
        print(l)
    if p.returncode != 0:
        print("child failed:\n" + p.stderr[-3000:])
    sys.exit(1 if (p.returncode != 0 or bad) else 0)

sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np
import torch
from qr_loader import load_package
import qr_oracle
qr = load_package()
spec = importlib.util.spec_from_file_location("qr_synth", os.path.join(ROOT, "quadray-engine_amd", "synth.py"))
synth = importlib.util.module_from_spec(spec); spec.loader.exec_module(synth)

cases = {
    "synth2000_built": qr.build_lists(synth.make_scene(shadow_lists=False, n_objects=2000, width=384, height=216, depth=4, box=45.0, gamma=True, fsaa=2)),
    "synth10k_built_640": qr.build_lists(synth.make_scene(shadow_lists=False, n_objects=10000, width=640, height=360, depth=4)),
    "synth300_own_lists": synth.make_scene(n_objects=300, width=320, height=240, depth=4, box=20.0),
    "swarm_demo01_240_mix": gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "swarm_demo01_240_mix.qrs.gz"), "rb").read()),
}
# a dense cloud with lowered grid thresholds (every list of 64 members gets its uniform grid, the plane its shadow grids): an image of
# ~300 MB, i.e. valid cell offsets beyond the 256 MB bound the guard had until round 3
cases["dense490_low_thresholds"] = qr.build_lists(synth.make_scene(shadow_lists=False, n_objects=490, width=320, height=180, depth=6, box=5.96, seed=20076))
# engine-authored surfaces of every kind, axis map and min/max pattern the fixtures hold (tests/_crowd.py), dense, built lists
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _crowd
cases["crowd400_dense_low_thresholds"] = qr.build_lists(_crowd.make_crowd(**_crowd.DENSE))
rc = 0
for name, blob in cases.items():
    low = name.endswith("low_thresholds")
    if low:
        os.environ.update({"QR_DDA": "64", "QR_GRID": "64"})
    try:
        scn = qr.Scene(blob, rebin_tiles=name.startswith(("synth", "crowd")))
    finally:
        if low:
            del os.environ["QR_DDA"], os.environ["QR_GRID"]
    if low:
        print(f"{name} image bytes {scn.info.device_bytes}", flush=True)
    frame, counts = scn.render_count()          # the counting launch prints "QR_GUARD n bad cell offsets" on stderr when n != 0
    torch.cuda.synchronize()
    out = frame.cpu().numpy().view(np.uint32)
    ref, _, _ = qr_oracle.render(blob, threads=16)
    ok = bool((out == ref).all())
    print(f"{name} frame_ok {int(ok)} rays {counts.as_dict()}", flush=True)
    if not ok:
        rc = 1
    scn.close()

# view rendering (qr_render_views_kernel) under the same guard: the snapshot's own camera at a quarter of its size in each
# dimension, on the scenes whose ray-query list is a long hierarchy with a grid (per-lane instance) and on a fixture (packet
# instance), against the oracle's frame of the snapshot rewritten to that frame with one tile holding the global list.  A guarded
# walk skips the cell it refuses, so a bad offset shows as a differing frame.  ("view_ok": the cases above are counted by name.)
spec = importlib.util.spec_from_file_location("qr_rays", os.path.join(ROOT, "quadray-engine_amd", "rays.py"))
rays = importlib.util.module_from_spec(spec); spec.loader.exec_module(rays)
for name in ("synth2000_built", "synth10k_built_640", "swarm_demo01_240_mix"):
    blob = cases[name]
    f, i = rays.frame_record(blob)
    w, h = int(i[31]) // 4, int(i[32]) // 4
    view = rays.view_of(blob)
    view[8:11] *= np.float32(4.0); view[12:15] *= np.float32(4.0)         # the same field of view
    b = bytearray(blob)
    off_frame, off_tiles = (int(x) for x in np.frombuffer(blob, dtype=np.uint32, count=26)[[10, 15]])
    i[4:7], i[7:10] = view[8:11].view(np.int32), view[12:15].view(np.int32)
    i[31], i[32], i[33], i[39], i[40] = w, h, w, 0, 1                     # frm_w, frm_h, frm_row, index, thnum
    i[34], i[35], i[36], i[37] = w, h, 1, 1                               # one tile ...
    b[off_frame:off_frame + 196] = i.tobytes()
    b[32:36] = np.uint32(1).tobytes()                                     # ... n_tiles ...
    b[off_tiles:off_tiles + 4] = i[38:39].tobytes()                       # ... that holds the global list
    ref, _, _ = qr_oracle.render(bytes(b), threads=16)
    scn = qr.Scene(blob, rebin_tiles=name.startswith("synth"), ray_queries=True)
    out = scn.render_views(torch.from_numpy(view[None]).cuda(), w, h)
    torch.cuda.synchronize()
    ok = bool((out[0].cpu().numpy().view(np.uint32) == ref).all())
    print(f"{name} {w}x{h} view_ok {int(ok)}", flush=True)
    scn.close()
    if not ok:
        rc = 1
sys.exit(rc)
