#!/usr/bin/env python3
"""Times of temporal reprojection with a motion table (Scene.reproject(motion=), include/qrhip.h qr_reproject_moving_async) on the
GPU box, next to the static launch on the same inputs and to the same step as a composition of torch gathers and elementwise
operations.  The scene is demo scene 2 (tests/golden/demo02_160 with its node tree, tests/golden/tree) seen through its own
camera widened to 1920 x 1080, with one object array (node NODE) spun by SPIN degrees a frame over FRAMES frames: every frame
is patched from the one before (hierarchy_apply, build_lists), uploaded as its OWN Scene, and hierarchy_motion gives its table.
  inputs        per frame Scene.view_hits and a spun 4-direction gather (the colour), from the frame's own scene
  static_ms     one qr_reproject_views_async launch of frame k against frame k - 1, outputs preallocated: device events around
                REPS launches, per launch.  Its kernel is the one of the commit before this call existed (tools/kernel_asm_diff.py
                reports it `same`); on an animated frame it loses the moved object's history, which costs it nothing
  identity_ms   the moving launch on the same inputs with a table of exact identity rows: the same pixels keep the same
                history (identity_same: every word of history, colour and variance equal to the static launch's), so the
                difference to static_ms is what the row loads and the move step cost
  moving_ms     the moving launch with the frame's table; kept_moved / kept_moved_static: pixels of moved surfaces whose
                history is longer than 1 with the table / with the static launch
  torch_ms      the same step as torch gathers and elementwise operations (tools/gpu_reproject.py torch_reproject on records moved
                by the same formulas in the same order), after the two were compared word for word (torch_same)
Steps (each its own child process under its own `timeout`; after a step that fails nothing else is started):
  demo2_1080p
One JSON line per step, then the kernels' resources from the build assembly.  A step that was not run is written as NOT MEASURED
with the reason.  No speed target is set.

usage: gpu_reproject_moving.py [--out FILE] [--step NAME]"""
import argparse
import importlib.util
import json
import os
import statistics
import struct
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STEPS = {"demo2_1080p": 300}   # s
FRAMES, REPS, NODE, SPIN, W, H = 8, 20, 8, 3.0, 1920, 1080


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def torch_move(torch, hits, table):
    """rays.move_hits in torch operations on the device, one rounding per operation: the records with pos and nrm moved, NaN
    beyond the table"""
    ids = hits.view(torch.int32)[..., 7]
    listed = (ids >= 0) & ((ids >> 1) < table.shape[0])
    r = table[torch.where(listed, ids >> 1, torch.zeros_like(ids)).long()].view(ids.shape + (3, 4))
    pos, nrm = hits[..., 0:3], hits[..., 4:7]
    mp = ((r[..., 0] * pos[..., None, 0] + r[..., 1] * pos[..., None, 1]) + r[..., 2] * pos[..., None, 2]) + r[..., 3]
    mn = (r[..., 0] * nrm[..., None, 0] + r[..., 1] * nrm[..., None, 1]) + r[..., 2] * nrm[..., None, 2]
    out = hits.clone()
    nan = torch.full_like(mp, float("nan"))
    hit = (ids >= 0)[..., None]
    out[..., 0:3] = torch.where(hit, torch.where(listed[..., None], mp, nan), pos)
    out[..., 4:7] = torch.where(hit, torch.where(listed[..., None], mn, nan), nrm)
    return out


def scene_figures(grq, gr):
    import numpy as np
    import torch
    qr, rm = grq.qr, grq.rays_mod
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _tree
    raw = grq.golden("demo02_160")
    t, table = _tree.load_tree(qr, "demo02_160")
    own = rm.view_of(raw)
    f, i = rm.frame_record(raw)
    fw, fh = int(i[31]), int(i[32])
    view = own.copy()
    centre = own[4:7] + own[8:11] * (fw / 2) + own[12:15] * (fh / 2)
    view[8:11], view[12:15] = own[8:11] * (fw / W), own[12:15] * (fw / W)
    view[4:7] = centre - view[8:11] * (W / 2) - view[12:15] * (H / 2)
    view = view.astype(np.float32)

    def events(fn, reps=1):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b) / reps)
        return round(statistics.median(ms), 4)

    flags = qr.HIER_RESET_TILES | qr.HIER_BOUNDS
    frames, blob, motion = [], qr.build_lists(raw), None
    vt = torch.from_numpy(view[None].copy()).cuda()
    dirs = torch.from_numpy(rm.cosine_dirs(4)).cuda()
    for k in range(FRAMES):
        if k:
            nxt = table.copy()
            nxt[NODE]["rot"][2] += np.float32(SPIN)
            patched = qr.hierarchy_apply(raw, nxt, t["opts"], camera=t["camera"], base=table, flags=flags)
            after = qr.hierarchy_records_after_apply(raw, nxt, t["opts"])
            motion = qr.hierarchy_motion(table, after, t["opts"], struct.unpack_from("<I", patched, 16)[0])
            raw, table, blob = patched, after, qr.build_lists(patched)
        scn = qr.Scene(blob, ray_queries=True)                       # every frame its own scene, closed after its inputs are made
        hits = scn.view_hits(vt, W, H)
        spin = torch.from_numpy(rm.spins((1, H, W), 7 + k)).cuda()
        gat, _ = scn.view_gather(vt, dirs, W, H, eps=1e-3, reach=2.0, frame=True, spin=spin)
        torch.cuda.synchronize()
        scn.close()
        frames.append((gat[..., :3].contiguous(), hits, None if motion is None else torch.from_numpy(motion).cuda()))
    scn = qr.Scene(blob)                                             # the launches read nothing of a scene but its device
    hit0 = frames[0][1]
    depth = float(hit0[..., 3][hit0.view(torch.int32)[..., 7] >= 0].median())
    pixel = float(np.linalg.norm(view[8:11])) * depth
    stops = dict(plane_max=pixel)
    p = rm.reproject_stops(**stops)
    nbytes = gr.launch_bytes(1, H, W, 3, False)
    res = {"width": W, "height": H, "frames": FRAMES, "reps": REPS, "node": NODE, "spin_degrees_per_frame": SPIN,
           "pixel_footprint": round(pixel, 6), "launch_bytes": nbytes, "table_rows": int(frames[-1][2].shape[0])}
    hist = [torch.empty((1, H, W, 8), dtype=torch.float32, device="cuda") for _ in range(2)]
    other = torch.empty_like(hist[0])
    cout, vout = torch.empty_like(frames[0][0]), torch.empty((1, H, W), dtype=torch.float32, device="cuda")
    c2, v2 = torch.empty_like(cout), torch.empty_like(vout)
    out = {k: [] for k in ("static_ms", "identity_ms", "moving_ms", "identity_same", "torch_ms", "torch_same", "kept", "moved_pixels",
                           "kept_moved", "kept_moved_static")}
    prev = None
    for k, (col, hits, table_k) in enumerate(frames):
        if table_k is None:
            table_k = torch.from_numpy(np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float32), (res["table_rows"], 1))).cuda()
        ident = torch.zeros_like(table_k)
        ident[:, 0], ident[:, 5], ident[:, 10] = 1.0, 1.0, 1.0
        dst = hist[k & 1]
        static = lambda: scn.reproject(col, hits, prev, None, out=other, colour_out=c2, variance_out=v2, **stops)
        identity = lambda: scn.reproject(col, hits, prev, None, out=dst, colour_out=cout, variance_out=vout, motion=ident, **stops)
        moving = lambda: scn.reproject(col, hits, prev, None, out=dst, colour_out=cout, variance_out=vout, motion=table_k, **stops)
        out["static_ms"].append(events(static, REPS))
        out["identity_ms"].append(events(identity, REPS))
        static(), identity()
        torch.cuda.synchronize()
        differ = sum(int((a.view(torch.int32) != b.view(torch.int32)).sum()) for a, b in ((other, dst), (c2, cout), (v2, vout)))
        out["identity_same"].append(differ == 0 or {"words_differing": differ})
        out["moving_ms"].append(events(moving, REPS))
        moving()
        th, tc, tv = gr.torch_reproject(torch, col, torch_move(torch, hits, table_k), None, prev, p)
        torch.cuda.synchronize()
        pairs = ((th, dst), (tc, cout), (tv, vout))
        differ = sum(int(((a.view(torch.int32) != b.view(torch.int32)) & ~(a.isnan() & b.isnan())).sum()) for a, b in pairs)
        out["torch_same"].append(differ == 0 or {"words_differing": differ, "of": sum(a.numel() for a, _ in pairs)})
        out["torch_ms"].append(events(lambda: gr.torch_reproject(torch, col, torch_move(torch, hits, table_k), None, prev, p), 2))
        ids = hits.view(torch.int32)[..., 7]
        rows = table_k[torch.where(ids >= 0, ids >> 1, torch.zeros_like(ids)).long()]
        moved = (ids >= 0) & ~(rows.view(torch.int32) == ident[0].view(torch.int32)).all(-1)
        out["kept"].append(round(float((dst[..., 6] > 1).float().mean()), 4))
        out["moved_pixels"].append(int(moved.sum()))
        out["kept_moved"].append(int((moved & (dst[..., 6] > 1)).sum()))
        out["kept_moved_static"].append(int((moved & (other[..., 6] > 1)).sum()))
        prev = (vt, hits, dst)
    res.update(out)
    res["identity_over_static"] = [round(a / b, 3) for a, b in zip(out["identity_ms"], out["static_ms"])]
    res["torch_ms_over_moving_ms"] = [round(a / b, 1) for a, b in zip(out["torch_ms"], out["moving_ms"])]
    res["moving_GB_per_s"] = [round(nbytes / t / 1e6, 1) for t in out["moving_ms"]]
    res["scalar_row_path"] = "NOT MEASURED: not built; the rows are per-lane 16-byte loads"
    scn.close()
    return res


def step(name):
    import torch
    grq, gr = _load("gpu_ray_query"), _load("gpu_reproject")
    res = {"version": grq.qr.lib().qr_version().decode(), "device": torch.cuda.get_device_name(0)}
    res.update(scene_figures(grq, gr))
    return res


def resources():
    sys.path.insert(0, HERE)
    import check_kernel_resources as ck
    asm = os.path.join(ROOT, "quadray-engine_amd", "csrc", "qr_device-hip-amdgcn-amd-amdhsa-gfx950.s")
    if not os.path.exists(asm):
        return {"resources": "no build assembly in this tree"}
    return {"resources": {k["name"]: {a: k[a] for a in ck.KEYS if a != "name"} for k in ck.kernels(asm)
                          if "qr_reproject_kernel" in k["name"] or "qr_reproj_moving_kernel" in k["name"]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.step:
        print(json.dumps({args.step: step(args.step)}), flush=True)
        return 0
    lines = []
    rc = 0
    names = list(STEPS)
    for k, name in enumerate(names):
        r = subprocess.run(["timeout", "-k", "10", str(STEPS[name]), sys.executable, os.path.abspath(__file__), "--step", name],
                           capture_output=True, text=True)
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not out:
            lines.append(f"# step {name} failed with status {r.returncode}: nothing after it was started\n# " +
                         r.stderr[-2000:].replace("\n", "\n# "))
            lines += [f"# {later}: NOT MEASURED (the step {name} before it failed)" for later in names[k + 1:]]
            rc = 1
            break
        lines.append(out[-1])
        print(out[-1], flush=True)
    if rc == 0:
        lines.append(json.dumps(resources()))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if rc:
        print("\n".join(lines[-len(names):]), file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
