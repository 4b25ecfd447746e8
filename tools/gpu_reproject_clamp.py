#!/usr/bin/env python3
"""Times of temporal reprojection with a clamp (Scene.reproject(clamp=), include/qrhip.h qr_reproject_clamped_async) on the GPU
box, next to the unclamped moving launch on the same inputs and to the same step as torch operations, and what the clamp does to
the trail of a moved shadow.  Scene, camera, size and motion are those of tools/gpu_reproject_moving.py
(profiles/r31_reproject_moving.txt): demo scene 2 through its own camera widened to 1920 x 1080, object array NODE spun by SPIN
degrees a frame over FRAMES frames, every frame its OWN Scene.  The colour of a frame is Scene.shade of its view rays: noise-free,
so that what the accumulated colour differs from it by is lag and nothing else.
  moving_ms     the unclamped moving launch of frame k against frame k - 1 (the kernel of the commit before this call:
                tools/kernel_asm_diff.py reports it `same`), outputs preallocated, device events around REPS launches
  clamp_ms      the clamped launch, moved_out given, per mode and radius; clamp_over_moving their ratio
  torch_ms      the same step as torch operations (tools/gpu_reproject.py torch_reproject(clamp=)) at radius 1 in both modes,
                after the two were compared word for word, moved plane included (torch_same)
  static_moved  pixels of surfaces that did not move (identity rows) whose moved is above 0, per frame (min/max, radius 1)
  trail_frames  after the last spun frame the scene stands still and its last frame is fed again: launches until the largest
                |colour_out - shade| over the static surfaces' pixels is below 1/255, without and with the clamp (min/max and
                variance at radius 1), TRAIL_MAX at the most; pixels_above: how many of those pixels are still at or above
                1/255 after 0, 1, 2, 4, ... launches; left: the largest difference at the end.  Reported, not gated
Steps (each its own child process under its own `timeout`; after a step that fails nothing else is started):
  demo2_1080p
One JSON line per step, then the kernels' resources from the build assembly.  The box is evaluated directly; a separable row and
column pass is NOT MEASURED: not built.  No speed target is set.

usage: gpu_reproject_clamp.py [--out FILE] [--step NAME]"""
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
STEPS = {"demo2_1080p": 420}   # s
FRAMES, REPS, NODE, SPIN, W, H, TRAIL_MAX = 8, 20, 8, 3.0, 1920, 1080, 96


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def scene_figures(grq, gr, gm):
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
        rays = torch.from_numpy(rm.view_rays(view, W, H, blob, 0)).cuda()
        col = scn.shade(rays, coherent=True).reshape(1, H, W, 3).contiguous()
        torch.cuda.synchronize()
        scn.close()
        frames.append((col, hits, None if motion is None else torch.from_numpy(motion).cuda()))
    scn = qr.Scene(blob)                                             # the launches read nothing of a scene but its device
    hit0 = frames[0][1]
    depth = float(hit0[..., 3][hit0.view(torch.int32)[..., 7] >= 0].median())
    pixel = float(np.linalg.norm(view[8:11])) * depth
    stops = dict(plane_max=pixel)                                    # max_len 32, alpha_min 0.05: the defaults
    p = rm.reproject_stops(**stops)
    rows = int(frames[-1][2].shape[0])
    ident = torch.zeros((rows, 12), dtype=torch.float32, device="cuda")
    ident[:, 0], ident[:, 5], ident[:, 10] = 1.0, 1.0, 1.0
    blocks = {f"{mode}_r{r}": rm.clamp_stops(mode, r) for mode in ("minmax", "variance") for r in (1, 2, 3)}
    res = {"width": W, "height": H, "frames": FRAMES, "reps": REPS, "node": NODE, "spin_degrees_per_frame": SPIN,
           "pixel_footprint": round(pixel, 6), "table_rows": rows, "colour": "Scene.shade of the frame's view rays"}
    new = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    plain_hist, clamp_hist = [new(1, H, W, 8) for _ in range(2)], [new(1, H, W, 8) for _ in range(2)]
    scratch, cout, vout, mout = new(1, H, W, 8), new(1, H, W, 3), new(1, H, W), new(1, H, W)
    out = {"moving_ms": [], "static_moved": [], "static_pixels": []}
    out.update({f"clamp_ms_{name}": [] for name in blocks})
    out.update({f"torch_ms_{name}": [] for name in ("minmax_r1", "variance_r1")})
    out.update({f"torch_same_{name}": [] for name in ("minmax_r1", "variance_r1")})
    prev_plain = prev_clamp = None
    for k, (col, hits, table_k) in enumerate(frames):
        table_k = ident if table_k is None else table_k
        moving = lambda dst=scratch, prev=prev_plain: scn.reproject(col, hits, prev, None, out=dst, colour_out=cout, variance_out=vout,
                                                                    motion=table_k, **stops)
        out["moving_ms"].append(events(moving, REPS))
        for name, c in blocks.items():
            clamped = lambda c=c: scn.reproject(col, hits, prev_clamp, None, out=scratch, colour_out=cout, variance_out=vout,
                                                motion=table_k, clamp=c, moved=mout, **stops)
            out[f"clamp_ms_{name}"].append(events(clamped, REPS))
            if name in ("minmax_r1", "variance_r1"):
                clamped()
                tt = gr.torch_reproject(torch, col, gm.torch_move(torch, hits, table_k), None, prev_clamp, p, clamp=c)
                torch.cuda.synchronize()
                pairs = tuple(zip(tt, (scratch, cout, vout, mout)))
                differ = sum(int(((a.view(torch.int32) != b.view(torch.int32)) & ~(a.isnan() & b.isnan())).sum()) for a, b in pairs)
                out[f"torch_same_{name}"].append(differ == 0 or {"words_differing": differ, "of": sum(a.numel() for a, _ in pairs)})
                out[f"torch_ms_{name}"].append(events(lambda: gr.torch_reproject(torch, col, gm.torch_move(torch, hits, table_k), None,
                                                                                 prev_clamp, p, clamp=c), 2))
        # the two chains go on: unclamped, and min/max at radius 1
        moving(plain_hist[k & 1], prev_plain)
        scn.reproject(col, hits, prev_clamp, None, out=clamp_hist[k & 1], colour_out=cout, variance_out=vout, motion=table_k,
                      clamp=blocks["minmax_r1"], moved=mout, **stops)
        ids = hits.view(torch.int32)[..., 7]
        rws = table_k[torch.where(ids >= 0, ids >> 1, torch.zeros_like(ids)).long()]
        static = (ids >= 0) & (rws.view(torch.int32) == ident[0].view(torch.int32)).all(-1)
        out["static_pixels"].append(int(static.sum()))
        out["static_moved"].append(int((static & (mout > 0)).sum()))
        prev_plain, prev_clamp = (vt, hits, plain_hist[k & 1]), (vt, hits, clamp_hist[k & 1])
    # the trail: the scene stands still from here on; each chain starts from the history the spun frames left it
    col, hits, _ = frames[-1]
    ids = hits.view(torch.int32)[..., 7]
    rws = frames[-1][2][torch.where(ids >= 0, ids >> 1, torch.zeros_like(ids)).long()]
    static = (ids >= 0) & (rws.view(torch.int32) == ident[0].view(torch.int32)).all(-1)
    trail = {}
    for name, c in (("unclamped", None), ("minmax_r1", blocks["minmax_r1"]), ("variance_r1", blocks["variance_r1"])):
        # the variance chain has no history of its own from the spun frames: it starts from the unclamped one, the worst case
        start = prev_plain[2] if name != "minmax_r1" else prev_clamp[2]
        pair = [start.clone(), torch.empty_like(start)]
        err = (pair[0][..., :3] - col).abs().amax(-1)[static]
        worst, n = float(err.max()), 0
        above = {0: int((err >= 1 / 255).sum())}
        while worst >= 1 / 255 and n < TRAIL_MAX:
            kw = {} if c is None else dict(clamp=c)
            scn.reproject(col, hits, (vt, hits, pair[n & 1]), None, out=pair[(n & 1) ^ 1], colour_out=cout, variance_out=vout,
                          motion=ident, **kw, **stops)
            n += 1
            err = (cout - col).abs().amax(-1)[static]
            worst = float(err.max())
            if n in (1, 2, 4, 8, 16, 32, 64):
                above[n] = int((err >= 1 / 255).sum())
        trail[name] = {"launches": n if worst < 1 / 255 else f"more than {TRAIL_MAX}", "left": round(worst, 6), "pixels_above": above}
    res.update(out)
    res["trail_frames"] = trail
    for name in blocks:
        res[f"clamp_over_moving_{name}"] = [round(a / b, 3) for a, b in zip(out[f"clamp_ms_{name}"], out["moving_ms"])]
    for name in ("minmax_r1", "variance_r1"):
        res[f"torch_over_clamp_{name}"] = [round(a / b, 1) for a, b in zip(out[f"torch_ms_{name}"], out[f"clamp_ms_{name}"])]
    res["separable_box"] = "NOT MEASURED: not built; the box is evaluated directly from the staged planes"
    scn.close()
    return res


def step(name):
    import torch
    grq, gr, gm = _load("gpu_ray_query"), _load("gpu_reproject"), _load("gpu_reproject_moving")
    res = {"version": grq.qr.lib().qr_version().decode(), "device": torch.cuda.get_device_name(0)}
    res.update(scene_figures(grq, gr, gm))
    return res


def resources():
    sys.path.insert(0, HERE)
    import check_kernel_resources as ck
    asm = os.path.join(ROOT, "quadray-engine_amd", "csrc", "qr_device-hip-amdgcn-amd-amdhsa-gfx950.s")
    if not os.path.exists(asm):
        return {"resources": "no build assembly in this tree"}
    return {"resources": {k["name"]: {a: k[a] for a in ck.KEYS if a != "name"} for k in ck.kernels(asm)
                          if "qr_reproj_clamp_kernel" in k["name"] or "qr_reproj_moving_kernel" in k["name"]}}


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
