#!/usr/bin/env python3
"""Times of view accumulation (Scene.render_views_mean, include/qrhip.h qr_render_views_mean_async) on the GPU box, next to the
two ways the same mean could be had before it:
  (a) render_views   the same N views in ONE launch of Scene.render_views: the same ray work, N packed frames written (and the
                     mean of those is of clamped, gamma-encoded, rounded pixels: not the same result)
  (b) shade_sum      Scene.shade(coherent=True) of every view's rays.view_rays and the output step's first half (clamp1, FSAA
                     reduce) and the sum in torch on the device: the same linear sum, N full-size float planes through HBM.  At
                     most 16 distinct ray sets are kept on the device and cycled (64 views at 1080p would hold 4 GB of rays).

Steps (each its own child process under its own `timeout`; after a step that fails nothing else is started):
  demo1_1080p_d10 / _d0   demo scene 1, N = 1, 4, 16, 64 copies of its own camera shifted within +-0.5 px, 1920x1080, depth 10 / 0
  demo1_270p_n64          64 views at 480x270, depth 10: one wave per footprint whatever N is -- about 2000 waves
  synth10k_1080p_d4_n4    the synthetic 10 000-quadric scene, 4 views at 1920x1080, depth 4 (the per-lane walk instance)
  resources               registers, spills and private segment of the two kernel instances, from the build's assembly (no GPU)
Timing as tools/gpu_render_views.py: HIP events around back-to-back launches over a window of >= 0.25 s after warm-up, the
candidates alternated A B C three times in one process; median and min .. max.  One JSON line per step.

usage: gpu_views_mean.py [--out FILE] [--window S] [--step NAME]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = {"demo1_1080p_d10": 240, "demo1_1080p_d0": 240, "demo1_270p_n64": 120, "synth10k_1080p_d4_n4": 240, "resources": 60}   # s


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def compare(grq, scn, blob, views_np, w, h, window, rounds=3, with_shade=True):
    import numpy as np
    import torch
    qr, rays_mod, timed = grq.qr, grq.rays_mod, grq.timed
    n = len(views_np)
    ns = 1 << int(scn.info.fsaa)
    vt = torch.from_numpy(np.stack(views_np)).cuda()
    frames = torch.empty((n, h, w), dtype=torch.int32, device="cuda")
    frame = torch.empty((h, w), dtype=torch.int32, device="cuda")
    acc = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    fns = {"views_mean": lambda: scn.render_views_mean(vt, w, h, sum=acc, frame=frame),
           "render_views": lambda: scn.render_views(vt, w, h, frames=frames)}
    if with_shade:
        sets = [[torch.from_numpy(rays_mod.view_rays(v, w, h, blob, k)).cuda() for k in range(ns)] for v in views_np[:16]]
        one = torch.tensor(1.0, device="cuda")

        def shade_sum():
            total = None
            for j in range(n):
                c = None
                for r in sets[j % len(sets)]:
                    x = torch.minimum(scn.shade(r, coherent=True), one)
                    c = x if c is None else c + x                  # (timing only: the reduce's halvings are left out)
                total = c if total is None else total + c
            return total
        fns["shade_sum"] = shade_sum
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn, window, warm=2))
    d = {k: spread(v) for k, v in t.items()}
    d["n_views"], d["n_rays"], d["depth"] = n, n * w * h * ns, int(scn.info.depth)
    d["grays_per_s"] = round(n * w * h * ns / (d["views_mean"]["median_ms"] * 1e-3) / 1e9, 3)
    d["mean_ms_over_render_views_ms"] = round(d["views_mean"]["median_ms"] / d["render_views"]["median_ms"], 3)
    if with_shade:
        d["mean_ms_over_shade_sum_ms"] = round(d["views_mean"]["median_ms"] / d["shade_sum"]["median_ms"], 3)
    return d


def jittered(rays_mod, view, n, seed=7):
    import numpy as np
    off = np.random.default_rng(seed).uniform(-0.5, 0.5, (n, 2))
    return [rays_mod.jitter_view(view, dx, dy) for dx, dy in off]


def step(name, window):
    if name == "resources":
        import importlib.util
        spec = importlib.util.spec_from_file_location("check_kernel_resources", os.path.join(HERE, "check_kernel_resources.py"))
        m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
        asm = os.path.join(HERE, "..", "quadray-engine_amd", "csrc", "qr_device-hip-amdgcn-amd-amdhsa-gfx950.s")
        if not os.path.exists(asm):
            return {"assembly": "not on this machine: run this step where the library was built"}
        ks = [k for k in m.kernels(asm) if "qr_views_mean_kernel" in k["name"] or "qr_render_views_kernel" in k["name"]]
        return {k["name"]: {a: k[a] for a in m.KEYS if a != "name"} for k in ks}
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("gpu_ray_query", os.path.join(HERE, "gpu_ray_query.py"))
    grq = importlib.util.module_from_spec(spec); spec.loader.exec_module(grq)
    qr, rays_mod = grq.qr, grq.rays_mod
    res = {"version": qr.lib().qr_version().decode(), "device": torch.cuda.get_device_name(0), "window_s": window}
    if name.startswith("demo1"):
        blob = grq.golden("c2b_demo01_1080p")
        scn = qr.Scene(blob, ray_queries=True)
        own = rays_mod.view_of(blob)
        if name == "demo1_270p_n64":
            import numpy as np
            w, h = 480, 270
            own[8:11] *= np.float32(scn.width / w); own[12:15] *= np.float32(scn.height / h)
            scn.set_depth(10)
            res["n64"] = compare(grq, scn, blob, jittered(rays_mod, own, 64), w, h, window, with_shade=False)
        else:
            scn.set_depth(10 if name.endswith("d10") else 0)
            for n in (1, 4, 16, 64):
                res[f"n{n}"] = compare(grq, scn, blob, jittered(rays_mod, own, n), scn.width, scn.height, window)
    else:
        blob = qr.build_lists(grq.synth.make_scene(shadow_lists=False, n_objects=10000, width=1920, height=1080, depth=4))
        scn = qr.Scene(blob, rebin_tiles=True, ray_queries=True)
        res["n4"] = compare(grq, scn, blob, jittered(rays_mod, rays_mod.view_of(blob), 4), scn.width, scn.height, window)
    scn.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.step:
        print(json.dumps({args.step: step(args.step, args.window)}), flush=True)
        return 0
    lines = []
    rc = 0
    for name, limit in STEPS.items():
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name,
                            "--window", str(args.window)], capture_output=True, text=True)
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not out:
            lines.append(f"# step {name} failed with status {r.returncode}: nothing after it was started\n# " +
                         r.stderr[-2000:].replace("\n", "\n# "))
            rc = 1
            break
        lines.append(out[-1])
        print(out[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if rc:
        print(lines[-1], file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
