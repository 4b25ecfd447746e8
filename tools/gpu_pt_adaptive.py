#!/usr/bin/env python3
"""Times of adaptive path-traced rays (Scene.pt_adaptive, include/qrhip.h qr_pt_adapt_rays_async) on the GPU box, next to what a host
would do without them.  The rays are the snapshot's own camera rays at 1080p (every pixel sample, in slot order) with the pinhole
spread; min_samples 8, max_samples 64, 8 candidates per call.  Per scene:
  tolerance    found by bisection so that about half of the LIT rays (a non-zero mean after 64 samples) stop before 64; the value
               used is in the result
  adaptive     reset, then step(8 candidates, open=True) until open == 0: time of the whole loop (the read of `open` after every
               call included) and the total of samples taken (the sum of plane 4)
  uniform64    Scene.pt_rays, 64 samples for every ray in 8 calls of 8: the same picture without a stop rule
  composition  what a host composes from pt_rays today: per round gather the open rays, their spread and their state columns,
               pt_rays.step(8) on the subset, scatter the columns back.  pt_rays has no noise estimate, so the open set of every
               round is GIVEN to this candidate (recorded from the adaptive run, uploaded before the clock starts): its time is a
               lower bound on the composition, which would also have to keep a second accumulation to find that set
Steps (each its own child process under its own `timeout`; after a step that fails nothing else is started):
  demo2_1080p   tests/golden/c3_demo02_1080p_gf_d3 with emission patched on (tests/_ptpatch.py)
  test18_1080p  tests/golden/pt/test18_1080p_pt (the reference's path-tracer scene)
Timing: wall clock around the whole loop between two device synchronisations, after one warm-up run, the three candidates
alternated three times in one process; median and min .. max.  One JSON line per step.

usage: gpu_pt_adaptive.py [--out FILE] [--step NAME]"""
import argparse
import gzip
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STEPS = {"demo2_1080p": 400, "test18_1080p": 400}   # s
MIN, MAX, PER_CALL = 8, 64, 8


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def scene_figures(grq, blob):
    import numpy as np
    import torch
    qr, rays_mod = grq.qr, grq.rays_mod
    scn = qr.Scene(blob, ray_queries=True)
    w, h, ns = scn.width, scn.height, 1 << int(scn.info.fsaa)
    view = rays_mod.view_of(blob)
    r = np.stack([rays_mod.view_rays(view, w, h, blob, k) for k in range(ns)], axis=1).reshape(w * h * ns, 8)
    sp = np.zeros_like(r)
    sp[:, 0:3], sp[:, 4:7] = view[8:11], view[12:15]
    if ns > 1:
        sp *= np.float32(0.5)                   # a frame with FSAA halves its jitter once more: an exact scaling
    n = len(r)
    rt, st = torch.from_numpy(np.ascontiguousarray(r)).cuda(), torch.from_numpy(sp).cuda()
    rgb = torch.empty((n, 3), dtype=torch.float32, device="cuda")

    def adaptive(tol, masks=None):
        """one whole run: (accumulator, calls); masks: a list that receives the open set before every call after the first"""
        acc = scn.pt_adaptive(n, MIN, MAX, tol)
        calls = 0
        while True:
            _, still = acc.step(rt, PER_CALL, spread=st, rgb=rgb, open=True)
            calls += 1
            if int(still) == 0 or calls >= MAX:
                return acc, calls
            if masks is not None:
                host = acc.state.cpu().numpy()
                masks.append(torch.from_numpy(rays_mod.pt_adapt_open(host, MIN, MAX, acc.tol2)).cuda())

    # the lit rays, from 64 samples for everyone
    uni = scn.pt_rays(n)

    def uniform64():
        uni.reset()
        for _ in range(MAX // PER_CALL):
            uni.step(rt, PER_CALL, spread=st, rgb=rgb)
    uniform64()
    torch.cuda.synchronize()
    lit = (rgb != 0).any(dim=1)
    n_lit = int(lit.sum())

    def early_of(tol):
        acc, _ = adaptive(tol)
        return float((acc.counts[lit] < MAX).float().mean()) if n_lit else 0.0
    lo, hi = 1e-4, 16.0                         # bisection on log(tol): the fraction stopped early grows with the tolerance
    for _ in range(9):
        mid = (lo * hi) ** 0.5
        if early_of(mid) < 0.5:
            lo = mid
        else:
            hi = mid
    tol = float(np.float32((lo * hi) ** 0.5))
    masks = []
    acc, calls = adaptive(tol, masks)
    counts = acc.counts.cpu().numpy().view(np.uint32)
    idxs = [torch.nonzero(m).squeeze(1) for m in masks]

    def composition():
        state = torch.empty((4, n), dtype=torch.int32, device="cuda")
        full = scn.pt_rays(n, state=state, samples=0)
        full.reset()
        full.step(rt, PER_CALL, spread=st, rgb=rgb)
        done = PER_CALL
        for idx in idxs:
            sub = scn.pt_rays(len(idx), state=state[:, idx].contiguous(), samples=done)
            out = sub.step(rt[idx].contiguous(), PER_CALL, spread=st[idx].contiguous())
            state[:, idx] = sub.state
            rgb[idx] = out
            done += PER_CALL

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    fns = {"adaptive": lambda: adaptive(tol), "uniform64": uniform64, "composition": composition}
    for fn in fns.values():
        fn()
    t = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            t[k].append(wall(fn))
    res = {"width": w, "height": h, "fsaa": int(scn.info.fsaa), "depth": int(scn.info.depth), "n_rays": n, "lit_rays": n_lit,
           "min_samples": MIN, "max_samples": MAX, "candidates_per_call": PER_CALL, "tol": tol, "tol2": float(acc.tol2),
           "lit_rays_stopped_early": round(float((counts[lit.cpu().numpy()] < MAX).mean()), 4) if n_lit else None,
           "calls_to_open_0": calls, "samples_taken": int(counts.sum()), "samples_uniform64": MAX * n,
           "composition_samples": int(PER_CALL * (n + sum(len(i) for i in idxs)))}
    res.update({k: spread(v) for k, v in t.items()})
    res["adaptive_ms_over_uniform64_ms"] = round(res["adaptive"]["median_ms"] / res["uniform64"]["median_ms"], 3)
    res["adaptive_ms_over_composition_ms"] = round(res["adaptive"]["median_ms"] / res["composition"]["median_ms"], 3)
    scn.close()
    return res


def step(name):
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("gpu_ray_query", os.path.join(HERE, "gpu_ray_query.py"))
    grq = importlib.util.module_from_spec(spec); spec.loader.exec_module(grq)
    res = {"version": grq.qr.lib().qr_version().decode(), "device": torch.cuda.get_device_name(0)}
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _ptpatch
    if name == "test18_1080p":
        res.update(scene_figures(grq, gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "pt", "test18_1080p_pt.qrs.gz"), "rb").read())))
    else:
        res.update(scene_figures(grq, _ptpatch.pt_patch(grq.golden("c3_demo02_1080p_gf_d3"))))
    return res


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
    for name, limit in STEPS.items():
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           capture_output=True, text=True)
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
