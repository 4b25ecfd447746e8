#!/usr/bin/env python3
"""Times of adaptive path-traced views (Scene.pt_adaptive_views, include/qrhip.h qr_pt_adapt_views_async) on the GPU box, next
to the two things a host has without them.  Scenes, camera and settings are those of tools/gpu_pt_adaptive.py and
profiles/r14_pt_adaptive.txt: the snapshot's own camera at 1080p, min_samples 8, max_samples 64, 8 candidates per call, and the
tolerances that run found (TOL).  Per scene:
  adaptive_views  reset, then step(8 candidates, open=True) until open == 0: time of the whole loop (the read of `open` after
                  every call included), the number of calls and the total of samples taken (the sum of plane 4)
  uniform64       Scene.pt_views, 64 samples for every slot in 8 calls of 8: the same picture without a stop rule
  adaptive_rays   Scene.pt_adaptive on the same camera's rays (every pixel sample, in slot order) with the pinhole spread, the
                  same loop: what a host does today, without the frame's output step
  cube_one / cube_six   a cube map at the camera's origin, six 512 x 512 views of 90 degrees: the adaptive loop with the six
                  views in ONE launch per call against six accumulations stepped one after the other (the loop ends when all
                  six report open == 0)
Steps (each its own child process under its own `timeout`; after a step that fails nothing else is started):
  demo2_1080p   tests/golden/c3_demo02_1080p_gf_d3 with emission patched on (tests/_ptpatch.py)
  test18_1080p  tests/golden/pt/test18_1080p_pt (the reference's path-tracer scene)
Timing: wall clock around the whole loop between two device synchronisations, after one warm-up run, the candidates alternated
three times in one process; median and min .. max.  One JSON line per step.

usage: gpu_pt_adaptive_views.py [--out FILE] [--step NAME]"""
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
STEPS = {"demo2_1080p": 300, "test18_1080p": 300}   # s
MIN, MAX, PER_CALL = 8, 64, 8
TOL = {"demo2_1080p": 0.2571115493774414, "test18_1080p": 0.00010117708006873727}       # profiles/r14_pt_adaptive.txt
CUBE = 512


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def scene_figures(grq, blob, tol):
    import numpy as np
    import torch
    qr, rays_mod = grq.qr, grq.rays_mod
    scn = qr.Scene(blob, ray_queries=True)
    w, h, ns = scn.width, scn.height, 1 << int(scn.info.fsaa)
    view = rays_mod.view_of(blob)
    vt = torch.from_numpy(view[None].copy()).cuda()
    frames = torch.empty((1, h, w), dtype=torch.int32, device="cuda")
    slots = w * h * ns

    def loop(accs, outs):
        """step every accumulation until all report open == 0: the number of rounds"""
        calls, live = 0, list(range(len(accs)))
        while live and calls < MAX:
            still = [accs[i].step(PER_CALL, frames=outs[i], open=True)[1] for i in live]
            calls += 1
            live = [i for i, s in zip(live, still) if int(s) != 0]
        return calls

    av = scn.pt_adaptive_views(vt, w, h, min_samples=MIN, max_samples=MAX, tol=tol)

    def adaptive_views():
        av.reset()
        return loop([av], [frames])

    uni = scn.pt_views(vt, w, h)

    def uniform64():
        uni.reset()
        for _ in range(MAX // PER_CALL):
            uni.step(PER_CALL, frames=frames)

    r = np.stack([rays_mod.view_rays(view, w, h, blob, k) for k in range(ns)], axis=1).reshape(slots, 8)
    sp = np.zeros_like(r)
    sp[:, 0:3], sp[:, 4:7] = view[8:11], view[12:15]
    if ns > 1:
        sp *= np.float32(0.5)                   # a frame with FSAA halves its jitter once more: an exact scaling
    rt, st = torch.from_numpy(np.ascontiguousarray(r)).cuda(), torch.from_numpy(sp).cuda()
    rgb = torch.empty((slots, 3), dtype=torch.float32, device="cuda")
    ar = scn.pt_adaptive(slots, MIN, MAX, tol)

    def adaptive_rays():
        ar.reset()
        calls = 0
        while calls < MAX:
            _, still = ar.step(rt, PER_CALL, spread=st, rgb=rgb, open=True)
            calls += 1
            if int(still) == 0:
                return calls
        return calls

    eye = view[0:3].astype(np.float64)
    faces = [((1, 0, 0), (0, 1, 0)), ((-1, 0, 0), (0, 1, 0)), ((0, 1, 0), (0, 0, 1)), ((0, -1, 0), (0, 0, 1)),
             ((0, 0, 1), (0, 1, 0)), ((0, 0, -1), (0, 1, 0))]
    cube = np.stack([rays_mod.look_at(eye, eye + np.array(d, dtype=np.float64), u, 90.0, CUBE, CUBE) for d, u in faces])
    ct = torch.from_numpy(cube).cuda()
    cf = torch.empty((6, CUBE, CUBE), dtype=torch.int32, device="cuda")
    c_one = scn.pt_adaptive_views(ct, CUBE, CUBE, min_samples=MIN, max_samples=MAX, tol=tol)
    c_six = [scn.pt_adaptive_views(ct[j:j + 1].contiguous(), CUBE, CUBE, min_samples=MIN, max_samples=MAX, tol=tol) for j in range(6)]

    def cube_one():
        c_one.reset()
        return loop([c_one], [cf])

    def cube_six():
        for a in c_six:
            a.reset()
        return loop(c_six, [cf[j:j + 1] for j in range(6)])

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    fns = {"adaptive_views": adaptive_views, "uniform64": uniform64, "adaptive_rays": adaptive_rays, "cube_one": cube_one,
           "cube_six": cube_six}
    calls = {k: fn() for k, fn in fns.items()}              # the warm-up run
    torch.cuda.synchronize()
    v_counts = av.counts.cpu().numpy().view(np.uint32)
    r_counts = ar.counts.cpu().numpy().view(np.uint32)
    lit = (uni.state[0, 1:4].cpu().numpy() != 0).any(axis=0)
    cube_same = all(bool((c_one.state[j] == c_six[j].state[0]).all()) for j in range(6))
    t = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            t[k].append(wall(fn))
    res = {"width": w, "height": h, "fsaa": int(scn.info.fsaa), "depth": int(scn.info.depth), "slots": slots, "lit_slots": int(lit.sum()),
           "min_samples": MIN, "max_samples": MAX, "candidates_per_call": PER_CALL, "tol": tol, "tol2": float(av.tol2),
           "lit_slots_stopped_early": round(float((v_counts[0][lit] < MAX).mean()), 4) if lit.any() else None,
           "calls_to_open_0": {k: v for k, v in calls.items() if v is not None},
           "samples_taken_views": int(v_counts.sum()), "samples_taken_rays": int(r_counts.sum()), "samples_uniform64": MAX * slots,
           "cube_size": CUBE, "cube_samples_taken": int(c_one.counts.cpu().numpy().view(np.uint32).sum()),
           "cube_samples_uniform64": 6 * MAX * CUBE * CUBE * ns, "cube_one_launch_state_equals_six_launches": cube_same}
    res.update({k: spread(v) for k, v in t.items()})
    res["adaptive_views_ms_over_uniform64_ms"] = round(res["adaptive_views"]["median_ms"] / res["uniform64"]["median_ms"], 3)
    res["adaptive_views_ms_over_adaptive_rays_ms"] = round(res["adaptive_views"]["median_ms"] / res["adaptive_rays"]["median_ms"], 3)
    res["cube_one_ms_over_cube_six_ms"] = round(res["cube_one"]["median_ms"] / res["cube_six"]["median_ms"], 3)
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
        blob = gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "pt", "test18_1080p_pt.qrs.gz"), "rb").read())
    else:
        blob = _ptpatch.pt_patch(grq.golden("c3_demo02_1080p_gf_d3"))
    res.update(scene_figures(grq, blob, TOL[name]))
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
