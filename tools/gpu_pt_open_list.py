#!/usr/bin/env python3
"""Times of the compacted adaptive loop (PtAdaptive.open_list + step(index=, count=, cap=); include/qrhip.h
qr_pt_adapt_open_list_async, qr_pt_adapt_list_rays_async) on the GPU box, next to the plain adaptive loop and the host-side
composition of tools/gpu_pt_adaptive.py -- same scenes, rays and settings: the snapshot's own camera rays at 1080p (every pixel
sample, in slot order) with the pinhole spread; min_samples 8, max_samples 64, 8 candidates per call; the tolerances recorded in
profiles/r14_pt_adaptive.txt (TOL below), not bisected again.  Per scene, in one process and one library:
  plain        reset, then step(8, open=True) until open == 0 (the read of `open` after every call included): the baseline
  compacted    reset, then open_list() and step(8, index, count, cap = the open read back, open=True) until that is 0
  composition  gather the open rays, their spread and their state columns, pt_rays.step(8) on the subset, scatter -- with the open
               set of every round GIVEN to it (recorded from a plain run before the clock starts), as in tools/gpu_pt_adaptive.py
  list_only    the three list launches alone on the state after the first plain call (n = 2 073 600): wall clock of 20 calls
               between two synchronisations, per call
The plain and the compacted loop must end with bit-identical states: asserted, with the sum of samples taken.
Steps (each its own child process under its own `timeout`; after a step that fails nothing else is started):
  demo2_1080p   tests/golden/c3_demo02_1080p_gf_d3 with emission patched on (tests/_ptpatch.py)
  test18_1080p  tests/golden/pt/test18_1080p_pt (the reference's path-tracer scene)
Timing: wall clock around the whole loop between two device synchronisations, after one warm-up run, the three candidates
alternated three times; median and min .. max.  One JSON line per step.

usage: gpu_pt_open_list.py [--out FILE] [--step NAME]"""
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
TOL = {"demo2_1080p": 0.2571115493774414, "test18_1080p": 0.00010117708006873727}      # profiles/r14_pt_adaptive.txt


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def scene_figures(grq, blob, tol):
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

    def plain(masks=None):
        """one whole run: (accumulator, open after every call); masks: a list that receives the open set before every call after the first"""
        acc = scn.pt_adaptive(n, MIN, MAX, tol)
        opens = []
        while True:
            _, still = acc.step(rt, PER_CALL, spread=st, rgb=rgb, open=True)
            opens.append(int(still))
            if opens[-1] == 0 or len(opens) >= MAX:
                return acc, opens
            if masks is not None:
                host = acc.state.cpu().numpy()
                masks.append(torch.from_numpy(rays_mod.pt_adapt_open(host, MIN, MAX, acc.tol2)).cuda())

    def compacted():
        acc = scn.pt_adaptive(n, MIN, MAX, tol)
        opens, cap = [], n
        while cap and len(opens) < MAX:
            index, count = acc.open_list()
            _, still = acc.step(rt, PER_CALL, spread=st, rgb=rgb, open=True, index=index, count=count, cap=cap)
            cap = int(still)
            opens.append(cap)
        return acc, opens

    masks = []
    pa, p_opens = plain(masks)
    ca, c_opens = compacted()
    torch.cuda.synchronize()
    assert torch.equal(pa.state, ca.state) and p_opens == c_opens, "the compacted loop does not end with the plain loop's state"
    counts = pa.counts.cpu().numpy().view(np.uint32)
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
    fns = {"plain": plain, "compacted": compacted, "composition": composition}
    for fn in fns.values():
        fn()
    t = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            t[k].append(wall(fn))
    # the list launches alone, on a state with open and closed rays side by side
    one = scn.pt_adaptive(n, MIN, MAX, tol)
    one.step(rt, PER_CALL, spread=st, rgb=False)
    _, cnt = one.open_list()

    def lists():
        for _ in range(20):
            one.open_list()
    lists()
    lt = [wall(lists) / 20 for _ in range(3)]
    res = {"width": w, "height": h, "fsaa": int(scn.info.fsaa), "depth": int(scn.info.depth), "n_rays": n,
           "min_samples": MIN, "max_samples": MAX, "candidates_per_call": PER_CALL, "tol": tol, "tol2": float(pa.tol2),
           "open_after_each_call": p_opens, "samples_taken": int(counts.sum()), "states_bit_identical": True,
           "list_only_open": int(cnt.cpu()[0])}
    res.update({k: spread(v) for k, v in t.items()})
    res["list_only"] = spread(lt)
    res["compacted_ms_over_plain_ms"] = round(res["compacted"]["median_ms"] / res["plain"]["median_ms"], 3)
    res["composition_ms_over_plain_ms"] = round(res["composition"]["median_ms"] / res["plain"]["median_ms"], 3)
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
        res.update(scene_figures(grq, gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "pt", "test18_1080p_pt.qrs.gz"), "rb").read()), TOL[name]))
    else:
        res.update(scene_figures(grq, _ptpatch.pt_patch(grq.golden("c3_demo02_1080p_gf_d3")), TOL[name]))
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
