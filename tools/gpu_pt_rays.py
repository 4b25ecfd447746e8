#!/usr/bin/env python3
"""Times of path-traced rays (Scene.pt_rays, include/qrhip.h qr_pt_rays_async) on the GPU box, each next to what it competes with:
  camera16     the snapshot's own camera rays (every pixel sample, in slot order) with the pinhole spread, 16 samples in ONE call,
               against pt_views of the same camera and samples (the same walks and bounces behind a view's ray set-up: what
               reading 32 to 64 bytes of ray and spread per sample, the incoherent first round and the missing output step cost)
               and against 16 calls of one sample (what keeping the state on chip between samples saves)
  random       random rays (origin uniform in the box of the surfaces' positions, direction uniform on the sphere), no
               spread, one sample and 16 samples per call: probe and lightmap rays
Steps (each its own child process under its own `timeout`; after a step that fails nothing else is started):
  demo2_1080p      tests/golden/c3_demo02_1080p_gf_d3 with emission patched on (tests/_ptpatch.py), camera16
  test18_1080p     tests/golden/pt/test18_1080p_pt (the reference's path-tracer scene), camera16
  demo2_random_1m  the patched demo scene 2, random, 1 M rays
  synth_random     a synthetic scene of 2 000 quadrics with emission patched on, random, 256 K rays (the path-tracer instance
                   has the packet walks alone: a long list is walked cell by cell)
  resources        registers, spills, LDS and private segment of the path-tracer kernels, from the build's assembly (no GPU)
Timing as tools/gpu_pt_views.py: HIP events around back-to-back launches over a window of >= 0.25 s after warm-up, the
candidates alternated three times in one process; median and min .. max.  One JSON line per step.

usage: gpu_pt_rays.py [--out FILE] [--window S] [--step NAME]"""
import argparse
import gzip
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STEPS = {"demo2_1080p": 240, "test18_1080p": 240, "demo2_random_1m": 240, "synth_random": 300, "resources": 60}   # s


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def alternate(fns, timed, window, rounds=3, warm=2):
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn, window, warm=warm))
    return {k: spread(v) for k, v in t.items()}


def keep(acc, fn):
    """keep the sample count far from its limit (2^24) however long a window runs: the work per sample does not depend on it"""
    def run():
        if acc.samples > (1 << 20):
            acc.samples = 0
        fn()
    return run


def camera16(grq, blob, window):
    import numpy as np
    import torch
    qr, rays_mod, timed = grq.qr, grq.rays_mod, grq.timed
    scn = qr.Scene(blob, ray_queries=True)
    w, h, ns = scn.width, scn.height, 1 << int(scn.info.fsaa)
    view = rays_mod.view_of(blob)
    # every pixel sample's unjittered ray, in slot order (y * w + x) * ns + k
    r = np.stack([rays_mod.view_rays(view, w, h, blob, k) for k in range(ns)], axis=1).reshape(w * h * ns, 8)
    sp = np.zeros_like(r)
    sp[:, 0:3], sp[:, 4:7] = view[8:11], view[12:15]
    if ns > 1:
        sp *= np.float32(0.5)                   # a frame with FSAA halves its jitter once more: an exact scaling
    rt, st = torch.from_numpy(np.ascontiguousarray(r)).cuda(), torch.from_numpy(sp).cuda()
    acc = scn.pt_rays(len(r))
    rgb = torch.empty((len(r), 3), dtype=torch.float32, device="cuda")
    vt = torch.from_numpy(view[None]).cuda()
    accv = scn.pt_views(vt)
    frames = torch.empty((1, h, w), dtype=torch.int32, device="cuda")

    def calls16():
        for _ in range(16):
            acc.step(rt, 1, spread=st, rgb=rgb)
    res = {"width": w, "height": h, "fsaa": int(scn.info.fsaa), "depth": int(scn.info.depth), "n_rays": len(r)}
    res["camera16"] = alternate({"pt_rays_one_call_of_16": keep(acc, lambda: acc.step(rt, 16, spread=st, rgb=rgb)),
                                 "pt_views_one_call_of_16": keep(accv, lambda: accv.step(16, frames=frames)),
                                 "pt_rays_16_calls_of_1": keep(acc, calls16)}, timed, window)
    c = res["camera16"]
    c["pt_rays_ms_over_pt_views_ms"] = round(c["pt_rays_one_call_of_16"]["median_ms"] / c["pt_views_one_call_of_16"]["median_ms"], 3)
    c["one_call_ms_over_16_calls_ms"] = round(c["pt_rays_one_call_of_16"]["median_ms"] / c["pt_rays_16_calls_of_1"]["median_ms"], 3)
    c["msamples_per_s"] = round(16 * len(r) / (c["pt_rays_one_call_of_16"]["median_ms"] * 1e-3) / 1e6, 1)
    scn.close()
    return res


def random(grq, blob, n, window, rebin=False):
    import torch
    qr, timed = grq.qr, grq.timed
    scn = qr.Scene(blob, rebin_tiles=rebin, ray_queries=True)
    rt = torch.from_numpy(grq.random_rays(blob, n, 1)).cuda()
    acc = scn.pt_rays(n)
    rgb = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    res = {"n_rays": n, "depth": int(scn.info.depth)}
    res["random"] = alternate({"one_sample": keep(acc, lambda: acc.step(rt, 1, rgb=rgb)),
                               "one_call_of_16": keep(acc, lambda: acc.step(rt, 16, rgb=rgb))}, timed, window, warm=1)
    c = res["random"]
    c["msamples_per_s_1"] = round(n / (c["one_sample"]["median_ms"] * 1e-3) / 1e6, 1)
    c["msamples_per_s_16"] = round(16 * n / (c["one_call_of_16"]["median_ms"] * 1e-3) / 1e6, 1)
    torch.cuda.synchronize()
    c["lit_fraction"] = round(float((rgb != 0).any(dim=1).float().mean()), 4)
    scn.close()
    return res


def step(name, window):
    import importlib.util
    if name == "resources":
        spec = importlib.util.spec_from_file_location("check_kernel_resources", os.path.join(HERE, "check_kernel_resources.py"))
        m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
        asm = os.path.join(ROOT, "quadray-engine_amd", "csrc", "qr_device-hip-amdgcn-amd-amdhsa-gfx950.s")
        if not os.path.exists(asm):
            return {"assembly": "not on this machine: run this step where the library was built"}
        ks = [k for k in m.kernels(asm) if any(s in k["name"] for s in ("qr_pt_rays_kernel", "qr_pt_views_kernel", "qr_render_pt_kernel"))]
        return {k["name"]: {a: k[a] for a in m.KEYS if a != "name"} for k in ks}
    import torch
    spec = importlib.util.spec_from_file_location("gpu_ray_query", os.path.join(HERE, "gpu_ray_query.py"))
    grq = importlib.util.module_from_spec(spec); spec.loader.exec_module(grq)
    res = {"version": grq.qr.lib().qr_version().decode(), "device": torch.cuda.get_device_name(0), "window_s": window}
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _ptpatch
    if name == "test18_1080p":
        res.update(camera16(grq, gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "pt", "test18_1080p_pt.qrs.gz"), "rb").read()), window))
    elif name == "demo2_1080p":
        res.update(camera16(grq, _ptpatch.pt_patch(grq.golden("c3_demo02_1080p_gf_d3")), window))
    elif name == "demo2_random_1m":
        res.update(random(grq, _ptpatch.pt_patch(grq.golden("c3_demo02_1080p_gf_d3")), 1 << 20, window))
    else:
        blob = grq.qr.build_lists(grq.synth.make_scene(shadow_lists=False, n_objects=2000, width=1920, height=1080, depth=4))
        res.update(random(grq, _ptpatch.pt_patch(blob), 1 << 18, window, rebin=True))
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
