#!/usr/bin/env python3
"""Times of path-traced views (Scene.pt_views, include/qrhip.h qr_pt_views_async) on the GPU box, each next to what it replaces
or competes with:
  own_camera   the snapshot's own camera at its own size, ONE sample per call, against set_pt(True) + render() of the same scene
               (qr_render_pt_kernel: the same instructions as before this feature, tools/kernel_asm_diff.py): what the view ray
               set-up, the walk of the ray-query list instead of the tile lists, and the state in four planes cost
  samples16    16 samples in ONE call against 16 calls of one sample: what keeping the state on chip between samples saves
  cube6        a cube map of six 512x512 views from the camera's position in ONE launch against six launches of one view
Steps (each its own child process under its own `timeout`; after a step that fails nothing else is started):
  test18_1080p     tests/golden/pt/test18_1080p_pt (the reference's path-tracer scene), own_camera and samples16
  demo2_1080p      tests/golden/c3_demo02_1080p_gf_d3 with emission patched on (tests/_ptpatch.py), own_camera and samples16
  cube_512         test18_1080p_pt, cube6
  resources        registers, spills, LDS and private segment of the two path-tracer kernels, from the build's assembly (no GPU)
Timing as tools/gpu_render_views.py: HIP events around back-to-back launches over a window of >= 0.25 s after warm-up, the
candidates alternated three times in one process; median and min .. max.  One JSON line per step.

usage: gpu_pt_views.py [--out FILE] [--window S] [--step NAME]"""
import argparse
import gzip
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STEPS = {"test18_1080p": 240, "demo2_1080p": 240, "cube_512": 180, "resources": 60}   # s


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def alternate(fns, timed, window, rounds=3):
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn, window, warm=2))
    return {k: spread(v) for k, v in t.items()}


def fresh(acc):
    """keep the sample count far from its limit (2^24) however long a window runs: the work per sample does not depend on it"""
    def wrap(fn):
        def run():
            if acc.samples > (1 << 20):
                acc.samples = 0
            fn()
        return run
    return wrap


def own_and_16(grq, blob, window):
    import torch
    qr, rays_mod, timed = grq.qr, grq.rays_mod, grq.timed
    scn = qr.Scene(blob, ray_queries=True)
    w, h = scn.width, scn.height
    vt = torch.from_numpy(rays_mod.view_of(blob)[None]).cuda()
    acc = scn.pt_views(vt)
    frames = torch.empty((1, h, w), dtype=torch.int32, device="cuda")
    f = scn.new_frame()
    scn.set_pt(True)
    keep = fresh(acc)

    def calls16():
        for _ in range(16):
            acc.step(1, frames=frames)
    res = {"width": w, "height": h, "fsaa": int(scn.info.fsaa), "depth": int(scn.info.depth)}
    res["own_camera"] = alternate({"pt_views_1": keep(lambda: acc.step(1, frames=frames)), "set_pt_render": lambda: scn.render(f)},
                                  timed, window)
    res["own_camera"]["pt_views_ms_over_render_ms"] = round(res["own_camera"]["pt_views_1"]["median_ms"] /
                                                            res["own_camera"]["set_pt_render"]["median_ms"], 3)
    res["samples16"] = alternate({"one_call_of_16": keep(lambda: acc.step(16, frames=frames)), "16_calls_of_1": keep(calls16)},
                                 timed, window)
    res["samples16"]["one_call_ms_over_16_calls_ms"] = round(res["samples16"]["one_call_of_16"]["median_ms"] /
                                                             res["samples16"]["16_calls_of_1"]["median_ms"], 3)
    scn.close()
    return res


def cube(grq, blob, window, size=512):
    import numpy as np
    import torch
    qr, rays_mod, timed = grq.qr, grq.rays_mod, grq.timed
    scn = qr.Scene(blob, ray_queries=True)
    eye = rays_mod.view_of(blob)[0:3].astype(np.float64)
    faces = [((1, 0, 0), (0, 0, 1)), ((-1, 0, 0), (0, 0, 1)), ((0, 1, 0), (0, 0, 1)), ((0, -1, 0), (0, 0, 1)),
             ((0, 0, 1), (0, 1, 0)), ((0, 0, -1), (0, 1, 0))]
    views = np.stack([rays_mod.look_at(eye, eye + np.array(d, dtype=np.float64), up, 90.0, size, size) for d, up in faces])
    vt = torch.from_numpy(views).cuda()
    acc6 = scn.pt_views(vt, size, size)
    acc1 = [scn.pt_views(vt[j:j + 1].contiguous(), size, size) for j in range(6)]
    f6 = torch.empty((6, size, size), dtype=torch.int32, device="cuda")
    f1 = torch.empty((1, size, size), dtype=torch.int32, device="cuda")

    def one_launch():
        if acc6.samples > (1 << 20):
            acc6.samples = 0
        acc6.step(1, frames=f6)

    def six_launches():
        for a in acc1:
            if a.samples > (1 << 20):
                a.samples = 0
            a.step(1, frames=f1)
    res = {"size": size, "depth": int(scn.info.depth)}
    res["cube6"] = alternate({"one_launch": one_launch, "six_launches": six_launches}, timed, window)
    res["cube6"]["one_launch_ms_over_six_ms"] = round(res["cube6"]["one_launch"]["median_ms"] / res["cube6"]["six_launches"]["median_ms"], 3)
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
        ks = [k for k in m.kernels(asm) if "qr_pt_views_kernel" in k["name"] or "qr_render_pt_kernel" in k["name"]]
        return {k["name"]: {a: k[a] for a in m.KEYS if a != "name"} for k in ks}
    import torch
    spec = importlib.util.spec_from_file_location("gpu_ray_query", os.path.join(HERE, "gpu_ray_query.py"))
    grq = importlib.util.module_from_spec(spec); spec.loader.exec_module(grq)
    res = {"version": grq.qr.lib().qr_version().decode(), "device": torch.cuda.get_device_name(0), "window_s": window}
    test18 = gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "pt", "test18_1080p_pt.qrs.gz"), "rb").read())
    if name == "test18_1080p":
        res.update(own_and_16(grq, test18, window))
    elif name == "demo2_1080p":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import _ptpatch
        res.update(own_and_16(grq, _ptpatch.pt_patch(grq.golden("c3_demo02_1080p_gf_d3")), window))
    else:
        res.update(cube(grq, test18, window))
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
