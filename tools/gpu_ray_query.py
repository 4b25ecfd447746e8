#!/usr/bin/env python3
"""Rates of the ray queries (Scene.trace / Scene.occluded, include/qrhip.h qr_trace_rays_async / qr_occluded_async) on the GPU box.

Workloads:
  demo1_1080p_camera  camera rays of demo scene 1 at 1920x1080 (rays.camera_rays), coherent=True and False, next to render()
                      of the same scene at depth 0 (the primary walk plus shading of one hit per pixel)
  demo2_random_1m     1 M random rays: origin uniform in the box of the surfaces' positions, direction uniform on the sphere
  synth10k_random_1m  the same on the synthetic 10 000-quadric scene (its global list carries a uniform grid)
Each figure is timed with HIP events around back-to-back launches over a window of >= 0.25 s after warm-up.  Prints one
JSON line (Grays/s, ms per batch, the kernel name to filter a rocprofv3 --kernel-trace by)."""
import argparse
import gzip
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qr_loader import load_package  # noqa: E402

qr = load_package()
_spec = importlib.util.spec_from_file_location("qr_rays", os.path.join(ROOT, "quadray-engine_amd", "rays.py"))
rays_mod = importlib.util.module_from_spec(_spec); _spec.loader.exec_module(rays_mod)
_spec = importlib.util.spec_from_file_location("qr_synth", os.path.join(ROOT, "quadray-engine_amd", "synth.py"))
synth = importlib.util.module_from_spec(_spec); _spec.loader.exec_module(synth)


def golden(name):
    return gzip.decompress(open(os.path.join(ROOT, "tests", "golden", name + ".qrs.gz"), "rb").read())


def timed(fn, window_s=0.25, warm=5):
    """ms per call: HIP events around back-to-back calls, the count grown until one window lasts >= window_s"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 4
    while True:
        e0.record()
        for _ in range(n):
            fn()
        e1.record(); e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= window_s * 1e3:
            return ms / n
        n = max(n * 2, int(n * window_s * 1e3 / max(ms, 1e-3) * 1.2))


def random_rays(blob, n, seed):
    s = np.frombuffer(blob, dtype=np.int32, count=26)
    n_srf, off_srf = int(s[4]), int(s[11])
    srf = np.frombuffer(blob, dtype=np.int32, count=n_srf * 64, offset=off_srf).reshape(n_srf, 64)
    real = (srf[:, 37] >= 0) & (srf[:, 37] < 9)
    pos = srf[real, 0:3].view(np.float32).astype(np.float64)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros((n, 8), dtype=np.float32)
    r[:, 0:3] = rng.uniform(lo, hi, size=(n, 3))
    r[:, 3] = 0.0
    r[:, 4:7] = d
    r[:, 7] = np.finfo(np.float32).max
    return r


def rate(n, ms):
    return {"ms": round(ms, 4), "grays_per_s": round(n / (ms * 1e-3) / 1e9, 3)}


def query_figures(scn, rays, coherent_too=False):
    r = torch.from_numpy(rays).cuda()
    n = len(rays)
    out = {"n_rays": n}
    modes = [False, True] if coherent_too else [False]
    for coh in modes:
        key = "coherent" if coh else "incoherent"
        out[f"closest_{key}"] = rate(n, timed(lambda: scn.trace(r, coherent=coh)))
        out[f"occluded_{key}"] = rate(n, timed(lambda: scn.occluded(r, coherent=coh)))
    t, ids = scn.trace(r); torch.cuda.synchronize()
    out["hit_fraction"] = round(float((ids >= 0).float().mean()), 4)
    out["occluded_fraction"] = round(float(scn.occluded(r).float().mean()), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--window", type=float, default=0.25)
    args = ap.parse_args()
    res = {"version": qr.lib().qr_version().decode(), "kernel": "qr_trace_kernel", "device": torch.cuda.get_device_name(0),
           "window_s": args.window}

    blob = golden("c2b_demo01_1080p")
    scn = qr.Scene(blob, ray_queries=True)
    cam = rays_mod.camera_rays(blob)
    d1 = query_figures(scn, cam, coherent_too=True)
    scn.set_depth(0)
    f = scn.new_frame()
    d1["render_depth0"] = rate(scn.width * scn.height, timed(lambda: scn.render(f)))
    res["demo1_1080p_camera"] = d1
    scn.close()

    blob = golden("c3_demo02_1080p_gf_d3")
    scn = qr.Scene(blob, ray_queries=True)
    res["demo2_random_1m"] = query_figures(scn, random_rays(blob, args.rays, 1))
    scn.close()

    blob = qr.build_lists(synth.make_scene(shadow_lists=False, n_objects=10000, width=1920, height=1080, depth=4))
    scn = qr.Scene(blob, rebin_tiles=True, ray_queries=True)
    st = qr.program_stats(blob, qr.UPLOAD_RAY_QUERIES)
    res["synth10k_random_1m"] = query_figures(scn, random_rays(blob, args.rays, 2))
    res["synth10k_random_1m"]["n_dda"] = st.n_dda
    scn.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
