#!/usr/bin/env python3
"""Rates of ray shading (Scene.shade, include/qrhip.h qr_shade_rays_async) on the GPU box.

Workloads:
  demo1_1080p_camera_d10 / _d0  camera rays of demo scene 1 at 1920x1080 (rays.camera_rays), shaded at depth 10 and at depth 0,
                                coherent=True and False, next to render() of the same scene at the same depth (one launch at a
                                time: the first hit there walks the tile lists, here the global list)
  demo2_random_1m               1 M random rays (tools/gpu_ray_query.py random_rays) on demo scene 2 at its own depth (3)
  synth10k_random_1m            the same on the synthetic 10 000-quadric scene at its own depth (4)
Timing as tools/gpu_ray_query.py: HIP events around back-to-back launches over a window of >= 0.25 s after warm-up.  Prints one
JSON line (Grays/s, ms per batch, the kernel name to filter a rocprofv3 --kernel-trace by)."""
import argparse
import importlib.util
import json
import os

import torch

_spec = importlib.util.spec_from_file_location("gpu_ray_query", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                             "gpu_ray_query.py"))
grq = importlib.util.module_from_spec(_spec); _spec.loader.exec_module(grq)
qr, rays_mod, synth, golden, timed, rate, random_rays = (grq.qr, grq.rays_mod, grq.synth, grq.golden, grq.timed, grq.rate,
                                                          grq.random_rays)


def shade_figures(scn, rays, window, coherent_too=False):
    r = torch.from_numpy(rays).cuda()
    n = len(rays)
    out = {"n_rays": n, "depth": int(scn.info.depth)}
    for coh in ([False, True] if coherent_too else [False]):
        out["shade_coherent" if coh else "shade_incoherent"] = rate(n, timed(lambda: scn.shade(r, coherent=coh), window))
    rgb, ids = scn.shade(r, ids=True)
    torch.cuda.synchronize()
    out["hit_fraction"] = round(float((ids >= 0).float().mean()), 4)
    out["mean_rgb"] = [round(float(v), 4) for v in rgb.mean(dim=0).cpu()]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--window", type=float, default=0.25)
    args = ap.parse_args()
    res = {"version": qr.lib().qr_version().decode(), "kernel": "qr_shade_rays_kernel", "device": torch.cuda.get_device_name(0),
           "window_s": args.window}

    blob = golden("c2b_demo01_1080p")
    scn = qr.Scene(blob, ray_queries=True)
    cam = rays_mod.camera_rays(blob)
    f = scn.new_frame()
    for depth in (10, 0):
        scn.set_depth(depth)
        d = shade_figures(scn, cam, args.window, coherent_too=True)
        d["render"] = rate(scn.width * scn.height, timed(lambda: scn.render(f), args.window))
        d["shade_ms_over_render_ms"] = round(d["shade_incoherent"]["ms"] / d["render"]["ms"], 3)
        res[f"demo1_1080p_camera_d{depth}"] = d
    scn.close()

    blob = golden("c3_demo02_1080p_gf_d3")
    scn = qr.Scene(blob, ray_queries=True)
    res["demo2_random_1m"] = shade_figures(scn, random_rays(blob, args.rays, 1), args.window)
    scn.close()

    blob = qr.build_lists(synth.make_scene(shadow_lists=False, n_objects=10000, width=1920, height=1080, depth=4))
    scn = qr.Scene(blob, rebin_tiles=True, ray_queries=True)
    res["synth10k_random_1m"] = shade_figures(scn, random_rays(blob, args.rays, 2), args.window)
    scn.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
