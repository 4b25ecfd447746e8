#!/usr/bin/env python3
"""Times of hit records (Scene.hits / Scene.view_hits, include/qrhip.h qr_hit_rays_async / qr_hit_views_async) on the GPU box,
next to the calls they extend.

Workloads:
  demo1_1080p_camera   hits against trace on the camera rays of demo scene 1 at 1920x1080 (rays.camera_rays), coherent and not
  demo2_random_1m      hits against trace on 1 M random rays: origin uniform in the box of the surfaces' positions, direction
                       uniform on the sphere
  synth10k_random_1m   the same on the synthetic 10 000-quadric scene (its global list carries a uniform grid)
  demo1_1080p_views    view_hits against render_views at depth 0 (one walk and one shaded hit per pixel) on demo scene 1's own
                       camera at 1920x1080
Each pair is alternated A B five times, each window HIP events around back-to-back launches for >= 0.25 s after warm-up; median
and min .. max of the five windows, and the ratio of the medians.  hits is trace plus 48 bytes per ray of stores (against 8) and
one material / texel round trip for the rays that hit.  Writes the figures, one JSON line under a few comment lines, to --out
(default profiles/r08_hit_records.txt) and prints the JSON line."""
import argparse
import gzip
import importlib.util
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qr_loader import load_package  # noqa: E402

qr = load_package()


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


rq = _tool("gpu_ray_query")             # timed, random_rays, golden; rays_mod and synth loaded once
rays_mod, synth, timed = rq.rays_mod, rq.synth, rq.timed


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def ab(fns, window, rounds=5):
    """{name: spread of the ms per window} with the candidates alternated: A B A B ..."""
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed(fn, window))
    return {k: spread(v) for k, v in out.items()}


def pair(scn, rays, window, coherent):
    r = torch.from_numpy(rays).cuda()
    d = ab({"hits": lambda: scn.hits(r, coherent=coherent), "trace": lambda: scn.trace(r, coherent=coherent)}, window)
    d["hits_ms_over_trace_ms"] = round(d["hits"]["median_ms"] / d["trace"]["median_ms"], 3)
    d["hits_grays_per_s"] = round(len(rays) / (d["hits"]["median_ms"] * 1e-3) / 1e9, 3)
    return d


def ray_figures(scn, rays, window, coherent_too=False):
    out = {"n_rays": len(rays), "incoherent": pair(scn, rays, window, False)}
    if coherent_too:
        out["coherent"] = pair(scn, rays, window, True)
    r = torch.from_numpy(rays).cuda()
    h = scn.hits(r)
    t, ids = scn.trace(r)
    torch.cuda.synchronize()
    _, ht, _, hid, _, _ = rays_mod.hit_fields(h)
    out["hit_fraction"] = round(float((ids >= 0).float().mean()), 4)
    out["t_and_id_equal_trace"] = bool((hid == ids).all()) and bool((ht.view(torch.int32) == t.view(torch.int32)).all())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_hit_records.txt"))
    args = ap.parse_args()
    res = {"version": qr.lib().qr_version().decode(), "kernel": "qr_hit_kernel", "device": torch.cuda.get_device_name(0),
           "window_s": args.window}

    blob = rq.golden("c2b_demo01_1080p")
    scn = qr.Scene(blob, ray_queries=True)
    res["demo1_1080p_camera"] = ray_figures(scn, rays_mod.camera_rays(blob), args.window, coherent_too=True)
    scn.set_depth(0)
    w, h = scn.width, scn.height
    views = torch.from_numpy(rays_mod.view_of(blob)[None]).cuda()
    frames = torch.empty((1, h, w), dtype=torch.int32, device="cuda")
    d = ab({"view_hits": lambda: scn.view_hits(views, w, h),
            "render_views_d0": lambda: scn.render_views(views, w, h, frames=frames)}, args.window)
    d["view_hits_ms_over_render_views_ms"] = round(d["view_hits"]["median_ms"] / d["render_views_d0"]["median_ms"], 3)
    d["n_pixels"] = w * h
    d["fsaa"] = int(scn.info.fsaa)
    res["demo1_1080p_views"] = d
    scn.close()

    blob = rq.golden("c3_demo02_1080p_gf_d3")
    scn = qr.Scene(blob, ray_queries=True)
    res["demo2_random_1m"] = ray_figures(scn, rq.random_rays(blob, args.rays, 1), args.window)
    scn.close()

    blob = qr.build_lists(synth.make_scene(shadow_lists=False, n_objects=10000, width=1920, height=1080, depth=4))
    scn = qr.Scene(blob, rebin_tiles=True, ray_queries=True)
    res["synth10k_random_1m"] = ray_figures(scn, rq.random_rays(blob, args.rays, 2), args.window)
    scn.close()

    line = json.dumps(res)
    head = [f"# tools/gpu_hit_records.py on one {res['device']} (build: {res['version']})",
            f"# HIP events around back-to-back launches, >= {args.window} s windows after warm-up, all in one process; each pair alternated",
            "# A B five times: median and min .. max of the five windows, ratio of the medians.  Not tuned: the first measurement of",
            "# these kernels.  hits = trace + 48 B per ray of stores (trace: 8 B) + one material / texel round trip per hit.",
            "# Kernel: qr_hit_kernel<VIEW, DIVK, COHERENT> -- caller rays <false,true,*>, views <true,DIVK,true> with DIVK chosen as",
            "# render_views chooses its instance; view_hits runs one lane per pixel (8x8 footprints) at every FSAA.",
            "# render_views_d0: render_views at depth 0 (the same first walk, then lights and shadow rays of one hit per sample)."]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(head) + "\n" + line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
