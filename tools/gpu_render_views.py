#!/usr/bin/env python3
"""Times of view rendering (Scene.render_views, include/qrhip.h qr_render_views_async) on the GPU box.

Workloads:
  demo1_1080p_own_d10 / _d0   demo scene 1, its own camera at 1920x1080, at depth 10 and 0: render_views next to
                              shade(coherent=True) of rays.camera_rays (the same rays through the ray API: same walk, same
                              shading, 32 B in and 12 B out per ray) and next to render() (tile lists instead of the global
                              list), alternated A/B/C five times; median and min .. max of each.  "views_within_shade_spread":
                              median(render_views) <= median(shade) + (max - min of the shade windows)
  demo1_2160p / demo1_270p    the same field of view at 3840x2160 and at 480x270, depth 10
  demo1_cube_6x1024           six 90-degree look_at views at 1024x1024 from the middle of the scene: one launch of six views next
                              to six launches of one view
  synth10k_1080p_d4           the synthetic 10 000-quadric scene, its own camera at 1920x1080, depth 4, next to shade and render()
Timing as tools/gpu_shade_rays.py: HIP events around back-to-back launches over a window of >= 0.25 s after warm-up, all in one
process.  Prints one JSON line (ms per launch, Grays/s = primary rays / time, the kernel name for a rocprofv3 --kernel-trace)."""
import argparse
import importlib.util
import json
import os
import statistics

import numpy as np
import torch

_spec = importlib.util.spec_from_file_location("gpu_ray_query", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                             "gpu_ray_query.py"))
grq = importlib.util.module_from_spec(_spec); _spec.loader.exec_module(grq)
qr, rays_mod, synth, golden, timed = grq.qr, grq.rays_mod, grq.synth, grq.golden, grq.timed


def resized(view, w0, h0, w, h):
    """the view that shows at w x h the field it shows at w0 x h0: same corner direction, pixel steps scaled"""
    v = view.copy()
    v[8:11] *= np.float32(w0 / w)
    v[12:15] *= np.float32(h0 / h)
    return v


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def abc(fns, window, rounds=5):
    """{name: [ms per window]} with the candidates alternated: A B C A B C ..."""
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed(fn, window))
    return out


def own_camera(scn, blob, window, ns):
    """render_views / shade(coherent) / render() of the snapshot's own camera at the scene's current depth"""
    w, h = scn.width, scn.height
    views = torch.from_numpy(rays_mod.view_of(blob)[None]).cuda()
    frames = torch.empty((1, h, w), dtype=torch.int32, device="cuda")
    cam = [torch.from_numpy(rays_mod.camera_rays(blob, k)).cuda() for k in range(ns)]
    f = scn.new_frame()

    def shade_all():
        for r in cam:
            scn.shade(r, coherent=True)

    t = abc({"render_views": lambda: scn.render_views(views, w, h, frames=frames), "shade_coherent": shade_all,
             "render": lambda: scn.render(f)}, window)
    d = {k: spread(v) for k, v in t.items()}
    sh = t["shade_coherent"]
    d["n_rays"] = w * h * ns
    d["depth"] = int(scn.info.depth)
    d["grays_per_s"] = round(w * h * ns / (d["render_views"]["median_ms"] * 1e-3) / 1e9, 3)
    d["views_ms_over_shade_ms"] = round(d["render_views"]["median_ms"] / d["shade_coherent"]["median_ms"], 3)
    d["views_ms_over_render_ms"] = round(d["render_views"]["median_ms"] / d["render"]["median_ms"], 3)
    d["views_within_shade_spread"] = bool(statistics.median(t["render_views"]) <= statistics.median(sh) + (max(sh) - min(sh)))
    torch.cuda.synchronize()
    same = bool((frames[0] == scn.render(f)).all())
    d["frame_equals_render"] = same          # tile lists against the global list: informative, equal for these scenes
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.25)
    args = ap.parse_args()
    res = {"version": qr.lib().qr_version().decode(), "kernel": "qr_render_views_kernel", "device": torch.cuda.get_device_name(0),
           "window_s": args.window}

    blob = golden("c2b_demo01_1080p")
    scn = qr.Scene(blob, ray_queries=True)
    ns = 1 << int(scn.info.fsaa)
    for depth in (10, 0):
        scn.set_depth(depth)
        res[f"demo1_1080p_own_d{depth}"] = own_camera(scn, blob, args.window, ns)
    scn.set_depth(10)
    own = rays_mod.view_of(blob)
    for tag, (w, h) in (("demo1_2160p", (3840, 2160)), ("demo1_270p", (480, 270))):
        v = torch.from_numpy(resized(own, scn.width, scn.height, w, h)[None]).cuda()
        fr = torch.empty((1, h, w), dtype=torch.int32, device="cuda")
        ms = [timed(lambda: scn.render_views(v, w, h, frames=fr), args.window) for _ in range(5)]
        res[tag] = dict(spread(ms), n_rays=w * h * ns, grays_per_s=round(w * h * ns / (statistics.median(ms) * 1e-3) / 1e9, 3))

    # a cube map from the middle of the scene's surfaces
    s = np.frombuffer(blob, dtype=np.int32, count=26)
    srf = np.frombuffer(blob, dtype=np.int32, count=int(s[4]) * 64, offset=int(s[11])).reshape(-1, 64)
    pos = srf[(srf[:, 37] >= 0) & (srf[:, 37] < 9), 0:3].view(np.float32).astype(np.float64)
    eye = (pos.min(axis=0) + pos.max(axis=0)) / 2
    faces = [((1, 0, 0), (0, 0, 1)), ((-1, 0, 0), (0, 0, 1)), ((0, 1, 0), (0, 0, 1)), ((0, -1, 0), (0, 0, 1)),
             ((0, 0, 1), (0, 1, 0)), ((0, 0, -1), (0, 1, 0))]
    n = 1024
    cube = torch.from_numpy(np.stack([rays_mod.look_at(eye, eye + np.float64(d), up, 90.0, n, n) for d, up in faces])).cuda()
    fr = torch.empty((6, n, n), dtype=torch.int32, device="cuda")

    def six_launches():
        for j in range(6):
            scn.render_views(cube[j:j + 1], n, n, frames=fr[j:j + 1])

    t = abc({"one_launch_of_six": lambda: scn.render_views(cube, n, n, frames=fr), "six_launches": six_launches}, args.window)
    _, ids = scn.render_views(cube, n, n, frames=fr, ids=True)
    torch.cuda.synchronize()
    res["demo1_cube_6x1024"] = dict({k: spread(v) for k, v in t.items()}, n_rays=6 * n * n * ns,
                                    hit_fraction=round(float((ids >= 0).float().mean()), 4))
    scn.close()

    blob = qr.build_lists(synth.make_scene(shadow_lists=False, n_objects=10000, width=1920, height=1080, depth=4))
    scn = qr.Scene(blob, rebin_tiles=True, ray_queries=True)
    res["synth10k_1080p_d4"] = own_camera(scn, blob, args.window, 1 << int(scn.info.fsaa))
    scn.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
