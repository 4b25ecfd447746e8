#!/usr/bin/env python3
"""Host cost of a call through the Python binding: on demo01_160, at the sizes of tests/_py_refusals.py
(64 rays, 2 views of 9x13, 4 directions; the image filters on those 2 frames), CALLS back-to-back calls of each method with one synchronise at the end, in
microseconds per call.  The kernels behind these sizes are tiny, so the figure is what the binding and the library's host
glue cost.

    python tools/time_py_glue.py [--calls 3000] [--binding FILE]

--binding: the __init__.py of another commit to time instead of the tree's (it loads the tree's libqrhip.so), so that two
bindings can be run alternately in one job.  Prints one JSON line: {"binding": ..., "us_per_call": {name: figure}}.
"""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_RAYS, N_VIEWS, WIDTH, HEIGHT, K_DIRS = 64, 2, 9, 13, 4


def load(binding):
    """the binding in FILE, or the tree's: both take the same way in, and both load the tree's library"""
    os.environ.setdefault("QR_LIB", os.path.join(ROOT, "quadray-engine_amd", "libqrhip.so"))
    path = os.path.abspath(binding or os.path.join(ROOT, "quadray-engine_amd", "__init__.py"))
    spec = importlib.util.spec_from_file_location("quadray_engine_amd", path, submodule_search_locations=[os.path.dirname(path)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["quadray_engine_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3000)
    ap.add_argument("--binding", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from conftest import load_blob
    qr = load(args.binding)
    from quadray_engine_amd import rays as R

    blob = load_blob("demo01_160")
    scn = qr.Scene(blob, ray_queries=True)
    dev = f"cuda:{scn.device}"
    cam = R.camera_rays(blob)
    pick = np.linspace(0, len(cam) - 1, N_RAYS).astype(np.int64)
    rays = torch.from_numpy(np.ascontiguousarray(cam[pick], dtype=np.float32)).to(dev)
    views = torch.from_numpy(np.stack([R.view_of(blob)] * N_VIEWS)).to(dev)
    dirs = torch.from_numpy(R.cosine_dirs(K_DIRS)).to(dev)
    pt_rays = scn.pt_rays(N_RAYS)
    adaptive = scn.pt_adaptive(N_RAYS, 1, 4, 0.01)
    index, count = adaptive.open_list()
    adaptive_views = scn.pt_adaptive_views(views, WIDTH, HEIGHT, 1, 4, 0.01)
    # the image filters: the frame's own hit records, a flat colour and variance, upsampling from factor 2, phase (0, 0)
    records = scn.view_hits(views, WIDTH, HEIGHT)
    colour = torch.full((N_VIEWS, HEIGHT, WIDTH, 3), 0.5, device=dev)
    variance = torch.full((N_VIEWS, HEIGHT, WIDTH), 0.25, device=dev)
    colour_lo, variance_lo = colour[:, ::2, ::2].contiguous(), variance[:, ::2, ::2].contiguous()
    prev = (views.clone(), records.clone(), torch.zeros((N_VIEWS, HEIGHT, WIDTH, 8), device=dev))
    temporal = scn.temporal(N_VIEWS, WIDTH, HEIGHT)

    calls = {
        "trace": lambda: scn.trace(rays),
        "hits": lambda: scn.hits(rays),
        "occlusion": lambda: scn.occlusion(rays, dirs, 1e-3),
        "gather": lambda: scn.gather(rays, dirs, 1e-3),
        "view_gather[frame]": lambda: scn.view_gather(views, dirs, WIDTH, HEIGHT, eps=1e-3, frame=True),
        "trace_layers": lambda: scn.trace_layers(rays, 4),
        "PtRays.step": lambda: pt_rays.step(rays),
        "PtAdaptive.step[list]": lambda: adaptive.step(rays, index=index, count=count),
        "PtAdaptiveViews.step[mean,counts,open]": lambda: adaptive_views.step(mean=True, counts=True, open=True),
        "atrous[variance]": lambda: scn.atrous(colour, records, variance),
        "denoise[2 passes]": lambda: scn.denoise(colour, records, variance, passes=2),
        "upsample[variance,weight]": lambda: scn.upsample(colour_lo, records, 2, variance=variance_lo, weight=True),
        "reproject[prev]": lambda: scn.reproject(colour, records, prev=prev, variance=variance),
        "Temporal.step": lambda: temporal.step(colour, records, views, variance),
    }
    out = {}
    for name, call in calls.items():
        for _ in range(50):
            call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call()
        torch.cuda.synchronize()
        out[name] = round((time.perf_counter() - t0) / args.calls * 1e6, 2)
    print(json.dumps({"binding": args.binding or "tree", "calls": args.calls, "us_per_call": out}))


if __name__ == "__main__":
    main()
