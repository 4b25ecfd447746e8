#!/usr/bin/env python3
"""Times of hit layers (Scene.trace_layers / Scene.view_layers, include/qrhip.h qr_layer_rays_async / qr_layer_views_async) on the
GPU box, next to the same answer through the calls that existed before them:
  fused     Scene.trace_layers(rays, k, coherent): one launch; the rays are read once, 4 N + 8 k N bytes written
  composed  k times Scene.trace on a working copy of the rays, and between the launches the device-side tmin update of
            rays.next_rays, in place (torch.where on the tmin column); before the first launch the column is set back to the
            rays' own tmin.  No result planes are gathered: every launch writes its own t and ids.
Before anything is timed the two answers are compared: every t (as bits) and every id of every layer must be equal.
Views: Scene.view_layers(view, k) with t and ids, and with hit records too, next to Scene.view_hits (one layer, records).

Steps (each its own child process under its own `timeout`; after a step that fails nothing else is started):
  demo1_1080p      demo scene 1, the camera rays of its own 1920x1080 frame, k = 4 and 8, with and without `coherent`
  synth10k_1080p   the synthetic 10 000-quadric scene (per-lane walks, a uniform grid), the same
  resources        registers, spills and private segment of the four kernel instances, from the build's assembly (no GPU)
Timing as tools/gpu_fans.py: HIP events around back-to-back launches over a window of >= 0.25 s after warm-up, the candidates
alternated three times in one process; median and min .. max.  One JSON line per step.

usage: gpu_layers.py [--out FILE] [--window S] [--step NAME]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = {"demo1_1080p": 300, "synth10k_1080p": 420, "resources": 60}   # s
KS = (4, 8)


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def compare_rays(grq, scn, rays, k, coherent, window, rounds=3):
    import torch
    timed = grq.timed
    n = rays.shape[0]
    work = rays.clone()
    tmin0 = rays[:, 3].clone()
    tmax = rays[:, 7]
    flt_max = torch.finfo(torch.float32).max
    end = torch.where(tmax > flt_max, torch.full_like(tmax, flt_max), tmax)

    def fused():
        return scn.trace_layers(rays, k, coherent=coherent)

    def composed():
        work[:, 3] = tmin0
        out = []
        for _ in range(k):
            t, ids = scn.trace(work, coherent=coherent)
            work[:, 3] = torch.where(ids >= 0, t, end)
            out.append((t, ids))
        return out

    cnt, t, ids = fused()
    parts = composed()
    torch.cuda.synchronize()
    ct = torch.stack([p[0] for p in parts]).view(torch.int32)
    ci = torch.stack([p[1] for p in parts])
    if not (torch.equal(ct, t.view(torch.int32)) and torch.equal(ci, ids)):
        raise RuntimeError(f"fused and composed layers differ in {int((ct != t.view(torch.int32)).sum())} t and {int((ci != ids).sum())} ids")
    tm = {"fused": [], "composed": []}
    for _ in range(rounds):
        tm["fused"].append(timed(fused, window, warm=2))
        tm["composed"].append(timed(composed, window, warm=2))
    d = {key: spread(v) for key, v in tm.items()}
    d["k"], d["coherent"], d["rays"] = k, bool(coherent), n
    d["hits_per_ray"] = round(float(cnt.float().mean()), 3)
    d["rays_at_k"] = round(float((cnt == k).float().mean()), 4)
    d["walks_fused"] = int(torch.clamp(cnt + 1, max=k).sum())           # lanes that walk: every hit and the first miss
    d["fused_bytes"] = 32 * n + 4 * n + 8 * k * n
    d["composed_bytes"] = k * (32 * n + 8 * n) + (k + 1) * 4 * n + k * 12 * n      # launches; tmin writes; the update's reads
    d["composed_ms_over_fused_ms"] = round(d["composed"]["median_ms"] / d["fused"]["median_ms"], 3)
    return d


def compare_views(grq, scn, view_np, w, h, window, rounds=3):
    import torch
    timed = grq.timed
    vt = torch.from_numpy(view_np[None].copy()).cuda()
    cands = {"view_hits": lambda: scn.view_hits(vt, w, h)}
    for k in KS:
        cands[f"view_layers_k{k}"] = (lambda k=k: scn.view_layers(vt, k, w, h))
        cands[f"view_layers_k{k}_records"] = (lambda k=k: scn.view_layers(vt, k, w, h, hits=True))
    vh = scn.view_hits(vt, w, h)
    lay = scn.view_layers(vt, KS[0], w, h, hits=True)
    torch.cuda.synchronize()
    if not torch.equal(lay[3][0].view(torch.int32), vh.view(torch.int32)):
        raise RuntimeError("layer 0 of view_layers is not view_hits")
    tm = {key: [] for key in cands}
    for _ in range(rounds):
        for key, fn in cands.items():
            tm[key].append(timed(fn, window, warm=2))
    d = {key: spread(v) for key, v in tm.items()}
    d["pixels"] = w * h
    for k in KS:
        d[f"view_layers_k{k}_ms_over_view_hits_ms"] = round(d[f"view_layers_k{k}"]["median_ms"] / d["view_hits"]["median_ms"], 3)
        d[f"view_layers_k{k}_records_ms_over_view_hits_ms"] = round(d[f"view_layers_k{k}_records"]["median_ms"] / d["view_hits"]["median_ms"], 3)
    return d


def step(name, window):
    import importlib.util
    if name == "resources":
        spec = importlib.util.spec_from_file_location("check_kernel_resources", os.path.join(HERE, "check_kernel_resources.py"))
        m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
        asm = os.path.join(HERE, "..", "quadray-engine_amd", "csrc", "qr_device-hip-amdgcn-amd-amdhsa-gfx950.s")
        if not os.path.exists(asm):
            return {"assembly": "not on this machine: run this step where the library was built"}
        ks = [k for k in m.kernels(asm) if "qr_layer_kernel" in k["name"]]
        return {k["name"]: {a: k[a] for a in m.KEYS if a != "name"} for k in ks}
    import torch
    spec = importlib.util.spec_from_file_location("gpu_ray_query", os.path.join(HERE, "gpu_ray_query.py"))
    grq = importlib.util.module_from_spec(spec); spec.loader.exec_module(grq)
    qr, rays_mod = grq.qr, grq.rays_mod
    res = {"version": qr.lib().qr_version().decode(), "device": torch.cuda.get_device_name(0), "window_s": window}
    if name.startswith("demo1"):
        blob = grq.golden("c2b_demo01_1080p")
        scn = qr.Scene(blob, ray_queries=True)
    else:
        blob = qr.build_lists(grq.synth.make_scene(shadow_lists=False, n_objects=10000, width=1920, height=1080, depth=4))
        scn = qr.Scene(blob, rebin_tiles=True, ray_queries=True)
    rays = torch.from_numpy(rays_mod.camera_rays(blob)).cuda()
    for k in KS:
        for coherent in (True, False):
            res[f"rays_k{k}_{'coherent' if coherent else 'incoherent'}"] = compare_rays(grq, scn, rays, k, coherent, window)
    res["views"] = compare_views(grq, scn, rays_mod.view_of(blob), scn.width, scn.height, window)
    scn.close()
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
