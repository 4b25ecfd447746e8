#!/usr/bin/env python3
"""Times of gather fans (Scene.view_gather, include/qrhip.h qr_gather_views_async) on the GPU box, next to the same answer
through the calls that existed before it:
  fused     Scene.view_gather(view, dirs, eps, reach, flip, cosine=True): one launch, 20 bytes per pixel written
  composed  Scene.view_hits -> rays.fan_rays in torch on the device -> Scene.shade -> the weighted sum in torch on the device, one
            float32 multiply and one float32 add per step as rays.gather_fold states them.  The K directions are taken 16 at a
            time (K = 64 at 1080p would hold 4 GB of rays at once); coherent=True is passed to shade() without flip, where
            neighbouring rays are neighbours, as the fused kernel chooses its walks.
Before anything is timed the two answers are compared: every word of the sums and every count must be equal.

Steps (each its own child process under its own `timeout`; after a step that fails nothing else is started):
  demo1_1080p_k16 / _k64      demo scene 1 from its own camera at 1920x1080, rays.sphere_dirs(16 / 64) with weights 1 / K, eps 1e-3,
                              reach 2
  synth10k_1080p_k16 / _k64   the synthetic 10 000-quadric scene (per-lane walks, a uniform grid), reach a tenth of its extent
  resources                   registers, spills, private segment and LDS of the five kernel instances, from the build's assembly
                              (no GPU)
each with flip off and on.  Timing as tools/gpu_fans.py: HIP events around back-to-back launches over a window of >= 0.25 s after
warm-up, the two candidates alternated in one process; median and min .. max.  The bytes are what each path must move by its
shapes (the scene image, read by both, is left out): fused 20 N written; composed 48 N written and read (hit records), 32 N K
written and read (rays), 12 N K written and read (colours), N K written and read (traced) and the 20 N of the sums read and
written once per chunk.
One JSON line per step.

usage: gpu_gather.py [--out FILE] [--window S] [--step NAME] [--rounds R]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = {"demo1_1080p_k16": 240, "demo1_1080p_k64": 300, "synth10k_1080p_k16": 300, "synth10k_1080p_k64": 420, "resources": 60}   # s
EPS = 1e-3


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def fold(torch, hits, dirs, col, traced, flip, acc, cnt):
    """rays.gather_fold's steps on device tensors, for a chunk of the table: acc float32 [N, 4] and cnt int32 [N] are updated"""
    nrm = hits[:, 4:7]
    for j in range(dirs.shape[0]):
        d = dirs[j]
        dot = (nrm[:, 0] * d[0] + nrm[:, 1] * d[1]) + nrm[:, 2] * d[2]
        wgt = d[3] * (torch.where(dot < 0, -dot, dot) if flip else dot)
        prod = col[:, j, :] * wgt[:, None]
        t = traced[:, j]
        acc[:, 0:3] = torch.where(t[:, None], acc[:, 0:3] + prod, acc[:, 0:3])
        acc[:, 3] = torch.where(t, acc[:, 3] + wgt, acc[:, 3])
        cnt += t.to(torch.int32)


def compare(grq, scn, view_np, w, h, k, reach, flip, window, rounds):
    import numpy as np
    import torch
    rays_mod, timed = grq.rays_mod, grq.timed
    vt = torch.from_numpy(view_np[None].copy()).cuda()
    table = np.concatenate([rays_mod.sphere_dirs(k), np.full((k, 1), 1.0 / k, dtype=np.float32)], axis=1)
    dirs = torch.from_numpy(table).cuda()
    n = w * h

    def fused():
        return scn.view_gather(vt, dirs, w, h, eps=EPS, reach=reach, flip=flip, cosine=True)

    def composed():
        hits = scn.view_hits(vt, w, h).reshape(n, 12)
        acc = torch.zeros((n, 4), dtype=torch.float32, device=hits.device)
        cnt = torch.zeros(n, dtype=torch.int32, device=hits.device)
        for c in range(0, k, 16):
            rays, traced = rays_mod.fan_rays(hits, dirs[c:c + 16], EPS, reach, flip)
            col = scn.shade(rays.reshape(-1, 8), coherent=not flip).reshape(n, -1, 3)
            fold(torch, hits, dirs[c:c + 16], col, traced, flip, acc, cnt)
        miss = rays_mod.hit_fields(hits)[3] < 0
        acc[miss] = 0.0
        cnt[miss] = -1
        return acc, cnt

    (ga, ca), (gb, cb) = fused(), composed()
    torch.cuda.synchronize()
    ga, ca = ga.reshape(n, 4), ca.reshape(n)
    if not (torch.equal(ca, cb) and torch.equal(ga.view(torch.int32), gb.view(torch.int32))):
        raise RuntimeError(f"fused and composed differ: {int((ca != cb).sum())} counts, "
                           f"{int((ga.view(torch.int32) != gb.view(torch.int32)).any(dim=1).sum())} rows of {n}")
    t = {"fused": [], "composed": []}
    for _ in range(rounds):
        t["fused"].append(timed(fused, window, warm=2))
        t["composed"].append(timed(composed, window, warm=1))
    d = {key: spread(v) for key, v in t.items()}
    hit = ca >= 0
    d["k"], d["flip"], d["pixels"], d["hit_fraction"] = k, bool(flip), n, round(float(hit.float().mean()), 4)
    d["traced_per_hit"] = round(float(ca[hit].float().mean()), 3) if bool(hit.any()) else None
    d["fused_bytes"] = 20 * n
    d["composed_bytes"] = 2 * 48 * n + 2 * 32 * n * k + 2 * 12 * n * k + 2 * n * k + 2 * 20 * n * ((k + 15) // 16)
    d["fan_grays_per_s_fused"] = round(n * k / (d["fused"]["median_ms"] * 1e-3) / 1e9, 3)      # directions, traced or not
    d["composed_ms_over_fused_ms"] = round(d["composed"]["median_ms"] / d["fused"]["median_ms"], 3)
    return d


def step(name, window, rounds):
    import importlib.util
    if name == "resources":
        spec = importlib.util.spec_from_file_location("check_kernel_resources", os.path.join(HERE, "check_kernel_resources.py"))
        m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
        asm = os.path.join(HERE, "..", "quadray-engine_amd", "csrc", "qr_device-hip-amdgcn-amd-amdhsa-gfx950.s")
        if not os.path.exists(asm):
            return {"assembly": "not on this machine: run this step where the library was built"}
        ks = [k for k in m.kernels(asm) if "qr_gather_kernel" in k["name"]]
        return {k["name"]: {a: k[a] for a in m.KEYS if a != "name"} for k in ks}
    import numpy as np
    import torch
    spec = importlib.util.spec_from_file_location("gpu_ray_query", os.path.join(HERE, "gpu_ray_query.py"))
    grq = importlib.util.module_from_spec(spec); spec.loader.exec_module(grq)
    qr, rays_mod = grq.qr, grq.rays_mod
    res = {"version": qr.lib().qr_version().decode(), "device": torch.cuda.get_device_name(0), "window_s": window, "eps": EPS}
    k = 64 if name.endswith("k64") else 16
    if name.startswith("demo1"):
        blob = grq.golden("c2b_demo01_1080p")
        scn = qr.Scene(blob, ray_queries=True)
        reach = 2.0
    else:
        blob = qr.build_lists(grq.synth.make_scene(shadow_lists=False, n_objects=10000, width=1920, height=1080, depth=4))
        scn = qr.Scene(blob, rebin_tiles=True, ray_queries=True)
        s = np.frombuffer(blob, dtype=np.int32, count=26)
        srf = np.frombuffer(blob, dtype=np.int32, count=int(s[4]) * 64, offset=int(s[11])).reshape(int(s[4]), 64)
        pos = srf[(srf[:, 37] >= 0) & (srf[:, 37] < 9), 0:3].view(np.float32).astype(np.float64)
        reach = float(np.float32(0.1 * np.max(pos.max(axis=0) - pos.min(axis=0))))
    res["reach"], res["depth"] = reach, scn.info.depth
    for flip in (False, True):
        res["flip" if flip else "noflip"] = compare(grq, scn, rays_mod.view_of(blob), scn.width, scn.height, k, reach, flip, window, rounds)
    scn.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--only", help="comma-separated steps to run instead of all")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.step:
        print(json.dumps({args.step: step(args.step, args.window, args.rounds)}), flush=True)
        return 0
    lines = []
    rc = 0
    for name, limit in STEPS.items():
        if args.only and name not in args.only.split(","):
            continue
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name,
                            "--window", str(args.window), "--rounds", str(args.rounds)], capture_output=True, text=True)
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
