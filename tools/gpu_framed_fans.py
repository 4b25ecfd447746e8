#!/usr/bin/env python3
"""Times of the framed fans (frame=True, spin= on Scene.view_occlusion and Scene.view_gather; include/qrhip.h
qr_fan_views_framed_async, qr_gather_views_framed_async) on the GPU box.  For the occlusion fan and for the gather fan, four
candidates at the same K, alternated in one process:
  framed       rays.cosine_dirs(K) in every pixel's own frame, no flip, no spin: every direction of a hit is traced
  framed_spin  the same with a spin plane rays.spins((1, H, W), 1): every pixel turns the table about its normal
  unframed     what the same K gives today: rays.sphere_dirs(K), weights 1 / K, flip=True (cosine=True for the gather)
  composed     the answer of framed_spin through the calls that existed before it: Scene.view_hits -> rays.fan_rays(frame=True,
               spin=) in torch on the device -> Scene.occluded / Scene.shade -> the count or the weighted sum in torch on the
               device (rays.gather_fold's steps: one float32 multiply and one float32 add each), the K directions 16 at a time
Before the composition is timed its answer is compared with framed_spin's: every count, every mask-free open number and every
word of the sums must be equal.  If they are not, the step says so, times the three launches and leaves the composition out.

Steps (each its own child process under its own `timeout`, all candidates of a step in that one process; after a step that fails
nothing else is started):
  demo1_1080p_k16 / _k64      demo scene 1 from its own camera at 1920x1080, eps 1e-3, reach 2
  synth10k_1080p_k16 / _k64   the synthetic 10 000-quadric scene (per-lane walks, a uniform grid), reach a tenth of its extent
  resources                   registers, spills, private segment and LDS of the ten framed kernel instances, from the build's
                              assembly (no GPU)
the settings of tools/gpu_gather.py (profiles/r17_gather_fans.txt).  Timing as there: HIP events around back-to-back launches
over a window of >= 0.25 s after warm-up; median and min .. max over the rounds.
One JSON line per step.

usage: gpu_framed_fans.py [--out FILE] [--window S] [--step NAME] [--only A,B] [--rounds R]"""
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


def compare(grq, scn, view_np, w, h, k, reach, window, rounds):
    import numpy as np
    import torch
    rays_mod, timed = grq.rays_mod, grq.timed
    vt = torch.from_numpy(view_np[None].copy()).cuda()
    cos_t = torch.from_numpy(rays_mod.cosine_dirs(k)).cuda()
    sph_t = torch.from_numpy(np.concatenate([rays_mod.sphere_dirs(k), np.full((k, 1), 1.0 / k, dtype=np.float32)], axis=1)).cuda()
    spin = torch.from_numpy(rays_mod.spins((1, h, w), 1)).cuda()
    n = w * h
    kw = dict(eps=EPS, reach=reach)

    def hits_and_rays(c):
        hits = scn.view_hits(vt, w, h).reshape(n, 12)
        rays, traced = rays_mod.fan_rays(hits, cos_t[c:c + 16], EPS, reach, False, frame=True, spin=spin.reshape(n, 2))
        return hits, rays, traced

    def occ_composed():
        total = torch.zeros(n, dtype=torch.int32, device=vt.device)
        for c in range(0, k, 16):
            hits, rays, traced = hits_and_rays(c)
            occ = scn.occluded(rays.reshape(-1, 8)).reshape(traced.shape)
            total += (traced & ~occ).sum(dim=1, dtype=torch.int32)
        hid = rays_mod.hit_fields(hits)[3]
        return torch.where(hid >= 0, total, torch.full_like(total, -1))

    def gat_composed():
        acc = torch.zeros((n, 4), dtype=torch.float32, device=vt.device)
        cnt = torch.zeros(n, dtype=torch.int32, device=vt.device)
        for c in range(0, k, 16):
            hits, rays, traced = hits_and_rays(c)
            col = scn.shade(rays.reshape(-1, 8)).reshape(n, -1, 3)
            for j in range(traced.shape[1]):
                wgt = cos_t[c + j, 3]
                t = traced[:, j]
                acc[:, 0:3] = torch.where(t[:, None], acc[:, 0:3] + col[:, j, :] * wgt, acc[:, 0:3])
                acc[:, 3] = torch.where(t, acc[:, 3] + wgt, acc[:, 3])
                cnt += t.to(torch.int32)
        miss = rays_mod.hit_fields(hits)[3] < 0
        acc[miss] = 0.0
        cnt[miss] = -1
        return acc, cnt

    cand = {
        "occlusion": {
            "framed": lambda: scn.view_occlusion(vt, cos_t, w, h, frame=True, **kw),
            "framed_spin": lambda: scn.view_occlusion(vt, cos_t, w, h, frame=True, spin=spin, **kw),
            "unframed": lambda: scn.view_occlusion(vt, sph_t, w, h, flip=True, **kw),
            "composed": occ_composed,
        },
        "gather": {
            "framed": lambda: scn.view_gather(vt, cos_t, w, h, frame=True, **kw),
            "framed_spin": lambda: scn.view_gather(vt, cos_t, w, h, frame=True, spin=spin, **kw),
            "unframed": lambda: scn.view_gather(vt, sph_t, w, h, flip=True, cosine=True, **kw),
            "composed": gat_composed,
        },
    }
    out = {"k": k, "pixels": n}
    # the composition must give framed_spin's bits before it is timed
    a, b = cand["occlusion"]["framed_spin"]().reshape(n), occ_composed()
    (ga, ca), (gb, cb) = cand["gather"]["framed_spin"](), gat_composed()
    torch.cuda.synchronize()
    ga, ca = ga.reshape(n, 4), ca.reshape(n)
    bad = {"occlusion": int((a != b).sum()),
           "gather": int((ca != cb).sum()) + int((ga.view(torch.int32) != gb.view(torch.int32)).any(dim=1).sum())}
    hit = ca >= 0
    out["hit_fraction"] = round(float(hit.float().mean()), 4)
    out["traced_per_hit"] = round(float(ca[hit].float().mean()), 3) if bool(hit.any()) else None
    out["open_per_hit"] = round(float(a[hit].float().mean()), 3) if bool(hit.any()) else None
    for fan, fns in cand.items():
        names = [key for key in fns if key != "composed" or bad[fan] == 0]
        t = {key: [] for key in names}
        for _ in range(rounds):
            for key in names:
                t[key].append(timed(fns[key], window, warm=1 if key == "composed" else 2))
        d = {key: spread(v) for key, v in t.items()}
        if bad[fan]:
            d["composed"] = f"NOT TIMED: differs from framed_spin in {bad[fan]} elements"
        else:
            d["composed_ms_over_framed_spin_ms"] = round(d["composed"]["median_ms"] / d["framed_spin"]["median_ms"], 3)
        d["framed_spin_ms_over_framed_ms"] = round(d["framed_spin"]["median_ms"] / d["framed"]["median_ms"], 3)
        d["framed_ms_over_unframed_ms"] = round(d["framed"]["median_ms"] / d["unframed"]["median_ms"], 3)
        out[fan] = d
    return out


def step(name, window, rounds):
    import importlib.util
    if name == "resources":
        spec = importlib.util.spec_from_file_location("check_kernel_resources", os.path.join(HERE, "check_kernel_resources.py"))
        m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
        asm = os.path.join(HERE, "..", "quadray-engine_amd", "csrc", "qr_device-hip-amdgcn-amd-amdhsa-gfx950.s")
        if not os.path.exists(asm):
            return {"assembly": "not on this machine: run this step where the library was built"}
        ks = [k for k in m.kernels(asm) if "_framed_kernel" in k["name"]]
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
    res.update(compare(grq, scn, rays_mod.view_of(blob), scn.width, scn.height, k, reach, window, rounds))
    scn.close()
    return res


def save(path, lines):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


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
        save(args.out, lines)                   # after every step: a run that is cut short keeps what it measured
    save(args.out, lines)
    if rc:
        print(lines[-1], file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
