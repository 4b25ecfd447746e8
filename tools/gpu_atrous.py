#!/usr/bin/env python3
"""Times of the guided a-trous filter (Scene.atrous / Scene.denoise, include/qrhip.h qr_atrous_views_async) on the GPU box, next to
the same passes as a composition of torch operations and to the bytes a pass must move.  Scenes and camera are those of
tools/gpu_pt_adaptive_views.py and profiles/r14_pt_adaptive.txt: the snapshot's own camera at 1080p.  Per scene:
  inputs      8 adaptive samples (min = max = 8), then PtAdaptiveViews.variance, Scene.view_hits: each timed
  pass_ms     one pass at step 1, 2, 4, 8, 16 with all three stops (at 64 too; and, at steps 1, 16 and 64, without any), the inputs being those
              the denoiser feeds that pass: device events around REPS launches, per launch
  bytes       what a pass must move by its shapes: colour and variance read and written once, the records read once
              (nrm + id always, pos with the plane stop: 16 B each); GB/s = bytes / time: how far a pass is from HBM bandwidth
  denoise_ms  the whole Scene.denoise, 5 passes, scratch allocation included
  torch_ms    the same passes as shifted slices and elementwise torch operations with the same formulas in the same order, after
              the two were compared word for word on this input (torch_same: per pass, are all words the same)
Steps (each its own child process under its own `timeout`; after a step that fails nothing else is started):
  demo2_1080p   tests/golden/c3_demo02_1080p_gf_d3 with emission patched on (tests/_ptpatch.py)
  test18_1080p  tests/golden/pt/test18_1080p_pt (the reference's path-tracer scene)
One JSON line per step, then the kernels' resources from the build assembly.

usage: gpu_atrous.py [--out FILE] [--step NAME]"""
import argparse
import gzip
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STEPS = {"demo2_1080p": 300, "test18_1080p": 300}   # s
SAMPLES, PASSES, REPS = 8, 5, 20
STOPS = dict(normal_power=128, luma=4.0, luma_eps=1e-6)          # plane: a 500th of the scene's extent, set per scene


def torch_pass(torch, col, var, hits, step, stops):
    """rays.atrous_pass in torch operations on the device: one rounding per operation, the taps as shifted slices of padded planes"""
    import torch.nn.functional as Fn
    flags, nsq, sz, sl2, el, af = (int(stops[0]), int(stops[1])) + tuple(float(x) for x in stops[2:])
    n, h, w, ch = col.shape
    ids = hits.view(torch.int32)[..., 7]
    hit = ids >= 0
    pos, nrm, alb = hits[..., 0:3], hits[..., 4:7], hits[..., 8:11]
    a = torch.where(alb > af, alb, torch.full_like(alb, af))
    a = torch.where(hit[..., None], a, torch.ones_like(a))
    c = col.clone()
    if flags & 8:
        c[..., 0:3] = c[..., 0:3] / a
    lum = (c[..., 0] * 0.2126 + c[..., 1] * 0.7152) + c[..., 2] * 0.0722
    v = torch.ones_like(lum) if var is None else var
    den = sl2 * v + el
    P = 2 * step
    pad3 = lambda t, val=0.0: Fn.pad(t, (P, P, P, P), value=val)
    pad4 = lambda t: Fn.pad(t, (0, 0, P, P, P, P))
    cP, lP, vP, nP, pP, iP = pad4(c), pad3(lum), pad3(v), pad4(nrm), pad4(pos), pad3(ids, -1)
    H = [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16]
    sc, sw, sv = torch.zeros_like(c), torch.zeros_like(lum), torch.zeros_like(lum)
    zero, sz_t = torch.zeros_like(lum), torch.full_like(lum, sz)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ys, xs = slice(P + dy * step, P + dy * step + h), slice(P + dx * step, P + dx * step + w)
            wt = torch.full_like(lum, H[dy + 2] * H[dx + 2])
            if dx == 0 and dy == 0:
                take = torch.ones_like(hit)
            else:
                ok = iP[:, ys, xs] >= 0
                if flags & 1:
                    nq = nP[:, ys, xs]
                    d = (nrm[..., 0] * nq[..., 0] + nrm[..., 1] * nq[..., 1]) + nrm[..., 2] * nq[..., 2]
                    d = torch.where(d > 0, d, zero)
                    for _ in range(nsq):
                        d = d * d
                    wt = wt * d
                if flags & 2:
                    e = pP[:, ys, xs] - pos
                    d = (nrm[..., 0] * e[..., 0] + nrm[..., 1] * e[..., 1]) + nrm[..., 2] * e[..., 2]
                    x = d.abs() / sz_t          # by a tensor: torch divides by a Python scalar through its reciprocal on the device
                    wt = wt * (1.0 / (1.0 + x * x))
                if flags & 4:
                    dl = lum - lP[:, ys, xs]
                    wt = wt * (1.0 / (1.0 + (dl * dl) / den))
                take = ok & (wt > 0)
            wt = torch.where(take, wt, zero)
            sc = torch.where(take[..., None], sc + cP[:, ys, xs] * wt[..., None], sc)
            sw = torch.where(take, sw + wt, sw)
            sv = torch.where(take, sv + vP[:, ys, xs] * (wt * wt), sv)
    out = sc / sw[..., None]
    vout = sv / (sw * sw)
    if flags & 16:
        out[..., 0:3] = out[..., 0:3] * a
    out = torch.where(hit[..., None], out, c)
    return out, (None if var is None else torch.where(hit, vout, var))


def pass_bytes(n, h, w, ch, variance, flags):
    """what one pass must move by its shapes: colour (+ variance) in and out, nrm + id of every record, pos with the plane stop,
    alb with de/modulation"""
    px = n * h * w
    rec = 16 + (16 if flags & 2 else 0) + (16 if flags & (8 | 16) else 0)
    return px * (2 * 4 * ch + (8 if variance else 0) + rec)


def scene_figures(grq, blob):
    import numpy as np
    import torch
    qr, rm = grq.qr, grq.rays_mod
    scn = qr.Scene(blob, ray_queries=True)
    scn.set_pt(False)
    w, h = scn.width, scn.height
    vt = torch.from_numpy(rm.view_of(blob)[None].copy()).cuda()

    def events(fn, reps=1):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b) / reps)
        return round(statistics.median(ms), 4)

    acc = scn.pt_adaptive_views(vt, w, h, min_samples=SAMPLES, max_samples=SAMPLES, tol=0.0)

    def sample():
        acc.reset()
        return acc.step(SAMPLES, mean=True)
    res = {"width": w, "height": h, "fsaa": int(scn.info.fsaa), "samples": SAMPLES, "passes": PASSES, "reps": REPS}
    res["adaptive_8_samples_ms"] = events(sample)
    _, mean = sample()
    var = acc.variance()
    hits = scn.view_hits(vt, w, h)
    res["variance_ms"] = events(lambda: acc.variance(out=var), REPS)
    res["view_hits_ms"] = events(lambda: scn.view_hits(vt, w, h), 3)
    ids = hits.view(torch.int32)[..., 7]
    pos = hits[..., 0:3][ids >= 0]
    extent = float((pos.max(0).values - pos.min(0).values).max())
    stops = dict(STOPS, plane=extent / 500)
    res["stops"] = stops
    res["misses"] = int((ids < 0).sum())
    flags_all = rm.atrous_stops(**stops)
    flags_none = rm.atrous_stops(normal_power=None)
    res["denoise_ms"] = events(lambda: scn.denoise(mean, hits, var, passes=PASSES, **stops), 5)
    res["std_in_out"] = [round(float(mean.std()), 5), round(float(scn.denoise(mean, hits, var, passes=PASSES, **stops)[0].std()), 5)]
    # per pass, on the inputs the denoiser feeds it
    c, v = mean, var
    per, tor, same, gbs, nbytes = {}, {}, {}, {}, {}
    out, vout = torch.empty_like(mean), torch.empty_like(var)
    for k in range(PASSES):
        step = 1 << k
        kw = dict(step=step, out=out, variance_out=vout, **stops)
        per[step] = events(lambda: scn.atrous(c, hits, v, **kw), REPS)
        nbytes[step] = pass_bytes(1, h, w, 3, True, flags_all[0])
        gbs[step] = round(nbytes[step] / per[step] / 1e6, 1)
        tc, tv = torch_pass(torch, c, v, hits, step, flags_all)
        kc, kv = scn.atrous(c, hits, v, step=step, **stops)
        torch.cuda.synchronize()
        same[step] = bool(torch.equal(tc.view(torch.int32), kc.view(torch.int32)) and torch.equal(tv.view(torch.int32), kv.view(torch.int32)))
        if not same[step]:
            same[f"{step}_words_differing"] = int((tc.view(torch.int32) != kc.view(torch.int32)).sum()) + int((tv.view(torch.int32) != kv.view(torch.int32)).sum())
        tor[step] = events(lambda: torch_pass(torch, c, v, hits, step, flags_all), 2)
        c, v = kc, kv
    res["pass_ms"], res["pass_bytes"], res["pass_GB_per_s"], res["torch_ms"], res["torch_same"] = per, nbytes, gbs, tor, same
    res["torch_ms_over_pass_ms"] = {s: round(tor[s] / per[s], 1) for s in per}
    res["denoise_torch_ms"] = round(sum(tor.values()), 3)
    bare = {}
    for step in (1, 16, 64):
        ms = events(lambda: scn.atrous(mean, hits, var, step=step, normal_power=None, out=out, variance_out=vout), REPS)
        b = pass_bytes(1, h, w, 3, True, flags_none[0])
        bare[step] = {"ms": ms, "bytes": b, "GB_per_s": round(b / ms / 1e6, 1)}
    res["pass_without_stops"] = bare
    res["pass_ms_step_64_all_stops"] = events(lambda: scn.atrous(mean, hits, var, step=64, out=out, variance_out=vout, **stops), REPS)
    scn.close()
    return res


def step(name):
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("gpu_ray_query", os.path.join(HERE, "gpu_ray_query.py"))
    grq = importlib.util.module_from_spec(spec); spec.loader.exec_module(grq)
    res = {"version": grq.qr.lib().qr_version().decode(), "device": torch.cuda.get_device_name(0)}
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _ptpatch
    if name == "test18_1080p":
        blob = gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "pt", "test18_1080p_pt.qrs.gz"), "rb").read())
    else:
        blob = _ptpatch.pt_patch(grq.golden("c3_demo02_1080p_gf_d3"))
    res.update(scene_figures(grq, blob))
    return res


def resources():
    sys.path.insert(0, HERE)
    import check_kernel_resources as ck
    asm = os.path.join(ROOT, "quadray-engine_amd", "csrc", "qr_device-hip-amdgcn-amd-amdhsa-gfx950.s")
    if not os.path.exists(asm):
        return {"resources": "no build assembly in this tree"}
    return {"resources": {k["name"]: {a: k[a] for a in ck.KEYS if a != "name"} for k in ck.kernels(asm)
                          if "qr_atrous_kernel" in k["name"] or "qr_pt_adapt_var_kernel" in k["name"]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.step:
        print(json.dumps({args.step: step(args.step)}), flush=True)
        return 0
    lines = []
    rc = 0
    for name, limit in STEPS.items():
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           capture_output=True, text=True)
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not out:
            lines.append(f"# step {name} failed with status {r.returncode}: nothing after it was started\n# " +
                         r.stderr[-2000:].replace("\n", "\n# "))
            rc = 1
            break
        lines.append(out[-1])
        print(out[-1], flush=True)
    if rc == 0:
        lines.append(json.dumps(resources()))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if rc:
        print(lines[-1], file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
