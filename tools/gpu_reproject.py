#!/usr/bin/env python3
"""Times of temporal reprojection (Scene.reproject / Scene.temporal, include/qrhip.h qr_reproject_views_async) on the GPU box, next
to the same step as a composition of torch gathers and elementwise operations and to the bytes a launch must move.  Scenes are
those of tools/gpu_atrous.py: the snapshot's own camera at 1080p, here moved sideways by FRAC of a pixel's footprint at the
median depth per frame (and half of that upwards) over FRAMES frames.  Per scene:
  inputs        per frame SAMPLES adaptive samples (min = max = SAMPLES) with their variance(), and Scene.view_hits: each timed
  launch_ms     one qr_reproject_views_async launch of frame k against frame k - 1, outputs preallocated: device events around
                REPS launches, per launch; frame 0 is the first frame (no taps)
  bytes         what a launch must move by its shapes: hits 48, colour 12, variance 4 read and history 32, colour 12, variance 4
                written per pixel (the tap gathers are left to the caches); GB/s = bytes / time
  kept          the share of pixels whose history is longer than 1 after the frame, and the mean length
  torch_ms      the same step as torch gathers and elementwise operations with the same formulas in the same order, after the
                two were compared word for word on this input (torch_same; where they differ, how many words)
  step_ms       Temporal.step (the launch, its outputs' allocation and the 48 B per pixel it copies) and Scene.denoise after it,
                against the time of the samples per pixel the history stands for: (mean length - 1) x the time of one sample
Steps (each its own child process under its own `timeout`; after a step that fails nothing else is started):
  demo2_1080p   tests/golden/c3_demo02_1080p_gf_d3 with emission patched on (tests/_ptpatch.py)
  test18_1080p  tests/golden/pt/test18_1080p_pt (the reference's path-tracer scene)
One JSON line per step, then the kernels' resources from the build assembly.  A step that was not run is written as NOT MEASURED
with the reason.  No speed target is set: the comparison is against the composition, never against the kernel itself.

usage: gpu_reproject.py [--out FILE] [--step NAME]"""
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
FRAMES, SAMPLES, PASSES, REPS, FRAC = 8, 2, 5, 20, 0.37


def torch_clamp_box(torch, c, hit, flags, r, gamma):
    """rays.clamp_box in torch operations on the device: the box of every pixel from zero-padded shifted views, a row's partials
    first, then the rows folded"""
    n, h, w, ch = c.shape
    cp = torch.zeros((n, h + 2 * r, w + 2 * r, ch), dtype=c.dtype, device=c.device)
    cp[:, r:r + h, r:r + w] = c
    okp = torch.zeros((n, h + 2 * r, w + 2 * r), dtype=torch.bool, device=c.device)
    okp[:, r:r + h, r:r + w] = hit
    inf = torch.full_like(c, float("inf"))
    if flags & 2:
        t1, t2, cnt = torch.zeros_like(c), torch.zeros_like(c), torch.zeros((n, h, w), dtype=torch.int32, device=c.device)
    else:
        lo, hi = inf.clone(), -inf
    for j in range(2 * r + 1):
        if flags & 2:
            r1, r2 = torch.zeros_like(c), torch.zeros_like(c)
        else:
            rl, rh = inf.clone(), -inf
        for i in range(2 * r + 1):
            v, ok = cp[:, j:j + h, i:i + w], okp[:, j:j + h, i:i + w]
            if flags & 2:
                cnt = cnt + ok
                r1, r2 = torch.where(ok[..., None], r1 + v, r1), torch.where(ok[..., None], r2 + v * v, r2)
            else:
                rl, rh = torch.where(ok[..., None] & (v < rl), v, rl), torch.where(ok[..., None] & (rh < v), v, rh)
        if flags & 2:
            t1, t2 = t1 + r1, t2 + r2
        else:
            lo, hi = torch.where(rl < lo, rl, lo), torch.where(hi < rh, rh, hi)
    if flags & 2:
        nf = cnt.float()[..., None]
        mu = t1 / nf
        vv = t2 / nf - mu * mu
        wd = torch.sqrt(torch.where(vv > 0, vv, torch.zeros_like(vv))) * gamma
        lo, hi = mu - wd, mu + wd
    return lo, hi


def torch_reproject(torch, col, hits, var, prev, p, clamp=None):
    """rays.reproject_pass in torch operations on the device: one rounding per operation, the taps as gathers by index.  clamp: a
    rays.clamp_stops block; the result is then extended by the moved plane"""
    n, h, w, ch = col.shape
    f = lambda k: float(p[k])
    ids = hits.view(torch.int32)[..., 7]
    hit = ids >= 0
    pos, nrm, alb = hits[..., 0:3], hits[..., 4:7], hits[..., 8:11]
    c = torch.zeros((n, h, w, 4), dtype=col.dtype, device=col.device)
    c[..., :ch] = col
    if int(p["flags"]) & 1:
        a = torch.where(alb > f("alb_floor"), alb, torch.full_like(alb, f("alb_floor")))
        c[..., 0:3] = torch.where(hit[..., None], c[..., 0:3] / a, c[..., 0:3])
    lum = (c[..., 0] * 0.2126 + c[..., 1] * 0.7152) + c[..., 2] * 0.0722
    lum2 = lum * lum
    one, zero = torch.ones_like(lum), torch.zeros_like(lum)
    vfresh = var if var is not None else torch.full_like(lum, f("unknown"))
    hist = torch.zeros((n, h, w, 8), dtype=col.dtype, device=col.device)
    hist[..., 0:4], hist[..., 4], hist[..., 5], hist[..., 6] = c, lum, lum2, one
    if prev is None:
        return (hist, hist[..., 0:ch].contiguous(), vfresh.clone()) + (() if clamp is None else (-one,))
    views, hq_all, gq_all = prev
    v = views[:, None, None, :]
    org, d, hor, ver = v[..., 0:3], v[..., 4:7], v[..., 8:11], v[..., 12:15]
    cross = lambda a, b: torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                                      a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    A, B, C = cross(hor, ver), cross(ver, d), cross(d, hor)
    det = dot(d, A)
    e = pos - org
    den, nu, nv = dot(e, A), dot(e, B), dot(e, C)
    fx, fy = nu / den - f("off_x"), nv / den - f("off_y")
    front = (((den > 0) & (det > 0)) | ((den < 0) & (det < 0))) & hit
    window = front & (fx > -1.0) & (fx < float(w)) & (fy > -1.0) & (fy < float(h))
    x0, y0 = torch.floor(fx), torch.floor(fy)
    wx, wy = fx - x0, fy - y0
    ix, iy = torch.where(window, x0, zero).long(), torch.where(window, y0, zero).long()
    vi = torch.arange(n, device=col.device)[:, None, None]
    idq, nq, pq = hq_all.view(torch.int32)[..., 7], hq_all[..., 4:7], hq_all[..., 0:3]
    sw, s1, s2, sl = zero.clone(), zero.clone(), zero.clone(), zero.clone()
    sc = torch.zeros_like(c)
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = ix + i, iy + j
            b = (wx if i else one - wx) * (wy if j else one - wy)
            ok = window & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            qx, qy = qx.clamp(0, w - 1), qy.clamp(0, h - 1)
            g = gq_all[vi, qy, qx]
            ok = ok & (idq[vi, qy, qx] == ids) & (g[..., 6] >= 1.0) & (dot(nrm, nq[vi, qy, qx]) > f("normal_min"))
            ok = ok & (dot(nrm, pq[vi, qy, qx] - pos).abs() <= f("plane_max")) & (b > 0)
            sw = torch.where(ok, sw + b, sw)
            sc = torch.where(ok[..., None], sc + g[..., 0:4] * b[..., None], sc)
            s1 = torch.where(ok, s1 + g[..., 4] * b, s1)
            s2 = torch.where(ok, s2 + g[..., 5] * b, s2)
            sl = torch.where(ok, sl + g[..., 6] * b, sl)
    keep = window & (sw > f("min_weight"))
    ln = sl / sw + one
    ln = torch.where(ln < f("max_len"), ln, torch.full_like(ln, f("max_len")))
    hc, mv = sc / sw[..., None], None
    if clamp is not None:
        lo, hi = torch_clamp_box(torch, c, hit, int(clamp["flags"]), int(clamp["radius"]), float(clamp["gamma"]))
        h1 = torch.where(hc < lo, lo, hc)
        h2 = torch.where(hi < h1, hi, h1)
        d = (h2 - hc).abs()
        mv = zero.clone()
        for k in range(ch):
            mv = torch.where(d[..., k] > mv, d[..., k], mv)
        if int(clamp["flags"]) & 4:
            short = torch.full_like(ln, float(clamp["short_len"]))
            ln = torch.where(mv > 0, torch.where(ln < short, ln, short), ln)
        hc = h2
    al = one / ln
    ac = torch.where(al > f("alpha_min"), al, torch.full_like(al, f("alpha_min")))
    am = torch.where(al > f("alpha_mom_min"), al, torch.full_like(al, f("alpha_mom_min")))
    cb = hc * (one - ac)[..., None] + c * ac[..., None]
    m1 = (s1 / sw) * (one - am) + lum * am
    m2 = (s2 / sw) * (one - am) + lum2 * am
    vv = m2 - m1 * m1
    vv = torch.where(vv > 0, vv, zero)
    hist[..., 0:ch] = torch.where(keep[..., None], cb[..., 0:ch], c[..., 0:ch])
    hist[..., 4], hist[..., 5], hist[..., 6] = torch.where(keep, m1, lum), torch.where(keep, m2, lum2), torch.where(keep, ln, one)
    vout = torch.where(keep & (ln >= f("var_min_len")), vv, vfresh)
    return (hist, hist[..., 0:ch].contiguous(), vout) + (() if clamp is None else (torch.where(keep, mv, -one),))


def launch_bytes(n, h, w, ch, variance):
    """what one launch must move by its shapes: the record, the colour and the variance read, the entry, the colour and the
    variance written"""
    return n * h * w * (48 + 4 * ch + (4 if variance else 0) + 32 + 4 * ch + 4)


def scene_figures(grq, blob):
    import numpy as np
    import torch
    qr, rm = grq.qr, grq.rays_mod
    scn = qr.Scene(blob, ray_queries=True)
    scn.set_pt(False)
    w, h = scn.width, scn.height
    base = rm.view_of(blob)
    f, i = rm.frame_record(blob)
    off = (float(f[10]), float(f[14])) if i[30] else (0.0, 0.0)

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

    vt0 = torch.from_numpy(base[None].copy()).cuda()
    hits0 = scn.view_hits(vt0, w, h)
    t0 = hits0[..., 3][hits0.view(torch.int32)[..., 7] >= 0]
    depth = float(t0.median())
    pixel = float(np.linalg.norm(base[8:11])) * depth           # one pixel's footprint at the median depth, world units
    stops = dict(plane_max=pixel, off=off)
    res = {"width": w, "height": h, "fsaa": int(scn.info.fsaa), "frames": FRAMES, "samples_per_frame": SAMPLES, "reps": REPS,
           "median_depth": round(depth, 4), "pixel_footprint": round(pixel, 6), "shift_pixels_per_frame": [FRAC, FRAC / 2],
           "stops": {k: (list(v) if isinstance(v, tuple) else v) for k, v in stops.items()}}
    right, up = base[8:11] / np.linalg.norm(base[8:11]), -base[12:15] / np.linalg.norm(base[12:15])
    views = []
    for k in range(FRAMES):
        v = base.copy()
        v[0:3] = base[0:3] + (right * FRAC + up * (FRAC / 2)) * (pixel * k)
        views.append(v)
    frames = []
    for k, v in enumerate(views):
        vt = torch.from_numpy(v[None].copy()).cuda()
        acc = scn.pt_adaptive_views(vt, w, h, min_samples=SAMPLES, max_samples=SAMPLES, tol=0.0)
        if k == 0:
            def sample():
                acc.reset()
                return acc.step(SAMPLES, mean=True)
            res["samples_ms"] = events(sample)
            res["view_hits_ms"] = events(lambda: scn.view_hits(vt, w, h), 3)
            acc.reset()
        _, mean = acc.step(SAMPLES, mean=True)
        frames.append((vt, mean, acc.variance(), scn.view_hits(vt, w, h)))
    p = rm.reproject_stops(**stops)
    nbytes = launch_bytes(1, h, w, 3, True)
    res["launch_bytes"] = nbytes
    per, gbs, kept, length, tor, same = [], [], [], [], [], []
    hist = [torch.empty((1, h, w, 8), dtype=torch.float32, device="cuda") for _ in range(2)]
    cout, vout = torch.empty_like(frames[0][1]), torch.empty_like(frames[0][2])
    prev = None
    for k, (vt, mean, var, hits) in enumerate(frames):
        out = hist[k & 1]
        call = lambda: scn.reproject(mean, hits, prev, var, out=out, colour_out=cout, variance_out=vout, **stops)
        per.append(events(call, REPS))
        gbs.append(round(nbytes / per[-1] / 1e6, 1))
        th, tc, tv = torch_reproject(torch, mean, hits, var, prev, p)
        call()
        torch.cuda.synchronize()
        pairs = ((th, out), (tc, cout), (tv, vout))
        differ = sum(int((a.view(torch.int32) != b.view(torch.int32)).sum()) for a, b in pairs)
        same.append(differ == 0 or {"words_differing": differ, "of": sum(a.numel() for a, _ in pairs)})
        tor.append(events(lambda: torch_reproject(torch, mean, hits, var, prev, p), 2))
        kept.append(round(float((out[..., 6] > 1).float().mean()), 4))
        length.append(round(float(out[..., 6].mean()), 3))
        prev = (vt, hits, out)
    res["launch_ms"], res["launch_GB_per_s"], res["kept"], res["mean_length"] = per, gbs, kept, length
    res["torch_ms"], res["torch_same"] = tor, same
    res["torch_ms_over_launch_ms"] = [round(a / b, 1) for a, b in zip(tor, per)]
    # the accumulator and the filter after it, against the samples the history stands for
    extent = float((hits0[..., 0:3][hits0.view(torch.int32)[..., 7] >= 0].max(0).values
                    - hits0[..., 0:3][hits0.view(torch.int32)[..., 7] >= 0].min(0).values).max())
    dstops = dict(normal_power=128, luma=4.0, plane=extent / 500)

    def chain(denoise):
        acc = scn.temporal(1, w, h, 3, **stops)
        for vt, mean, var, hits in frames:
            c, v = acc.step(mean, hits, vt, var)
            if denoise:
                c, v = scn.denoise(c, hits, v, passes=PASSES, albedo=True, **dstops)
        return c
    res["temporal_8_frames_ms"] = events(lambda: chain(False))
    res["temporal_and_denoise_8_frames_ms"] = events(lambda: chain(True))
    res["temporal_step_ms"] = round(res["temporal_8_frames_ms"] / FRAMES, 4)
    res["temporal_step_and_denoise_ms"] = round(res["temporal_and_denoise_8_frames_ms"] / FRAMES, 4)
    res["one_sample_ms"] = round(res["samples_ms"] / SAMPLES, 4)
    res["samples_replaced_ms"] = round((length[-1] - 1.0) * res["samples_ms"], 3)     # a history entry is one frame of SAMPLES samples
    noisy, clean = frames[-1][1], chain(True)
    res["std_noisy_accumulated_denoised"] = [round(float(noisy.std()), 5), round(float(chain(False).std()), 5), round(float(clean.std()), 5)]
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
    return {"resources": {k["name"]: {a: k[a] for a in ck.KEYS if a != "name"} for k in ck.kernels(asm) if "qr_reproject_kernel" in k["name"]}}


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
    names = list(STEPS)
    for k, name in enumerate(names):
        r = subprocess.run(["timeout", "-k", "10", str(STEPS[name]), sys.executable, os.path.abspath(__file__), "--step", name],
                           capture_output=True, text=True)
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not out:
            lines.append(f"# step {name} failed with status {r.returncode}: nothing after it was started\n# " +
                         r.stderr[-2000:].replace("\n", "\n# "))
            lines += [f"# {later}: NOT MEASURED (the step {name} before it failed)" for later in names[k + 1:]]
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
        print("\n".join(lines[-len(names):]), file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
