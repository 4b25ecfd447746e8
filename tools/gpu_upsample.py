#!/usr/bin/env python3
"""Times of guided upsampling (Scene.upsample, include/qrhip.h qr_upsample_views_async) on the GPU box, next to the bytes a launch
must move, to the same step as a composition of torch gathers and elementwise operations, to one a-trous pass on the same frame,
and inside the pipeline it exists for.  The snapshot's own camera at 1080p, one view, 3 channels.  Per scene:
  inputs        Scene.view_hits; the framed K-direction cosine gather with a spin plane at full size (view_gather) and, per
                factor, on rays.coarse_hits (hit_gather): each timed.  The coarse colour is the gather's first three channels
  launch_ms     one qr_upsample_views_async launch into preallocated outputs, normal stop at power 128 and plane stop at two
                coarse footprints at the median depth: colour only; with variance and weight; with both and MODULATE
  bytes         what a launch must move by its shapes: per full pixel 32 B of record (48 with MODULATE) read and 12 B of colour
                written, plus 4 B variance and 4 B weight where given; the coarse side adds (12 + 4 + 48) / s^2 (12 + 48
                without a variance).  GB/s = bytes / time
  atrous_ms     the yardstick: one Scene.atrous pass at step 1 with the normal and plane stops on the full-size gather, without
                and with a variance
  torch_ms      the same step as torch gathers and elementwise operations with the same formulas in the same order, timed
                only after the two were compared word for word on this input (torch_same; where they differ, how many words)
  pipeline      view_hits, then hit_gather on coarse_hits at factor 2 (and 4), then upsample, against view_gather at full size
                with the same K; each chain timed as a whole
  quality       reported, not gated: the upsampled gather against the full-size one (mean absolute and root mean square
                difference over the hit pixels, the full-size frame's own mean), and the share of pixels per stage
Steps (each its own child process under its own `timeout`; after a step that fails nothing else is started):
  demo1_1080p     demo scene 1 from its own camera, eps 1e-3, reach 2
  synth10k_1080p  the synthetic 10 000-quadric scene (per-lane walks, a uniform grid), reach a tenth of its extent
One JSON line per step, then the kernels' resources from the build assembly.  A step that was not run is written as NOT MEASURED
with the reason.  No speed target is set: the comparisons are against existing code measured in the same process.

usage: gpu_upsample.py [--out FILE] [--step NAME]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STEPS = {"demo1_1080p": 400, "synth10k_1080p": 500}   # s
K, EPS, FACTORS, ROUNDS, WINDOW = 16, 1e-3, (2, 4), 3, 0.25


def torch_upsample(torch, col_lo, var_lo, hits, s, phase, flags, normal_sq, sigma_z, alb_floor):
    """rays.upsample_pass in torch operations on the tensors' device: one rounding per operation, the taps as gathers by index.
    Every division is tensor by tensor: torch divides a device tensor by a host number through the number's reciprocal, which
    rounds twice.  Returns (colour, variance or None, weight)"""
    px, py = phase
    n, h, w = hits.shape[:3]
    hl, wl, ch = col_lo.shape[1:]
    dev = hits.device
    ids = hits.view(torch.int32)[..., 7]
    pos, nrm, alb = hits[..., 0:3], hits[..., 4:7], hits[..., 8:11]
    guide = hits[:, py::s, px::s]
    gid = guide.view(torch.int32)[..., 7]
    gpos, gnrm, galb = guide[..., 0:3], guide[..., 4:7], guide[..., 8:11]
    floor = torch.tensor(alb_floor, dtype=torch.float32, device=dev)
    col = col_lo.clone()
    if flags & 8:
        a = torch.where(galb > floor, galb, floor)
        col[..., 0:3] = torch.where((gid >= 0)[..., None], col[..., 0:3] / a, col[..., 0:3])
    var = var_lo if var_lo is not None else torch.zeros((n, hl, wl), dtype=torch.float32, device=dev)
    ys, xs = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
    x0, y0 = torch.div(xs - px, s, rounding_mode="floor"), torch.div(ys - py, s, rounding_mode="floor")
    rx, ry = (xs - px) - x0 * s, (ys - py) - y0 * s
    one, zero = torch.ones((n, h, w), dtype=torch.float32, device=dev), torch.zeros((n, h, w), dtype=torch.float32, device=dev)
    sf = torch.full((h, w), float(s), dtype=torch.float32, device=dev)
    wx, wy = rx.float() / sf, ry.float() / sf
    sigma = torch.full((n, h, w), sigma_z, dtype=torch.float32, device=dev)
    hit_p = ids >= 0
    vi = torch.arange(n, device=dev)[:, None, None]
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    each = []
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = x0 + i, y0 + j
            inside = (qx >= 0) & (qx < wl) & (qy >= 0) & (qy < hl)
            qx, qy = qx.clamp(0, wl - 1), qy.clamp(0, hl - 1)
            b = (wx if i else 1.0 - wx) * (wy if j else 1.0 - wy)
            idg = gid[vi, qy, qx]
            g = one
            if flags & 1:
                d = dot(nrm, gnrm[vi, qy, qx])
                d = torch.where(d > 0, d, zero)
                for _ in range(normal_sq):
                    d = d * d
                g = g * d
            if flags & 2:
                t = dot(nrm, gpos[vi, qy, qx] - pos).abs() / sigma
                g = g * (one / (one + t * t))
            ok = (idg >= 0) & ((idg == ids) if flags & 4 else True)
            elig = inside[None] & torch.where(hit_p, ok, idg < 0)
            each.append((elig, b, torch.where(hit_p, g, one), qy, qx))
    sums = []
    for stage in (1, 2):
        sc, sw, sv = torch.zeros((n, h, w, ch), dtype=torch.float32, device=dev), zero, zero
        for elig, b, g, qy, qx in each:
            wt = b[None] * g if stage == 1 else g
            take = elig & (wt > 0)
            wt = torch.where(take, wt, zero)
            sc = torch.where(take[..., None], sc + col[vi, qy, qx] * wt[..., None], sc)
            sw = torch.where(take, sw + wt, sw)
            sv = torch.where(take, sv + var[vi, qy, qx] * (wt * wt), sv)
        sums.append((sc, sw, sv))
    first = sums[0][1] > 0
    sc = torch.where(first[..., None], sums[0][0], sums[1][0])
    sw, sv = torch.where(first, sums[0][1], sums[1][1]), torch.where(first, sums[0][2], sums[1][2])
    served = sw > 0
    nx = (x0 + (2 * rx >= s).long()).clamp(0, wl - 1)
    ny = (y0 + (2 * ry >= s).long()).clamp(0, hl - 1)
    out = torch.where(served[..., None], sc / sw[..., None], col[vi, ny, nx])
    vout = torch.where(served, sv / (sw * sw), var[vi, ny, nx])
    weight = torch.where(first, sw, torch.where(served, zero, -one))
    if flags & 16:
        a = torch.where(alb > floor, alb, floor)
        out = torch.cat([torch.where(hit_p[..., None], out[..., 0:3] * a, out[..., 0:3]), out[..., 3:]], -1)
    return out, (vout if var_lo is not None else None), weight


def launch_bytes(n, h, w, s, variance, weight, modulate):
    """what one launch must move by its shapes: per full pixel the record's pos and nrm quads (and the albedo quad with MODULATE)
    read and the colour, variance and weight written; per coarse pixel the colour, the variance and the whole guide record"""
    full = (48 if modulate else 32) + 12 + (4 if variance else 0) + (4 if weight else 0)
    coarse = 12 + (4 if variance else 0) + 48
    hl, wl = (h + s - 1) // s, (w + s - 1) // s
    return n * (h * w * full + hl * wl * coarse)


def scene_figures(grq, scn, blob, reach):
    import numpy as np
    import torch
    qr, rm, timed = grq.qr, grq.rays_mod, grq.timed
    w, h = scn.width, scn.height
    base = rm.view_of(blob)
    vt = torch.from_numpy(base[None].copy()).cuda()
    dirs = torch.from_numpy(rm.cosine_dirs(K)).cuda()
    spin = torch.from_numpy(rm.spins((1, h, w), 1)).cuda()
    kw = dict(eps=EPS, reach=reach, frame=True)

    def med(fns):
        """median over ROUNDS rounds of every candidate, the candidates taken in turn in each round"""
        t = {k: [] for k in fns}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                t[k].append(timed(fn, WINDOW, warm=2))
        return {k: round(statistics.median(v), 4) for k, v in t.items()}

    hits = scn.view_hits(vt, w, h)
    hid = hits.view(torch.int32)[..., 7]
    depth = float(hits[..., 3][hid >= 0].median())
    pixel = float(np.linalg.norm(base[8:11])) * depth           # one pixel's footprint at the median depth, world units
    full, _ = scn.view_gather(vt, dirs, w, h, spin=spin, **kw)
    full3 = full[..., 0:3].contiguous()
    res = {"width": w, "height": h, "fsaa": int(scn.info.fsaa), "k": K, "eps": EPS, "reach": reach, "rounds": ROUNDS, "window_s": WINDOW,
           "median_depth": round(depth, 4), "pixel_footprint": round(pixel, 6), "hit_fraction": round(float((hid >= 0).float().mean()), 4)}
    var_full = (full3.mean(-1) * 0.1 + 1e-3).contiguous()
    res["inputs_ms"] = med({"view_hits": lambda: scn.view_hits(vt, w, h),
                            "view_gather_full": lambda: scn.view_gather(vt, dirs, w, h, spin=spin, **kw)})
    res["atrous_ms"] = med({"step1_normal_plane": lambda: scn.atrous(full3, hits, None, 1, normal_power=128, plane=pixel),
                            "step1_normal_plane_variance": lambda: scn.atrous(full3, hits, var_full, 1, normal_power=128, plane=pixel)})
    hit = hid >= 0
    for s in FACTORS:
        ph = (0, 0)
        wl, hl = rm.coarse_size(w, h, s, ph)
        lo_hits = rm.coarse_hits(hits, s, ph)
        lo_spin = spin[:, ph[1]::s, ph[0]::s].contiguous()
        lo, _ = scn.hit_gather(lo_hits, dirs, spin=lo_spin, **kw)
        lo3 = lo[..., 0:3].contiguous()
        lo_var = (lo3.mean(-1) * 0.1 + 1e-3).contiguous()
        sigma = 2.0 * s * pixel
        stops = dict(normal_power=128, plane=sigma)
        out, vout, wout = torch.empty_like(full3), torch.empty((1, h, w), device="cuda"), torch.empty((1, h, w), device="cuda")
        cand = {"colour": lambda: scn.upsample(lo3, hits, s, ph, out=out, **stops),
                "variance_weight": lambda: scn.upsample(lo3, hits, s, ph, variance=lo_var, out=out, variance_out=vout, weight=wout, **stops),
                "variance_weight_modulate": lambda: scn.upsample(lo3, hits, s, ph, variance=lo_var, out=out, variance_out=vout, weight=wout,
                                                                 modulate=True, **stops)}
        nbytes = {"colour": launch_bytes(1, h, w, s, False, False, False), "variance_weight": launch_bytes(1, h, w, s, True, True, False),
                  "variance_weight_modulate": launch_bytes(1, h, w, s, True, True, True)}
        r = {"coarse": [wl, hl], "sigma_z": round(sigma, 6), "launch_bytes": nbytes}
        r["launch_ms"] = med(cand)
        r["launch_GB_per_s"] = {k: round(nbytes[k] / r["launch_ms"][k] / 1e6, 1) for k in cand}
        r["launch_ms_over_atrous_ms"] = {"colour": round(r["launch_ms"]["colour"] / res["atrous_ms"]["step1_normal_plane"], 3),
                                         "variance_weight": round(r["launch_ms"]["variance_weight"] / res["atrous_ms"]["step1_normal_plane_variance"], 3)}
        # the composition must give the launch's bits before it is timed
        flags, nsq, sz, af = rm.upsample_stops(**stops)
        args = (lo3, lo_var, hits, s, ph, flags, nsq, float(sz), float(af))
        tc, tv, tw = torch_upsample(torch, *args)
        cand["variance_weight"]()
        torch.cuda.synchronize()
        pairs = ((tc, out), (tv, vout), (tw, wout))
        each = [int((a.view(torch.int32) != b.view(torch.int32)).sum()) for a, b in pairs]
        differ = sum(each)
        r["torch_same"] = differ == 0 or {"words_differing": differ, "of": sum(a.numel() for a, _ in pairs),
                                          "colour_variance_weight": each,
                                          "largest_in_last_places": max(int((a.view(torch.int32) - b.view(torch.int32)).abs().max()) for a, b in pairs)}
        if differ == 0:
            r["torch_ms"] = round(timed(lambda: torch_upsample(torch, *args), WINDOW, warm=1), 4)
            r["torch_ms_over_launch_ms"] = round(r["torch_ms"] / r["launch_ms"]["variance_weight"], 1)
        else:
            r["torch_ms"] = "NOT TIMED: the composition differs from the launch"
        r["stage_share"] = [round(float((wout > 0).float().mean()), 5), round(float((wout == 0).float().mean()), 5),
                            round(float((wout < 0).float().mean()), 5)]
        # the pipeline: records, the coarse gather from the strided records, the upsample -- against the gather at full size
        def coarse_chain():
            hh = scn.view_hits(vt, w, h)
            g, _ = scn.hit_gather(rm.coarse_hits(hh, s, ph), dirs, spin=lo_spin, **kw)
            return scn.upsample(g, hh, s, ph, **stops)
        r["pipeline_ms"] = med({"hits_coarse_gather_upsample": coarse_chain,
                                "coarse_gather_alone": lambda: scn.hit_gather(lo_hits, dirs, spin=lo_spin, **kw),
                                "view_gather_full": lambda: scn.view_gather(vt, dirs, w, h, spin=spin, **kw)})
        r["full_ms_over_pipeline_ms"] = round(r["pipeline_ms"]["view_gather_full"] / r["pipeline_ms"]["hits_coarse_gather_upsample"], 2)
        up = scn.upsample(lo3, hits, s, ph, **stops)
        d = (up - full3)[hit]
        r["quality_vs_full_gather"] = {"mean_abs": round(float(d.abs().mean()), 5), "rms": round(float((d * d).mean().sqrt()), 5),
                                       "full_mean": round(float(full3[hit].mean()), 5)}
        res[f"factor_{s}"] = r
    return res


def step(name):
    import importlib.util
    import numpy as np
    import torch
    spec = importlib.util.spec_from_file_location("gpu_ray_query", os.path.join(HERE, "gpu_ray_query.py"))
    grq = importlib.util.module_from_spec(spec); spec.loader.exec_module(grq)
    qr = grq.qr
    res = {"version": qr.lib().qr_version().decode(), "device": torch.cuda.get_device_name(0)}
    if name == "demo1_1080p":
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
    res.update(scene_figures(grq, scn, blob, reach))
    scn.close()
    return res


def resources():
    sys.path.insert(0, HERE)
    import check_kernel_resources as ck
    asm = os.path.join(ROOT, "quadray-engine_amd", "csrc", "qr_device-hip-amdgcn-amd-amdhsa-gfx950.s")
    if not os.path.exists(asm):
        return {"resources": "no build assembly in this tree"}
    return {"resources": {k["name"]: {a: k[a] for a in ck.KEYS if a != "name"} for k in ck.kernels(asm) if "qr_upsample_kernel" in k["name"]}}


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
