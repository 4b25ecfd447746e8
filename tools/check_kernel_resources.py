#!/usr/bin/env python3
"""Build-time check (called by csrc/Makefile after the device TU is compiled): the register budget the frame times depend on.

Reads the code-object metadata of the -save-temps assembly (qr_device-hip-amdgcn-amd-amdhsa-gfx950.s) and fails the build when
  * the packet-walk instance qr_render_kernel<false,4,false> (every scene of the reference engine) spills a vector register, uses
    more than 128 VGPRs (4 waves per SIMD) or a private segment above the recursion frames' bytes (QR_MAX_SCRATCH, default 528);
  * the per-lane instance <false,3,true> exceeds 168 VGPRs (3 waves per SIMD) or spills more vector registers than QR_MAX_DIVK_SPILL;
  * a ray-query instance qr_trace_kernel<SHADOW, COHERENT> spills a vector register or uses more than 128 (occlusion) / 168 VGPRs;
  * a ray-shading instance qr_shade_rays_kernel<COHERENT> exceeds the per-lane render instance's budget (168 VGPRs,
    QR_MAX_DIVK_SPILL spilled, 640 B private segment);
  * a view-rendering instance qr_render_views_kernel<DIVK, WAVES> exceeds that same budget, or its packet-walk instance
    <false,4> 128 VGPRs;
  * a view-accumulation instance qr_views_mean_kernel<DIVK, WAVES> exceeds the budget of the view-rendering instance it mirrors;
  * the path-traced view kernel qr_pt_views_kernel exceeds 168 VGPRs (3 waves per SIMD, its launch bound), spills a vector
    register or has a larger private segment than the scene's own path-tracer kernel (2128 B);
  * the path-traced ray kernel qr_pt_rays_kernel exceeds that same budget;
  * the adaptive path-traced ray kernel qr_pt_adapt_kernel exceeds that same budget;
  * the adaptive path-traced view kernel qr_pt_adapt_views_kernel exceeds that same budget;
  * the indexed adaptive kernel qr_pt_list_kernel exceeds that same budget, or one of the three open-list kernels
    (qr_openlist.hpp) spills a vector register or has a private segment;
  * a hit-record instance qr_hit_kernel<VIEW, DIVK, COHERENT> spills a vector register, has a private segment, or uses more than
    168 VGPRs (128: the view instance with packet walks only);
  * an occlusion-fan instance qr_fan_kernel<SRC, DIVK, COHERENT> spills a vector register, has a private segment, or uses more
    than 168 VGPRs (128: the view instance with packet walks only and the instance that reads caller records);
  * a gather-fan instance qr_gather_kernel<SRC, DIVK, COHERENT, WAVES> exceeds the budget of the ray-shading or view-rendering
    instance whose machine it runs (168 VGPRs, 128 for the view instance with packet walks only; QR_MAX_DIVK_SPILL; 640 B);
  * a framed-fan instance qr_fan_framed_kernel<SRC, DIVK, COHERENT> or qr_gather_framed_kernel<SRC, DIVK, COHERENT, WAVES>
    exceeds the budget of the unframed instance it mirrors;
  * a hit-layer instance qr_layer_kernel<VIEW, DIVK, COHERENT> spills a vector register, has a private segment, or uses more
    than 168 VGPRs (128: the view instance with packet walks only);
  * a guided a-trous instance qr_atrous_kernel<CH> or qr_pt_adapt_var_kernel spills a vector register, has a private segment or
    uses more than 64 VGPRs, or a filter instance more LDS than its 36 x 12 staged entries (20736 B / 22464 B);
  * a temporal reprojection instance qr_reproject_kernel<CH> spills a vector register, has a private segment, uses any LDS or
    more than 96 (3 channels) / 80 (4 channels) VGPRs, or an instance with a motion table qr_reproj_moving_kernel<CH> more than
    those plus its 12 row words (108 / 92);
  * a clamped reprojection instance qr_reproj_clamp_kernel<CH, MOVING> spills a vector register, has a private segment, uses more
    than 96 (3 channels) / 80 (4 channels) VGPRs or more LDS than its 38 x 14 staged entries of CH + 1 planes (8512 B / 10640 B);
  * a guided upsampling instance qr_upsample_kernel<CH> spills a vector register, has a private segment, uses more than 64 VGPRs
    or more LDS than its 34 x 10 staged entries (14960 B / 16320 B);
  * the hand-written cull loop's fixed scalar registers s[88:99] (qr_walk.hpp cull_run) are missing from its clobber list.
usage: check_kernel_resources.py <file.s> [--print]
"""
import os, re, sys

SCR = int(os.environ.get("QR_MAX_SCRATCH", "528"))
LIMITS = {
    # mangled-name fragment: (max vgpr_count, max vgpr_spill_count, max private_segment_fixed_size)
    "16qr_render_kernelILb0ELi4ELb0EE": (128, 0, SCR),
    "22qr_render_multi_kernelILi4ELb0EE": (128, 0, SCR),
    "16qr_render_kernelILb0ELi3ELb1EE": (168, int(os.environ.get("QR_MAX_DIVK_SPILL", "24")), 640),
    # ray queries (qr_query.hpp), with and without QR_TRACE_COHERENT, nothing spilled: occlusion at 4 waves per SIMD; closest hit at
    # the per-lane render instance's 3 (the hit the hand-over pool carries: 128 registers spilled 35 of them)
    "15qr_trace_kernelILb0ELb0EE": (168, 0, SCR),
    "15qr_trace_kernelILb0ELb1EE": (168, 0, SCR),
    "15qr_trace_kernelILb1ELb0EE": (128, 0, SCR),
    "15qr_trace_kernelILb1ELb1EE": (128, 0, SCR),
    # ray shading (qr_kernel.hpp qr_shade_rays_kernel<COHERENT>): the per-lane render instance's machine, held to its budget
    "20qr_shade_rays_kernelILb0EE": (168, int(os.environ.get("QR_MAX_DIVK_SPILL", "24")), 640),
    "20qr_shade_rays_kernelILb1EE": (168, int(os.environ.get("QR_MAX_DIVK_SPILL", "24")), 640),
    # view rendering (qr_kernel.hpp qr_render_views_kernel<DIVK, WAVES>): the same machine on the rays of caller-supplied cameras,
    # same budget; its packet-walk instance at the packet render instance's 128 registers (4 waves per SIMD)
    "22qr_render_views_kernelILb0ELi4EE": (128, int(os.environ.get("QR_MAX_DIVK_SPILL", "24")), 640),
    "22qr_render_views_kernelILb1ELi3EE": (168, int(os.environ.get("QR_MAX_DIVK_SPILL", "24")), 640),
    # view accumulation (qr_kernel.hpp qr_views_mean_kernel<DIVK, WAVES>): the view instances' machine run once per view, the sum
    # of the views live in three more registers across it: held to the view instances' budgets
    "20qr_views_mean_kernelILb0ELi4EE": (128, int(os.environ.get("QR_MAX_DIVK_SPILL", "24")), 640),
    "20qr_views_mean_kernelILb1ELi3EE": (168, int(os.environ.get("QR_MAX_DIVK_SPILL", "24")), 640),
    # path-traced views (qr_kernel.hpp qr_pt_views_kernel): the path-tracer instance (packet walks, launch bound 3 waves per SIMD:
    # 168 registers) on view rays in a loop over samples; nothing spilled and no more private segment than qr_render_pt_kernel,
    # whose recursion frames it shares (2128 B there with the eager machine's levels, which this kernel leaves out: 880 B)
    "18qr_pt_views_kernel7LaunchP": (168, 0, 2128),
    # path-traced rays (qr_kernel.hpp qr_pt_rays_kernel): the same instance and sample loop on caller rays: the same budget
    "17qr_pt_rays_kernel": (168, 0, 2128),
    # adaptive path-traced rays (qr_kernel.hpp qr_pt_adapt_kernel): that kernel with per-ray counts and a stop rule: the same budget
    "18qr_pt_adapt_kernel": (168, 0, 2128),
    # indexed adaptive path-traced rays (qr_kernel.hpp qr_pt_list_kernel): that kernel with its rays taken from a list: the same budget
    "17qr_pt_list_kernel": (168, 0, 2128),
    # adaptive path-traced views (qr_kernel.hpp qr_pt_adapt_views_kernel): qr_pt_views_kernel's grid and output step around the
    # adaptive ray kernel's sample loop: the same budget
    "24qr_pt_adapt_views_kernel": (168, 0, 2128),
    # the open list (qr_openlist.hpp): a rule, a ballot and a scan: nothing spilled, no private segment
    "20qr_open_count_kernel": (128, 0, 0),
    "19qr_open_scan_kernel": (128, 0, 0),
    "22qr_open_scatter_kernel": (128, 0, 0),
    # hit records (qr_hitrec.hpp qr_hit_kernel<VIEW, DIVK, COHERENT>): a walk and one surface point, no recursion: nothing spilled and
    # no private segment at all; caller rays and views of scenes with long lists at the closest-hit query's 168 registers, views of
    # the others at the packet instances' 128
    "13qr_hit_kernelILb0ELb1ELb0EE": (168, 0, 0),
    "13qr_hit_kernelILb0ELb1ELb1EE": (168, 0, 0),
    "13qr_hit_kernelILb1ELb1ELb1EE": (168, 0, 0),
    "13qr_hit_kernelILb1ELb0ELb1EE": (128, 0, 0),
    # occlusion fans (qr_fan.hpp qr_fan_kernel<SRC, DIVK, COHERENT>; SRC 0 caller rays, 1 views, 2 caller records): a first walk and
    # one surface point as a hit-record instance, then the occlusion query's walk in a loop with point, normal, count and mask
    # word live across it: nothing spilled, no private segment; the hit-record instances' registers where there is a first
    # walk, the occlusion query's 128 (4 waves per SIMD) where there is none
    "13qr_fan_kernelILi0ELb1ELb0EE": (168, 0, 0),
    "13qr_fan_kernelILi0ELb1ELb1EE": (168, 0, 0),
    "13qr_fan_kernelILi1ELb1ELb1EE": (168, 0, 0),
    "13qr_fan_kernelILi1ELb0ELb1EE": (128, 0, 0),
    "13qr_fan_kernelILi2ELb1ELb0EE": (128, 0, 0),
    # gather fans (qr_gather.hpp qr_gather_kernel<SRC, DIVK, COHERENT, WAVES>): a fan kernel's first walk and loop around the ray
    # shading machine, with point, normal, sums and count parked in LDS across it: held to the budget of the shading instance each
    # one runs (qr_shade_rays_kernel for caller rays and records, qr_render_views_kernel<DIVK, WAVES> for views)
    "16qr_gather_kernelILi0ELb1ELb0ELi3EE": (168, int(os.environ.get("QR_MAX_DIVK_SPILL", "24")), 640),
    "16qr_gather_kernelILi0ELb1ELb1ELi3EE": (168, int(os.environ.get("QR_MAX_DIVK_SPILL", "24")), 640),
    "16qr_gather_kernelILi2ELb1ELb0ELi3EE": (168, int(os.environ.get("QR_MAX_DIVK_SPILL", "24")), 640),
    "16qr_gather_kernelILi1ELb1ELb1ELi3EE": (168, int(os.environ.get("QR_MAX_DIVK_SPILL", "24")), 640),
    "16qr_gather_kernelILi1ELb0ELb1ELi4EE": (128, int(os.environ.get("QR_MAX_DIVK_SPILL", "24")), 640),
    # framed fans (qr_fan_framed.hpp): the five occlusion-fan instances with the element's frame (u, v: six more registers across
    # the loop) and the five gather-fan instances with the spin parked beside the rest; each held to its unframed twin's budget
    "20qr_fan_framed_kernelILi0ELb1ELb0EE": (168, 0, 0),
    "20qr_fan_framed_kernelILi0ELb1ELb1EE": (168, 0, 0),
    "20qr_fan_framed_kernelILi1ELb1ELb1EE": (168, 0, 0),
    "20qr_fan_framed_kernelILi1ELb0ELb1EE": (128, 0, 0),
    "20qr_fan_framed_kernelILi2ELb1ELb0EE": (128, 0, 0),
    "23qr_gather_framed_kernelILi0ELb1ELb0ELi3EE": (168, int(os.environ.get("QR_MAX_DIVK_SPILL", "24")), 640),
    "23qr_gather_framed_kernelILi0ELb1ELb1ELi3EE": (168, int(os.environ.get("QR_MAX_DIVK_SPILL", "24")), 640),
    "23qr_gather_framed_kernelILi2ELb1ELb0ELi3EE": (168, int(os.environ.get("QR_MAX_DIVK_SPILL", "24")), 640),
    "23qr_gather_framed_kernelILi1ELb1ELb1ELi3EE": (168, int(os.environ.get("QR_MAX_DIVK_SPILL", "24")), 640),
    "23qr_gather_framed_kernelILi1ELb0ELb1ELi4EE": (128, int(os.environ.get("QR_MAX_DIVK_SPILL", "24")), 640),
    # hit layers (qr_layers.hpp qr_layer_kernel<VIEW, DIVK, COHERENT>): a hit-record instance's walk and surface point in a loop over
    # the layers, with the ray, the count and the alive flag live across it: nothing spilled, no private segment, and no more
    # registers than the hit-record instance each one mirrors
    "15qr_layer_kernelILb0ELb1ELb0EE": (168, 0, 0),
    "15qr_layer_kernelILb0ELb1ELb1EE": (168, 0, 0),
    "15qr_layer_kernelILb1ELb1ELb1EE": (168, 0, 0),
    "15qr_layer_kernelILb1ELb0ELb1EE": (128, 0, 0),
    # guided a-trous filter (qr_atrous.hpp qr_atrous_kernel<CH>): 25 taps out of LDS, bound by LDS and memory, not by registers:
    # nothing spilled, no private segment, 64 VGPRs (8 waves per SIMD: seven workgroups of 4 waves per CU fit their LDS), and no
    # more LDS than 36 x 12 entries of 13 planes; the variance kernel beside it likewise
    "16qr_atrous_kernelILi3EE": (64, 0, 0),
    "16qr_atrous_kernelILi4EE": (64, 0, 0),
    "22qr_pt_adapt_var_kernel": (64, 0, 0),
    # temporal reprojection (qr_reproject.hpp qr_reproject_kernel<CH>): a projection and four gathered taps per pixel, bound by the
    # bytes it moves: nothing spilled, no private segment, no LDS at all, and the registers of the build's assembly rounded up to
    # the next occupancy step: 82 VGPRs -> 96 (5 waves per SIMD), 74 -> 80 (6 waves).  The registers are the sixteen quads of
    # the four taps in flight at once, which is what the launch time rests on (qr_reproject.hpp)
    "19qr_reproject_kernelILi3EE": (96, 0, 0),
    "19qr_reproject_kernelILi4EE": (80, 0, 0),
    # temporal reprojection with a motion table (qr_reproject.hpp qr_reproj_moving_kernel<CH>): the same pixel with the move step:
    # nothing spilled, no private segment, no LDS, and the static instance's limit plus the 12 row words a lane may hold at once
    # (108 / 92; the build's assembly has 80 / 74)
    "23qr_reproj_moving_kernelILi3EE": (108, 0, 0),
    "23qr_reproj_moving_kernelILi4EE": (92, 0, 0),
    # temporal reprojection with a clamp (qr_reproject.hpp qr_reproj_clamp_kernel<CH, MOVING>): the same pixel behind a staged
    # neighbourhood and a box out of LDS: nothing spilled, no private segment, no more LDS than (32 + 6) x (8 + 6) staged entries
    # of CH + 1 planes, and the registers of the build's assembly rounded up to the next occupancy step: 84 / 82 VGPRs -> 96
    # (5 waves per SIMD), 78 / 76 -> 80 (6 waves), the steps of the instances without the clamp
    "22qr_reproj_clamp_kernelILi3ELb0EE": (96, 0, 0),
    "22qr_reproj_clamp_kernelILi3ELb1EE": (96, 0, 0),
    "22qr_reproj_clamp_kernelILi4ELb0EE": (80, 0, 0),
    "22qr_reproj_clamp_kernelILi4ELb1EE": (80, 0, 0),
    # guided upsampling (qr_upsample.hpp qr_upsample_kernel<CH>): four taps out of LDS per full pixel, bound by the bytes it moves:
    # nothing spilled, no private segment, and the registers of the build's assembly (35 / 36 VGPRs) rounded up to the next
    # occupancy step, 64 (8 waves per SIMD, all a SIMD holds); no more LDS than 34 x 10 staged entries of 8 + CH planes, of which
    # eight workgroups of 4 waves -- a CU's 32 waves -- fit beside each other
    "18qr_upsample_kernelILi3EE": (64, 0, 0),
    "18qr_upsample_kernelILi4EE": (64, 0, 0),
}
LDS_LIMITS = {"16qr_atrous_kernelILi3EE": 20736, "16qr_atrous_kernelILi4EE": 22464,
              "19qr_reproject_kernelILi3EE": 0, "19qr_reproject_kernelILi4EE": 0,
              "23qr_reproj_moving_kernelILi3EE": 0, "23qr_reproj_moving_kernelILi4EE": 0,
              "22qr_reproj_clamp_kernelILi3ELb0EE": 8512, "22qr_reproj_clamp_kernelILi3ELb1EE": 8512,
              "22qr_reproj_clamp_kernelILi4ELb0EE": 10640, "22qr_reproj_clamp_kernelILi4ELb1EE": 10640,
              "18qr_upsample_kernelILi3EE": 14960, "18qr_upsample_kernelILi4EE": 16320}
KEYS = ("name", "group_segment_fixed_size", "private_segment_fixed_size", "sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count")


def kernels(path):
    out, cur = [], None
    for line in open(path, errors="replace"):
        m = re.match(r"\s+-?\s*\.(\w+):\s+(\S+)", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2)
        if k == "group_segment_fixed_size":
            cur = {}; out.append(cur)
        if cur is not None and k in KEYS:
            cur[k] = v if k == "name" else int(v)
    return [k for k in out if "name" in k and "vgpr_count" in k]


def main():
    path = sys.argv[1]
    ks = kernels(path)
    bad = []
    for k in ks:
        if "--print" in sys.argv:
            print({a: k.get(a) for a in KEYS})
        for frag, (vg, sp, scr) in LIMITS.items():
            if frag in k["name"]:
                if k["vgpr_count"] > vg: bad.append(f"{k['name']}: {k['vgpr_count']} VGPRs > {vg} (a wave per SIMD lost)")
                if k["vgpr_spill_count"] > sp: bad.append(f"{k['name']}: {k['vgpr_spill_count']} vector registers spilled > {sp}")
                if k["private_segment_fixed_size"] > scr: bad.append(f"{k['name']}: private segment {k['private_segment_fixed_size']} B > {scr}")
        for frag, lds in LDS_LIMITS.items():
            if frag in k["name"] and k["group_segment_fixed_size"] > lds:
                bad.append(f"{k['name']}: {k['group_segment_fixed_size']} B of LDS > {lds} (a workgroup per CU lost)")
    missing = [frag for frag in LIMITS if not any(frag in k["name"] for k in ks)]
    if missing:
        bad.append(f"kernel instances missing from {path}: {missing}")
    src = os.path.join(os.path.dirname(os.path.abspath(path)), "qr_walk.hpp")
    if os.path.exists(src):
        text = open(src).read()
        if "cull_run" in text and "s88" in text:
            for r in range(88, 100):
                if not re.search(r'"s%d"' % r, text):
                    bad.append(f"qr_walk.hpp cull_run: s{r} is used by name but missing from the clobber list")
    if bad:
        print("KERNEL RESOURCE CHECK FAILED:\n  " + "\n  ".join(bad), file=sys.stderr)
        return 1
    print(f"kernel resource check ok ({len(ks)} kernels)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
