"""Ray batches and views for Scene.trace / Scene.occluded / Scene.shade (include/qrhip.h qr_trace_rays_async, qr_shade_rays_async): one
ray per row of a float32 [N, 8] array, (org x, y, z, tmin, dir x, y, z, tmax) -- the layout of qr_ray.

camera_rays turns a snapshot's camera into such a batch: the primary rays of the render kernel (qr_kernel.hpp, the reference's
tracer.cpp:1287-1322) in its own fp32 operation order, so that tracing them gives the frame's hit ids bit for bit.
pack_colors is the frame's output step (clamp, FSAA reduce, gamma, scale, pack) for the linear colours Scene.shade returns.
Together they give the frame that a walk of the global list renders (with the snapshot's own tile lists the frame can differ
only where the engine's tiles hold other surfaces than its global list):

    scn = Scene(blob, ray_queries=True)
    ns = 1 << fsaa                                  # the snapshot's FSAA: 0, 1 or 2
    rgb = torch.stack([scn.shade(torch.from_numpy(camera_rays(blob, sample=k)).cuda()) for k in range(ns)])
    frame = pack_colors(rgb.cpu().numpy(), blob)    # uint32 [H, W], 0x00RRGGBB

Scene.hits / Scene.view_hits return hit records (qr_hit: position, t, normal, id, albedo, material); hit_fields splits them into
typed views, offset_rays and reflect_rays build a host's own secondary rays from them.  Fans of many visibility rays per hit
(ambient occlusion, sky visibility) need no rays: Scene.occlusion / view_occlusion / hit_occlusion trace a shared direction table
(sphere_dirs) from every hit in one launch; fan_rays states what they trace, fan_bits unpacks their masks.  Scene.gather /
view_gather / hit_gather SHADE the same fans and return one weighted sum of colours per hit (final gather, irradiance, lightmap
and probe baking); gather_fold states the sum.  Scene.trace_layers /
Scene.view_layers give the first k hits along a ray, in order, in one launch; layers_of states them as a composition of trace(),
next_rays builds the rays that resume a layered ray where a call stopped.

Whole frames from pinhole cameras do not need that detour: Scene.render_views renders them on the GPU from qr_view records
(view_of: the snapshot's own camera; look_at: eye / target / up / field of view), at any frame size, and view_rays gives the
rays it computes.

    views = torch.from_numpy(np.stack([view_of(blob), look_at(eye, target, up, 60.0, 512, 512)])).cuda()
    frames = scn.render_views(views, 512, 512)      # int32 [2, 512, 512]

Scene.render_views_mean gives ONE frame that is the mean of many views, summed in linear fp32 colour on the GPU: jitter_view
(sub-pixel-shifted copies: supersampling) and thin_lens_views (depth of field) make such view sets; reduce_colors, pack_linear and
mean_of_views state its arithmetic in numpy.

    views = torch.from_numpy(np.stack([jitter_view(view_of(blob), dx, dy) for dx, dy in offsets])).cuda()
    frame, sum = scn.render_views_mean(views)       # int32 [H, W], float32 [H, W, 3]

Scene.pt_views accumulates path-traced frames of such views in a state tensor the caller owns; pt_seeds gives the seed plane
every view starts from and pt_random the generator's step, so that a host can predict, edit or checkpoint a state.

Scene.pt_rays is the same accumulation for caller rays (include/qrhip.h qr_pt_rays_async): path-traced samples for a host's own
camera, probe or lightmap rays, or more samples only where a picture is still noisy.  Its state is int32 [4, N], ray i in
column i, reset to pt_seeds(N, 1, 1).  An optional spread per ray (du, dv: the change of direction per pixel step) jitters every
sample's direction through the renderer's tent filter: pt_jitter gives the two draws and spread_rays the rays they make.
pt_view_rays gives the rays ONE path-traced sample of a pinhole view traces (Scene.pt_views, set_pt + render), in slot order:

    acc = scn.pt_rays(n)                            # state: seeds of slots 0 .. n - 1, means 0
    rgb = acc.step(rays, samples=16, spread=spread) # float32 [n, 3]: running means after 16 samples, before any clamp
    rgb = acc.step(other_rays, samples=4)           # the state belongs to the accumulation, not to a ray set

Scene.pt_adaptive is pt_rays with a sample count and a noise estimate per ray (include/qrhip.h qr_pt_adapt_rays_async): the state
is int32 [8, N] -- pt_rays' four planes, then the count m and Welford's M2 of r, g, b -- and a stop rule on that column decides
before every sample whether the ray takes it.  pt_adapt_open states the rule and pt_adapt_fold the update, in float32 numpy:

    acc = scn.pt_adaptive(n, min_samples=4, max_samples=64, tol=0.01)
    while True:
        rgb, still = acc.step(rays, samples=8, spread=spread, open=True)    # up to 8 more samples where the rule asks for them
        if int(still) == 0: break                                            # acc.counts: samples per ray

A wave of that step holds 64 consecutive rays and runs as long as its slowest.  PtAdaptive.open_list writes the indices of the open
rays on the device and step(index=, count=) serves 64 LISTED rays per wave; the state is bit for bit the same (pt_adapt_open_list
and pt_adapt_fold_list are the specification):

    cap = n
    while cap:
        index, count = acc.open_list()                                       # on the device; nothing is read back
        _, still = acc.step(rays, 8, spread=spread, rgb=False, open=True, index=index, count=count, cap=cap)
        cap = int(still)                                                     # exactly the next list's length

Scene.denoise removes the noise of such frames on the GPU: passes of a guided a-trous filter (include/qrhip.h
qr_atrous_views_async) stopped by the hit records of the same views and by the accumulator's own variance.  atrous_pass, denoise
and pt_adapt_view_variance state them in float32 numpy, operation for operation; atrous_stops is the host side of the arguments:

    views_acc = scn.pt_adaptive_views(views, w, h, min_samples=8, max_samples=8)
    _, mean = views_acc.step(8, mean=True)
    clean, var = scn.denoise(mean, scn.view_hits(views, w, h), views_acc.variance(), passes=5, plane=0.05, luma=4.0)

Scene.temporal reuses the samples of the frames before under a moving camera (include/qrhip.h qr_reproject_views_async): every
pixel of this frame's hit records is projected into the previous camera (project_to_view), the previous history is fetched there
through four bilinear taps held to the same surface, and this frame's colour is blended in.  reproject_pass states one call,
Temporal / temporal the accumulator's chain, in float32 numpy; reproject_stops is the host side of the arguments:

    acc = scn.temporal(1, w, h, plane_max=0.02)     # about one pixel's footprint, world units
    for view in camera_path:                        # float32 [1, 16] tensors
        hits = scn.view_hits(view, w, h)
        colour, var = acc.step(noisy_mean_of(view), hits, view, variance_of(view))
        clean, _ = scn.denoise(colour, hits, var, passes=5, plane=0.05, luma=4.0)

For a scene animated through hierarchy_apply, step(..., motion=, scene=) takes the package's hierarchy_motion table of the two
frames' node tables (move_hits is the step it adds: qr_reproject_moving_async) and the frame's own Scene:

    table = torch.from_numpy(qr.hierarchy_motion(nodes_prev, nodes_cur, opts, n_srf)).cuda()
    colour, var = acc.step(noisy, hits, view, motion=table, scene=scene_of_this_frame)

Light that changes on a surface that stands still (the shadow of an object that moved on) trails by the history length unless
the fetched history is held to the colours this frame shows around the pixel (clamp_box is the box, clamp_stops the block:
qr_reproject_clamped_async):

    acc = scn.temporal(1, w, h, plane_max=0.02, clamp=clamp_stops("variance", radius=1, gamma=1.0, short_len=1))
"""
import struct

import numpy as np

# qr_frame (include/qr_scene.h) as 49 little-endian 32-bit words
_F_TMAX, _F_DIR, _F_HOR, _F_VER, _F_HORA, _F_VERA = 0, 1, 4, 7, 10, 14
_F_TMIN, _F_ORG, _F_FSAA, _F_W, _F_H = 24, 25, 30, 31, 32
_F_CLAMP, _F_CMASK, _F_FLAGS = 18, 19, 28
PROP_GAMMA = 0x40                                           # QR_PROP_GAMMA in qr_frame.ctx_flags


def frame_record(blob):
    """The snapshot's qr_frame as (float32 view, int32 view) of its 49 words (copies)."""
    off = struct.unpack_from("<I", blob, 4 * 10)[0]          # qr_header.off_frame
    w = np.frombuffer(blob, dtype=np.int32, count=49, offset=off).copy()
    return w.view(np.float32), w


def camera_rays(blob, sample=0):
    """Primary rays of every pixel of the snapshot's frame, row-major: float32 [H*W, 8].

    Every step is one IEEE fp32 operation (numpy float32, no fused multiply-add), in the kernel's order:
    hs = x + hor_a, vs = y + ver_a (plus the zero jitter of a non-path-traced frame), the six products hor * hs and
    ver * vs, their sums, then + dir.  tmin / tmax are the frame's t_min / t_max.  `sample`: which FSAA sub-sample
    (0 .. 2^fsaa - 1) of a frame captured with anti-aliasing."""
    _, i = frame_record(blob)
    return view_rays(view_of(blob), int(i[_F_W]), int(i[_F_H]), blob, sample)


def view_of(blob):
    """The snapshot's own camera as a qr_view (include/qrhip.h): float32 [16] = org xyz, t_min, dir xyz, t_max, hor xyz, 0,
    ver xyz, 0 -- one row of the `views` argument of Scene.render_views."""
    f, _ = frame_record(blob)
    v = np.zeros(16, dtype=np.float32)
    v[0:3], v[3] = f[_F_ORG:_F_ORG + 3], f[_F_TMIN]
    v[4:7], v[7] = f[_F_DIR:_F_DIR + 3], f[_F_TMAX]
    v[8:11] = f[_F_HOR:_F_HOR + 3]
    v[12:15] = f[_F_VER:_F_VER + 3]
    return v


def look_at(eye, target, up, fov_deg, width, height):
    """A pinhole camera as a qr_view, float32 [16], in the engine's convention: pixel (x, y) looks along
    dir + hor * x + ver * y with dir = forward - hor * W/2 - ver * H/2, so that the centre of the frame looks at `target`;
    hor = normalize(forward x up) * s and ver = forward x hor * s with s = tan(fov/2) / (W/2): square pixels, `fov_deg` across
    the frame's width, x to the right and y downwards for a viewer whose head points along `up`.  Computed in float64 and
    rounded to float32 once.  t_min = 0, t_max = FLT_MAX."""
    eye, target, up = (np.asarray(a, dtype=np.float64).reshape(3) for a in (eye, target, up))
    if not (width >= 1 and height >= 1 and 0.0 < fov_deg < 180.0):
        raise ValueError("look_at needs width, height >= 1 and 0 < fov_deg < 180")
    fwd = target - eye
    n = np.linalg.norm(fwd)
    if not n > 0.0:
        raise ValueError("look_at: eye and target coincide")
    fwd = fwd / n
    hor = np.cross(fwd, up)
    n = np.linalg.norm(hor)
    if not n > 1e-12 * np.linalg.norm(up):
        raise ValueError("look_at: up is parallel to the viewing direction")
    hor = hor / n
    ver = np.cross(fwd, hor)
    s = np.tan(np.radians(fov_deg) * 0.5) / (width * 0.5)
    hor, ver = hor * s, ver * s
    d = fwd - hor * (width * 0.5) - ver * (height * 0.5)
    v = np.zeros(16, dtype=np.float32)
    v[0:3], v[3] = eye, 0.0
    v[4:7], v[7] = d, np.finfo(np.float32).max
    v[8:11] = hor
    v[12:15] = ver
    return v


def view_rays(view, width, height, blob, sample=0):
    """camera_rays for a view (view_of, look_at) and a frame size: the primary rays Scene.render_views computes for the
    width x height frame of `view`, row-major, float32 [H*W, 8], in the kernel's fp32 operation order.  FSAA and its sample
    offsets are the snapshot's (`blob`); tmin / tmax are the view's (tmax +inf stays: the ray API takes it as FLT_MAX)."""
    v = np.asarray(view, dtype=np.float32).reshape(16)
    f, i = frame_record(blob)
    fsaa, w, h = int(i[_F_FSAA]), int(width), int(height)
    if not 0 <= sample < (1 << fsaa):
        raise ValueError(f"sample must be 0..{(1 << fsaa) - 1} for fsaa {fsaa}")
    if w < 1 or h < 1:
        raise ValueError("width and height must be at least 1")
    x = np.tile(np.arange(w, dtype=np.float32), h)
    y = np.repeat(np.arange(h, dtype=np.float32), w)
    if fsaa == 0:
        ai = np.zeros(w * h, dtype=np.int64)
    elif fsaa == 1:
        ai = (np.tile(np.arange(w), h) & 1) * 2 + sample
    else:
        ai = np.full(w * h, sample, dtype=np.int64)
    zero = np.float32(0.0)
    hs = (x + f[_F_HORA:_F_HORA + 4][ai]) + zero
    vs = (y + f[_F_VERA:_F_VERA + 4][ai]) + zero
    out = np.empty((w * h, 8), dtype=np.float32)
    for k in range(3):
        a = v[8 + k] * hs
        b = v[12 + k] * vs
        out[:, 4 + k] = (a + b) + v[4 + k]
        out[:, k] = v[k]
    out[:, 3] = v[3]
    out[:, 7] = v[7]
    return out


def _cvt_near(x):
    """the kernel's cvt_near: round to nearest even; outside the int32 range (and NaN) 0x80000000"""
    f = np.rint(x)
    ok = (f >= np.float32(-2147483648.0)) & (f < np.float32(2147483648.0))
    return np.where(ok, np.where(ok, f, np.float32(0)).astype(np.int64), np.int64(-2147483648))


def pack_colors(rgb, blob):
    """The frame's output step (qr_kernel.hpp XX_end) for the linear colours Scene.shade gives for camera_rays(blob, sample=k),
    k = 0 .. 2^fsaa - 1: rgb float32 [H*W, 3] (fsaa 0) or [ns, H*W, 3] (sample k in row k).  Returns the uint32 [H, W] frame.

    Every step is one IEEE fp32 operation (numpy float32, no fused operations), in the kernel's order: clamp1 of each sample
    (x < 1 ? x : 1); the FSAA reduce -- every sample * 0.5, samples (0, 1) and (2, 3) added, and for 4x once more * 0.5 and the
    two sums added; the square root when ctx_flags holds QR_PROP_GAMMA; * clamp, round to nearest even, & cmask, packed as
    r << 16 | g << 8 | b."""
    f, i = frame_record(blob)
    fsaa, w, h = int(i[_F_FSAA]), int(i[_F_W]), int(i[_F_H])
    ns = 1 << fsaa
    c = np.asarray(rgb)
    if c.ndim == 2:
        c = c[None]
    if c.dtype != np.float32 or c.shape != (ns, w * h, 3):
        raise ValueError(f"rgb must be float32 [{w * h}, 3] or [{ns}, {w * h}, 3] for this snapshot (fsaa {fsaa}), got "
                         f"{c.dtype} {list(c.shape)}")
    one, half = np.float32(1.0), np.float32(0.5)
    c = np.where(c < one, c, one)                           # clamp1: NaN gives 1 as well
    if fsaa >= 1:
        c = c * half
        c = np.stack([c[0] + c[1]] if fsaa == 1 else [c[0] + c[1], c[2] + c[3]])
    if fsaa >= 2:
        c = c * half
        c = (c[0] + c[1])[None]
    c = c[0]
    if int(i[_F_FLAGS]) & PROP_GAMMA:
        c = np.sqrt(c)
    c = c * f[_F_CLAMP]
    q = _cvt_near(c) & np.int64(np.uint32(i[_F_CMASK]))
    p = (q[:, 0] << 16) | (q[:, 1] << 8) | q[:, 2]
    return (p & np.int64(0xFFFFFFFF)).astype(np.uint32).reshape(h, w)


# ---- view accumulation (include/qrhip.h qr_render_views_mean_async; Scene.render_views_mean): the contract in numpy ----

def reduce_colors(rgb, blob):
    """The first half of the output step, up to and including the FSAA reduce, for linear colours of any number of pixels:
    rgb float32 [ns, P, 3] (sample k in row k; ns = 2^fsaa of the snapshot) or [P, 3] at fsaa 0.  Returns float32 [P, 3]: the
    linear pixel colour qr_render_views_mean_async adds per view.  One IEEE fp32 operation per step, as in pack_colors: clamp1
    of each sample, every sample * 0.5 and samples (0, 1), (2, 3) added, for 4x once more * 0.5 and the two sums added."""
    _, i = frame_record(blob)
    fsaa = int(i[_F_FSAA])
    ns = 1 << fsaa
    c = np.asarray(rgb)
    if c.ndim == 2:
        c = c[None]
    if c.dtype != np.float32 or c.ndim != 3 or c.shape[0] != ns or c.shape[2] != 3:
        raise ValueError(f"rgb must be float32 [P, 3] or [{ns}, P, 3] for this snapshot (fsaa {fsaa}), got {c.dtype} {list(c.shape)}")
    one, half = np.float32(1.0), np.float32(0.5)
    c = np.where(c < one, c, one)                           # clamp1: NaN gives 1 as well
    if fsaa >= 1:
        c = c * half
        c = np.stack([c[0] + c[1]] if fsaa == 1 else [c[0] + c[1], c[2] + c[3]])
    if fsaa >= 2:
        c = c * half
        c = (c[0] + c[1])[None]
    return c[0]


def pack_linear(lin, blob, width, height):
    """The second half of the output step for linear pixel colours lin, float32 [height * width, 3] (or [height, width, 3]): the
    square root when ctx_flags holds QR_PROP_GAMMA, * clamp, round to nearest even, & cmask, packed as r << 16 | g << 8 | b.
    Returns the uint32 [height, width] frame.  pack_linear(reduce_colors(rgb, blob), blob, W, H) is pack_colors(rgb, blob)."""
    f, i = frame_record(blob)
    w, h = int(width), int(height)
    c = np.asarray(lin)
    if c.dtype != np.float32 or c.size != w * h * 3 or c.shape[-1] != 3:
        raise ValueError(f"lin must be float32 [{w * h}, 3], got {c.dtype} {list(c.shape)}")
    c = c.reshape(w * h, 3)
    if int(i[_F_FLAGS]) & PROP_GAMMA:
        with np.errstate(invalid="ignore"):
            c = np.sqrt(c)
    c = c * f[_F_CLAMP]
    q = _cvt_near(c) & np.int64(np.uint32(i[_F_CMASK]))
    p = (q[:, 0] << 16) | (q[:, 1] << 8) | q[:, 2]
    return (p & np.int64(0xFFFFFFFF)).astype(np.uint32).reshape(h, w)


def mean_of_views(colours, blob, width, height, scale, start=None):
    """The contract of qr_render_views_mean_async in numpy: colours is the per-view list of reduce_colors results (float32
    [height * width, 3] each, in view order).  s = colours[0] (start=None) or `start` (the sum of an earlier call: the resumed
    launch), then s = s + c for every remaining view -- one fp32 add per channel and view, in order.  Returns (frame, sum):
    sum float32 [height, width, 3], frame = pack_linear(sum * float32(scale)) (one fp32 multiply), uint32 [height, width]."""
    w, h = int(width), int(height)
    cs = [np.asarray(c) for c in colours]
    for c in cs:
        if c.dtype != np.float32 or c.shape != (w * h, 3):
            raise ValueError(f"every view's colours must be float32 [{w * h}, 3], got {c.dtype} {list(c.shape)}")
    if start is None:
        if not cs:
            raise ValueError("mean_of_views needs a view or a start")
        s, rest = cs[0].copy(), cs[1:]
    else:
        s = np.asarray(start)
        if s.dtype != np.float32 or s.size != w * h * 3:
            raise ValueError(f"start must be float32 [{h}, {w}, 3], got {s.dtype} {list(s.shape)}")
        s, rest = s.reshape(w * h, 3).copy(), cs
    for c in rest:
        s = s + c
    frame = pack_linear(s * np.float32(scale), blob, w, h)
    return frame, s.reshape(h, w, 3)


def jitter_view(view, dx, dy):
    """The view shifted by a sub-pixel offset: pixel (x, y) of the result looks where (x + dx, y + dy) of `view` looks --
    dir + hor * dx + ver * dy, computed in float64 and rounded to float32 once; everything else kept.  An offset of (0, 0)
    returns the same bits.  N such copies through Scene.render_views_mean supersample a frame beyond the scene's FSAA."""
    v = np.asarray(view, dtype=np.float32).reshape(16).copy()
    if dx == 0 and dy == 0:
        return v
    d, hor, ver = (v[a:a + 3].astype(np.float64) for a in (4, 8, 12))
    v[4:7] = d + hor * np.float64(dx) + ver * np.float64(dy)
    return v


def thin_lens_views(eye, target, up, fov_deg, width, height, aperture, focus, n, seed):
    """n pinhole views (float32 [n, 16]) that sample a thin lens: look_at(eye, target, up, fov_deg, width, height) with the
    origin moved by an offset on the disc of diameter `aperture` around `eye`, perpendicular to the viewing direction (uniform
    over its area, numpy default_rng(seed): deterministic), and `dir` moved by -offset / focus, so that all views see the same
    point of the plane at distance `focus` (along the viewing direction) through the same pixel: that plane stays sharp in
    their mean (Scene.render_views_mean), everything else blurs with the aperture.  Float64, rounded to float32 once.
    aperture = 0 gives n copies of look_at, bit for bit."""
    base = look_at(eye, target, up, fov_deg, width, height)
    if not (n >= 0 and aperture >= 0.0 and focus > 0.0):
        raise ValueError("thin_lens_views needs n >= 0, aperture >= 0 and focus > 0")
    out = np.tile(base, (int(n), 1))
    if aperture == 0:
        return out
    eye, target, up = (np.asarray(a, dtype=np.float64).reshape(3) for a in (eye, target, up))
    fwd = (target - eye) / np.linalg.norm(target - eye)
    uh = np.cross(fwd, up)
    uh = uh / np.linalg.norm(uh)
    uv = np.cross(fwd, uh)
    s = np.tan(np.radians(fov_deg) * 0.5) / (width * 0.5)
    d = fwd - uh * s * (width * 0.5) - uv * s * (height * 0.5)
    rng = np.random.default_rng(seed)
    r = 0.5 * aperture * np.sqrt(rng.uniform(0.0, 1.0, int(n)))
    phi = rng.uniform(0.0, 2.0 * np.pi, int(n))
    off = (r * np.cos(phi))[:, None] * uh + (r * np.sin(phi))[:, None] * uv
    out[:, 0:3] = eye + off
    out[:, 4:7] = d - off / np.float64(focus)
    return out


# ---- path-traced views (include/qrhip.h qr_pt_views_async; Scene.pt_views): the generator and its seeds in numpy ----

def pt_seeds(width, height, samples_per_pixel=1):
    """The seed plane a path-traced accumulation starts from (qr_scene_set_pt, qr_pt_views_reset; the reference's
    rt_Scene::reset_pseed): uint32 [width * height * samples_per_pixel].  A 48-bit LCG, x <- (x * 25214903917 + 11) mod 2^48
    from x = 1, walks over the slots and each slot keeps the low 32 bits of its x; pixel (x, y), sample k has slot
    (y * width + x) * samples_per_pixel + k.  Every view of a Scene.pt_views state starts from this same plane (plane 0 of
    its block of the state tensor)."""
    n = int(width) * int(height) * int(samples_per_pixel)
    if n < 1:
        raise ValueError("pt_seeds needs width, height and samples_per_pixel >= 1")
    m48 = np.uint64((1 << 48) - 1)
    # a[k - 1], c[k - 1]: k steps are x -> a * x + c (mod 2^48; uint64 products wrap mod 2^64, which 2^48 divides)
    a = np.array([25214903917], dtype=np.uint64)
    c = np.array([11], dtype=np.uint64)
    with np.errstate(over="ignore"):
        while len(a) < n:
            am, cm = a[-1], c[-1]
            a, c = np.concatenate([a, (a * am) & m48]), np.concatenate([c, (a * cm + c) & m48])
        x = (a[:n] + c[:n]) & m48
    return (x & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def pt_random(state):
    """One step of the path tracer's generator (qr_shade.hpp pt_random) on uint32 states of any shape: returns (new states,
    the numbers drawn as float32 in [0, 1)): s <- s * 214013 + 2531011 (mod 2^32), value = ((s >> 8) & 0xFFFFFF) / 2^24.
    A sample's first two draws are its horizontal and vertical jitter ("Order of draws")."""
    s = np.asarray(state, dtype=np.uint32)
    with np.errstate(over="ignore"):
        s = (s.astype(np.uint64) * np.uint64(214013) + np.uint64(2531011)).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    s = s.astype(np.uint32)
    v = ((s >> np.uint32(8)) & np.uint32(0xFFFFFF)).astype(np.float32) / np.float32(16777216.0)
    return s, v


# ---- path-traced rays (include/qrhip.h qr_pt_rays_async; Scene.pt_rays): the jitter and the rays of a sample in numpy ----

def _pt_tent(u):
    """the renderer's tent filter on numbers in [0, 1) (qr_kernel.hpp, tracer.cpp:1218-1285): float32 in [-0.5, 0.5)"""
    one, two, half = np.float32(1.0), np.float32(2.0), np.float32(0.5)
    u = np.asarray(u, dtype=np.float32)
    u = u + u
    with np.errstate(invalid="ignore"):
        a = np.sqrt(u) - one
        b = one - np.sqrt(two - u)
    return np.where(u < one, a, b) * half


def pt_jitter(states):
    """The two numbers a path-traced sample draws before its walk ("Order of draws", item 1), through the tent
    filter: returns (states after the two draws, h, v), uint32 and float32 of the shape of `states`.  Horizontal first.  Per
    number u = u + u; a = u < 1 ? sqrt(u) - 1 : 1 - sqrt(2 - u); a = a * 0.5 -- one IEEE fp32 operation per step.  A frame
    with FSAA halves both once more (pt_view_rays); caller rays (qr_pt_rays_async with a spread) do not."""
    s, u = pt_random(states)
    h = _pt_tent(u)
    s, u = pt_random(s)
    v = _pt_tent(u)
    return s, h, v


def spread_rays(rays, spread, h, v):
    """The rays qr_pt_rays_async traces for `rays` float32 [N, 8] with `spread` float32 [N, 8] (du xyz, pad, dv xyz, pad) and
    the jitter h, v (float32 [N], pt_jitter): per component a = du * h; b = dv * v; a = a + b; dir = dir + a, one IEEE fp32
    operation per step.  Origin, tmin and tmax are kept.  Returns a new float32 [N, 8] array."""
    r = np.array(rays, dtype=np.float32, copy=True)
    sp = np.asarray(spread, dtype=np.float32)
    h, v = np.asarray(h, dtype=np.float32), np.asarray(v, dtype=np.float32)
    if r.ndim != 2 or r.shape[1] != 8 or sp.shape != r.shape or h.shape != r.shape[:1] or v.shape != r.shape[:1]:
        raise ValueError("spread_rays needs rays [N, 8], spread [N, 8], h [N] and v [N]")
    for k in range(3):
        a = sp[:, k] * h
        b = sp[:, 4 + k] * v
        a = a + b
        r[:, 4 + k] = r[:, 4 + k] + a
    return r


def pt_view_rays(view, width, height, blob, states):
    """The rays ONE path-traced sample of a view traces (Scene.pt_views; set_pt + render on the snapshot rewritten to the view):
    returns (rays float32 [W * H * ns, 8] in slot order -- slot (y * W + x) * ns + k, ns = 2^fsaa of the snapshot --, states
    after the two jitter draws, uint32 [W * H * ns]).  `states`: the slots' generator states before the sample (pt_seeds(W, H,
    ns) for the first).  view_rays' arithmetic with hs = (x + hor_a) + hr, vs = (y + ver_a) + vr, where hr, vr are pt_jitter's
    values, halved once more when the snapshot has FSAA."""
    vw = np.asarray(view, dtype=np.float32).reshape(16)
    f, i = frame_record(blob)
    fsaa, w, h = int(i[_F_FSAA]), int(width), int(height)
    ns = 1 << fsaa
    if w < 1 or h < 1:
        raise ValueError("width and height must be at least 1")
    st = np.asarray(states, dtype=np.uint32)
    if st.shape != (w * h * ns,):
        raise ValueError(f"states must be uint32 [{w * h * ns}] (width * height * samples per pixel)")
    xi = np.repeat(np.tile(np.arange(w), h), ns)
    x = xi.astype(np.float32)
    y = np.repeat(np.arange(h, dtype=np.float32), w * ns)
    k = np.tile(np.arange(ns), w * h)
    if fsaa == 0:
        ai = np.zeros(w * h, dtype=np.int64)
    elif fsaa == 1:
        ai = (xi & 1) * 2 + k
    else:
        ai = k
    st, hr, vr = pt_jitter(st)
    if fsaa != 0:
        hr, vr = hr * np.float32(0.5), vr * np.float32(0.5)
    hs = (x + f[_F_HORA:_F_HORA + 4][ai]) + hr
    vs = (y + f[_F_VERA:_F_VERA + 4][ai]) + vr
    out = np.empty((w * h * ns, 8), dtype=np.float32)
    for c in range(3):
        a = vw[8 + c] * hs
        b = vw[12 + c] * vs
        out[:, 4 + c] = (a + b) + vw[4 + c]
        out[:, c] = vw[c]
    out[:, 3] = vw[3]
    out[:, 7] = vw[7]
    return out, st


# ---- adaptive path-traced rays (include/qrhip.h qr_pt_adapt_rays_async; Scene.pt_adaptive): the rule and the update in numpy ----

def _pt_adapt_state(state):
    st = np.ascontiguousarray(state)
    if st.ndim != 2 or st.shape[0] != 8 or st.dtype.itemsize != 4:
        raise ValueError("an adaptive state is [8, N] of 32-bit words")
    return st.view(np.uint32)


def pt_adapt_open(state, min_samples, max_samples, tol2):
    """The stop rule of qr_pt_adapt_rays_async on a state [8, N] (uint32 or int32): bool [N], True where the ray would take one
    more sample.  Per ray, with m = plane 4 (unsigned) and M2 = planes 5..7 (float32):
        lim = float32(m) * float32(m - 1);  lim = lim * tol2                 (two fp32 multiplies; m - 1 wraps for m = 0, unused)
        conv = M2r <= lim and M2g <= lim and M2b <= lim                      (a NaN never converges)
        take = m < max_samples and (m < min_samples or m < 2 or not conv)"""
    st = _pt_adapt_state(state)
    m = st[4]
    with np.errstate(over="ignore", invalid="ignore"):
        lim = m.astype(np.float32) * (m - np.uint32(1)).astype(np.float32)
        lim = lim * np.float32(tol2)
        m2 = st[5:8].view(np.float32)
        conv = (m2[0] <= lim) & (m2[1] <= lim) & (m2[2] <= lim)
    return (m < np.uint32(max_samples)) & ((m < np.uint32(min_samples)) | (m < np.uint32(2)) | ~conv)


def pt_adapt_fold(state, cols, rngs, min_samples, max_samples, tol2):
    """The specification of one qr_pt_adapt_rays_async call, given what every candidate sample WOULD give: cols float32 [N, S, 3],
    the colours of the S consecutive samples of every ray from the state's generator word, and rngs uint32 [N, S], the generator
    word after each.  A ray's candidate sequence does not depend on how many it takes -- it keeps a prefix -- so this is exact.
    Before each candidate the rule (pt_adapt_open) decides; a ray that takes it is updated, one IEEE fp32 operation per step:
        m = m + 1;  o = 1 / float32(m);  u = 1 - o
        per channel:  d1 = col - mean;  a = col * o;  b = mean * u;  mean = a + b;  d2 = col - mean;  p = d1 * d2;  M2 = M2 + p
        plane 0 = the generator word after the sample
    Returns (state' uint32 [8, N], rgb float32 [N, 3] = the means of every ray, open = the number of rays the rule would still
    let take a sample on state')."""
    st = _pt_adapt_state(state).copy()
    n = st.shape[1]
    cols = np.asarray(cols, dtype=np.float32)
    rngs = np.asarray(rngs, dtype=np.uint32)
    if cols.ndim != 3 or cols.shape[0] != n or cols.shape[2] != 3 or rngs.shape != cols.shape[:2]:
        raise ValueError("pt_adapt_fold needs cols [N, S, 3] and rngs [N, S] for a state [8, N]")
    one = np.float32(1.0)
    mean, m2 = st[1:4].view(np.float32), st[5:8].view(np.float32)
    taken = np.zeros(n, dtype=np.int64)                 # candidates taken so far in this call: a prefix
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(cols.shape[1]):
            t = np.nonzero(pt_adapt_open(st, min_samples, max_samples, tol2) & (taken == s))[0]
            if len(t) == 0:
                break
            taken[t] += 1
            m = st[4, t] + np.uint32(1)
            o = one / m.astype(np.float32)
            u = one - o
            for ch in range(3):
                c, mu = cols[t, s, ch], mean[ch, t]
                d1 = c - mu
                a = c * o
                b = mu * u
                mu = a + b
                d2 = c - mu
                p = d1 * d2
                mean[ch, t] = mu
                m2[ch, t] = m2[ch, t] + p
            st[4, t] = m
            st[0, t] = rngs[t, s]
    rgb = np.ascontiguousarray(mean.T).copy()
    return st, rgb, int(pt_adapt_open(st, min_samples, max_samples, tol2).sum())


def pt_adapt_open_list(state, min_samples, max_samples, tol2):
    """The specification of qr_pt_adapt_open_list_async: the indices of the open rays of a state [8, N], ascending, uint32 [count]"""
    return np.flatnonzero(pt_adapt_open(state, min_samples, max_samples, tol2)).astype(np.uint32)


def pt_adapt_fold_list(state, index, count, cols, rngs, min_samples, max_samples, tol2, cap=None):
    """The specification of one qr_pt_adapt_list_rays_async call: pt_adapt_fold restricted to the listed columns.  index: ray
    indices (distinct); the first min(cap, count) entries are served (cap=None: no bound), entries >= N are skipped.  cols
    [N, S, 3] and rngs [N, S] are indexed by RAY, not by list position, as for pt_adapt_fold.
    Returns (state' uint32 [8, N] -- unlisted columns as they were --, rgb float32 [N, 3] with NaN in the rows of unlisted rays,
    which the call does not write, open = the number of LISTED rays the rule would still let take a sample on state')."""
    st = _pt_adapt_state(state).copy()
    n = st.shape[1]
    cols = np.asarray(cols, dtype=np.float32)
    rngs = np.asarray(rngs, dtype=np.uint32)
    if cols.ndim != 3 or cols.shape[0] != n or cols.shape[2] != 3 or rngs.shape != cols.shape[:2]:
        raise ValueError("pt_adapt_fold_list needs cols [N, S, 3] and rngs [N, S] for a state [8, N]")
    ix = np.asarray(index).reshape(-1).astype(np.int64)
    served = min(int(count), len(ix)) if cap is None else min(int(count), int(cap), len(ix))
    ix = ix[:max(served, 0)]
    ix = ix[(ix >= 0) & (ix < n)]
    if len(np.unique(ix)) != len(ix):
        raise ValueError("the entries of a list must be distinct")
    sub, srgb, op = pt_adapt_fold(st[:, ix], cols[ix], rngs[ix], min_samples, max_samples, tol2)
    st[:, ix] = sub
    rgb = np.full((n, 3), np.nan, dtype=np.float32)
    rgb[ix] = srgb
    return st, rgb, op


# ---- adaptive path-traced views (include/qrhip.h qr_pt_adapt_views_async; Scene.pt_adaptive_views): the outputs in numpy ----
# The fold itself is pt_adapt_fold on every state[j]: one view's block is an adaptive ray state of `slots` columns.

def _pt_adapt_view_state(state):
    st = np.ascontiguousarray(state)
    if st.ndim == 2:
        st = st[None]
    if st.ndim != 3 or st.shape[1] != 8 or st.dtype.itemsize != 4:
        raise ValueError("an adaptive view state is [N, 8, slots] (or [8, slots]) of 32-bit words")
    return st.view(np.uint32)


def pt_adapt_view_counts(state, spp):
    """The sample heat map of qr_pt_adapt_views_async (counts_dev) for a state [N, 8, slots] (or one view's [8, slots]): int32
    [N, H * W], per pixel the sum of plane 4 over its `spp` slots (slot = pixel * spp + k)."""
    st = _pt_adapt_view_state(state)
    spp = int(spp)
    if spp < 1 or st.shape[2] % spp != 0:
        raise ValueError("the slots of a view are pixels * samples per pixel")
    m = st[:, 4].astype(np.int64).reshape(st.shape[0], st.shape[2] // spp, spp)
    return m.sum(axis=2).astype(np.int32)


def pt_adapt_view_frames(state, blob, width, height):
    """The frames and means of qr_pt_adapt_views_async for a state [N, 8, slots] (or one view's [8, slots]) of the snapshot
    `blob` (its FSAA, gamma, clamp and mask): the output step on planes 1..3 -- clamp1 and the FSAA reduce (reduce_colors),
    then gamma, scale, round, mask and pack (pack_linear).  Returns (frames uint32 [N, height, width], mean float32
    [N, height, width, 3])."""
    st = _pt_adapt_view_state(state)
    _, i = frame_record(blob)
    ns = 1 << int(i[_F_FSAA])
    w, h = int(width), int(height)
    if st.shape[2] != w * h * ns:
        raise ValueError(f"the state holds {st.shape[2]} slots per view, the frame {w * h * ns}")
    frames = np.empty((st.shape[0], h, w), dtype=np.uint32)
    mean = np.empty((st.shape[0], h, w, 3), dtype=np.float32)
    for j in range(st.shape[0]):
        rgb = st[j, 1:4].view(np.float32).T.reshape(w * h, ns, 3).transpose(1, 0, 2)       # [ns, P, 3]: sample k in row k
        lin = reduce_colors(np.ascontiguousarray(rgb), blob)
        mean[j] = lin.reshape(h, w, 3)
        frames[j] = pack_linear(lin, blob, w, h)
    return frames, mean


# ---- hit records (include/qrhip.h qr_hit; Scene.hits, Scene.view_hits): float32 [..., 12] = pos xyz, t, nrm xyz, id, alb xyz, mat ----

def hit_fields(h):
    """Typed VIEWS (no copies) of hit records h, a float32 [..., 12] torch tensor or numpy array: the tuple
    (pos [..., 3], t [...], nrm [..., 3], id [...], alb [..., 3], mat [...]) with id and mat viewed as int32
    (id = surface << 1 | side, mat = snapshot material index; both -1 on a miss)."""
    if h.shape[-1] != 12 or "float32" not in str(h.dtype):
        raise ValueError(f"hit records are float32 [..., 12], got {h.dtype} {list(h.shape)}")
    if isinstance(h, np.ndarray):
        i = h.view(np.int32)
    else:
        import torch
        i = h.view(torch.int32)
    return h[..., 0:3], h[..., 3], h[..., 4:7], i[..., 7], h[..., 8:11], i[..., 11]


def _secondary(hits, dirs, eps):
    import torch
    pos, _, _, hid, _, _ = hit_fields(hits)
    n = hits.shape[0]
    out = torch.empty((n, 8), dtype=torch.float32, device=hits.device)
    out[:, 0:3] = pos
    out[:, 3] = eps
    out[:, 4:7] = dirs
    tmin = out[:, 3]
    out[:, 7] = torch.where(hid >= 0, torch.full_like(tmin, float("inf")), tmin)      # a miss: tmax = tmin, the interval is empty
    return out


def offset_rays(hits, dirs, eps):
    """Secondary rays that leave hit points: hits float32 [N, 12] (Scene.hits), dirs float32 [N, 3] on the same device.
    Returns float32 [N, 8] qr_ray rows: origin = pos, direction = dirs, tmin = eps (the step off the surface, in units of
    |dir|: no self-exclusion in the ray API), tmax = +inf; rows of misses get tmax = tmin and hit nothing.
    A helper for a host's own passes with one direction per hit (probes, a bounce); NOT the renderer's bit-exact children: those
    start at tmin 0 with the originating surface excluded, which the ray API does not offer.  Ambient occlusion and other fans of
    many directions per hit need no rays at all: Scene.occlusion / Scene.view_occlusion / Scene.hit_occlusion trace them from
    the hit in one launch (fan_rays states what they trace)."""
    return _secondary(hits, dirs, eps)


def reflect_rays(rays, hits, eps):
    """Mirror rays: rays float32 [N, 8] (the rays that gave `hits`), hits float32 [N, 12].  Direction d - 2 (d . n) n with the
    incoming direction d as given (not normalised) and the record's normal n, in plain float32 torch arithmetic; origin,
    tmin = eps and the rows of misses as offset_rays.  NOT the renderer's bit-exact reflection children (it normalises d first,
    in its own operation order, and excludes the originating surface instead of stepping off it)."""
    _, _, nrm, _, _, _ = hit_fields(hits)
    d = rays[:, 4:7]
    dn = (d * nrm).sum(dim=1, keepdim=True)
    return _secondary(hits, d - 2.0 * dn * nrm, eps)


# ---- occlusion fans (include/qrhip.h qr_fan_*_async; Scene.occlusion, Scene.view_occlusion, Scene.hit_occlusion) ----

def fan_frame(nrm, spin=None):
    """The frame of a framed fan (include/qrhip.h "Framed fans"): nrm float32 [..., 3], spin float32 [..., 2] = (c, sn) or None
    (which is (1, 0) through the same operations), numpy arrays or torch tensors on one device.  Returns (u [..., 3],
    v [..., 3], valid bool [...]).  The branchless orthonormal basis of Duff et al. 2017, every operation float32, in this order:
        s  = nz < 0 ? -1 : 1                       (-0.0 and NaN give +1)
        a  = -1 / (s + nz)
        b  = (nx * ny) * a
        t  = (1 + ((s * nx) * nx) * a,  s * b,  -(s * nx))
        bt = (b,  s + (ny * ny) * a,  -ny)
        u  = t * c + bt * sn        per component: two products, then one add
        v  = bt * c - t * sn        per component: two products, then one subtract
    valid iff every word of nrm, u and v has |w| <= FLT_MAX.  For a unit normal and a unit spin (u, v, nrm) is orthonormal to
    a few ulp and right-handed: u x v = nrm."""
    if nrm.shape[-1] != 3 or "float32" not in str(nrm.dtype):
        raise ValueError(f"nrm must be float32 [..., 3], got {nrm.dtype} {list(nrm.shape)}")
    if spin is not None and (tuple(spin.shape) != tuple(nrm.shape[:-1]) + (2,) or "float32" not in str(spin.dtype)):
        raise ValueError(f"spin must be float32 {list(nrm.shape[:-1]) + [2]}, got {spin.dtype} {list(spin.shape)}")
    flt_max = float(np.finfo(np.float32).max)
    nx, ny, nz = nrm[..., 0], nrm[..., 1], nrm[..., 2]
    if isinstance(nrm, np.ndarray):
        const = lambda x: np.full(nz.shape, x, dtype=np.float32)
        where, stack, absf = np.where, (lambda c: np.stack(c, axis=-1)), np.abs
        ctx = np.errstate(invalid="ignore", over="ignore", divide="ignore")
    else:
        import contextlib
        import torch
        const = lambda x: torch.full_like(nz, x)
        where, stack, absf = torch.where, (lambda c: torch.stack(c, dim=-1)), torch.abs
        ctx = contextlib.nullcontext()
    with ctx:
        one = const(1.0)
        s = where(nz < 0, const(-1.0), one)
        a = const(-1.0) / (s + nz)
        b = (nx * ny) * a
        sx = s * nx
        t = (one + (sx * nx) * a, s * b, -sx)
        bt = (b, s + (ny * ny) * a, -ny)
        c, sn = (one, const(0.0)) if spin is None else (spin[..., 0], spin[..., 1])
        u = stack([t[i] * c + bt[i] * sn for i in range(3)])
        v = stack([bt[i] * c - t[i] * sn for i in range(3)])
        valid = ((absf(nrm) <= flt_max) & (absf(u) <= flt_max) & (absf(v) <= flt_max)).all(-1)
    return u, v, valid


def fan_rays(hits, dirs, eps, reach=float("inf"), flip=False, frame=False, spin=None):
    """The rays an occlusion fan traces, as a composition of the ray API: hits float32 [N, 12] (Scene.hits, or view_hits
    reshaped), dirs float32 [K, 3] or [K, 4] (the fourth column is ignored), numpy arrays or torch tensors on one device.
    Returns (rays float32 [N, K, 8], traced bool [N, K]).

    For hit i and direction d = dirs[k]:  dot = (nrm.x * d.x + nrm.y * d.y) + nrm.z * d.z -- three float32 products and two
    float32 adds in that order, nothing fused.  flip=False: the ray is (pos, eps, d, reach) and it is traced iff the record is
    a hit (id >= 0) and 0 < dot: the renderer's rule for lights; otherwise the surface itself closes the direction.
    flip=True: the ray is (pos, eps, -d, reach) where dot < 0 and (pos, eps, d, reach) otherwise, and every direction of a
    hit is traced.  A NaN dot decides as these comparisons do (closed without flip, traced as d with it).  Rows of misses are
    filled the same way and never traced.  Direction k of element i is OPEN iff it is traced and Scene.occluded answers False
    for its ray; Scene.occlusion counts the open directions (-1 for a miss) and sets bit k & 31 of mask plane k >> 5.

    frame=True (framed fans): the table is in the hit's own frame, (u, v, valid) = fan_frame(nrm, spin) with spin float32 [N, 2]
    or None.  dot = z = dirs[k, 2]: the table's own cosine.  (x', y', z') is the row, under flip mirrored to (-x, -y, -z) where
    z < 0; the ray is (pos, eps, (u * x' + v * y') + n * z', reach) -- per component three float32 products and two adds in
    that order -- and it is traced iff the record is a hit, its frame is valid and (flip or 0 < z).  A NaN z decides as these
    comparisons do."""
    pos, _, nrm, hid, _, _ = hit_fields(hits)
    if hits.ndim != 2:
        raise ValueError(f"hits must be [N, 12], got {list(hits.shape)}")
    if dirs.ndim != 2 or dirs.shape[1] not in (3, 4) or "float32" not in str(dirs.dtype):
        raise ValueError(f"dirs must be float32 [K, 3] or [K, 4], got {dirs.dtype} {list(dirs.shape)}")
    if spin is not None and not frame:
        raise ValueError("spin needs frame=True")
    n, k = hits.shape[0], dirs.shape[0]
    d = dirs[:, 0:3]
    if frame:
        u, v, valid = fan_frame(nrm, spin)
    if isinstance(hits, np.ndarray):
        where, full = np.where, (lambda shape, dt: np.empty(shape, dtype=dt))
        f32, bool_ = np.float32, np.bool_
        ctx = np.errstate(invalid="ignore", over="ignore")
    else:
        import contextlib
        import torch
        where, full = torch.where, (lambda shape, dt: torch.empty(shape, dtype=dt, device=hits.device))
        f32, bool_ = torch.float32, torch.bool
        ctx = contextlib.nullcontext()
    with ctx:
        rays = full((n, k, 8), f32)
        traced = full((n, k), bool_)
        rays[:, :, 0:3] = pos[:, None, :]
        rays[:, :, 3] = eps
        rays[:, :, 7] = reach
        hit = (hid >= 0)[:, None]
        if frame:
            z = d[:, 2]
            loc = where((z < 0)[:, None], -d, d) if flip else d                         # [K, 3]: the row as it is traced
            for i in range(3):
                p0 = u[:, i:i + 1] * loc[:, 0][None, :]
                p1 = v[:, i:i + 1] * loc[:, 1][None, :]
                p2 = nrm[:, i:i + 1] * loc[:, 2][None, :]
                rays[:, :, 4 + i] = (p0 + p1) + p2
            traced[:, :] = hit & valid[:, None] if flip else hit & valid[:, None] & (0 < z)[None, :]
            return rays, traced
        p0 = nrm[:, 0:1] * d[:, 0][None, :]
        p1 = nrm[:, 1:2] * d[:, 1][None, :]
        p2 = nrm[:, 2:3] * d[:, 2][None, :]
        dot = (p0 + p1) + p2                                    # [N, K]
        if flip:
            neg = (dot < 0)[:, :, None]
            rays[:, :, 4:7] = where(neg, -d[None, :, :], d[None, :, :])
            traced[:, :] = hit
        else:
            rays[:, :, 4:7] = d[None, :, :]
            traced[:, :] = hit & (0 < dot)
    return rays, traced


def fan_bits(mask, k):
    """The mask planes of an occlusion fan as booleans: mask int32 or uint32 [ceil(k / 32), ...] (numpy array or torch tensor, as
    Scene.occlusion(..., mask=True) returns it) -> bool [..., k]: entry j is bit j & 31 of plane j >> 5."""
    k = int(k)
    if k < 1 or mask.ndim < 1 or mask.shape[0] != (k + 31) // 32:
        raise ValueError(f"a mask of {k} directions has {(k + 31) // 32} planes, got shape {list(mask.shape)}")
    cols = [((mask[j >> 5] >> (j & 31)) & 1) != 0 for j in range(k)]
    if isinstance(mask, np.ndarray):
        return np.stack(cols, axis=-1)
    import torch
    return torch.stack(cols, dim=-1)


def sphere_dirs(n):
    """n directions on a Fibonacci sphere, float32 [n, 3], unit length: with i = arange(n) + 0.5, z = 1 - 2 i / n,
    phi = i * pi * (3 - sqrt(5)), s = sqrt(1 - z^2), the direction is (s cos phi, s sin phi, z).  Computed in float64 and
    rounded to float32 once.  A direction table for Scene.occlusion: with flip=True every point sees all n mirrored into its
    own hemisphere; without, about half of them lie above any surface."""
    n = int(n)
    if n < 1:
        raise ValueError("sphere_dirs needs n >= 1")
    i = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    s = np.sqrt(1.0 - z * z)
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1).astype(np.float32)


def cosine_dirs(n):
    """n directions of a cosine-distributed hemisphere about local +z with their weights, float32 [n, 4]: with i = arange(n) +
    0.5, r = sqrt(i / n), phi = i * pi * (3 - sqrt(5)), a row is (r cos phi, r sin phi, sqrt(1 - r^2), 1 / n).  Computed in
    float64 and rounded to float32 once.  A table for the framed fans (frame=True): every direction lies above the surface, so
    none is wasted, and the density is the cosine, so the plain sum (cosine=False) of Scene.gather is the irradiance estimate,
    acc.w is 1 where nothing is refused, and open / n of Scene.occlusion is cosine-weighted ambient occlusion."""
    n = int(n)
    if n < 1:
        raise ValueError("cosine_dirs needs n >= 1")
    i = np.arange(n, dtype=np.float64) + 0.5
    r = np.sqrt(i / n)
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - r * r), np.full(n, 1.0 / n)], axis=1).astype(np.float32)


def spins(shape, seed):
    """Spin planes for the framed fans: float32 shape + [2] = (cos a, sin a) with the angles a drawn by
    np.random.default_rng(seed).uniform(0, 2 pi, shape); cos and sin are taken in float64 and rounded to float32 once.  One
    turn of the table about the normal per element: neighbouring elements no longer share their K directions."""
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(x) for x in shape)
    a = np.random.default_rng(seed).uniform(0.0, 2.0 * np.pi, shape)
    return np.stack([np.cos(a), np.sin(a)], axis=-1).astype(np.float32)


# ---- gather fans (include/qrhip.h qr_gather_*_async; Scene.gather, Scene.view_gather, Scene.hit_gather) ----

def gather_fold(hits, dirs, colours, flip=False, cosine=False, start=None, frame=False, spin=None):
    """The sum a gather fan takes, in float32 numpy: hits float32 [N, 12], dirs float32 [K, 4] (direction xyz, weight) or
    [K, 3] (weight 1.0), colours float32 [N, K, 3]: entry (i, k) is what Scene.shade returns for fan_rays' ray (i, k); entries
    of untraced rays are not read.  Returns (gather float32 [N, 4], count int32 [N]).

    For hit i, k = 0 .. K-1 in table order, with fan_rays' dot = (nrm.x * d.x + nrm.y * d.y) + nrm.z * d.z and its traced rule
    (flip=False: the record is a hit and 0 < dot; flip=True: the record is a hit): an untraced direction does nothing; a traced
    one has wgt = weight, with cosine=True wgt = weight * c where c = dot without flip and (-dot if dot < 0 else dot) with it,
    then acc.rgb = acc.rgb + colour * wgt (one float32 multiply, then one float32 add), acc.w = acc.w + wgt, count += 1.
    acc and count start from zero, or from start = (gather, count) of an earlier call: a table cut into consecutive chunks and
    folded one after the other gives the bits of one fold.  A record that is no hit (id < 0) gets a zero row and count -1,
    whatever `start` holds.

    frame=True (framed fans; spin float32 [N, 2] or None): the traced rule is framed fan_rays' and dot = z = dirs[k, 2], so
    with cosine=True wgt = weight * z, or weight * (-z if z < 0 else z) with flip.  A hit whose frame is invalid
    (fan_frame) traces nothing and gets a zero row and count 0, whatever `start` holds."""
    hits, dirs, colours = np.asarray(hits), np.asarray(dirs), np.asarray(colours)
    spin = None if spin is None else np.asarray(spin)
    _, traced = fan_rays(hits, dirs, np.float32(0.0), flip=flip, frame=frame, spin=spin)
    n, k = traced.shape
    if colours.dtype != np.float32 or colours.shape != (n, k, 3):
        raise ValueError(f"colours must be float32 [{n}, {k}, 3], got {colours.dtype} {list(colours.shape)}")
    _, _, nrm, hid, _, _ = hit_fields(hits)
    weight = dirs[:, 3] if dirs.shape[1] == 4 else np.ones(k, dtype=np.float32)
    if start is None:
        acc, cnt = np.zeros((n, 4), dtype=np.float32), np.zeros(n, dtype=np.int32)
    else:
        acc, cnt = np.asarray(start[0]), np.asarray(start[1])
        if acc.dtype != np.float32 or acc.shape != (n, 4) or cnt.dtype != np.int32 or cnt.shape != (n,):
            raise ValueError(f"start must be (float32 [{n}, 4], int32 [{n}])")
        acc, cnt = acc.copy(), cnt.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(k):
            t = traced[:, j]
            wgt = np.full(n, weight[j], dtype=np.float32)
            if cosine:
                if frame:
                    dot = np.full(n, dirs[j, 2], dtype=np.float32)
                else:
                    dot = (nrm[:, 0] * dirs[j, 0] + nrm[:, 1] * dirs[j, 1]) + nrm[:, 2] * dirs[j, 2]
                wgt = wgt * (np.where(dot < 0, -dot, dot) if flip else dot)
            prod = colours[:, j, :] * wgt[:, None]
            acc[t, 0:3] = (acc[:, 0:3] + prod)[t]
            acc[t, 3] = (acc[:, 3] + wgt)[t]
            cnt[t] += 1
    if frame:
        bad = ~fan_frame(nrm, spin)[2]
        acc[bad] = 0.0
        cnt[bad] = 0
    miss = hid < 0
    acc[miss] = 0.0
    cnt[miss] = -1
    return acc, cnt


# ---- hit layers (include/qrhip.h qr_layer_*_async; Scene.trace_layers, Scene.view_layers) ----

def next_rays(rays, t, ids):
    """The rays that continue behind a hit: rays float32 [N, 8], t float32 [N] and ids int32 [N] as Scene.trace answers for them
    (or the last plane of Scene.trace_layers), numpy arrays or torch tensors on one device.  Returns a new float32 [N, 8]:
    where ids >= 0 the same ray with tmin = t, bit for bit, no epsilon -- a hit counts when tmin < t' < tmax and the ray API
    has no self-exclusion, so its closest hit is the NEXT surface along the ray; where the ray ended (ids < 0) tmin = tmax
    (+inf taken as FLT_MAX): an empty interval, so that every later call answers a miss with t = tmax.  Origin, direction and
    tmax are kept.  k1 layers, then k2 layers on next_rays(rays, t[k1 - 1], ids[k1 - 1]), are one call with k1 + k2."""
    if rays.ndim != 2 or rays.shape[1] != 8 or "float32" not in str(rays.dtype):
        raise ValueError(f"rays must be float32 [N, 8], got {rays.dtype} {list(rays.shape)}")
    if tuple(t.shape) != (rays.shape[0],) or tuple(ids.shape) != (rays.shape[0],) or "float32" not in str(t.dtype):
        raise ValueError(f"t (float32) and ids must be [N] for rays [N, 8], got {list(t.shape)} and {list(ids.shape)}")
    flt_max = float(np.finfo(np.float32).max)
    if isinstance(rays, np.ndarray):
        out = rays.copy()
        tmax = rays[:, 7]
        end = np.where(tmax > np.float32(flt_max), np.float32(flt_max), tmax)
        out[:, 3] = np.where(ids >= 0, t, end)
    else:
        import torch
        out = rays.clone()
        tmax = rays[:, 7]
        end = torch.where(tmax > flt_max, torch.full_like(tmax, flt_max), tmax)
        out[:, 3] = torch.where(ids >= 0, t, end)
    return out


def layers_of(trace, rays, k):
    """What Scene.trace_layers computes, as a composition of closest-hit queries: trace is any callable with Scene.trace's
    signature on numpy arrays -- trace(rays float32 [M, 8]) -> (t float32 [M], ids int32 [M]), a miss answered as t = tmax
    (FLT_MAX for +inf), id = -1 -- rays float32 [N, 8] (numpy), 1 <= k.  Returns (count int32 [N], t float32 [k, N], ids int32
    [k, N]).

    Layer 0 is trace(rays); layer j + 1 is trace(next_rays(layer j's rays, t_j, ids_j)): the same ray with tmin = t_j, bit for
    bit.  A ray ends at its first miss: from that layer on its planes hold t = tmax (FLT_MAX for +inf), id = -1 -- what trace
    answers for next_rays' empty interval, so ended rays are not handed to trace again -- and count is the number of hits
    found, 0..k."""
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    k = int(k)
    if rays.ndim != 2 or rays.shape[1] != 8 or k < 1:
        raise ValueError(f"layers_of needs rays [N, 8] and k >= 1, got {list(rays.shape)} and k = {k}")
    n = rays.shape[0]
    flt_max = np.finfo(np.float32).max
    end = np.where(rays[:, 7] > flt_max, flt_max, rays[:, 7]).astype(np.float32)
    t = np.tile(end, (k, 1))
    ids = np.full((k, n), -1, dtype=np.int32)
    cur = rays
    alive = np.arange(n)
    for j in range(k):
        if len(alive) == 0:
            break
        tj, ij = trace(cur)
        tj, ij = np.asarray(tj, dtype=np.float32), np.asarray(ij, dtype=np.int32)
        t[j, alive], ids[j, alive] = tj, ij
        hit = ij >= 0
        cur = next_rays(cur, tj, ij)[hit]
        alive = alive[hit]
    return (ids >= 0).sum(axis=0).astype(np.int32), t, ids


# ---- guided a-trous filter (include/qrhip.h qr_atrous_views_async; Scene.atrous, Scene.denoise) ----

ATROUS_NORMAL, ATROUS_PLANE, ATROUS_LUMA, ATROUS_DEMODULATE, ATROUS_MODULATE = 1, 2, 4, 8, 16      # QR_ATROUS_* flags
ATROUS_MAX_STEP = 64                                                                               # QR_ATROUS_MAX_STEP
ATROUS_H = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], dtype=np.float32)                       # the 1-D kernel: binary fractions


def _stop_number(x, what):
    """a stop of atrous_stops and upsample_stops as float32: ValueError for what float32 does not convert and for what is not a
    finite float32 above 0"""
    try:
        v = np.float32(x)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a number") from None
    if not (v > 0 and np.isfinite(v)):
        raise ValueError(f"{what} must be a finite float32 above 0")
    return v


def _normal_power(normal_power):
    """(is the normal stop on?, normal_sq): None is no stop, a power of two 1..128 is sent as its log2"""
    if normal_power is None:
        return False, 0
    if isinstance(normal_power, bool) or not isinstance(normal_power, (int, np.integer)) or normal_power not in (1, 2, 4, 8, 16, 32, 64, 128):
        raise ValueError("normal_power must be None or a power of two, 1..128")
    return True, int(normal_power).bit_length() - 1


def atrous_stops(normal_power=128, plane=None, luma=None, luma_eps=1e-6, demodulate=False, modulate=False, albedo_floor=1 / 256):
    """The host side of Scene.atrous' arguments: (flags, normal_sq, sigma_z, sigma_l2, eps_l, alb_floor) as qr_atrous_params
    takes them.  normal_power: None (no normal stop) or a power of two 1..128, sent as its log2; plane: sigma_z or None; luma:
    the tolerance in standard deviations or None, sigma_l2 = float32(luma) * float32(luma); a stop that is off sends 1.0.
    Raises ValueError for anything else."""
    normal, normal_sq = _normal_power(normal_power)
    flags = ATROUS_NORMAL if normal else 0
    sigma_z = sigma_l2 = np.float32(1.0)
    if plane is not None:
        sigma_z = _stop_number(plane, "plane")
        flags |= ATROUS_PLANE
    if luma is not None:
        t = _stop_number(luma, "luma")
        with np.errstate(over="ignore", under="ignore"):
            sigma_l2 = _stop_number(t * t, "luma squared")
        flags |= ATROUS_LUMA
    eps_l, alb_floor = _stop_number(luma_eps, "luma_eps"), _stop_number(albedo_floor, "albedo_floor")
    if demodulate:
        flags |= ATROUS_DEMODULATE
    if modulate:
        flags |= ATROUS_MODULATE
    return flags, normal_sq, sigma_z, sigma_l2, eps_l, alb_floor


def _atrous_args(colour, variance, hits):
    colour, hits = np.asarray(colour), np.asarray(hits)
    if colour.dtype != np.float32 or colour.ndim not in (3, 4) or colour.shape[-1] not in (3, 4):
        raise ValueError(f"colour must be float32 [N, H, W, 3|4] or [H, W, 3|4], got {colour.dtype} {list(colour.shape)}")
    lead = colour.shape[:-1]
    if hits.dtype != np.float32 or hits.shape != lead + (12,):
        raise ValueError(f"hits must be float32 {list(lead) + [12]}, got {hits.dtype} {list(hits.shape)}")
    if variance is not None:
        variance = np.asarray(variance)
        if variance.dtype != np.float32 or variance.shape != lead:
            raise ValueError(f"variance must be float32 {list(lead)}, got {variance.dtype} {list(variance.shape)}")
    return colour, variance, hits


def atrous_pass(colour, variance, hits, step, flags=0, normal_sq=0, sigma_z=1.0, sigma_l2=1.0, eps_l=1e-6, alb_floor=1 / 256,
                weights=None):
    """The specification of one qr_atrous_views_async pass in float32 numpy, every operation elementwise so that it rounds once:
    colour float32 [N, H, W, C] (or [H, W, C]; C 3 or 4), variance float32 [N, H, W] or None, hits float32 [N, H, W, 12]
    (qr_hit records), step 1..ATROUS_MAX_STEP, flags of ATROUS_*, the rest as qr_atrous_params.  Returns (colour', variance' or
    None), new arrays.

    Per pixel p (include/qrhip.h has the full text): with ATROUS_DEMODULATE every colour is first divided, channels 0..2, by
    a = alb if alb > alb_floor else alb_floor of its own record (id < 0: not divided); lum = (r * 0.2126 + g * 0.7152) + b * 0.0722.
    id_p < 0: colour as read and variance pass through.  Otherwise the taps dy = -2..2 outer, dx = -2..2 inner, q = p + (dx, dy) *
    step, h = H[dy + 2] * H[dx + 2]: the centre is taken with w = h; another tap is skipped outside the frame or when id_q < 0;
    else w = h, times the NORMAL stop max(0, n_p . n_q) squared normal_sq times, times the PLANE stop 1 / (1 + x * x) with
    x = |n_p . (pos_q - pos_p)| / sigma_z, times the LUMA stop 1 / (1 + (dl * dl) / (sigma_l2 * v_p + eps_l)), v_p = 1 without
    a variance; taken iff 0 < w.  sum_c += c_q * w, sum_w += w, sum_v += var_q * (w * w) in tap order; c = sum_c / sum_w,
    var = sum_v / (sum_w * sum_w); with ATROUS_MODULATE c * a_p on channels 0..2.

    weights: if a list is given, the 25 (taken bool [N, H, W], w float32 [N, H, W]) pairs are appended to it in tap order (w
    is 0 where the tap is not taken): what a test needs to evaluate the same sums in another precision."""
    f = np.float32
    colour, variance, hits = _atrous_args(colour, variance, hits)
    single = colour.ndim == 3
    if single:
        colour, hits = colour[None], hits[None]
        variance = None if variance is None else variance[None]
    step, flags, normal_sq = int(step), int(flags), int(normal_sq)
    if not 1 <= step <= ATROUS_MAX_STEP or not 0 <= normal_sq <= 7 or flags & ~31:
        raise ValueError("step must be 1..64, normal_sq 0..7, flags of ATROUS_*")
    sigma_z, sigma_l2, eps_l, alb_floor = f(sigma_z), f(sigma_l2), f(eps_l), f(alb_floor)
    if not (sigma_z > 0 and sigma_l2 > 0 and eps_l > 0 and alb_floor > 0):
        raise ValueError("sigma_z, sigma_l2, eps_l and alb_floor must be above 0")
    n, h, w, ch = colour.shape
    pos, _, nrm, ids, alb, _ = hit_fields(hits)
    hit = ids >= 0
    with np.errstate(all="ignore"):
        a = np.where(alb > alb_floor, alb, alb_floor)                       # a NaN albedo gives the floor
        a = np.where(hit[..., None], a, f(1.0))
        col = colour.copy()
        if flags & ATROUS_DEMODULATE:
            col[..., 0:3] = np.where(hit[..., None], col[..., 0:3] / a, col[..., 0:3])
        lum = (col[..., 0] * f(0.2126) + col[..., 1] * f(0.7152)) + col[..., 2] * f(0.0722)
        var = np.ones((n, h, w), dtype=f) if variance is None else variance
        den = sigma_l2 * var + eps_l
        ys, xs = np.mgrid[0:h, 0:w]
        sc, sw, sv = np.zeros((n, h, w, ch), dtype=f), np.zeros((n, h, w), dtype=f), np.zeros((n, h, w), dtype=f)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + dy * step, xs + dx * step
                ok = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                wt = np.full((n, h, w), ATROUS_H[dy + 2] * ATROUS_H[dx + 2], dtype=f)
                if dx == 0 and dy == 0:
                    take = np.ones((n, h, w), dtype=bool)
                else:
                    ok = ok[None] & (ids[:, qy, qx] >= 0)
                    if flags & ATROUS_NORMAL:
                        nq = nrm[:, qy, qx]
                        d = (nrm[..., 0] * nq[..., 0] + nrm[..., 1] * nq[..., 1]) + nrm[..., 2] * nq[..., 2]
                        d = np.where(0 < d, d, f(0.0))
                        for _ in range(normal_sq):
                            d = d * d
                        wt = wt * d
                    if flags & ATROUS_PLANE:
                        e = pos[:, qy, qx] - pos
                        d = (nrm[..., 0] * e[..., 0] + nrm[..., 1] * e[..., 1]) + nrm[..., 2] * e[..., 2]
                        x = np.abs(d) / sigma_z
                        wt = wt * (f(1.0) / (f(1.0) + x * x))
                    if flags & ATROUS_LUMA:
                        dl = lum - lum[:, qy, qx]
                        wt = wt * (f(1.0) / (f(1.0) + (dl * dl) / den))
                    take = ok & (0 < wt)
                wt = np.where(take, wt, f(0.0))
                if weights is not None:
                    weights.append((take, wt))
                sc = np.where(take[..., None], sc + col[:, qy, qx] * wt[..., None], sc)
                sw = np.where(take, sw + wt, sw)
                sv = np.where(take, sv + var[:, qy, qx] * (wt * wt), sv)
        out = sc / sw[..., None]
        vout = sv / (sw * sw)
        if flags & ATROUS_MODULATE:
            out[..., 0:3] = out[..., 0:3] * a
        out = np.where(hit[..., None], out, col).astype(f)
        vout = None if variance is None else np.where(hit, vout, variance).astype(f)
    if single:
        return out[0], None if vout is None else vout[0]
    return out, vout


def denoise(colour, variance, hits, passes=5, albedo=False, **stops):
    """The specification of Scene.denoise: `passes` (1..7) atrous_pass calls with step = 1, 2, 4, ..., each fed the colour and
    variance of the one before; with albedo=True ATROUS_DEMODULATE is set on the first pass and ATROUS_MODULATE on the last.
    stops: normal_power, plane, luma, luma_eps, albedo_floor as atrous_stops takes them.  Returns (colour, variance or None)."""
    passes = int(passes)
    if not 1 <= passes <= 7:
        raise ValueError("passes must be 1..7")
    if "demodulate" in stops or "modulate" in stops:
        raise ValueError("denoise sets demodulate and modulate itself (albedo=True)")
    c, v = colour, variance
    for k in range(passes):
        flags, nsq, sz, sl2, el, af = atrous_stops(demodulate=albedo and k == 0, modulate=albedo and k == passes - 1, **stops)
        c, v = atrous_pass(c, v, hits, 1 << k, flags, nsq, sz, sl2, el, af)
    return c, v


def pt_adapt_view_variance(state, spp, unknown=1.0):
    """The specification of qr_pt_adapt_views_variance_async (PtAdaptiveViews.variance) for a state [N, 8, slots] (or one view's
    [8, slots]): float32 [N, H * W].  Per slot, m = plane 4 (unsigned): where 2 <= m, s = (M2r + M2g) + M2b, s = s if 0 < s else
    0, v = s / ((float32(m) * float32(m - 1)) * 3); elsewhere v = unknown.  Per pixel (v_0 + v_1 + ... in slot order) * (1 /
    (spp * spp)): the channel-mean variance of the pixel's FSAA-reduced mean, its slots taken as independent."""
    f = np.float32
    st = _pt_adapt_view_state(state)
    spp = int(spp)
    if spp not in (1, 2, 4) or st.shape[2] % spp != 0:
        raise ValueError("the slots of a view are pixels * samples per pixel, 1, 2 or 4")
    m = st[:, 4]
    m2 = st[:, 5:8].view(f)
    with np.errstate(all="ignore"):
        s = (m2[:, 0] + m2[:, 1]) + m2[:, 2]
        s = np.where(0 < s, s, f(0.0))
        v = s / ((m.astype(f) * (m - np.uint32(1)).astype(f)) * f(3.0))
        v = np.where(m >= np.uint32(2), v, f(unknown)).astype(f)
        v = v.reshape(st.shape[0], st.shape[2] // spp, spp)
        acc = v[..., 0]
        for k in range(1, spp):
            acc = acc + v[..., k]
        return (acc * (f(1.0) / f(spp * spp))).astype(f)


# ---- temporal reprojection (include/qrhip.h qr_reproject_views_async; Scene.reproject, Scene.temporal) ----

REPROJ_DEMODULATE = 1                                                                               # QR_REPROJ_DEMODULATE
REPROJ_NAN = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]                            # the NaN the call writes
_REPROJ_FIELDS = ("flags", "off_x", "off_y", "normal_min", "plane_max", "min_weight", "alpha_min", "alpha_mom_min", "max_len",
                  "var_min_len", "unknown", "alb_floor")


def reproject_stops(normal_min=0.9, plane_max=None, min_weight=0.01, alpha_min=0.05, alpha_mom_min=0.2, max_len=32, var_min_len=4,
                    unknown=1.0, albedo_floor=1 / 256, demodulate=False, off=(0, 0)):
    """The host side of Scene.reproject's arguments: a dict of qr_reproject_params' fields (flags, off_x, off_y, normal_min,
    plane_max, min_weight, alpha_min, alpha_mom_min, max_len, var_min_len, unknown, alb_floor), the floats as float32, that
    reproject_pass takes as keywords.  The defaults are starting points, not tuned: normal_min 0.9; plane_max should be about one
    pixel's footprint in world units at the scene's depth (None: +inf, the plane test only closes NaN); min_weight 0.01; and
    SVGF's customary alpha_min 0.05, alpha_mom_min 0.2, max_len 32, var_min_len 4.  off: the sub-pixel offset of the records'
    rays, the frame's (hor_a[0], ver_a[0]); (0, 0) without FSAA.  Raises ValueError for what the call would refuse."""
    f = np.float32

    def number(x, what):            # its own copy: any finite value, no bool or str; through _stop_number the call cost 0.5 us more
        try:
            v = f(x)
        except (TypeError, ValueError):
            raise ValueError(f"{what} must be a number") from None
        if isinstance(x, (bool, str)):
            raise ValueError(f"{what} must be a number")
        return v
    try:
        off_x, off_y = off
    except (TypeError, ValueError):
        raise ValueError("off must be a pair of numbers") from None
    p = dict(flags=REPROJ_DEMODULATE if demodulate else 0, off_x=number(off_x, "off"), off_y=number(off_y, "off"),
             normal_min=number(normal_min, "normal_min"), plane_max=f(np.inf) if plane_max is None else number(plane_max, "plane_max"),
             min_weight=number(min_weight, "min_weight"), alpha_min=number(alpha_min, "alpha_min"),
             alpha_mom_min=number(alpha_mom_min, "alpha_mom_min"), max_len=number(max_len, "max_len"),
             var_min_len=number(var_min_len, "var_min_len"), unknown=number(unknown, "unknown"),
             alb_floor=number(albedo_floor, "albedo_floor"))
    _reproject_params(p)
    return p


def _reproject_params(p):
    """the refusals of qr_reproject_views_async that concern the parameters alone, as ValueError"""
    if int(p["flags"]) & ~REPROJ_DEMODULATE:
        raise ValueError("flags must be of REPROJ_*")
    if not (np.isfinite(p["off_x"]) and np.isfinite(p["off_y"])):
        raise ValueError("off must be finite")
    if np.isnan(p["normal_min"]):
        raise ValueError("normal_min must be a number, not NaN")
    if not (p["plane_max"] > 0 and p["alb_floor"] > 0):
        raise ValueError("plane_max and albedo_floor must be above 0")
    if not p["min_weight"] >= 0:
        raise ValueError("min_weight must be 0 or more")
    if not (0 <= p["alpha_min"] <= 1 and 0 <= p["alpha_mom_min"] <= 1):
        raise ValueError("alpha_min and alpha_mom_min must be 0..1")
    if not (p["max_len"] >= 1 and p["var_min_len"] >= 1):
        raise ValueError("max_len and var_min_len must be 1 or more")


CLAMP_MINMAX, CLAMP_VARIANCE, CLAMP_SHORTEN = 1, 2, 4                                               # QR_CLAMP_*
CLAMP_MAX_RADIUS = 3                                                                                # QR_CLAMP_MAX_RADIUS


def clamp_stops(mode="variance", radius=1, gamma=1.0, short_len=None):
    """The clamp block of Scene.reproject(clamp=) / reproject_pass(clamp=) as a dict of qr_clamp_params' fields (flags, radius,
    gamma, short_len; include/qrhip.h qr_reproject_clamped_async): the fetched history colour is held to a box of this frame's
    colours in the (2 * radius + 1)^2 neighbourhood of the pixel.  mode: "variance" (the mean +- gamma standard deviations) or
    "minmax" (the neighbourhood's minimum and maximum; gamma is not used).  radius 1..CLAMP_MAX_RADIUS.  short_len: None, or the
    history length (>= 1) a pixel whose history was moved is cut to (CLAMP_SHORTEN).  Starting points, not tuned.  Raises
    ValueError for what the call would refuse."""
    modes = {"variance": CLAMP_VARIANCE, "minmax": CLAMP_MINMAX}
    if not isinstance(mode, str) or mode not in modes:
        raise ValueError('mode must be "variance" or "minmax"')
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)):
        raise ValueError(f"radius must be an integer, 1..{CLAMP_MAX_RADIUS}")
    for x, what in ((gamma, "gamma"), (short_len, "short_len")):
        if x is not None and (isinstance(x, (bool, str)) or not isinstance(x, (int, float, np.integer, np.floating))):
            raise ValueError(f"{what} must be a number")
    c = dict(flags=modes[mode] | (0 if short_len is None else CLAMP_SHORTEN), radius=int(radius), gamma=np.float32(gamma),
             short_len=np.float32(1.0 if short_len is None else short_len))
    _clamp_params(c)
    return c


def _clamp_params(c):
    """the refusals of qr_reproject_clamped_async that concern the clamp block alone, as ValueError; returns (flags, radius,
    gamma, short_len)"""
    try:
        flags, radius, gamma, short_len = int(c["flags"]), int(c["radius"]), np.float32(c["gamma"]), np.float32(c["short_len"])
        extra = set(c) - {"flags", "radius", "gamma", "short_len"}
    except (TypeError, KeyError, ValueError):
        raise ValueError("clamp must be None or a dict of flags, radius, gamma and short_len (clamp_stops)") from None
    if extra:
        raise ValueError("clamp must be None or a dict of flags, radius, gamma and short_len (clamp_stops)")
    if flags & (CLAMP_MINMAX | CLAMP_VARIANCE) not in (CLAMP_MINMAX, CLAMP_VARIANCE):
        raise ValueError("a clamp is CLAMP_MINMAX or CLAMP_VARIANCE: exactly one of the two")
    if flags & ~(CLAMP_MINMAX | CLAMP_VARIANCE | CLAMP_SHORTEN):
        raise ValueError("clamp flags must be of CLAMP_*")
    if not 1 <= radius <= CLAMP_MAX_RADIUS:
        raise ValueError(f"radius must be 1..{CLAMP_MAX_RADIUS}")
    if not gamma >= 0:
        raise ValueError("gamma must be 0 or more")
    if np.isnan(short_len) or (flags & CLAMP_SHORTEN and not short_len >= 1):
        raise ValueError("short_len must not be NaN, and 1 or more with CLAMP_SHORTEN")
    return flags, radius, gamma, short_len


def clamp_box(col, valid, flags, radius, gamma=1.0):
    """The box of the clamp step (include/qrhip.h qr_reproject_clamped_async) in float32 numpy, operation for operation: col
    float32 [N, H, W, C], the colours after the read step; valid bool [N, H, W] (id >= 0).  Returns (lo, hi [N, H, W, C], n
    [N, H, W]): per pixel over the valid neighbours within `radius` inside the frame of the same view, a row's partials first (i
    ascending), then the rows' folded (j ascending).  CLAMP_VARIANCE: mu -+ gamma * sqrt(max(0, t2 / n - mu * mu)); CLAMP_MINMAX:
    lo = v if v < lo else lo, hi = v if hi < v else hi from (+inf, -inf), per row and again over the rows.  A pixel without a
    valid neighbour (n = 0: it is a miss itself) gets what the statements give; the call never looks at it."""
    f = np.float32
    r = int(radius)
    n, h, w, ch = col.shape
    colp = np.zeros((n, h + 2 * r, w + 2 * r, ch), dtype=f)
    colp[:, r:r + h, r:r + w] = col
    okp = np.zeros((n, h + 2 * r, w + 2 * r), dtype=bool)
    okp[:, r:r + h, r:r + w] = valid
    cnt = np.zeros((n, h, w), dtype=np.int64)
    with np.errstate(all="ignore"):
        if flags & CLAMP_VARIANCE:
            t1, t2 = np.zeros((n, h, w, ch), dtype=f), np.zeros((n, h, w, ch), dtype=f)
            for j in range(-r, r + 1):
                r1, r2 = np.zeros((n, h, w, ch), dtype=f), np.zeros((n, h, w, ch), dtype=f)
                for i in range(-r, r + 1):
                    v, ok = colp[:, r + j:r + j + h, r + i:r + i + w], okp[:, r + j:r + j + h, r + i:r + i + w]
                    cnt += ok
                    r1 = np.where(ok[..., None], r1 + v, r1)
                    r2 = np.where(ok[..., None], r2 + v * v, r2)
                t1, t2 = t1 + r1, t2 + r2
            nf = cnt.astype(f)[..., None]
            mu = t1 / nf
            var = t2 / nf - mu * mu
            var = np.where(0 < var, var, f(0.0))
            wd = f(gamma) * np.sqrt(var)
            return (mu - wd).astype(f), (mu + wd).astype(f), cnt
        lo, hi = np.full((n, h, w, ch), np.inf, dtype=f), np.full((n, h, w, ch), -np.inf, dtype=f)
        for j in range(-r, r + 1):
            rl, rh = np.full((n, h, w, ch), np.inf, dtype=f), np.full((n, h, w, ch), -np.inf, dtype=f)
            for i in range(-r, r + 1):
                v, ok = colp[:, r + j:r + j + h, r + i:r + i + w], okp[:, r + j:r + j + h, r + i:r + i + w]
                cnt += ok
                rl = np.where(ok[..., None] & (v < rl), v, rl)
                rh = np.where(ok[..., None] & (rh < v), v, rh)
            lo = np.where(rl < lo, rl, lo)
            hi = np.where(hi < rh, rh, hi)
        return lo, hi, cnt


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def project_to_view(view, pos, off=(0, 0), dtype=np.float32):
    """The projection of qr_reproject_views_async, operation for operation: where world-space points pos [..., 3] fall in the
    frame of `view` (a qr_view [16], or [..., 16] broadcast against pos).  With A = hor x ver, B = ver x dir, C = dir x hor, det
    = (dir.x * A.x + dir.y * A.y) + dir.z * A.z and e = pos - org: den = e . A, nu = e . B, nv = e . C in that association, fx =
    nu / den - off[0], fy = nv / den - off[1], front = (0 < den and 0 < det) or (den < 0 and det < 0).  Returns (xy [..., 2],
    front [...]): pixel (x, y)'s own ray gives (x, y) to rounding; a point behind the eye is not front.  dtype: float32 is the
    call's arithmetic; float64 evaluates the same text in double precision."""
    f = np.dtype(dtype).type
    v, pos = np.asarray(view).astype(f), np.asarray(pos).astype(f)
    org, d, hor, ver = v[..., 0:3], v[..., 4:7], v[..., 8:11], v[..., 12:15]
    with np.errstate(all="ignore"):
        A, B, C = _cross(hor, ver), _cross(ver, d), _cross(d, hor)
        det = _dot(d, A)
        e = pos - org
        den, nu, nv = _dot(e, A), _dot(e, B), _dot(e, C)
        fx, fy = nu / den - f(off[0]), nv / den - f(off[1])
        front = ((0 < den) & (0 < det)) | ((den < 0) & (det < 0))
    return np.stack([fx, fy], axis=-1), front


def _motion_table(motion):
    """the motion table of reproject_pass / move_hits: float32 [n, 12], n >= 1 (ValueError otherwise)"""
    m = np.asarray(motion)
    if m.dtype != np.float32 or m.ndim != 2 or m.shape[1] != 12 or m.shape[0] < 1:
        raise ValueError(f"motion must be float32 [n, 12] with n >= 1, got {m.dtype} {list(m.shape)}")
    return m


def move_hits(hits, motion):
    """The move step of qr_reproject_moving_async in float32 numpy, operation for operation: hits float32 [..., 12] (qr_hit
    records), motion float32 [n, 12] (row s = the three quads r0 r1 r2 of surface record s).  Returns (pos' [..., 3], nrm'
    [..., 3], listed [...]): with s = id >> 1, pos'.k = ((rk.x * pos.x + rk.y * pos.y) + rk.z * pos.z) + rk.w and nrm'.k =
    (rk.x * nrm.x + rk.y * nrm.y) + rk.z * nrm.z (not renormalised); listed is false for a miss (id < 0) and for s >= n, whose
    pos' and nrm' are NaN: such a pixel gets a fresh entry."""
    m = _motion_table(motion)
    pos, _, nrm, ids, _, _ = hit_fields(np.asarray(hits))
    listed = (ids >= 0) & ((ids >> 1) < len(m))
    r = m[np.where(listed, ids >> 1, 0)].reshape(ids.shape + (3, 4))
    with np.errstate(all="ignore"):
        mp = ((r[..., 0] * pos[..., None, 0] + r[..., 1] * pos[..., None, 1]) + r[..., 2] * pos[..., None, 2]) + r[..., 3]
        mn = (r[..., 0] * nrm[..., None, 0] + r[..., 1] * nrm[..., None, 1]) + r[..., 2] * nrm[..., None, 2]
    return (np.where(listed[..., None], mp, REPROJ_NAN).astype(np.float32), np.where(listed[..., None], mn, REPROJ_NAN).astype(np.float32),
            listed)


def reproject_pass(colour, hits, variance=None, prev=None, flags=0, off_x=0.0, off_y=0.0, normal_min=0.9, plane_max=np.inf,
                   min_weight=0.01, alpha_min=0.05, alpha_mom_min=0.2, max_len=32.0, var_min_len=4.0, unknown=1.0, alb_floor=1 / 256,
                   taps=None, motion=None, clamp=None, moved=False):
    """The specification of one qr_reproject_views_async call in float32 numpy, every operation elementwise so that it rounds
    once: colour float32 [N, H, W, C] (or [H, W, C]; C 3 or 4), hits float32 [N, H, W, 12] (this frame's qr_hit records),
    variance float32 [N, H, W] or None, prev = None (the first frame) or (views_prev [N, 16], hits_prev [N, H, W, 12], history
    [N, H, W, 8]), the rest as qr_reproject_params (reproject_stops gives them as a dict).  Returns (history' [N, H, W, 8],
    colour' [N, H, W, C], variance' [N, H, W], coords [N, H, W, 2]), new arrays.

    Per pixel p (include/qrhip.h has the full text): c = the colour, with REPROJ_DEMODULATE and id_p >= 0 channels 0..2 divided by
    alb if alb > alb_floor else alb_floor; l = (r * 0.2126 + g * 0.7152) + b * 0.0722.  The fresh entry is (c, l, l * l, 1, 0)
    with the variance variance[p] (unknown without one); a miss, the first frame, a point not in front of the previous camera
    (project_to_view) give it, and NaN coords.  Else coords = (fx, fy), and inside -1 < fx < W, -1 < fy < H the four taps q =
    (floor(fx) + i, floor(fy) + j), j outer, b = (wx if i else 1 - wx) * (wy if j else 1 - wy), are taken where q is inside the
    frame, id_q == id_p, 1 <= len_q, normal_min < n_p . n_q, |n_p . (pos_q - pos_p)| <= plane_max and 0 < b: sw += b, sc += c_q
    * b, s1 += m1_q * b, s2 += m2_q * b, sl += len_q * b.  Where min_weight < sw: len = min(sl / sw + 1, max_len), a = 1 / len,
    c = (sc / sw) * (1 - max(a, alpha_min)) + c * max(a, alpha_min), m1 and m2 likewise with alpha_mom_min, the variance max(0,
    m2 - m1 * m1) where var_min_len <= len; elsewhere the fresh entry.

    motion: None is the static call.  A float32 [n, 12] table (qr_reproject_moving_async; move_hits is the step): pos and nrm of
    the pixel are replaced by pos' and nrm' in the projection, the normal test and the plane test -- everything else, the
    colour's demodulation by the pixel's own albedo included, is the static text; a surface beyond the table is fresh.

    clamp: None, or a clamp block (clamp_stops; qr_reproject_clamped_async): where the pixel keeps history the fetched colour hc =
    sc / sw is held per channel to the box (lo, hi) of clamp_box over this frame's demodulated colours, h2 = min(max(hc, lo), hi)
    in the header's comparison form, which takes its place in the blend; with CLAMP_SHORTEN a pixel whose history was moved
    (0 < max |h2 - hc|) has its length cut to short_len after the max_len cap.  moved=True (it needs a clamp) appends a fifth array
    [N, H, W]: -1 where the entry is fresh, else that maximum.  With the defaults the 4-tuple and the bits are the unclamped call's.

    taps: if a list is given, the four (taken bool [N, H, W], b float32 [N, H, W]) pairs are appended to it in tap order."""
    f = np.float32
    if motion is not None:
        motion = _motion_table(motion)
    if clamp is not None:
        clamp = _clamp_params(clamp)
    elif moved:
        raise ValueError("moved needs a clamp")
    colour, variance, hits = _atrous_args(colour, variance, hits)
    single = colour.ndim == 3
    if single:
        colour, hits = colour[None], hits[None]
        variance = None if variance is None else variance[None]
    par = dict(flags=int(flags), off_x=f(off_x), off_y=f(off_y), normal_min=f(normal_min), plane_max=f(plane_max),
               min_weight=f(min_weight), alpha_min=f(alpha_min), alpha_mom_min=f(alpha_mom_min), max_len=f(max_len),
               var_min_len=f(var_min_len), unknown=f(unknown), alb_floor=f(alb_floor))
    _reproject_params(par)
    n, h, w, ch = colour.shape
    if prev is not None:
        try:
            views_prev, hits_prev, hist_in = prev
        except (TypeError, ValueError):
            raise ValueError("prev must be None or (views_prev, hits_prev, history)") from None
        if single:
            views_prev, hits_prev, hist_in = (np.asarray(a)[None] for a in (views_prev, hits_prev, hist_in))
        views_prev, hits_prev, hist_in = np.asarray(views_prev), np.asarray(hits_prev), np.asarray(hist_in)
        for a, shape, what in ((views_prev, (n, 16), "views_prev"), (hits_prev, (n, h, w, 12), "hits_prev"), (hist_in, (n, h, w, 8), "history")):
            if a.dtype != f or a.shape != shape:
                raise ValueError(f"{what} must be float32 {list(shape)}, got {a.dtype} {list(a.shape)}")
    pos, _, nrm, ids, alb, _ = hit_fields(hits)
    hit = ids >= 0
    listed = hit
    if motion is not None:
        pos, nrm, listed = move_hits(hits, motion)                                   # beyond the table: fresh, as a miss is
    one, zero = f(1.0), f(0.0)
    with np.errstate(all="ignore"):
        a = np.where(alb > par["alb_floor"], alb, par["alb_floor"])                 # a NaN albedo gives the floor
        col = np.zeros((n, h, w, 4), dtype=f)
        col[..., :ch] = colour
        if par["flags"] & REPROJ_DEMODULATE:
            col[..., 0:3] = np.where(hit[..., None], col[..., 0:3] / a, col[..., 0:3])
        lum = (col[..., 0] * f(0.2126) + col[..., 1] * f(0.7152)) + col[..., 2] * f(0.0722)
        lum2 = lum * lum
        var = np.full((n, h, w), par["unknown"], dtype=f) if variance is None else variance.copy()
        hist = np.zeros((n, h, w, 8), dtype=f)
        hist[..., 0:4], hist[..., 4], hist[..., 5], hist[..., 6] = col, lum, lum2, one
        coords = np.full((n, h, w, 2), REPROJ_NAN, dtype=f)
        mv_out = np.full((n, h, w), -1.0, dtype=f)
        if prev is not None:
            xy, front = project_to_view(views_prev[:, None, None, :], pos, (par["off_x"], par["off_y"]))
            front = front & listed
            coords = np.where(front[..., None], xy, REPROJ_NAN).astype(f)
            fx, fy = xy[..., 0], xy[..., 1]
            window = front & (-one < fx) & (fx < f(w)) & (-one < fy) & (fy < f(h))
            x0, y0 = np.floor(fx), np.floor(fy)
            wx, wy = fx - x0, fy - y0
            ix, iy = np.where(window, x0, zero).astype(np.int64), np.where(window, y0, zero).astype(np.int64)
            pos_q, _, nrm_q, ids_q, _, _ = hit_fields(hits_prev)
            vi = np.arange(n)[:, None, None]
            sw, s1, s2, sl = (np.zeros((n, h, w), dtype=f) for _ in range(4))
            sc = np.zeros((n, h, w, 4), dtype=f)
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = ix + i, iy + j
                    b = (wx if i else one - wx) * (wy if j else one - wy)
                    ok = window & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                    hq, nq = hist_in[vi, qy, qx], nrm_q[vi, qy, qx]
                    ok = ok & (ids_q[vi, qy, qx] == ids) & (one <= hq[..., 6])
                    ok = ok & (par["normal_min"] < _dot(nrm, nq))
                    ok = ok & (np.abs(_dot(nrm, pos_q[vi, qy, qx] - pos)) <= par["plane_max"]) & (0 < b)
                    if taps is not None:
                        taps.append((ok, np.where(ok, b, zero)))
                    sw = np.where(ok, sw + b, sw)
                    sc = np.where(ok[..., None], sc + hq[..., 0:4] * b[..., None], sc)
                    s1 = np.where(ok, s1 + hq[..., 4] * b, s1)
                    s2 = np.where(ok, s2 + hq[..., 5] * b, s2)
                    sl = np.where(ok, sl + hq[..., 6] * b, sl)
            keep = window & (par["min_weight"] < sw)
            hc = sc / sw[..., None]
            ln = sl / sw + one
            ln = np.where(ln < par["max_len"], ln, par["max_len"])
            if clamp is not None:
                cflags, radius, gamma, short_len = clamp
                lo, hi, _ = clamp_box(col, hit, cflags, radius, gamma)
                h1 = np.where(hc < lo, lo, hc)
                h2 = np.where(hi < h1, hi, h1)
                d = np.abs(h2 - hc)
                mv = np.zeros((n, h, w), dtype=f)
                for k in range(ch):
                    mv = np.where(d[..., k] > mv, d[..., k], mv)
                if cflags & CLAMP_SHORTEN:
                    ln = np.where(0 < mv, np.where(ln < short_len, ln, short_len), ln)
                hc = h2
                mv_out = np.where(keep, mv, f(-1.0)).astype(f)
            al = one / ln
            ac = np.where(al > par["alpha_min"], al, par["alpha_min"])
            am = np.where(al > par["alpha_mom_min"], al, par["alpha_mom_min"])
            cb = hc * (one - ac)[..., None] + col * ac[..., None]
            m1 = (s1 / sw) * (one - am) + lum * am
            m2 = (s2 / sw) * (one - am) + lum2 * am
            v = m2 - m1 * m1
            v = np.where(0 < v, v, zero)
            hist[..., 0:ch] = np.where(keep[..., None], cb[..., 0:ch], col[..., 0:ch])
            hist[..., 4], hist[..., 5], hist[..., 6] = np.where(keep, m1, lum), np.where(keep, m2, lum2), np.where(keep, ln, one)
            var = np.where(keep & (par["var_min_len"] <= ln), v, var).astype(f)
    out = (hist, hist[..., 0:ch].copy(), var, coords)
    if moved:
        out = out + (mv_out,)
    return tuple(o[0] for o in out) if single else out


class Temporal:
    """The accumulator's chain in numpy (temporal(); what Scene.temporal's Temporal computes on the GPU): two history arrays it
    alternates between and copies of the last hit records and cameras.  step(colour, hits, views, variance=None, motion=None) is
    one reproject_pass (with the accumulator's clamp block, if it was given one) against the frame before -- the first frame after the start or a reset() has none -- and returns (colour,
    variance); history / length are the entry array [N, H, W, 8] and its length plane after the last step (None before the
    first); clone() continues independently."""

    def __init__(self, n_views, width, height, channels=3, clamp=None, **params):
        if channels not in (3, 4) or min(int(n_views), int(width), int(height)) < 1:
            raise ValueError("channels must be 3 or 4 and n_views, width, height at least 1")
        self.shape, self.channels, self.params = (int(n_views), int(height), int(width)), int(channels), reproject_stops(**params)
        if clamp is not None:
            _clamp_params(clamp)
        self.clamp = None if clamp is None else dict(clamp)
        self._hist = [np.zeros(self.shape + (8,), dtype=np.float32) for _ in range(2)]
        self._cur, self._hits, self._views, self.frames = 0, None, None, 0

    def reset(self):
        """the next step is a first frame"""
        self._hits = self._views = None
        self.frames = 0

    def clone(self):
        other = Temporal(self.shape[0], self.shape[2], self.shape[1], self.channels, clamp=self.clamp)
        other.params = dict(self.params)
        other._hist = [a.copy() for a in self._hist]
        other._cur, other.frames = self._cur, self.frames
        other._hits = None if self._hits is None else self._hits.copy()
        other._views = None if self._views is None else self._views.copy()
        return other

    @property
    def history(self):
        return None if self._hits is None else self._hist[self._cur]

    @property
    def length(self):
        return None if self._hits is None else self._hist[self._cur][..., 6]

    def step(self, colour, hits, views, variance=None, motion=None):
        colour, hits, views = np.asarray(colour), np.asarray(hits), np.asarray(views)
        if colour.shape != self.shape + (self.channels,) or views.shape != (self.shape[0], 16) or views.dtype != np.float32:
            raise ValueError(f"this accumulation holds float32 colour {list(self.shape) + [self.channels]} and views [{self.shape[0]}, 16]")
        prev = None if self._hits is None else (self._views, self._hits, self._hist[self._cur])
        hist, col, var, _ = reproject_pass(colour, hits, variance, prev, motion=motion, clamp=self.clamp, **self.params)
        self._cur ^= 1
        self._hist[self._cur][...] = hist
        self._hits, self._views = hits.copy(), views.copy()
        self.frames += 1
        return col, var


def temporal(n_views, width, height, channels=3, clamp=None, **params):
    """The specification of Scene.temporal: a Temporal accumulator in numpy.  params: as reproject_stops takes them; clamp: None
    or a clamp_stops block applied on every step."""
    return Temporal(n_views, width, height, channels, clamp=clamp, **params)


# ---- guided upsampling (include/qrhip.h qr_upsample_views_async; Scene.upsample) ----

UPSAMPLE_NORMAL, UPSAMPLE_PLANE, UPSAMPLE_SAME_ID, UPSAMPLE_DEMODULATE, UPSAMPLE_MODULATE = 1, 2, 4, 8, 16     # QR_UPSAMPLE_* flags
UPSAMPLE_MAX_FACTOR = 16                                                                            # QR_UPSAMPLE_MAX_FACTOR


def upsample_stops(normal_power=128, plane=None, same_id=False, demodulate=False, modulate=False, albedo_floor=1 / 256):
    """The host side of Scene.upsample's arguments: (flags, normal_sq, sigma_z, alb_floor) as qr_upsample_params takes them.
    normal_power: None (no normal stop) or a power of two 1..128, sent as its log2; plane: sigma_z in world units or None (sent
    as 1.0); same_id: a tap must be the pixel's own surface and side; demodulate / modulate: divide the coarse colour by its
    guide's albedo / multiply the result by the full pixel's.  Validates like atrous_stops: ValueError for anything else."""
    normal, normal_sq = _normal_power(normal_power)
    flags = UPSAMPLE_NORMAL if normal else 0
    alb_floor, sigma_z = _stop_number(albedo_floor, "albedo_floor"), np.float32(1.0)
    if plane is not None:
        sigma_z = _stop_number(plane, "plane")
        flags |= UPSAMPLE_PLANE
    for on, bit, what in ((same_id, UPSAMPLE_SAME_ID, "same_id"), (demodulate, UPSAMPLE_DEMODULATE, "demodulate"),
                          (modulate, UPSAMPLE_MODULATE, "modulate")):
        if not isinstance(on, (bool, np.bool_)):
            raise ValueError(f"{what} must be True or False")
        if on:
            flags |= bit
    return flags, normal_sq, sigma_z, alb_floor


def _lattice(factor, phase):
    """(s, px, py) of a lattice, validated"""
    ok = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    if not ok(factor) or not 1 <= factor <= UPSAMPLE_MAX_FACTOR:
        raise ValueError(f"factor must be an integer, 1..{UPSAMPLE_MAX_FACTOR}")
    if not (isinstance(phase, (tuple, list)) and len(phase) == 2 and ok(phase[0]) and ok(phase[1])
            and 0 <= phase[0] < factor and 0 <= phase[1] < factor):
        raise ValueError("phase must be a pair of integers (px, py), each 0..factor - 1")
    return int(factor), int(phase[0]), int(phase[1])


def coarse_size(width, height, factor, phase=(0, 0)):
    """(Wl, Hl) of the coarse frame of a width x height frame: coarse pixel (X, Y) is full pixel (factor * X + px, factor * Y + py),
    Wl = ceil((width - px) / factor), Hl = ceil((height - py) / factor).  ValueError for a factor outside 1..UPSAMPLE_MAX_FACTOR,
    a phase outside 0..factor - 1 or beyond the frame (the coarse frame would be empty)."""
    s, px, py = _lattice(factor, phase)
    if isinstance(width, bool) or isinstance(height, bool) or not isinstance(width, (int, np.integer)) \
            or not isinstance(height, (int, np.integer)) or width < 1 or height < 1:
        raise ValueError("width and height must be integers, at least 1")
    if px >= width or py >= height:
        raise ValueError(f"phase {(px, py)} lies beyond the {width} x {height} frame: the coarse frame is empty")
    return (int(width) - px + s - 1) // s, (int(height) - py + s - 1) // s


def coarse_hits(hits, factor, phase=(0, 0)):
    """The coarse G-buffer: hits[:, py::factor, px::factor] of full-frame hit records (float32 [N, H, W, 12] or [H, W, 12], a numpy
    array or a torch tensor), made contiguous -- the guides of qr_upsample_views_async, and the records to hand to hit_gather,
    hit_occlusion and the other calls that take caller-supplied records, so that the coarse light is traced from exactly the
    points it is later weighted by."""
    s, px, py = _lattice(factor, phase)
    if hits.ndim not in (3, 4) or hits.shape[-1] != 12:
        raise ValueError(f"hits must be [N, H, W, 12] or [H, W, 12], got {list(hits.shape)}")
    coarse_size(int(hits.shape[-2]), int(hits.shape[-3]), s, (px, py))
    sub = hits[..., py::s, px::s, :]
    return np.ascontiguousarray(sub) if isinstance(sub, np.ndarray) else sub.contiguous()


def coarse_view(view, factor, phase=(0, 0)):
    """The qr_view whose pixel (X, Y) looks where the full view's pixel (factor * X + px, factor * Y + py) looks: hor * factor,
    ver * factor, dir + hor * px + ver * py computed in float64 and rounded once; org, t_min and t_max are kept.  For pt_views,
    pt_adaptive_views and render_views at coarse_size.  At phase (0, 0) and a factor that is a power of two the coarse rays
    are the full view's rays bit for bit (on a scene without FSAA); otherwise they differ by a few roundings.  On a scene with
    FSAA the scene's sample offsets scale with hor and ver: a coarse sample then spreads over `factor` full pixels, and the
    guide stays sample 0's full record."""
    s, px, py = _lattice(factor, phase)
    v = np.array(view, dtype=np.float32).reshape(16)
    d, hor, ver = (v[k:k + 3].astype(np.float64) for k in (4, 8, 12))
    v[4:7] = d + hor * px + ver * py
    v[8:11] = hor * s
    v[12:15] = ver * s
    return v


def upsample_pass(colour_lo, variance_lo, hits, factor, phase=(0, 0), flags=0, normal_sq=0, sigma_z=1.0, alb_floor=1 / 256, taps=None):
    """The specification of qr_upsample_views_async in float32 numpy, every operation elementwise so that it rounds once:
    colour_lo float32 [N, Hl, Wl, C] (or [Hl, Wl, C]; C 3 or 4), variance_lo float32 [N, Hl, Wl] or None, hits float32
    [N, H, W, 12] -- the FULL frame's records, (Wl, Hl) = coarse_size(W, H, factor, phase) --, flags of UPSAMPLE_*, the rest
    as qr_upsample_params.  Returns (colour [N, H, W, C], variance [N, H, W] or None, weight [N, H, W]), new arrays.

    Per full pixel p = (x, y) (include/qrhip.h has the full text): X0 = floor_div(x - px, s), rx = (x - px) - X0 * s,
    wx = float(rx) / float(s), rows likewise; taps j = 0, 1 outer, i = 0, 1 inner at Q = (X0 + i, Y0 + j) with the guide G = the
    full record at (s * Q.x + px, s * Q.y + py) and b the bilinear weight.  A coarse colour is read divided by max(alb_G,
    alb_floor) under DEMODULATE where id_G >= 0.  A miss pixel takes inside miss taps with g = 1; a hit pixel inside hit taps
    (of its own id under SAME_ID) with g = the NORMAL stop times the PLANE stop.  Stage 1: w = b * g, taken iff 0 < w, colour =
    sum(c * w) / sum(w), variance = sum(var * (w * w)) / (sum(w) * sum(w)), weight = sum(w).  Stage 2, when stage 1 took nothing:
    w = g, weight = +0.0.  Stage 3, when stage 2 took nothing: the nearest coarse pixel (X0 + (2 * rx >= s), clamped), weight =
    -1.0.  MODULATE multiplies channels 0..2 by max(alb_p, alb_floor) where id_p >= 0.

    taps: if a list is given, the four (eligible bool [N, H, W], b float32 [H, W], g float32 [N, H, W], qy [H, W], qx [H, W])
    tuples are appended in tap order (qy, qx clipped into the coarse frame): what a test needs to evaluate the same sums in
    another precision."""
    f = np.float32
    s, px, py = _lattice(factor, phase)
    colour_lo, hits = np.asarray(colour_lo), np.asarray(hits)
    single = hits.ndim == 3
    if single:
        colour_lo, hits = colour_lo[None], hits[None]
        variance_lo = None if variance_lo is None else np.asarray(variance_lo)[None]
    if hits.dtype != np.float32 or hits.ndim != 4 or hits.shape[-1] != 12:
        raise ValueError(f"hits must be float32 [N, H, W, 12] or [H, W, 12], got {hits.dtype} {list(hits.shape)}")
    n, h, w = hits.shape[:3]
    wl, hl = coarse_size(w, h, s, (px, py))
    if colour_lo.dtype != np.float32 or colour_lo.ndim != 4 or colour_lo.shape[:3] != (n, hl, wl) or colour_lo.shape[3] not in (3, 4):
        raise ValueError(f"colour_lo must be float32 [{n}, {hl}, {wl}, 3|4], got {colour_lo.dtype} {list(colour_lo.shape)}")
    if variance_lo is not None:
        variance_lo = np.asarray(variance_lo)
        if variance_lo.dtype != np.float32 or variance_lo.shape != (n, hl, wl):
            raise ValueError(f"variance_lo must be float32 [{n}, {hl}, {wl}], got {variance_lo.dtype} {list(variance_lo.shape)}")
    flags, normal_sq = int(flags), int(normal_sq)
    if not 0 <= normal_sq <= 7 or flags & ~31:
        raise ValueError("normal_sq must be 0..7, flags of UPSAMPLE_*")
    sigma_z, alb_floor = f(sigma_z), f(alb_floor)
    if not (sigma_z > 0 and alb_floor > 0):
        raise ValueError("sigma_z and alb_floor must be above 0")
    ch = colour_lo.shape[3]
    pos, _, nrm, ids, alb, _ = hit_fields(hits)
    one, zero = f(1.0), f(0.0)
    with np.errstate(all="ignore"):
        guide = hits[:, py::s, px::s]                                       # [n, hl, wl, 12]: the full records at the lattice points
        gpos, _, gnrm, gid, galb, _ = hit_fields(guide)
        col = colour_lo.copy()
        if flags & UPSAMPLE_DEMODULATE:
            a = np.where(galb > alb_floor, galb, alb_floor)                 # a NaN albedo gives the floor
            col[..., 0:3] = np.where((gid >= 0)[..., None], col[..., 0:3] / a, col[..., 0:3])
        var = np.zeros((n, hl, wl), dtype=f) if variance_lo is None else variance_lo
        ys, xs = np.mgrid[0:h, 0:w]
        x0, y0 = (xs - px) // s, (ys - py) // s                             # floor division: -1 left of / above the lattice
        rx, ry = (xs - px) - x0 * s, (ys - py) - y0 * s
        wx, wy = rx.astype(f) / f(s), ry.astype(f) / f(s)
        hit_p = ids >= 0
        each = []
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                inside = (qx >= 0) & (qx < wl) & (qy >= 0) & (qy < hl)
                qx, qy = np.clip(qx, 0, wl - 1), np.clip(qy, 0, hl - 1)
                b = (wx if i else one - wx) * (wy if j else one - wy)
                idg = gid[:, qy, qx]
                g = np.ones((n, h, w), dtype=f)
                if flags & UPSAMPLE_NORMAL:
                    nq = gnrm[:, qy, qx]
                    d = (nrm[..., 0] * nq[..., 0] + nrm[..., 1] * nq[..., 1]) + nrm[..., 2] * nq[..., 2]
                    d = np.where(0 < d, d, zero)
                    for _ in range(normal_sq):
                        d = d * d
                    g = g * d
                if flags & UPSAMPLE_PLANE:
                    e = gpos[:, qy, qx] - pos
                    d = (nrm[..., 0] * e[..., 0] + nrm[..., 1] * e[..., 1]) + nrm[..., 2] * e[..., 2]
                    t = np.abs(d) / sigma_z
                    g = g * (one / (one + t * t))
                ok = (idg >= 0) & ((idg == ids) if flags & UPSAMPLE_SAME_ID else True)
                elig = inside[None] & np.where(hit_p, ok, idg < 0)
                g = np.where(hit_p, g, one).astype(f)
                each.append((elig, b, g, qy, qx))
        if taps is not None:
            taps.extend(each)
        sums = []
        for stage in (1, 2):
            sc, sw, sv = np.zeros((n, h, w, ch), dtype=f), np.zeros((n, h, w), dtype=f), np.zeros((n, h, w), dtype=f)
            for elig, b, g, qy, qx in each:
                wt = b[None] * g if stage == 1 else g
                take = elig & (0 < wt)
                wt = np.where(take, wt, zero)
                sc = np.where(take[..., None], sc + col[:, qy, qx] * wt[..., None], sc)
                sw = np.where(take, sw + wt, sw)
                sv = np.where(take, sv + var[:, qy, qx] * (wt * wt), sv)
            sums.append((sc, sw, sv))
        first = 0 < sums[0][1]
        sc = np.where(first[..., None], sums[0][0], sums[1][0])
        sw = np.where(first, sums[0][1], sums[1][1])
        sv = np.where(first, sums[0][2], sums[1][2])
        served = 0 < sw
        nx = np.clip(x0 + (2 * rx >= s), 0, wl - 1)
        ny = np.clip(y0 + (2 * ry >= s), 0, hl - 1)
        out = np.where(served[..., None], sc / sw[..., None], col[:, ny, nx]).astype(f)
        vout = np.where(served, sv / (sw * sw), var[:, ny, nx]).astype(f)
        weight = np.where(first, sw, np.where(served, zero, f(-1.0))).astype(f)
        if flags & UPSAMPLE_MODULATE:
            a = np.where(alb > alb_floor, alb, alb_floor)
            out[..., 0:3] = np.where(hit_p[..., None], out[..., 0:3] * a, out[..., 0:3])
    if variance_lo is None:
        vout = None
    if single:
        return out[0], None if vout is None else vout[0], weight[0]
    return out, vout, weight
