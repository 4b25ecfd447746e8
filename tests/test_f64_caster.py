"""The ray contract's geometry against a float64 ray caster (tests/_f64cast.py) on the synthetic scenes and on the crowd scenes
crowd_hier and crowd_flat_dda (tests/_crowd.py: engine-authored surfaces of every tag 0..8, 30 axis maps, 25 min/max patterns,
the two-plane solver, conic == 2, coefficients up to 6.25, endless cylinders and plane strips).

Every other test of the ray API compares the kernels with oracle/qr_oracle.c bit for bit; the oracle is pinned to the reference
only for whole frames from the fixtures' cameras.  The open interval tmin < t < tmax, origins inside solids, un-normalised
directions, the side a hit names, hit point and normal, "layer j + 1 is the next crossing" and "occluded = any casting surface in
the interval" are the project's own contract, stated twice by the same hands.  The caster states it a third time, in float64,
from the surfaces alone: no list, hierarchy, tile or grid.  CPU tests hold the oracle to it, GPU tests the kernels.

Domain: untransformed, unclipped surfaces, as tests/_f64cast.py states and asserts (test_caster_refuses_scenes_outside_its_domain).
Own transforms, surfaces under a trnode and clipper lists -- the fixture scenes -- are covered by tests/test_f64_fixtures.py with
tests/_f64xform.py, a subclass of this caster that returns its arrays bit for bit on this domain.  Still outside both: a
transform node under another one and has_trm == 1, which no scene of either file holds.

Margins (tests/_f64cast.py, stated once there): position 1e-3 scene units, t 1e-4 relative, grazing |disc| < 1e-4 (B^2 + |AC|), apex
1e-2.  Two roots count as apart when they differ by twice a root's margin (each carries its own error).  The crowd scenes are
cast with grazing at 1e-5 and the noise rule at 4 ulps (the same place says why); the synthetic scenes as committed.

Families (at most 8 192 rays each, every second one of them for the 8 layers):
  camera  8 seeded cameras of _rayq.random_cameras at 32 x 32, origins within 0.4 units of object centres
  scale   every 6th of those with dir * 2^k and tmin, tmax * 2^-k, k = -60, -40, -20, 0, 20, 40
  axis    axis-parallel rays with exact zeros, +0.0 in one copy and -0.0 in the other, from a 26 x 26 lattice over each face of
          the scene box grown by a unit, both ways
  inside  origins within 0.1 of every object's pos, tmin 0, tmax cycling through 0.5, 2 and 50 over the rays: 16 random
          directions an object on the small scene and the crowds; 9 on the dense cloud, whose 900 objects x 16 would pass 8 192 rays
  aimed   (crowd scenes only) 16 rays at every real surface, aimed at a point of it, un-normalised, tmax cycling through 0.5, 2,
          50 and inf, every fourth origin inside the surface's box (aimed_rays): what brings the rare kinds, maps and min/max
          patterns under the conditions of test_caps
  patched (occlusion only) synth_small with QR_PROP_TRANSP set and QR_PROP_REFRACT cleared on every third object: camera, inside

Measured on the CPU, the oracle (qro_trace_rays, rays.layers_of over it, tests/hitrec_oracle.c) against the caster, decided rays;
no decided ray differed in surface, side, count, occlusion or layer sequence:
                             undecided share                largest relative t difference    pos, nrm error as a share
  scene          family      closest  occlusion  layers     closest hit    layers            of their bounds
  synth_small    camera      3.30 %   2.08 %     7.08 %     8.60e-6        1.49e-5           0.0444   0.0285
  synth_small    scale       3.59 %   2.34 %     7.47 %     6.30e-6        7.75e-6           0.0287   0.0198
  synth_small    axis        4.83 %   3.53 %     7.94 %     3.78e-6        2.16e-6           0.0221   0.0123
  synth_small    inside      2.52 %   1.73 %     2.75 %     3.94e-6        7.68e-6           0.0516   0.0290
  synth_dense    camera      1.01 %   0.00 %     9.47 %     7.57e-6        9.39e-6           0.0360   0.0246
  synth_dense    scale       1.10 %   0.00 %     9.96 %     7.25e-6        8.83e-6           0.0313   0.0209
  synth_dense    axis        1.85 %   0.71 %    11.39 %     2.28e-6        2.28e-6           0.0133   0.0076
  synth_dense    inside      3.84 %   0.65 %     6.59 %     4.14e-5        3.60e-5           0.0562   0.0290
  crowd_hier     camera      4.76 %   3.10 %     5.57 %     2.57e-5        1.59e-5           0.0985   0.0412
  crowd_hier     scale       4.40 %   2.93 %     5.57 %     1.43e-5        1.43e-5           0.0420   0.0258
  crowd_hier     axis        2.69 %   0.74 %     5.23 %     6.26e-6        6.26e-6           0.0260   0.0098
  crowd_hier     inside      3.27 %   2.47 %     4.09 %     7.10e-6        7.44e-6           0.0490   0.0250
  crowd_hier     aimed       5.29 %   3.37 %     8.29 %     2.50e-5        2.50e-5           0.0812   0.0435
  crowd_flat_dda camera      6.47 %   3.99 %    11.67 %     2.16e-5        2.19e-5           0.0759   0.0493
  crowd_flat_dda scale       5.64 %   3.30 %    11.43 %     1.46e-5        1.53e-5           0.0476   0.0316
  crowd_flat_dda axis       10.06 %   7.59 %    15.43 %     8.41e-6        8.41e-6           0.0349   0.0180
  crowd_flat_dda inside      3.36 %   2.33 %     4.91 %     1.18e-5        1.42e-5           0.0564   0.0321
  crowd_flat_dda aimed       5.77 %   3.43 %     9.95 %     5.91e-5        2.71e-5           0.1700   0.0502
(synth_small_dda, synth_flat and synth_flat_dda hold synth_small's surfaces: the caster's answers are the same.)  The dense
cloud's decided layer rays have three or more layers in 100 %, 100 %, 54 % and 55 % of the cases.  The crowds' shares are of
their own bounds, with T_BOUND_CROWD in them.  Caps on the crowds' undecided shares: 0.12 / 0.12 / 0.25 (0.05 / 0.05 / 0.25 on
the synthetic scenes).
On an MI355X the kernels (trace with and without QR_TRACE_COHERENT, hits, trace_layers with the records of all 8 layers, view_hits)
agree with the caster on every decided ray of the crowd scenes too; their largest t difference is the oracle's, 5.91e-5
(crowd_flat_dda aimed), and with the deeper layers' records they use at most 0.170 of the pos bound and 0.054 of the nrm
bound (the oracle's closest hits: 0.170 and 0.050).
Coverage on the crowds (test_caps, over the five families, decided closest hits): crowd_hier 15 700 hits, 38 % on inner sides,
48 % of the decided rays miss, at least 69 hits on every tag, 12 on every axis map (0x506, which one member holds), 19 on
every min/max pattern, every real surface hit; crowd_flat_dda 25 555 hits, 47 % inner, 33 % miss, at least 123 / 37 / 65,
every real surface hit.
crowd_dense_dda is left out: it meets the undecided caps (at most 5.5 % closest, 2.8 % occlusion, 18.0 % layers) but, named
dense, owes three or more layers on 20 % of every family's decided layer rays, and `inside` has them on 14.5 %.

Bounds:
  ids, sides, counts, occlusion   exact on decided rays
  t     |t - t64| <= T_BOUND |t64| with T_BOUND = 1.7e-4 = 4 x 4.14e-5, the largest difference above on the synthetic scenes
        (below the 1e-3 that test_gpu_t_matches_float64_intersection gives grazing hits).  On the crowd scenes T_BOUND_CROWD =
        2.4e-4 = 4 x 5.91e-5, their largest: a cone 0.1 across hit near its apex from 4.3 units away, where the coefficients of
        F about pos, of mixed sign, are 1.9 ulps of their terms off.  The `aimed` family found it; without it the crowds'
        largest is 2.57e-5 and T_BOUND would have covered them.
  pos   per coordinate |pos - (org + t64 dir)| <= 2^-20 max(|org|_inf, |pos64|_inf) + T_BOUND |t64| |dir|: 16 fp32 ulps at the
        size of the operands of the two fp32 operations qrhip.h pins (dir * t, + org), plus t's bound carried along the ray
  nrm   |nrm - n64| <= max_a |sci[a]| sqrt(3) pos_bound / (|grad F| / 2) + 2^-20.  The normal is grad F / |grad F| with
        grad F = 2 (sci loc - scj), so a hit point off by e (at most sqrt(3) times its per-coordinate bound) moves grad F by at
        most 2 max |sci| e and turns the normal by at most max |sci| e / (|grad F| / 2) -- e over the local radius where
        max |sci| = 1, as on every synthetic surface; 2^-20 for the fp32 arithmetic of the normal itself.  Planes: exactly
        -+ sgn e_k of their axis map, two +0.0.
        The float64 normal faces by the record's own side bit.  On conic == 0 surfaces that bit is held to the caster's first; on
        conic != 0 surfaces, where the solver names the side by root order, the facing of the normal is therefore NOT pinned,
        only its line.
  The oracle uses at most 0.056 of the pos bound and 0.029 of the nrm bound on the synthetic scenes (with T_BOUND = 1.7e-4 in
  them, as committed), 0.170 and 0.050 on the crowds: more than the 4 x room asked for, which test_oracle_hit_records asserts.

Caster rules found while reading disagreements (each stated in tests/_f64cast.py):
  the apex rule, which the synthetic cones already needed, now measured from the singular set of any conic != 0 surface;
  the noise rule: the oracle's t was 1.4e-4 to 1.5e-3 off on `aimed` rays that start inside the box of a cap 0.004 thick cut
    from a sphere of radius 4.7 to 18.75 and run along it.  The reference's solver evaluates F about pos in fp32 as the oracle
    and the kernels do, so this is what the engine computes, no oracle bug: such roots are uncertain (crowd scenes only).
With these the oracle and the caster agree on every decided ray.
"""
import zlib

import numpy as np
import pytest

import _f64cast as F
import _rayq
import _rayset as RS

T_BOUND = 1.7e-4                                            # 4 x 4.14e-5, the oracle's largest (header); at most 1e-3
T_BOUND_CROWD = 2.4e-4                                      # 4 x 5.91e-5, its largest on the crowd scenes (header)
POS_REL = 2.0 ** -20
NRM_ULPS = 2.0 ** -20
assert T_BOUND <= T_BOUND_CROWD <= 1e-3
K = 8
MAX_RAYS, MAX_LAYER_RAYS = 8192, 4096

CROWDS = ["crowd_hier", "crowd_flat_dda"]
CPU_SCENES = ["synth_small", "synth_dense_dda"] + CROWDS
GPU_SCENES = ["synth_small", "synth_small_dda", "synth_flat", "synth_flat_dda", "synth_dense_dda"] + CROWDS
FAMILIES = ["camera", "scale", "axis", "inside"]
PATCHED = "synth_small_patched"
CAP_UNDECIDED, CAP_UNDECIDED_LAYERS = 0.05, 0.25
CAP_UNDECIDED_CROWD = 0.12                                  # closest hit and occlusion; the layers' cap is the same 0.25


def is_crowd(name):
    return name.startswith("crowd")


def families(name):
    return FAMILIES + ["aimed"] if is_crowd(name) else FAMILIES


def cap_undecided(name):
    return CAP_UNDECIDED_CROWD if is_crowd(name) else CAP_UNDECIDED


def t_bound(name):
    return T_BOUND_CROWD if is_crowd(name) else T_BOUND


def margins(name):
    """the crowd scenes' own grazing margin and noise rule (tests/_f64cast.py, "The crowd scenes"); every other margin, and
    every margin of the synthetic scenes, as committed"""
    return F.crowd_margins() if is_crowd(name) else F.Margins()


def pairs(names):
    """(scene, family) parameters, scenes outermost"""
    return [pytest.param(n, f, id=f"{n}-{f}") for n in names for f in families(n)]


@pytest.fixture(scope="module")
def rays_mod():
    import importlib
    from qr_loader import load_package
    load_package()
    return importlib.import_module("quadray_engine_amd.rays")


@pytest.fixture(scope="module")
def helper():
    from test_hit_records import _helper
    return _helper()


# ------------------------------------------------------------------------------------------------------------ scenes, rays

_BLOBS, _DOMAINS, _CASES = {}, {}, {}


def patch_transparent(blob):
    """QR_PROP_TRANSP set and QR_PROP_REFRACT cleared on both sides of every third object: surfaces that cast no shadow"""
    b = bytearray(blob)
    h = _rayq._hdr(b)
    s = np.frombuffer(b, dtype=np.int32, count=h[4] * 64, offset=h[11]).reshape(h[4], 64).copy()
    obj = _rayq.real_surfaces(blob)[1::3]
    s[obj, 42:44] = (s[obj, 42:44] | _rayq.PROP_TRANSP) & ~_rayq.PROP_REFRACT
    b[h[11]:h[11] + s.nbytes] = s.tobytes()
    return bytes(b)


def scene_blob(name):
    if name not in _BLOBS:
        _BLOBS[name] = patch_transparent(RS.scene_blob("synth_small")) if name == PATCHED else RS.scene_blob(name)
    return _BLOBS[name]


def domain(name):
    """one Domain per set of surfaces: the hierarchy, flat and grid versions of a scene hold the same surfaces"""
    s, _ = _rayq.surfaces(scene_blob(name))
    real = _rayq.real_surfaces(scene_blob(name))
    key = zlib.crc32(real.tobytes() + s[real, :44].tobytes())       # the surfaces' numbers and records; words 44..47: lists, not geometry
    if key not in _DOMAINS:
        _DOMAINS[key] = F.Domain(scene_blob(name))
    return key, _DOMAINS[key]


def _seed(name, fam):
    """the versions of synth_small share its seeds (one set of surfaces, one set of rays); every other scene, each crowd
    among them, has its own"""
    base = "synth_small" if name.startswith("synth_small") or name.startswith("synth_flat") else name
    return [zlib.crc32(base.encode()), zlib.crc32(fam.encode())]


def camera_rays(blob, name, rays_mod):
    """8 seeded cameras among the objects at 32 x 32: origins within a few tenths of a unit of object centres"""
    cams = _rayq.random_cameras(blob, seed=_seed(name, "camera")[0], n=8, size=32)
    return np.concatenate([rays_mod.camera_rays(c) for c in cams])


def scale_rays(blob, name, rays_mod):
    """every 6th camera ray with dir * 2^k and tmin, tmax * 2^-k"""
    base = camera_rays(blob, name, rays_mod)[::6][:MAX_RAYS // 6]
    out = []
    for k in (-60, -40, -20, 0, 20, 40):
        s = np.float32(2.0 ** k)
        r = base.copy()
        r[:, 4:7] *= s
        r[:, 3] /= s
        with np.errstate(over="ignore"):                            # FLT_MAX * 2^60: +inf, which the API takes as FLT_MAX
            r[:, 7] /= s
        out.append(r)
    return np.concatenate(out)


def axis_rays(blob, name):
    """axis-parallel rays with exact zeros (+0.0 in one copy, -0.0 in the other) from a lattice through and around the box"""
    lo, hi = _rayq.scene_box(blob)
    lo, hi = lo - 1.0, hi + 1.0
    g = 26
    out = []
    for k in range(3):
        i, j = [a for a in range(3) if a != k]
        u, v = np.meshgrid(np.linspace(-0.05, 1.05, g), np.linspace(-0.05, 1.05, g), indexing="ij")
        for s in (1.0, -1.0):
            o = np.zeros((g * g, 3))
            o[:, i] = lo[i] + u.ravel() * (hi[i] - lo[i])
            o[:, j] = lo[j] + v.ravel() * (hi[j] - lo[j])
            o[:, k] = (lo[k] - 2.0) if s > 0 else (hi[k] + 2.0)
            d = np.zeros((g * g, 3)); d[:, k] = s
            out.append(RS._rays(o, d))
    r = np.concatenate(out)
    neg = r.copy()
    z = neg[:, 4:7] == 0
    neg[:, 4:7][z] = np.float32(-0.0)
    r = np.concatenate([r, neg])
    assert len(r) <= MAX_RAYS
    return r


def inside_rays(blob, name):
    """origins within 0.1 of every object's pos, random unit directions, tmin 0, tmax cycling through 0.5, 2 and 50: 16 directions
    an object where that stays within MAX_RAYS (the small scene), else as many as fit (9 on the dense cloud)"""
    rng = np.random.default_rng(_seed(name, "inside"))
    _, f = _rayq.surfaces(blob)
    obj = _rayq.real_surfaces(blob)[1:]
    per = min(16, MAX_RAYS // len(obj))
    assert per >= 6
    p = np.repeat(f[obj, 0:3].astype(np.float64), per, axis=0)
    off = RS._unit(rng.normal(size=p.shape)) * rng.uniform(0, 0.1, (len(p), 1))
    d = RS._unit(rng.normal(size=p.shape))
    tmax = np.tile([0.5, 2.0, 50.0], len(p) // 3 + 1)[:len(p)]
    return RS._rays(p + off, d, tmin=0.0, tmax=tmax)


AIMED_PER, AIMED_T, AIMED_TRIES = 16, 0.4, 16


def _surface_points(rng, s, f, real, srf, lo, hi):
    """for every entry of srf (indices into real) a seeded point of that surface inside its box, relative to pos: of
    AIMED_TRIES seeded points of the box, each brought onto the surface by two Newton steps along grad F (planes: the box
    already lies in the plane), the one that ends farthest inside the clip bounds minmax_t flags.  An aid to aiming and no
    more: a point that is poorly placed costs coverage, which test_caps counts, and nothing else."""
    n = len(srf)
    sci, scj = f[real, 24:28].astype(np.float64)[srf, None], f[real, 28:31].astype(np.float64)[srf, None]
    quadric = (s[real, 37] != 0)[srf, None, None]
    loc = lo[srf, None] + rng.uniform(0, 1, (n, AIMED_TRIES, 3)) * (hi - lo)[srf, None]
    with np.errstate(all="ignore"):
        for _ in range(2):
            g = 2.0 * (sci[..., 0:3] * loc - scj)
            Fv = (sci[..., 0:3] * loc * loc - 2.0 * scj * loc).sum(axis=2) - sci[..., 3]
            loc = np.where(quadric, loc - (Fv / (g * g).sum(axis=2))[..., None] * g, loc)
    mm = s[real, 7][srf, None]
    room = np.full((n, AIMED_TRIES), np.inf)
    for a in range(3):
        room = np.where(((mm >> a) & 1) == 1, np.minimum(room, loc[..., a] - lo[srf, None, a]), room)
        room = np.where(((mm >> (3 + a)) & 1) == 1, np.minimum(room, hi[srf, None, a] - loc[..., a]), room)
    room = np.where(np.isfinite(loc).all(axis=2), room, -np.inf)
    return loc[np.arange(n), np.argmax(room, axis=1)]


def aimed_rays(blob, name):
    """16 rays at every real surface, each aimed at a seeded point of the surface within its box (_surface_points), from a
    seeded origin 2 to 6 units from the box's centre, every fourth origin inside the box instead.  (16, where 12 would do for
    all but one axis map: crowd_hier holds 0x506 on a single member, the cap below, from inside whose box no ray is decided --
    the noise rule -- so that 12 rays leave it 9 decided hits at the most, and test_caps asks for 10.)
    The box: the record's min / max fields about pos, which on an engine-authored record hold the clipped shape's box on every
    axis, flagged in minmax_t or not (tests/_crowd.py); where a field lies beyond 1e30, on the endless members, 1 unit about
    pos; a plane's own axis at 0.  Its centre is pos itself for most members; a cap cut from a sphere of radius 9.4 has its
    pos that far from anything a ray can hit.
    Aiming at a point of the box alone leaves two members all but unseen: that cap, 0.004 thick, most of which lies within
    POS_MARGIN of its clip bound, and an ellipsoid that shows only at the edges of a box it pokes out of.
    dir is the whole way to the aimed point over AIMED_T = 0.4, not a unit vector: the point lies at t = 0.4, so that every
    tmax of the cycle 0.5, 2, 50, inf over the rays reaches it and 0.5 ends the ray a quarter of the way behind it; tmin 0.
    The origins inside the box move on by one ray from surface to surface, so that they meet every tmax."""
    rng = np.random.default_rng(_seed(name, "aimed"))
    s, f = _rayq.surfaces(blob)
    real = _rayq.real_surfaces(blob)
    assert len(real) * AIMED_PER <= MAX_RAYS
    lo, hi = f[real, 4:7].astype(np.float64), f[real, 8:11].astype(np.float64)
    lo, hi = np.where(np.abs(lo) <= F.OPEN, lo, -1.0), np.where(np.abs(hi) <= F.OPEN, hi, 1.0)
    k = (s[real, 23] >> 4) & 3
    pl = np.nonzero(s[real, 37] == 0)[0]
    lo[pl, k[pl]] = hi[pl, k[pl]] = 0.0
    n = len(real) * AIMED_PER
    srf, j = np.repeat(np.arange(len(real)), AIMED_PER), np.tile(np.arange(AIMED_PER), len(real))
    pos = f[real, 0:3].astype(np.float64)[srf]
    tgt = pos + _surface_points(rng, s, f, real, srf, lo, hi)
    near = pos + lo[srf] + rng.uniform(0, 1, (n, 3)) * (hi - lo)[srf]
    away = pos + 0.5 * (lo + hi)[srf] + RS._unit(rng.normal(size=(n, 3))) * rng.uniform(2.0, 6.0, (n, 1))
    org = np.where(((j + srf) % 4 == 3)[:, None], near, away)
    d = (tgt - org) / AIMED_T
    d[~(np.linalg.norm(d, axis=1) >= 1e-6)] = (1.0, 0.0, 0.0)
    return RS._rays(org, d, tmin=0.0, tmax=np.array([0.5, 2.0, 50.0, np.inf])[j % 4])


def family_rays(name, fam, rays_mod):
    blob = scene_blob(name)
    if fam == "aimed":
        return aimed_rays(blob, name)
    if fam == "camera":
        return camera_rays(blob, name, rays_mod)
    if fam == "scale":
        return scale_rays(blob, name, rays_mod)
    if fam == "axis":
        return axis_rays(blob, name)
    if fam == "inside":
        return inside_rays(blob, name)
    raise KeyError(fam)


def case(name, fam, rays_mod):
    """(rays, the caster's closest hits, indices of the layer rays, the caster's K layers of those), computed once a set of
    surfaces and family and never changed"""
    key = (domain(name)[0], fam)
    if key not in _CASES:
        rays = family_rays(name, fam, rays_mod)
        assert len(rays) <= MAX_RAYS
        dom = domain(name)[1]
        sub = np.arange(0, len(rays), -(-len(rays) // MAX_LAYER_RAYS))
        _CASES[key] = (rays, dom.cast(rays, 1, margins(name)), sub, dom.cast(rays[sub], K, margins(name)))
    return _CASES[key]


def view_case(name, rays_mod):
    """(a seeded camera among the objects as a qr_view, its rays at 67 x 45 -- no multiple of a footprint --, the caster's hits)"""
    key = (domain(name)[0], "view")
    if key not in _CASES:
        blob = scene_blob(name)
        view = rays_mod.view_of(_rayq.random_cameras(blob, seed=_seed(name, "view")[1], n=1)[0])
        rays = rays_mod.view_rays(view, 67, 45, blob)
        _CASES[key] = (view, rays, domain(name)[1].cast(rays, 1, margins(name)))
    return _CASES[key]


# ------------------------------------------------------------------------------------------------------------ comparisons

def _first(mask):
    return int(np.nonzero(mask)[0][0])


def compare_trace(where, dom, rays, c, t, ids, stats=None, tb=T_BOUND):
    """closest hit: surface, side (conic == 0) and t on decided rays"""
    dec = c["decided"]
    want = c["id"][0]
    hit = dec & (want >= 0)
    got = np.asarray(ids, dtype=np.int64)
    srf_bad = dec & ((got >> 1) != (want >> 1))
    assert not srf_bad.any(), (f"{where}: {int(srf_bad.sum())} decided rays name another surface; first {_first(srf_bad)}: ray "
                               f"{rays[_first(srf_bad)].tolist()} got {got[_first(srf_bad)]} want {want[_first(srf_bad)]} at t {c['t'][0, _first(srf_bad)]}")
    plain = hit & ~dom.all_conic[np.maximum(want, 0) >> 1]
    side_bad = plain & ((got & 1) != (want & 1))
    assert not side_bad.any(), (f"{where}: {int(side_bad.sum())} decided hits name the other side; first {_first(side_bad)}: ray "
                                f"{rays[_first(side_bad)].tolist()} got {got[_first(side_bad)]} want {want[_first(side_bad)]}")
    t64 = c["t"][0]
    tmax = np.minimum(rays[:, 7].astype(np.float64), F.FLT_MAX)
    miss = dec & (want < 0)
    assert (np.asarray(t, dtype=np.float64)[miss] == tmax[miss]).all(), f"{where}: a miss does not answer t = tmax"
    err = np.abs(np.asarray(t, dtype=np.float64)[hit] - t64[hit]) / np.abs(t64[hit])
    worst = float(err.max()) if hit.any() else 0.0
    print(f"{where}: {len(rays)} rays, undecided {1 - dec.mean():.4f}, {int(hit.sum())} decided hits, worst relative t difference {worst:.3g}")
    if stats is not None:
        stats["t"] = max(stats.get("t", 0.0), worst)
    assert worst <= tb, f"{where}: t off by {worst:.3g} relative (bound {tb:.3g})"
    return hit


def compare_occluded(where, c, occ):
    dec = c["occ_decided"]
    bad = dec & (np.asarray(occ, dtype=bool) != c["occ"])
    assert not bad.any(), f"{where}: {int(bad.sum())} decided occlusion answers differ; first ray {_first(bad)}, the caster says {bool(c['occ'][_first(bad)])}"
    return dec


def compare_layers(where, dom, rays, c, cnt, t, ids, tb=T_BOUND):
    """the whole id sequence (sides on conic == 0 surfaces), the count and every t of decided rays"""
    dec = c["decided"]
    want = c["id"]                                                  # [K, N]
    got = np.asarray(ids, dtype=np.int64)
    cnt_bad = dec & (np.asarray(cnt) != c["count"])
    assert not cnt_bad.any(), (f"{where}: {int(cnt_bad.sum())} decided rays count other layers; first {_first(cnt_bad)}: ray "
                               f"{rays[_first(cnt_bad)].tolist()} got {np.asarray(cnt)[_first(cnt_bad)]} {got[:, _first(cnt_bad)].tolist()} "
                               f"want {c['count'][_first(cnt_bad)]} {want[:, _first(cnt_bad)].tolist()} at {c['t'][:, _first(cnt_bad)].tolist()}")
    srf_bad = dec[None] & ((got >> 1) != (want >> 1))
    assert not srf_bad.any(), f"{where}: {int(srf_bad.any(axis=0).sum())} decided rays differ in their surface sequence"
    conic = dom.all_conic[np.maximum(want, 0) >> 1]
    side_bad = dec[None] & (want >= 0) & ~conic & ((got & 1) != (want & 1))
    assert not side_bad.any(), f"{where}: {int(side_bad.any(axis=0).sum())} decided rays differ in a side bit"
    h = dec[None] & (want >= 0)
    err = np.abs(np.asarray(t, dtype=np.float64)[h] - c["t"][h]) / np.abs(c["t"][h])
    worst = float(err.max()) if h.any() else 0.0
    print(f"{where}: {len(rays)} rays, undecided {1 - dec.mean():.4f}, {int(h.sum())} decided layer hits, "
          f"{(c['count'][dec] >= 3).mean() if dec.any() else 0:.3f} with three or more, worst relative t difference {worst:.3g}")
    assert worst <= tb, f"{where}: a layer's t off by {worst:.3g} relative (bound {tb:.3g})"


def compare_records(where, dom, rays, c, rec, stats=None, tb=T_BOUND):
    """hit records of decided hits: pos against org + t64 * dir, nrm against the float64 normal, planes exactly"""
    rec = np.ascontiguousarray(rec, dtype=np.float32).reshape(-1, 12)
    ids = rec.view(np.int32)[:, 7].astype(np.int64)
    hit = c["decided"] & (c["id"][0] >= 0)
    assert ((ids >> 1) == (c["id"][0] >> 1))[hit].all(), f"{where}: a record of a decided hit names another surface"
    r, t64 = rays[hit], c["t"][0][hit]
    p64, n64, gl, turn = dom.hit_point(r, ids[hit], t64)            # facing by the record's own side bit: cones name it by root order
    o = np.abs(r[:, 0:3].astype(np.float64)).max(axis=1)
    dl = np.linalg.norm(r[:, 4:7].astype(np.float64), axis=1)
    pos_bound = POS_REL * np.maximum(o, np.abs(p64).max(axis=1)) + tb * np.abs(t64) * dl
    perr = np.abs(rec[hit, 0:3].astype(np.float64) - p64).max(axis=1)
    pr = float((perr / pos_bound).max())
    assert pr <= 1.0, f"{where}: pos off by {pr:.3g} of its bound; ray {r[int(np.argmax(perr / pos_bound))].tolist()}"
    plane = dom.all_tag[ids[hit] >> 1] == 0
    n32 = rec[hit, 4:7]
    want_plane = n64[plane].astype(np.float32)
    assert (n32[plane].view(np.uint32) == (want_plane + np.float32(0.0)).view(np.uint32)).all(), f"{where}: a plane's normal is not exactly +-e_k of its map with two +0.0"
    q = ~plane
    ang = np.linalg.norm(n32[q].astype(np.float64) - n64[q], axis=1)      # the chord: the angle where it is small, and no acos
    nrm_bound = turn[q] * np.sqrt(3.0) * pos_bound[q] / (0.5 * gl[q]) + NRM_ULPS
    nr = float((ang / nrm_bound).max()) if q.any() else 0.0
    print(f"{where}: {int(hit.sum())} records, worst pos error {pr:.3g} of its bound, worst normal angle {nr:.3g} of its bound "
          f"(largest angle {float(ang.max()) if q.any() else 0:.3g})")
    if stats is not None:
        stats["pos"] = max(stats.get("pos", 0.0), pr)
        stats["nrm"] = max(stats.get("nrm", 0.0), nr)
    assert nr <= 1.0, f"{where}: a normal is off by {nr:.3g} of its bound"
    return pr, nr


def caps_of_scene(name, rays_mod):
    """the conditions on what the decided rays of a scene's families cover (the caster's own answers: no oracle, no GPU)"""
    dom = domain(name)[1]
    ids, cap = [], cap_undecided(name)
    for fam in families(name):
        rays, c1, sub, c8 = case(name, fam, rays_mod)
        und, und_occ, und_l = 1 - c1["decided"].mean(), 1 - c1["occ_decided"].mean(), 1 - c8["decided"].mean()
        print(f"{name} {fam}: undecided {und:.4f} closest, {und_occ:.4f} occlusion, {und_l:.4f} layers")
        assert und <= cap and und_occ <= cap, f"{name} {fam}: {und:.3f} / {und_occ:.3f} of the rays undecided"
        assert und_l <= CAP_UNDECIDED_LAYERS, f"{name} {fam}: {und_l:.3f} of the layer rays undecided"
        ids.append(c1["id"][0][c1["decided"]])
        if "dense" in name:
            deep = (c8["count"][c8["decided"]] >= 3).mean()
            assert deep >= 0.20, f"{name} {fam}: {deep:.3f} of the decided rays have three or more layers"
    ids = np.concatenate(ids)
    hits = ids[ids >= 0]
    assert len(hits) >= 1000, f"{name}: {len(hits)} decided hits"
    assert (hits & 1).mean() >= 0.10, f"{name}: {(hits & 1).mean():.3f} of the decided hits on an inner side"
    assert name == "synth_dense_dda" or (ids < 0).mean() >= 0.05, f"{name}: {(ids < 0).mean():.3f} of the decided rays miss"
    tags = dom.all_tag[hits >> 1]
    if not is_crowd(name):
        for tag in range(5):                                        # the kinds synth.py writes
            assert (tags == tag).sum() >= 50, f"{name}: {(tags == tag).sum()} decided hits on a {F.TAGS[tag]}"
        return
    # the crowds: every kind, axis map and min/max pattern the scene holds, and nearly every surface
    per_tag = [int((tags == tag).sum()) for tag in F.TAGS]
    print(f"{name}: {len(hits)} decided hits, {(hits & 1).mean():.3f} inner, {(ids < 0).mean():.3f} of the decided rays miss, per tag {per_tag}")
    for tag, kind in F.TAGS.items():
        assert per_tag[tag] >= 40, f"{name}: {per_tag[tag]} decided hits on a {kind}"
    for what, of_srf in (("axis map", dom.all_axes), ("min/max pattern", dom.all_minmax)):
        held, got = np.unique(of_srf[dom.index]), of_srf[hits >> 1]
        count = {int(v): int((got == v).sum()) for v in held}
        print(f"{name}: decided hits per {what}: {count}")
        thin = {hex(v): n for v, n in count.items() if n < 10}
        assert not thin, f"{name}: fewer than 10 decided hits on {what} {thin}"
    seen = np.isin(dom.index, hits >> 1).mean()
    print(f"{name}: {seen:.4f} of the real surfaces hit")
    assert seen >= 0.95, f"{name}: {seen:.3f} of the real surfaces are hit by a decided ray"


# --------------------------------------------------------------------------------------------------------------------- CPU

def test_caster_refuses_scenes_outside_its_domain():
    """a transformed surface, one that reads its trnode's fields, a clipper list, a trnode, a tag past 8 (a record with a solver
    that real_surfaces would pass over) or an axis map that names an axis twice is an error, never a skipped surface"""
    blob = scene_blob("synth_small")
    h = _rayq._hdr(blob)
    for word, value in ((15, 1), (19, 1), (38, 0), (39, 0), (37, 9), (23, 0x014)):
        b = bytearray(blob)
        s = np.frombuffer(b, dtype=np.int32, count=h[4] * 64, offset=h[11]).reshape(h[4], 64).copy()
        s[7, word] = value
        b[h[11]:h[11] + s.nbytes] = s.tobytes()
        with pytest.raises(AssertionError, match="outside the caster's domain"):
            F.Domain(bytes(b))


@pytest.mark.parametrize("name", GPU_SCENES)
def test_caps(rays_mod, name):
    """every scene the GPU tests upload, here: the caps speak of the caster's answers alone"""
    caps_of_scene(name, rays_mod)


@pytest.mark.parametrize("name, fam", pairs(CPU_SCENES))
def test_oracle_trace_and_occlusion(oracle, rays_mod, name, fam):
    blob, dom = scene_blob(name), domain(name)[1]
    rays, c1, _, _ = case(name, fam, rays_mod)
    t, ids = oracle.trace_rays(blob, rays, "trace", threads=16)
    compare_trace(f"{name} {fam}", dom, rays, c1, t, ids, tb=t_bound(name))
    compare_occluded(f"{name} {fam}", c1, oracle.trace_rays(blob, rays, "occluded", threads=16))


@pytest.mark.parametrize("name, fam", pairs(CPU_SCENES))
def test_oracle_layers(oracle, rays_mod, name, fam):
    blob, dom = scene_blob(name), domain(name)[1]
    rays, _, sub, c8 = case(name, fam, rays_mod)
    cnt, t, ids = rays_mod.layers_of(lambda r: oracle.trace_rays(blob, r, "trace", threads=16), rays[sub], K)
    compare_layers(f"{name} {fam} layers", dom, rays[sub], c8, cnt, t, ids, tb=t_bound(name))


@pytest.mark.parametrize("name, fam", pairs(CPU_SCENES))
def test_oracle_hit_records(helper, rays_mod, name, fam):
    """the hit-record oracle, which is pinned to the reference, stays inside the pos and nrm bounds with 4x room"""
    blob, dom = scene_blob(name), domain(name)[1]
    rays, c1, _, _ = case(name, fam, rays_mod)
    rec = helper(blob, rays)
    compare_trace(f"{name} {fam} records", dom, rays, c1, rec[:, 3], rec.view(np.int32)[:, 7], tb=t_bound(name))     # their own ids and t first
    pr, nr = compare_records(f"{name} {fam}", dom, rays, c1, rec, tb=t_bound(name))
    assert pr <= 0.25 and nr <= 0.25, f"{name} {fam}: the oracle uses {pr:.3g} / {nr:.3g} of the pos / nrm bounds: less than 4x room"


@pytest.mark.parametrize("name", CPU_SCENES)
def test_oracle_view_rays(helper, rays_mod, name):
    """the rays of the GPU tests' view_hits case"""
    dom = domain(name)[1]
    view, rays, c1 = view_case(name, rays_mod)
    assert 1 - c1["decided"].mean() <= cap_undecided(name)
    rec = helper(scene_blob(name), rays)
    hit = compare_trace(f"{name} view", dom, rays, c1, rec[:, 3], rec.view(np.int32)[:, 7], tb=t_bound(name))
    assert hit.sum() >= 500
    compare_records(f"{name} view", dom, rays, c1, rec, tb=t_bound(name))


@pytest.mark.parametrize("fam", ["camera", "inside"])
def test_oracle_occlusion_behind_surfaces_that_cast_nothing(oracle, rays_mod, fam):
    """every third object transparent and not refracting: non-casting surfaces stand in front of casters"""
    blob = scene_blob(PATCHED)
    rays, c1, _, _ = case(PATCHED, fam, rays_mod)
    dec = compare_occluded(f"{PATCHED} {fam}", c1, oracle.trace_rays(blob, rays, "occluded", threads=16))
    assert 1 - dec.mean() <= CAP_UNDECIDED
    share = c1["occ"][dec].mean()
    assert 0.10 <= share <= 0.90, f"{share:.3f} of the decided rays occluded: one answer is rare"
    plain = case("synth_small", fam, rays_mod)[1]
    both = dec & plain["occ_decided"]
    assert (plain["occ"][both] & ~c1["occ"][both]).sum() >= 100, "few rays lose their occluder to the patch"


# ---- teeth: the caster reads a deliberately altered scene or rule, the oracle the true one; the comparison must fail

def _altered(blob, edit):
    b = bytearray(blob)
    h = _rayq._hdr(b)
    s = np.frombuffer(b, dtype=np.int32, count=h[4] * 64, offset=h[11]).reshape(h[4], 64).copy()
    edit(s, s.view(np.float32))
    b[h[11]:h[11] + s.nbytes] = s.tobytes()
    return bytes(b)


def test_teeth_radius(oracle, rays_mod):
    """every tenth object's sci[3] (radius^2 of spheres and cylinders) 2 % larger"""
    blob = scene_blob("synth_small")
    rays = case("synth_small", "camera", rays_mod)[0]
    t, ids = oracle.trace_rays(blob, rays, "trace", threads=16)

    def edit(s, f):
        f[1::10, 27] *= np.float32(1.02)
    wrong = F.Domain(_altered(blob, edit))
    with pytest.raises(AssertionError, match="t off by|another surface"):
        compare_trace("radius", wrong, rays, wrong.cast(rays, 1), t, ids)


def _cylinder_top_rays(blob):
    """(surface index of a cylinder, rays aimed level at its axis just above its top: they pass over it)"""
    s, f = _rayq.surfaces(blob)
    cyl = int(np.nonzero(s[:, 37] == 1)[0][0])
    p, r = f[cyl, 0:3].astype(np.float64), float(f[cyl, 8])
    top = p[2] + float(f[cyl, 10])
    a = np.linspace(0, 2 * np.pi, 64, endpoint=False)
    o = np.stack([p[0] + 3 * r * np.cos(a), p[1] + 3 * r * np.sin(a), np.full(64, top) + np.tile([0.05, 0.2, 0.35, 0.5], 16) * r], axis=1)
    d = np.stack([-np.cos(a), -np.sin(a), np.zeros(64)], axis=1)
    return cyl, RS._rays(o, d)


def test_teeth_clip_bound(oracle):
    """the max z bit cleared in one cylinder's minmax_t: rays that pass over its top now hit its wall"""
    blob = scene_blob("synth_small")
    dom = domain("synth_small")[1]
    cyl, rays = _cylinder_top_rays(blob)
    t, ids = oracle.trace_rays(blob, rays, "trace", threads=16)
    c = dom.cast(rays, 1)
    assert c["decided"].mean() >= 0.9 and ((c["id"][0] >> 1) != cyl).all()
    compare_trace("clip bound, true scene", dom, rays, c, t, ids)

    def edit(s, f):
        s[cyl, 7] &= ~(1 << 5)
    wrong = F.Domain(_altered(blob, edit))
    with pytest.raises(AssertionError, match="another surface"):
        compare_trace("clip bound", wrong, rays, wrong.cast(rays, 1), t, ids)


def test_teeth_side(oracle, rays_mod):
    """the side rule inverted"""
    blob = scene_blob("synth_small")
    rays = case("synth_small", "inside", rays_mod)[0]
    t, ids = oracle.trace_rays(blob, rays, "trace", threads=16)
    wrong = F.Domain(blob, flip_side=True)
    with pytest.raises(AssertionError, match="the other side"):
        compare_trace("side", wrong, rays, wrong.cast(rays, 1), t, ids)


def test_teeth_closed_interval(oracle):
    """tmax at exactly a hit's t: rays straight down onto the ground plane from heights that are whole numbers, so that t is the
    same number in fp32 and float64 and no margin is needed (the caster runs with all margins zero); the open interval
    excludes the hit, a closed one names it"""
    blob = scene_blob("synth_small")
    dom = domain("synth_small")[1]
    g = np.arange(-14.0, 14.5, 1.0)
    x, y = np.meshgrid(g, g, indexing="ij")
    o = np.stack([x.ravel() + 0.25, y.ravel() + 0.25, np.full(x.size, 32.0)], axis=1)
    rays = RS._rays(o, (0.0, 0.0, -1.0))
    c = dom.cast(rays, 1)
    ground = c["decided"] & (c["id"][0] == 0)                        # surface 0, outer side: nothing stands above
    assert ground.sum() >= 100
    rays = rays[ground]
    assert (c["t"][0][ground] == 32.0).all()
    t, ids = oracle.trace_rays(blob, rays, "trace", threads=16)
    assert (ids == 0).all() and (t == np.float32(32.0)).all()
    rays[:, 7] = t
    t, ids = oracle.trace_rays(blob, rays, "trace", threads=16)
    exact = F.Margins(pos=0.0, t_rel=0.0)
    c = dom.cast(rays, 1, margins=exact)
    assert c["decided"].all() and (c["id"][0] == -1).all()
    compare_trace("open interval", dom, rays, c, t, ids)
    wrong = F.Domain(blob, closed=True)
    with pytest.raises(AssertionError, match="another surface"):
        compare_trace("closed interval", wrong, rays, wrong.cast(rays, 1, margins=exact), t, ids)


def _mapped_plane(dom, c):
    """the plane of a crowd whose normal axis is not z with the most decided closest hits in cast c: (surface index, hits)"""
    ids = c["id"][0][c["decided"] & (c["id"][0] >= 0)] >> 1
    planes = [int(i) for i in dom.index if dom.all_tag[i] == 0 and (dom.all_axes[i] >> 4) & 3 != 2]
    best = max(planes, key=lambda i: int((ids == i).sum()))
    return best, int((ids == best).sum())


def _crowd_teeth(oracle, rays_mod, edit, match):
    """the caster reads crowd_hier with `edit` applied to its surface records, the oracle the true scene, on the aimed rays"""
    name = "crowd_hier"
    blob, dom = scene_blob(name), domain(name)[1]
    rays, c1, _, _ = case(name, "aimed", rays_mod)
    t, ids = oracle.trace_rays(blob, rays, "trace", threads=16)
    compare_trace("true crowd", dom, rays, c1, t, ids, tb=t_bound(name))
    wrong = F.Domain(_altered(blob, lambda s, f: edit(s, f, dom, c1)))
    with pytest.raises(AssertionError, match=match):
        compare_trace("altered crowd", wrong, rays, wrong.cast(rays, 1, margins(name)), t, ids, tb=t_bound(name))


def test_teeth_plane_sign(oracle, rays_mod):
    """bit 10 of axes, the sign of the normal, flipped on one plane whose normal axis is x or y: its hits name the other side"""
    def edit(s, f, dom, c1):
        plane, n = _mapped_plane(dom, c1)
        assert n >= 5
        s[plane, 23] ^= 1 << 10
    _crowd_teeth(oracle, rays_mod, edit, "the other side")


def test_teeth_plane_axis(oracle, rays_mod):
    """map_k of that plane exchanged with map_i: it lies elsewhere"""
    def edit(s, f, dom, c1):
        plane, n = _mapped_plane(dom, c1)
        assert n >= 5
        a = int(s[plane, 23])
        s[plane, 23] = (a & ~0x33) | ((a & 3) << 4) | ((a >> 4) & 3)
    _crowd_teeth(oracle, rays_mod, edit, "another surface|t off by")


def test_teeth_hyperboloid_sign(oracle, rays_mod):
    """the negative sci coefficient of every hyperboloid (tag 5) made positive: ellipsoids in their place"""
    def edit(s, f, dom, c1):
        hyp = np.nonzero(s[:, 37] == 5)[0]
        neg = f[hyp, 24:27] < 0
        assert len(hyp) >= 10 and (neg.sum(axis=1) == 1).all()
        f[hyp, 24:27] = np.abs(f[hyp, 24:27])
    _crowd_teeth(oracle, rays_mod, edit, "another surface|t off by")


# --------------------------------------------------------------------------------------------------------------------- GPU

_SCENES = {}


@pytest.fixture(scope="module")
def scenes(qr):
    """one Scene per scene name for the whole module, uploaded under the scene's own environment"""
    def get(name):
        if name not in _SCENES:
            with RS.upload_env("synth_small" if name == PATCHED else name):
                _SCENES[name] = qr.Scene(scene_blob(name), ray_queries=True)
        return _SCENES[name]
    yield get
    for s in _SCENES.values():
        s.close()
    _SCENES.clear()


def _dev(scn, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(f"cuda:{scn.device}")


def _host(*tensors):
    """every launch synchronised and copied back before anything is compared"""
    import torch
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in tensors]


@pytest.mark.gpu
@pytest.mark.parametrize("name, fam", pairs(GPU_SCENES))
def test_gpu_trace_occluded_hits(scenes, rays_mod, name, fam):
    scn, dom = scenes(name), domain(name)[1]
    rays, c1, _, _ = case(name, fam, rays_mod)
    r = _dev(scn, rays)
    for coherent in (False, True):
        t, ids = _host(*scn.trace(r, coherent=coherent))
        compare_trace(f"{name} {fam} coherent={coherent}", dom, rays, c1, t, ids, tb=t_bound(name))
    occ, rec = _host(scn.occluded(r), scn.hits(r))
    compare_occluded(f"{name} {fam}", c1, occ)
    compare_trace(f"{name} {fam} hits", dom, rays, c1, rec[:, 3], rec.view(np.int32)[:, 7], tb=t_bound(name))
    compare_records(f"{name} {fam}", dom, rays, c1, rec, tb=t_bound(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name, fam", pairs(GPU_SCENES))
def test_gpu_layers(scenes, rays_mod, name, fam):
    scn, dom = scenes(name), domain(name)[1]
    rays, _, sub, c8 = case(name, fam, rays_mod)
    cnt, t, ids, rec = _host(*scn.trace_layers(_dev(scn, rays[sub]), K, hits=True))
    where = f"{name} {fam} layers"
    compare_layers(where, dom, rays[sub], c8, cnt, t, ids, tb=t_bound(name))
    assert (rec.view(np.int32)[:, :, 7] == ids).all() and (rec[:, :, 3].view(np.uint32) == t.view(np.uint32)).all(), f"{where}: the records name other hits"
    for j in range(K):                                              # every layer's record against that crossing
        layer = {"decided": c8["decided"], "id": c8["id"][j:j + 1], "t": c8["t"][j:j + 1]}
        if (layer["decided"] & (layer["id"][0] >= 0)).any():
            compare_records(f"{where} {j}", dom, rays[sub], layer, rec[j], tb=t_bound(name))


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["camera", "inside"])
def test_gpu_occlusion_behind_surfaces_that_cast_nothing(scenes, rays_mod, fam):
    scn = scenes(PATCHED)
    rays, c1, _, _ = case(PATCHED, fam, rays_mod)
    occ, = _host(scn.occluded(_dev(scn, rays)))
    dec = compare_occluded(f"{PATCHED} {fam}", c1, occ)
    assert 0.10 <= c1["occ"][dec].mean() <= 0.90


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_SCENES)
def test_gpu_view_hits(scenes, rays_mod, name):
    scn, dom = scenes(name), domain(name)[1]
    view, rays, c1 = view_case(name, rays_mod)
    rec, = _host(scn.view_hits(_dev(scn, view[None]), 67, 45))
    rec = rec.reshape(-1, 12)
    hit = compare_trace(f"{name} view", dom, rays, c1, rec[:, 3], rec.view(np.int32)[:, 7], tb=t_bound(name))
    assert hit.sum() >= 500
    compare_records(f"{name} view", dom, rays, c1, rec, tb=t_bound(name))
