"""The ray contract's geometry against the float64 ray caster on the fixture scenes themselves: own transforms, surfaces under a
trnode and clipper lists (tests/_f64xform.py XDomain, a subclass of tests/_f64cast.py Domain; the model is stated there).

tests/test_f64_caster.py holds the oracle and the kernels to a float64 caster on untransformed, unclipped surfaces.  The device
code that the synthetic and crowd scenes never reach is what the fixtures are made of: trnode cells and the cached-transform path
(QR_OPT_TRNODE, QR_OPF_CACHED, QR_OPF_OWN), own transforms with rotation, scale and both, mirrored and non-unit scalers, min/max
bounds applied to a local hit, the clipper program (CClip, fast plane cells, QR_CLT_QUADJ / QR_CLT_QUAD, QR_CLT_TRNODE /
QR_CLT_TRSAME, QR_CLF_LASTC, the ENTER / LEAVE accumulators with c_def), lists that may not take the per-lane walk because a cell
has a clipper, and the hit record's normal through the transposed matrix of the transform node.  An error there that oracle and
kernels share passed the suite; here the oracle (CPU) and the kernels (GPU) answer to a third statement, from the surfaces and
their clipper lists alone.  Snapshots come from conftest.load_blob; _rayset.SCENES is not touched.

Scenes: test03_160_j18 (9 surfaces: a rotated hyperboloid behind an accumulator group of six planes, rotated and scaled planes),
test12_160_j8 (21: 19 own transforms, 13 of them mirrored, all non-unit, two cylinders with accumulator groups), test13_160 (104
real surfaces, 97 under rotating trnodes, 22 clipper lists with trnode elements), demo03_160 (152: 81 under trnodes, 18 own
transforms with rotation and scale), demo01_160 (43: 22 under trnodes, 4 own, 18 clipper lists, three accumulator groups, one
with a trnode element inside), demo02_160_gf_d5 (106: 31 under trnodes, 22 clipper lists) on CPU and GPU; test17_160_j18 (8) and
swarm_demo01_240 (283) on the CPU only.

Families (at most 8 192 rays each; every ray of at most 4 096, else every second one, for the K = 8 layers): camera, scale and axis
are tests/test_f64_caster.py's.  `inside` is that file's with the objects' world positions (a surface under a trnode keeps its
pos in the trnode's space).  `aimed`: min(64, 4 096 // surfaces) rays at every real surface, aimed at a point chosen on the
surface in its LOCAL space and carried to the world through the inverse map (aimed_rays); among the candidate points those the
clipper program keeps are preferred, on every fourth ray not, so that clipped-away parts are aimed at too.  Random cameras put
38 to 110 of 4 096 rays on the demos' transformed members; with `aimed` every class below has hundreds to thousands.

Margins: the parent's defaults (position 1e-3, t 1e-4 relative, grazing 1e-4, apex 1e-2, no noise rule of the parent's) and
_f64xform's transform noise rule, found here while reading a disagreement (below).

Measured, decided rays; no decided ray differed in surface, side (conic == 0), count, occlusion or layer sequence, on the CPU
(oracle: qro_trace_rays, rays.layers_of over it, tests/hitrec_oracle.c) or on an MI355X (kernels: trace with and without
QR_TRACE_COHERENT, occluded, hits, trace_layers(8, hits=True), view_hits at 67 x 45).  The kernels' t differences are the
oracle's in every row:
                            rays    undecided share            decided hits     largest relative t difference        pos, nrm error as a share of their bounds
  scene            family          closest occlusion layers   closest layers   oracle: closest, layers   kernels     oracle            kernels, all layers' records
  test03_160_j18   camera   8192   0.33 %   0.18 %   0.54 %    5105    4108   1.32e-05  1.32e-05      1.32e-05    0.0786  0.1050    0.0786  0.1050
  test03_160_j18   scale    8190   0.29 %   0.22 %   0.51 %    5124    4116   1.15e-06  4.84e-06      4.84e-06    0.0100  0.1050    0.0268  0.1050
  test03_160_j18   axis     8112   0.42 %   0.02 %   0.69 %    7670    5924   8.96e-06  6.35e-06      8.96e-06    0.0633  0.1050    0.0633  0.1050
  test03_160_j18   inside    128   2.34 %   2.34 %   2.34 %      78     103   1.63e-06  1.63e-06      1.63e-06    0.0490  0.1050    0.0490  0.1050
  test03_160_j18   aimed     576   6.08 %   0.17 %   8.85 %     534    1155   7.57e-06  7.57e-06      7.57e-06    0.0407  0.1050    0.0407  0.1050
  test12_160_j8    camera   8192   0.17 %   0.12 %   0.27 %    3510    2437   4.36e-06  4.07e-06      4.36e-06    0.0294  0.0059    0.0294  0.0059
  test12_160_j8    scale    8190   0.15 %   0.07 %   0.22 %    3498    2430   1.31e-06  1.94e-06      1.94e-06    0.0079  0.0004    0.0138  0.0059
  test12_160_j8    axis     8112   0.79 %   0.64 %   0.74 %    1050     992   4.72e-06  2.93e-06      4.72e-06    0.0361  0.0077    0.0361  0.0080
  test12_160_j8    inside    320   0.62 %   0.31 %   0.62 %      78     104   1.34e-06  1.34e-06      1.34e-06    0.0282  0.0164    0.0282  0.0164
  test12_160_j8    aimed    1344   8.78 %   2.46 %   9.97 %     566     973   7.16e-06  7.31e-06      7.31e-06    0.0522  0.0182    0.0530  0.0202
  test13_160       camera   8192   1.57 %   0.09 %   2.56 %    7493    4344   1.48e-06  2.86e-06      2.86e-06    0.0111  0.0971    0.0210  0.0971
  test13_160       scale    8190   1.83 %   0.07 %   2.42 %    7464    4320   1.48e-06  2.77e-06      2.77e-06    0.0111  0.0971    0.0210  0.0971
  test13_160       axis     8112   3.06 %   2.76 %   9.96 %    4760    4476   0.00e+00  2.83e-06      2.83e-06    0.0000  0.0000    0.0216  0.0971
  test13_160       aimed    4056  10.01 %   0.10 %  20.66 %    3618    9797   5.90e-06  5.90e-06      5.90e-06    0.0398  0.0971    0.0398  0.0971
  demo03_160       camera   8192   1.45 %   0.15 %   9.35 %    7650    9291   9.42e-06  8.62e-06      9.42e-06    0.0695  0.0704    0.0695  0.0704
  demo03_160       scale    8190   1.90 %   0.22 %  10.11 %    7584    9225   2.38e-06  7.33e-06      7.33e-06    0.0175  0.0704    0.0521  0.0704
  demo03_160       inside   2416   9.40 %   2.94 %  10.39 %    1847    3695   1.22e-05  1.22e-05      1.22e-05    0.0883  0.0704    0.0883  0.0704
  demo03_160       aimed    3952   8.17 %   1.62 %  20.77 %    3613   10759   8.65e-06  8.97e-06      8.97e-06    0.0519  0.0704    0.0544  0.0704
  demo01_160       camera   8192   0.39 %   0.16 %   0.88 %    6626    5527   6.26e-06  7.61e-06      7.61e-06    0.0447  0.0599    0.0578  0.0599
  demo01_160       scale    8190   0.29 %   0.15 %   0.66 %    6648    5529   2.52e-06  3.26e-06      3.26e-06    0.0153  0.0317    0.0237  0.0317
  demo01_160       axis     8112   0.15 %   0.10 %   0.39 %    3686    3092   3.69e-06  3.69e-06      3.69e-06    0.0281  0.1150    0.0281  0.1150
  demo01_160       inside    672   6.55 %   2.53 %   7.29 %     420     650   3.14e-05  3.14e-05      3.14e-05    0.0837  0.1150    0.0837  0.1150
  demo01_160       aimed    2752   5.92 %   1.20 %   9.81 %    2467    6262   3.12e-05  3.12e-05      3.12e-05    0.0357  0.1150    0.0357  0.1150
  demo02_160_gf_d5 camera   8192   1.86 %   0.05 %   5.35 %    7832    7297   3.48e-06  2.88e-06      3.48e-06    0.0263  0.0283    0.0263  0.0283
  demo02_160_gf_d5 scale    8190   2.42 %   0.00 %   5.79 %    7776    7263   1.40e-06  1.46e-06      1.46e-06    0.0200  0.0283    0.0200  0.0283
  demo02_160_gf_d5 axis     8112   1.06 %   0.69 %   3.70 %    4754    4820   0.00e+00  2.47e-06      2.47e-06    0.0000  0.0000    0.0188  0.0283
  demo02_160_gf_d5 inside   1680   9.11 %   2.86 %  12.50 %    1024    1755   1.26e-05  1.26e-05      1.26e-05    0.0390  0.0283    0.0390  0.0283
  demo02_160_gf_d5 aimed    4028  10.05 %   0.15 %  20.63 %    3606    9691   1.76e-05  1.76e-05      1.76e-05    0.0381  0.0283    0.0539  0.0382
  test17_160_j18   camera   8192   0.20 %   0.13 %   0.32 %    6836    4882   2.03e-06  8.27e-07      -           0.0164  0.0691    -
  test17_160_j18   scale    8190   0.07 %   0.07 %   0.29 %    6846    4893   6.40e-07  6.40e-07      -           0.0143  0.0691    -
  test17_160_j18   axis     8112   0.30 %   0.15 %   0.49 %    5162    3590   4.29e-06  1.36e-06      -           0.0187  0.0691    -
  test17_160_j18   aimed     512   9.57 %   0.39 %   9.57 %     461     751   5.39e-06  5.39e-06      -           0.0292  0.0691    -
  swarm_demo01_240 camera   8192   6.36 %   4.60 %  12.60 %    4210    4800   8.56e-06  8.56e-06      -           0.0635  0.1150    -
  swarm_demo01_240 scale    8190   5.79 %   4.25 %  12.38 %    4248    4824   6.88e-06  6.99e-06      -           0.0500  0.1150    -
  swarm_demo01_240 axis     8112  10.01 %   8.28 %  16.27 %    2644    2028   6.25e-06  6.35e-06      -           0.0478  0.1150    -
  swarm_demo01_240 inside   4512   1.06 %   0.44 %   1.86 %    3853    2575   1.14e-05  1.14e-05      -           0.0475  0.1150    -
  swarm_demo01_240 aimed    3962  11.13 %   6.44 %  16.10 %    3430    8280   1.76e-05  1.76e-05      -           0.0549  0.1150    -
  test03_160_j18   view     3015   0.17 %                      1488          4.18e-07              4.18e-07    0.0027  0.0014    0.0027  0.0014
  test12_160_j8    view     3015   0.33 %                       693          3.04e-06              3.04e-06    0.0225  0.0059    0.0225  0.0059
  test13_160       view     3015   0.93 %                      2987          9.56e-08              9.56e-08    0.0009  0.0000    0.0009  0.0000
  demo03_160       view     3015   2.45 %                      1259          4.64e-06              4.64e-06    0.0292  0.0141    0.0292  0.0141
  demo01_160       view     3015   0.56 %                       931          5.02e-06              5.02e-06    0.0319  0.1150    0.0319  0.1150
  demo02_160_gf_d5 view     3015   1.59 %                      2967          2.51e-06              2.51e-06    0.0183  0.0103    0.0183  0.0103
oracle: largest t difference 3.14e-5 (demo01_160 inside), pos 0.0883, nrm 0.115 of their bounds.  kernels, with the records of all 8 layers: 3.14e-5, 0.0883, 0.115.

Dropped (scene, family) pairs -- the caster alone cannot keep them inside the caps 0.12 / 0.12 / 0.25, which are the crowds' and are
not loosened; every scene keeps camera, aimed and four families:
  demo03_160 axis           9.91 % / 9.17 % / 38.07 %: axis-parallel rays through a scene of axis-aligned boxes; 38 % of the layer
                            rays meet an uncertain root, or two roots less than their margins apart, among the first 8
  test13_160 inside         18.3 % / 5.3 % closest / occlusion, test17_160_j18 inside 20.5 % / 11.6 %: origins within 0.1 of
                            surfaces under trnodes whose pos lies several units away -- the short rays the transform noise rule
                            leaves undecided (before that rule: 9.3 % and 2.7 %, and the oracle 5.8e-4 off on demo03_160)

Coverage over a scene's families, decided closest hits (test_conditions; a class counts where the scene holds at least three
surfaces of it).  hits / inner share / hits on surfaces under a trnode / with an own transform / with a clipper list / rays whose
answer lies behind a root that passed interval and min/max and that the clipper program alone rejected / of those through an
accumulator group:
  test03_160_j18    18 511  0.53       -  17 134  15 601  2 232  343
  test12_160_j8      8 702  0.58       -   8 660   3 211  5 088    0
  test13_160        23 335  0.32   2 734       -     371    356    -
  demo03_160        20 694  0.48   6 200     317       -      -    -
  demo01_160        19 847  0.56   1 409     904  11 584  3 807  147
  demo02_160_gf_d5  24 992  0.40   1 535       -     517    455    -
  test17_160_j18    19 305  0.50   4 527       -       -      -    -     (2 own transforms: below three, 14 778 hits all the same)
  swarm_demo01_240  18 385  0.31   3 694     376     904  8 290   45
  test12_160_j8 cannot give a rejection through its accumulator groups with any ray: the groups cut the box of planes 3..8
  (11..16) out of cylinder 10 (18), and the cylinder's wall does not pass through that box -- of 20 000 points sampled on either
  wall inside its min/max bounds the group rejects none.  The groups are still run: all 3 211 decided hits on the two cylinders
  pass through them (the condition asks for 100), and a group evaluated wrongly would reject them.
Unseen -- real surfaces with a transform or a clipper list that no decided ray can hit (UNSEEN; every other such surface is hit by
a decided ray), each checked by test_unseen_surfaces_cannot_be_seen on 4 000 points sampled on the surface inside its min/max bounds:
  wholly clipped away by their own clipper (the program keeps no sampled point): test12_160_j8 4..8, 12..16 (box faces kept inside
    a cylinder that they lie outside of), demo01_160 24, 40, 43, 46, swarm_demo01_240 214, 234, 240, 248 (the same members)
  a min bound above its max bound, an empty surface: test12_160_j8 3, 11, 20
  lying in another surface's plane, inside its bounds, where fp32 cannot tell the two apart and a hit on either is undecided:
    test13_160 80, 81, 90, 91, 94, 97 (box bottoms in the ground plane 44), demo02_160_gf_d5 83, 84, 92, 94 (in 58), demo01_160 47
    (in 17), swarm_demo01_240 257 (in 183); a ray that passes the other surface's bounds may still decide one, so some are hit
The oracle's answers on all of them agree with the caster's (misses, or the surface in front).

Bounds:
  ids, sides (conic == 0), counts, layer sequences, occlusion   exact on decided rays
  t     |t - t64| <= T_BOUND_X |t64|, T_BOUND_X = 1.3e-4 = 4 x 3.14e-5, the oracle's largest above (at most 1e-3)
  pos   the parent's: per coordinate 2^-20 max(|org|_inf, |pos64|_inf) + T_BOUND_X |t64| |dir|
  nrm   n = M^T g / |M^T g| with g the local gradient at loc = M (x - P) - Q.  A world hit point off by e (at most sqrt(3) times
        its per-coordinate bound) is off by at most sigma_max e locally; g = 2 (sci loc - scj) moves by at most
        2 max |sci| sigma_max e, M^T g by at most sigma_max times that, and |M^T g| >= sigma_min |g|: the normal turns by at most
        (sigma_max / sigma_min) max |sci| sigma_max e / (|g| / 2) -- the parent's term with the local position error
        sigma_max e and the turn through M^T.  A plane's g is constant, so a transformed plane has no such term (max |sci| taken
        as 0) and is compared like a quadric, with the fp32 term alone; untransformed planes stay exact, two +0.0.
        The fp32 term: 2^-20 sigma_max / sigma_min -- 16 ulps at sigma_max's size, the size of the products that M^T g sums,
        against a result of sigma_min's size.  It holds for the renormalised normals with 8 x room: the oracle uses at most
        0.115 of the whole bound (demo01_160, swarm_demo01_240; test03_160_j18 0.105), below the quarter that
        test_oracle_hit_records asserts.
        Facing by the record's own side bit, as in the parent.

Caster rule found while reading a disagreement (stated in tests/_f64xform.py): transform noise.  demo03_160 `inside`, a ray that
starts 0.004 in front of a plane under a rotating trnode 10 units away and meets it at 78 degrees: the oracle's t was 5.8e-4
off, 1.2e-5 in space.  The engine computes the local origin and direction in fp32, so this is what it computes, no oracle bug;
such roots are uncertain.  With it the oracle and the caster agree on every decided ray, and the largest t difference fell from
5.8e-4 to 3.14e-5.

Teeth (CPU): the oracle runs on an altered snapshot, the caster on the original, and decided rays must disagree -- a trnode's
matrix transposed, an own transform's local z row negated, a clipper's side flipped, an enter / leave pair unlinked, a Q moved
by 0.05; and a caster that carries the gradient through M in place of M^T fails compare_records on a surface of
test12_160_j8 with sigma_max > 1.5 sigma_min.
"""
import numpy as np
import pytest

import _f64cast as F
import _f64xform as X
import _rayq
import _rayset as RS
import test_f64_caster as T
from conftest import load_blob

T_BOUND_X = 1.3e-4                                          # 4 x 3.14e-5, the oracle's largest on these scenes (header); at most 1e-3
POS_REL, NRM_ULPS = T.POS_REL, T.NRM_ULPS
assert T_BOUND_X <= 1e-3
K = T.K
MAX_RAYS, MAX_LAYER_RAYS = T.MAX_RAYS, T.MAX_LAYER_RAYS
CAP_UNDECIDED, CAP_UNDECIDED_LAYERS = T.CAP_UNDECIDED_CROWD, T.CAP_UNDECIDED_LAYERS       # 0.12 / 0.12 / 0.25: the crowds' caps

GPU_SCENES = ["test03_160_j18", "test12_160_j8", "test13_160", "demo03_160", "demo01_160", "demo02_160_gf_d5"]
CPU_SCENES = GPU_SCENES + ["test17_160_j18", "swarm_demo01_240"]
FAMILIES = ["camera", "scale", "axis", "inside", "aimed"]
DROPPED = {("demo03_160", "axis"), ("test13_160", "inside"), ("test17_160_j18", "inside")}                        # the caster alone cannot keep it inside the caps (header, "Dropped")
GROUP_SCENES = ["test03_160_j18", "demo01_160"]             # owe clip-only rejections through an accumulator group; test12_160_j8: header
# real surfaces with a transform or a clipper list that no decided ray can hit (header, "Unseen"): wholly clipped away by their
# own clipper, or lying in another surface's plane, where fp32 cannot tell the two apart and every ray is undecided
UNSEEN = {"test12_160_j8": {3: "empty", 4: "clipped", 5: "clipped", 6: "clipped", 7: "clipped", 8: "clipped", 11: "empty", 12: "clipped",
                            13: "clipped", 14: "clipped", 15: "clipped", 16: "clipped", 20: "empty"},
          "test13_160": {80: 44, 81: 44, 90: 44, 91: 44, 94: 44, 97: 44},
          "demo01_160": {24: "clipped", 40: "clipped", 43: "clipped", 46: "clipped", 47: 17},
          "demo02_160_gf_d5": {83: 58, 84: 58, 92: 58, 94: 58},
          "swarm_demo01_240": {214: "clipped", 234: "clipped", 240: "clipped", 248: "clipped", 257: 183}}


def families(name):
    return [f for f in FAMILIES if (name, f) not in DROPPED]


def pairs(names):
    return [pytest.param(n, f, id=f"{n}-{f}") for n in names for f in families(n)]


rays_mod, helper = T.rays_mod, T.helper                     # the module's fixtures, one instance a module

_DOMAINS, _CASES = {}, {}


def domain(name):
    if name not in _DOMAINS:
        _DOMAINS[name] = X.XDomain(load_blob(name))
    return _DOMAINS[name]


# ------------------------------------------------------------------------------------------------------------------- rays

def world_of(dom, j, loc):
    """the world points of local points loc [n, 3] of the real surfaces j [n]: x = P + M^-1 (loc + Q)"""
    return dom.P[j] + np.einsum("mab,mb->ma", dom.Minv[j], loc + dom.Q[j])


def inside_rays(blob, name):
    """the file's `inside` family with the objects' WORLD positions (loc = 0 carried through the inverse map): a surface under
    a trnode keeps its pos in the trnode's space"""
    rng = np.random.default_rng(T._seed(name, "inside"))
    dom = domain(name)
    obj = np.arange(1, len(dom.index))
    per = min(16, MAX_RAYS // len(obj))
    assert per >= 6
    p = np.repeat(world_of(dom, obj, np.zeros((len(obj), 3))), per, axis=0)
    off = RS._unit(rng.normal(size=p.shape)) * rng.uniform(0, 0.1, (len(p), 1))
    d = RS._unit(rng.normal(size=p.shape))
    tmax = np.tile([0.5, 2.0, 50.0], len(p) // 3 + 1)[:len(p)]
    return RS._rays(p + off, d, tmin=0.0, tmax=tmax)


AIMED_PER, AIMED_T, AIMED_TRIES = 64, 0.4, 16


def _surface_points(rng, dom, srf, lo, hi):
    """for every entry of srf (real surfaces) a seeded LOCAL point of that surface inside its box: AIMED_TRIES seeded points of
    the box, brought onto the surface by two Newton steps along grad F (planes: the box lies in the plane).  Of those the one
    farthest inside the flagged min/max bounds among the points that the clipper program keeps (margin-less) -- on every
    fourth ray among all of them, so that clipped-away parts are aimed at too.  An aid to aiming and no more: a poor point
    costs coverage, which test_conditions counts."""
    n = len(srf)
    sci, scj = dom.sci[srf, None], dom.scj[srf, None]
    quadric = ~dom.plane[srf, None, None]
    loc = lo[srf, None] + rng.uniform(0, 1, (n, AIMED_TRIES, 3)) * (hi - lo)[srf, None]
    with np.errstate(all="ignore"):
        for _ in range(2):
            g = 2.0 * (sci[..., 0:3] * loc - scj)
            Fv = (sci[..., 0:3] * loc * loc - 2.0 * scj * loc).sum(axis=2) - sci[..., 3]
            loc = np.where(quadric, loc - (Fv / (g * g).sum(axis=2))[..., None] * g, loc)
    room = np.full((n, AIMED_TRIES), np.inf)
    for a in range(3):
        room = np.where(dom.has_mn[srf, None, a], np.minimum(room, loc[..., a] - lo[srf, None, a]), room)
        room = np.where(dom.has_mx[srf, None, a], np.minimum(room, hi[srf, None, a] - loc[..., a]), room)
    room = np.where(np.isfinite(loc).all(axis=2), room, -np.inf)
    room = np.minimum(room, 1e6)
    flat = np.repeat(srf, AIMED_TRIES)
    with np.errstate(all="ignore"):
        h = world_of(dom, flat, np.nan_to_num(loc.reshape(-1, 3)))
        kept = np.ones(len(flat), dtype=bool)
        sel = np.nonzero(dom.has_clip[flat])[0]
        if len(sel):
            ct, cf, _ = dom._clip(flat[sel], h[sel], np.zeros(len(sel)))
            kept[sel] = ct & ~cf
    plain = (np.arange(n) % 4 == 1)[:, None]
    score = np.where(kept.reshape(n, AIMED_TRIES) | plain, room, room - 2e6)
    return loc[np.arange(n), np.argmax(score, axis=1)]


def aimed_rays(blob, name):
    """16 rays at every real surface, each aimed at a point chosen on the surface in its LOCAL space (_surface_points) and
    carried to the world through the inverse map, from a seeded origin 2 to 6 units from the box's centre, every fourth origin
    inside the surface's box instead.  The box: the record's min / max fields, local (1 unit about the local origin where a
    field lies beyond 1e30; a plane's own axis at 0).  dir is the whole way to the aimed point over AIMED_T = 0.4, tmax cycles
    through 0.5, 2, 50 and inf, tmin 0: tests/test_f64_caster.py aimed_rays, in local space."""
    rng = np.random.default_rng(T._seed(name, "aimed"))
    dom = domain(name)
    _, f = _rayq.surfaces(blob)
    real = dom.index
    per = min(AIMED_PER, MAX_LAYER_RAYS // len(real))              # every aimed ray is a layer ray too
    assert per >= 12
    lo, hi = f[real, 4:7].astype(np.float64), f[real, 8:11].astype(np.float64)
    lo, hi = np.where(np.abs(lo) <= F.OPEN, lo, -1.0), np.where(np.abs(hi) <= F.OPEN, hi, 1.0)
    pl = np.nonzero(dom.plane)[0]
    lo[pl, dom.pk[pl]] = hi[pl, dom.pk[pl]] = 0.0
    n = len(real) * per
    srf, j = np.repeat(np.arange(len(real)), per), np.tile(np.arange(per), len(real))
    tgt = world_of(dom, srf, _surface_points(rng, dom, srf, lo, hi))
    near = lo[srf] + rng.uniform(0, 1, (n, 3)) * (hi - lo)[srf]
    lift = rng.uniform(0.02, 0.5, n) * rng.choice([-1.0, 1.0], n)  # a plane's box is flat: an origin in it would lie on the plane
    near[np.arange(n), dom.pk[srf]] += np.where(dom.plane[srf], lift, 0.0)
    near = world_of(dom, srf, near)
    away = world_of(dom, srf, 0.5 * (lo + hi)[srf]) + RS._unit(rng.normal(size=(n, 3))) * rng.uniform(2.0, 6.0, (n, 1))
    org = np.where(((j + srf) % 4 == 3)[:, None], near, away)
    d = (tgt - org) / AIMED_T
    d[~(np.linalg.norm(d, axis=1) >= 1e-6)] = (1.0, 0.0, 0.0)
    return RS._rays(org, d, tmin=0.0, tmax=np.array([0.5, 2.0, 50.0, np.inf])[j % 4])


def family_rays(name, fam, rays_mod):
    blob = load_blob(name)
    if fam == "camera":
        return T.camera_rays(blob, name, rays_mod)
    if fam == "scale":
        return T.scale_rays(blob, name, rays_mod)
    if fam == "axis":
        return T.axis_rays(blob, name)
    if fam == "inside":
        return inside_rays(blob, name)
    if fam == "aimed":
        return aimed_rays(blob, name)
    raise KeyError(fam)


def case(name, fam, rays_mod):
    """(rays, the caster's closest hits, indices of the layer rays, the caster's K layers of those), computed once and never changed"""
    if (name, fam) not in _CASES:
        rays = family_rays(name, fam, rays_mod)
        assert len(rays) <= MAX_RAYS
        dom = domain(name)
        sub = np.arange(0, len(rays), -(-len(rays) // MAX_LAYER_RAYS))
        _CASES[name, fam] = (rays, dom.cast(rays, 1), sub, dom.cast(rays[sub], K))
    return _CASES[name, fam]


def view_case(name, rays_mod):
    """(a seeded camera among the objects as a qr_view, its rays at 67 x 45, the caster's hits)"""
    if (name, "view") not in _CASES:
        blob = load_blob(name)
        view = rays_mod.view_of(_rayq.random_cameras(blob, seed=T._seed(name, "view")[1], n=1)[0])
        rays = rays_mod.view_rays(view, 67, 45, blob)
        _CASES[name, "view"] = (view, rays, domain(name).cast(rays, 1))
    return _CASES[name, "view"]


# ------------------------------------------------------------------------------------------------------------ comparisons

def compare_records(where, dom, rays, c, rec, stats=None):
    """hit records of decided hits: pos against org + t64 * dir, nrm against the float64 normal (the header's bound);
    untransformed planes exactly"""
    rec = np.ascontiguousarray(rec, dtype=np.float32).reshape(-1, 12)
    ids = rec.view(np.int32)[:, 7].astype(np.int64)
    hit = c["decided"] & (c["id"][0] >= 0)
    assert ((ids >> 1) == (c["id"][0] >> 1))[hit].all(), f"{where}: a record of a decided hit names another surface"
    r, t64 = rays[hit], c["t"][0][hit]
    p64, n64, gl, turn, kappa, exact = dom.hit_point_x(r, ids[hit], t64)
    o = np.abs(r[:, 0:3].astype(np.float64)).max(axis=1)
    dl = np.linalg.norm(r[:, 4:7].astype(np.float64), axis=1)
    pos_bound = POS_REL * np.maximum(o, np.abs(p64).max(axis=1)) + T_BOUND_X * np.abs(t64) * dl
    perr = np.abs(rec[hit, 0:3].astype(np.float64) - p64).max(axis=1)
    pr = float((perr / pos_bound).max())
    assert pr <= 1.0, f"{where}: pos off by {pr:.3g} of its bound; ray {r[int(np.argmax(perr / pos_bound))].tolist()}"
    n32 = rec[hit, 4:7]
    want_plane = n64[exact].astype(np.float32)
    assert (n32[exact].view(np.uint32) == (want_plane + np.float32(0.0)).view(np.uint32)).all(), f"{where}: an untransformed plane's normal is not exactly +-e_k of its map with two +0.0"
    q = ~exact
    ang = np.linalg.norm(n32[q].astype(np.float64) - n64[q], axis=1)
    nrm_bound = turn[q] * np.sqrt(3.0) * pos_bound[q] / (0.5 * gl[q]) + NRM_ULPS * kappa[q]
    nr = float((ang / nrm_bound).max()) if q.any() else 0.0
    print(f"{where}: {int(hit.sum())} records, worst pos error {pr:.3g} of its bound, worst normal angle {nr:.3g} of its bound "
          f"(largest angle {float(ang.max()) if q.any() else 0:.3g})")
    if stats is not None:
        stats["pos"], stats["nrm"] = max(stats.get("pos", 0.0), pr), max(stats.get("nrm", 0.0), nr)
    assert nr <= 1.0, f"{where}: a normal is off by {nr:.3g} of its bound; ray {r[np.nonzero(q)[0][int(np.argmax(ang / nrm_bound))]].tolist()}"
    return pr, nr


# --------------------------------------------------------------------------------------------------------------------- CPU

def test_old_domain_answers_do_not_move(rays_mod):
    """on the parent's own domain the subclass returns the parent's arrays, every key, closest hit and layers"""
    for name in ("synth_small", "crowd_hier"):
        blob = T.scene_blob(name)
        dom, xdom = T.domain(name)[1], X.XDomain(blob)
        assert not xdom.xf.any() and not xdom.has_clip.any()
        for fam in ("camera", "inside"):
            rays, c1, sub, c8 = T.case(name, fam, rays_mod)
            for k, rr, c in ((1, rays, c1), (K, rays[sub], c8)):
                got = xdom.cast(rr, k, T.margins(name))
                for key in ("count", "id", "t", "decided", "occ", "occ_decided"):
                    assert np.array_equal(got[key], c[key]), f"{name} {fam} k={k}: {key} moved"
        hit = c1["decided"] & (c1["id"][0] >= 0)
        for a, b in zip(dom.hit_point(rays[hit], c1["id"][0][hit], c1["t"][0][hit]), xdom.hit_point(rays[hit], c1["id"][0][hit], c1["t"][0][hit])):
            assert np.array_equal(a, b), f"{name}: hit_point moved"


def _class_counts(dom):
    return {"under a trnode": dom.under, "with an own transform": dom.own, "with a clipper list": dom.has_clip}


@pytest.mark.parametrize("name", CPU_SCENES)
def test_conditions(rays_mod, name):
    """the issue's conditions on the caster's own answers: undecided shares, and what the decided rays cover"""
    dom = domain(name)
    fams = families(name)
    assert "camera" in fams and "aimed" in fams and len(fams) >= 4
    ids, rej, rej_g = [], 0, 0
    for fam in fams:
        rays, c1, sub, c8 = case(name, fam, rays_mod)
        und, und_occ, und_l = 1 - c1["decided"].mean(), 1 - c1["occ_decided"].mean(), 1 - c8["decided"].mean()
        print(f"{name} {fam}: {len(rays)} rays, undecided {und:.4f} closest, {und_occ:.4f} occlusion, {und_l:.4f} layers")
        assert und <= CAP_UNDECIDED and und_occ <= CAP_UNDECIDED, f"{name} {fam}: {und:.3f} / {und_occ:.3f} of the rays undecided"
        assert und_l <= CAP_UNDECIDED_LAYERS, f"{name} {fam}: {und_l:.3f} of the layer rays undecided"
        ids.append(c1["id"][0][c1["decided"]])
        rej += int((c1["cliprej"] & c1["decided"]).sum())
        rej_g += int((c1["cliprej_group"] & c1["decided"]).sum())
    ids = np.concatenate(ids)
    hits = ids[ids >= 0]
    where = np.full(len(dom.all_tag), -1, dtype=np.int64)
    where[dom.index] = np.arange(len(dom.index))
    hj = where[hits >> 1]
    print(f"{name}: {len(hits)} decided hits, {(hits & 1).mean():.3f} inner, {rej} clip-only rejections in front of an answer, {rej_g} through a group")
    assert len(hits) >= 1000, f"{name}: {len(hits)} decided hits"
    assert (hits & 1).mean() >= 0.10, f"{name}: {(hits & 1).mean():.3f} of the decided hits on an inner side"
    for what, mask in _class_counts(dom).items():
        print(f"{name}: {int(mask.sum())} surfaces {what}, {int(mask[hj].sum())} decided hits on them")
        if mask.sum() >= 3:
            assert mask[hj].sum() >= 100, f"{name}: {int(mask[hj].sum())} decided hits on surfaces {what}"
    if dom.has_clip.sum() >= 3:
        assert rej >= 40, f"{name}: {rej} decided rays whose answer lies behind a root the clipper program alone rejected"
    if name in GROUP_SCENES:
        assert rej_g >= 1, f"{name}: no clip-only rejection through an accumulator group"
    owed = np.nonzero(dom.xf | dom.has_clip)[0]
    unseen = [int(dom.index[j]) for j in owed if not (hj == j).any()]
    print(f"{name}: transformed or clipped surfaces without a decided hit: {unseen}")
    assert set(unseen) <= set(UNSEEN.get(name, [])), f"{name}: no decided ray hits the transformed or clipped surfaces {unseen}; the header excuses {UNSEEN.get(name, [])}"
    grouped = int(dom.has_group[hj].sum())
    print(f"{name}: {int(dom.has_group.sum())} surfaces with an accumulator group, {grouped} decided hits on them")
    if dom.has_group.any():
        assert grouped >= 100, f"{name}: {grouped} decided hits on surfaces whose clipper list holds an accumulator group"


def _sample_surface(dom, blob, j, n=4000):
    """world points of n seeded local points of real surface j inside its box and, a quadric's, brought onto it by Newton steps
    and kept where they end inside the flagged min/max bounds"""
    rng = np.random.default_rng(j)
    _, f = _rayq.surfaces(blob)
    i = int(dom.index[j])
    lo, hi = f[i, 4:7].astype(np.float64), f[i, 8:11].astype(np.float64)
    lo, hi = np.where(np.abs(lo) <= F.OPEN, lo, -1.0), np.where(np.abs(hi) <= F.OPEN, hi, 1.0)
    if dom.plane[j]:
        lo[dom.pk[j]] = hi[dom.pk[j]] = 0.0
    loc = lo + rng.uniform(0, 1, (n, 3)) * (hi - lo)
    if not dom.plane[j]:
        sci, scj = dom.sci[j], dom.scj[j]
        with np.errstate(all="ignore"):
            for _ in range(6):
                g = 2.0 * (sci[0:3] * loc - scj)
                loc = loc - (((sci[0:3] * loc * loc - 2.0 * scj * loc).sum(axis=1) - sci[3]) / (g * g).sum(axis=1))[:, None] * g
        ok = np.isfinite(loc).all(axis=1)
        ok &= (~dom.has_mn[j] | (loc >= dom.mn[j])).all(axis=1) & (~dom.has_mx[j] | (loc <= dom.mx[j])).all(axis=1)
        loc = loc[ok]
    return world_of(dom, np.full(len(loc), j), loc)


@pytest.mark.parametrize("name", sorted(UNSEEN))
def test_unseen_surfaces_cannot_be_seen(name):
    """every surface that UNSEEN excuses from the coverage count is what the header says of it: empty (a min bound above its max
    bound), wholly clipped away (its clipper program keeps none of 4 000 points sampled on it), or lying in the plane of the
    surface named, inside that surface's bounds (every sampled point within POS_MARGIN of it)"""
    blob, dom = load_blob(name), domain(name)
    where = {int(i): j for j, i in enumerate(dom.index)}
    for srf, why in UNSEEN[name].items():
        j = where[srf]
        assert dom.xf[j] or dom.has_clip[j]
        if why == "empty":
            assert (dom.has_mn[j] & dom.has_mx[j] & (dom.mn[j] > dom.mx[j])).any(), f"{name} {srf}: its bounds admit points"
            continue
        h = _sample_surface(dom, blob, j)
        assert len(h) >= 1000
        if why == "clipped":
            ct, cf, _ = dom._run(dom.prog[j], h, np.zeros(len(h)))
            assert not (ct & ~cf).any(), f"{name} {srf}: its clipper program keeps {(ct & ~cf).mean():.4f} of the sampled points"
            continue
        k = where[why]
        assert dom.plane[k]
        p = (h - dom.P[k]) @ dom.M[k].T - dom.Q[k]
        inside = (~dom.has_mn[k] | (p >= dom.mn[k] - F.POS_MARGIN)).all(axis=1) & (~dom.has_mx[k] | (p <= dom.mx[k] + F.POS_MARGIN)).all(axis=1)
        assert (inside & (np.abs(p[:, dom.pk[k]]) < F.POS_MARGIN)).all(), f"{name} {srf}: not wholly in the plane of {why}"


@pytest.mark.parametrize("name, fam", pairs(CPU_SCENES))
def test_oracle_trace_and_occlusion(oracle, rays_mod, name, fam):
    blob, dom = load_blob(name), domain(name)
    rays, c1, _, _ = case(name, fam, rays_mod)
    t, ids = oracle.trace_rays(blob, rays, "trace", threads=16)
    T.compare_trace(f"{name} {fam}", dom, rays, c1, t, ids, tb=T_BOUND_X)
    T.compare_occluded(f"{name} {fam}", c1, oracle.trace_rays(blob, rays, "occluded", threads=16))


@pytest.mark.parametrize("name, fam", pairs(CPU_SCENES))
def test_oracle_layers(oracle, rays_mod, name, fam):
    blob, dom = load_blob(name), domain(name)
    rays, _, sub, c8 = case(name, fam, rays_mod)
    cnt, t, ids = rays_mod.layers_of(lambda r: oracle.trace_rays(blob, r, "trace", threads=16), rays[sub], K)
    T.compare_layers(f"{name} {fam} layers", dom, rays[sub], c8, cnt, t, ids, tb=T_BOUND_X)


@pytest.mark.parametrize("name, fam", pairs(CPU_SCENES))
def test_oracle_hit_records(helper, rays_mod, name, fam):
    """the hit-record oracle, which is pinned to the reference, stays inside the pos and nrm bounds with 4x room"""
    blob, dom = load_blob(name), domain(name)
    rays, c1, _, _ = case(name, fam, rays_mod)
    rec = helper(blob, rays)
    T.compare_trace(f"{name} {fam} records", dom, rays, c1, rec[:, 3], rec.view(np.int32)[:, 7], tb=T_BOUND_X)
    pr, nr = compare_records(f"{name} {fam}", dom, rays, c1, rec)
    assert pr <= 0.25 and nr <= 0.25, f"{name} {fam}: the oracle uses {pr:.3g} / {nr:.3g} of the pos / nrm bounds: less than 4x room"


@pytest.mark.parametrize("name", GPU_SCENES)
def test_oracle_view_rays(helper, rays_mod, name):
    """the rays of the GPU tests' view_hits case"""
    dom = domain(name)
    view, rays, c1 = view_case(name, rays_mod)
    assert 1 - c1["decided"].mean() <= CAP_UNDECIDED
    rec = helper(load_blob(name), rays)
    hit = T.compare_trace(f"{name} view", dom, rays, c1, rec[:, 3], rec.view(np.int32)[:, 7], tb=T_BOUND_X)
    assert hit.sum() >= 500
    compare_records(f"{name} view", dom, rays, c1, rec)


# ---- teeth: the oracle runs on an altered snapshot, the caster on the original; decided rays must disagree

def _altered(blob, edit):
    """the snapshot with edit(s, f, e) applied to its surface records (int32 and float32 views) and elements"""
    b = bytearray(blob)
    h = _rayq._hdr(b)
    s = np.frombuffer(b, dtype=np.int32, count=h[4] * 64, offset=h[11]).reshape(h[4], 64).copy()
    e = np.frombuffer(b, dtype=np.int32, count=h[7] * 4, offset=h[14]).reshape(h[7], 4).copy()
    edit(s, s.view(np.float32), e)
    b[h[11]:h[11] + s.nbytes] = s.tobytes()
    b[h[14]:h[14] + e.nbytes] = e.tobytes()
    return bytes(b)


def _teeth(oracle, rays_mod, name, fam, edit, match="another surface|the other side|t off by"):
    blob, dom = load_blob(name), domain(name)
    rays, c1, _, _ = case(name, fam, rays_mod)
    t, ids = oracle.trace_rays(blob, rays, "trace", threads=16)
    T.compare_trace(f"{name} {fam}, true scene", dom, rays, c1, t, ids, tb=T_BOUND_X)
    t, ids = oracle.trace_rays(_altered(blob, lambda s, f, e: edit(s, f, e, dom, c1)), rays, "trace", threads=16)
    with pytest.raises(AssertionError, match=match):
        T.compare_trace(f"{name} {fam}, altered scene", dom, rays, c1, t, ids, tb=T_BOUND_X)


def _most_hit(dom, c1, mask):
    """the real surface (its index in the snapshot) of `mask` (over real surfaces) with the most decided closest hits"""
    ids = c1["id"][0][c1["decided"] & (c1["id"][0] >= 0)] >> 1
    best = max((int(i) for i in dom.index[mask]), key=lambda i: int((ids == i).sum()))
    assert (ids == best).sum() >= 20
    return best


def test_teeth_trnode_transposed(oracle, rays_mod):
    """the matrix of the trnode with the most decided hits under it transposed: a rotation turned the other way"""
    def edit(s, f, e, dom, c1):
        i = _most_hit(dom, c1, dom.under)
        t = int(s[i, 39])
        m = np.stack([f[t, 12:15], f[t, 16:19], f[t, 20:23]]).copy()
        assert np.abs(m - m.T).max() > 0.1
        f[t, 12:15], f[t, 16:19], f[t, 20:23] = m.T[0], m.T[1], m.T[2]
    _teeth(oracle, rays_mod, "test13_160", "camera", edit)


def test_teeth_own_scale_negated(oracle, rays_mod):
    """the local z row of an own transform negated on a surface clipped at a local z bound: the other half shows"""
    def edit(s, f, e, dom, c1):
        half = dom.own & ~dom.plane & (dom.has_mn[:, 2] ^ dom.has_mx[:, 2])
        f[_most_hit(dom, c1, half), 20:23] *= np.float32(-1.0)
    _teeth(oracle, rays_mod, "test12_160_j8", "aimed", edit)


def test_teeth_clipper_side(oracle, rays_mod):
    """the side (data) of the one plain clipper of the most-hit clipped plane flipped"""
    def edit(s, f, e, dom, c1):
        plain = np.array([dom.has_clip[j] and len(dom.prog[j]) == 1 and dom.prog[j][0][0] == "clip" for j in range(len(dom.index))])
        el = [x for x in X.clip_list(load_blob("demo01_160"), _most_hit(dom, c1, plain)) if s[x[1], 37] >= 0]
        assert len(el) == 1
        e[el[0][0], 1] = -e[el[0][0], 1]
    _teeth(oracle, rays_mod, "demo01_160", "aimed", edit)


def test_teeth_accumulator_pair_removed(oracle, rays_mod):
    """the enter and leave markers of the hyperboloid's clipper list unlinked: it keeps what its six planes enclose, not the rest"""
    def edit(s, f, e, dom, c1):
        i = int(dom.index[np.nonzero(dom.has_group)[0][0]])
        lst = X.clip_list(load_blob("test03_160_j18"), i)
        assert lst[0][1] == -1 and lst[0][2] <= 0 and lst[-1][1] == -1 and lst[-1][2] > 0
        s[i, 38] = lst[1][0]
        e[lst[-2][0], 2] = -1
    _teeth(oracle, rays_mod, "test03_160_j18", "aimed", edit)


def test_teeth_q_moved(oracle, rays_mod):
    """pos of the most-hit plane under a trnode (its Q, in the trnode's space) moved by 0.05 along the plane's normal axis"""
    def edit(s, f, e, dom, c1):
        i = _most_hit(dom, c1, dom.under & dom.plane)
        f[i, (int(s[i, 23]) >> 4) & 3] += np.float32(0.05)
    _teeth(oracle, rays_mod, "test13_160", "aimed", edit)


def test_teeth_normal_transpose(helper, rays_mod):
    """a caster that carries the local gradient through M in place of M^T fails compare_records on the most-hit surface of
    test12_160_j8 whose transform is far from uniform (sigma_max > 1.5 sigma_min)"""
    name = "test12_160_j8"
    blob, dom = load_blob(name), domain(name)
    rays, c1, _, _ = case(name, "aimed", rays_mod)
    srf = _most_hit(dom, c1, dom.own & (dom.smax > 1.5 * dom.smin))
    on = c1["decided"] & ((c1["id"][0] >> 1) == srf)
    sub = {"decided": c1["decided"][on], "id": c1["id"][:, on], "t": c1["t"][:, on]}
    rec = helper(blob, rays[on])
    compare_records(f"{name}, surface {srf}", dom, rays[on], sub, rec)
    wrong = X.XDomain(blob, transpose_normal=False)
    with pytest.raises(AssertionError, match="a normal is off"):
        compare_records(f"{name}, surface {srf}, M for M^T", wrong, rays[on], sub, rec)


# --------------------------------------------------------------------------------------------------------------------- GPU

_SCENES = {}


@pytest.fixture(scope="module")
def scenes(qr):
    def get(name):
        if name not in _SCENES:
            _SCENES[name] = qr.Scene(load_blob(name), ray_queries=True)
        return _SCENES[name]
    yield get
    for s in _SCENES.values():
        s.close()
    _SCENES.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("name, fam", pairs(GPU_SCENES))
def test_gpu_trace_occluded_hits(scenes, rays_mod, name, fam):
    scn, dom = scenes(name), domain(name)
    rays, c1, _, _ = case(name, fam, rays_mod)
    r = T._dev(scn, rays)
    for coherent in (False, True):
        t, ids = T._host(*scn.trace(r, coherent=coherent))
        T.compare_trace(f"{name} {fam} coherent={coherent}", dom, rays, c1, t, ids, tb=T_BOUND_X)
    occ, rec = T._host(scn.occluded(r), scn.hits(r))
    T.compare_occluded(f"{name} {fam}", c1, occ)
    T.compare_trace(f"{name} {fam} hits", dom, rays, c1, rec[:, 3], rec.view(np.int32)[:, 7], tb=T_BOUND_X)
    compare_records(f"{name} {fam}", dom, rays, c1, rec)


@pytest.mark.gpu
@pytest.mark.parametrize("name, fam", pairs(GPU_SCENES))
def test_gpu_layers(scenes, rays_mod, name, fam):
    scn, dom = scenes(name), domain(name)
    rays, _, sub, c8 = case(name, fam, rays_mod)
    cnt, t, ids, rec = T._host(*scn.trace_layers(T._dev(scn, rays[sub]), K, hits=True))
    where = f"{name} {fam} layers"
    T.compare_layers(where, dom, rays[sub], c8, cnt, t, ids, tb=T_BOUND_X)
    assert (rec.view(np.int32)[:, :, 7] == ids).all() and (rec[:, :, 3].view(np.uint32) == t.view(np.uint32)).all(), f"{where}: the records name other hits"
    stats = {}
    for j in range(K):                                              # every layer's record against that crossing
        layer = {"decided": c8["decided"], "id": c8["id"][j:j + 1], "t": c8["t"][j:j + 1]}
        if (layer["decided"] & (layer["id"][0] >= 0)).any():
            compare_records(f"{where} {j}", dom, rays[sub], layer, rec[j], stats)
    print(f"{where}: all layers' records use at most {stats.get('pos', 0):.3g} / {stats.get('nrm', 0):.3g} of the pos / nrm bounds")


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_SCENES)
def test_gpu_view_hits(scenes, rays_mod, name):
    scn, dom = scenes(name), domain(name)
    view, rays, c1 = view_case(name, rays_mod)
    rec, = T._host(scn.view_hits(T._dev(scn, view[None]), 67, 45))
    rec = rec.reshape(-1, 12)
    hit = T.compare_trace(f"{name} view", dom, rays, c1, rec[:, 3], rec.view(np.int32)[:, 7], tb=T_BOUND_X)
    assert hit.sum() >= 500
    compare_records(f"{name} view", dom, rays, c1, rec)
