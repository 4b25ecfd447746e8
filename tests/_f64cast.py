"""A float64 ray caster over untransformed, unclipped surfaces, for tests/test_f64_caster.py: the geometry of the ray contract
(include/qrhip.h, "Ray queries") stated a third time, by plain numpy, sharing nothing with oracle/ or rays.py.

Domain: the real surfaces of a snapshot (tests/_rayq.py real_surfaces) as synth.py and tests/_crowd.py write them -- tags 0..8,
axis-aligned, untransformed, without clipper lists, any axis map whose three 2-bit fields are a permutation of 0, 1, 2 -- and
nothing else of the snapshot: no element list, bounding volume, tile or grid.  A transform (has_trm), shift, a clipper list, a
trnode, a malformed axis map or a record with a solver whose tag lies outside 0..8 is an error (Domain.__init__ asserts), never
a skipped surface.  tests/_f64xform.py carries the caster to transforms, trnodes and clipper lists (XDomain, a subclass).

Geometry, with loc = org + t * dir - pos, in world axes (sci and scj are stored per world axis; the axis map matters to planes
alone):
  plane    loc[k] = 0 with k = map_k = (axes >> 4) & 3, so t = -(org - pos)[k] / dir[k]; sgn = -1 where bit 10 of axes is set
  quadric  F(loc) = sum sci[a] loc[a]^2 - 2 sum scj[a] loc[a] - sci[3] = 0.  Along the ray F = A t^2 + 2 B t + C; the roots are
           q / A and C / q with q = -(B + sgn(B) sqrt(B^2 - A C)): no cancellation.  Mixed signs and zero coefficients (tags 5..8)
           need no case of their own.  A == 0 -- a ray along a cylinder's axis, a paraboloid's or paracylinder's open direction,
           an asymptote of a hyperbolic kind, one of a hypercylinder's two planes -- leaves the one root C / q = -C / 2B, and
           none when B == 0 too (q == 0); B == 0 alone gives q = -sqrt(-A C) and the roots -+ sqrt(-C / A).  The two-plane
           solver (tag 7: sci[j] = scj = sci[3] = 0) solves this same F.
  a root is a hit iff tmin < t < tmax (+inf: FLT_MAX) and min[a] <= loc[a] <= max[a] on the axes flagged in minmax_t; a
           flagged bound beyond 1e30 (the endless members') never clips, and minmax_t == 0 clips nothing
  side     1 iff grad F . dir > 0 (dF/dt = 2 (A t + B) > 0): the hit names the side the ray arrives on; planes: 1 iff
           sgn * dir[k] > 0.  On conic != 0 surfaces -- cones and hyperboloids (1), hypercylinders (2) alike -- the solver names
           the side by root order (qrhip.h; oracle/qr_oracle.c quadric_roots: the sign of A picks which root is "outer"):
           compare the surface index only there.
  normal   -+ grad F / |grad F|, facing the ray; planes: -+ sgn * e_k, exactly, the other two components +0.0.

Decided rays.  fp32 cannot decide what lies within its own error of a bound, so every root is ACCEPTED, REJECTED or UNCERTAIN
against the margins below, and a query is answered only where no uncertain root can change the answer:
  POS_MARGIN  scene units, on every active clip bound (plus T_REL * |t| |dir|: the hit point moves with t's error)
  T_REL       relative, on t against tmin and tmax (plus POS_MARGIN / |dir|, absolute)
  GRAZE       a quadric with |B^2 - A C| < GRAZE * (B^2 + |A C|) grazes: one uncertain root at -B / A, its t within
              sqrt(2 GRAZE) |B / A| of that, uncertain when that stretch meets the interval and the clip box with that slack
  APEX        a root on a conic != 0 surface within APEX of the surface's singular set is uncertain, not rejected: the
              renderer's conic-singularity fix (qr_surface.t_eps) moves the hit point there.  The singular set is where
              grad F = 2 (sci loc - scj) = 0: loc[a] = scj[a] / sci[a] on the axes with sci[a] != 0, anything on an axis with
              sci[a] == scj[a] == 0.  A point on cones and hyperboloids, a line on conic == 2 surfaces (the line the two
              planes share; the fix measures loc on map_i and map_k alone there), and |loc| < APEX on the synthetic cones.
  noise       (Margins.noise, in fp32 ulps; 0 = off) a quadric's root is uncertain where fp32's own error in F at the hit
              point, noise * 2^-24 * (sum |sci[a]| loc[a]^2 + 2 sum |scj[a] loc[a]| + |sci[3]|), carried to t through
              dF/dt = 2 (A t + B), exceeds T_REL |t|: there fp32 does not resolve t to the margin the caster itself grants.

The crowd scenes are cast with crowd_margins(): GRAZE_CROWD = 1e-5 and NOISE_CROWD = 4; the synthetic scenes with the
defaults, GRAZE = 1e-4 and no noise rule, so that every figure committed for them stands bit for bit.
  Grazing.  The rule fires on |disc| / scale, which is small for any small object seen from far away, grazing or not: the
  crowd's donors are scaled to radius 0.2..1 in a box of 14..18 units, and a ray along x against x^2 - 2.25 y^2 = 0 from 20
  units away that passes 0.1 off the line has disc / scale of about 3e-5.  fp32's error in disc is a few 2^-24 of scale, two
  orders of magnitude below even 1e-5.  A probe at 1e-4 left 3.6 % to 30 % of a family's rays undecided for the closest hit
  and up to 45 % for the layers; at 1e-5 it is 2.7 % to 10.1 % and up to 15.4 % (tests/test_f64_caster.py's table), and the
  oracle agrees with the caster on every decided ray at that value.
  Noise.  Found while reading a disagreement: rays that start inside the box of a cap 0.004 thick cut from a sphere of radius
  4.7 to 18.75 -- 0.004 from a surface whose pos is that far away -- and run along it for a few tenths of a unit.  The
  reference's solver, like the oracle and the kernels, evaluates F about pos in fp32 (oracle/qr_oracle.c QD_ptr), so C and
  the hit point carry 2^-24 of 2 R^2 = 700 while |dF/dt| |t| is 0.1: t came out 1.4e-4 to 1.5e-3 off, relatively, and within
  POS_MARGIN in space.  The error was 0.1 to 1.1 times the rule's expression with noise = 1 on every such ray; 4 allows three
  roundings a term and the sum's.  It takes the decision from 8 + 28 of the crowds' 3 536 + 8 080 `aimed` rays and from no
  ray of another family.  It would mark 23 decided roots of synth_dense_dda's `inside` family as well (short rays off nearby surfaces; that family
  holds the synthetic scenes' largest t difference, 4.14e-5): they stay decided, as committed.
"""
import numpy as np

import _rayq

POS_MARGIN = 1e-3
T_REL = 1e-4
GRAZE = 1e-4
GRAZE_CROWD = 1e-5
NOISE_CROWD = 4.0
APEX = 1e-2
OPEN = 1e30

FLT_MAX = float(np.finfo(np.float32).max)
REJECTED, ACCEPTED, UNCERTAIN = 0, 1, 2
TAGS = {0: "plane", 1: "cylinder", 2: "sphere", 3: "cone", 4: "paraboloid", 5: "hyperboloid", 6: "paracylinder",
        7: "hypercylinder", 8: "hyperparaboloid"}


class Margins:
    def __init__(self, pos=POS_MARGIN, t_rel=T_REL, graze=GRAZE, apex=APEX, noise=0.0):
        self.pos, self.t_rel, self.graze, self.apex, self.noise = pos, t_rel, graze, apex, noise


def crowd_margins():
    """the margins of the crowd scenes (the module's text: "The crowd scenes")"""
    return Margins(graze=GRAZE_CROWD, noise=NOISE_CROWD)


class Domain:
    """the real surfaces of a snapshot as float64 arrays; closed / flip_side are the teeth tests' deliberate errors"""

    def __init__(self, blob, closed=False, flip_side=False):
        s, f = _rayq.surfaces(blob)
        real = _rayq.real_surfaces(blob)
        assert len(real) > 0
        assert (s[real, 15] == 0).all(), "a transformed surface: outside the caster's domain"
        assert (s[real, 38] == -1).all(), "a surface with a clipper list: outside the caster's domain"
        assert (s[real, 39] == -1).all(), "a surface under a trnode: outside the caster's domain"
        assert (s[real, 19] == 0).all(), "a surface that reads its trnode's fields (shift): outside the caster's domain"
        maps = np.stack([(s[real, 23] >> (2 * a)) & 3 for a in range(3)], axis=1)
        assert (np.sort(maps, axis=1) == (0, 1, 2)).all(), "a malformed axis map: outside the caster's domain"
        tag = s[real, 37]
        other = np.ones(len(s), dtype=bool)
        other[real] = False
        # arrays and bounding volumes carry no solver (srf_t[0] == 0); a record that has one is a surface the walks intersect
        assert np.isin(tag, list(TAGS)).all() and (s[other, 34] == 0).all(), "a surface kind outside tags 0..8: outside the caster's domain"
        self.index = real.astype(np.int64)
        self.all_conic, self.all_tag = s[:, 11] != 0, s[:, 37].copy()          # by surface index, for the tests
        self.all_axes, self.all_minmax = s[:, 23].copy(), s[:, 7] & 63
        self.tag = tag
        self.plane = tag == 0
        self.conic = s[real, 11] != 0
        self.pos = f[real, 0:3].astype(np.float64)
        self.mn = f[real, 4:7].astype(np.float64)
        self.mx = f[real, 8:11].astype(np.float64)
        mm = s[real, 7]
        self.has_mn = np.stack([(mm >> a) & 1 for a in range(3)], axis=1).astype(bool)
        self.has_mx = np.stack([(mm >> (3 + a)) & 1 for a in range(3)], axis=1).astype(bool)
        assert not (self.has_mn & (self.mn > OPEN)).any() and not (self.has_mx & (self.mx < -OPEN)).any(), "a clip bound that clips everything"
        self.has_mn &= self.mn >= -OPEN                             # a flagged bound beyond 1e30: an endless member's, it never clips
        self.has_mx &= self.mx <= OPEN
        self.sci = f[real, 24:28].astype(np.float64)
        self.scj = f[real, 28:31].astype(np.float64)
        # planes: the normal axis map_k and its sign (bit 10: -e_k)
        self.pk = maps[:, 2].astype(np.int64)
        self.psgn = np.where((s[real, 23] >> 10) & 1, -1.0, 1.0)
        # the singular set, where grad F = 2 (sci loc - scj) = 0: loc[a] = scj[a] / sci[a] on the axes with sci[a] != 0, any
        # loc[a] on those with sci[a] == scj[a] == 0 (free), nowhere when an axis has sci[a] == 0 != scj[a]
        sci3 = self.sci[:, 0:3]
        with np.errstate(all="ignore"):
            self.sing = np.where(sci3 != 0, self.scj / sci3, 0.0)
        self.sing_axes = sci3 != 0
        self.has_sing = ~((sci3 == 0) & (self.scj != 0)).any(axis=1)
        self.turn = np.where(self.plane, 1.0, np.abs(sci3).max(axis=1))         # the normal bound's factor: max |sci[a]|
        self.casts = _rayq.casts(blob)[real]                        # [S, 2]
        self.closed, self.flip_side = closed, flip_side

    # -- roots of a chunk of rays against every surface -------------------------------------------------------------------
    def _roots(self, rays, m):
        """the roots that are not rejected -- the two roots and the grazing stand-in of every surface -- as flat arrays (ray,
        surface, state, t, t_lo, side): t_lo is where an uncertain root may begin (t itself for the others)"""
        o = rays[:, 0:3].astype(np.float64)
        d = rays[:, 4:7].astype(np.float64)
        tmin = rays[:, 3].astype(np.float64)[:, None]
        tmax = np.minimum(rays[:, 7].astype(np.float64), FLT_MAX)[:, None]
        dl = np.sqrt((d * d).sum(axis=1))[:, None]                  # [n, 1]
        # F along the ray, A t^2 + 2 B t + C, as products of [n, 3] and [S, 3] matrices: with l0 = org - pos,
        # A = sum sci d^2, B = sum d (sci l0 - scj), C = sum l0 (sci l0 - 2 scj) - sci[3], expanded in org and pos.  float64
        # leaves 1e-13 of a scene's size squared after the cancellation: a root moves by less than 1e-9 of itself, five digits below
        # the margins.
        sci = self.sci[:, 0:3]
        w = sci * self.pos + self.scj                               # [S, 3]
        k0 = (self.pos * (sci * self.pos + 2.0 * self.scj)).sum(axis=1) - self.sci[:, 3]
        with np.errstate(all="ignore"):
            dot = lambda x, y: np.einsum("na,sa->ns", x, y)         # [n, 3] . [S, 3]: far quicker than a BLAS call at depth 3
            A = dot(d * d, sci)
            B = dot(d * o, sci) - dot(d, w)
            C = dot(o * o, sci) - 2.0 * dot(o, w) + k0[None]
            disc = B * B - A * C
            scale = B * B + np.abs(A * C)
            # few pairs of ray and surface have a root: from here on flat arrays over the pairs that may (every plane; quadrics
            # whose discriminant is positive or within the grazing band)
            pr, ps = np.nonzero(self.plane[None] | (disc > -m.graze * scale))
            A, B, C, disc, scale = A[pr, ps], B[pr, ps], C[pr, ps], disc[pr, ps], scale[pr, ps]
            plane = self.plane[ps]
            graze = (np.abs(disc) < m.graze * scale) & ~plane
            q = -(B + np.where(B >= 0, 1.0, -1.0) * np.sqrt(np.maximum(disc, 0.0)))
            none = (disc < 0) | graze
            r1 = np.where(none | (A == 0), np.nan, q / A)           # A == 0: a ray along a cylinder's or paraboloid's axis
            r2 = np.where(none | (q == 0), np.nan, C / q)
            pk = self.pk[ps]
            tp = -(o[pr, pk] - self.pos[ps, pk]) / d[pr, pk]        # planes: loc[map_k] = 0
            r1 = np.where(plane, tp, r1)
            r2 = np.where(plane, np.nan, r2)
            mid = np.where(graze & (A != 0), -B / A, np.nan)
            slack = np.sqrt(2.0 * m.graze) * np.abs(mid)
        out = [self._classify(pr, ps, t, slk, o, d, dl, A, B, tmin, tmax, m) for t, slk in ((r1, None), (r2, None), (mid, slack))]
        return [np.concatenate([x[j] for x in out]) for j in range(6)]

    def _classify(self, pr, ps, t, slack, o, d, dl, A, B, tmin, tmax, m):
        """the roots t (flat, over the pairs of ray pr and surface ps; nan or inf: none) that are not rejected:
        (ray, surface, state, t, t_lo, side)"""
        with np.errstate(all="ignore"):
            # the interval first (it rejects most roots): fp32's t is off relative to itself, and near a bound it is the bound's size
            lo_b, hi_b, dn = tmin[pr, 0], tmax[pr, 0], dl[pr, 0]
            sl = np.zeros(len(pr)) if slack is None else slack
            inside = ((t >= lo_b) & (t <= hi_b)) if self.closed else ((t > lo_b) & (t < hi_b))
            near = ((np.abs(t - lo_b) < m.t_rel * np.abs(lo_b) + m.pos / dn + sl) |
                    (np.abs(t - hi_b) < m.t_rel * np.abs(hi_b) + m.pos / dn + sl))     # strict: a zero margin is never near
            have = np.isfinite(t) & (inside | near)
            ri, si, A, B, t0, sl, dn, near = pr[have], ps[have], A[have], B[have], t[have], sl[have], dn[have], near[have]
            dd = d[ri]
            loc = (o[ri] - self.pos[si]) + t0[:, None] * dd
            # the clip box, bounds inclusive
            mp = (m.pos + m.t_rel * np.abs(t0) * dn + sl * dn)[:, None]
            hm, hx, mn, mx = self.has_mn[si], self.has_mx[si], self.mn[si], self.mx[si]
            edge = ((hm & (np.abs(loc - mn) < mp)) | (hx & (np.abs(loc - mx) < mp))).any(axis=1)
            clip_rej = ((hm & (loc < mn)) | (hx & (loc > mx))).any(axis=1) & ~edge
            off = np.where(self.sing_axes[si], loc - self.sing[si], 0.0)        # from the singular set: a point or a line
            apex = self.conic[si] & self.has_sing[si] & ((off * off).sum(axis=1) < m.apex * m.apex)
            # fp32's own noise in F at the root, carried to t through dF/dt = 2 (A t + B), against what T_REL allows
            sci, scj = self.sci[si], self.scj[si]
            terms = (np.abs(sci[:, 0:3]) * loc * loc).sum(axis=1) + 2.0 * np.abs(scj * loc).sum(axis=1) + np.abs(sci[:, 3])
            blur = ~self.plane[si] & (m.noise * 2.0 ** -24 * terms > m.t_rel * np.abs(t0) * 2.0 * np.abs(A * t0 + B))
            st = np.full(len(ri), ACCEPTED, dtype=np.int8)
            st[near | edge | apex | blur] = UNCERTAIN
            if slack is not None:
                st[:] = UNCERTAIN
            st[clip_rej & ~apex] = REJECTED
            sd = np.where(self.plane[si], self.psgn[si] * dd[np.arange(len(si)), self.pk[si]] > 0, (A * t0 + B) > 0)
            if self.flip_side:
                sd = ~sd
        keep = st != REJECTED
        return ri[keep], si[keep], st[keep], t0[keep], (t0 - sl)[keep], sd[keep]

    # -- queries ------------------------------------------------------------------------------------------------------------
    def cast(self, rays, k=1, margins=None, chunk=1024):
        """The first k hits of every ray.  Returns a dict of
          count   int [N]      accepted hits found, 0..k
          id      int [k, N]   surface << 1 | side of the j-th accepted hit, -1 from `count` on
          t       f64 [k, N]   its t (inf from `count` on)
          decided bool [N]     no uncertain root lies before the k-th accepted root plus its margin (before the interval's end
                               where fewer than k are found), and consecutive accepted roots -- the k + 1-th included -- lie a
                               margin apart
          occ, occ_decided     is a casting side hit in the interval / is that certain"""
        m = margins or Margins()
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        n = len(rays)
        res = dict(count=np.zeros(n, dtype=np.int64), id=np.full((k, n), -1, dtype=np.int64), t=np.full((k, n), np.inf),
                   decided=np.zeros(n, dtype=bool), occ=np.zeros(n, dtype=bool), occ_decided=np.zeros(n, dtype=bool))
        both, one = self.casts.all(axis=1), self.casts.any(axis=1)
        for c0 in range(0, n, chunk):
            r = rays[c0:c0 + chunk]
            nn = len(r)
            ri, si, st, tt, lo, sd = self._roots(r, m)
            acc, unc = st == ACCEPTED, st == UNCERTAIN
            any_of = lambda mask: np.bincount(ri[mask], minlength=nn) > 0
            # occlusion: the side hit decides whether a root casts; on a conic surface the solver names the side by root order,
            # so a root there casts for certain only where both sides do
            cast = np.where(self.conic[si], both[si], self.casts[si, sd.astype(np.int64)])
            occ = any_of(acc & cast)
            occ_unc = any_of((unc & one[si]) | (acc & self.conic[si] & one[si] & ~both[si]))
            res["occ"][c0:c0 + nn] = occ
            res["occ_decided"][c0:c0 + nn] = occ | ~occ_unc
            # the accepted roots of every ray in order: the first k + 1 as tp [nn, k + 1], inf where there is none
            a_ri, a_t = ri[acc], tt[acc]
            a_id = (self.index[si[acc]] << 1) | sd[acc].astype(np.int64)
            order = np.lexsort((a_t, a_ri))
            a_ri, a_t, a_id = a_ri[order], a_t[order], a_id[order]
            rank = np.arange(len(a_ri)) - np.searchsorted(a_ri, a_ri, side="left")
            first = rank <= k
            tp = np.full((nn, k + 1), np.inf)
            ids = np.full((nn, k + 1), -1, dtype=np.int64)
            tp[a_ri[first], rank[first]] = a_t[first]
            ids[a_ri[first], rank[first]] = a_id[first]
            cnt = np.isfinite(tp[:, :k]).sum(axis=1)
            res["count"][c0:c0 + nn] = cnt
            res["id"][:, c0:c0 + nn] = ids[:, :k].T
            res["t"][:, c0:c0 + nn] = tp[:, :k].T
            # decided
            pos_t = m.pos / np.linalg.norm(r[:, 4:7].astype(np.float64), axis=1)[:, None]       # the position margin in t
            with np.errstate(invalid="ignore"):
                mg = np.where(np.isfinite(tp), m.t_rel * np.abs(tp) + pos_t, 0.0)               # [nn, k + 1]: a root's margin
            kth = np.where(cnt == k, tp[:, k - 1] + mg[:, k - 1], np.inf)       # k found: nothing behind the k-th matters
            unc_lo = np.full(nn, np.inf)
            np.minimum.at(unc_lo, ri[unc], lo[unc])
            dec = ~(np.isfinite(unc_lo) & (unc_lo <= kth))
            with np.errstate(invalid="ignore"):
                close = np.isfinite(tp[:, 1:]) & (tp[:, 1:] - tp[:, :-1] <= 2.0 * mg[:, 1:])    # the k + 1-th against the k-th too
            dec &= ~close.any(axis=1)
            res["decided"][c0:c0 + nn] = dec
        return res

    def hit_point(self, rays, hit_id, t):
        """(pos f64 [N, 3], unit normal f64 [N, 3] facing by the id's side bit, |grad F| [N], max |sci[a]| [N]: how fast the
        gradient turns, 1 on planes) of hits (id >= 0) at float64 t"""
        where = np.full(len(self.all_tag), -1, dtype=np.int64)
        where[self.index] = np.arange(len(self.index))
        j = where[np.asarray(hit_id, dtype=np.int64) >> 1]
        assert (j >= 0).all(), "a hit on something that is no real surface"
        o = rays[:, 0:3].astype(np.float64)
        d = rays[:, 4:7].astype(np.float64)
        p = o + t[:, None] * d
        loc = p - self.pos[j]
        g = 2.0 * (self.sci[j, 0:3] * loc - self.scj[j])
        pl = np.nonzero(self.plane[j])[0]
        g[pl] = 0.0
        g[pl, self.pk[j[pl]]] = self.psgn[j[pl]]                    # planes: sgn * e_k stands for grad F
        gl = np.linalg.norm(g, axis=1)
        sign = np.where((np.asarray(hit_id) & 1) == 1, -1.0, 1.0)  # side 1: grad F along the ray, the normal faces back
        with np.errstate(all="ignore"):
            n = g / gl[:, None] * sign[:, None]
        return p, n, gl, self.turn[j]
