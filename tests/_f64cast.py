"""A float64 ray caster over the synthetic scenes' surfaces, for tests/test_f64_caster.py: the geometry of the ray contract
(include/qrhip.h, "Ray queries") stated a third time, by plain numpy, sharing nothing with oracle/ or rays.py.

Domain: the real surfaces of a snapshot (tests/_rayq.py real_surfaces) as synth.py writes them -- axis-aligned, untransformed,
without clipper lists -- and nothing else of the snapshot: no element list, bounding volume, tile or grid.  A real surface with
a transform, a clipper list, a trnode or another axis map is an error (Domain.__init__ asserts), never a skipped surface.

Geometry, with loc = org + t * dir - pos:
  plane    loc[2] = 0
  quadric  F(loc) = sum sci[a] loc[a]^2 - 2 sum scj[a] loc[a] - sci[3] = 0.  Along the ray F = A t^2 + 2 B t + C; the roots are
           q / A and C / q with q = -(B + sgn(B) sqrt(B^2 - A C)): no cancellation.  A == 0: the one root C / q = -C / 2B.
  a root is a hit iff tmin < t < tmax (+inf: FLT_MAX) and min[a] <= loc[a] <= max[a] on the axes flagged in minmax_t
  side     1 iff grad F . dir > 0 (dF/dt = 2 (A t + B) > 0): the hit names the side the ray arrives on; planes: 1 iff dir[2] > 0.
           On conic != 0 surfaces the solver names the side by root order (qrhip.h): compare the surface index only there.
  normal   -+ grad F / |grad F|, facing the ray (planes: -+ e_z).

Decided rays.  fp32 cannot decide what lies within its own error of a bound, so every root is ACCEPTED, REJECTED or UNCERTAIN
against the three margins below, and a query is answered only where no uncertain root can change the answer:
  POS_MARGIN  scene units, on every active clip bound (plus T_REL * |t| |dir|: the hit point moves with t's error)
  T_REL       relative, on t against tmin and tmax (plus POS_MARGIN / |dir|, absolute)
  GRAZE       a quadric with |B^2 - A C| < GRAZE * (B^2 + |A C|) grazes: one uncertain root at -B / A, its t within
              sqrt(2 GRAZE) |B / A| of that, uncertain when that stretch meets the interval and the clip box with that slack
  APEX        a root on a conic != 0 surface with |loc| < APEX is uncertain, not rejected: the renderer's conic-singularity
              fix (qr_surface.t_eps) moves the hit point there.
"""
import numpy as np

import _rayq

POS_MARGIN = 1e-3
T_REL = 1e-4
GRAZE = 1e-4
APEX = 1e-2

FLT_MAX = float(np.finfo(np.float32).max)
REJECTED, ACCEPTED, UNCERTAIN = 0, 1, 2
TAGS = {0: "plane", 1: "cylinder", 2: "sphere", 3: "cone", 4: "paraboloid"}


class Margins:
    def __init__(self, pos=POS_MARGIN, t_rel=T_REL, graze=GRAZE, apex=APEX):
        self.pos, self.t_rel, self.graze, self.apex = pos, t_rel, graze, apex


class Domain:
    """the real surfaces of a snapshot as float64 arrays; closed / flip_side are the teeth tests' deliberate errors"""

    def __init__(self, blob, closed=False, flip_side=False):
        s, f = _rayq.surfaces(blob)
        real = _rayq.real_surfaces(blob)
        assert len(real) > 0
        assert (s[real, 15] == 0).all(), "a transformed surface: outside the caster's domain"
        assert (s[real, 38] == -1).all(), "a surface with a clipper list: outside the caster's domain"
        assert (s[real, 39] == -1).all(), "a surface under a trnode: outside the caster's domain"
        assert (s[real, 23] == 0x024).all(), "a surface with another axis map: outside the caster's domain"
        tag = s[real, 37]
        assert np.isin(tag, list(TAGS)).all(), "a surface kind synth.py does not write"
        self.index = real.astype(np.int64)
        self.all_conic, self.all_tag = s[:, 11] != 0, s[:, 37].copy()          # by surface index, for the tests
        self.tag = tag
        self.plane = tag == 0
        self.conic = s[real, 11] != 0
        self.pos = f[real, 0:3].astype(np.float64)
        self.mn = f[real, 4:7].astype(np.float64)
        self.mx = f[real, 8:11].astype(np.float64)
        mm = s[real, 7]
        self.has_mn = np.stack([(mm >> a) & 1 for a in range(3)], axis=1).astype(bool)
        self.has_mx = np.stack([(mm >> (3 + a)) & 1 for a in range(3)], axis=1).astype(bool)
        self.sci = f[real, 24:28].astype(np.float64)
        self.scj = f[real, 28:31].astype(np.float64)
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
            tp = -(o[pr, 2] - self.pos[ps, 2]) / d[pr, 2]           # planes: loc[2] = 0
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
            apex = self.conic[si] & ((loc * loc).sum(axis=1) < m.apex * m.apex)
            st = np.full(len(ri), ACCEPTED, dtype=np.int8)
            st[near | edge | apex] = UNCERTAIN
            if slack is not None:
                st[:] = UNCERTAIN
            st[clip_rej & ~apex] = REJECTED
            sd = np.where(self.plane[si], dd[:, 2] > 0, (A * t0 + B) > 0)
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
        """(pos f64 [N, 3], unit normal f64 [N, 3] facing by the id's side bit, |grad F| [N]) of hits (id >= 0) at float64 t"""
        where = np.full(len(self.all_tag), -1, dtype=np.int64)
        where[self.index] = np.arange(len(self.index))
        j = where[np.asarray(hit_id, dtype=np.int64) >> 1]
        assert (j >= 0).all(), "a hit on something that is no real surface"
        o = rays[:, 0:3].astype(np.float64)
        d = rays[:, 4:7].astype(np.float64)
        p = o + t[:, None] * d
        loc = p - self.pos[j]
        g = 2.0 * (self.sci[j, 0:3] * loc - self.scj[j])
        g[self.plane[j]] = (0.0, 0.0, 1.0)
        gl = np.linalg.norm(g, axis=1)
        sign = np.where((np.asarray(hit_id) & 1) == 1, -1.0, 1.0)  # side 1: grad F along the ray, the normal faces back
        with np.errstate(all="ignore"):
            n = g / gl[:, None] * sign[:, None]
        return p, n, gl
