"""The float64 ray caster of tests/_f64cast.py carried to transformed and clipped surfaces, for tests/test_f64_fixtures.py: own
transforms, surfaces under a trnode and clipper lists, as the fixture scenes hold them.  XDomain is a subclass of Domain: the
queries (cast) and every margin are the parent's; what changes is where a surface's equation is evaluated and one more test a
root has to pass.  On the parent's own domain XDomain.cast returns the parent's arrays, bit for bit
(test_old_domain_answers_do_not_move).

Still read from the surfaces alone: no element list of the walk, bounding volume, tile or grid.  A surface's clipper list is part
of the surface's definition and is read (qr_surface.clip; elements simd, data, next).

World to local.  Every real surface i has an affine map loc_i(x) = M (x - P) - Q, and its direction is M d, NOT renormalised, so
that t stays the world ray's t:
  has_trm == 0                          M = I, P = pos_i, Q = 0
  has_trm != 0, trnode == i             own transform: M = rows tci, tcj, tck of i (the diagonal alone when has_trm == 1),
                                        P = pos_i, Q = 0
  has_trm != 0, trnode == T != i        M, P from T's rows and pos (T: a record with a negative tag whose trnode is itself),
                                        Q = pos_i: the surface's pos lies in the trnode's space
No deeper level exists in the fixtures; __init__ asserts that, and that shift (the record's "read the trnode fields") is set
exactly where has_trm is.  Never a skipped surface.

Roots, side, min/max, apex, grazing, noise: the parent's, with loc_i(org) and M d in place of org - pos and dir.  The min/max
bounds and the singular set are local.  A world position margin e becomes sigma_max(M) e locally.  The side stays A t + B > 0
(planes: sgn (M d)[k] > 0), under mirrored M too: grad F . (M d) is the derivative of F along the ray whatever M is.

Transform noise (NOISE_X = 4 fp32 ulps; transformed surfaces only, so the parent's domain is untouched).  Found while reading a
disagreement: demo03_160, an `inside` ray that starts 0.004 in front of a plane under a rotating trnode whose pos lies 10 units
away and meets it at 78 degrees from the normal; the oracle's t = 0.020577 against 0.020565, 5.8e-4 off relatively and 1.2e-5
in space.  The engine -- the reference, the oracle and the kernels alike -- computes the local origin M (org - P) - Q and the
local direction M dir in fp32 (oracle/qr_oracle.c xform: three products and two sums a row), so the local origin carries
about eps_o = NOISE_X 2^-24 (sigma_max |org - P| + |Q|) and the local direction eps_d = NOISE_X 2^-24 sigma_max |dir|; 4 allows
three roundings a term and the sum's, the parent's figure for its own noise rule.  Carried to t through the surface's equation
that is |g_loc| (eps_o + |t| eps_d) / |dF/dt| (planes: over |(M dir)[k]|).  Where it exceeds T_REL |t|, fp32 does not resolve t
to the margin the caster itself grants, and the root is uncertain: short rays off a nearby transformed surface, and rays that
graze one.

Clipper list of surface i at the world hit h = org + t dir, elements in order, keep = true at the start:
  simd == QR_NULL           an accumulator marker: enter (data <= 0) saves keep and sets keep = (c_def != 0); leave (data > 0)
                            sets keep = saved AND NOT keep
  a record with a negative tag (a trnode of the clip list: the engine caches its transform for the elements up to `data`)
                            contributes nothing of its own; the clippers behind it are evaluated through their own trnode field,
                            which __init__ asserts to be that record
  a clipper k (a real surface; srf_t[2] = 1 plane, 2 quadric with scj, 3 quadric without) is evaluated at p = loc_k(h):
                            plane f = +-p[map_k] (sign: bit 10 of axes); quadric f = sum sci p^2 - 2 sum scj p - sci[3]
                            (kind 3 leaves the scj term out); keep AND= (f >= 0) if data < 0, else (f <= 0)
So keep = AND(plain elements) AND, for every accumulator group, NOT (c_def AND AND(the group's elements)).
  Margins.  h carries the root's position margin e = POS_MARGIN + T_REL |t| |dir| + the grazing slack, sigma_max(M_k) e in k's
  space; f moves by at most |grad f(p)| e_k + max |sci| e_k^2 (f is quadratic: its second-order term, which matters only where
  grad f vanishes, at a clipping cone's apex).  Within that, the clipper's decision is uncertain, and the program runs in
  three-valued logic (AND, NOT over true / false / uncertain).  An uncertain result makes the root UNCERTAIN, false rejects it,
  true keeps it as the interval, min/max, apex and noise rules left it.  A root within APEX of its surface's singular set stays
  uncertain, as in the parent.

Hit point and normal.  pos = org + t dir.  nrm = +- normalise(M^T g_loc), g_loc the local gradient (planes: sgn e_k), facing by
the record's side bit (include/qrhip.h: "through the transposed matrix of the surface's transform node").  M in place of M^T is
the teeth test's deliberate error (transpose_normal=False).

cast() returns, beside the parent's keys, for k == 1:
  cliprej        bool [N]  a root of the ray in front of its answer (any root where it misses) was ACCEPTED by interval and
                           min/max with their margins and rejected by the clipper program alone, for certain
  cliprej_group  bool [N]  ... and an accumulator group's term was false for certain there
"""
import numpy as np

import _f64cast as F
import _rayq

REJECTED, ACCEPTED, UNCERTAIN = F.REJECTED, F.ACCEPTED, F.UNCERTAIN
NOISE_X = 4.0


def elements(blob):
    """qr_elem records as an [n_elm, 4] int32 array: simd, data, next, kind"""
    h = _rayq._hdr(blob)
    return np.frombuffer(blob, dtype=np.int32, count=h[7] * 4, offset=h[14]).reshape(h[7], 4).copy()


def clip_list(blob, srf):
    """[(element index, simd, data)] of surface srf's clipper list"""
    s, _ = _rayq.surfaces(blob)
    e = elements(blob)
    out, c = [], int(s[srf, 38])
    while c != -1:
        assert len(out) < len(e), "a clipper list that does not end"
        out.append((c, int(e[c, 0]), int(e[c, 1])))
        c = int(e[c, 2])
    return out


class XDomain(F.Domain):
    """the real surfaces of a snapshot with their transforms and clipper programs; transpose_normal=False is a teeth test's
    deliberate error"""

    def __init__(self, blob, closed=False, flip_side=False, transpose_normal=True):
        s, f = _rayq.surfaces(blob)
        real = _rayq.real_surfaces(blob)
        n = len(real)
        assert n > 0
        maps = np.stack([(s[real, 23] >> (2 * a)) & 3 for a in range(3)], axis=1)
        assert (np.sort(maps, axis=1) == (0, 1, 2)).all(), "a malformed axis map: outside the caster's domain"
        tag = s[real, 37]
        self.index = real.astype(np.int64)
        self.all_conic, self.all_tag = s[:, 11] != 0, s[:, 37].copy()
        self.all_axes, self.all_minmax = s[:, 23].copy(), s[:, 7] & 63
        self.tag = tag
        self.plane = tag == 0
        assert ((s[real, 34] == 1) == self.plane).all() and np.isin(s[real, 34], (1, 2, 3)).all(), "a solver that does not fit the tag"
        self.conic = s[real, 11] != 0
        self.pos = f[real, 0:3].astype(np.float64)
        self.mn = f[real, 4:7].astype(np.float64)
        self.mx = f[real, 8:11].astype(np.float64)
        mm = s[real, 7]
        self.has_mn = np.stack([(mm >> a) & 1 for a in range(3)], axis=1).astype(bool)
        self.has_mx = np.stack([(mm >> (3 + a)) & 1 for a in range(3)], axis=1).astype(bool)
        assert not (self.has_mn & (self.mn > F.OPEN)).any() and not (self.has_mx & (self.mx < -F.OPEN)).any(), "a clip bound that clips everything"
        self.has_mn &= self.mn >= -F.OPEN
        self.has_mx &= self.mx <= F.OPEN
        self.sci = f[real, 24:28].astype(np.float64)
        self.scj = f[real, 28:31].astype(np.float64)
        self.pk = maps[:, 2].astype(np.int64)
        self.psgn = np.where((s[real, 23] >> 10) & 1, -1.0, 1.0)
        sci3 = self.sci[:, 0:3]
        with np.errstate(all="ignore"):
            self.sing = np.where(sci3 != 0, self.scj / sci3, 0.0)
        self.sing_axes = sci3 != 0
        self.has_sing = ~((sci3 == 0) & (self.scj != 0)).any(axis=1)
        self.casts = _rayq.casts(blob)[real]
        self.closed, self.flip_side, self.transpose_normal = closed, flip_side, transpose_normal

        # -- world to local: loc(x) = M (x - P) - Q
        ht, tr = s[real, 15], s[real, 39]
        assert ((s[real, 19] != 0) == (ht != 0)).all(), "shift is not set exactly where has_trm is"
        assert (tr[ht == 0] == -1).all(), "an untransformed surface that names a trnode"
        self.xf = ht != 0
        self.own = self.xf & (tr == real)
        self.under = self.xf & ~self.own
        self.tnode = np.where(self.xf, tr, -1).astype(np.int64)    # by real surface: the record the matrix is read from
        self.M = np.tile(np.eye(3), (n, 1, 1))
        self.P, self.Q = self.pos.copy(), np.zeros((n, 3))
        for j in np.nonzero(self.xf)[0]:
            T = int(tr[j])
            assert 0 <= T < len(s) and s[T, 15] != 0 and s[T, 39] == T, "a transform node under another one, or without a matrix"
            assert self.own[j] or s[T, 37] < 0, "a surface under another surface's transform"
            m = np.stack([f[T, 12:15], f[T, 16:19], f[T, 20:23]]).astype(np.float64)
            self.M[j] = np.diag(np.diag(m)) if s[T, 15] == 1 else m
            self.P[j] = f[T, 0:3].astype(np.float64)
            if not self.own[j]:
                self.Q[j] = self.pos[j]
        sv = np.linalg.svd(self.M, compute_uv=False)
        self.smax, self.smin = sv[:, 0].copy(), sv[:, 2].copy()
        assert (self.smin > 1e-6 * self.smax).all(), "a singular transform"
        self.smax[~self.xf] = self.smin[~self.xf] = 1.0
        self.Minv = np.linalg.inv(self.M)
        self.pure_rot = np.zeros(n, dtype=bool)
        self.pure_rot[self.xf] = s[tr[self.xf], 15] == 2                        # has_trm == 2: the engine does not renormalise
        self.xcols = np.nonzero(self.xf)[0]
        # the normal bound's factor (tests/test_f64_fixtures.py derives it): max |sci| sigma_max^2 / sigma_min; a transformed
        # plane's gradient does not move with the hit point
        base = np.where(self.plane, np.where(self.xf, 0.0, 1.0), np.abs(sci3).max(axis=1))
        self.turn = base * self.smax * self.smax / self.smin

        # -- clipper programs
        where = np.full(len(s), -1, dtype=np.int64)
        where[real] = np.arange(n)
        self.ckind = s[real, 36]
        self.prog = {}
        self.has_clip = s[real, 38] != -1
        self.has_group = np.zeros(n, dtype=bool)
        for j in np.nonzero(self.has_clip)[0]:
            ops, inside, group_tr = [], False, -1
            for _, k, data in clip_list(blob, int(real[j])):
                if k == -1:
                    if data <= 0:
                        assert not inside, "an accumulator group inside another"
                        ops.append(("enter", bool(s[real[j], 3] != 0)))
                    else:
                        assert inside, "an accumulator group left that was never entered"
                        ops.append(("leave",))
                        self.has_group[j] = True
                    inside = data <= 0
                elif s[k, 37] < 0:
                    assert s[k, 15] != 0 and s[k, 39] == k, "a clip list's trnode without a transform of its own"
                    group_tr = k
                else:
                    kj = int(where[k])
                    assert kj >= 0 and self.ckind[kj] in (1, 2, 3), "a clipper that is no real surface, or has no clip kind"
                    assert (self.ckind[kj] == 1) == bool(self.plane[kj]), "a clip kind that does not fit the tag"
                    assert not self.under[kj] or self.tnode[kj] == group_tr, "a clipper under a trnode its clip list does not name"
                    ops.append(("clip", kj, data < 0))
            assert not inside, "an accumulator group that is never left"
            self.prog[int(j)] = ops

    # -- local coordinates of pairs (ray ri, surface si) -----------------------------------------------------------------------
    def _local(self, ri, si, o, d):
        """(loc_si(o[ri]), M_si d[ri]); an untransformed surface's by the parent's own expressions"""
        plain_o, plain_d = o[ri] - self.pos[si], d[ri]
        x = self.xf[si]
        if not x.any():
            return plain_o, plain_d
        M = self.M[si]
        lo = np.einsum("mab,mb->ma", M, o[ri] - self.P[si]) - self.Q[si]
        ld = np.einsum("mab,mb->ma", M, d[ri])
        return np.where(x[:, None], lo, plain_o), np.where(x[:, None], ld, plain_d)

    # -- roots ----------------------------------------------------------------------------------------------------------------
    def _roots(self, rays, m):
        o = rays[:, 0:3].astype(np.float64)
        d = rays[:, 4:7].astype(np.float64)
        tmin = rays[:, 3].astype(np.float64)[:, None]
        tmax = np.minimum(rays[:, 7].astype(np.float64), F.FLT_MAX)[:, None]
        dl = np.sqrt((d * d).sum(axis=1))[:, None]
        sci = self.sci[:, 0:3]
        w = sci * self.pos + self.scj
        k0 = (self.pos * (sci * self.pos + 2.0 * self.scj)).sum(axis=1) - self.sci[:, 3]
        with np.errstate(all="ignore"):
            dot = lambda x, y: np.einsum("na,sa->ns", x, y)
            # untransformed surfaces: the parent's expansion in org and pos, the same operations in the same order
            A = dot(d * d, sci)
            B = dot(d * o, sci) - dot(d, w)
            C = dot(o * o, sci) - 2.0 * dot(o, w) + k0[None]
            X = self.xcols
            if len(X):
                # transformed surfaces: F along the local ray lo + t ld.  |lo| is a scene's size times sigma_max, so float64
                # leaves C about 1e-13 of that squared: five digits below the margins, as in the parent
                lo = np.einsum("sab,nsb->nsa", self.M[X], o[:, None, :] - self.P[X][None]) - self.Q[X][None]
                ld = np.einsum("sab,nb->nsa", self.M[X], d)
                g = sci[X][None] * lo - self.scj[X][None]
                A[:, X] = (sci[X][None] * ld * ld).sum(axis=2)
                B[:, X] = (ld * g).sum(axis=2)
                C[:, X] = (lo * (g - self.scj[X][None])).sum(axis=2) - self.sci[X, 3][None]
            disc = B * B - A * C
            scale = B * B + np.abs(A * C)
            pr, ps = np.nonzero(self.plane[None] | (disc > -m.graze * scale))
            A, B, C, disc, scale = A[pr, ps], B[pr, ps], C[pr, ps], disc[pr, ps], scale[pr, ps]
            plane = self.plane[ps]
            graze = (np.abs(disc) < m.graze * scale) & ~plane
            q = -(B + np.where(B >= 0, 1.0, -1.0) * np.sqrt(np.maximum(disc, 0.0)))
            none = (disc < 0) | graze
            r1 = np.where(none | (A == 0), np.nan, q / A)
            r2 = np.where(none | (q == 0), np.nan, C / q)
            pk = self.pk[ps]
            ol, od = self._local(pr, ps, o, d)
            at = np.arange(len(pr))
            tp = -ol[at, pk] / od[at, pk]                           # planes: loc[map_k] = 0
            r1 = np.where(plane, tp, r1)
            r2 = np.where(plane, np.nan, r2)
            mid = np.where(graze & (A != 0), -B / A, np.nan)
            slack = np.sqrt(2.0 * m.graze) * np.abs(mid)
        out = [self._classify_x(pr, ps, t, slk, ol, od, o, d, dl, A, B, tmin, tmax, m) for t, slk in ((r1, None), (r2, None), (mid, slack))]
        return [np.concatenate([x[j] for x in out]) for j in range(6)]

    def _classify_x(self, pr, ps, t, slack, ol, od, o, d, dl, A, B, tmin, tmax, m):
        """the parent's _classify in local coordinates, then the clipper program"""
        with np.errstate(all="ignore"):
            lo_b, hi_b, dn = tmin[pr, 0], tmax[pr, 0], dl[pr, 0]
            sl = np.zeros(len(pr)) if slack is None else slack
            inside = ((t >= lo_b) & (t <= hi_b)) if self.closed else ((t > lo_b) & (t < hi_b))
            near = ((np.abs(t - lo_b) < m.t_rel * np.abs(lo_b) + m.pos / dn + sl) |
                    (np.abs(t - hi_b) < m.t_rel * np.abs(hi_b) + m.pos / dn + sl))
            have = np.isfinite(t) & (inside | near)
            ri, si, A, B, t0, sl, dn, near = pr[have], ps[have], A[have], B[have], t[have], sl[have], dn[have], near[have]
            dd = od[have]
            loc = ol[have] + t0[:, None] * dd
            mw = m.pos + m.t_rel * np.abs(t0) * dn + sl * dn         # the root's position margin, world
            mp = (mw * self.smax[si])[:, None]                       # ... and in the surface's space
            hm, hx, mn, mx = self.has_mn[si], self.has_mx[si], self.mn[si], self.mx[si]
            edge = ((hm & (np.abs(loc - mn) < mp)) | (hx & (np.abs(loc - mx) < mp))).any(axis=1)
            clip_rej = ((hm & (loc < mn)) | (hx & (loc > mx))).any(axis=1) & ~edge
            off = np.where(self.sing_axes[si], loc - self.sing[si], 0.0)
            apex = self.conic[si] & self.has_sing[si] & ((off * off).sum(axis=1) < m.apex * m.apex)
            sci, scj = self.sci[si], self.scj[si]
            terms = (np.abs(sci[:, 0:3]) * loc * loc).sum(axis=1) + 2.0 * np.abs(scj * loc).sum(axis=1) + np.abs(sci[:, 3])
            blur = ~self.plane[si] & (m.noise * 2.0 ** -24 * terms > m.t_rel * np.abs(t0) * 2.0 * np.abs(A * t0 + B))
            # fp32's own noise in the local origin and direction of a transformed surface (the module's text, "Transform noise")
            x = self.xf[si]
            eps = NOISE_X * 2.0 ** -24 * (self.smax[si] * np.linalg.norm(o[ri] - self.P[si], axis=1) + np.linalg.norm(self.Q[si], axis=1)
                                          + np.abs(t0) * self.smax[si] * dn)
            at = np.arange(len(si))
            gn = np.where(self.plane[si], 1.0, 2.0 * np.linalg.norm(sci[:, 0:3] * loc - scj, axis=1))
            along = np.where(self.plane[si], np.abs(dd[at, self.pk[si]]), 2.0 * np.abs(A * t0 + B))
            blur |= x & (gn * eps > m.t_rel * np.abs(t0) * along)
            st = np.full(len(ri), ACCEPTED, dtype=np.int8)
            st[near | edge | apex | blur] = UNCERTAIN
            if slack is not None:
                st[:] = UNCERTAIN
            st[clip_rej & ~apex] = REJECTED
            # the clipper program, at the world hit
            todo = np.nonzero((st != REJECTED) & self.has_clip[si])[0]
            if not len(todo):
                self._log.append((ri[:0], t0[:0], np.zeros(0, dtype=bool)))     # one entry a call: cast() counts them
            else:
                h = o[ri[todo]] + t0[todo, None] * d[ri[todo]]
                ct, cf, gf = self._clip(si[todo], h, mw[todo])
                no, maybe = cf & ~ct, cf & ct
                lone = no & (st[todo] == ACCEPTED)                   # rejected by the clipper program alone
                self._log.append((ri[todo][lone], t0[todo][lone], gf[lone]))
                st[todo[maybe]] = UNCERTAIN
                st[todo[no & ~apex[todo]]] = REJECTED
                st[todo[no & apex[todo]]] = UNCERTAIN
            sd = np.where(self.plane[si], self.psgn[si] * dd[np.arange(len(si)), self.pk[si]] > 0, (A * t0 + B) > 0)
            if self.flip_side:
                sd = ~sd
        keep = st != REJECTED
        return ri[keep], si[keep], st[keep], t0[keep], (t0 - sl)[keep], sd[keep]

    def _clip(self, si, h, mw):
        """the clipper programs of surfaces si at world points h with world position margins mw, in three-valued logic:
        (may be true, may be false, an accumulator group's term is false for certain)"""
        n = len(si)
        ct, cf, gf = np.ones(n, dtype=bool), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        for j in np.unique(si):
            sel = np.nonzero(si == j)[0]
            ct[sel], cf[sel], gf[sel] = self._run(self.prog[int(j)], h[sel], mw[sel])
        return ct, cf, gf

    def _run(self, prog, h, mw):
        n = len(h)
        kt, kf, gf = np.ones(n, dtype=bool), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        saved = None
        for op in prog:
            if op[0] == "enter":
                saved = (kt, kf)
                kt, kf = np.full(n, op[1]), np.full(n, not op[1])
            elif op[0] == "leave":
                nt, nf = kf, kt                                     # NOT keep
                gf = gf | (nf & ~nt)
                kt, kf = saved[0] & nt, saved[1] | nf
            else:
                k, keep_ge = op[1], op[2]
                p = (h - self.P[k]) @ self.M[k].T - self.Q[k]
                e = mw * self.smax[k]
                if self.plane[k]:
                    fv, tol = self.psgn[k] * p[:, self.pk[k]], e
                else:
                    sci, scj = self.sci[k, 0:3], (self.scj[k] if self.ckind[k] == 2 else np.zeros(3))
                    fv = (sci * p * p - 2.0 * scj * p).sum(axis=1) - self.sci[k, 3]
                    tol = 2.0 * np.linalg.norm(sci * p - scj, axis=1) * e + np.abs(sci).max() * e * e
                ok = (fv >= 0) if keep_ge else (fv <= 0)
                unc = np.abs(fv) <= tol
                kt, kf = kt & (ok | unc), kf | (~ok | unc)
        return kt, kf, gf

    # -- queries ----------------------------------------------------------------------------------------------------------------
    def cast(self, rays, k=1, margins=None, chunk=1024):
        """the parent's cast; for k == 1 with the keys cliprej and cliprej_group (the module's text) beside the parent's"""
        m = margins or F.Margins()
        self._log = []
        res = super().cast(rays, k, m, chunk)
        log, self._log = self._log, []
        if k != 1:
            return res
        # the parent asks for the roots chunk by chunk, three calls of _classify_x a chunk: ray numbers are the chunk's own
        n = len(res["count"])
        res["cliprej"], res["cliprej_group"] = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        r64 = np.ascontiguousarray(rays, dtype=np.float32)
        pos_t = m.pos / np.linalg.norm(r64[:, 4:7].astype(np.float64), axis=1)
        for c, (ri, t0, gf) in enumerate(log):
            ri = ri + (c // 3) * chunk
            ans = res["t"][0][ri]
            front = t0 + m.t_rel * np.abs(t0) + pos_t[ri] < ans      # inf where the ray misses
            res["cliprej"][ri[front]] = True
            res["cliprej_group"][ri[front & gf]] = True
        return res

    def hit_point_x(self, rays, hit_id, t):
        """(pos f64 [N, 3], unit normal f64 [N, 3] facing by the id's side bit, |g_loc| [N], the normal bound's factor turn [N],
        sigma_max / sigma_min [N], the surface is an untransformed plane [N]) of hits (id >= 0) at float64 t"""
        where = np.full(len(self.all_tag), -1, dtype=np.int64)
        where[self.index] = np.arange(len(self.index))
        j = where[np.asarray(hit_id, dtype=np.int64) >> 1]
        assert (j >= 0).all(), "a hit on something that is no real surface"
        o = rays[:, 0:3].astype(np.float64)
        d = rays[:, 4:7].astype(np.float64)
        p = o + t[:, None] * d
        ol, od = self._local(np.arange(len(j)), j, o, d)
        loc = np.where(self.xf[j][:, None], ol + t[:, None] * od, p - self.pos[j])        # untransformed: the parent's expression
        g = 2.0 * (self.sci[j, 0:3] * loc - self.scj[j])
        pl = np.nonzero(self.plane[j])[0]
        g[pl] = 0.0
        g[pl, self.pk[j[pl]]] = self.psgn[j[pl]]
        gl = np.linalg.norm(g, axis=1)
        gw = np.einsum("mba,mb->ma" if self.transpose_normal else "mab,mb->ma", self.M[j], g)
        gw = np.where(self.xf[j][:, None], gw, g)
        sign = np.where((np.asarray(hit_id) & 1) == 1, -1.0, 1.0)
        with np.errstate(all="ignore"):
            nw = gw / np.linalg.norm(gw, axis=1)[:, None] * sign[:, None]
        return p, nw, gl, self.turn[j], self.smax[j] / self.smin[j], self.plane[j] & ~self.xf[j]

    def hit_point(self, rays, hit_id, t):
        return self.hit_point_x(rays, hit_id, t)[:4]
