/*
 * qr_builder.cpp - the programs of the device image (qr_program.h): surface lists, clipper lists, light lists with their
 * shadow lists and grids.
 *
 * What the list compiler resolves statically is the reference's per-ray walk state that depends only on the
 * list position: `ctx_LOCAL(OBJ)` (tracer.cpp:1385-1417: are we inside a trnode whose transform is cached?),
 * the end of bounding-volume arrays (AR_skp 3955-4054), and, for clipper lists, the same caching of the clipper
 * trnode (1931-2151).
 */
#include "qr_list_filter.hpp"

namespace qrc {

/* a side that casts no shadow (CHECK_SHAD, tracer.cpp:549-589): a light's own body, plain transparency */
static bool no_shadow(int p) { return (p & QR_PROP_LIGHT) || ((p & QR_PROP_TRANSP) && !(p & QR_PROP_REFRACT)); }

/* ---- surface lists ---- */

void Builder::dedup_add(uint64_t key, uint32_t off, uint8_t heavy)
{
    if ((dedup_ent.size() + 1) * 2 > dedup_slot.size())
    {
        dedup_slot.assign(dedup_slot.size() * 4, -1);
        for (size_t i = 0; i < dedup_ent.size(); i++)
        {
            int32_t &sl = dedup_slot[(size_t)(dedup_ent[i].key >> 20) & (dedup_slot.size() - 1)];
            dedup_ent[i].next = sl; sl = (int32_t)i;
        }
    }
    int32_t &sl = dedup_slot[(size_t)(key >> 20) & (dedup_slot.size() - 1)];
    dedup_ent.push_back(DedupEnt{ dedup_pool.size(), dk.size(), key, off, heavy, sl });
    sl = dedup_last = (int32_t)dedup_ent.size() - 1;
    dedup_pool.insert(dedup_pool.end(), dk.begin(), dk.end());
}

/*
 * as_shadow: the program is only ever walked by shadow rays (CLight::shadow).  A hit on a solver cell that casts no shadow
 * (QR_OPF_NOSHAD) changes nothing in such a walk -- it occludes nobody, and a shadow walk keeps no depth -- so the cell is left
 * out the way a marker element is: array ends and trnode ranges stay what they were.  Every shadow ray of the demo scenes aims at
 * such a cell, the light's own body, which no cull removes: more than half of their shadow walks' solves
 * (profiles/r25_own_surface_roots.txt).  A chain that is also a tile or side list keeps its full program beside this one;
 * one without such a surface has a single program for both.
 */
uint32_t Builder::compile_list(int head, bool as_shadow)
{
    if (head == QR_NULL) return 0;
    if (E.size() + 1 > list_off.size())
    {
        /* chains appended by the shadow grids */
        const size_t n1 = E.size() + 1;
        list_off.resize(n1, 0); light_off.resize(n1, 0); list_heavy.resize(n1, 0); shadow_off.resize(n1, 0);
        chain_pos.resize(n1, 0); chain_stamp.resize(n1, -1);
    }
    /* memo and dedup */
    uint32_t &memo_off = as_shadow ? shadow_off[head] : list_off[head];
    if (memo_off) return memo_off;
    bool shadowless = false;
    const int n = chain_begin(head, as_shadow, shadowless);
    if (as_shadow && !shadowless) return shadow_off[head] = compile_list(head);
    if (box_ok && n >= QR_LONG_CELLS) throw Restart{};
    uint64_t dkey;
    const bool dedup = dedup_key(head, as_shadow, dkey);
    if (dedup)
        if (const DedupEnt *d = dedup_find(dkey)) { list_heavy[head] = d->heavy; return memo_off = d->off; }
    /* classify, check, bound */
    ch.clear();
    for (int e = head; e != QR_NULL; e = E[e].next) ch.push_back(Tmp{e, 0, E[e].simd, QR_NULL, true});
    classify(n, as_shadow);
    check_nesting(n);
    array_spheres(n);
    const ListProps lp = list_props(n);
    /* lay out: slot index of every cell: a bounding-volume cell takes two slots (its extension carries the volume) */
    emit_idx.assign((size_t)n + 1, 0);
    int ne = 0;
    for (int i = 0; i < n; i++) { emit_idx[i] = ne; if (ch[i].emit) ne += (ch[i].op & QR_OPT_BV) ? 2 : 1; }
    emit_idx[n] = ne;
    /* uniform grid (CDda) for long world-space lists without clipper programs: decided before the cells are placed,
     * the record sits in the 64 bytes in front of the program.  Not for a program of shadow rays alone (as_shadow here: the
     * one with cells left out): only nearest-hit rays walk a grid (qr_walk.hpp traverse, !SHADOW) */
    const bool want_dda = !as_shadow && wants_dda(n, lp);
    /* Lists the per-lane walk with hand-over may take (world-space cells only, no clipper program) carry their LENGTH in the
     * word in front of the program -- in a cell of their own, or in the grid record's spare word: (bytes of cells in front of
     * the END cell) | 1 when no cell is a bounding volume (every multiple of 32 bytes is then a cell boundary).  walk_pool
     * cuts such a flat list in halves for idle lanes (qr_walk.hpp); a list program ends with an END cell, so without this
     * word a lane knows where its range ends only when it gets there. */
    const bool want_len = lp.world && lp.div;
    const size_t front = want_dda ? sizeof(CDda) : (want_len ? sizeof(CCell) : 0);
    const uint32_t base = alloc((size_t)(ne + 1) * sizeof(CCell) + front, 64);
    const uint32_t off = base + (uint32_t)front;
    if (want_len) *at<uint32_t>(off - 4u) = (uint32_t)ne * (uint32_t)sizeof(CCell) | (lp.n_bv == 0 ? 1u : 0u);
    emit_cells(n, off, lp.has_trnode);      /* END cell: already zero */
    st.n_lists++; st.n_cells += (uint32_t)lp.n_emitted; st.n_dropped += (uint32_t)(n - lp.n_emitted);
    /* flags in the offset's low bits: may the per-lane walk take this list, is it a long hierarchy */
    uint32_t lf = (lp.div ? QR_LISTF_DIV : 0u) | (lp.world ? QR_LISTF_WORLD : 0u);
    /* a long hierarchy: rays part ways on it.  (96 cells until round 3: demo scene 2's ~110-cell lists then put its frames on
     * the per-lane kernel instance, which renders them at 3 waves per SIMD -- 34.8 against 46.5 Grays/s with this one.) */
    if (lp.n_emitted >= QR_LONG_CELLS && lp.n_bv >= 4) { lf |= QR_LISTF_LONG; any_long = true; }
    if (want_dda) { build_dda(base, off, n); lf |= QR_LISTF_DDA; any_long = true; }
    memo_off = off | lf;
    list_heavy[head] = lp.heavy;
    if (dedup) dedup_add(dkey, off | lf, lp.heavy);
    return off | lf;
}

/* numbers the chain's elements (chain_pos, under a fresh stamp); returns its length.  shadowless: a shadow program of this
 * chain would leave a cell out */
int Builder::chain_begin(int head, bool as_shadow, bool &shadowless)
{
    stamp++;
    int n = 0;
    for (int e = head; e != QR_NULL; e = E[e].next)
    {
        if ((size_t)n >= E.size()) throw Fail{QR_ERR_ARG, "cyclic list"};
        chain_stamp[e] = stamp; chain_pos[e] = n++;
        if (as_shadow && kn.drop_shadowless)
        {
            const qr_surface &q = v.srf[E[e].simd];
            if (is_real(q) && no_shadow(q.props[0]) && no_shadow(q.props[1])) shadowless = true;
        }
    }
    return n;
}

/*
 * The engine hands every screen tile a chain of its own, and most neighbours hold the same surfaces in the same order:
 * a chain whose elements (surface, kind, position of the array's last member) equal those of a chain compiled
 * before IS that program -- the cells depend on nothing else.  One copy: a third of the compile time at 1080p, and
 * the waves of a frame read a few hundred list programs through the scalar cache instead of tens of thousands.
 * The chain's content goes to `dk`, its hash to `key`; false: no dedup for this chain.
 */
bool Builder::dedup_key(int head, bool as_shadow, uint64_t &key)
{
    key = 1469598103934665603ull;
    if (!kn.dedup) return false;
    dk.clear();
    if (as_shadow) { dk.push_back(-2); key = (key ^ 0xFFFFFFFEu) * 1099511628211ull; }       /* a key no full program has: theirs hold triples */
    for (int e = head; e != QR_NULL; e = E[e].next)
    {
        const qr_elem &el = E[e];
        int rel = -1;
        if (el.data != QR_NULL)
        {
            if (el.data < 0 || (size_t)el.data >= chain_stamp.size() || chain_stamp[el.data] != stamp) return false;
            rel = chain_pos[el.data];
        }
        const int32_t w3[3] = { el.simd, el.kind, rel };
        for (int k = 0; k < 3; k++) { dk.push_back(w3[k]); key = (key ^ (uint32_t)w3[k]) * 1099511628211ull; }
    }
    return true;
}

const Builder::DedupEnt *Builder::dedup_find(uint64_t key)
{
    int32_t hit = -1;
    if (dedup_last >= 0 && dedup_equal(dedup_ent[(size_t)dedup_last], key)) hit = dedup_last;
    else
        for (int32_t i = dedup_slot[(size_t)(key >> 20) & (dedup_slot.size() - 1)]; i >= 0; i = dedup_ent[(size_t)i].next)
            if (dedup_equal(dedup_ent[(size_t)i], key)) { hit = i; break; }
    if (hit < 0) return nullptr;
    dedup_last = hit;
    return &dedup_ent[(size_t)hit];
}

/* every element's op word (type, transform mode, axes, shadow and cull flags) and, for array elements, the position of the
 * last member; lo_self / lo_after: the cached trnode's last element at / behind every position */
void Builder::classify(int n, bool as_shadow)
{
    lo_after.assign((size_t)n, QR_NULL); lo_self.assign((size_t)n, QR_NULL);
    int local_obj = QR_NULL;
    for (int i = 0; i < n; i++)
    {
        Tmp &t = ch[i];
        const qr_elem &el = E[t.e];
        const qr_surface &s = v.srf[el.simd];
        const bool arr = s.srf_t[3] < 0, real = is_real(s);
        const bool bv = (el.kind & 3) == 1;
        uint32_t mode, type;
        bool trnode_cell = false;
        if (!arr && local_obj != QR_NULL)
        {
            mode = QR_OPF_CACHED;
            if (t.e == local_obj) local_obj = QR_NULL;
        }
        else if (s.has_trm == 0) mode = 0;
        else if (arr) { mode = 0; trnode_cell = true; local_obj = el.data; }
        else mode = QR_OPF_OWN;
        lo_self[i] = local_obj;
        const int solver = real ? s.srf_t[0] : 0;
        if (trnode_cell)
        {
            if (bv) throw Fail{QR_ERR_UNSUP, "bounding volume on a transformed array element"};
            if (el.data == QR_NULL || chain_stamp[el.data] != stamp || chain_pos[el.data] < i)
                throw Fail{QR_ERR_ARG, "trnode's last element is not behind it in its list"};
            type = QR_OPT_TRNODE; t.last = chain_pos[el.data];
        }
        else if (bv)
        {
            if (el.data == QR_NULL || chain_stamp[el.data] != stamp || chain_pos[el.data] < i)
                throw Fail{QR_ERR_ARG, "array's last element is not behind it in its list"};
            type = QR_OPT_BV; t.last = chain_pos[el.data];
        }
        else if (solver == 1) type = QR_OPT_PLANE;
        else if (solver == 2) type = QR_OPT_QUADRIC;
        else if (solver == 3) type = QR_OPT_TWOPLANE;
        else { type = 0; t.emit = false; }          /* marker: touches only state nobody reads */
        if (t.emit && type != QR_OPT_TRNODE && ((s.shift != 0) != (mode != 0)))
            throw Fail{QR_ERR_UNSUP, "surface reads the trnode-space diff outside a trnode (or the reverse)"};
        uint32_t op = type | mode;
        if (s.has_trm != 1) op |= QR_OPF_FULLM;
        if (type & QR_OPT_SOLVER)
        {
            const uint32_t ak = (s.axes >> 4) & 3u, ai = (s.axes >> 0) & 3u;
            if (ak == 0) op |= QR_OPF_KX; else if (ak == 1) op |= QR_OPF_KY;
            if ((s.axes >> 10) & 1u) op |= QR_OPF_SGNK;
            if (ai == 0) op |= QR_OPF_IX; else if (ai == 1) op |= QR_OPF_IY;
            const bool n0 = no_shadow(s.props[0]), n1 = no_shadow(s.props[1]);
            if (n0 && n1) op |= QR_OPF_NOSHAD; else if (n0 || n1) op |= QR_OPF_SIDESHAD;
            if (s.clip != QR_NULL) op |= QR_OPF_CLIP;
            if (s.conic != 0) op |= QR_OPF_CONIC;
            const bool open_shape = s.srf_t[0] == 1 || !(s.sci[0] > 0.0f && s.sci[1] > 0.0f && s.sci[2] > 0.0f);
            const bool want = kn.cull >= 3 || (kn.cull == 2 && open_shape) || (kn.cull == 1 && s.srf_t[0] == 1);
            if (want && bs[el.simd].r < 1e18f)
            {
                op |= QR_OPF_CULL;
                /* box or sphere: whichever shows the smaller silhouette on average (a convex body's mean projected area
                 * is a quarter of its surface).  Box cull cells (QR_OPF_BOX) only in images whose lists are all short: the
                 * packet-walk kernel instance serves them */
                const BSphere &bb = bs[el.simd];
                if (box_ok && bb.lo[0] <= bb.hi[0])
                {
                    const double a = (double)bb.hi[0] - bb.lo[0], b = (double)bb.hi[1] - bb.lo[1], c = (double)bb.hi[2] - bb.lo[2];
                    if (0.5 * (a * b + b * c + c * a) < 0.8 * 3.14159265358979 * (double)bb.r * bb.r) { op |= QR_OPF_BOX; any_box = true; }
                }
            }
        }
        t.op = op;
        if (as_shadow && (op & QR_OPF_NOSHAD)) t.emit = false;
        lo_after[i] = local_obj;
    }
}

/* static state must not depend on whether a ray walked through an array or skipped it (AR_skp:
 * e = last; if (e == local_obj) local_obj = NULL), and arrays must nest */
void Builder::check_nesting(int n)
{
    std::vector<int> &open = open_arr;
    open.clear();
    for (int i = 0; i < n; i++)
    {
        while (!open.empty() && open.back() < i) open.pop_back();
        if (!(ch[i].op & QR_OPT_BV) || !ch[i].emit) continue;
        const int j = ch[i].last;
        int lo = lo_self[i];
        if (lo == ch[j].e) lo = QR_NULL;
        if (lo != lo_after[j]) throw Fail{QR_ERR_UNSUP, "a trnode's range crosses the end of a bounding-volume array"};
        if (!open.empty() && j > open.back()) throw Fail{QR_ERR_UNSUP, "bounding-volume arrays are not nested"};
        open.push_back(j);
    }
}

/* bounding-volume arrays get a conservative sphere of their own (ours): the union of the members' bounding
 * spheres around the first bounded member's centre.  The walk skips an array that lies entirely behind a
 * ray's origin or entirely beyond its current depth bound -- the reference's own test only asks whether the
 * LINE meets the volume.  No sphere (no cull) when a member is unbounded. */
void Builder::array_spheres(int n)
{
    arr_sphere.resize((size_t)n);
    if (kn.cull < 3) return;
    auto member = [&](int k) { return ch[k].emit && (ch[k].op & QR_OPT_SOLVER) ? &bs[ch[k].si] : nullptr; };
    for (int i = 0; i < n; i++)
    {
        if (!(ch[i].op & QR_OPT_BV) || !ch[i].emit) continue;
        const BSphere *c0; double R;
        if (!array_union(i, ch[i].last, member, c0, R)) continue;
        R = R * 1.0001 + 1e-4;
        if (!(R < 1e18)) continue;
        arr_sphere[i].c[0] = c0->c[0]; arr_sphere[i].c[1] = c0->c[1]; arr_sphere[i].c[2] = c0->c[2]; arr_sphere[i].r = (float)R * 1.0001f;
        ch[i].op |= QR_OPF_CULL;
        /* the volume itself a plain sphere around all members' bounds?  Then it is the cull sphere. */
        const qr_surface &q = v.srf[ch[i].si];
        if (!(ch[i].op & QR_OPF_LOCAL) && q.has_trm == 0 && q.sci[0] == 1.0f && q.sci[1] == 1.0f && q.sci[2] == 1.0f
            && q.sci[3] > 0.0f && q.sci[3] < 1e30f)
        {
            const double rq = __builtin_sqrt((double)q.sci[3]);
            bool inside = true;
            for (int k = i + 1; k <= ch[i].last && inside; k++)
                if (const BSphere *m = member(k))
                {
                    const double dx = (double)m->c[0] - q.pos[0], dy = (double)m->c[1] - q.pos[1], dz = (double)m->c[2] - q.pos[2];
                    if (__builtin_sqrt(dx * dx + dy * dy + dz * dz) + (double)m->r > rq * 1.0001) inside = false;
                }
            if (inside)
            {
                arr_sphere[i].c[0] = q.pos[0]; arr_sphere[i].c[1] = q.pos[1]; arr_sphere[i].c[2] = q.pos[2];
                arr_sphere[i].r = (float)(rq * 1.0002 + 1e-4);
                ch[i].op |= QR_OPF_SPHBV;
            }
        }
    }
}

Builder::ListProps Builder::list_props(int n) const
{
    ListProps lp;
    for (int i = 0; i < n; i++)
    {
        const qr_surface &q = v.srf[ch[i].si];
        if (is_real(q))
            for (int k = 0; k < 2; k++)
            {
                if (q.props[k] & QR_PROP_REFLECT) lp.heavy |= 1;
                if (!(q.props[k] & QR_PROP_OPAQUE)) lp.heavy |= 2;
            }
        if (!ch[i].emit) continue;
        const uint32_t op = ch[i].op;
        lp.n_emitted++;
        if (op & QR_OPT_BV) lp.n_bv++;
        if (op & QR_OPF_CLIP) lp.div = false;
        if (op & (QR_OPT_TRNODE | QR_OPF_CACHED)) lp.has_trnode = true;
        if (op & (QR_OPT_TRNODE | QR_OPF_LOCAL)) lp.world = false;
    }
    return lp;
}

/* a list of world-space cells without clipper programs (what carries a length word) with enough small members */
bool Builder::wants_dda(int n, const ListProps &lp) const
{
    if (kn.dda_min <= 0 || !lp.world || !lp.div) return false;
    int n_small = 0;
    for (int i = 0; i < n; i++)
        if (ch[i].emit && (ch[i].op & QR_OPT_SOLVER) && bs[ch[i].si].r < 1e17f) n_small++;
    return n_small >= kn.dda_min;
}

void Builder::emit_cells(int n, uint32_t off, bool has_trnode)
{
    for (int i = 0; i < n; i++)
    {
        if (!ch[i].emit) continue;
        CCell c;
        memset(&c, 0, sizeof(c));
        c.op = ch[i].op; c.srf = srf_off(ch[i].si);
        if (c.op & QR_OPT_BV) c.end = off + (uint32_t)emit_idx[ch[i].last + 1] * (uint32_t)sizeof(CCell);
        c.r = __builtin_inff();
        if (!(c.op & QR_OPT_BV)) { c.r2 = __builtin_inff(); c.r2x = __builtin_inff(); }   /* no cull: no test of walk_pool's fails */
        if (c.op & QR_OPF_BOX)
        {
            /* + box_pad: the slab test's own rounding, 2e-6 of the scene's largest coordinate (qr_walk.hpp) */
            const BSphere &bb = bs[ch[i].si];
            c.r2 = bb.lo[0] - box_pad; c.r2x = bb.lo[1] - box_pad; c.cx = bb.lo[2] - box_pad;
            c.cy = bb.hi[0] + box_pad; c.cz = bb.hi[1] + box_pad; c.r = bb.hi[2] + box_pad;
        }
        else if (c.op & QR_OPF_CULL)
        {
            const BSphere &bsp = (c.op & QR_OPT_BV) ? arr_sphere[i] : bs[ch[i].si];
            c.cx = bsp.c[0]; c.cy = bsp.c[1]; c.cz = bsp.c[2]; c.r = bsp.r;
            if (!(c.op & QR_OPT_BV)) { c.r2 = bsp.r * bsp.r; c.r2x = c.r2 * 1.01f; }      /* BV: the slot holds `end` */
        }
        if (c.op & QR_OPT_BV) c.r2x = (c.op & QR_OPF_SPHBV) ? -1.0f : __builtin_inff();
        *at<CCell>(off + (uint32_t)emit_idx[i] * (uint32_t)sizeof(CCell)) = c;
        if (c.op & QR_OPT_BV)
        {
            /* extension slot: what AR_ptr reads of the volume's surface record, so that the walk needs no
             * second, dependent load for it */
            const qr_surface &q = v.srf[ch[i].si];
            CBvExt x;
            memset(&x, 0, sizeof(x));
            for (int k = 0; k < 3; k++) x.pos[k] = q.pos[k];
            for (int k = 0; k < 4; k++) x.sci[k] = q.sci[k];
            /* hand-over boundary: the child (direct member or nested array) that starts nearest to the middle of the
             * array's cells.  Only where a walk carries no trnode state and the array is worth splitting. */
            const int s0 = emit_idx[i] + 2, s1 = emit_idx[ch[i].last + 1];
            if (!has_trnode && s1 - s0 >= 12)
            {
                int best = -1;
                for (int k = i + 1; k <= ch[i].last; )
                {
                    if (ch[k].emit && emit_idx[k] > s0 && (best < 0 || abs(2 * emit_idx[k] - (s0 + s1)) < abs(2 * emit_idx[best] - (s0 + s1))))
                        best = k;
                    k = (ch[k].emit && (ch[k].op & QR_OPT_BV)) ? ch[k].last + 1 : k + 1;
                }
                if (best >= 0) x.mid = off + (uint32_t)emit_idx[best] * (uint32_t)sizeof(CCell);
            }
            *at<CBvExt>(off + (uint32_t)(emit_idx[i] + 1) * (uint32_t)sizeof(CCell)) = x;
        }
    }
}

/*
 * CDda of the list just emitted at `off` (ch / emit_idx still describe it): bins the members' bounding spheres.
 */
void Builder::build_dda(uint32_t rec_off, uint32_t off, int n)
{
    /* members: emitted solver cells; small ones span the grid */
    double lo[3] = { 1e300, 1e300, 1e300 }, hi[3] = { -1e300, -1e300, -1e300 };
    std::vector<int> mem;
    std::vector<float> rad;
    for (int i = 0; i < n; i++)
        if (ch[i].emit && (ch[i].op & QR_OPT_SOLVER)) { mem.push_back(i); if (bs[ch[i].si].r < 1e17f) rad.push_back(bs[ch[i].si].r); }
    std::vector<float> sorted = rad;
    std::sort(sorted.begin(), sorted.end());
    const double r_big = 4.0 * (double)sorted[sorted.size() / 2] + 1e-3;        /* larger than 4 median radii: tested up front */
    int n_small = 0;
    for (int i : mem)
    {
        const BSphere &b = bs[ch[i].si];
        if (!(b.r < r_big)) continue;
        n_small++;
        for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], (double)b.c[k] - b.r); hi[k] = std::max(hi[k], (double)b.c[k] + b.r); }
    }
    CDda g;
    memset(&g, 0, sizeof(g));
    double ext[3], vol = 1.0;
    for (int k = 0; k < 3; k++) { lo[k] -= 1e-3; hi[k] += 1e-3; ext[k] = hi[k] - lo[k]; vol *= ext[k]; }
    const double c0 = __builtin_cbrt(vol / ((kn.dda_cells > 0.01 ? kn.dda_cells : 2.0) * (n_small > 0 ? n_small : 1)));
    int dim[3];
    for (int k = 0; k < 3; k++)
    {
        int d = (int)(ext[k] / c0 + 0.5);
        dim[k] = d < 1 ? 1 : (d > (int)QR_GRID_MAX ? (int)QR_GRID_MAX : d);
        g.org[k] = (float)lo[k]; g.size[k] = (float)(ext[k] / dim[k]); g.inv[k] = (float)(dim[k] / ext[k]);
    }
    g.dims = (uint32_t)dim[0] | ((uint32_t)dim[1] << 8) | ((uint32_t)dim[2] << 16);
    const size_t n_cells = (size_t)dim[0] * dim[1] * dim[2];
    /* count, then fill (members in list order inside a cell) */
    auto range = [&](const BSphere &b, int k, int &a0, int &a1) {
        /* cells overlap: members are entered a thousandth of a cell beyond their sphere's box, so that a hit within
         * rounding of a cell face is found from either side */
        const double pad = 1e-3 * g.size[k] + 1e-4;
        a0 = (int)__builtin_floor(((double)b.c[k] - b.r - pad - lo[k]) * dim[k] / ext[k]);
        a1 = (int)__builtin_floor(((double)b.c[k] + b.r + pad - lo[k]) * dim[k] / ext[k]);
        a0 = a0 < 0 ? 0 : a0; a1 = a1 >= dim[k] ? dim[k] - 1 : a1;
    };
    std::vector<uint32_t> cnt(n_cells + 1, 0);
    std::vector<int> outl;
    for (int i : mem)
    {
        const BSphere &b = bs[ch[i].si];
        if (!(b.r < r_big)) { outl.push_back(i); continue; }
        int x0, x1, y0, y1, z0, z1;
        range(b, 0, x0, x1); range(b, 1, y0, y1); range(b, 2, z0, z1);
        for (int z = z0; z <= z1; z++) for (int y = y0; y <= y1; y++) for (int x = x0; x <= x1; x++)
            cnt[((size_t)z * dim[1] + y) * dim[0] + x + 1]++;
    }
    g.n_out = (uint32_t)outl.size();
    cnt[0] = g.n_out;
    for (size_t c = 1; c <= n_cells; c++) cnt[c] += cnt[c - 1];
    const uint32_t n_refs = cnt[n_cells];
    g.n_refs = n_refs;
    std::vector<CCell> refs(n_refs);
    auto ref_of = [&](int i) {
        CCell c = *at<CCell>(off + (uint32_t)emit_idx[i] * (uint32_t)sizeof(CCell));
        uint32_t pos = off + (uint32_t)emit_idx[i] * (uint32_t)sizeof(CCell);
        memcpy(&c.r2x, &pos, 4);            /* the original cell: list order decides between equal depths */
        return c;
    };
    for (size_t q = 0; q < outl.size(); q++) refs[q] = ref_of(outl[q]);
    std::vector<uint32_t> fill(cnt.begin(), cnt.end() - 1);
    for (int i : mem)
    {
        const BSphere &b = bs[ch[i].si];
        if (!(b.r < r_big)) continue;
        int x0, x1, y0, y1, z0, z1;
        range(b, 0, x0, x1); range(b, 1, y0, y1); range(b, 2, z0, z1);
        const CCell c = ref_of(i);
        for (int z = z0; z <= z1; z++) for (int y = y0; y <= y1; y++) for (int x = x0; x <= x1; x++)
            refs[fill[((size_t)z * dim[1] + y) * dim[0] + x]++] = c;
    }
    g.cells = alloc((n_cells + 1) * 4, 16);
    memcpy(at<uint32_t>(g.cells), cnt.data(), (n_cells + 1) * 4);
    g.refs = alloc((size_t)(n_refs + 2) * sizeof(CCell), 32);        /* + slack: the walk loads 32 bytes at its cursor */
    if (n_refs) memcpy(at<CCell>(g.refs), refs.data(), (size_t)n_refs * sizeof(CCell));
    g.pad[1] = *at<uint32_t>(off - 4u);                            /* the list's length word (compile_list) lives in the record's last word */
    *at<CDda>(rec_off) = g;
    n_dda++;
}

/* ---- clipper programs ---- */
uint32_t Builder::compile_clip(int owner)
{
    const qr_surface &s = v.srf[owner];
    if (s.clip == QR_NULL) return 0;
    const int cdef = s.c_def != 0 ? 1 : 0;
    for (const ClipKey &k : clip_memo)
        if (k.head == s.clip && k.trnode == s.trnode && k.cdef == cdef) return k.off;
    std::vector<CClip> prog;
    int redx = QR_NULL;
    int group_last = -1;                /* index in prog of the last cell emitted for the open cached group */
    for (int e = s.clip; e != QR_NULL; e = E[e].next)
    {
        const qr_elem &el = E[e];
        /* the cached trnode space of a group ends behind its last element (redx), whether or not that element emits a cell */
        struct Closer { int &redx, &group_last; std::vector<CClip> &prog; int e;
                        ~Closer() { if (group_last >= 0 && redx == QR_NULL) { prog[(size_t)group_last].op |= QR_CLF_LASTC; group_last = -1; } } } closer{redx, group_last, prog, e};
        CClip c;
        memset(&c, 0, sizeof(c));
        if (el.simd == QR_NULL)
        {
            c.op = el.data > 0 ? QR_CLT_LEAVE : (QR_CLT_ENTER | (cdef ? QR_CLF_CDEF : 0u));
            prog.push_back(c);
            if (redx != QR_NULL) group_last = (int)prog.size() - 1;
            continue;
        }
        const qr_surface &k = v.srf[el.simd];
        const bool karr = k.srf_t[3] < 0;
        c.srf = srf_off(el.simd);
        if (k.has_trm != 1) c.op |= QR_CLF_FULLM;
        uint32_t mode;
        if (!karr)
        {
            if (redx != QR_NULL) { mode = QR_CLF_CACHED; if (e == redx) redx = QR_NULL; }
            else mode = k.has_trm != 0 ? QR_CLF_OWN : 0u;
        }
        else if (el.simd == s.trnode)
        {
            if (s.has_trm == 0) throw Fail{QR_ERR_UNSUP, "clipper trnode shared with an untransformed surface"};
            c.op |= QR_CLT_TRSAME; redx = el.data; prog.push_back(c); group_last = (int)prog.size() - 1; if (e == redx) redx = QR_NULL; continue;
        }
        else
        {
            if (k.has_trm == 0)
            {
                /* array without transform: outside a cached trnode it writes only state nobody reads */
                if (redx != QR_NULL) throw Fail{QR_ERR_UNSUP, "untransformed array inside a clipper trnode"};
                continue;
            }
            c.op |= QR_CLT_TRNODE; redx = el.data; prog.push_back(c); group_last = (int)prog.size() - 1; if (e == redx) redx = QR_NULL; continue;
        }
        const int ckind = k.srf_t[2];
        if (ckind == 0) continue;                   /* no clip function: no effect */
        if ((k.shift != 0) != (mode != 0))
            throw Fail{QR_ERR_UNSUP, "clipper reads the trnode-space hit outside a trnode (or the reverse)"};
        c.op |= (ckind == 1 ? QR_CLT_PLANE : ckind == 2 ? QR_CLT_QUADJ : QR_CLT_QUAD) | mode;
        if (el.data < 0) c.op |= QR_CLF_INNER;
        const uint32_t ak = (k.axes >> 4) & 3u;
        if (ak == 0) c.op |= QR_CLF_KX; else if (ak == 1) c.op |= QR_CLF_KY;
        if ((k.axes >> 10) & 1u) c.op |= QR_CLF_SGNK;
        if (ckind == 1 && mode != QR_CLF_OWN && ak <= 2)
        {
            /* fast plane cell: the plane's position along its axis with the sign folded in (qr_program.h) */
            c.op |= QR_CLF_FASTPL;
            const float val = (c.op & QR_CLF_SGNK) ? -k.pos[ak] : k.pos[ak];
            memcpy(&c.aux, &val, 4);
            c.sgn = (c.op & QR_CLF_SGNK) ? 0x80000000u : 0u;
            c.mx = ak == 0 ? 0xFFFFFFFFu : 0u; c.my = ak == 1 ? 0xFFFFFFFFu : 0u; c.mz = ak == 2 ? 0xFFFFFFFFu : 0u;
        }
        prog.push_back(c);
        if (mode == QR_CLF_CACHED) group_last = (int)prog.size() - 1;
    }
    CClip endc;
    memset(&endc, 0, sizeof(endc));
    prog.push_back(endc);
    const uint32_t off = alloc(prog.size() * sizeof(CClip), 32);
    memcpy(at<CClip>(off), prog.data(), prog.size() * sizeof(CClip));
    clip_memo.push_back(ClipKey{s.clip, s.trnode, cdef, off});
    st.n_clip_cells += (uint32_t)prog.size() - 1;
    return off;
}

/* ---- light lists ---- */
/*
 * Shadow lists by hit position for surface `si` (an untransformed plane with a finite clip rectangle) and light `lg`,
 * whose shadow list `sh` holds many surfaces: CGrid, qr_program.h.  Returns the record's offset | QR_LISTF_GRID, or 0.
 */
uint32_t Builder::compile_grid(int si, int lg, int sh)
{
    int a, b;
    if (!grid_plane(si, a, b)) return 0;
    const qr_surface &s = v.srf[si];
    const double lo_a = s.min[a], hi_a = s.max[a], lo_b = s.min[b], hi_b = s.max[b];
    const double ea = hi_a - lo_a, eb = hi_b - lo_b;
    /* long enough to be worth it? */
    int n_real = 0;
    for (int e = sh; e != QR_NULL && n_real < kn.grid_min; e = E[e].next) if (is_real(v.srf[E[e].simd])) n_real++;
    if (n_real < kn.grid_min) return 0;
    ListFilter lf(v, bs, *Egrow, sh);
    const double cell = (ea > eb ? ea : eb) / (double)QR_GRID_MAX;
    auto cells = [&](double ext) { int n = (int)(ext / cell + 0.5); return n < 1 ? 1 : (n > (int)QR_GRID_MAX ? (int)QR_GRID_MAX : n); };
    const int nx = cells(ea), ny = cells(eb);
    CGrid g;
    g.nx = (uint32_t)nx; g.ny = (uint32_t)ny; g.comps = (uint32_t)a | ((uint32_t)b << 2);
    g.org_a = (float)lo_a; g.org_b = (float)lo_b;
    g.inv_a = (float)(nx / ea); g.inv_b = (float)(ny / eb);
    std::vector<uint32_t> table((size_t)nx * ny, 0u);
    const double ca = ea / nx, cb = eb / ny;
    /* cells overlap: the kernel's cell index comes from the fp32 local hit (error far below a thousandth of a cell
     * at any sane scale), and the shadow ray starts at the world-space hit, the same point up to rounding */
    const double pad_a = 2e-3 * ca + 1e-3, pad_b = 2e-3 * cb + 1e-3;
    const double pr = __builtin_sqrt((0.5 * ca + pad_a) * (0.5 * ca + pad_a) + (0.5 * cb + pad_b) * (0.5 * cb + pad_b)) + 1e-3;
    /* the chains of the cells: filtered by worker threads (a cell's filter reads the chain and nothing else: 16 us each,
     * 4 x 4 096 of them are 0.27 s of config 5's upload on one core), then appended to E and compiled in cell order -- the
     * image a single thread builds.  QR_HOST_THREADS=1: one thread. */
    const int n_cells = nx * ny;
    std::vector<ListFilter::Run> runs((size_t)n_cells);
    std::vector<int> heads((size_t)n_cells, QR_NULL);
    for_ranges(n_cells, kn.threads(n_cells), [&](int, int c0, int c1) {
        for (int c = c0; c < c1; c++)
        {
            const int i = c % nx, j = c / nx;
            double pc[3] = { s.pos[0], s.pos[1], s.pos[2] };
            pc[a] += lo_a + (i + 0.5) * ca; pc[b] += lo_b + (j + 0.5) * cb;
            const HullPred pred(v.lgt[lg].pos, pc, pr);
            heads[(size_t)c] = lf.filter_run(pred, runs[(size_t)c]);
        }
    });
    for (int c = 0; c < n_cells; c++)
    {
        const int h = lf.append(runs[(size_t)c], heads[(size_t)c]);
        runs[(size_t)c] = ListFilter::Run();
        table[(size_t)c] = compile_list(h);
        n_grid_lists++;
    }
    g.table = alloc(table.size() * 4, 4);
    memcpy(at<uint32_t>(g.table), table.data(), table.size() * 4);
    const uint32_t off = alloc(sizeof(CGrid), 32);
    *at<CGrid>(off) = g;
    n_grids++;
    any_long = true;                /* the kernel instance that knows grids */
    return off | QR_LISTF_GRID;
}

/* compile_grid's geometric conditions: an untransformed plane with a finite clip rectangle; a, b: the in-plane components */
bool Builder::grid_plane(int si, int &a, int &b) const
{
    const qr_surface &s = v.srf[si];
    if (!is_real(s) || s.srf_t[0] != 1 || s.has_trm != 0 || s.shift != 0) return false;
    const int k = (int)((s.axes >> 4) & 3);
    if (k > 2) return false;
    a = k == 0 ? 1 : 0; b = k == 2 ? 1 : 2;
    const bool fin = (s.minmax_t & (1u << a)) && (s.minmax_t & (1u << (3 + a))) && (s.minmax_t & (1u << b)) && (s.minmax_t & (1u << (3 + b)));
    if (!fin) return false;
    const double ea = (double)s.max[a] - s.min[a], eb = (double)s.max[b] - s.min[b];
    return ea > 1e-3 && eb > 1e-3 && ea < 1e18 && eb < 1e18;
}

/*
 * Packet shadow pyramid for surface `si` (a plane as compile_grid takes them), light `lg` and shadow chain `sh`, in an image
 * the packet instance serves: CGrid with QR_GRIDC_PYR, qr_program.h.  `top` is the chain's plain shadow program, the node of
 * level L.  A node's list is what HullPred keeps of its PARENT's list for the node's own patch (centre, half diagonal + the
 * padding of compile_grid for a cell of that size), so it is a sub-sequence of the parent's whatever the predicate's rounding.
 * Returns the record's offset | QR_LISTF_GRID, or 0.
 */
uint32_t Builder::compile_pgrid(int si, int lg, int sh, uint32_t top)
{
    int a, b;
    if (!grid_plane(si, a, b) || top == 0) return 0;
    const qr_surface &s = v.srf[si];
    int n_real = 0;
    for (int e = sh; e != QR_NULL && n_real < kn.pgrid_min; e = E[e].next) if (is_real(v.srf[E[e].simd])) n_real++;
    if (n_real < kn.pgrid_min) return 0;
    const double lo_a = s.min[a], lo_b = s.min[b], ea = (double)s.max[a] - lo_a, eb = (double)s.max[b] - lo_b;
    ListFilter lf(v, bs, *Egrow, sh);
    const int L = kn.pgrid_levels, N = 1 << L, n_pos = (int)lf.ch.size();
    CGrid g;
    g.nx = g.ny = (uint32_t)N; g.comps = (uint32_t)a | ((uint32_t)b << 2) | QR_GRIDC_PYR | ((uint32_t)L << 8);
    g.org_a = (float)lo_a; g.org_b = (float)lo_b;
    g.inv_a = (float)(N / ea); g.inv_b = (float)(N / eb);
    const uint32_t n_words = QR_PGRID_LEVEL_OFF((uint32_t)N, (uint32_t)L) + 1u;
    std::vector<uint32_t> table(n_words, 0u);
    table[n_words - 1] = top;
    /* keep[node][position in the chain], level by level from the top: the parent's AND the node's own predicate.  The nodes of
     * a level are filtered by worker threads, then appended and compiled in node order, as compile_grid does. */
    std::vector<uint8_t> up((size_t)n_pos, 1), cur;
    for (int l = L - 1; l >= 0; l--)
    {
        const int n = N >> l, n_nodes = n * n;
        const double ca = ea / n, cb = eb / n;
        const double pad_a = 2e-3 * ca + 1e-3, pad_b = 2e-3 * cb + 1e-3;
        const double pr = __builtin_sqrt((0.5 * ca + pad_a) * (0.5 * ca + pad_a) + (0.5 * cb + pad_b) * (0.5 * cb + pad_b)) + 1e-3;
        cur.assign((size_t)n_nodes * n_pos, 0);
        std::vector<ListFilter::Run> runs((size_t)n_nodes);
        std::vector<int> heads((size_t)n_nodes, QR_NULL);
        const int np = n >> 1 ? n >> 1 : 1;             /* nodes per row of the level above (one node at level L) */
        for_ranges(n_nodes, kn.threads(n_nodes), [&](int, int c0, int c1) {
            for (int c = c0; c < c1; c++)
            {
                const int i = c % n, j = c / n;
                double pc[3] = { s.pos[0], s.pos[1], s.pos[2] };
                pc[a] += lo_a + (i + 0.5) * ca; pc[b] += lo_b + (j + 0.5) * cb;
                const HullPred pred(v.lgt[lg].pos, pc, pr);
                const uint8_t *par = l == L - 1 ? up.data() : up.data() + (size_t)((j >> 1) * np + (i >> 1)) * n_pos;
                uint8_t *mine = cur.data() + (size_t)c * n_pos;
                for (int q = 0; q < n_pos; q++)
                {
                    const ListFilter::Node &nd = lf.ch[(size_t)q];
                    mine[q] = par[q] && (nd.head ? (!nd.bounded || pred(nd.bound, true)) : pred(nd.bound, nd.bounded));
                }
                /* the nodes keep their bounding-volume elements (flat_max -1): on the engine's chains a volume stands in front
                 * of a trnode, and a wave that misses it skips the transform (profiles/r30_packet_shadow_pyramid.txt) */
                heads[(size_t)c] = lf.filter_nodes_run([&](int q) { return mine[q] != 0; }, runs[(size_t)c], -1);
            }
        });
        uint32_t *row = table.data() + QR_PGRID_LEVEL_OFF((uint32_t)N, (uint32_t)l);
        for (int c = 0; c < n_nodes; c++)
        {
            if (heads[(size_t)c] == ListFilter::SOURCE_LIST) { row[c] = top; n_pgrid_nodes++; continue; }
            const int h = lf.append(runs[(size_t)c], heads[(size_t)c]);
            runs[(size_t)c] = ListFilter::Run();
            row[c] = compile_list(h, true);
            if (row[c]) n_pgrid_nodes++;
        }
        up.swap(cur);
    }
    n_pgrid_nodes++;                /* the top */
    g.table = alloc(table.size() * 4, 4);
    memcpy(at<uint32_t>(g.table), table.data(), table.size() * 4);
    const uint32_t off = alloc(sizeof(CGrid), 32);
    *at<CGrid>(off) = g;
    n_pgrids++;
    return off | QR_LISTF_GRID;
}

uint32_t Builder::compile_lights(int head)
{
    if (head == QR_NULL) return 0;
    if (light_off[head]) return light_off[head];
    std::vector<CLight> ls;
    for (int e = head; e != QR_NULL; e = E[e].next)
    {
        CLight l;
        l.lgt = o_lgt + (uint32_t)E[e].simd * (uint32_t)sizeof(qr_light);
        const int sh = E[e].data, lg = E[e].simd;       /* copies: compile_grid appends to E */
        l.shadow = compile_list(sh, true);
        if (Egrow != nullptr && light_user[head] >= 0 && sh != QR_NULL)
        {
            const uint32_t g = kn.grid_min > 0 ? compile_grid(light_user[head], lg, sh) : 0u;
            if (g) l.shadow = g;
            else if (pgrid_ok) { if (const uint32_t pg = compile_pgrid(light_user[head], lg, sh, l.shadow)) l.shadow = pg; }
        }
        ls.push_back(l);
    }
    ls.back().lgt |= QR_CLIGHT_LAST;
    const uint32_t off = alloc(ls.size() * sizeof(CLight), 8);
    memcpy(at<CLight>(off), ls.data(), ls.size() * sizeof(CLight));
    light_off[head] = off;
    return off;
}

} // namespace qrc
