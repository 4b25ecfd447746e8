/*
 * qr_lists.cpp - per-surface list building (the role of rt_SceneThread::ssort / lsort, engine.cpp:2134-2753):
 * qr_snapshot_build_lists and its C entry.  Snapshot in, snapshot out; the compiler proper (qr_compile.cpp) comes after it.
 */
#include "qr_list_filter.hpp"
#include "qr_sides.h"

using namespace qrc;

/*
 * For scenes that arrive with one global surface list only (scenes the reference engine did not prepare: the
 * synthetic 10k-quadric scene, user scenes), build what the engine's ssort / lsort build with their bounding-box
 * predicates (bbox_shad rtgeom.cpp:1004, bbox_side rtgeom.cpp:1954):
 *   - per surface and light a SHADOW list: the members of the global list that can stand between the light
 *     and the surface -- here: whose conservative bounding sphere (qr_bounds.hpp) meets the hull of the light's
 *     position and the surface's bounding sphere;
 *   - per surface side a REFLECTION / REFRACTION list: for an untransformed plane the members that reach into
 *     the half-space that side faces; everything for other shapes (what the engine does for them too);
 *   - light lists: every light, with its shadow list.
 * Lists only cull (a shorter list must not change any pixel), so the predicates are our own conservative ones, not
 * the engine's box arithmetic.  The global list's ORDER and STRUCTURE are kept: members keep their relative order,
 * a bounding-volume or trnode element stays in front of its first kept member with `data` patched to the last
 * kept one -- the format the walk (and the reference) expects.  Arrays whose union sphere fails the predicate are
 * pruned without visiting their members.  Output: a new snapshot.
 *
 * Per-side placement (qr_sides.cpp = the engine's bbox_side / clip_side): NOT a cull in the engine but part of its picture.
 * Lights: with RT_OPTS_2SIDED its lsort (engine.cpp:2503-2533) enters a light on the outer and / or the inner light list by
 * where it stands relative to the clipped surface, so the inside of a closed convex shell never gets a light that stands
 * outside, whether or not the shell casts a shadow.  Surfaces: ssort (engine.cpp:2134-2450) puts every node on the outer
 * and / or inner list of a surface whose material reflects or is not opaque; a convex shape is absent from its own outer
 * list, a bowl's inside holds what the box test sees through its opening.  The engine's per-side lists are copies of its
 * hierarchy per surface -- memory grows with the square of the scene (engine.cpp:2951-2956) -- so scenes with more than
 * QR_SIDES_EXACT_MAX real surfaces keep ONE shared list for both sides of their quadrics (a superset of what the engine would
 * place there; planes get the half-space filter below).
 */
int qr_snapshot_build_lists(const qr_scene_view &v, std::vector<uint8_t> &out, std::string &err)
{
    const Knobs kn;
    int rc = qr_snapshot_validate(v, err);
    if (rc != QR_OK) return rc;
    const qr_frame &fr = *v.frame;
    if (fr.clist == QR_NULL) { err = "snapshot has no global list (clist)"; return QR_ERR_ARG; }
    std::vector<BSphere> bs;
    qr_bound_spheres(v, bs);
    const int n_srf = (int)v.hdr->n_srf, n_lgt = (int)v.hdr->n_lgt;
    std::vector<qr_elem> E(v.elm, v.elm + v.hdr->n_elm);
    std::vector<qr_surface> S(v.srf, v.srf + n_srf);
    ListFilter lf(v, bs, E, fr.clist);
    QrSideGeom geom(v);
    const bool exact_sides = lf.n_real <= kn.sides_exact_max;
    std::vector<uint8_t> mask(lf.ch.size());
    /* boxes of the chain's array elements (transform nodes; bounding-volume nodes where the list has them: the engine drops
     * them from a camera list when its screen tiling is on, engine.cpp:1711-1725) */
    std::vector<int> head_box(lf.ch.size(), -1);
    if (exact_sides)
    {
        std::vector<int> leaves;
        for (size_t k = 0; k < lf.ch.size(); k++)
        {
            if (!lf.ch[k].head) continue;
            leaves.clear();
            for (int q = (int)k + 1; q <= lf.ch[k].last; q++)
                if (!lf.ch[q].head && is_real(v.srf[lf.ch[q].si])) leaves.push_back(lf.ch[q].si);
            const qr_surface &rec = v.srf[lf.ch[k].si];
            int space = rec.srf_t[3] < 0 ? lf.ch[k].si : rec.trnode;          /* a transform node's box lives in its own space */
            if (rec.srf_t[3] >= 0 && rec.trnode == QR_NULL && rec.sci[3] != 0.75f && !leaves.empty())
            {
                /* sphere form of a transform node's inner box (object.cpp:2268-2289): the box is in the members' space */
                int t = v.srf[leaves[0]].trnode;
                for (int m : leaves) if (v.srf[m].trnode != t) t = QR_NULL;
                space = t;
            }
            head_box[k] = geom.add_array_box(leaves.data(), (int)leaves.size(), space);
        }
    }

    /* one surface: its two side lists, its light lists with their shadow lists.  Appends to the element array it is given */
    auto one_surface = [&](int i, ListFilter &lf, std::vector<qr_elem> &E, std::vector<uint8_t> &mask, std::vector<qr_surface> &S)
    {
        qr_surface &s = S[i];
        if (!is_real(s)) return;
        const BSphere &sb = bs[i];
        const bool s_bounded = sb.r < 1e18f;
        /* reflection / refraction lists per side */
        int side_list[2] = { fr.clist, fr.clist };
        if (exact_sides)
        {
            /* the walk of ssort / lsort over the hierarchy, engine.cpp:2222-2330, 2575-2680: a node's sides come from
             * bbox_side -- unless an array above it was seen from one side only: then everything under that array goes where
             * the array went, unasked; an array seen from no side (every corner within the margin of a plane) is not entered
             * at all.  The same placement serves the surface lists and, below, the shadow list of each side's light entries */
            int inherit_until = -1; uint8_t c = 3;
            for (int k = 0; k < (int)lf.ch.size(); k++)
            {
                if (k > inherit_until)
                {
                    inherit_until = -1;
                    const ListFilter::Node &nd = lf.ch[k];
                    if (nd.head) c = (uint8_t)geom.side(head_box[k], i);
                    else c = is_real(v.srf[nd.si]) ? (uint8_t)geom.side(nd.si, i) : (uint8_t)3;
                    if (nd.head && c < 3) inherit_until = nd.last;
                }
                mask[k] = c;
            }
            /* surfaces whose material neither reflects nor lets light through keep the global list on both sides (no ray
             * ever walks it, engine.cpp:2155-2176) */
            if (geom.builds_side_lists(i))
                for (int side = 0; side < 2; side++)
                {
                    const uint8_t bit = side == 0 ? 2 : 1;          /* side 0 = outer */
                    side_list[side] = lf.filter_nodes([&](int k) { return (mask[k] & bit) != 0; });
                }
        }
        else if (s.srf_t[0] == 1 && s.has_trm == 0)
        {
            const int k = (int)((s.axes >> 4) & 3);
            const double sg = ((s.axes >> 10) & 1) ? -1.0 : 1.0;
            for (int side = 0; side < 2; side++)
            {
                /* side 0 (outer) is hit by rays travelling against the signed axis: it faces +sg along k */
                const double face = side == 0 ? sg : -sg;
                side_list[side] = lf.filter([&](const BSphere &x, bool bounded) {
                    if (!bounded) return true;
                    return ((double)x.c[k] - (double)s.pos[k]) * face + (double)x.r * 1.001 + 1e-3 >= 0.0;
                });
            }
        }
        s.lst[1] = side_list[0]; s.lst[3] = side_list[1];
        /* light lists of the two sides; which side a light is entered on is the engine's rule (clip_side), not a cull */
        int l_head[2] = { QR_NULL, QR_NULL }, l_tail[2] = { QR_NULL, QR_NULL };
        for (int l = 0; l < n_lgt; l++)
        {
            /* what may stand between the light and the surface (bbox_shad's role): the hull of the light's position and the
             * surface's bounding sphere; an unbounded surface, or a light inside / next to that sphere, keeps everything */
            const double sc[3] = { sb.c[0], sb.c[1], sb.c[2] };
            const HullPred hp(v.lgt[l].pos, sc, s_bounded ? (double)sb.r : 1e30);
            int shadow = fr.clist;
            if (!exact_sides && !hp.all) shadow = lf.filter(hp);
            const int sides = geom.clip_side(i, v.lgt[l].pos);
            for (int side = 0; side < 2; side++)
            {
                const uint8_t bit = side == 0 ? 2 : 1;
                if (!(sides & bit)) continue;
                /* the engine keeps one shadow list per side a light is entered on: what may cast a shadow (its bbox_shad; here
                 * the hull predicate above) AND is placed on that side of the surface (lsort, engine.cpp:2590-2612) -- the
                 * outer side of a convex shape never tests the shape itself */
                int side_shadow = shadow;
                if (exact_sides)
                    side_shadow = lf.filter_nodes([&](int k) {
                        if (!(mask[k] & bit)) return false;
                        const ListFilter::Node &nd = lf.ch[k];
                        if (!nd.head && !is_real(v.srf[nd.si])) return true;
                        /* the engine's own box predicate, not a tighter or looser one of ours: where it misses a caster (its
                         * corner / face / edge tests are not exhaustive) the reference's picture has no shadow there */
                        return geom.shad(v.lgt[l].pos, nd.head ? head_box[k] : nd.si, i) != 0;
                    });
                qr_elem c; c.simd = l; c.data = side_shadow; c.next = QR_NULL; c.kind = 0;
                E.push_back(c);
                const int ix = (int)E.size() - 1;
                if (l_tail[side] != QR_NULL) E[l_tail[side]].next = ix; else l_head[side] = ix;
                l_tail[side] = ix;
            }
        }
        s.lst[0] = l_head[0]; s.lst[2] = l_head[1];
    };

    /*
     * Large scenes (the hull-predicate path): surfaces are independent of each other, so ranges of them go to worker threads,
     * each with its own copy of the source elements to append to; the appended runs are then concatenated in surface order and
     * their indices shifted -- element for element the array a single thread builds (10 000 objects x 4 lights: 0.67 s on one
     * core).  QR_HOST_THREADS=1: one thread.  The exact path (<= QR_SIDES_EXACT_MAX surfaces) is small and stays serial.
     */
    const int n_thr = exact_sides ? 1 : kn.threads(n_srf);
    if (n_thr == 1)
    {
        for (int i = 0; i < n_srf; i++) one_surface(i, lf, E, mask, S);
    }
    else
    {
        const size_t n0 = E.size();
        struct Part { int lo, hi; std::vector<qr_elem> el; };
        std::vector<Part> part((size_t)n_thr);
        for_ranges(n_srf, n_thr, [&](int t, int lo, int hi) {
            std::vector<qr_elem> Et(E.begin(), E.begin() + (ptrdiff_t)n0);
            ListFilter lft(v, bs, Et, fr.clist);
            std::vector<uint8_t> mk(lft.ch.size());
            for (int i = lo; i < hi; i++) one_surface(i, lft, Et, mk, S);
            part[(size_t)t] = Part{lo, hi, std::vector<qr_elem>(Et.begin() + (ptrdiff_t)n0, Et.end())};
        });
        for (const Part &p : part)
        {
            /* indices >= n0 of this part are its own appended elements: they move to where the part lands */
            const int shift = (int)E.size() - (int)n0;
            auto fix = [&](int32_t &x) { if (x >= (int32_t)n0) x += shift; };
            for (qr_elem c : p.el) { fix(c.next); fix(c.data); E.push_back(c); }
            for (int i = p.lo; i < p.hi; i++)
                if (is_real(S[(size_t)i])) for (int k = 0; k < 4; k++) fix(S[(size_t)i].lst[k]);
        }
    }

    /* serialise the new snapshot: same sections, larger element array */
    qr_header h = *v.hdr;
    auto a16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    size_t off = a16(sizeof(qr_header));
    h.header_bytes = sizeof(qr_header);
    h.off_frame = (uint32_t)off;  off = a16(off + sizeof(qr_frame));
    h.off_srf = (uint32_t)off;    off = a16(off + (size_t)n_srf * sizeof(qr_surface));
    h.off_mat = (uint32_t)off;    off = a16(off + (size_t)h.n_mat * sizeof(qr_material));
    h.off_lgt = (uint32_t)off;    off = a16(off + (size_t)h.n_lgt * sizeof(qr_light));
    h.off_elm = (uint32_t)off;    off = a16(off + E.size() * sizeof(qr_elem));
    h.off_tiles = (uint32_t)off;  off = a16(off + (size_t)h.n_tiles * 4);
    h.off_texels = (uint32_t)off; off = a16(off + (size_t)h.n_texels * 4);
    if (off > 0xFFFFFFFFull) { err = "snapshot exceeds 4 GiB"; return QR_ERR_NOMEM; }
    h.n_elm = (uint32_t)E.size();
    h.total_bytes = (uint32_t)off;
    out.assign(off, 0);
    memcpy(out.data(), &h, sizeof(h));
    memcpy(out.data() + h.off_frame, v.frame, sizeof(qr_frame));
    memcpy(out.data() + h.off_srf, S.data(), S.size() * sizeof(qr_surface));
    if (h.n_mat) memcpy(out.data() + h.off_mat, v.mat, (size_t)h.n_mat * sizeof(qr_material));
    if (h.n_lgt) memcpy(out.data() + h.off_lgt, v.lgt, (size_t)h.n_lgt * sizeof(qr_light));
    memcpy(out.data() + h.off_elm, E.data(), E.size() * sizeof(qr_elem));
    if (h.n_tiles) memcpy(out.data() + h.off_tiles, v.tiles, (size_t)h.n_tiles * 4);
    if (h.n_texels) memcpy(out.data() + h.off_texels, v.texels, (size_t)h.n_texels * 4);
    return QR_OK;
}

extern "C" int qr_snapshot_build_lists_c(const void *blob, uint64_t size, void **out_blob, uint64_t *out_size)
{
    if (blob == nullptr || out_blob == nullptr || out_size == nullptr) return qr_fail(QR_ERR_ARG, "null argument");
    qr_scene_view v;
    const int rc0 = qr_scene_view_init(&v, blob, size);
    if (rc0 != 0) return qr_fail(QR_ERR_ARG, "malformed snapshot (qr_scene_view_init " + std::to_string(rc0) + ")");
    std::vector<uint8_t> out;
    std::string err;
    const int rc = qr_snapshot_build_lists(v, out, err);
    if (rc != QR_OK) return qr_fail(rc, err);
    void *p = malloc(out.size());
    if (p == nullptr) return qr_fail(QR_ERR_NOMEM, "out of memory");
    memcpy(p, out.data(), out.size());
    *out_blob = p; *out_size = out.size();
    return QR_OK;
}
