/*
 * qr_list_filter.hpp - filtered copies of a surface list by the members' bounds: what the per-surface list building
 * (qr_lists.cpp) and the shadow grids (qr_builder.cpp compile_grid) make their lists with.  Host only.
 */
#ifndef QR_LIST_FILTER_HPP
#define QR_LIST_FILTER_HPP

#include "qr_compile.hpp"

#ifndef QR_FLAT_LIST_MAX
#define QR_FLAT_LIST_MAX 128                /* a filtered list of at most this many surfaces is written without its arrays */
#endif

namespace qrc {

struct ListFilter
{
    const qr_scene_view &v;
    const std::vector<BSphere> &bs;
    std::vector<qr_elem> &E;                /* grows */
    struct Node { int e; int si; int last; bool head; BSphere bound; bool bounded; };
    std::vector<Node> ch;
    int n_real = 0;                         /* surfaces in the chain */

    /* the chain at `clist` of E (which also receives the filtered chains: elements are read by index only) */
    ListFilter(const qr_scene_view &v_, const std::vector<BSphere> &bs_, std::vector<qr_elem> &E_, int clist)
        : v(v_), bs(bs_), E(E_)
    {
        std::vector<int> pos_of(E.size(), -1);
        for (int e = clist; e != QR_NULL; e = E[e].next) { pos_of[e] = (int)ch.size(); ch.push_back(Node{e, E[e].simd, -1, false, {}, false}); }
        const int n = (int)ch.size();
        n_real = 0;
        for (int i = 0; i < n; i++) if (is_real(v.srf[ch[i].si])) n_real++;
        for (int i = 0; i < n; i++)
        {
            const qr_elem el = E[ch[i].e];
            const qr_surface &s = v.srf[el.simd];
            const bool head = (el.kind & 3) == 1 || s.srf_t[3] < 0;
            ch[i].head = head && el.data != QR_NULL && pos_of[el.data] >= i;
            if (ch[i].head) ch[i].last = pos_of[el.data];
            else { ch[i].bound = bs[el.simd]; ch[i].bounded = is_real(s) && bs[el.simd].r < 1e18f; }
        }
        /* union spheres of arrays, innermost first (a later head nests inside an earlier one) */
        for (int i = n - 1; i >= 0; i--)
        {
            if (!ch[i].head) continue;
            const BSphere *c0; double R;
            ch[i].bounded = array_union(i, ch[i].last, [&](int k) {
                return !ch[k].head && is_real(v.srf[ch[k].si]) ? &ch[k].bound : nullptr; }, c0, R);
            if (!ch[i].bounded) continue;
            ch[i].bound = *c0; ch[i].bound.r = (float)(R * 1.0001 + 1e-4);
        }
    }

    /*
     * A filtered chain before it is part of E: its elements with `next` (and the `data` of kept array heads, flagged in
     * `local`) as indices INTO THE RUN.  filter_run only reads the filter and E, so many threads may filter one chain at a time;
     * append() then makes a run part of E, one after the other.
     */
    struct Run { std::vector<qr_elem> el; std::vector<uint8_t> local; };
    enum { SOURCE_LIST = -2 };              /* filter_run's result when nothing was dropped: the source chain itself */

    /* keep(sphere, bounded) -> may a surface with this bound matter; returns the new list's head */
    template <typename Pred>
    int filter(Pred keep)
    {
        Run run;
        return append(run, filter_run(keep, run));
    }
    template <typename Pred>
    int filter_run(Pred keep, Run &run) const
    {
        return filter_nodes_run([&](int i) {
            const Node &nd = ch[i];
            if (nd.head) return !nd.bounded || keep(nd.bound, true);
            return keep(nd.bound, nd.bounded);
        }, run);
    }

    /* keep(i) by position in the chain: for an array element "may any member matter" (false prunes the array without
     * visiting its members), for a surface "does it belong on the list".  A list that keeps everything IS the source list:
     * its head is returned and nothing is allocated (per-surface copies of one global list are what makes the engine's
     * lists grow with the square of the scene). */
    template <typename Pred>
    int filter_nodes(Pred keep)
    {
        Run run;
        return append(run, filter_nodes_run(keep, run));
    }

    /* the run becomes the tail of E; head as filter_nodes_run returned it -> the chain's head in E */
    int append(const Run &run, int head)
    {
        if (head == SOURCE_LIST) return ch[0].e;
        const int base = (int)E.size();
        for (size_t i = 0; i < run.el.size(); i++)
        {
            qr_elem c = run.el[i];
            if (c.next != QR_NULL) c.next += base;
            if (run.local[i] && c.data != QR_NULL) c.data += base;
            E.push_back(c);
        }
        return head == QR_NULL ? QR_NULL : head + base;
    }

    /* flat_max: a run that keeps at most this many surfaces is written without its bounding-volume elements (-1: never) */
    template <typename Pred>
    int filter_nodes_run(Pred keep, Run &run, int flat_max = QR_FLAT_LIST_MAX) const
    {
        run.el.clear(); run.local.clear();
        std::vector<qr_elem> &R = run.el;
        bool dropped = false;
        struct Open { int idx; int out; int last; };
        std::vector<Open> open;
        int head = QR_NULL, tail = QR_NULL;
        auto emit = [&](int src_e, int data) {
            qr_elem c = E[src_e];
            c.data = data; c.next = QR_NULL;
            R.push_back(c); run.local.push_back(0);
            const int ix = (int)R.size() - 1;
            if (tail != QR_NULL) R[tail].next = ix; else head = ix;
            tail = ix;
            return ix;
        };
        auto close_until = [&](int i) {
            while (!open.empty() && open.back().last < i)
            {
                if (open.back().out != QR_NULL) { R[open.back().out].data = tail; run.local[open.back().out] = 1; }     /* last kept member */
                open.pop_back();
            }
        };
        const int n = (int)ch.size();
        for (int i = 0; i < n; )
        {
            close_until(i);
            const Node &nd = ch[i];
            if (nd.head)
            {
                if (!keep(i)) { dropped = true; i = nd.last + 1; continue; }      /* prune the array */
                open.push_back(Open{i, QR_NULL, nd.last});
                i++;
                continue;
            }
            const bool real = is_real(v.srf[nd.si]);
            if (!real || keep(i))
            {
                for (Open &o : open) if (o.out == QR_NULL) o.out = emit(ch[o.idx].e, QR_NULL);
                emit(nd.e, E[nd.e].data);
            }
            else dropped = true;
            i++;
        }
        close_until(n);
        if (!dropped && n > 0) { R.clear(); run.local.clear(); return SOURCE_LIST; }
        /* a list that keeps only a handful of surfaces does not need their bounding-volume elements (AR_ptr elements
         * only skip work, tracer.cpp:3955-4054): written flat it is a fraction of the cells.  Trnode elements stay. */
        int kept = 0;
        for (int e = head; e != QR_NULL; e = R[e].next) if (is_real(v.srf[R[e].simd])) kept++;
        if (kept <= flat_max)
        {
            int nh = QR_NULL, nt = QR_NULL;
            for (int e = head; e != QR_NULL; )
            {
                const int nx = R[e].next;
                if ((R[e].kind & 3) != 1)
                {
                    if (nt != QR_NULL) R[nt].next = e; else nh = e;
                    nt = e; R[e].next = QR_NULL;
                }
                e = nx;
            }
            head = nh;
        }
        return head;
    }
};


/*
 * May a surface with bounding sphere x stand between the point lp and some point of the sphere (sc, sr)?  The hull of
 * the light position and that sphere: at parameter tau in [0,1] along the axis a sphere of radius tau sr; x meets it iff
 * min_tau |c - axis(tau)| - tau sr <= r_x; the minimum is at least d_min sqrt(1 - rho^2) - tc sr with d_min the
 * distance to the axis segment and tc its parameter (bbox_shad's role, rtgeom.cpp:1004).
 */
struct HullPred
{
    double lp[3], D[3], D2, Dl, sr, shrink; bool all;
    HullPred(const float *light_pos, const double *sc, double sr_) : sr(sr_)
    {
        for (int k = 0; k < 3; k++) { lp[k] = light_pos[k]; D[k] = sc[k] - lp[k]; }
        D2 = D[0] * D[0] + D[1] * D[1] + D[2] * D[2]; Dl = __builtin_sqrt(D2);
        const double rho = Dl > 0.0 ? sr / Dl : 2.0;
        all = !(rho < 0.95);
        shrink = all ? 0.0 : __builtin_sqrt(1.0 - rho * rho);
    }
    bool operator()(const BSphere &x, bool bounded) const
    {
        if (all || !bounded) return true;
        const double P[3] = { x.c[0] - lp[0], x.c[1] - lp[1], x.c[2] - lp[2] };
        const double t = (P[0] * D[0] + P[1] * D[1] + P[2] * D[2]) / D2;
        const double tc = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
        const double q[3] = { P[0] - tc * D[0], P[1] - tc * D[1], P[2] - tc * D[2] };
        const double dmin = __builtin_sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
        const double xr = (double)x.r * 1.001 + 1e-3;
        if (t > 1.0 + (sr + xr) / Dl + 1e-3) return false;          /* behind the surface */
        return dmin * shrink <= xr + tc * sr * 1.001 + 1e-3;
    }
};

} // namespace qrc

#endif /* QR_LIST_FILTER_HPP */
