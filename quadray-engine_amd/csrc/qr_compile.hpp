/*
 * qr_compile.hpp - what the scene compiler's translation units share (host only; nothing the device code includes).
 *
 *   qr_validate.cpp      qr_snapshot_validate, qr_bound_spheres
 *   qr_compile.cpp       qr_program_build: the steps of one image, the restart loop; qr_program_stats
 *   qr_builder.cpp       Builder: list, clipper and light-list programs (classify, bound, lay out, emit, flag)
 *   qr_schedule.cpp      the wave schedule, a function of the tile lists
 *   qr_verify.cpp        qr_program_verify
 *   qr_lists.cpp         qr_snapshot_build_lists (with qr_list_filter.hpp: ListFilter, HullPred)
 */
#ifndef QR_COMPILE_HPP
#define QR_COMPILE_HPP

#include "qr_internal.h"
#include "qr_program.h"

#include <cstring>
#include <cstdlib>
#include <cstdio>
#include <ctime>
#include <algorithm>
#include <thread>

#ifndef QR_SIDES_EXACT_MAX
#define QR_SIDES_EXACT_MAX 512              /* see qr_lists.cpp */
#endif

namespace qrc {

inline bool is_real(const qr_surface &s) { return s.srf_t[3] >= 0 && s.srf_t[3] < QR_TAG_SURFACE_MAX; }

struct Fail { int rc; std::string msg; };

/*
 * The compiler's knobs: read from the environment at the start of every qr_program_build / qr_snapshot_build_lists call (tests
 * and A/B runs change them between builds inside one process) and passed down.
 */
struct Knobs
{
    int    cull = 3;                        /* QR_CULL: cull cells on 0 nothing, 1 planes, 2 planes + open quadrics, 3 all */
    int    grid_min = 256;                  /* QR_GRID: shadow lists with at least this many surfaces get a grid (CGrid); 0 turns the grids off */
    int    pgrid_min = 12;                  /* QR_PGRID: in images the packet instance serves, a clipped plane's shadow list with at least this many
                                             * surfaces gets a pyramid of filtered lists (CGrid with QR_GRIDC_PYR); 0 turns them off */
    int    pgrid_levels = 4;                /* QR_PGRID_LEVELS: L of the pyramids, 2^L x 2^L cells at level 0 (1..QR_PGRID_LEVELS_MAX) */
    int    dda_min = 512;                   /* QR_DDA: lists with at least this many bounded members get a uniform grid (CDda); 0 turns them off */
    double dda_cells = 2.0;                 /* QR_DDA_CELLS: grid cells per member: 0.5 .. 8 are within 5 % of each other on the 10k scene */
    bool   drop_shadowless = true;          /* QR_SHADOWLESS=0: shadow lists keep the cells that cast no shadow */
    bool   boxes = true;                    /* QR_BOX=0: cull cells carry spheres only (A/B runs, tests) */
    bool   dedup = true;                    /* QR_LIST_DEDUP=0: one program per chain (A/B) */
    int    host_threads = -1;               /* QR_HOST_THREADS: worker threads of the host passes; unset (-1): the machine's */
    int    sides_exact_max = QR_SIDES_EXACT_MAX;    /* QR_SIDES_EXACT_MAX: scenes up to this many surfaces get the engine's per-side lists */
    Knobs();                                /* from the environment (qr_compile.cpp) */
    /* worker threads of a host pass over n items: at most 16, no more than one per 64 items */
    int threads(int n) const
    {
        int t = host_threads >= 0 ? host_threads : (int)std::thread::hardware_concurrency();
        if (t > 16) t = 16;
        if (t > n / 64) t = n / 64;
        return t < 1 ? 1 : t;
    }
};

/* f(t, lo, hi) over [0, n) cut into n_thr ranges, range t on a thread of its own; returns when all are done.  The callers
 * merge what the ranges made in range order, so the result is what one thread builds. */
template <typename F>
void for_ranges(int n, int n_thr, F f)
{
    if (n_thr <= 1) { f(0, 0, n); return; }
    std::vector<std::thread> pool;
    for (int t = 0; t < n_thr; t++)
        pool.emplace_back(f, t, (int)((long long)n * t / n_thr), (int)((long long)n * (t + 1) / n_thr));
    for (std::thread &t : pool) t.join();
}

/* QR_COMPILE_TIMING / QR_VERIFY_TIMING: "  <label> <phase> <ms>" on stderr at the end of every phase (tools/host_compile_time.py) */
struct PhaseTimer
{
    const bool on; const char *label; const int width;
    struct timespec t0;
    PhaseTimer(bool on_, const char *label_, int width_) : on(on_), label(label_), width(width_) { if (on) clock_gettime(CLOCK_MONOTONIC, &t0); }
    void tick(const char *what)
    {
        if (!on) return;
        struct timespec t1; clock_gettime(CLOCK_MONOTONIC, &t1);
        fprintf(stderr, "  %s %-*s %.3f ms\n", label, width, what, (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6);
        t0 = t1;
    }
};

/*
 * The union of an array's members' bounding spheres around the first member's centre: member(k) is the sphere of chain
 * position k in (i, last], nullptr where k is no member.  False when there is no member or one is unbounded; else the centre
 * member and the radius, unpadded -- every caller pads it its own way.
 */
template <typename Member>
bool array_union(int i, int last, Member member, const BSphere *&c0, double &R)
{
    c0 = nullptr; R = 0.0;
    for (int k = i + 1; k <= last; k++)
    {
        const BSphere *m = member(k);
        if (m == nullptr) continue;
        if (!(m->r < 1e18f)) return false;
        if (c0 == nullptr) c0 = m;
        const double dx = (double)m->c[0] - c0->c[0], dy = (double)m->c[1] - c0->c[1], dz = (double)m->c[2] - c0->c[2];
        const double d = __builtin_sqrt(dx * dx + dy * dy + dz * dz) + (double)m->r;
        if (d > R) R = d;
    }
    return c0 != nullptr;
}

/*
 * The image-only words of a material record (qr_program.h, QR_MATX_*): `m` is the IMAGE's record (`tex` a byte offset into
 * `img`).  A one-texel texture's colour is finished here, with shade()'s operations: (float)(int32_t)((texel >> s) & cmask) /
 * clamp, one fp32 conversion and one IEEE fp32 division per channel -- the bits the kernel's own division gives.
 */
inline float channel_colour(uint32_t v, uint32_t cmask, float clamp)
{
    volatile float num = (float)(int32_t)(v & cmask);      /* volatile: fp32 operands, one fp32 division, whatever the flags */
    volatile float den = clamp;
    return num / den;
}

inline void material_colour(qr_material &m, const uint8_t *img, uint32_t lut = 0)
{
    for (int k = 0; k < 8; k++) m.pad[k] = 0;
    if (m.xmask != 0 || m.ymask != 0)
    {
        if (lut != 0) { m.pad[QR_MATX_FLAGS] = (int32_t)QR_MATF_LUT; m.pad[QR_MATX_LUT] = (int32_t)lut; }
        return;
    }
    uint32_t texel;
    memcpy(&texel, img + (uint32_t)m.tex, 4);
    const int sh[3] = {16, 8, 0};
    for (int c = 0; c < 3; c++)
    {
        const float q = channel_colour(texel >> sh[c], m.cmask, m.clamp);
        memcpy(&m.pad[QR_MATX_COL + c], &q, 4);
    }
    m.pad[QR_MATX_FLAGS] = (int32_t)QR_MATF_COLOUR;
}

/* the image under construction: the blob, its fixed sections, and the list / clipper / light-list programs (qr_builder.cpp) */
struct Builder
{
    const qr_scene_view &v;
    const std::vector<qr_elem> &E;          /* cells: the snapshot's, or the binning pass's                 */
    std::vector<qr_elem> *Egrow = nullptr;  /* the same vector when the compiler may append filtered chains (shadow grids) */
    std::vector<int> light_user;            /* light list head -> the one surface that uses it, -2 several, -1 none */
    const std::vector<BSphere> &bs;
    const Knobs &kn;
    std::vector<uint8_t> &blob;
    int n_srf, n_elm;
    uint32_t o_srf = 0, o_shd = 0, o_mat = 0, o_lgt = 0, o_tex = 0;
    uint32_t n_dda = 0, n_grids = 0, n_grid_lists = 0;
    uint32_t n_pgrids = 0, n_pgrid_nodes = 0;   /* packet shadow pyramids and their nodes with a list (n_grids counts plain CGrids only) */
    bool pgrid_ok = false;                  /* the attempt takes every list for short: pyramids may be built (compile_pgrid) */

    std::vector<uint32_t> list_off;         /* surface list head -> byte offset of its program (0 unseen)   */
    std::vector<uint32_t> shadow_off;       /* ... of its program as a shadow list, where that is another one (compile_list) */
    std::vector<uint32_t> light_off;        /* light list head  -> byte offset                               */
    std::vector<uint8_t> list_heavy;        /* surface list head -> 1 holds a reflective, 2 a non-opaque surface */
    struct ClipKey { int head, trnode, cdef; uint32_t off; };
    std::vector<ClipKey> clip_memo;
    std::vector<int> chain_pos, chain_stamp; int stamp = 0;
    /* scratch of compile_list, kept between calls (a 1080p frame compiles thousands of short tile lists) */
    struct Tmp { int e; uint32_t op; int si; int last; bool emit; };
    std::vector<Tmp> ch;
    std::vector<int> lo_after, lo_self, open_arr, emit_idx;
    std::vector<BSphere> arr_sphere;
    QrProgramStats st = {};
    bool any_long = false;
    bool box_ok = false;                    /* every list is short: cull cells may carry boxes (QR_OPF_BOX) */
    bool any_box = false;
    float box_pad = 0.0f;
    float big = 0.0f;                       /* the scene's largest coordinate: camera origin, finite surface bounds */

    Builder(const qr_scene_view &v_, const std::vector<qr_elem> &E_, const std::vector<BSphere> &bs_, const Knobs &kn_, std::vector<uint8_t> &b)
        : v(v_), E(E_), bs(bs_), kn(kn_), blob(b), n_srf((int)v_.hdr->n_srf), n_elm((int)E_.size())
    {
        list_off.assign((size_t)n_elm + 1, 0); light_off.assign((size_t)n_elm + 1, 0); list_heavy.assign((size_t)n_elm + 1, 0);
        shadow_off.assign((size_t)n_elm + 1, 0);
        chain_pos.assign((size_t)n_elm + 1, 0); chain_stamp.assign((size_t)n_elm + 1, -1);
    }

    uint32_t alloc(size_t bytes, size_t align)
    {
        size_t o = (blob.size() + align - 1) & ~(align - 1);
        if (o + bytes > 0xFFFFFFF0ull) throw Fail{QR_ERR_NOMEM, "compiled scene exceeds 4 GiB"};
        blob.resize(o + bytes, 0);
        return (uint32_t)o;
    }
    template <typename T> T *at(uint32_t off) { return (T *)(blob.data() + off); }
    uint32_t srf_off(int si) const { return o_srf + (uint32_t)si * (uint32_t)sizeof(DSurf); }

    struct Restart {};                      /* thrown by compile_list: a long chain in a build that assumed there is none */

    uint32_t compile_list(int head, bool as_shadow = false);
    uint32_t compile_clip(int owner);
    uint32_t compile_lights(int head);

private:
    /* chains compiled so far by content (see compile_list): an open hash of entry indices, entries chained on collisions */
    struct DedupEnt { size_t first, len; uint64_t key; uint32_t off; uint8_t heavy; int32_t next; };
    std::vector<DedupEnt> dedup_ent;
    std::vector<int32_t> dedup_slot = std::vector<int32_t>(1024, -1);
    std::vector<int32_t> dedup_pool, dk;
    int32_t dedup_last = -1;                /* the entry the previous chain matched or made: neighbouring tiles repeat it */
    bool dedup_equal(const DedupEnt &d, uint64_t key) const
    {
        return d.key == key && d.len == dk.size() && memcmp(dedup_pool.data() + d.first, dk.data(), dk.size() * sizeof(int32_t)) == 0;
    }
    void dedup_add(uint64_t key, uint32_t off, uint8_t heavy);

    /* what compile_list knows of the whole list once its cells are classified */
    struct ListProps
    {
        int n_emitted = 0, n_bv = 0;        /* cells, bounding-volume cells among them */
        bool has_trnode = false;            /* a walk carries trnode state: a trnode cell, or a cell in a CACHED trnode space */
        bool world = true;                  /* no trnode cell and no cell with a transform at all (CACHED or OWN) */
        bool div = true;                    /* no cell with a clipper program */
        uint8_t heavy = 0;                  /* 1 holds a reflective, 2 a non-opaque surface (emitted or not) */
    };
    /* the steps of compile_list over the chain in `ch` */
    int  chain_begin(int head, bool as_shadow, bool &shadowless);
    bool dedup_key(int head, bool as_shadow, uint64_t &key);
    const DedupEnt *dedup_find(uint64_t key);
    void classify(int n, bool as_shadow);
    void check_nesting(int n);
    void array_spheres(int n);
    ListProps list_props(int n) const;
    bool wants_dda(int n, const ListProps &lp) const;
    void emit_cells(int n, uint32_t off, bool has_trnode);
    void build_dda(uint32_t rec_off, uint32_t off, int n);
    uint32_t compile_grid(int si, int lg, int sh);
    uint32_t compile_pgrid(int si, int lg, int sh, uint32_t top);
    bool grid_plane(int si, int &a, int &b) const;
};

/*
 * The wave schedule (qr_schedule.cpp): `order` gets one entry {footprint | heaviness << 30, tile-list offset} per wave;
 * sched_blocks > 1 groups it by horizontal block of the frame, see QrProgram.  Throws Fail.
 */
void build_schedule(const qr_frame &frm, const std::vector<uint32_t> &tile_off, const std::vector<uint8_t> &tile_heavy, int sched_blocks,
                    int clear_run, std::vector<uint32_t> &order, std::vector<uint32_t> &block_first, std::vector<uint32_t> &block_row,
                    PhaseTimer &timer);

} // namespace qrc

#endif /* QR_COMPILE_HPP */
