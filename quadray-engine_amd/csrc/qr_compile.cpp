/*
 * qr_compile.cpp - host side: snapshot (include/qr_scene.h) -> the compiled device image of qr_program.h.
 *
 *   qr_program_build       per-surface records, list programs, clipper programs, light lists, wave schedule: the steps of one
 *                          image in order, each a function of what it reads and writes, and the restart loop around them
 *   qr_program_stats[_ex]  validate + compile + verify a snapshot without a device
 *
 * The pieces are listed in qr_compile.hpp.  Pure host code: no HIP here, so the CPU test-suite exercises it on every fixture.
 */
#include "qr_compile.hpp"

using namespace qrc;

static int env_int(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }

Knobs::Knobs()
    : cull(env_int("QR_CULL", 3)), grid_min(env_int("QR_GRID", 256)),
      pgrid_min(env_int("QR_PGRID", 12)), pgrid_levels(std::min(std::max(env_int("QR_PGRID_LEVELS", 4), 1), (int)QR_PGRID_LEVELS_MAX)), dda_min(env_int("QR_DDA", 512)),
      drop_shadowless(env_int("QR_SHADOWLESS", 1) != 0), boxes(env_int("QR_BOX", 1) != 0), dedup(env_int("QR_LIST_DEDUP", 1) != 0),
      host_threads(getenv("QR_HOST_THREADS") ? std::max(0, env_int("QR_HOST_THREADS", 0)) : -1),
      sides_exact_max(env_int("QR_SIDES_EXACT_MAX", QR_SIDES_EXACT_MAX))
{
    if (const char *pm = getenv("QR_DDA_CELLS")) dda_cells = atof(pm);
}

namespace {

/* QR_COMPILE_TIMING, QR_CLEAR_RUN: read once per process */
bool compile_timing() { static const bool on = getenv("QR_COMPILE_TIMING") != nullptr; return on; }
int clear_run_max()
{
    static const int r = std::min(std::max(env_int("QR_CLEAR_RUN", QR_CLEAR_RUN_MAX), 1), QR_CLEAR_RUN_MAX);
    return r;
}

/* shadow grids (CGrid) append filtered chains to the cell array: the build works on a copy then.  Only scenes with long
 * shadow lists on clipped planes get any, so the per-frame compile of the engine's scenes never copies. */
bool wants_shadow_grids(const qr_scene_view &v, size_t n_elm, const Knobs &kn, bool pgrid_ok)
{
    const bool grids = kn.grid_min > 0 && n_elm >= (size_t)kn.grid_min;
    const bool pgrids = pgrid_ok && n_elm >= (size_t)kn.pgrid_min;     /* packet shadow pyramids (compile_pgrid) append chains too */
    if (!grids && !pgrids) return false;
    for (int i = 0; i < (int)v.hdr->n_srf; i++)
    {
        const qr_surface &q = v.srf[i];
        if (is_real(q) && q.srf_t[0] == 1 && q.has_trm == 0 && q.shift == 0 && (q.lst[0] != QR_NULL || q.lst[2] != QR_NULL)) return true;
    }
    return false;
}

void find_light_users(Builder &b, size_t n_elm)
{
    b.light_user.assign(n_elm + 1, -1);
    for (int i = 0; i < b.n_srf; i++)
    {
        const qr_surface &q = b.v.srf[i];
        if (!is_real(q)) continue;
        for (int k = 0; k < 2; k++)
        {
            const int h = q.lst[k * 2];
            if (h == QR_NULL) continue;
            b.light_user[h] = (b.light_user[h] == -1 || b.light_user[h] == i) ? i : -2;
        }
    }
}

/* textured, channels of at most 8 bits: one colour table i -> (float)(i & cmask) / clamp per distinct (cmask, clamp) */
bool lut_material(const qr_material &m) { return (m.xmask != 0 || m.ymask != 0) && m.cmask <= 0xFFu; }

struct Layout { uint32_t o_lut, o_til, o_ord; size_t n_sched; };

/* fixed sections; index n_* is a zero record so that masked-off lanes may read it */
Layout fixed_layout(Builder &b, size_t n_tiles, const qr_frame &frm)
{
    const qr_scene_view &v = b.v;
    const int n_mat = (int)v.hdr->n_mat;
    b.alloc(sizeof(DevHeader), 256);
    b.o_srf = b.alloc((size_t)(b.n_srf + 1) * sizeof(DSurf), 128);
    if (b.o_srf != QR_OFF_SRF) throw Fail{QR_ERR_ARG, "layout: DSurf array is not at QR_OFF_SRF"};
    b.o_shd = b.alloc((size_t)(b.n_srf + 1) * sizeof(DShade), 32);
    b.o_mat = b.alloc((size_t)(n_mat + 1) * sizeof(qr_material), 128);
    b.o_lgt = b.alloc((size_t)(v.hdr->n_lgt + 1) * sizeof(qr_light), 64);
    b.o_tex = b.alloc((size_t)(v.hdr->n_texels + 1) * 4, 16);
    /* colour tables of the textured materials (qr_program.h QR_MATF_LUT): room for one per distinct (cmask, clamp) */
    uint32_t n_lut = 0;
    for (int i = 0; i < n_mat; i++)
    {
        const qr_material &m = v.mat[i];
        if (!lut_material(m)) continue;
        bool seen = false;
        for (int j = 0; j < i && !seen; j++)
            seen = (v.mat[j].xmask != 0 || v.mat[j].ymask != 0) && v.mat[j].cmask == m.cmask && memcmp(&v.mat[j].clamp, &m.clamp, 4) == 0;
        if (!seen) n_lut++;
    }
    Layout l;
    l.o_lut = n_lut ? b.alloc((size_t)n_lut * 1024, 64) : 0u;
    l.o_til = b.alloc((n_tiles + 1) * 4, 16);
    /* wave schedule geometry */
    const int fw = frm.fsaa == 2 ? 4 : 8, fh = frm.fsaa == 0 ? 8 : 4;
    const int nbx = (frm.frm_w + fw - 1) / fw, nby = (frm.frm_h + fh - 1) / fh;
    if (nbx > 0x3FFF || nby > 0x3FFF) throw Fail{QR_ERR_ARG, "frame too large"};
    l.n_sched = (size_t)nbx * nby;
    l.o_ord = b.alloc(l.n_sched * 8 + 16, 16);
    return l;
}

/* materials, lights, texels, colour tables */
void fill_materials(Builder &b, uint32_t o_lut)
{
    const qr_scene_view &v = b.v;
    const int n_mat = (int)v.hdr->n_mat;
    qr_material *mat = b.at<qr_material>(b.o_mat);
    memcpy(mat, v.mat, (size_t)n_mat * sizeof(qr_material));
    for (int i = 0; i < n_mat; i++) mat[i].tex = (int32_t)(b.o_tex + (uint32_t)v.mat[i].tex * 4u);
    mat[n_mat].tex = (int32_t)b.o_tex;
    mat[n_mat].clamp = 1.0f;
    memcpy(b.at<qr_light>(b.o_lgt), v.lgt, (size_t)v.hdr->n_lgt * sizeof(qr_light));
    memcpy(b.at<uint32_t>(b.o_tex), v.texels, (size_t)v.hdr->n_texels * 4);
    /* the image-only words of the material records (qr_program.h): written here, from the image's own `tex`, `cmask` and
     * `clamp` and the image's texels, so that whatever sets those three is followed by this */
    struct LutKey { uint32_t cmask, clamp_bits, off; };
    std::vector<LutKey> luts;
    for (int i = 0; i <= n_mat; i++)
    {
        uint32_t lut = 0;
        if (lut_material(mat[i]))
        {
            uint32_t cb; memcpy(&cb, &mat[i].clamp, 4);
            for (const LutKey &k : luts) if (k.cmask == mat[i].cmask && k.clamp_bits == cb) lut = k.off;
            if (lut == 0) { lut = o_lut + (uint32_t)luts.size() * 1024u; luts.push_back(LutKey{mat[i].cmask, cb, lut}); }
        }
        material_colour(mat[i], b.blob.data(), lut);
    }
    for (const LutKey &k : luts)
    {
        float cl; memcpy(&cl, &k.clamp_bits, 4);
        for (uint32_t i = 0; i < 256; i++) b.at<float>(k.off)[i] = channel_colour(i, k.cmask, cl);
    }
}

/* box cull cells (QR_OPF_BOX) for images whose lists are all short: no list of such an image can be flagged as a long
 * hierarchy or get a uniform / shadow grid (each needs a chain of >= QR_LONG_CELLS elements), so only packet walks read its cells. */
void box_setup(Builder &b, const qr_frame &frm, bool assume_short)
{
    double big = 0.0;
    for (int k = 0; k < 3; k++) big = std::max(big, (double)__builtin_fabsf(frm.org[k]));
    for (int i = 0; i < b.n_srf; i++)
        if (b.bs[i].lo[0] <= b.bs[i].hi[0])
            for (int k = 0; k < 3; k++) big = std::max(big, std::max((double)__builtin_fabsf(b.bs[i].lo[k]), (double)__builtin_fabsf(b.bs[i].hi[k])));
    b.box_pad = (float)(2e-6 * big);
    b.big = (float)big;
    b.box_ok = b.kn.cull >= 3 && b.kn.boxes && assume_short;    /* the second attempt: compile_list met a chain of QR_LONG_CELLS elements */
}

/* the records of surface i (filled after the lists they point to exist) */
void surface_record(Builder &b, int i, const qr_surface &q)
{
    const int n_mat = (int)b.v.hdr->n_mat;
    const bool real = is_real(q);
    DSurf d;
    memset(&d, 0, sizeof(d));
    for (int k = 0; k < 3; k++)
    {
        d.pos[k] = q.pos[k]; d.scj[k] = q.scj[k];
        /* an axis without clipping gets an infinite bound: the kernel compares unconditionally */
        d.min[k] = (q.minmax_t & (1u << k)) ? q.min[k] : -__builtin_inff();
        d.max[k] = (q.minmax_t & (1u << (3 + k))) ? q.max[k] : __builtin_inff();
        d.tci[k] = q.tci[k]; d.tcj[k] = q.tcj[k]; d.tck[k] = q.tck[k];
    }
    for (int k = 0; k < 4; k++) d.sci[k] = q.sci[k];
    d.d_eps = q.d_eps; d.t_eps = q.t_eps;
    d.trn = q.trnode != QR_NULL ? b.srf_off(q.trnode) : b.srf_off(b.n_srf);
    d.props0 = q.props[0]; d.props1 = q.props[1];
    uint32_t f = 0;
    f |= q.minmax_t & 63u;
    f |= ((uint32_t)q.conic & 3u) << 6;
    f |= ((uint32_t)q.has_trm & 3u) << 8;
    f |= (q.shift ? 1u : 0u) << 10;
    f |= ((q.axes >> 0) & 3u) << 11; f |= ((q.axes >> 2) & 3u) << 13; f |= ((q.axes >> 4) & 3u) << 15;
    f |= ((q.axes >> 8) & 7u) << 17;
    f |= (real ? ((uint32_t)q.srf_t[0] & 3u) : 0u) << 20;
    f |= ((uint32_t)q.srf_t[1] & 3u) << 22;
    f |= ((uint32_t)q.srf_t[2] & 3u) << 24;
    f |= (q.srf_t[3] < 0 ? 1u : 0u) << 26;
    f |= (q.c_def != 0 ? 1u : 0u) << 28;
    d.flags = f;
    DShade h;
    memset(&h, 0, sizeof(h));
    h.srf = b.srf_off(i);
    h.mat[0] = h.mat[1] = b.o_mat + (uint32_t)n_mat * (uint32_t)sizeof(qr_material);
    if (real)
    {
        d.clip = b.compile_clip(i);
        for (int k = 0; k < 2; k++)
        {
            h.mat[k] = b.o_mat + (uint32_t)q.mat[k] * (uint32_t)sizeof(qr_material);
            h.lgt[k] = b.compile_lights(q.lst[k * 2]);
            h.lst[k] = b.compile_list(q.lst[k * 2 + 1]);
        }
    }
    b.at<DSurf>(b.o_srf)[i] = d;
    b.at<DShade>(b.o_shd)[i] = h;
}

void surface_records(Builder &b)
{
    for (int i = 0; i < b.n_srf; i++) surface_record(b, i, b.v.srf[i]);
    /* index n_srf: the record of no surface at all -- nothing set, no trnode, a tag that is neither a surface nor an array */
    qr_surface none;
    memset(&none, 0, sizeof(none));
    none.trnode = QR_NULL; none.srf_t[3] = QR_TAG_SURFACE_MAX;
    surface_record(b, b.n_srf, none);
}

/* the ray-query list (QR_UPLOAD_RAY_QUERIES): the snapshot's own global list -- never a camera-dependent tile list of the
 * binning pass -- compiled last, like a secondary-ray list, so that every other record of the image keeps its offset.
 * It leaves the render path as it is: no box cells for it (the query kernel's walks do not cull on them; a long list
 * would otherwise restart the build without box cells everywhere) and no say in which kernel instance renders frames. */
uint32_t query_list(Builder &b)
{
    const bool box0 = b.box_ok, long0 = b.any_long;
    b.box_ok = false;
    uint32_t q_off = b.compile_list(b.v.frame->clist);
    b.box_ok = box0; b.any_long = long0;
    if (q_off == 0) q_off = b.alloc(sizeof(CCell), 64);         /* no global list: one END cell, every query misses */
    return q_off;
}

/* header, tail padding, the QrProgram's own fields */
void finish(Builder &b, const Layout &l, const qr_frame &frm, size_t n_tiles, uint32_t q_off, QrProgram &out)
{
    const qr_header &hd = *b.v.hdr;
    const size_t n_waves = out.order.size() / 2;        /* schedule entries: one per wave (fewer than footprints: clear runs) */
    memcpy(b.at<uint32_t>(l.o_ord), out.order.data(), out.order.size() * 4);
    DevHeader &h = *b.at<DevHeader>(0);
    h.fr = frm;
    h.off_shade = b.o_shd; h.off_tiles = l.o_til; h.off_order = l.o_ord; h.n_blocks = (uint32_t)n_waves;
    h.off_query = q_off;
    h.reach = 2.0f * b.big;
    h.off_mat = b.o_mat; h.n_mat = hd.n_mat;
    b.alloc(64, 64);                    /* tail padding: wide scalar loads of the last record stay inside */
    out.off_order = l.o_ord; out.n_sched = (uint32_t)n_waves;
    out.off_query = q_off;
    out.off_srf = b.o_srf; out.off_shade = b.o_shd; out.off_mat = b.o_mat; out.off_lgt = b.o_lgt; out.off_tex = b.o_tex; out.off_tiles = l.o_til;
    out.n_srf = hd.n_srf; out.n_mat = hd.n_mat; out.n_lgt = hd.n_lgt; out.n_tex = hd.n_texels; out.n_tiles = (uint32_t)n_tiles;
    out.off_lists = l.o_ord + (uint32_t)(l.n_sched * 8 + 16);
    b.st.bytes = out.blob.size(); b.st.n_grids = b.n_grids; b.st.n_grid_lists = b.n_grid_lists; b.st.n_dda = b.n_dda;
    b.st.n_pgrids = b.n_pgrids; b.st.n_pgrid_nodes = b.n_pgrid_nodes;
    out.stats = b.st;
    out.has_long_lists = b.any_long;
    out.has_grids = b.n_grids != 0;
    /* box cells and a list the per-lane walkers take (possible only with lowered QR_DDA / QR_GRID thresholds: by default such a
     * list has QR_LONG_CELLS elements and has ended the first attempt already): build again without box cells */
    if ((b.box_ok || b.n_pgrids != 0) && (b.any_long || b.n_grids != 0)) throw Builder::Restart{};
    b.at<DevHeader>(0)->img_flags = b.any_box ? QR_IMG_BOXES : 0u;
    b.at<DevHeader>(0)->img_bytes = (uint32_t)out.blob.size();
}

/* one attempt.  assume_short: take every chain for shorter than QR_LONG_CELLS without measuring them first (the engine's scenes:
 * tens of thousands of tile chains of two or three elements); compile_list throws Restart at the first chain that is not */
int program_build_once(const qr_scene_view &v, const std::vector<qr_elem> &E, const std::vector<int32_t> &T,
                       const qr_frame &frm, const std::vector<BSphere> &bs, const Knobs &kn, QrProgram &out, std::string &err,
                       int sched_blocks, bool verify, uint32_t flags, bool assume_short, bool &restart)
{
    PhaseTimer timer(compile_timing(), "compile", 10);
    const qr_header &hd = *v.hdr;
    out.blob.clear();
    out.frm = frm;
    if ((size_t)frm.tls_row * frm.tls_col != T.size()) { err = "tile grid does not match the tile array"; return QR_ERR_ARG; }
    try
    {
        out.blob.reserve(sizeof(DevHeader) + (size_t)(hd.n_srf + 1) * (sizeof(DSurf) + sizeof(DShade)) + (size_t)(hd.n_mat + 1) * sizeof(qr_material)
                         + (size_t)hd.n_texels * 4 + T.size() * 4 + E.size() * 80 + (size_t)frm.frm_w * frm.frm_h / 8 + 65536);
        std::vector<qr_elem> Eg;
        /* packet shadow pyramids: only in an attempt that takes every list for short -- an image that turns out to need the
         * per-lane instance is built again without them (finish) */
        const bool pgrid_ok = kn.pgrid_min > 0 && assume_short && !(flags & QR_BUILD_NO_PGRID);
        const bool want_grids = wants_shadow_grids(v, E.size(), kn, pgrid_ok);
        if (want_grids) Eg = E;
        timer.tick("pre");
        Builder b(v, want_grids ? Eg : E, bs, kn, out.blob);
        timer.tick("builder");
        if (want_grids) { b.Egrow = &Eg; b.pgrid_ok = pgrid_ok; find_light_users(b, E.size()); }
        const Layout l = fixed_layout(b, T.size(), frm);
        fill_materials(b, l.o_lut);
        timer.tick("fixed");
        box_setup(b, frm, assume_short);
        timer.tick("setup");
        std::vector<uint32_t> tile_off(T.size());
        for (size_t i = 0; i < T.size(); i++) tile_off[i] = b.compile_list(T[i]);
        memcpy(b.at<uint32_t>(l.o_til), tile_off.data(), tile_off.size() * 4);
        timer.tick("tiles");
        surface_records(b);
        timer.tick("surfaces");
        uint32_t q_off = 0;
        if (flags & QR_UPLOAD_RAY_QUERIES) { q_off = query_list(b); timer.tick("query"); }
        /* (scratch kept per thread between frames, like the schedule's own) */
        static thread_local std::vector<uint8_t> tl_tile_heavy;
        std::vector<uint8_t> &tile_heavy = tl_tile_heavy;
        tile_heavy.resize(T.size());
        for (size_t t = 0; t < T.size(); t++) tile_heavy[t] = T[t] != QR_NULL ? b.list_heavy[T[t]] : 0;
        build_schedule(frm, tile_off, tile_heavy, sched_blocks, clear_run_max(), out.order, out.block_first, out.block_row, timer);
        finish(b, l, frm, T.size(), q_off, out);
    }
    catch (const Fail &f) { err = f.msg; return f.rc; }
    catch (const Builder::Restart &) { restart = true; return QR_OK; }
    timer.tick("finish");
    if (!verify) return QR_OK;
    const int vrc = qr_program_verify(out, err);
    timer.tick("verify");
    return vrc;
}

} // namespace

int qr_program_build(const qr_scene_view &v, const std::vector<qr_elem> &E, const std::vector<int32_t> &T,
                     const qr_frame &frm, const std::vector<BSphere> &bs, QrProgram &out, std::string &err, int sched_blocks, bool verify,
                     uint32_t flags)
{
    const Knobs kn;
    bool restart = false;
    int rc = program_build_once(v, E, T, frm, bs, kn, out, err, sched_blocks, verify, flags, true, restart);
    if (restart) rc = program_build_once(v, E, T, frm, bs, kn, out, err, sched_blocks, verify, flags, false, restart);
    return rc;
}

/* host-only entry point: validate + compile a snapshot without a device (used by the CPU test-suite) */
extern "C" int qr_program_stats(const void *blob, uint64_t size, qr_program_info *info)
{
    return qr_program_stats_ex(blob, size, 0u, info);
}

extern "C" int qr_program_stats_ex(const void *blob, uint64_t size, uint32_t flags, qr_program_info *info)
{
    if (blob == nullptr || info == nullptr) return qr_fail(QR_ERR_ARG, "null argument");
    if (flags & QR_UPLOAD_REBIN_TILES) return qr_fail(QR_ERR_UNSUP, "QR_UPLOAD_REBIN_TILES bins on the GPU: not available to a host-only compile");
    if (flags & ~QR_UPLOAD_RAY_QUERIES) return qr_fail(QR_ERR_ARG, "unknown upload flags");
    qr_scene_view v;
    const int rc0 = qr_scene_view_init(&v, blob, size);
    if (rc0 != 0) return qr_fail(QR_ERR_ARG, "malformed snapshot (qr_scene_view_init " + std::to_string(rc0) + ")");
    std::string err;
    PhaseTimer timer(compile_timing(), "compile", 10);
    int rc = qr_snapshot_validate(v, err);
    if (rc != QR_OK) return qr_fail(rc, err);
    timer.tick("validate");
    std::vector<BSphere> bs;
    qr_bound_spheres(v, bs);
    timer.tick("bounds");
    std::vector<qr_elem> E(v.elm, v.elm + v.hdr->n_elm);
    std::vector<int32_t> T(v.tiles, v.tiles + v.hdr->n_tiles);
    timer.tick("copies");
    QrProgram p;
    rc = qr_program_build(v, E, T, *v.frame, bs, p, err, 0, true, flags);
    if (rc != QR_OK) return qr_fail(rc, err);
    if (const char *dump = getenv("QR_DUMP_IMAGE"))        /* debugging aid: the device image as a file */
        if (FILE *f = fopen(dump, "wb")) { fwrite(p.blob.data(), 1, p.blob.size(), f); fclose(f); }
    memset(info, 0, sizeof(*info));
    info->bytes = p.stats.bytes; info->n_lists = p.stats.n_lists; info->n_cells = p.stats.n_cells;
    info->n_dropped = p.stats.n_dropped; info->n_clip_cells = p.stats.n_clip_cells; info->n_sched = p.n_sched;
    info->n_grids = p.stats.n_grids; info->n_grid_lists = p.stats.n_grid_lists; info->n_dda = p.stats.n_dda;
    info->n_pgrids = p.stats.n_pgrids; info->n_pgrid_nodes = p.stats.n_pgrid_nodes;
    return QR_OK;
}
