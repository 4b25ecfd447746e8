/*
 * qr_verify.cpp - qr_program_verify: walks the finished image of qr_program.h once more and checks every offset the kernel
 * will follow.  Shares no code with the builder but the records' layout and the material colour words.
 */
#include "qr_compile.hpp"

using namespace qrc;

int qr_program_verify(const QrProgram &p, std::string &err)
{
    const std::vector<uint8_t> &b = p.blob;
    const size_t N = b.size();
    auto bad = [&](const char *m) { err = std::string("compiled scene fails verification: ") + m; return QR_ERR_ARG; };
    if (N < sizeof(DevHeader) + 64) return bad("too small");
    const size_t limit = N - 64;        /* records end before the tail padding */
    auto in_arr = [&](uint32_t off, uint32_t base, uint32_t n, size_t sz) {
        return off >= base && (off - base) % sz == 0 && (off - base) / sz <= n && (size_t)off + sz <= limit;
    };
    /* per 32-byte slot of the image: 1 = a list starts here (already checked), 2 = a cell starts here */
    static thread_local std::vector<uint8_t> slot;
    slot.assign(N / 32 + 1, 0);
    /* a list program: cells inside the list area, END-terminated, array ends on cell boundaries inside the run */
    auto check_list = [&](uint32_t off) -> const char * {
        if (off == 0) return nullptr;
        if (off & 8u) return "list offset carries unknown flag bits";
        const bool world = (off & QR_LISTF_WORLD) != 0, dda = (off & QR_LISTF_DDA) != 0, div_ok = (off & QR_LISTF_DIV) != 0;
        off &= ~31u;
        if (off < p.off_lists || (size_t)off + 32 > limit) return "list offset out of range";
        if (slot[off / 32] & 1) return (((slot[off / 32] & 4) != 0) == world && ((slot[off / 32] & 8) != 0) == dda) ? nullptr : "list referenced with different flags";
        slot[off / 32] |= (world ? 5 : 1) | (dda ? 8 : 0);
        uint32_t o = off, end_cell = 0;
        for (;;)
        {
            if ((size_t)o + 32 > limit) return "list runs off the image";
            const CCell *c = (const CCell *)(b.data() + o);
            slot[o / 32] |= 2;
            if (c->op == 0) { end_cell = o; break; }
            o += (c->op & QR_OPT_BV) ? 64 : 32;
        }
        if (world && div_ok)
        {
            /* the length word in front of the program: what walk_pool cuts ranges by */
            uint32_t lw; memcpy(&lw, b.data() + off - 4u, 4);
            bool any_bv = false;
            for (uint32_t q = off; q < end_cell; ) { const CCell *cq = (const CCell *)(b.data() + q); const bool bvq = (cq->op & QR_OPT_BV) != 0; any_bv = any_bv || bvq; q += bvq ? 64 : 32; }
            if ((lw & ~31u) != end_cell - off || (lw & 30u) != 0 || ((lw & 1u) != 0) != !any_bv) return "list length word";
        }
        for (o = off; o < end_cell; )
        {
            const CCell *c = (const CCell *)(b.data() + o);
            const uint32_t t = c->op & QR_OPT_MASK;
            if (t == 0 || (t & (t - 1)) != 0) return "bad opcode";
            if (!in_arr(c->srf, p.off_srf, p.n_srf, sizeof(DSurf)) || c->srf == p.off_srf + p.n_srf * (uint32_t)sizeof(DSurf)) return "cell surface offset out of range";
            if (t == QR_OPT_BV && (c->end <= o + 32 || c->end > end_cell || (c->end & 31) || !(slot[c->end / 32] & 2)))
                return "array end outside its list";
            if (t == QR_OPT_BV)
            {
                const uint32_t mid = ((const CBvExt *)(b.data() + o + 32))->mid;
                if (mid != 0 && (mid <= o + 64 || mid >= c->end || (mid & 31) || !(slot[mid / 32] & 2))) return "array hand-over boundary outside the array";
            }
            if ((c->op & QR_OPF_CACHED) && (c->op & QR_OPF_OWN)) return "bad transform mode";
            /* the cull run tells an array with a sphere by QR_OPF_CULL | QR_OPT_BV under a mask that may hold the box bit (qr_walk.hpp) */
            if ((c->op & QR_OPF_BOX) && !(t & QR_OPT_SOLVER)) return "box cull bit on a cell that is no solver cell";
            if (world && (t == QR_OPT_TRNODE || (c->op & QR_OPF_LOCAL))) return "transform in a list flagged world-space";
            if ((c->op & QR_OPF_CULL) && !(t & (QR_OPT_SOLVER | QR_OPT_BV))) return "cull flag on a cell without solver or volume";
            if (c->op & QR_OPF_BOX)
            {
                if (!(c->op & QR_OPF_CULL) || !(t & QR_OPT_SOLVER) || dda) return "box flag on the wrong kind of cell";
                if (!(c->r2 <= c->cy) || !(c->r2x <= c->cz) || !(c->cx <= c->r) || !(c->r2 > -1e30f) || !(c->r < 1e30f)) return "box cull cell: bad box";
            }
            if ((c->op & QR_OPF_SPHBV) && (t != QR_OPT_BV || !(c->op & QR_OPF_CULL) || (c->op & QR_OPF_LOCAL))) return "sphere-volume flag on the wrong kind of cell";
            if ((c->op & QR_OPF_KX) && (c->op & QR_OPF_KY)) return "bad axis k";
            if ((c->op & QR_OPF_IX) && (c->op & QR_OPF_IY)) return "bad axis i";
            o += (t == QR_OPT_BV) ? 64 : 32;
        }
        if (dda)
        {
            /* the uniform grid in front of the program: tables inside the image, every ref a solver cell of THIS list */
            if (!world || off < p.off_lists + sizeof(CDda)) return "grid record in front of a list that cannot have one";
            const CDda *g = (const CDda *)(b.data() + off - sizeof(CDda));
            const uint32_t nx = g->dims & 255u, ny = (g->dims >> 8) & 255u, nz = (g->dims >> 16) & 255u;
            if ((g->dims >> 24) || nx < 1 || ny < 1 || nz < 1 || nx > QR_GRID_MAX || ny > QR_GRID_MAX || nz > QR_GRID_MAX) return "grid dimensions";
            const size_t nc = (size_t)nx * ny * nz;
            if ((g->cells & 3) || g->cells < p.off_lists || (size_t)g->cells + (nc + 1) * 4 > limit) return "grid cell table";
            if ((g->refs & 31) || g->refs < p.off_lists || (size_t)g->refs + ((size_t)g->n_refs + 2) * sizeof(CCell) > limit) return "grid refs";
            const uint32_t *cs = (const uint32_t *)(b.data() + g->cells);
            if (cs[0] != g->n_out || cs[nc] != g->n_refs) return "grid cell table ends";
            for (size_t q = 0; q < nc; q++) if (cs[q] > cs[q + 1]) return "grid cell table not monotone";
            for (int k = 0; k < 3; k++) if (!(g->size[k] > 0.0f) || !(g->inv[k] > 0.0f) || !(g->size[k] < 1e30f) || !(g->inv[k] < 1e30f)) return "grid cell size";
            const CCell *rf = (const CCell *)(b.data() + g->refs);
            for (uint32_t q = 0; q < g->n_refs; q++)
            {
                const uint32_t t = rf[q].op & QR_OPT_MASK;
                if (t == 0 || (t & (t - 1)) != 0 || !(t & QR_OPT_SOLVER) || (rf[q].op & (QR_OPF_LOCAL | QR_OPF_CLIP))) return "grid ref opcode";
                if (!in_arr(rf[q].srf, p.off_srf, p.n_srf, sizeof(DSurf)) || rf[q].srf == p.off_srf + p.n_srf * (uint32_t)sizeof(DSurf)) return "grid ref surface";
                uint32_t pos; memcpy(&pos, &rf[q].r2x, 4);
                if (pos < off || pos >= end_cell || (pos & 31) || !(slot[pos / 32] & 2)) return "grid ref position";
                const CCell *oc = (const CCell *)(b.data() + pos);
                if (oc->op != rf[q].op || oc->srf != rf[q].srf) return "grid ref is not a copy of its cell";
            }
        }
        return nullptr;
    };
    static const bool vt = getenv("QR_VERIFY_TIMING") != nullptr;
    PhaseTimer timer(vt, "verify", 8);
    const DevHeader *h = (const DevHeader *)b.data();
    if (h->off_tiles != p.off_tiles || h->off_order != p.off_order || h->off_shade != p.off_shade || h->off_query != p.off_query)
        return bad("header offsets");
    if (const char *m = check_list(p.off_query)) return bad(m);        /* the ray-query list (0: none) */
    if ((size_t)p.off_tiles + (size_t)p.n_tiles * 4 > limit) return bad("tile array");
    const uint32_t *tl = (const uint32_t *)(b.data() + p.off_tiles);
    /* neighbouring tiles mostly share one program (lists are stored once per content): a head equal to the one just checked
     * needs no second look */
    { uint32_t prev = 0; for (uint32_t i = 0; i < p.n_tiles; i++) { if (tl[i] == prev) continue; if (const char *m = check_list(tl[i])) return bad(m); prev = tl[i]; } }
    timer.tick("tiles");
    if ((size_t)p.off_order + (size_t)p.n_sched * 8 > limit) return bad("schedule");
    const uint32_t *ord = (const uint32_t *)(b.data() + p.off_order);
    const int fw = p.frm.fsaa == 2 ? 4 : 8, fh = p.frm.fsaa == 0 ? 8 : 4;
    const uint32_t max_bx = (uint32_t)((p.frm.frm_w + fw - 1) / fw), max_by = (uint32_t)((p.frm.frm_h + fh - 1) / fh);
    uint32_t prev_hd = 0;
    for (uint32_t i = 0; i < p.n_sched; i++)
    {
        const uint32_t e = ord[2 * i], hd = ord[2 * i + 1];
        if ((e & 0x3FFFu) >= max_bx || ((e >> 14) & 0x3FFFu) >= max_by) return bad("schedule footprint outside the frame");
        if (hd == prev_hd && hd >= 256u) continue;
        if (hd < 256u)
        {
            /* a run of hd empty footprints along the row (0: one) */
            if (hd > QR_CLEAR_RUN_MAX || ((int)(e & 0x3FFFu) + (int)(hd ? hd : 1u) - 1) * fw >= p.frm.frm_w) return bad("clear run leaves the frame");
        }
        else if (hd != QR_SCHED_PER_LANE) { if (const char *m = check_list(hd)) return bad(m); prev_hd = hd; }
    }
    timer.tick("sched");
    for (uint32_t i = 0; i <= p.n_srf; i++)
    {
        const DSurf *d = (const DSurf *)(b.data() + p.off_srf) + i;
        const DShade *s = (const DShade *)(b.data() + p.off_shade) + i;
        if (!in_arr(d->trn, p.off_srf, p.n_srf, sizeof(DSurf))) return bad("trnode offset");
        if (d->clip != 0)
        {
            if ((d->clip & 31) || d->clip < p.off_lists) return bad("clipper program offset");
            bool in_group = false;
            for (uint32_t o = d->clip;; o += (uint32_t)sizeof(CClip))
            {
                if ((size_t)o + sizeof(CClip) > limit) return bad("clipper program runs off the image");
                const CClip *c = (const CClip *)(b.data() + o);
                if (c->op == 0) { if (in_group) return bad("clipper program ends inside a trnode group"); break; }
                const uint32_t t = c->op & QR_CLT_MASK;
                if (t == 0 || (t & (t - 1)) != 0) return bad("bad clipper opcode");
                if (t != QR_CLT_ENTER && t != QR_CLT_LEAVE && (!in_arr(c->srf, p.off_srf, p.n_srf, sizeof(DSurf)) || c->srf == p.off_srf + p.n_srf * (uint32_t)sizeof(DSurf))) return bad("clipper surface offset");
                if ((c->op & QR_CLF_KX) && (c->op & QR_CLF_KY)) return bad("bad clipper axis");
                if ((c->op & QR_CLF_CACHED) && (c->op & QR_CLF_OWN)) return bad("bad clipper transform mode");
                /* the cached trnode space: opened by a trnode cell, closed behind the cell flagged QR_CLF_LASTC; cached cells
                 * only inside, fast plane cells with one axis mask and a consistent sign */
                if (t == QR_CLT_TRNODE || t == QR_CLT_TRSAME) in_group = true;
                else if ((c->op & QR_CLF_CACHED) && !in_group) return bad("cached clipper cell outside a trnode group");
                else if (!(c->op & QR_CLF_CACHED) && in_group && t != QR_CLT_ENTER && t != QR_CLT_LEAVE) return bad("world-space clipper cell inside a trnode group");
                if (c->op & QR_CLF_LASTC) { if (!in_group) return bad("group end flag outside a group"); in_group = false; }
                if (c->op & QR_CLF_FASTPL)
                {
                    const uint32_t ones = (c->mx == 0xFFFFFFFFu) + (c->my == 0xFFFFFFFFu) + (c->mz == 0xFFFFFFFFu);
                    const uint32_t zeros = (c->mx == 0u) + (c->my == 0u) + (c->mz == 0u);
                    if (t != QR_CLT_PLANE || (c->op & QR_CLF_OWN) || ones != 1 || zeros != 2) return bad("fast plane cell");
                    if (c->sgn != ((c->op & QR_CLF_SGNK) ? 0x80000000u : 0u)) return bad("fast plane cell sign");
                }
            }
        }
        for (int k = 0; k < 2; k++)
        {
            if (!in_arr(s->mat[k], p.off_mat, p.n_mat, sizeof(qr_material))) return bad("material offset");
            if (const char *m = check_list(s->lst[k])) return bad(m);
            if (s->lgt[k] != 0)
            {
                if ((s->lgt[k] & 7) || s->lgt[k] < p.off_lists) return bad("light list offset");
                for (uint32_t o = s->lgt[k];; o += 8)
                {
                    if ((size_t)o + 8 > limit) return bad("light list runs off the image");
                    const CLight *l = (const CLight *)(b.data() + o);
                    const uint32_t lo = l->lgt & ~QR_CLIGHT_LAST;
                    if (!in_arr(lo, p.off_lgt, p.n_lgt, sizeof(qr_light)) || lo == p.off_lgt + p.n_lgt * (uint32_t)sizeof(qr_light)) return bad("light offset");
                    if (l->shadow & QR_LISTF_GRID)
                    {
                        /* shadow lists by hit position: record, table and every list in it */
                        const uint32_t go = l->shadow & ~31u;
                        if ((l->shadow & 31u) != QR_LISTF_GRID || go < p.off_lists || (size_t)go + sizeof(CGrid) > limit) return bad("shadow grid offset");
                        const CGrid *g = (const CGrid *)(b.data() + go);
                        if (g->nx < 1 || g->nx > QR_GRID_MAX || g->ny < 1 || g->ny > QR_GRID_MAX) return bad("shadow grid size");
                        const uint32_t ca = g->comps & 3u, cb = (g->comps >> 2) & 3u;
                        const bool pyr = (g->comps & QR_GRIDC_PYR) != 0;
                        const uint32_t L = QR_GRIDC_LEVELS(g->comps);
                        if ((g->comps & ~(15u | (pyr ? QR_GRIDC_PYR | (7u << 8) : 0u))) || ca > 2 || cb > 2 || ca == cb) return bad("shadow grid components");
                        /* a pyramid: 2^L x 2^L cells, in an image of the packet instance alone */
                        if (pyr && (L < 1 || L > QR_PGRID_LEVELS_MAX || g->nx != (1u << L) || g->ny != g->nx || p.has_grids || p.has_long_lists))
                            return bad("shadow pyramid record");
                        if (!pyr && !p.has_grids) return bad("shadow grid in an image that reports none");
                        const size_t n_words = pyr ? QR_PGRID_LEVEL_OFF(g->nx, L) + 1u : (size_t)g->nx * g->ny;
                        if ((g->table & 3) || g->table < p.off_lists || (size_t)g->table + n_words * 4 > limit) return bad("shadow grid table");
                        const uint32_t *tb = (const uint32_t *)(b.data() + g->table);
                        for (size_t q = 0; q < n_words; q++) if (const char *m = check_list(tb[q])) return bad(m);
                        if (pyr)
                        {
                            /* every node's program a sub-sequence of its parent's: the same cells (type, surface) in the same order */
                            auto next_cell = [&](uint32_t &o) { const CCell *c = (const CCell *)(b.data() + o); o += (c->op & QR_OPT_BV) ? 64 : 32; return c; };
                            auto sub_seq = [&](uint32_t child, uint32_t parent) {
                                if (child == 0 || child == parent) return true;
                                if (parent == 0) return false;
                                uint32_t oc = child & ~31u, op = parent & ~31u;
                                for (;;)
                                {
                                    const CCell *c = next_cell(oc);
                                    if (c->op == 0) return true;
                                    for (;;)
                                    {
                                        const CCell *q = next_cell(op);
                                        if (q->op == 0) return false;
                                        if ((q->op & QR_OPT_MASK) == (c->op & QR_OPT_MASK) && q->srf == c->srf) break;
                                    }
                                }
                            };
                            if (tb[n_words - 1] == 0) return bad("shadow pyramid without a top program");
                            for (uint32_t l = 0; l < L; l++)
                            {
                                const uint32_t n = g->nx >> l, np = n >> 1;
                                const uint32_t *row = tb + QR_PGRID_LEVEL_OFF(g->nx, l), *par = tb + QR_PGRID_LEVEL_OFF(g->nx, l + 1);
                                for (uint32_t j = 0; j < n; j++) for (uint32_t i = 0; i < n; i++)
                                    if (!sub_seq(row[j * n + i], par[(j >> 1) * np + (i >> 1)])) return bad("shadow pyramid node holds what its parent does not");
                            }
                        }
                    }
                    else if (const char *m = check_list(l->shadow)) return bad(m);
                    if (l->lgt & QR_CLIGHT_LAST) break;
                }
            }
        }
        if (s->srf != p.off_srf + i * (uint32_t)sizeof(DSurf)) return bad("shade record surface offset");
    }
    timer.tick("surfaces");
    for (uint32_t i = 0; i <= p.n_mat; i++)
    {
        const qr_material *m = (const qr_material *)(b.data() + p.off_mat) + i;
        const uint64_t n = (uint64_t)(m->xmask + 1) * (m->ymask + 1);
        if ((uint32_t)m->tex < p.off_tex || ((uint32_t)m->tex & 3) || (uint64_t)(uint32_t)m->tex + n * 4 > (uint64_t)p.off_tex + ((uint64_t)p.n_tex + 1) * 4)
            return bad("texture offset");
        /* the finished colour (QR_MATF_COLOUR) exactly for one-texel textures, and equal to what the record's texel, mask and
         * clamp give now */
        qr_material want = *m;
        const bool lut_ok = (m->xmask != 0 || m->ymask != 0) && m->cmask <= 0xFFu;
        const uint32_t lut = (uint32_t)m->pad[QR_MATX_LUT];
        if (lut_ok)
        {
            /* the table: inside the fixed sections, and every entry what the record's mask and clamp give */
            if (lut == 0 || (lut & 63) || lut < p.off_tex || (uint64_t)lut + 1024 > p.off_lists) return bad("material colour table offset");
            const float *t = (const float *)(b.data() + lut);
            for (uint32_t k = 0; k < 256; k++)
            {
                const float w = channel_colour(k, m->cmask, m->clamp);
                if (memcmp(&w, &t[k], 4) != 0) return bad("material colour table");
            }
        }
        material_colour(want, b.data(), lut_ok ? lut : 0u);
        if (memcmp(want.pad, m->pad, sizeof(want.pad)) != 0) return bad("material colour words");
    }
    const DevHeader *dh = (const DevHeader *)b.data();
    if (dh->off_mat != p.off_mat || dh->n_mat != p.n_mat) return bad("header material table");
    return QR_OK;
}
