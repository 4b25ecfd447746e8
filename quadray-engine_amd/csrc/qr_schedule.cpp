/*
 * qr_schedule.cpp - the whole-frame wave schedule: one entry {footprint | heaviness << 30, tile-list offset} per wave
 * footprint.  heavy = the footprint's tile list holds a reflective or non-opaque surface: those waves can spawn recursion,
 * are started first and get issue priority.  A function of the tile lists' offsets and nothing else of the image.
 */
#include "qr_compile.hpp"

namespace qrc {

/*
 * Footprints over an empty tile only have zeros to store: runs of them along a row share ONE wave (schedule head = run
 * length, 1..QR_CLEAR_RUN_MAX: values below 256 are no list offsets).  Half of demo scene 1's 32 400 footprints at 1080p are
 * such; QR_CLEAR_RUN=1 gives every one its own wave again.  add() the empty footprints of a row from left to right, flush()
 * at every footprint that is not empty and at the end of the row.
 */
struct ClearRuns
{
    uint32_t *dst; const uint32_t row; const int cap;
    int run0 = 0, run = 0;                  /* the clear run being collected: first footprint, length */
    ClearRuns(uint32_t *dst_, int by, int cap_) : dst(dst_), row((uint32_t)by << 14), cap(cap_) {}
    void add(int bx) { if (run == 0) run0 = bx; if (++run == cap) flush(); }
    void flush() { if (run) { dst[0] = (uint32_t)run0 | row; dst[1] = (uint32_t)run; dst += 2; run = 0; } }
};

void build_schedule(const qr_frame &frm, const std::vector<uint32_t> &tile_off, const std::vector<uint8_t> &tile_heavy, int sched_blocks,
                    int clear_run, std::vector<uint32_t> &order, std::vector<uint32_t> &block_first, std::vector<uint32_t> &block_row,
                    PhaseTimer &timer)
{
    const int fw = frm.fsaa == 2 ? 4 : 8, fh = frm.fsaa == 0 ? 8 : 4;
    const int nbx = (frm.frm_w + fw - 1) / fw, nby = (frm.frm_h + fh - 1) / fh;
    /* (scratch kept per thread between frames; bound to references once: every use of a thread_local of a shared
     * library is a call) */
    static thread_local std::vector<uint8_t> tl_empty;
    static thread_local std::vector<int> tl_fb, tl_blk_of;
    static thread_local std::vector<std::vector<uint32_t>> tl_part;    /* [3 * k + class] */
    static thread_local std::vector<uint32_t *> tl_cur;                 /* write cursors into part[] */
    std::vector<uint8_t> &empty = tl_empty;
    std::vector<int> &fb = tl_fb, &blk_of = tl_blk_of;
    std::vector<std::vector<uint32_t>> &part = tl_part;
    std::vector<uint32_t *> &cur = tl_cur;
    /* The drop-in path launches block by block (K horizontal blocks of footprint rows) and copies block k back while block
     * k + 1 renders: the entries are collected per block, recursion-capable footprints first, then the others, then the
     * clear runs */
    const int K = sched_blocks > 1 ? std::min(sched_blocks, std::max(1, nby)) : 1;
    fb.resize((size_t)K + 1); blk_of.resize((size_t)nby);
    for (int k = 0; k <= K; k++) fb[k] = (int)((long long)nby * k / K);
    for (int k = 0; k < K; k++) for (int y = fb[k]; y < fb[k + 1]; y++) blk_of[y] = k;
    if (part.size() < (size_t)K * 3) part.resize((size_t)K * 3);
    cur.resize((size_t)K * 3);
    for (int i = 0; i < K * 3; i++)
    {
        const size_t cap = (size_t)(fb[i / 3 + 1] - fb[i / 3]) * nbx * 2;
        if (part[i].size() < cap) part[i].resize(cap);
        cur[i] = part[i].data();
    }
    timer.tick("s-prep");
    /* footprints are enumerated tile by tile (32x8 pixel groups) to keep neighbours together */
    const int gx = 32 / fw, gy = 8 / fh;
    const bool nest = frm.tile_w == 32 && frm.tile_h == 8;      /* group (tx, ty) IS tile (tx, ty) */
    if (nest && gy == 1)
    {
        /* the plain frame: a row of tiles is a row of footprints, gx of them per tile with the tile's list */
        for (int by = 0; by < nby; by++)
        {
            uint32_t **c3 = &cur[(size_t)blk_of[by] * 3];
            uint32_t *p_hv = c3[0], *p_lt = c3[1];
            ClearRuns clear(c3[2], by, clear_run);
            const bool in_rows = by < frm.tls_col;
            const uint32_t *t_off = tile_off.data() + (size_t)by * frm.tls_row;
            const uint8_t *t_hv = tile_heavy.data() + (size_t)by * frm.tls_row;
            for (int tx = 0; tx * gx < nbx; tx++)
            {
                const bool in = in_rows && tx < frm.tls_row;
                const uint32_t head = in ? t_off[tx] : QR_SCHED_PER_LANE;
                const uint32_t hv = in ? t_hv[tx] : 0u;
                const int bx0 = tx * gx, cnt = std::min(gx, nbx - bx0);
                if (head == 0) { for (int i = 0; i < cnt; i++) clear.add(bx0 + i); continue; }
                clear.flush();
                uint32_t *&dst = hv ? p_hv : p_lt;
                const uint32_t ent = ((uint32_t)by << 14) | ((hv & 3u) << 30);
                for (int i = 0; i < cnt; i++) { dst[0] = ent | (uint32_t)(bx0 + i); dst[1] = head; dst += 2; }
            }
            clear.flush();
            c3[0] = p_hv; c3[1] = p_lt; c3[2] = clear.dst;
        }
        timer.tick("s-enum");
    }
    else
    {
        empty.assign((size_t)nbx * nby, 0);
        for (int ty = 0; ty * gy < nby; ty++)
            for (int tx = 0; tx * gx < nbx; tx++)
            {
                int g_hv = 0; uint32_t g_head = QR_SCHED_PER_LANE;
                if (nest && tx < frm.tls_row && ty < frm.tls_col)
                {
                    const size_t t = (size_t)ty * frm.tls_row + tx;
                    g_hv = tile_heavy[t]; g_head = tile_off[t];
                }
                for (int j = 0; j < gy; j++)
                {
                    const int by = ty * gy + j;
                    if (by >= nby) break;
                    uint32_t **row3 = &cur[(size_t)blk_of[by] * 3];
                    if (nest && g_head == 0)
                    {
                        for (int i = 0; i < gx && tx * gx + i < nbx; i++) empty[(size_t)by * nbx + tx * gx + i] = 1;
                        continue;
                    }
                    for (int i = 0; i < gx; i++)
                    {
                        const int bx = tx * gx + i;
                        if (bx >= nbx) break;
                        int hv = g_hv; uint32_t head = g_head;
                        if (!nest)
                        {
                            const int x0 = bx * fw, y0 = by * fh;
                            const int x1 = std::min(x0 + fw - 1, frm.frm_w - 1), y1 = std::min(y0 + fh - 1, frm.frm_h - 1);
                            const int tlx = x0 / frm.tile_w, tly = y0 / frm.tile_h;
                            hv = tile_heavy[(size_t)tly * frm.tls_row + tlx];
                            head = QR_SCHED_PER_LANE;
                            if (tlx == x1 / frm.tile_w && tly == y1 / frm.tile_h) head = tile_off[(size_t)tly * frm.tls_row + tlx];
                            else for (int yy = tly; yy <= y1 / frm.tile_h; yy++) for (int xx = tlx; xx <= x1 / frm.tile_w; xx++) hv |= tile_heavy[(size_t)yy * frm.tls_row + xx];
                        }
                        if (head == 0) { empty[(size_t)by * nbx + bx] = 1; continue; }
                        const uint32_t ent = (uint32_t)bx | ((uint32_t)by << 14) | ((uint32_t)(hv & 3) << 30);
                        uint32_t *&dst = row3[hv ? 0 : 1];
                        dst[0] = ent; dst[1] = head; dst += 2;
                    }
                }
            }
        timer.tick("s-enum");
        for (int by = 0; by < nby; by++)
        {
            ClearRuns clear(cur[(size_t)blk_of[by] * 3 + 2], by, clear_run);
            const uint8_t *em = empty.data() + (size_t)by * nbx;
            for (int bx = 0; bx < nbx; bx++) if (em[bx]) clear.add(bx); else clear.flush();
            clear.flush();
            cur[(size_t)blk_of[by] * 3 + 2] = clear.dst;
        }
    }
    timer.tick("s-clear");
    size_t total = 0;
    for (int i = 0; i < K * 3; i++) total += (size_t)(cur[i] - part[i].data());
    if (total > (size_t)nbx * nby * 2 || (total & 1)) throw Fail{QR_ERR_ARG, "schedule size mismatch"};
    order.resize(total);
    block_first.clear(); block_row.clear();
    size_t pos = 0;
    for (int k = 0; k < K; k++)
    {
        if (sched_blocks > 1)
        {
            block_first.push_back((uint32_t)(pos / 2));
            block_row.push_back((uint32_t)std::min(fb[k] * fh, frm.frm_h));
        }
        for (int c = 0; c < 3; c++)
        {
            const size_t cnt = (size_t)(cur[(size_t)k * 3 + c] - part[(size_t)k * 3 + c].data());
            if (cnt) memcpy(order.data() + pos, part[(size_t)k * 3 + c].data(), cnt * 4);
            pos += cnt;
        }
    }
    if (sched_blocks > 1)
    {
        block_first.push_back((uint32_t)(pos / 2));
        block_row.push_back((uint32_t)frm.frm_h);
    }
    timer.tick("schedule");
}

} // namespace qrc
