/*
 * compile_digest.cpp - host-only: one line per compile of a snapshot, with a 64-bit hash over everything the scene compiler
 * hands the launch code (the device image, the wave schedule, the block tables).  Two builds of the compiler that print the
 * same lines for the same snapshots and environment compile the same images: the check a refactor of csrc/qr_compile*.cpp
 * and its neighbours is held to (profiles/r27_compile_split.txt).  Uses the declarations of qr_internal.h only.
 *
 *   make -C quadray-engine_amd/csrc digest          (g++, AddressSanitizer + UBSan; no GPU, no HIP)
 *   tools/compile_digest [--no-retile] a.qrs b.qrs ...      uncompressed snapshots
 *
 * Per snapshot: the snapshot as it is; re-tiled in memory (tile_w = 8, four tiles where one was, each with the wide tile's
 * list: a valid tiling that reaches the schedule's non-nested path, which otherwise only a GPU rebin reaches); and, where it
 * has a global list, the output of qr_snapshot_build_lists -- hashed, then compiled the same ways.
 */
#include "qr_internal.h"

#include <cstdio>
#include <cstring>

static uint64_t fnv(uint64_t h, const void *p, size_t n)
{
    const uint8_t *b = (const uint8_t *)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}
template <typename T> static uint64_t fnv_vec(uint64_t h, const std::vector<T> &v)
{
    const uint64_t n = v.size();
    h = fnv(h, &n, sizeof(n));
    return v.empty() ? h : fnv(h, v.data(), v.size() * sizeof(T));
}

static void builds(const char *name, const char *what, const qr_scene_view &v, const std::vector<qr_elem> &E,
                   const std::vector<int32_t> &T, const qr_frame &frm, const std::vector<BSphere> &bs)
{
    const int blocks[3] = { 0, 1, 4 };
    for (int sb : blocks)
        for (uint32_t flags : { 0u, (uint32_t)QR_UPLOAD_RAY_QUERIES })
        {
            QrProgram p;
            std::string err;
            const int rc = qr_program_build(v, E, T, frm, bs, p, err, sb, true, flags);
            if (rc != QR_OK) { printf("%s %s sb=%d q=%d rc=%d %s\n", name, what, sb, flags ? 1 : 0, rc, err.c_str()); continue; }
            uint64_t h = 1469598103934665603ull;
            h = fnv_vec(h, p.blob); h = fnv_vec(h, p.order); h = fnv_vec(h, p.block_first); h = fnv_vec(h, p.block_row);
            const QrProgramStats &s = p.stats;
            printf("%s %s sb=%d q=%d %016llx n_sched=%u bytes=%llu lists=%u cells=%u dropped=%u clip=%u grids=%u grid_lists=%u dda=%u long=%d has_grids=%d\n",
                   name, what, sb, flags ? 1 : 0, (unsigned long long)h, p.n_sched, (unsigned long long)s.bytes, s.n_lists, s.n_cells,
                   s.n_dropped, s.n_clip_cells, s.n_grids, s.n_grid_lists, s.n_dda, (int)p.has_long_lists, (int)p.has_grids);
        }
}

/* validate, bound, compile: as it is and re-tiled.  false: the snapshot was rejected (the line says why) */
static bool snapshot(const char *name, const char *what, const std::vector<uint8_t> &blob, bool retile, qr_scene_view &v)
{
    const int rc0 = qr_scene_view_init(&v, blob.data(), blob.size());
    if (rc0 != 0) { printf("%s %s view_init %d\n", name, what, rc0); return false; }
    std::string err;
    const int rc = qr_snapshot_validate(v, err);
    if (rc != QR_OK) { printf("%s %s validate rc=%d %s\n", name, what, rc, err.c_str()); return false; }
    std::vector<BSphere> bs;
    qr_bound_spheres(v, bs);
    std::vector<qr_elem> E(v.elm, v.elm + v.hdr->n_elm);
    std::vector<int32_t> T(v.tiles, v.tiles + v.hdr->n_tiles);
    builds(name, what, v, E, T, *v.frame, bs);
    if (retile && v.frame->tile_w == 32)
    {
        qr_frame f = *v.frame;
        f.tile_w = 8; f.tls_row *= 4;
        std::vector<int32_t> T4((size_t)f.tls_row * f.tls_col);
        for (int ty = 0; ty < f.tls_col; ty++)
            for (int tx = 0; tx < f.tls_row; tx++) T4[(size_t)ty * f.tls_row + tx] = T[(size_t)ty * v.frame->tls_row + tx / 4];
        builds(name, (std::string(what) + "-tile8").c_str(), v, E, T4, f, bs);
    }
    return true;
}

int main(int argc, char **argv)
{
    bool retile = true;
    for (int a = 1; a < argc; a++)
    {
        if (strcmp(argv[a], "--no-retile") == 0) { retile = false; continue; }
        FILE *f = fopen(argv[a], "rb");
        if (f == nullptr) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> blob;
        uint8_t buf[65536];
        for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0; ) blob.insert(blob.end(), buf, buf + n);
        fclose(f);
        const char *name = strrchr(argv[a], '/') ? strrchr(argv[a], '/') + 1 : argv[a];
        qr_scene_view v;
        if (!snapshot(name, "raw", blob, retile, v) || v.frame->clist == QR_NULL) continue;
        std::vector<uint8_t> built;
        std::string err;
        const int rc = qr_snapshot_build_lists(v, built, err);
        if (rc != QR_OK) { printf("%s build_lists rc=%d %s\n", name, rc, err.c_str()); continue; }
        printf("%s build_lists %016llx bytes=%zu\n", name, (unsigned long long)fnv_vec(1469598103934665603ull, built), built.size());
        qr_scene_view vb;
        snapshot(name, "built", built, retile, vb);
    }
    return 0;
}
