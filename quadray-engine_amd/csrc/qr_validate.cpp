/*
 * qr_validate.cpp - what the scene compiler checks and measures before it compiles a snapshot (include/qr_scene.h):
 *
 *   qr_snapshot_validate   every index, list and tag the compiler follows (a malformed snapshot is rejected
 *                          here and can never become an out-of-bounds device access)
 *   qr_bound_spheres       conservative world-space bounds of every surface (qr_bounds.hpp)
 */
#include "qr_compile.hpp"
#include "qr_bounds.hpp"

using namespace qrc;

int qr_snapshot_validate(const qr_scene_view &v, std::string &err)
{
    const qr_frame &fr = *v.frame;
    auto bad = [&](int rc, const char *m) { err = m; return rc; };
    if (fr.fsaa < 0 || fr.fsaa > 2) return bad(QR_ERR_UNSUP, "unsupported fsaa");
    if (fr.frm_w <= 0 || fr.frm_h <= 0 || fr.tile_w <= 0 || fr.tile_h <= 0) return bad(QR_ERR_ARG, "bad frame parameters");
    if (fr.depth < 0) return bad(QR_ERR_ARG, "negative recursion depth");
    if (fr.tls_row <= 0 || fr.tls_col <= 0) return bad(QR_ERR_ARG, "tile grid must be positive");
    if ((int64_t)fr.tls_row * fr.tile_w < fr.frm_w || (int64_t)fr.tls_col * fr.tile_h < fr.frm_h)
        return bad(QR_ERR_ARG, "tile grid does not cover the frame");
    if (fr.thnum < 0 || fr.index < 0 || (fr.thnum > 0 && fr.index >= fr.thnum) || (fr.thnum == 0 && fr.index != 0))
        return bad(QR_ERR_ARG, "bad index/thnum");

    const int n_srf = (int)v.hdr->n_srf, n_mat = (int)v.hdr->n_mat, n_lgt = (int)v.hdr->n_lgt;
    const int n_elm = (int)v.hdr->n_elm, n_tex = (int)v.hdr->n_texels;
    auto ok_elm = [&](int i) { return i == QR_NULL || (i >= 0 && i < n_elm); };
    auto ok_srf = [&](int i) { return i >= 0 && i < n_srf; };
    for (int i = 0; i < n_elm; i++)
        if (!ok_elm(v.elm[i].next)) return bad(QR_ERR_ARG, "element next out of range");
    for (uint32_t i = 0; i < v.hdr->n_tiles; i++)
        if (!ok_elm(v.tiles[i])) return bad(QR_ERR_ARG, "tile head out of range");
    if (!ok_elm(fr.clist)) return bad(QR_ERR_ARG, "clist out of range");
    for (int i = 0; i < n_mat; i++)
    {
        const qr_material &m = v.mat[i];
        const uint64_t n = (uint64_t)(m.xmask + 1) * (m.ymask + 1);
        if (m.tex < 0 || (uint64_t)m.tex + n > (uint64_t)n_tex) return bad(QR_ERR_ARG, "texture out of range");
        if (m.t_map[0] < 0 || m.t_map[0] > 1 || m.t_map[1] < 0 || m.t_map[1] > 1) return bad(QR_ERR_ARG, "bad t_map");
        if ((m.xmask & (m.xmask + 1)) != 0 || (m.ymask & (m.ymask + 1)) != 0) return bad(QR_ERR_ARG, "texture size not a power of two");
        if (((uint64_t)m.ymask << (m.yshft & 31)) + m.xmask >= n) return bad(QR_ERR_ARG, "texture addressing exceeds texture");
    }
    /* every list is walked once per kind with a step bound (cycle check) */
    std::vector<uint8_t> checked((size_t)n_elm + 1, 0);
    auto check_list = [&](int head, int kind) -> const char * {
        /* kind 0 surfaces, 1 clippers, 2 lights */
        if (head == QR_NULL) return nullptr;
        if (checked[head] & (1u << kind)) return nullptr;
        checked[head] |= (uint8_t)(1u << kind);
        int cnt = 0;
        for (int e = head; e != QR_NULL; e = v.elm[e].next)
        {
            if (++cnt > n_elm) return "cyclic list";
            const qr_elem &el = v.elm[e];
            if (kind == 2)
            {
                if (el.simd < 0 || el.simd >= n_lgt) return "light index out of range";
                if (!ok_elm(el.data)) return "shadow list out of range";
            }
            else if (kind == 0)
            {
                if (!ok_srf(el.simd)) return "surface index out of range";
                if (el.data != QR_NULL && !ok_elm(el.data)) return "array last element out of range";
            }
            else if (el.simd != QR_NULL)
            {
                if (!ok_srf(el.simd)) return "clipper index out of range";
                if (v.srf[el.simd].srf_t[3] < 0 && !ok_elm(el.data)) return "clip trnode last out of range";
            }
        }
        return nullptr;
    };
    for (uint32_t i = 0; i < v.hdr->n_tiles; i++)
        if (const char *m = check_list(v.tiles[i], 0)) return bad(QR_ERR_ARG, m);
    if (const char *m = check_list(fr.clist, 0)) return bad(QR_ERR_ARG, m);
    for (int i = 0; i < n_srf; i++)
    {
        const qr_surface &s = v.srf[i];
        if (s.trnode != QR_NULL && !ok_srf(s.trnode)) return bad(QR_ERR_ARG, "trnode out of range");
        const bool real = is_real(s);
        if (s.has_trm != 0 && s.trnode == QR_NULL && real) return bad(QR_ERR_ARG, "transformed surface without trnode");
        for (int k = 0; k < 3; k++)
            if (((s.axes >> (2 * k)) & 3) > 2) return bad(QR_ERR_ARG, "bad axis map");
        if ((s.conic & ~3) || (s.has_trm & ~3) || (s.srf_t[0] & ~3) || (s.srf_t[1] & ~3) || (s.srf_t[2] & ~3))
            return bad(QR_ERR_ARG, "surface tag fields out of range");
        if (!real) continue;
        if (s.smask != 0x80000000u) return bad(QR_ERR_ARG, "surface smask is not the fp32 sign bit");
        if ((s.shift != 0) != (s.has_trm != 0))
            return bad(QR_ERR_UNSUP, "surface with trnode shift but no transform flags (or the reverse)");
        for (int k = 0; k < 2; k++)
            if (s.mat[k] < 0 || s.mat[k] >= n_mat) return bad(QR_ERR_ARG, "material index out of range");
        if (!ok_elm(s.clip) || !ok_elm(s.lst[0]) || !ok_elm(s.lst[1]) || !ok_elm(s.lst[2]) || !ok_elm(s.lst[3]))
            return bad(QR_ERR_ARG, "surface list head out of range");
        if (const char *m = check_list(s.clip, 1)) return bad(QR_ERR_ARG, m);
        if (const char *m = check_list(s.lst[0], 2)) return bad(QR_ERR_ARG, m);
        if (const char *m = check_list(s.lst[2], 2)) return bad(QR_ERR_ARG, m);
        if (const char *m = check_list(s.lst[1], 0)) return bad(QR_ERR_ARG, m);
        if (const char *m = check_list(s.lst[3], 0)) return bad(QR_ERR_ARG, m);
        for (int side = 0; side < 2; side++)
            for (int e = s.lst[side * 2]; e != QR_NULL; e = v.elm[e].next)
                if (const char *m = check_list(v.elm[e].data, 0)) return bad(QR_ERR_ARG, m);
    }
    return QR_OK;
}

void qr_bound_spheres(const qr_scene_view &v, std::vector<BSphere> &out)
{
    const int n = (int)v.hdr->n_srf;
    out.resize((size_t)n + 1);
    for (int i = 0; i < n; i++)
    {
        out[i] = bound_sphere(v, i);
    }
    out[n].c[0] = out[n].c[1] = out[n].c[2] = 0.0f; out[n].r = __builtin_inff();
}
