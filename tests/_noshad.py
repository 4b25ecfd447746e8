"""Large scenes with surfaces that cast no shadow, for tests/test_noshad_walks.py, and a reader of the dumped device image that
shares nothing with the compiler's own verification (qr_program_verify).

The patch rule (patched): the members in the order of _rayq.real_surfaces(blob)[1:] -- the ground plane stays --
  j % 3 == 0   both props words become (p | TRANSP) & ~(REFRACT | OPAQUE): plainly transparent, a QR_OPF_NOSHAD cell
  j % 3 == 1   the inner side's word alone: the outer side casts, the inner does not, a QR_OPF_SIDESHAD cell
  otherwise    the record stays
light_bodies: in a FLAT crowd (moving a member out of its array's volume would break the volume) the first n_lgt members of
tag 2 are moved to the lights' positions and get QR_PROP_LIGHT on both sides: every shadow ray then aims at a cell that the
shadow program leaves out, as the demo scenes' do on short lists.

The image reader (ShadowImage) knows the layout of csrc/qr_program.h and nothing of the compiler: DevHeader.off_shade ->
DShade.lgt[side] -> the CLight entries (in the order of the snapshot's light list) -> the list program or the CGrid.
"""
import os

import numpy as np

import _crowd
import _rayq

P_LIGHT, P_OPAQUE, P_TRANSP, P_REFRACT = 0x10, 0x200, 0x400, 0x2000
S_SOLVER, S_TAG, S_PROPS, S_LST = 34, 37, 42, 44                # qr_surface words (include/qr_scene.h)

# csrc/qr_program.h
OPT_SOLVER, OPT_BV, OPT_TRNODE = 7, 8, 16
LISTF_DIV, LISTF_LONG, LISTF_WORLD, LISTF_GRID, LISTF_DDA = 1, 2, 4, 8, 16
OFF_SRF, DSURF, DSHADE, CELL = 256, 128, 32, 32
H_OFF_SHADE, H_IMG_BYTES = 49, 54                               # DevHeader words behind the 49 of qr_frame


# ------------------------------------------------------------------------------------------------ snapshots

def _with_surfaces(blob, s):
    b = bytearray(blob)
    off = _rayq._hdr(b)[11]
    b[off:off + s.nbytes] = s.tobytes()
    return bytes(b)


def patched(blob):
    """the snapshot with every third member plainly transparent and every third one-sided (the module's text)"""
    s, _ = _rayq.surfaces(blob)
    for j, i in enumerate(_rayq.real_surfaces(blob)[1:]):
        for k in ((0, 1) if j % 3 == 0 else (1,) if j % 3 == 1 else ()):
            s[i, S_PROPS + k] = (int(s[i, S_PROPS + k]) | P_TRANSP) & ~(P_REFRACT | P_OPAQUE)
    return _with_surfaces(blob, s)


def lights(blob):
    """qr_light records as float32 [n_lgt, 16]"""
    h = _rayq._hdr(blob)
    return np.frombuffer(blob, dtype=np.float32, count=h[6] * 16, offset=h[13]).reshape(h[6], 16).copy()


def light_bodies(blob):
    """(snapshot, surface indices): the first n_lgt members of tag 2 of a flat crowd as the lights' bodies"""
    s, f = _rayq.surfaces(blob)
    assert not ((elems(blob)[:, 3] & 3) == 1).any(), "light_bodies: a flat crowd only"
    L = lights(blob)
    which = [int(i) for i in _rayq.real_surfaces(blob)[1:] if s[i, S_TAG] == 2][:len(L)]
    assert len(which) == len(L)
    for i, l in zip(which, L):
        f[i, 0:3] = l[1:4]
        s[i, S_PROPS:S_PROPS + 2] |= P_LIGHT
    return _with_surfaces(blob, s), which


def elems(blob):
    """qr_elem records as int32 [n_elm, 4]: simd, data, next, kind"""
    h = _rayq._hdr(blob)
    return np.frombuffer(blob, dtype=np.int32, count=h[7] * 4, offset=h[14]).reshape(h[7], 4).copy()


def chain(E, head):
    out = []
    while head >= 0:
        out.append(head)
        head = int(E[head, 2])
    return out


SCENES = ["hier_raw", "hier_built", "dense_built", "open_raw", "flat_lights", "mid_own", "mid_built"]
_BLOBS = {}


def _qr():
    from qr_loader import load_package
    return load_package()


def base_blob(name):
    """the scene as its generator writes it, before the patch rule"""
    key = ("base", name)
    if key not in _BLOBS:
        S = _crowd.synth()
        if name.startswith("mid"):
            from test_synth import MID
            b = S.make_scene(**MID) if name == "mid_own" else S.make_scene(shadow_lists=False, **MID)
        elif name == "flat_lights":
            b = _crowd.make_crowd(**dict(_crowd.HIER, hierarchy=False))
        else:
            b = _crowd.make_crowd(**{"hier": _crowd.HIER, "dense": _crowd.DENSE, "open": _crowd.OPEN}[name.split("_")[0]])
        _BLOBS[key] = b
    return _BLOBS[key]


def scene_blob(name):
    """the patched scene `name` of SCENES; the *_built ones through the product's list-building pass after the patch"""
    if name not in _BLOBS:
        b = patched(base_blob(name))
        if name == "flat_lights":
            b = light_bodies(b)[0]
        if name.endswith("_built"):
            b = bytes(_qr().build_lists(b))
        _BLOBS[name] = b
    return _BLOBS[name]


class env:
    def __init__(self, e):
        self.e = {k: str(v) for k, v in e.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.e}
        os.environ.update(self.e)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def dump_image(qr, blob, path, e=None, flags=0):
    """(program_stats, the device image as uint32 words) of the snapshot uploaded under the environment `e`"""
    with env(dict(e or {}, QR_DUMP_IMAGE=path)):
        st = qr.program_stats(blob, flags) if flags else qr.program_stats(blob)
    img = np.fromfile(path, dtype=np.uint32)
    os.remove(path)
    return st, img


# ------------------------------------------------------------------------------------------------ the image reader

class ImageError(AssertionError):
    pass


def _need(cond, *what):
    if not cond:
        raise ImageError(" ".join(str(w) for w in what))


class ShadowImage:
    """The shadow programs of a dumped image, read against the snapshot it was built from."""

    def __init__(self, blob, img):
        self.img = img
        self.n_bytes = img.size * 4
        self.s, _ = _rayq.surfaces(blob)
        self.E = elems(blob)
        self.real = [int(i) for i in _rayq.real_surfaces(blob)]
        self.casting = _rayq.casts(blob).any(axis=1)
        self.off_shade = int(img[H_OFF_SHADE])
        _need(int(img[H_IMG_BYTES]) == self.n_bytes, "img_bytes", int(img[H_IMG_BYTES]), self.n_bytes)
        _need(self.off_shade % 4 == 0 and self.off_shade + DSHADE * len(self.s) <= self.n_bytes, "off_shade")
        self._programs = {}
        self._chains = {}

    def word(self, off):
        _need(off % 4 == 0 and 0 <= off and off + 4 <= self.n_bytes, "offset outside the image:", off)
        return int(self.img[off // 4])

    def is_solver(self, i):
        return 0 <= self.s[i, S_TAG] < 9 and 1 <= self.s[i, S_SOLVER] <= 3

    def chain_solvers(self, head):
        """solver surfaces of the snapshot chain, in chain order"""
        if head not in self._chains:
            self._chains[head] = [int(self.E[e, 0]) for e in chain(self.E, head) if self.is_solver(int(self.E[e, 0]))]
        return self._chains[head]

    def program(self, word):
        """solver surfaces of the list program a list word points at, in program order; checks every bounding-volume cell's
        `end` and `mid` and the length word of a world-space list without clippers on the way"""
        off = word & ~31
        if off in self._programs:
            return self._programs[off]
        _need(off >= OFF_SRF + DSURF * len(self.s), "program inside the header or the surface records:", off)
        p, solvers, bvs, bounds = off, [], [], set()
        while True:
            bounds.add(p)
            op = self.word(p)
            if op == 0:
                break
            kind = op & 31
            _need(kind in (1, 2, 4, OPT_BV, OPT_TRNODE), "cell type bits", hex(op), "at", p)
            srf = self.word(p + 4) - OFF_SRF
            _need(srf >= 0 and srf % DSURF == 0 and srf // DSURF < len(self.s), "cell's surface offset at", p)
            if kind & OPT_SOLVER:
                _need(self.is_solver(srf // DSURF), "solver cell of a surface without solver at", p)
                solvers.append(srf // DSURF)
            if kind == OPT_BV:
                bvs.append((p, self.word(p + 8), self.word(p + CELL + 12)))
                p += CELL
            p += CELL
            _need(p - off <= CELL * 4 * (len(self.E) + 1), "program without END cell at", off)
        end_cell = p
        open_ends = []
        for at, end, mid in bvs:
            while open_ends and open_ends[-1] <= at:
                open_ends.pop()
            _need(end in bounds, "array end", end, "of the cell at", at, "is no cell boundary of the program at", off)
            _need(at + 2 * CELL <= end <= end_cell, "array end", end, "of the cell at", at, "program", off, "..", end_cell)
            _need(not open_ends or end <= open_ends[-1], "array at", at, "ends behind the array around it")
            open_ends.append(end)
            _need(mid == 0 or (mid in bounds and at + 2 * CELL < mid < end), "hand-over offset", mid, "of the array at", at)
        if word & LISTF_DIV and word & LISTF_WORLD:         # the length word in front of the program (walk_pool)
            want = (end_cell - off) | (0 if bvs else 1)
            _need(self.word(off - 4) == want, "length word", self.word(off - 4), "of the program at", off, "want", want)
        self._programs[off] = solvers
        return solvers

    def light_entries(self, i, side):
        """[(light, shadow head of the snapshot, CLight::shadow)] of surface i's side"""
        head = int(self.s[i, S_LST + 2 * side])
        chain_l = chain(self.E, head)
        at = self.word(self.off_shade + DSHADE * i + 8 + 4 * side)
        _need((at == 0) == (not chain_l), "light list of surface", i, "side", side)
        out = []
        for k, e in enumerate(chain_l):
            lgt, shadow = self.word(at + 8 * k), self.word(at + 8 * k + 4)
            _need((lgt & 1) == (k == len(chain_l) - 1), "QR_CLIGHT_LAST of surface", i, "side", side, "entry", k)
            out.append((int(self.E[e, 0]), int(self.E[e, 1]), shadow))
        return out

    def check(self, shadowless=True):
        """every shadow word of every real surface against the snapshot's shadow chain; returns the counts
        dict(refs, left_out, grids, grid_lists)"""
        n = dict(refs=0, left_out=0, grids=0, grid_lists=0)
        grids = set()
        for i in self.real:
            for side in (0, 1):
                for lgt, head, shadow in self.light_entries(i, side):
                    where = f"surface {i} side {side} light {lgt}"
                    full = self.chain_solvers(head)
                    if head < 0:
                        _need(shadow == 0, where, "no shadow chain, yet a program")
                        continue
                    if shadow & LISTF_GRID:
                        g = shadow & ~31
                        if g in grids:
                            continue
                        grids.add(g)
                        table, nx, ny = self.word(g), self.word(g + 4), self.word(g + 8)
                        _need(1 <= nx <= 64 and 1 <= ny <= 64, where, "grid size", nx, ny)
                        for c in range(nx * ny):
                            w = self.word(table + 4 * c)
                            if w == 0:
                                continue
                            it = iter(full)
                            _need(all(x in it for x in self.program(w)), where, "grid cell", c, "holds what the chain does not")
                            n["grid_lists"] += 1
                        n["grids"] += 1
                        continue
                    want = [x for x in full if self.casting[x]] if shadowless else full
                    got = self.program(shadow)
                    _need(got == want, where, f"program of {len(got)} solver cells, want {len(want)} of the chain's {len(full)}")
                    n["refs"] += 1
                    n["left_out"] += len(full) - len(got)
        return n

    def shadow_words(self, i, side=0):
        return [w for _, _, w in self.light_entries(i, side)]

    def side_list_word(self, i, side=0):
        """DShade.lst[side]: the surface's list for secondary rays"""
        return self.word(self.off_shade + DSHADE * i + 16 + 4 * side)
