"""The case table of tests/test_api_refusals.py and tools/record_api_refusals.py: for every entry point of the ray API
(qr_trace_rays_async .. qr_layer_views_async and the image filters after them, qr_upsample_views_async ..
qr_reproject_moving_async, include/qrhip.h) a good call, the single bad arguments the function checks,
and every pair of them that can be applied together.  A case records (status, qr_last_error()); the pairs pin which refusal
wins when two apply.

Every case carries at least one refused argument or has zero elements, so no case launches a kernel: run() stops at the
first case that returns QR_OK with elements (or reaches the device at all) instead of going on.
"""
import ctypes
import hashlib
import itertools

FIXTURES = ["demo01_160", "demo01_160_aa2_t2500", "demo02_odd_33x17_aa4"]      # footprints 8x8, 8x4 and 4x4
N_RAYS, N_VIEWS, WIDTH, HEIGHT = 64, 2, 9, 13
QR_OK, QR_ERR_DEVICE = 0, -4
SLOT = 1 << 19              # bytes of device memory behind every good pointer
NAN, INF = float("nan"), float("inf")
VIEW_MAX_VIEWS, VIEW_MAX_DIM = 65535, 16384
ATROUS_FLAGS = UPSAMPLE_FLAGS = 31
REPROJ_FLAGS = 1


# ------------------------------------------------------------------------------------------------------- arguments
# An argument is (name, kind, good value, single bad values).  Kinds: "s" scene handle, "i" int, "q" int64, "f" float,
# "u" uint32 flags, "p" device pointer, "o" uint64 *bytes_out, "a" a parameter block (its good value: the binding's structure
# class by name and the good field values; an override "p.field" sets one field), "st" stream.

def S():
    return ("s", "s", "query", [("null", None)])


def N(what="n"):
    return (what, "q", N_RAYS, [("neg", -1), ("big", 1 << 31)])


def I(name, good, *bad):
    return (name, "i", good, [(str(b), b) for b in bad])


def F(name, good, *bad):
    return (name, "f", good, [(repr(b), b) for b in bad])


def FLAGS(allowed):
    return ("flags", "u", 0, [(f"bit{b}", 1 << b) for b in range(32) if not (allowed >> b) & 1])


def P(name, align, required=True):
    """a device pointer the function wants `align`-byte aligned (0: unchecked), null refused when required"""
    bad = [("null", "null")] if required else []
    bad += [(f"off{o}", o) for o in {16: (4, 8), 8: (4,), 4: (2,), 0: ()}[align]]
    return (name, "p", 0, bad)


def OUT():
    return ("bytes_out", "o", "good", [("null", None)])


STREAM = ("stream", "st", None, [])


def VIEWS(limit):
    """n_views, width, height; limit: the function holds views x footprints to one grid"""
    return [("n_views", "i", N_VIEWS, [("neg", -1), ("big", VIEW_MAX_VIEWS + 1)]),
            ("width", "i", WIDTH, [("0", 0), ("big", VIEW_MAX_DIM + 1)]),
            ("height", "i", HEIGHT, [("0", 0), ("big", VIEW_MAX_DIM + 1)])], \
           ([("overflow", dict(n_views=VIEW_MAX_VIEWS, width=VIEW_MAX_DIM, height=VIEW_MAX_DIM))] if limit else [])


K_FAN = I("k", 4, 0, 1025)
EPS, REACH = F("eps", 1e-3, NAN), F("reach", 1.0, NAN)
SAMPLES = I("samples", 1, 0, 513)
DONE = I("done", 0, -1, (1 << 24) - 1)
RULE = [I("min_samples", 1, -1), I("max_samples", 4, 0, 1 << 24), F("tol2", 0.01, -1.0, NAN, INF)]
RULE_X = [("min_gt_max", dict(min_samples=5, max_samples=4))]
# more pixel samples of state than one launch holds, in footprints that still fit one grid where the frame has no FSAA
SLOTS30 = [("slots30", dict(n_views=1025, width=1024, height=1024))]
SLOTS29 = SLOTS30 + [("slots29", dict(n_views=513, width=1024, height=1024))]


def fn(name, args, extra=(), zero=(), noquery=False, pt=False):
    """zero: the overrides that make the call one of no elements, e.g. [dict(n=0)]"""
    flat, more = [], list(extra)
    for a in args:
        if isinstance(a, tuple) and isinstance(a[0], list):      # VIEWS()
            flat += a[0]; more += a[1]
        elif isinstance(a, list):
            flat += a
        else:
            flat.append(a)
    return dict(name=name, args=flat, extra=more, zero=list(zero), noquery=noquery, pt=pt)


def _rays_fn(name, outs, flags=1, pt=False):
    return fn(name, [S(), P("rays", 16), N()] + outs + [FLAGS(flags), STREAM], zero=[dict(n=0)], noquery=True, pt=pt)


def _fan(name, src, views, framed, gather):
    allowed = (2 | 4 | 8) if gather else 2
    if src == "rays":
        allowed |= 1
    head = [S(), P(src, 16)] + ([VIEWS(True)] if views else [N()])
    spin = [P("spin", 8, False)] if framed else []
    outs = [P("gather", 16), P("count", 4)] if gather else [P("open", 4), P("mask", 4, False)]
    return fn(name, head + [P("dirs", 16), K_FAN] + spin + [EPS, REACH] + outs + [FLAGS(allowed), STREAM],
              zero=[dict(n_views=0) if views else dict(n=0)], noquery=True, pt=gather)


def PARAMS(cls, **good):
    return ("p", "a", (cls, good), [])


def _few_flags(allowed):
    """the flags word of a parameter block, thinned: the lowest unknown bit and bit 31"""
    low = min(b for b in range(32) if not (allowed >> b) & 1)
    return [(f"p.bit{b}", {"p.flags": 1 << b}) for b in (low, 31)]


def _floats(*fields_and_bad):
    """[(tag, override)]: per field of the parameter block its single bad values"""
    return [(f"{f}{b!r}", {"p." + f: b}) for f, *bad in fields_and_bad for b in bad]


def _atrous():
    par = [("p.null", {"p": None}),
           ("step0", {"p.step": 0}), ("step65", {"p.step": 65}), ("channels2", {"p.channels": 2}), ("channels5", {"p.channels": 5}),
           ("normal_sq-1", {"p.normal_sq": -1}), ("normal_sq8", {"p.normal_sq": 8})]
    par += [(f"p.bit{b}", {"p.flags": 1 << b}) for b in range(32) if not (ATROUS_FLAGS >> b) & 1]
    for f in ("sigma_z", "sigma_l2", "eps_l", "alb_floor"):
        par += [(f"{f}0", {"p." + f: 0.0}), (f"{f}nan", {"p." + f: NAN})]
    # one of the pair alone is refused, both null is a good call: never applied together ("var" is no argument)
    par += [("var_in.alone", {"var_in": "null", "var": 0}), ("var_out.alone", {"var_out": "null", "var": 0}),
            ("colour.inplace", {"colour_out": "=colour_in"}), ("var.inplace", {"var_out": "=var_in"})]
    return fn("qr_atrous_views_async",
              [S(), P("colour_in", 4), P("var_in", 4, False), P("hits", 16), VIEWS(False),
               PARAMS("AtrousParams", step=1, channels=3, normal_sq=0, flags=0, sigma_z=1.0, sigma_l2=1.0, eps_l=1.0, alb_floor=1.0),
               P("colour_out", 4), P("var_out", 4, False), STREAM], extra=par, zero=[dict(n_views=0)])


def _upsample():
    par = [("p.null", {"p": None}), ("factor0", {"p.factor": 0}), ("factor17", {"p.factor": 17}),
           ("phase_x-1", {"p.phase_x": -1}), ("phase_x2", {"p.phase_x": 2}), ("phase_y-1", {"p.phase_y": -1}), ("phase_y2", {"p.phase_y": 2}),
           # inside the lattice of factor 16, beyond the 9 x 13 frame
           ("phase_x.beyond", {"p.factor": 16, "p.phase_x": WIDTH}), ("phase_y.beyond", {"p.factor": 16, "p.phase_y": HEIGHT}),
           ("channels2", {"p.channels": 2}), ("channels5", {"p.channels": 5}),
           ("normal_sq-1", {"p.normal_sq": -1}), ("normal_sq8", {"p.normal_sq": 8})]
    par += _few_flags(UPSAMPLE_FLAGS) + _floats(("sigma_z", 0.0, NAN), ("alb_floor", 0.0, NAN))
    # as in _atrous(): one of the pair alone is refused, both null is a good call
    par += [("var_lo.alone", {"var_lo": "null", "var": 0}), ("var_out.alone", {"var_out": "null", "var": 0}),
            ("colour_out.is_colour_lo", {"colour_out": "=colour_lo"}), ("var_out.is_var_lo", {"var_out": "=var_lo"}),
            ("weight_out.is_hits", {"weight_out": "=hits"})]
    return fn("qr_upsample_views_async",
              [S(), P("colour_lo", 4), P("var_lo", 4, False), P("hits", 16), VIEWS(False),
               PARAMS("UpsampleParams", factor=2, phase_x=0, phase_y=0, channels=3, normal_sq=0, flags=0, sigma_z=1.0, alb_floor=1.0),
               P("colour_out", 4), P("var_out", 4, False), P("weight_out", 4, False), STREAM], extra=par, zero=[dict(n_views=0)])


def _reproject(moving):
    par = [("p.null", {"p": None}), ("channels2", {"p.channels": 2}), ("channels5", {"p.channels": 5})]
    par += _few_flags(REPROJ_FLAGS)
    par += [(f"reserved{i}", {"p.reserved": tuple(int(j == i) for j in range(3))}) for i in range(3)]
    par += _floats(("off_x", NAN, INF), ("off_y", NAN), ("normal_min", NAN), ("plane_max", 0.0, NAN), ("alb_floor", 0.0, NAN),
                   ("min_weight", -1.0, NAN), ("alpha_min", 1.5, NAN), ("alpha_mom_min", -0.5, NAN), ("max_len", 0.5, NAN),
                   ("var_min_len", 0.5, NAN))
    # the previous triple: all three is the good call and none a good first frame, so one or two alone are never applied
    # together ("prev" is no argument)
    trio = ("views_prev", "hits_prev", "hist_in")
    par += [(f"{a}.missing", {a: "null", "prev": 0}) for a in trio]
    par += [(f"{a}.alone", {**{b: "null" for b in trio if b != a}, "prev": 0}) for a in trio]
    par.append(("hist_out.is_hist_in", {"hist_out": "=hist_in"}))
    table = []
    if moving:
        table = [P("motion_dev", 16, False), I("n_motion", 3, -1, (1 << 30) + 1)]
        # a table without rows and rows without a table: both together are the static call, a good one ("motion" is no argument)
        par += [("n_motion.missing", {"n_motion": 0, "motion": 0}), ("motion_dev.missing", {"motion_dev": "null", "motion": 0})]
    return fn("qr_reproject_moving_async" if moving else "qr_reproject_views_async",
              [S(), P("colour_in", 4), P("hits", 16), P("var_in", 4, False), P("views_prev", 16, False), P("hits_prev", 16, False),
               P("hist_in", 16, False)] + table + [VIEWS(False),
               PARAMS("ReprojectParams", channels=3, flags=0, off_x=0.0, off_y=0.0, normal_min=0.5, plane_max=1.0, min_weight=0.5,
                      alpha_min=0.5, alpha_mom_min=0.5, max_len=2.0, var_min_len=2.0, unknown=1.0, alb_floor=1.0),
               P("hist_out", 16), P("colour_out", 4, False), P("var_out", 4, False), P("coords_out", 4, False), STREAM],
              extra=par, zero=[dict(n_views=0)])


FUNCTIONS = [
    _rays_fn("qr_trace_rays_async", [P("t_out", 0), P("id_out", 0)]),
    _rays_fn("qr_occluded_async", [P("occ_out", 0)]),
    _rays_fn("qr_shade_rays_async", [P("rgb_out", 0), P("id_out", 0, False)], pt=True),
    fn("qr_render_views_async", [S(), P("views", 16), VIEWS(True), P("frames", 4), P("ids", 4, False), P("depth", 4, False),
                                 FLAGS(0), STREAM], zero=[dict(n_views=0)], noquery=True, pt=True),
    # no footprint limit here (its grid is one frame), so no overflow case: that call would be a good one
    fn("qr_render_views_mean_async", [S(), P("views", 16), VIEWS(False), P("sum", 4), P("frame", 4, False),
                                      F("scale", 1.0, NAN, 0.0, INF), FLAGS(1), STREAM], zero=[dict(n_views=0)], noquery=True, pt=True),
    fn("qr_pt_views_state_bytes", [S(), VIEWS(True), OUT()], extra=SLOTS30, zero=[dict(n_views=0)]),
    fn("qr_pt_views_reset", [S(), VIEWS(True), P("state", 4)], extra=SLOTS30, zero=[dict(n_views=0)]),
    fn("qr_pt_views_async", [S(), P("views", 16), VIEWS(True), P("state", 4), DONE, SAMPLES, P("frames", 4), P("mean", 4, False),
                             FLAGS(0), STREAM], extra=SLOTS30, zero=[dict(n_views=0)], noquery=True),
    fn("qr_pt_rays_state_bytes", [S(), N(), OUT()], zero=[dict(n=0)]),
    fn("qr_pt_rays_reset", [S(), N(), P("state", 4)], zero=[dict(n=0)]),
    fn("qr_pt_rays_async", [S(), P("rays", 16), P("spread", 16, False), N(), P("state", 4), DONE, SAMPLES, P("rgb", 4, False),
                            FLAGS(0), STREAM], zero=[dict(n=0)], noquery=True),
    fn("qr_pt_adapt_state_bytes", [S(), N(), OUT()], zero=[dict(n=0)]),
    fn("qr_pt_adapt_reset", [S(), N(), P("state", 4)], zero=[dict(n=0)]),
    fn("qr_pt_adapt_rays_async", [S(), P("rays", 16), P("spread", 16, False), N(), P("state", 4), SAMPLES] + RULE +
       [P("rgb", 4, False), P("open", 4, False), FLAGS(0), STREAM], extra=RULE_X, zero=[dict(n=0)], noquery=True),
    fn("qr_pt_adapt_views_state_bytes", [S(), VIEWS(True), OUT()], extra=SLOTS29, zero=[dict(n_views=0)]),
    fn("qr_pt_adapt_views_reset", [S(), VIEWS(True), P("state", 4)], extra=SLOTS29, zero=[dict(n_views=0)]),
    fn("qr_pt_adapt_views_async", [S(), P("views", 16), VIEWS(True), P("state", 4), SAMPLES] + RULE +
       [P("frames", 4), P("mean", 4, False), P("counts", 4, False), P("open", 4, False), FLAGS(0), STREAM],
       extra=RULE_X + SLOTS29, zero=[dict(n_views=0)], noquery=True),
    fn("qr_pt_adapt_views_variance_async", [S(), P("state", 4), VIEWS(True), F("unknown", 1.0), P("var", 4), FLAGS(0), STREAM],
       extra=SLOTS29, zero=[dict(n_views=0)]),
    _atrous(),
    fn("qr_pt_adapt_list_work_bytes", [S(), N(), OUT()], zero=[dict(n=0)]),
    fn("qr_pt_adapt_open_list_async", [S(), P("state", 4), N()] + RULE + [P("index", 4), P("count", 4), P("work", 4), FLAGS(0), STREAM],
       extra=RULE_X, zero=[dict(n=0)], noquery=True),
    fn("qr_pt_adapt_list_rays_async", [S(), P("rays", 16), P("spread", 16, False), N(), P("state", 4), P("index", 4), P("count", 4),
                                       ("cap", "q", N_RAYS, [("neg", -1)]), SAMPLES] + RULE +
       [P("rgb", 4, False), P("open", 4, False), FLAGS(0), STREAM], extra=RULE_X, zero=[dict(n=0), dict(cap=0)], noquery=True),
    fn("qr_hit_rays_async", [S(), P("rays", 16), N(), P("hits", 16), FLAGS(1), STREAM], zero=[dict(n=0)], noquery=True),
    fn("qr_hit_views_async", [S(), P("views", 16), VIEWS(True), P("hits", 16), FLAGS(0), STREAM], zero=[dict(n_views=0)], noquery=True),
    _fan("qr_fan_rays_async", "rays", False, False, False), _fan("qr_fan_rays_framed_async", "rays", False, True, False),
    _fan("qr_fan_hits_async", "hits", False, False, False), _fan("qr_fan_hits_framed_async", "hits", False, True, False),
    _fan("qr_fan_views_async", "views", True, False, False), _fan("qr_fan_views_framed_async", "views", True, True, False),
    _fan("qr_gather_rays_async", "rays", False, False, True), _fan("qr_gather_rays_framed_async", "rays", False, True, True),
    _fan("qr_gather_hits_async", "hits", False, False, True), _fan("qr_gather_hits_framed_async", "hits", False, True, True),
    _fan("qr_gather_views_async", "views", True, False, True), _fan("qr_gather_views_framed_async", "views", True, True, True),
    fn("qr_layer_rays_async", [S(), P("rays", 16), N(), I("k", 4, 0, 65), P("count", 4), P("t", 4, False), P("id", 4, False),
                               P("hits", 16, False), FLAGS(1), STREAM], zero=[dict(n=0)], noquery=True),
    fn("qr_layer_views_async", [S(), P("views", 16), VIEWS(True), I("k", 4, 0, 65), P("count", 4), P("t", 4, False), P("id", 4, False),
                                P("hits", 16, False), FLAGS(0), STREAM], zero=[dict(n_views=0)], noquery=True),
    _upsample(), _reproject(False), _reproject(True),
]
assert len({f["name"] for f in FUNCTIONS}) == len(FUNCTIONS) == 41
# The recordings under tests/golden, each with the functions it holds.  The three image filters that came after the first
# recording have a file of their own, so that the first one stands as it was recorded, byte for byte.
RECORDINGS = {"api_refusals.json": FUNCTIONS[:38], "api_refusals_filters.json": FUNCTIONS[38:]}


# ----------------------------------------------------------------------------------------------------------- cases

def singles(f):
    """[(id, overrides, zero)]: the single cases of one function, in a fixed order"""
    out = [(f"{a[0]}.{tag}", {a[0]: val}, False) for a in f["args"] for tag, val in a[3]]
    out += [(tag, dict(ov), False) for tag, ov in f["extra"]]
    if f["noquery"]:
        out.append(("s.noquery", {"s": "noquery"}, False))
    if f["pt"]:
        out.append(("s.pt", {"s": "pt"}, False))
    ptrs = {a[0]: "null" for a in f["args"] if a[1] == "p"}
    ptrs.update({a[0]: None for a in f["args"] if a[1] == "o"})
    for z in f["zero"]:
        key = "+".join(f"{k}0" for k in z)
        out.append((f"zero.{key}", dict(z), True))                   # no elements, every pointer good
        out.append((f"zero.{key}.nullptrs", {**z, **ptrs}, True))    # no elements, every pointer null
    return out


def _clash(a, b):
    return any(x == y or x.startswith(y + ".") or y.startswith(x + ".") for x in a for y in b)


def cases(f):
    """the single cases, then every unordered pair of them whose overrides touch different arguments.  Two zero-element
    cases are no pair: together they carry no refused argument more than each alone."""
    one = singles(f)
    out = list(one)
    for (ia, oa, za), (ib, ob, zb) in itertools.combinations(one, 2):
        if not _clash(oa, ob) and not (za and zb):
            out.append((f"{ia}&{ib}", {**oa, **ob}, za or zb))
    return out


def table_digest(f):
    return hashlib.sha1("\n".join(i for i, _, _ in cases(f)).encode()).hexdigest()[:16]


# --------------------------------------------------------------------------------------------------------- calling

class Rig:
    """The scenes of one fixture and the device memory the good pointers point into."""

    def __init__(self, qr, blob, with_variants):
        import torch
        self.qr, self.L = qr, qr.lib()
        self.scenes = {"query": qr.Scene(blob, ray_queries=True)}
        if with_variants:
            self.scenes["noquery"] = qr.Scene(blob)
            self.scenes["pt"] = qr.Scene(blob, ray_queries=True)
            self.scenes["pt"].set_pt(True)
        self.mem = torch.zeros(24 * SLOT, dtype=torch.uint8, device="cuda:0")
        self.base = (self.mem.data_ptr() + 255) & ~255
        self.bytes_out = ctypes.c_uint64()
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def close(self):
        for s in self.scenes.values():
            s.close()

    def call(self, f, over):
        """(status, message) of one call of f with the overrides applied to the good call"""
        where = {a[0]: self.base + i * SLOT for i, a in enumerate(a for a in f["args"] if a[1] == "p")}
        argv = []
        for name, kind, good, _ in f["args"]:
            v = over.get(name, good)
            if kind == "s":
                argv.append(None if v is None else self.scenes[v]._h)
            elif kind == "p":
                if v == "null":
                    argv.append(None)
                elif isinstance(v, str):                             # "=other": the other argument's good pointer
                    argv.append(where[v[1:]])
                else:
                    argv.append(where[name] + v)
            elif kind == "o":
                argv.append(None if v is None else ctypes.byref(self.bytes_out))
            elif kind == "a":
                if v is None:
                    argv.append(None)
                else:
                    cls, fields = v
                    fields = {**fields, **{k[2:]: x for k, x in over.items() if k.startswith("p.")}}
                    argv.append(ctypes.byref(getattr(self.qr, cls)(**fields)))
            elif kind == "st":
                argv.append(self.stream)
            else:
                argv.append(v)
        rc = getattr(self.L, f["name"])(*argv)
        return (rc, "" if rc == QR_OK else self.L.qr_last_error().decode())


def open_rigs(qr, load_blob):
    return {fx: Rig(qr, load_blob(fx), fx == FIXTURES[0]) for fx in FIXTURES}


def run(rigs, visit, functions=FUNCTIONS):
    """Every case of every one of `functions` on every fixture: visit(fixture, function, case id, (status, message)) right after each
    call.  A call that got as far as the device (QR_OK with elements, or a device error) ends the run at once."""
    for fixture, rig in rigs.items():
        for f in functions:
            for cid, over, zero in cases(f):
                if over.get("s") in ("noquery", "pt") and len(rig.scenes) == 1:
                    continue                                     # those two scenes exist for the first fixture alone
                got = rig.call(f, over)
                if (got[0] == QR_OK and not zero) or got[0] == QR_ERR_DEVICE:
                    raise AssertionError(f"{fixture} {f['name']} {cid}: the case was not refused before the device: {got}")
                visit(fixture, f["name"], cid, got)


def survivor_trace(rig, oracle, blob):
    """After the refusals: 64 camera rays of the fixture's own frame, spread over it, traced on the scene that took every
    refused call.  Returns (ids, the oracle's ids of those pixels)."""
    import importlib
    import numpy as np
    import torch
    import _rayq
    rays_mod = importlib.import_module("quadray_engine_amd.rays")
    cam = _rayq.with_frame(blob)
    _, ref, _ = oracle.render(cam, depth=0, threads=16, want_ids=True)
    rays = rays_mod.camera_rays(cam)
    pick = np.linspace(0, len(rays) - 1, N_RAYS).astype(np.int64)
    r = torch.from_numpy(np.ascontiguousarray(rays[pick], dtype=np.float32)).to("cuda:0")
    _, ids = rig.scenes["query"].trace(r)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), ref.reshape(-1)[pick]
