"""The case table of tests/test_py_refusals.py and tools/record_py_refusals.py: the Python-level twin of _api_refusals.py.
For every public method of Scene from trace() through render_views_mean(), for the four accumulators (constructor,
step, open_list, variance, clone) and, after them, for the image filters upsample() and reproject() and for Temporal
(constructor, step, clone) a good call, the single bad arguments that the method or the library behind it refuses,
and every pair of them that can be applied together.  A case records (exception type name, str(exception)), or ("ok", the
shapes and dtypes of what came back) for a call of no elements; the pairs pin which refusal wins when two apply.

Every case carries at least one refused argument or has zero elements, so no case launches a kernel of the library:
run() stops at the first case that returns with elements instead of going on.
"""
import hashlib
import itertools

FIXTURE = "demo01_160"
N_RAYS, N_VIEWS, WIDTH, HEIGHT, K_DIRS = 64, 2, 9, 13, 4       # the C table's sizes
SLOTS = WIDTH * HEIGHT                                          # the fixture has no FSAA (Rig checks)
NAN, INF = float("nan"), float("inf")
OMIT = ("omit",)            # the argument is not passed at all
OTHER = {"float32": "float64", "int32": "int64"}


class Same:
    """The very tensor that member `index` of the call's tuple argument `name` is."""

    def __init__(self, name, index):
        self.name, self.index = name, index


# ------------------------------------------------------------------------------------------------------- arguments

class T:
    """A tensor of zeros to be made on the rig: dtype, shape, where it lives ("cuda", "cpu", "numpy") and whether it is a
    non-contiguous view."""

    def __init__(self, dtype, *shape, where="cuda", strided=False):
        self.dtype, self.shape, self.where, self.strided = dtype, tuple(shape), where, strided

    def key(self):
        return (self.dtype, self.shape, self.where, self.strided)

    def numpy(self):
        return T(self.dtype, *self.shape, where="numpy")

    def cpu(self):
        return T(self.dtype, *self.shape, where="cpu")

    def wide(self):
        return T(self.dtype, *self.shape, strided=True)

    def make(self):
        import numpy as np
        import torch
        if self.where == "numpy":
            return np.zeros(self.shape, dtype=self.dtype)
        dev = "cuda:0" if self.where == "cuda" else "cpu"
        if not self.strided:
            return torch.zeros(self.shape, dtype=getattr(torch, self.dtype), device=dev)
        t = torch.zeros(self.shape[:-1] + (2 * self.shape[-1],), dtype=getattr(torch, self.dtype), device=dev)[..., ::2]
        assert tuple(t.shape) == self.shape and not t.is_contiguous()
        return t


def kinds(good, rank=True, last=False, rows=False, strided=True):
    """the kinds of badness the binding tells apart in a tensor argument whose good value is `good`.  rank: True for one more
    leading dimension, or the shape to use; last: the last dimension is part of the contract; rows: so is the first"""
    d, s = good.dtype, good.shape
    out = [("numpy", good.numpy()), ("dtype", T(OTHER[d], *s))]
    if rank:
        out.append(("rank", T(d, 1, *s) if rank is True else T(d, *rank)))
    if last:
        out.append(("last", T(d, *s[:-1], s[-1] + 1)))
    if rows:
        out.append(("rows", T(d, s[0] + 1, *s[1:])))
    if strided:
        out.append(("strided", good.wide()))
    out.append(("cpu", good.cpu()))
    return out


def A(name, good, *bad):
    """an argument: its name, its good value and the single bad values as (tag, value)"""
    return (name, good, [b if isinstance(b, tuple) and len(b) == 2 and isinstance(b[0], str) else (repr(b), b) for b in bad])


def TA(name, good, given=True, **kw):
    """a tensor argument; given=False: the good call leaves it None"""
    return (name, good if given else None, kinds(good, **kw))


F32, I32 = "float32", "int32"
RAYS, RAYS0 = T(F32, N_RAYS, 8), T(F32, 0, 8)
VIEWS, VIEWS0 = T(F32, N_VIEWS, 16), T(F32, 0, 16)
HITS, HITS0 = T(F32, N_RAYS, 12), T(F32, 0, 12)
DIRS = T(F32, K_DIRS, 4)
E_RAYS, E_VIEWS = (N_RAYS,), (N_VIEWS, HEIGHT, WIDTH)            # the element shapes

S_QUERY = A("s", "query", ("noquery", "noquery"))
A_RAYS = TA("rays", RAYS, last=True)
A_VIEWS = TA("views", VIEWS, last=True)
A_SIZE = [A("width", WIDTH, 0, 1.5), A("height", HEIGHT, 0)]
A_HITS = TA("hits", HITS, rank=(12,), last=True)
# dirs need not be contiguous (the binding makes them so): no strided kind; dirs.strided stands in EXTRA_DIRS with a refused eps
A_DIRS = ("dirs", DIRS, kinds(DIRS, last=True, strided=False) + [("k0", T(F32, 0, 4)), ("k1025", T(F32, 1025, 4))])
A_EPS, A_REACH = A("eps", 1e-3, None, NAN), A("reach", 1.0, NAN)
EXTRA_DIRS = [("dirs.strided+eps.None", dict(dirs=DIRS.wide(), eps=None))]
A_SAMPLES = A("samples", 1, 1.5, 0, 513)
A_RULE = [A("min_samples", 1, -1, 1.5), A("max_samples", 4, 0, 1 << 24), A("tol", 0.01, -1, "x", 1e30, NAN)]
X_RULE = [("min_gt_max", dict(min_samples=5, max_samples=4))]


def fn(name, target, args, extra=(), zero=()):
    """target: ("scene", method), ("new", class) or ("acc", class, method).  zero: the overrides that make the call one of no
    elements (or one that only copies: clone)"""
    flat = []
    for a in args:
        flat += a if isinstance(a, list) else [a]
    return dict(name=name, target=target, args=flat, extra=list(extra), zero=list(zero))


def _rays_fn(meth, more=()):
    return fn(meth, ("scene", meth), [S_QUERY, A_RAYS] + list(more), zero=[("rays0", dict(rays=RAYS0))])


def _fan(meth, src, gather, framed):
    elem = E_VIEWS if src == "views" else E_RAYS
    head = {"rays": [A_RAYS], "views": [A_VIEWS] + A_SIZE, "hits": [A_HITS]}[src]
    empty = {"rays": RAYS0, "views": VIEWS0, "hits": HITS0}[src]
    zero = {src: empty}
    args = [S_QUERY] + head + [A_DIRS, A_EPS, A_REACH]
    extra = list(EXTRA_DIRS)
    if framed:
        spin = T(F32, *elem, 2)
        args += [A("frame", True), TA("spin", spin, last=True, rows=True)]
        zero["spin"] = T(F32, 0, *elem[1:], 2)
    else:
        args += [A("spin", None, ("noframe", T(F32, *elem, 2)))]
    if gather:
        out, count = T(F32, *elem, 4), T(I32, *elem)
        args += [TA("out", out, given=False, last=True, rows=True), TA("count", count, given=False, rows=True),
                 A("resume", False, True)]
        extra += [("resume+out", dict(resume=True, out=out)), ("resume+count", dict(resume=True, count=count))]
    else:
        args += [A("mask", True)]
    return fn(meth + ("[framed]" if framed else ""), ("scene", meth), args, extra=extra, zero=[(src + "0", zero)])


def _atrous_tensors():
    n, h, w = E_VIEWS
    col, hits, var = T(F32, n, h, w, 3), T(F32, n, h, w, 12), T(F32, n, h, w)
    return [("colour", col, kinds(col, rank=(h, w, 3)) + [("channels5", T(F32, n, h, w, 5)), ("empty", T(F32, 0, h, w, 3))]),
            TA("hits", hits, last=True, rows=True), TA("variance", var, rows=True)], col, var


def _atrous():
    tens, col, var = _atrous_tensors()
    return fn("atrous", ("scene", "atrous"),
              [A("s", "query")] + tens + [A("step", 1, 0, 65, True, 1.5), A("normal_power", 128, 3), A("plane", None, 0.0),
                                          A("luma", None, -2.0), TA("out", col, given=False, last=True, rows=True),
                                          TA("variance_out", var, given=False, rows=True)],
              extra=[("variance_out.alone", dict(variance=None, variance_out=var))])


def _denoise():
    tens, _, _ = _atrous_tensors()
    return fn("denoise", ("scene", "denoise"),
              [A("s", "query")] + tens + [A("passes", 5, 0, 8, True), A("plane", None, 0.0), A("demodulate", OMIT, True),
                                          A("modulate", OMIT, False), A("nonsense", OMIT, 1)])


LAYER_K = A("k", 4, 0, 65, 1.5)
FRAMES = TA("frames", T(I32, *E_VIEWS), given=False, rows=True)
MEAN = ("mean", False, kinds(T(F32, *E_VIEWS, 3), last=True, rows=True))
COUNTS = ("counts", False, kinds(T(I32, *E_VIEWS), rows=True))
OPEN = ("open", True, kinds(T(I32, 1), rank=False, rows=True, strided=False))
SPREAD = TA("spread", T(F32, N_RAYS, 8), given=False, last=True, rows=True)
RGB = ("rgb", True, kinds(T(F32, N_RAYS, 3), last=True, rows=True))
ACC_RAYS = TA("rays", RAYS, last=True, rows=True)         # rows: a ray count that differs from the accumulator's
ACC = A("acc", "query", ("noquery", "noquery"))


def _state(*shape):
    st = T(I32, *shape)
    return TA("state", st, given=False, rows=True), st


def _index(n, given, **kw):
    """index and count of an open list"""
    return [TA("index", T(I32, n), given=given, **kw), TA("count", T(I32, 1), given=given, rows=True, strided=False)]


ST_VIEWS, ST_VIEWS_T = _state(N_VIEWS, 4, SLOTS)
ST_RAYS, ST_RAYS_T = _state(4, N_RAYS)
ST_ADAPT, _ = _state(8, N_RAYS)
ST_AVIEWS, _ = _state(N_VIEWS, 8, SLOTS)
A_N = A("n", N_RAYS, -1, 1.5)


def _held(state):
    """`samples` of the two plain accumulators: refused with a new state, checked with a caller's"""
    return [("state+samples-1", dict(state=state, samples=-1)), ("state+samples1.5", dict(state=state, samples=1.5))]


FUNCTIONS = [
    _rays_fn("trace"), _rays_fn("occluded"), _rays_fn("shade", [A("ids", True)]), _rays_fn("hits"),
    fn("view_hits", ("scene", "view_hits"), [S_QUERY, A_VIEWS, A("width", WIDTH, 0, 1.5, 16385), A("height", HEIGHT, 0)],
       zero=[("views0", dict(views=VIEWS0))]),
    _atrous(), _denoise(),
    _fan("occlusion", "rays", False, False), _fan("occlusion", "rays", False, True),
    _fan("view_occlusion", "views", False, False), _fan("view_occlusion", "views", False, True),
    _fan("hit_occlusion", "hits", False, False), _fan("hit_occlusion", "hits", False, True),
    _fan("gather", "rays", True, False), _fan("gather", "rays", True, True),
    _fan("view_gather", "views", True, False), _fan("view_gather", "views", True, True),
    _fan("hit_gather", "hits", True, False), _fan("hit_gather", "hits", True, True),
    _rays_fn("trace_layers", [LAYER_K, A("hits", True)]),
    fn("view_layers", ("scene", "view_layers"), [S_QUERY, A_VIEWS, LAYER_K] + A_SIZE + [A("hits", True)],
       zero=[("views0", dict(views=VIEWS0))]),
    fn("render_views", ("scene", "render_views"), [S_QUERY, A_VIEWS] + A_SIZE + [FRAMES, A("ids", True), A("depth", True)],
       zero=[("views0", dict(views=VIEWS0))]),
    fn("render_views_mean", ("scene", "render_views_mean"),
       [S_QUERY, A_VIEWS] + A_SIZE + [TA("sum", T(F32, HEIGHT, WIDTH, 3), given=False, last=True, rows=True),
                                      ("frame", True, kinds(T(I32, HEIGHT, WIDTH), rows=True)),
                                      A("scale", None, 0.0, INF, NAN), A("resume", False, True)],
       extra=[("resume+sum", dict(resume=True, sum=T(F32, HEIGHT, WIDTH, 3)))], zero=[("views0", dict(views=VIEWS0))]),

    fn("PtViews", ("new", "PtViews"), [A_VIEWS] + A_SIZE + [ST_VIEWS, A("samples", 0, 1)], extra=_held(ST_VIEWS_T),
       zero=[("views0", dict(views=VIEWS0))]),
    fn("PtViews.step", ("acc", "PtViews", "step"), [ACC, A_SAMPLES, FRAMES, MEAN], zero=[("acc0", dict(acc="zero"))]),
    fn("PtViews.clone", ("acc", "PtViews", "clone"), [A("acc", "query")], zero=[("clone", {})]),
    fn("PtRays", ("new", "PtRays"), [A_N, ST_RAYS, A("samples", 0, 1)], extra=_held(ST_RAYS_T), zero=[("n0", dict(n=0))]),
    fn("PtRays.step", ("acc", "PtRays", "step"), [ACC, ACC_RAYS, A_SAMPLES, SPREAD, RGB],
       zero=[("acc0", dict(acc="zero", rays=RAYS0))]),
    fn("PtRays.clone", ("acc", "PtRays", "clone"), [A("acc", "query")], zero=[("clone", {})]),
    fn("PtAdaptive", ("new", "PtAdaptive"), [A_N] + A_RULE + [ST_ADAPT], extra=X_RULE, zero=[("n0", dict(n=0))]),
    fn("PtAdaptive.open_list", ("acc", "PtAdaptive", "open_list"), [ACC] + _index(N_RAYS, False, rows=True),
       zero=[("acc0", dict(acc="zero"))]),
    fn("PtAdaptive.step", ("acc", "PtAdaptive", "step"),
       [ACC, ACC_RAYS, A_SAMPLES, SPREAD, RGB, OPEN, A("index", None), A("count", None), A("cap", None)],
       # each names the argument it leaves out, so that no two of them pair up into a good list call
       extra=[("index.alone", dict(index=T(I32, N_RAYS), count=None)), ("count.alone", dict(count=T(I32, 1), index=None)),
              ("cap.alone", dict(cap=3, index=None))], zero=[("acc0", dict(acc="zero", rays=RAYS0))]),
    # the list form: any length of index is a good one, so its first dimension is not part of the contract
    fn("PtAdaptive.step[list]", ("acc", "PtAdaptive", "step"),
       [ACC, ACC_RAYS, A_SAMPLES, SPREAD, RGB, OPEN] + _index(N_RAYS, True, rank=(1, N_RAYS))
       + [A("cap", None, -1, N_RAYS + 1, 1.5)], zero=[("acc0", dict(acc="zero", rays=RAYS0)), ("cap0", dict(cap=0))]),
    fn("PtAdaptive.clone", ("acc", "PtAdaptive", "clone"), [A("acc", "query")], zero=[("clone", {})]),
    fn("PtAdaptiveViews", ("new", "PtAdaptiveViews"), [A_VIEWS] + A_SIZE + A_RULE + [ST_AVIEWS], extra=X_RULE,
       zero=[("views0", dict(views=VIEWS0))]),
    fn("PtAdaptiveViews.variance", ("acc", "PtAdaptiveViews", "variance"),
       [A("acc", "query"), TA("out", T(F32, *E_VIEWS), given=False, rows=True), A("unknown", 1.0, "x")],
       zero=[("acc0", dict(acc="zero"))]),
    fn("PtAdaptiveViews.open_list", ("acc", "PtAdaptiveViews", "open_list"),
       [A("acc", "query", ("noquery", "noquery"), ("zero", "zero")), A("view", 0, -1, N_VIEWS, 1.5)] + _index(SLOTS, False, rows=True)),
    fn("PtAdaptiveViews.step", ("acc", "PtAdaptiveViews", "step"), [ACC, A_SAMPLES, FRAMES, MEAN, COUNTS, OPEN],
       zero=[("acc0", dict(acc="zero"))]),
    fn("PtAdaptiveViews.clone", ("acc", "PtAdaptiveViews", "clone"), [A("acc", "query")], zero=[("clone", {})]),
]


# The image filters that came after the recording of the functions above: appended, so that the earlier cases keep their places.
# The frame is the table's, 2 views of 9 x 13; upsample() at factor 2, phase (0, 0): a coarse frame of 5 x 7.
FACTOR, W_LO, H_LO = 2, 5, 7
FRAME = (N_VIEWS, HEIGHT, WIDTH)
COLOUR, RECORDS, VARIANCE = T(F32, *FRAME, 3), T(F32, *FRAME, 12), T(F32, *FRAME)
HISTORY, MOTION = T(F32, *FRAME, 8), T(F32, 3, 12)
PREV = (VIEWS, RECORDS, HISTORY)
# a colour of 4 channels is a good one: no `last` kind, as in _atrous_tensors()
A_COLOUR = ("colour", COLOUR, kinds(COLOUR, rank=(HEIGHT, WIDTH, 3)) + [("channels5", T(F32, *FRAME, 5)), ("empty", T(F32, 0, HEIGHT, WIDTH, 3))])
A_MOTION = kinds(MOTION, last=True) + [("rows0", T(F32, 0, 12))]
REPROJ_STOPS = [A("normal_min", 0.9, NAN), A("plane_max", None, 0.0), A("min_weight", 0.01, -1), A("alpha_min", 0.05, 2),
                A("alpha_mom_min", 0.2, -1), A("max_len", 32, 0), A("var_min_len", 4, 0.5), A("unknown", 1.0, "x"),
                A("albedo_floor", 1 / 256, 0.0), A("off", (0, 0), 5, (NAN, 0), ("('x', 0)", ("x", 0))), A("nonsense", OMIT, 1)]


def _upsample():
    lo, var_lo = T(F32, N_VIEWS, H_LO, W_LO, 3), T(F32, N_VIEWS, H_LO, W_LO)
    return fn("upsample", ("scene", "upsample"),
              [A("s", "query"),
               ("colour_lo", lo, kinds(lo, rank=(H_LO, W_LO, 3), rows=True) + [("channels5", T(F32, N_VIEWS, H_LO, W_LO, 5))]),
               ("hits", RECORDS, kinds(RECORDS, rank=(HEIGHT, WIDTH, 12), last=True, rows=True) + [("empty", T(F32, 0, HEIGHT, WIDTH, 12))]),
               A("factor", FACTOR, 0, 17, 1.5, True), A("phase", (0, 0), (2, 0), (0, -1), (0.5, 0), 1),
               TA("variance", var_lo, rows=True), A("normal_power", 128, 3), A("plane", None, 0.0), A("same_id", False, 1),
               A("demodulate", False, 1), A("modulate", False, "x"), A("albedo_floor", 1 / 256, 0.0),
               TA("out", COLOUR, given=False, last=True, rows=True), TA("variance_out", VARIANCE, given=False, rows=True),
               ("weight", False, kinds(VARIANCE, rows=True)), A("nonsense", OMIT, 1)],
              # inside the lattice of factor 16 and beyond the 9 x 13 frame
              extra=[("phase.beyond_x", dict(factor=16, phase=(WIDTH, 0))), ("phase.beyond_y", dict(factor=16, phase=(0, HEIGHT))),
                     ("variance_out.alone", dict(variance=None, variance_out=VARIANCE))])


def _prev_bad():
    """prev with one member of each bad kind, of the wrong length and of no length at all"""
    how = (("views_prev", dict(last=True, rows=True)), ("hits_prev", dict(last=True, rows=True)), ("history", dict(last=True, rows=True)))
    out = [(f"{name}.{tag}", PREV[:i] + (bad,) + PREV[i + 1:]) for i, (name, kw) in enumerate(how) for tag, bad in kinds(PREV[i], **kw)]
    return out + [("len2", PREV[:2]), ("len4", PREV + (HISTORY,)), ("5", 5)]


def _reproject(moving):
    """reproject() has no refusal for a variance_out without a variance (it hands out `unknown`), so there is no such case"""
    motion = TA("motion", MOTION, last=True) if moving else ("motion", None, A_MOTION)
    if moving:
        motion = (motion[0], motion[1], A_MOTION)
    return fn("reproject[motion]" if moving else "reproject", ("scene", "reproject"),
              [A("s", "query"), A_COLOUR, TA("hits", RECORDS, last=True, rows=True), ("prev", PREV, _prev_bad()),
               TA("variance", VARIANCE, rows=True), TA("out", HISTORY, given=False, last=True, rows=True),
               ("colour_out", True, kinds(COLOUR, last=True, rows=True)), ("variance_out", True, kinds(VARIANCE, rows=True)),
               ("coords", False, kinds(T(F32, *FRAME, 2), last=True, rows=True)), motion]
              # with a table the stops are the same code: one of them, the unknown keyword and the pair of numbers
              + (REPROJ_STOPS[:1] + REPROJ_STOPS[-2:] if moving else REPROJ_STOPS),
              # it names prev, so that it meets no other prev
              extra=[("out.is_history", dict(out=Same("prev", 2), prev=PREV))])


FUNCTIONS += [
    _upsample(), _reproject(False), _reproject(True),
    fn("Temporal", ("new", "Temporal"),
       [A("n_views", N_VIEWS, 0, 1.5, True), A("width", WIDTH, 0), A("height", HEIGHT, 0), A("channels", 3, 5)] + REPROJ_STOPS),
    # the reprojection needs no ray-query list, so a step on the other scene is a good call: scene= takes what is no Scene
    fn("Temporal.step", ("acc", "Temporal", "step"),
       [A("acc", "query"), TA("colour", COLOUR, rank=(HEIGHT, WIDTH, 3), last=True, rows=True), TA("hits", RECORDS, last=True, rows=True),
        TA("views", VIEWS, last=True, rows=True), TA("variance", VARIANCE, rows=True), ("motion", None, A_MOTION),
        A("scene", None, 7, "query")]),
    fn("Temporal.clone", ("acc", "Temporal", "clone"), [A("acc", "query")], zero=[("clone", {})]),
]
assert len({f["name"] for f in FUNCTIONS}) == len(FUNCTIONS)


# ----------------------------------------------------------------------------------------------------------- cases

def singles(f):
    """[(id, overrides, zero)]: the single cases of one function, in a fixed order"""
    out = [(f"{a[0]}.{tag}", {a[0]: val}, False) for a in f["args"] for tag, val in a[2]]
    out += [(tag, dict(ov), False) for tag, ov in f["extra"]]
    out += [(f"zero.{tag}", dict(ov), True) for tag, ov in f["zero"]]
    return out


def cases(f):
    """the single cases, then every unordered pair of them whose overrides touch different arguments.  Two zero-element
    cases are no pair: together they carry no refused argument more than each alone."""
    one = singles(f)
    out = list(one)
    for (ia, oa, za), (ib, ob, zb) in itertools.combinations(one, 2):
        if not (set(oa) & set(ob)) and not (za and zb):
            out.append((f"{ia}&{ib}", {**oa, **ob}, za or zb))
    return out


def table_digest(functions):
    return hashlib.sha1("\n".join(f"{f['name']}:{i}" for f in functions for i, _, _ in cases(f)).encode()).hexdigest()[:16]


# The recordings under tests/golden, each with the functions it holds.  The image filters and Temporal, which came after the first
# recording, have a file of their own, so that the first one stands as it was recorded, byte for byte.
RECORDINGS = {"py_refusals.json": FUNCTIONS[:-6], "py_refusals_filters.json": FUNCTIONS[-6:]}


# --------------------------------------------------------------------------------------------------------- calling

def describe(x):
    """shapes and dtypes of what a call returned"""
    if x is None or isinstance(x, (bool, int, float)):
        return repr(x)
    if isinstance(x, (tuple, list)):
        return "(" + ", ".join(describe(y) for y in x) + ")"
    if hasattr(x, "history"):                                            # a Temporal
        return f"Temporal(shape={list(x.shape)}, channels={x.channels}, frames={x.frames}, history={describe(x.history)})"
    if hasattr(x, "state"):                                              # an accumulator
        held = f", samples={x.samples}" if hasattr(x, "samples") else ""
        return f"{type(x).__name__}(state={describe(x.state)}{held})"
    return f"{str(x.dtype).replace('torch.', '')}{list(x.shape)}"


class Rig:
    """The two scenes of the fixture, their accumulators, and the tensors the cases pass."""

    def __init__(self, qr, blob):
        self.qr = qr
        self.scenes = {"query": qr.Scene(blob, ray_queries=True), "noquery": qr.Scene(blob)}
        assert self.scenes["query"].info.fsaa == 0
        self.made = {}
        views, views0 = self.make("views", VIEWS), self.make("views", VIEWS0)
        self.accs = {}
        for key, scn in self.scenes.items():
            self.accs[key] = {"PtViews": scn.pt_views(views, WIDTH, HEIGHT), "PtRays": scn.pt_rays(N_RAYS),
                              "PtAdaptive": scn.pt_adaptive(N_RAYS, 1, 4, 0.01),
                              "PtAdaptiveViews": scn.pt_adaptive_views(views, WIDTH, HEIGHT, 1, 4, 0.01)}
        scn = self.scenes["query"]
        self.accs["zero"] = {"PtViews": scn.pt_views(views0, WIDTH, HEIGHT), "PtRays": scn.pt_rays(0),
                             "PtAdaptive": scn.pt_adaptive(0, 1, 4, 0.01),
                             "PtAdaptiveViews": scn.pt_adaptive_views(views0, WIDTH, HEIGHT, 1, 4, 0.01)}
        self.accs["query"]["Temporal"] = scn.temporal(N_VIEWS, WIDTH, HEIGHT)

    def close(self):
        for s in self.scenes.values():
            s.close()

    def make(self, name, v):
        """one tensor per argument name and description: no case writes one, and no two arguments of a call share one"""
        if isinstance(v, tuple) and any(isinstance(x, T) for x in v):
            return tuple(self.make(f"{name}[{i}]", x) for i, x in enumerate(v))
        if not isinstance(v, T):
            return v
        key = (name,) + v.key()
        if key not in self.made:
            self.made[key] = v.make()
        return self.made[key]

    def call(self, f, over):
        """(type name, text) of one call of f with the overrides applied to the good call"""
        kw = {name: self.make(name, over.get(name, good)) for name, good, _ in f["args"]}
        kw = {k: kw[v.name][v.index] if isinstance(v, Same) else v for k, v in kw.items() if v is not OMIT}
        target = f["target"]
        try:
            if target[0] == "scene":
                got = getattr(self.scenes[kw.pop("s")], target[1])(**kw)
            elif target[0] == "new":
                got = getattr(self.qr, target[1])(self.scenes["query"], **kw)
            else:
                acc = self.accs[kw.pop("acc")][target[1]]
                got = getattr(acc, target[2])(**kw)
                if hasattr(acc, "samples"):                              # a call of no elements leaves them as they were
                    return ("ok", f"{describe(got)} held={acc.samples}")
            return ("ok", describe(got))
        except Exception as e:
            return (type(e).__name__, str(e))


def run(rig, visit, functions=FUNCTIONS):
    """Every case of every one of `functions`: visit(function, case id, outcome) right after each call.  A call that returns although it
    has elements ends the run at once."""
    for f in functions:
        for cid, over, zero in cases(f):
            got = rig.call(f, over)
            if got[0] == "ok" and not zero:
                raise AssertionError(f"{f['name']} {cid}: the case was not refused: {got}")
            visit(f["name"], cid, got)
