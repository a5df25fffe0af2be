"""Every entry point that takes a row stride, a batch stride or a table of frame numbers, run on frames that lie beyond 2^32 bytes, 2^31
elements and 2^32 elements from the pointer it is handed (tests/far_addr.py has the buffer and its poison).

The bar is the header's own sentence: results depend on the frames, not on stride or alignment.  So every call is made twice -- on the
far frames and on the same frames copied to a small dense buffer -- and the two results are compared BIT FOR BIT; after the far call
every byte of the 33 GiB allocation outside the cells the call may write is poison again.  The dense result is anchored so that the two
cannot be wrong together: tests/gmm_ref.py (long double) for llk / em_accumulate / tv_stats, the exact operands of tests/dgemm_ref.py for
the GEMM, numpy fp64 for the moments, the normalisation and gather / scatter on frames whose sums are exact (multiples of 1/4).

Two layouts.  WIDE ROWS: ldx = 2^22, so frame 256 (float32) / 128 (float64) starts at 2^32 bytes, frame 512 at 2^31 elements, frame 1024
(float32) at 2^32 elements; columns >= D of a row are poison.  FAR FRAMES: a dense ldx = D view whose tables name short runs below,
across and above each threshold and one run near frame 0 (a kernel that drops the high word of a frame number reads other DATA there
or poison); with D = 1 the frame numbers themselves pass 2^31 and 2^32.  Tables go in as host and as device arrays where both are
allowed.  An entry point whose output is indexed like its input (the rewriters) cannot have a dense output for far frame NUMBERS: in
that layout it runs in place; the wide-rows layout has all three modes (far -> dense, dense -> far through ldo, in place).
gmmiv_feat_compensate and gmmiv_feat_map take (x, T, ldx) and no table of frame numbers, so they run in the wide-rows layout only: a dense
view of far frames would reach them as a pointer offset computed by the caller, which is no arithmetic of the library's.

What the allocation bounds.  The guard below a window (2^31 float64 elements) and the window share 34 GiB at most, so: a float64 far
output holds 544 rows, and float32 frames go into it from the first 544 of them (the 1056 go far into a float32 output); batch strides and model strides of 2^31 + 8
doubles are run with two matrices / models (a third would start 32 GiB above the window); gmmiv_score_normalize, which has no ld, runs
on a contiguous 2 x (2^30 + 2) matrix whose last elements lie past 2^31 doubles.

Entry points that are not layout-independent by the header's words are judged by those words: gmmiv_tv_stats on <= 16 utterances
("tv_stats_split": the order depends on how many utterances share the call -- both calls share the same table, so bitwise holds);
the *_models statistics depend on their segment's place in its 16-frame block (gmmiv_plan_model_tiles: "a segment cannot be shifted
inside its blocks"), so the dense twin keeps every first frame modulo 64.
"""
import contextlib

import numpy as np
import pytest

import far_addr as fa
import gmm_ref as gr
from conftest import make_frames, make_gmm

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

F32, F64 = np.float32, np.float64
DTYPES = (F32, F64)
SHAPES = ((64, 20), (24, 96))       # (C, D): the MFMA paths; the generic D > 80 kernels
DEFAULTS = {"stats_z": 1, "topc_fused": 1, "topc_z": 1, "topc_use_lanes": 4}
LO, HI = -1e9, 1e9
WORKSPACE = {}                      # what the summary reports: gmmiv_ctx_workspace_bytes around feat_norm_online with a device table


def name_of(dtype):
    return np.dtype(dtype).name


@pytest.fixture(scope="module")
def far():
    import torch
    assert torch.cuda.is_available()
    fb = fa.FarBuffer()
    yield fb
    print("far buffer: %d bytes allocated, %d far calls swept" % (fa.ALLOC_BYTES, fb.calls))
    print("feat_norm_online with a device file_begin on wide rows, workspace bytes of the context before / after: %s" % sorted(WORKSPACE.items()))
    fb.close()


@pytest.fixture(scope="module")
def ctx():
    import torch
    from lia_ral_amd import capi
    c = capi.Context(0, torch.cuda.current_stream().cuda_stream)      # torch's stream: the fixture's copies and the calls are ordered
    yield c
    c.close()


@contextlib.contextmanager
def options(ctx, opts):
    """set, run, restore (as test_gpu_gmm_elementwise.options)"""
    try:
        for k, v in opts.items():
            prev = ctx.set_option(k, v)
            assert prev == DEFAULTS[k], "option %s was %r, expected the default %r" % (k, prev, DEFAULTS[k])
        yield
    finally:
        for k, v in opts.items():
            back = ctx.set_option(k, DEFAULTS[k])
            assert back == v, "option %s read back %r after it was set to %r" % (k, back, v)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def filled(shape, dtype):
    """a dense device array that starts as the far buffer does: poison"""
    import torch
    return torch.full(tuple(shape), fa.POISON[dtype], dtype=fa.tdtype(dtype), device="cuda")


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def same(what, got, want):
    """dicts, tuples and arrays, bit for bit"""
    if isinstance(want, dict):
        assert set(got) == set(want), what
        for k in want:
            same("%s [%s]" % (what, k), got[k], want[k])
    elif isinstance(want, (tuple, list)):
        assert len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            same("%s [%d]" % (what, i), g, w)
    elif want is None or np.isscalar(want):
        assert got == want, "%s: far %r, dense %r" % (what, got, want)
    else:
        fa.same_bits(what, host(got), host(want))


def exact_frames(n, D, dtype, seed):
    """multiples of 1/4 in [-10, 10]: sums of values and of squares are exact in fp64, and 1/4-steps never meet the poison"""
    return (np.random.default_rng([seed, n, D]).integers(-40, 41, (n, D)) / 4.0).astype(dtype)


_MODELS = {}


def model(C, D, shift=0):
    key = (C, D, shift)
    if key not in _MODELS:
        w, mean, iv = make_gmm(C, D, seed=C + D)
        if shift:
            mean = mean + np.random.default_rng(shift).normal(0.0, 0.1, mean.shape)
        _MODELS[key] = (w, mean, iv)
    return _MODELS[key]


def gmm_frames(C, D, T, dtype):
    return make_frames(*model(C, D), T, seed=T + C, dtype=dtype)


# ================================================================================================ GMM side, wide rows
def utt_bounds(T):
    """utterances that cut 16-frame blocks and end on, before and after the threshold frames; an empty one among them"""
    marks = (0, 5, 5, 127, 130, 255, 256, 300, 511, 513, 700, 1023, 1024, 1025, T - 7, T)
    return np.array(sorted(b for b in marks if b <= T), np.int64)


def gmm_entries(ctx, C, D, T, dense_x):
    """{name: fn(x) -> arrays}, the paths that reach each entry, and the handles to close"""
    g = ctx.gmm(*model(C, D))
    clients = [ctx.gmm(*model(C, D, s)) for s in (5, 6, 7)]
    ub = utt_bounds(T)
    fb = np.ascontiguousarray(ub[::2])              # files: every other bound; the frames behind the last one belong to no file
    nfiles = len(fb) - 1
    lines = [[0, 2], [1], list(range(nfiles)), [nfiles - 1, 0]]
    ctop = 10
    top = g.llk_determine_top(dense_x, ctop, True, LO, HI)        # the world's selection, from the dense frames, for USE_TOP_DISTRIBS

    def llk(x):
        sums = np.zeros(2)
        return {"llk": g.llk(x, LO, HI, sums=sums), "sums": sums}

    def tv(x):
        return g.tv_stats(x, ub)

    E = {
        "llk": llk,
        "occ": lambda x: g.occ(x),
        "em_accumulate": lambda x: g.em_accumulate(x),
        "tv_stats": tv,
        "tv_stats_lines": lambda x: g.tv_stats_lines(x, fb, lines),
        "llk_determine_top": lambda x: g.llk_determine_top(x, ctop, True, LO, HI),
        "llk_determine_top partial": lambda x: g.llk_determine_top(x, ctop, False, LO, HI),
        "llk_use_top": lambda x: clients[0].llk_use_top(x, top["idx"], top["nontop_llk"], True, LO, HI),
        "llk_use_top_multi": lambda x: type(g).llk_use_top_multi(clients, x, top["idx"], top["nontop_llk"], True, LO, HI),
        "topgauss_compute count": lambda x: g.topgauss_compute(x, ctop, 5.0, True, LO, HI),
        "topgauss_compute mass": lambda x: g.topgauss_compute(x, ctop, 0.9, True, LO, HI),
    }
    stats = ("em_accumulate", "tv_stats", "tv_stats_lines")
    tops = ("llk_determine_top", "llk_determine_top partial", "topgauss_compute count", "topgauss_compute mass")
    paths = [("defaults", {}, tuple(E)), ("stats_z 0", {"stats_z": 0}, stats), ("topc_fused 0", {"topc_fused": 0}, tops),
             ("topc_fused 0 topc_z 0", {"topc_fused": 0, "topc_z": 0}, tops), ("topc_use_lanes 1", {"topc_use_lanes": 1}, ("llk_use_top", "llk_use_top_multi"))]
    return E, paths, [g] + clients, ub


@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_gmm_side_on_wide_rows(far, ctx, shape, dtype):
    from test_gpu_gmm_elementwise import Judge, check_acc
    assert gr.HAVE_LONGDOUBLE, gr.SKIP_MESSAGE
    C, D = shape
    T = fa.WIDE_T[dtype]
    X = gmm_frames(C, D, T, dtype)
    xd, v = dev(X), far.wide(dtype, D)
    assert v.stride(0) == fa.WIDE_LD and v.shape == (T, D)
    E, paths, handles, ub = gmm_entries(ctx, C, D, T, xd)
    label = "%dx%d %s wide rows" % (C, D, name_of(dtype))
    dense = {}
    for path, opts, entries in paths:
        with options(ctx, opts):
            for e in entries:
                want = E[e](xd)
                dense[path, e] = want
                got, _ = far.run("%s | %s | %s" % (label, path, e), lambda: E[e](v), inputs=[(v, X)])
                same("%s | %s | %s" % (label, path, e), got, want)
    # the anchor: the dense results against the long double reference, under the bars of the elementwise module
    ref = gr.Reference(*model(C, D), X)
    j = Judge(label, "defaults")
    j("llk", "(t)", dense["defaults", "llk"]["llk"], ref.llk, ref.B)
    check_acc(j, "em w=1", handles[0], dense["defaults", "em_accumulate"], ref, (1.0,))
    j.path = "stats_z 0"
    check_acc(j, "em w=1", handles[0], dense["stats_z 0", "em_accumulate"], ref, (1.0,))
    Nr, Fr, Nb, Fb = ref.utt_stats(ub)
    for path in ("defaults", "stats_z 0"):
        j.path = path
        N, F = dense[path, "tv_stats"]
        j("tv N", "(u, c)", N, Nr, Nb)
        j("tv F", "(u, c, d)", F.reshape(Fr.shape), Fr, Fb)
    j.finish()
    for h in handles:
        h.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
def test_frame_moments_and_the_unusable_count_on_wide_rows(far, ctx, dtype):
    D, T = 20, fa.WIDE_T[dtype]
    X = exact_frames(T, D, dtype, 1)
    v = far.wide(dtype, D)
    label = "%s wide rows" % name_of(dtype)
    got, _ = far.run(label + " | frame_moments", lambda: ctx.frame_moments(v), inputs=[(v, X)])
    same(label + " | frame_moments", got, ctx.frame_moments(dev(X)))
    x64 = X.astype(F64)
    fa.same_bits(label + " | frame_moments against numpy (exact sums)", got, np.concatenate([x64.sum(0), (x64 * x64).sum(0), [float(T)]]))
    # unusable values planted on both sides of every threshold frame: a count is only right when the right frames were read
    B = X.copy()
    planted = [t for t in (0, 127, 128, 255, 256, 300, 511, 512, 513, 1023, 1024, 1055) if t < T]
    for i, t in enumerate(planted):
        B[t, (3 * i) % D] = (np.nan, np.inf, -np.inf, 1e30)[i % 4]
    got, _ = far.run(label + " | count_unusable_frames", lambda: ctx.count_unusable_frames(v), inputs=[(v, B)])
    assert got == len(planted) == ctx.count_unusable_frames(dev(B)), (label, got, len(planted))


# ================================================================================================ frame movers and rewriters
WIDE_RUNS = ((2, 9), (120, 13), (250, 11), (505, 13), (520, 9), (1017, 13), (1040, 11))     # (first frame, length): across frames 128, 256, 512, 1024


def wide_runs(T):
    return [r for r in WIDE_RUNS if r[0] + r[1] <= T]


def group_table(runs, groups):
    """[nrun, 3] (first frame, length, group): group ids non-decreasing"""
    return np.array([(f, n, g) for (f, n), g in zip(runs, groups)], np.int64).reshape(-1, 3)


def groups_of(n):
    return [min(i // 2, (n - 1) // 2) for i in range(n)]      # two runs per group / file


class Frames:
    """one data set in its far and its dense form: far cells + dense device matrix + the run firsts of each"""

    def __init__(self, far, dtype, D, layout, seed=0, T=None):
        self.far, self.dtype, self.D, self.layout = far, dtype, D, layout
        if layout == "wide":
            T = fa.WIDE_T[dtype] if T is None else T        # fewer frames: what a far output of the wider dtype can hold
            self.X = exact_frames(T, D, dtype, seed)
            self.runs_far = self.runs_dense = wide_runs(T)
            self.T_far = self.T_dense = T
            self.view = far.wide(dtype, D, T)
            self.cells = [self.view]
            self.data = [self.X]
            self.dense0 = self.X
        else:
            self.runs_far, self.T_far = fa.far_runs(dtype, D)
            self.runs_dense, self.T_dense = fa.compact(self.runs_far)
            self.view = far.dense(dtype, D, self.T_far)
            self.data = [exact_frames(n, D, dtype, seed + 1 + i) for i, (f, n) in enumerate(self.runs_far)]
            self.cells = [self.view[f:f + n] for f, n in self.runs_far]
            self.dense0 = np.full((self.T_dense, D), fa.POISON[dtype], dtype)
            for (f, n), d in zip(self.runs_dense, self.data):
                self.dense0[f:f + n] = d
        self.lens = [n for f, n in self.runs_far]
        self.firsts_far = [f for f, n in self.runs_far]
        self.firsts_dense = [f for f, n in self.runs_dense]

    def inputs(self):
        return list(zip(self.cells, self.data))

    def dense(self):
        return dev(self.dense0)

    def run_rows(self, a, firsts):
        """the frames of the runs, run by run, of a host matrix indexed like the frames"""
        return [a[f:f + n] for f, n in zip(firsts, self.lens)]

    def read(self, what, fn, tables=("host", "device")):
        """fn(x, firsts, tab): an entry point that only READS the frames; tab turns a host table into the form under test.  Far against
        dense for every table form -> the dense result"""
        want = fn(self.dense(), self.firsts_dense, np.asarray)
        for form in tables:
            tab = dev if form == "device" else np.asarray
            got, _ = self.far.run("%s | %s tables" % (what, form), lambda: fn(self.view, self.firsts_far, tab), inputs=self.inputs())
            same("%s | %s tables" % (what, form), got, want)
        return want

    def rewrite_in_place(self, what, fn, tables=("host", "device")):
        """fn(x, out, firsts, tab) with out == x: the run cells are inputs and outputs -> (dense result rows per run, fn's dense return)"""
        xd = self.dense()
        ret = fn(xd, xd, self.firsts_dense, np.asarray)
        want = host(xd)
        for form in tables:
            tab = dev if form == "device" else np.asarray
            got_ret, got = self.far.run("%s | in place | %s tables" % (what, form), lambda: fn(self.view, self.view, self.firsts_far, tab), inputs=self.inputs(),
                                        outputs=self.cells)
            if self.layout == "wide":
                same("%s | in place | %s tables" % (what, form), got[0], want)
            else:
                same("%s | in place | %s tables" % (what, form), got, self.run_rows(want, self.firsts_dense))
            same("%s | in place | %s tables | returned" % (what, form), got_ret, ret)
        return want, ret

    def rewrite_across(self, what, fn, odtype, tables=("host",)):
        """wide rows only: far frames into a dense output, dense frames into a far output (ldo = 2^22) -> the dense output.  A float64 far
        output holds 544 rows: the tests run float32 frames into it from a Frames of T = 544 (short()), the 1056 go into float32 only."""
        assert self.layout == "wide"
        T, D = self.T_far, self.D
        out0 = filled((T, D), odtype)
        ret = fn(self.dense(), out0, self.firsts_dense, np.asarray)
        want = host(out0)
        vo = self.far.wide(odtype, D, T) if T <= fa.WIDE_T[odtype] else None
        for form in tables:
            tab = dev if form == "device" else np.asarray
            out = filled((T, D), odtype)
            got_ret, _ = self.far.run("%s | far -> dense %s | %s tables" % (what, name_of(odtype), form), lambda: fn(self.view, out, self.firsts_far, tab),
                                      inputs=self.inputs())
            same("%s | far -> dense %s | %s tables" % (what, name_of(odtype), form), out, want)
            same("%s | far -> dense | returned" % what, got_ret, ret)
            if vo is None:
                continue
            xd = self.dense()
            got_ret, got = self.far.run("%s | dense -> far %s | %s tables" % (what, name_of(odtype), form), lambda: fn(xd, vo, self.firsts_dense, tab), outputs=[vo])
            same("%s | dense -> far %s | %s tables" % (what, name_of(odtype), form), got[0], want)
            same("%s | dense -> far | returned" % what, got_ret, ret)
        return want, ret


LAYOUTS = (("wide", F32, 20), ("wide", F64, 20), ("far", F32, 1), ("far", F32, 20), ("far", F64, 20))
LAYOUT_IDS = ["%s-%s-D%d" % (l, name_of(t), d) for l, t, d in LAYOUTS]


def short(far, fr, seed=0):
    """the first 544 float32 frames of the wide-rows layout: what goes, dense -> far, into a float64 far output (None when there is no such case)"""
    if fr.layout != "wide" or fr.dtype != F32:
        return None
    return Frames(far, F32, fr.D, "wide", seed=seed, T=fa.WIDE_T[F64])


@pytest.mark.parametrize("layout,dtype,D", LAYOUTS, ids=LAYOUT_IDS)
def test_gather_and_scatter(far, ctx, layout, dtype, D):
    fr = Frames(far, dtype, D, layout)
    label = "%s %s D=%d" % (layout, name_of(dtype), D)
    nrow = sum(fr.lens)
    rows = np.concatenate([[0], np.cumsum(fr.lens)])[:-1]
    expect = np.concatenate(fr.data) if layout == "far" else np.concatenate(fr.run_rows(fr.X, fr.firsts_far))

    def frames(x, firsts, tab):
        idx = np.concatenate([np.arange(f, f + n) for f, n in zip(firsts, fr.lens)])[::-1].astype(np.int64)       # descending: not a run
        return ctx.gather_frames(x, tab(idx), filled((nrow, D), dtype))

    def runs(x, firsts, tab):
        return ctx.gather_runs(x, tab(np.array([(f, r, n) for f, r, n in zip(firsts, rows, fr.lens)], np.int64)), filled((nrow, D), dtype))

    fa.same_bits(label + " | gather_frames against numpy", host(fr.read(label + " | gather_frames", frames)), expect[::-1])
    fa.same_bits(label + " | gather_runs against numpy", host(fr.read(label + " | gather_runs", runs)), expect)
    # scatter: a dense matrix of other values goes back to the far frames; nothing else of the buffer changes
    src = exact_frames(nrow, D, dtype, 77)

    def scatter(x, out, firsts, tab):
        ctx.scatter_runs(out, tab(np.array([(f, r, n) for f, r, n in zip(firsts, rows, fr.lens)], np.int64)), dev(src))

    want, _ = fr.rewrite_in_place(label + " | scatter_runs", scatter)
    fa.same_bits(label + " | scatter_runs against numpy", np.concatenate(fr.run_rows(want, fr.firsts_dense)), src)
    if layout != "far":
        return
    # the other side of the table: the ROW numbers (dst) of the compact matrix are far -- out of gather_runs / in of scatter_runs is the
    # far view (ld = D), the frames are a small dense matrix; with D = 1 float32 the row numbers pass 2^31 and 2^32
    for form, tab in (("host", np.asarray), ("device", dev)):
        table = tab(np.array([(r, f, n) for r, f, n in zip(rows, fr.firsts_far, fr.lens)], np.int64))
        what = "%s | gather_runs into far rows | %s tables" % (label, form)
        _, got = far.run(what, lambda: ctx.gather_runs(dev(src), table, fr.view), outputs=fr.cells)
        fa.same_bits(what + " against numpy", np.concatenate(got), src)
        what = "%s | scatter_runs from far rows | %s tables" % (label, form)
        back = filled((nrow, D), dtype)
        far.run(what, lambda: ctx.scatter_runs(back, table, fr.view), inputs=fr.inputs())
        fa.same_bits(what + " against numpy", host(back), expect)


@pytest.mark.parametrize("layout,dtype,D", LAYOUTS, ids=LAYOUT_IDS)
def test_moments_groups_and_norm_apply(far, ctx, layout, dtype, D):
    fr = Frames(far, dtype, D, layout)
    label = "%s %s D=%d" % (layout, name_of(dtype), D)
    moments_and_apply(ctx, fr, label, DTYPES)
    if short(far, fr) is not None:
        moments_and_apply(ctx, short(far, fr), label + " first 544 frames", (F64,), across_only=True)


def moments_and_apply(ctx, fr, label, odtypes, across_only=False):
    layout, dtype, D = fr.layout, fr.dtype, fr.D
    grp = groups_of(len(fr.lens))
    ng = grp[-1] + 1
    rows = fr.run_rows(fr.dense0.astype(F64), fr.firsts_dense)
    want = np.zeros((ng, 2 * D + 1))
    for r, g in zip(rows, grp):
        want[g] += np.concatenate([r.sum(0), (r * r).sum(0), [len(r)]])
    if not across_only:
        acc = fr.read(label + " | frame_moments_groups", lambda x, firsts, tab: ctx.frame_moments_groups(x, tab(group_table(zip(firsts, fr.lens), grp)), ng))
        fa.same_bits(label + " | frame_moments_groups against numpy (exact sums)", acc, want)
    mean, std = (want[:, :D] / want[:, -1:]), np.sqrt(np.maximum(want[:, D:2 * D] / want[:, -1:] - (want[:, :D] / want[:, -1:]) ** 2, 0.25))

    def apply(x, out, firsts, tab):
        ctx.feat_norm_apply(x, tab(group_table(zip(firsts, fr.lens), grp)), tab(mean) if tab is dev else mean, tab(std) if tab is dev else std, out=out)

    def numpy_apply(odtype):
        return [((r - mean[g]) / std[g]).astype(odtype) for r, g in zip(rows, grp)]

    if not across_only:
        got, _ = fr.rewrite_in_place(label + " | feat_norm_apply", apply)
        same(label + " | feat_norm_apply in place against numpy", fr.run_rows(got, fr.firsts_dense), numpy_apply(dtype))
    if layout == "wide":
        for odtype in odtypes:
            got, _ = fr.rewrite_across(label + " | feat_norm_apply", apply, odtype, tables=("host", "device"))
            same(label + " | feat_norm_apply against numpy", fr.run_rows(got, fr.firsts_dense), numpy_apply(odtype))


@pytest.mark.parametrize("layout,dtype,D", LAYOUTS, ids=LAYOUT_IDS)
def test_online_and_windowed_normalisation(far, ctx, layout, dtype, D):
    from lia_ral_amd import capi
    fr = Frames(far, dtype, D, layout)
    label = "%s %s D=%d" % (layout, name_of(dtype), D)
    # online mode: files = contiguous frame ranges.  Wide rows: the whole matrix as files that end on and around the threshold frames,
    # host and DEVICE file_begin (the scratch of the scan is then sized from the allocation that holds x: 33 GiB, read by rows of 2^22).
    # Far frames: one call per run (a file), host table only -- a device table would size the scratch from 2^32 frames.
    if layout == "wide":
        def online_of(f):
            T = f.T_far
            fb = np.array([b for b in (0, 40, 40, 129, 256, 300, 512, 515, 1024, 1030) if b < T] + [T], np.int64)

            def online(x, out, firsts, tab):
                watch = tab is dev and x is fr.view and x is out
                if watch:
                    WORKSPACE.setdefault((name_of(dtype), "before"), sum(ctx.workspace_bytes(s) for s in range(64)))
                ctx.feat_norm_online(x, tab(fb), window=30, look_ahead=7, out=out)
                if watch:
                    WORKSPACE[name_of(dtype), "after"] = sum(ctx.workspace_bytes(s) for s in range(64))
            return online

        fr.rewrite_in_place(label + " | feat_norm_online", online_of(fr))
        for odtype in DTYPES:
            fr.rewrite_across(label + " | feat_norm_online", online_of(fr), odtype, tables=("host", "device"))
        fs = short(far, fr)
        if fs is not None:
            fs.rewrite_across(label + " first 544 frames | feat_norm_online", online_of(fs), F64, tables=("host", "device"))
    else:
        def online(x, out, firsts, tab):
            for f, n in zip(firsts, fr.lens):
                ctx.feat_norm_online(x, np.array([f, f + n // 2, f + n], np.int64), window=5, look_ahead=2, out=out)

        fr.rewrite_in_place(label + " | feat_norm_online", online, tables=("host",))
    # windowed mode: the schedule is planned once, on the dense table (begins are counted from the file's first frame, so it is the same
    # schedule), and the steps name runs by their index
    grp = groups_of(len(fr.lens))
    nf = grp[-1] + 1
    dense_tab = group_table(zip(fr.firsts_dense, fr.lens), grp)
    first = np.array([min(f for f, g in zip(fr.firsts_dense, grp) if g == k) for k in range(nf)], np.int64)
    off, steps, alpha = capi.plan_norm_windows(dense_tab, nf, first, 0.15, 1.0, 0.01)
    assert len(alpha) >= 1

    def window(x, out, firsts, tab):
        return ctx.feat_norm_window(x, tab(group_table(zip(firsts, fr.lens), grp)), nf, tab(off), tab(steps), dev(alpha) if tab is dev else alpha,
                                    gstat=dev(np.zeros((nf, 2 * D))) if tab is dev else None, step_stat=dev(np.zeros((len(alpha), 2 * D))) if tab is dev else None)

    fr.rewrite_in_place(label + " | feat_norm_window", window)


@pytest.mark.parametrize("layout,dtype,D", LAYOUTS, ids=LAYOUT_IDS)
def test_energy_detector_and_turn_curve(far, ctx, layout, dtype, D):
    from lia_ral_amd import capi
    fr = Frames(far, dtype, D, layout, seed=5)
    label = "%s %s D=%d" % (layout, name_of(dtype), D)
    grp = groups_of(len(fr.lens))
    nf = grp[-1] + 1

    def energy(x, firsts, tab):
        runs = tab(group_table(zip(firsts, fr.lens), grp))
        col = x[:, 0:1]                                     # the energy column: a pointer offset with the full stride
        out = [dev(np.zeros((nf, 9))), dev(np.zeros(nf)), dev(np.zeros(nf, np.int32))] if tab is dev else [None, None, None]
        m, th, st = ctx.energy_train(col, runs, nf, C=3, nb_train_it=4, model=out[0], threshold=out[1], status=out[2])
        th_h = host(th)
        thr = np.where(np.isfinite(th_h), th_h, 0.0)
        above, cnt = ctx.energy_select(col, runs, nf, thr)
        so = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        sb, sl = np.zeros(int(so[-1]), np.int64), np.zeros(int(so[-1]), np.int64)
        if tab is dev:
            a2, c2, sb, sl = ctx.energy_select(col, runs, nf, dev(thr), seg_off=dev(so), seg_begin=dev(sb), seg_len=dev(sl), n_above=dev(above), seg_count=dev(cnt))
        else:
            a2, c2, sb, sl = ctx.energy_select(col, runs, nf, thr, seg_off=so, seg_begin=sb, seg_len=sl)
        return {"model": m, "threshold": th, "status": st, "above": above, "count": cnt, "above2": a2, "count2": c2, "seg_begin": sb, "seg_len": sl}

    r = fr.read(label + " | energy_train / energy_select", energy)
    assert host(r["above"]).sum() > 0 and host(r["count"]).sum() > 0, "the selection is empty: the case checks nothing"

    W, S = 4, 2
    po = capi.plan_turn_positions(group_table(zip(fr.firsts_dense, fr.lens), grp), nf, W, S)
    npos = int(po[-1])
    assert npos >= len(fr.lens)

    def turn(x, firsts, tab):
        runs = tab(group_table(zip(firsts, fr.lens), grp))
        if tab is dev:
            return ctx.turn_curve(x, runs, nf, dev(po), W, S, "GLR", LO, HI, value=dev(np.zeros(npos)), status=dev(np.zeros(npos, np.int32)), npos=npos)
        return ctx.turn_curve(x, runs, nf, po, W, S, "GLR", LO, HI)

    v, st = fr.read(label + " | turn_curve", turn)
    assert np.isfinite(host(v)).sum() > npos // 2, "most positions have no value: the case checks nothing"


@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
def test_feat_compensate_and_feat_map_on_wide_rows(far, ctx, dtype):
    C, D = 64, 20
    T = fa.WIDE_T[dtype]
    fr = Frames(far, dtype, D, "wide")
    fr.X = gmm_frames(C, D, T, dtype)
    fr.data, fr.dense0 = [fr.X], fr.X
    fs = short(far, fr)
    if fs is not None:
        fs.X = fr.X[:fs.T_far]
        fs.data, fs.dense0 = [fs.X], fs.X
    w, mean, iv = model(C, D)
    g = ctx.gmm(w, mean, iv)
    rng = np.random.default_rng(3)
    offset = rng.normal(0.0, 0.3, (C, D))
    ci_mean, ci_cov = mean + rng.normal(0.0, 0.1, (C, D)), (1.0 / iv) * np.exp(rng.normal(0.0, 0.1, (C, D)))
    label = "%s wide rows" % name_of(dtype)

    def comp(x, out, firsts, tab):
        g.feat_compensate(x, offset, out=out)

    def fmap(x, out, firsts, tab):
        return g.feat_map(mean, 1.0 / iv, ci_mean, ci_cov, x, out=out)[1]

    for path, opts in (("defaults", {}), ("stats_z 0", {"stats_z": 0})):
        with options(ctx, opts):
            fr.rewrite_in_place("%s | %s | feat_compensate" % (label, path), comp, tables=("host",))
            for odtype in DTYPES:
                fr.rewrite_across("%s | %s | feat_compensate" % (label, path), comp, odtype)
            if fs is not None:
                fs.rewrite_across("%s first 544 frames | %s | feat_compensate" % (label, path), comp, F64)
    for path, opts in (("defaults", {}), ("topc_fused 0", {"topc_fused": 0}), ("topc_fused 0 topc_z 0", {"topc_fused": 0, "topc_z": 0})):
        with options(ctx, opts):
            fr.rewrite_in_place("%s | %s | feat_map" % (label, path), fmap, tables=("host",))
            for odtype in DTYPES:
                fr.rewrite_across("%s | %s | feat_map" % (label, path), fmap, odtype)
            if fs is not None:
                fs.rewrite_across("%s first 544 frames | %s | feat_map" % (label, path), fmap, F64)
    g.close()


# ================================================================================================ batched models and trials
def seg_groups(dtype, D):
    """contiguous segment tables: one group near frame 0 and one around the frame that holds each threshold element -- a segment that ends
    below it, one that straddles it, an empty one and one above it.  The gaps between the groups belong to no segment, so a group is a
    call (frames before seg_begin[0] and from seg_begin[nseg] on are not read and their outputs are not touched)."""
    out = [np.array([3, 20, 37, 37, 60], np.int64)]
    for e in fa.THRESHOLDS[dtype]:
        f = e // D
        out.append(np.array([f - 40, f - 9, f + 8, f + 8, f + 30], np.int64))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
def test_batched_models_and_trials_on_far_segments(far, ctx, dtype):
    import torch
    C, D, G = 64, 20, 3
    w, mean, iv = model(C, D)
    means = np.stack([model(C, D, s)[1] for s in (0, 5, 6)])
    b = ctx.gmm_batch(G, C, D).load(w, means, iv)
    world = ctx.gmm(w, mean, iv)
    offsets = np.random.default_rng(4).normal(0.0, 0.3, (G, C, D))
    seg_model = np.array([2, 0, 1, 1], np.int32)
    trial_seg, trial_model = np.array([0, 0, 1, 3, 3, 2], np.int32), np.array([0, 1, 2, 0, 2, 1], np.int32)
    label = "far segments %s" % name_of(dtype)
    paths = (("defaults", {}), ("stats_z 0", {"stats_z": 0}), ("topc_fused 0", {"topc_fused": 0}), ("topc_fused 0 topc_z 0", {"topc_fused": 0, "topc_z": 0}),
             ("topc_use_lanes 1", {"topc_use_lanes": 1}))
    for sb in seg_groups(dtype, D):
        lo, hi = int(sb[0]), int(sb[-1])
        n = hi - lo
        X = gmm_frames(C, D, n, dtype)
        shift = lo - lo % 64                              # the dense twin keeps every frame number modulo 64
        sbd = sb - shift
        xd0 = np.full((int(sbd[-1]), D), fa.POISON[dtype], dtype)
        xd0[int(sbd[0]):] = X
        view = far.dense(dtype, D, hi)
        cells = view[lo:hi]

        def entries(x, s, T):
            sent = torch.full((T,), -7.5, dtype=torch.float64, device="cuda")
            llk, seg_sum = b.llk(x, s, seg_model, LO, HI, out=sent)
            assert bool((llk[:int(s[0])] == -7.5).all()), "llk_models wrote before the first segment"
            r = {"llk": host(llk[int(s[0]):]), "seg_sum": seg_sum}
            r["tv"] = b.tv_stats(x, s, seg_model)
            r["em"] = b.em_stats(x, s, seg_model)
            r["trials"] = b.llr_trials(world, x, s, trial_seg, trial_model, 10, True, LO, HI)
            return r

        def compensate(x, s):
            b.feat_compensate(x, s, seg_model, offsets, out=x)

        for path, opts in paths:
            what = "%s | frames %d .. %d | %s" % (label, lo, hi, path)
            with options(ctx, opts):
                want = entries(dev(xd0), sbd, int(sbd[-1]))
                got, _ = far.run(what, lambda: entries(view, sb, hi), inputs=[(cells, X)])
                same(what, got, want)
                if path in ("defaults", "stats_z 0"):
                    xd = dev(xd0)
                    compensate(xd, sbd)
                    _, got = far.run(what + " | feat_compensate_models in place", lambda: compensate(view, sb), inputs=[(cells, X)], outputs=[cells])
                    same(what + " | feat_compensate_models in place", got[0], host(xd)[int(sbd[0]):])
        # the anchor: the dense per-frame values under each segment's own model
        j = []
        for s in range(4):
            a, e = int(sbd[s]) - int(sbd[0]), int(sbd[s + 1]) - int(sbd[0])
            if e > a:
                ref = gr.Reference(w, means[seg_model[s]], iv, X[a:e])
                err = gr.ratio(want["llk"][a:e].astype(gr.LD) - ref.llk, ref.B)
                if err.max() > 1.0:
                    j.append("segment %d: llk_models off its reference by %.3g bars" % (s, err.max()))
        assert not j, what + "\n" + "\n".join(j)
    world.close()
    b.close()


def test_model_tables_with_strides_beyond_2_31(far, ctx):
    """gmmiv_gmm_batch_load with mean_stride = 2^31 + 8 and gmmiv_map_adapt_models with cur_stride = 2^31 + 8: model 1 starts past 2^31
    doubles.  Two models: a third would start 32 GiB above the window, outside an allocation that also holds the guard."""
    C, D, G = 64, 20, 2
    stride = (1 << 31) + 8
    w, mean, iv = model(C, D)
    means = np.stack([model(C, D, s)[1] for s in (5, 6)]).reshape(G, C * D)
    view = far.view(F64, (G, C * D), (stride, 1))
    T = 300
    X = gmm_frames(C, D, T, F32)
    sb, sm = np.array([0, 140, T], np.int64), np.array([1, 0], np.int32)
    want_b = ctx.gmm_batch(G, C, D).load(w, means, iv)
    want = want_b.llk(X, sb, sm, LO, HI)
    got_b = ctx.gmm_batch(G, C, D)
    wd, ivd = dev(w), dev(iv)
    far.run("gmm_batch_load mean_stride 2^31 + 8", lambda: got_b.load(wd, view, ivd, strides=(0, stride, 0)), inputs=[(view, means)])
    same("gmm_batch_load mean_stride 2^31 + 8: llk_models of the loaded batch", got_b.llk(X, sb, sm, LO, HI), want)
    same("gmm_batch_load mean_stride 2^31 + 8: packed model 1", got_b.packed(1), want_b.packed(1))
    # cur_mean is read only for a Gaussian WITHOUT occupancy (N = 0 exactly; a posterior is tiny but never 0), and under MAPOccDep such a
    # Gaussian gets a = 0 and the a-priori mean whatever cur_mean holds.  So some Gaussians of both models lose their statistics and the
    # method is MAPConst: their means are 0.75 mean0 + 0.25 cur_mean[g], which for model 1 lies 2^31 + 8 doubles from the pointer.
    N, F, seg_llk = want_b.tv_stats(X, sb, sm)
    empty = [3, 17, 40, 63]
    N[:, empty] = 0.0
    F.reshape(G, C, D)[:, empty, :] = 0.0
    assert (np.delete(N, empty, axis=1) > 0).all()
    Nd, Fd, cnt = dev(N), dev(F), dev(np.ascontiguousarray(seg_llk[:, 1]))
    kw = dict(method="MAPConst", alpha_mean=0.75)
    want = want_b.map_adapt(Nd, Fd, cnt, w, mean, dev(means), **kw)
    got, _ = far.run("map_adapt_models cur_stride 2^31 + 8", lambda: want_b.map_adapt(Nd, Fd, cnt, w, mean, view, cur_stride=stride, **kw), inputs=[(view, means)])
    same("map_adapt_models cur_stride 2^31 + 8", got, want)
    got_means = host(got[0]).reshape(G, C, D)
    cur = means.reshape(G, C, D)
    for g in range(G):
        expect = (0.75 * mean[empty]) + ((1 - 0.75) * cur[g][empty])
        fa.same_bits("map_adapt_models: the Gaussians without occupancy of model %d against numpy (0.75 mean0 + 0.25 cur_mean[%d])" % (g, g),
                     got_means[g][empty], expect)
    assert not np.array_equal(cur[0][empty], cur[1][empty]) and not np.array_equal(got_means[0][empty], got_means[1][empty])
    want_b.close()
    got_b.close()


# ================================================================================================ matrices with ld
def test_segment_means_and_cohort_statistics_with_ld_beyond_2_30(far, ctx):
    ld, rows, cols = (1 << 30) + 2, 3, 100
    V = exact_frames(rows, cols, F64, 9)
    view = far.view(F64, (rows, cols), (ld, 1))
    assert view.stride(0) * 2 > 1 << 31
    sb = np.array([0, 7, 7, 40, 100], np.int64)
    vd = dev(V)
    got, _ = far.run("segment_means ld 2^30 + 2", lambda: ctx.segment_means(view, sb), inputs=[(view, V)])
    same("segment_means ld 2^30 + 2", got, ctx.segment_means(vd, sb))
    want = np.array([[V[r, a:e].sum() / (e - a) if e > a else 0.0 for a, e in zip(sb, sb[1:])] for r in range(rows)])
    fa.same_bits("segment_means against numpy (exact sums)", got, want)
    for axis in (0, 1):
        for kw in ({}, {"mean_mode": 1, "percent_h": 0.1, "percent_l": 0.05}):
            what = "score_cohort_stats ld 2^30 + 2 axis %d %s" % (axis, kw)
            got, _ = far.run(what, lambda: ctx.score_cohort_stats(view, axis, **kw), inputs=[(view, V)])
            same(what, got, ctx.score_cohort_stats(vd, axis, **kw))
    m, s = ctx.score_cohort_stats(vd, 0)
    n = V.shape[1]
    fa.same_bits("score_cohort_stats mean against numpy (exact sums)", m, V.sum(1) / n)


def test_score_normalize_past_2_31_elements(far, ctx):
    """gmmiv_score_normalize has no ld: its matrix is contiguous.  M = 2, S = 2^30 + 2 is the smallest whose last elements lie past 2^31
    doubles and that fits above the guard (a third row would end 24 GiB above the window).  Every element is checked on the device in
    slabs against the two IEEE operations the header names, and the ends of both rows against the entry point on a small matrix."""
    import torch
    from lia_ral_amd import capi
    M, S = 2, (1 << 30) + 2
    view = far.view(F64, (M, S), (S, 1))
    flat = view.reshape(-1)
    SL = 1 << 27
    rm, rs = np.array([0.75, -1.25]), np.array([3.0, 7.0])
    rmd, rsd = dev(rm), dev(rs)         # device operands: torch divides by a tensor with a true division (a host scalar becomes a reciprocal)

    def value(lo, hi):
        i = torch.arange(lo, hi, device="cuda", dtype=torch.int64)
        return ((i * 2654435761) % 1021).to(torch.float64) * 0.25 - 100.0

    def check(flat):
        bad = torch.zeros((), dtype=torch.int64, device="cuda")
        for lo in range(0, M * S, SL):
            hi = min(lo + SL, M * S)
            for m in range(M):
                a, e = max(lo, m * S), min(hi, (m + 1) * S)
                if e > a:
                    bad += ((value(a, e) - rmd[m]) / rsd[m] != flat[a:e]).sum()
        return int(bad.item()), [host(view[:, :64]), host(view[:, S - 64:])]

    _, (bad, ends) = far.run_flat("score_normalize M = 2, S = 2^30 + 2", flat, value, lambda: ctx.score_normalize(view, capi.NORM_Z, row_mean=rm, row_std=rs),
                                  check)
    small = torch.stack([torch.cat([value(m * S, m * S + 64), value((m + 1) * S - 64, (m + 1) * S)]) for m in range(M)])
    ctx.score_normalize(small, capi.NORM_Z, row_mean=rm, row_std=rs)
    same("score_normalize: the ends of both rows against a small matrix", np.concatenate(ends, 1), small)
    assert bad == 0, "score_normalize: %d of %d elements are not (x - row_mean) / row_std" % (bad, M * S)


DGEMM_PAIRS = ((False, False), (False, True), (True, False))      # NN, NT, TN


@pytest.mark.parametrize("pair", DGEMM_PAIRS, ids=lambda p: "NT"[p[0]] + "NT"[p[1]])
def test_dgemm_with_far_leading_dimensions_and_batch_strides(far, ctx, pair):
    import dgemm_ref as dr
    ta, tb = pair
    M, N, K = 130, 130, 18
    shA, shB = ((K, M) if ta else (M, K)), ((N, K) if tb else (K, N))
    label = "dgemm %s%s 130 x 130 x 18" % ("NT"[ta], "NT"[tb])

    def run(batch, which, ld=None, stride=None):
        A, B, C0, acc = dr._exact_operands(3, ta, tb, M, N, K, batch, (batch,) + shA, (batch,) + shB, (batch, M, N))
        ops = {"A": np.array(A), "B": np.array(B), "C": np.array(C0)}
        ref = (-0.5 * acc.astype(F64)) + 2.0 * ops["C"]           # small integers and halves: exact
        d = {k: dev(v if batch > 1 else v[0]) for k, v in ops.items()}
        want = ctx.dgemm(ta, tb, -0.5, d["A"], d["B"], 2.0, d["C"].clone())
        fa.same_bits("%s batch %d: the dense call against the exact product" % (label, batch), host(want).reshape(ref.shape), ref)
        r, c = ops[which].shape[1:]
        if batch > 1:
            view = far.view(F64, (batch, r, c), (stride, c, 1))
            data = ops[which]
        else:
            view = far.view(F64, (r, c), (ld, 1))
            data = ops[which][0]
        d[which] = view
        what = "%s batch %d %s far (ld %s, batch stride %s)" % (label, batch, which, ld, stride)
        res, got = far.run(what, lambda: ctx.dgemm(ta, tb, -0.5, d["A"], d["B"], 2.0, d["C"] if which == "C" else d["C"].clone()), inputs=[(view, data)],
                           outputs=[view] if which == "C" else [])
        same(what, got[0] if which == "C" else res, want)

    # ld = 2^24 under 130 rows (row 32 at 2^32 bytes, row 128 at 2^31 doubles); an operand of K = 18 rows -- B in NN and TN, A in TN --
    # crosses nothing at that stride, so it gets ld = 2^27: row 4 at 2^32 bytes, rows 16 and 17 at and past 2^31 doubles
    for which in "ABC":
        rows = {"A": shA, "B": shB, "C": (M, N)}[which][0]
        run(1, which, ld=1 << 24 if rows == 130 else 1 << 27)
    # batch strides of 2^31 + 8 doubles: two matrices (the third would start 32 GiB above the window, outside an allocation of 34 GiB
    # that also holds the guard below it)
    for which in "ABC":
        run(2, which, stride=(1 << 31) + 8)
