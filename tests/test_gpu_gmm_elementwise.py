"""The GMM kernels (k_llk_mfma, k_stats_z, k_stats_mfma, k_posteriors, the top-C family, the batched MM instantiation) judged per frame,
per pair (t, c) and per element of every accumulator against the long double log-domain reference and the derived bars of
tests/gmm_ref.py -- never against the largest entry of an array, so a Gaussian that carries no frame (most of them in the parity
cases of the other files) is held to its own posteriors and its own accumulator rows.

Every case of gmm_ref.CASES runs the default paths with float32 and float64 frames through Gmm.llk (+ sums), Gmm.occ,
Gmm.em_accumulate (weights 1 and 0.5, and a call accumulating into an earlier one; count and llk too), Gmm.tv_stats (one frame per
utterance, ragged utterances that cut 16-frame blocks, one utterance), llk_determine_top (COMPLETE; llk per frame, lk per selected
pair, the selection itself) and llk_use_top of a shifted client.  gmm_ref.PATH_CASES run every option path on the entry points it
affects (float32 frames), with bitwise equality where the project documents it; gmm_ref.BATCH_CASES run GmmBatch.llk / tv_stats.
The stored-likelihood path cuts a call only into chunks of at least 4096 frames, so the chunked path ("z_scratch_mb") runs the
models of PATH_CASES on frame streams just longer than one such chunk.

A failure names case, path, entry point, the first offending index, the value, the reference and the ratio to the bar.  With
GMM_ERRORS_JSON set to a path the largest ratio per (case, path, entry point) is written there (profiles/r14/gmm_errors.json).
"""
import contextlib
import json
import os

import numpy as np
import pytest

import gmm_ref as gr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300), pytest.mark.skipif(not gr.HAVE_LONGDOUBLE, reason=gr.SKIP_MESSAGE)]

LD = gr.LD
DEFAULTS = {"glds": 1, "em_chunks": 0, "wg_waves": 8, "prune_log2": 0, "stats_z": 1, "z_scratch_mb": 16384, "tv_stats_split": 1, "topc_z": 1,
            "topc_fused": 1, "assume_finite": 0, "z_waves": 8, "z_tv4": 1, "z_depth_em": 2, "z_depth_tv": 4, "short_calls": 1, "timing": 0}
ALL = ("llk", "occ", "em", "tv", "top")
# path -> (options away from the defaults, the entry points the options reach, the floor of a posterior)
PATHS = {
    "stats_z 0": ({"stats_z": 0}, ("em", "tv"), gr.PHI),
    "wg_waves 4": ({"wg_waves": 4}, ALL, gr.PHI),
    "short_calls 0": ({"short_calls": 0}, ALL, gr.PHI),
    "glds 0": ({"glds": 0}, ALL, gr.PHI),
    "z_waves 4": ({"z_waves": 4}, ("em", "tv"), gr.PHI),
    "z_waves 16": ({"z_waves": 16}, ("em", "tv"), gr.PHI),
    "z_tv4 0": ({"z_tv4": 0}, ("tv",), gr.PHI),
    "z_depth_em 4": ({"z_depth_em": 4}, ("em",), gr.PHI),
    "z_depth_tv 2": ({"z_depth_tv": 2}, ("tv",), gr.PHI),
    "tv_stats_split 0": ({"tv_stats_split": 0}, ("tv",), gr.PHI),
    "em_chunks 8": ({"em_chunks": 8}, ("em",), gr.PHI),
    "prune_log2 100": ({"prune_log2": 100}, ("em", "tv"), 2.0 ** -100),
    "topc_fused 0": ({"topc_fused": 0}, ("top",), gr.PHI),
    "topc_fused 0 topc_z 0": ({"topc_fused": 0, "topc_z": 0}, ("top",), gr.PHI),
}
RATIOS = {}


@pytest.fixture(scope="module")
def ctx():
    from lia_ral_amd import capi
    c = capi.Context(0)
    yield c
    c.close()
    path = os.environ.get("GMM_ERRORS_JSON")
    if path and RATIOS:
        per_path = {}
        for (case, p, entry), v in RATIOS.items():
            per_path[p] = max(per_path.get(p, 0.0), v)
        with open(path, "w") as f:
            json.dump({"bound": "tests/gmm_ref.py: rho = (2D + 16) u S per logit, B_t per frame, gamma (rho + B_t + 8u) + phi per posterior, "
                                "sum of these + (n + 8) u sum gamma |v| per accumulator element",
                       "max_ratio": max(RATIOS.values()), "paths": {k: float("%.4g" % v) for k, v in sorted(per_path.items())},
                       "entries": {" | ".join(k): float("%.4g" % v) for k, v in sorted(RATIOS.items())}}, f, indent=1)


@contextlib.contextmanager
def options(ctx, opts):
    """set, run, restore (as test_gpu_dgemm.options): set_option hands back what was there"""
    try:
        for k, v in opts.items():
            prev = ctx.set_option(k, v)
            assert prev == DEFAULTS[k], "option %s was %r, expected the default %r" % (k, prev, DEFAULTS[k])
        yield
    finally:
        for k, v in opts.items():
            back = ctx.set_option(k, DEFAULTS[k])
            assert back == v, "option %s read back %r after it was set to %r" % (k, back, v)


class Judge:
    """collects the failures of one test; every comparison goes through gmm_ref.ratio against a bar of gmm_ref"""

    def __init__(self, case, path):
        self.case, self.path, self.bad = case, path, []

    def __call__(self, entry, axes, got, ref, bar):
        got = np.asarray(got, np.float64)
        ref = np.broadcast_to(ref, got.shape)
        r = gr.ratio(got.astype(LD) - ref, bar)
        worst = float(r.max()) if r.size else 0.0
        key = (self.case, self.path, entry)
        RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
        if worst > 1.0:
            i = tuple(int(v) for v in np.argwhere(r > 1.0)[0])
            self.bad.append("%s | %s | %s: %d of %d outside the bar, first at %s = %s: got %r, reference %r, |error| / bar = %.3g (largest %.3g)"
                            % (self.case, self.path, entry, int((r > 1.0).sum()), r.size, axes, i, float(got[i]), float(ref[i]), float(r[i]), worst))

    def same_bits(self, entry, a, b, what):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape or not np.array_equal(a.view(np.int64), b.view(np.int64)):
            i = tuple(int(v) for v in np.argwhere(a.view(np.int64) != b.view(np.int64))[0]) if a.shape == b.shape else ()
            self.bad.append("%s | %s | %s: not the bits of %s, first at %s: %r against %r"
                            % (self.case, self.path, entry, what, i, float(a[i]) if i else a.shape, float(b[i]) if i else b.shape))

    def note(self, entry, text):
        self.bad.append("%s | %s | %s: %s" % (self.case, self.path, entry, text))

    def finish(self):
        assert not self.bad, "%d comparisons failed:\n" % len(self.bad) + "\n".join(self.bad[:30])


def label(case, dtype, extra=""):
    return "%s %s%s" % (gr.case_name(case), gr.dtype_name(dtype), extra)


def layouts(T):
    """utterance bounds: (a) one frame per utterance -- every posterior of the N / F mode under its own bar; (b) ragged utterances
    that cut 16-frame blocks, an empty one among them; (c) one utterance"""
    return (("a", np.arange(T + 1, dtype=np.int64)), ("b", gr.ragged_bounds(T)), ("c", np.array([0, T], np.int64)))


# ---------------------------------------------------------------- the entry points
def run_llk(j, g, x, ref):
    sums = np.zeros(2)
    got = g.llk(x, -1e9, 1e9, sums=sums)
    j("llk", "(t)", got, ref.llk, ref.B)
    s, sb = ref.llk_sum()
    j("llk sums", "()", sums[0], s, sb)
    if sums[1] != ref.T:
        j.note("llk sums", "frame count %r, expected %d" % (sums[1], ref.T))
    return got


def run_occ(j, g, x, ref):
    j("occ", "(t, c)", g.occ(x), ref.gamma, ref.dgamma)


def check_acc(j, entry, g, acc, ref, weights):
    """an EM accumulator holding the calls of `weights` on the same frames"""
    a = g.split_acc(acc)
    parts = [ref.sums(s=s) for s in weights]
    for k, axes in (("occ", "(c)"), ("sx", "(c, d)"), ("sxx", "(c, d)")):
        j("%s %s" % (entry, k), axes, a[k], sum(p[k] for p in parts), sum(p[k + "_b"] for p in parts))
    ls = [ref.llk_sum(s=s) for s in weights]
    j(entry + " llk", "()", a["llk"], sum(l[0] for l in ls), sum(l[1] for l in ls))
    j(entry + " count", "()", a["count"], *ref.count_bar(weights))


def run_em(j, g, x, ref):
    one = g.em_accumulate(x)
    check_acc(j, "em w=1", g, one, ref, (1.0,))
    check_acc(j, "em w=0.5", g, g.em_accumulate(x, weight=0.5), ref, (0.5,))
    check_acc(j, "em w=1 then 0.5", g, g.em_accumulate(x, weight=0.5, acc=one.copy()), ref, (1.0, 0.5))
    return one


def run_tv(j, g, x, ref, which="abc"):
    out = {}
    for name, ub in layouts(ref.T):
        if name not in which:
            continue
        N, F = g.tv_stats(x, ub)
        Nr, Fr, Nb, Fb = ref.utt_stats(ub)
        j("tv(%s) N" % name, "(u, c)", N, Nr, Nb)
        j("tv(%s) F" % name, "(u, c, d)", F.reshape(Fr.shape), Fr, Fb)
        out[name] = (N, F)
    return out


def run_top(j, g, client, x, ref, cref):
    """DETERMINE_TOP_DISTRIBS (ctop = min(10, C), COMPLETE) on the world model, USE_TOP_DISTRIBS of a shifted client on its selection"""
    ctop = min(10, ref.C)
    d = g.llk_determine_top(x, ctop, True, -1e9, 1e9)
    idx = d["idx"].astype(np.int64)
    if idx.min() < 0 or idx.max() >= ref.C or any(len(set(r)) != ctop for r in idx.tolist()):
        j.note("top idx", "indices outside the model or repeated in a row")
        return
    short, slack = ref.selection_shortfall(idx)
    j("top idx", "(t, j)", short, 0.0, slack)
    j("top llk", "(t)", d["llk"], ref.llk, ref.B)
    j("top lk", "(t, j)", d["lk"], *ref.selected_lk(idx))
    ln, mask = ref.nontop(idx)
    want_llk, bar = gr.use_top(cref, idx, ln, ref, mask)
    j("use_top llk", "(t)", client.llk_use_top(x, d["idx"], d["nontop_llk"], True, -1e9, 1e9), want_llk, bar)


RUN = {"llk": run_llk, "occ": run_occ, "em": run_em, "tv": run_tv}
CLIENT_SHIFT = 5


def run_entries(ctx, j, case, dtype, entries, floor=gr.PHI, x=None):
    ref = gr.reference(case, gr.dtype_name(dtype), 0, floor)
    g = ctx.gmm(*gr.model(case))
    x = gr.frames(case, dtype) if x is None else x
    out = {}
    for e in entries:
        if e == "top":
            client = ctx.gmm(*gr.model(case, CLIENT_SHIFT))
            run_top(j, g, client, x, ref, gr.reference(case, gr.dtype_name(dtype), CLIENT_SHIFT, floor))
            client.close()
        else:
            out[e] = RUN[e](j, g, x, ref)
    g.close()
    return out


# ---------------------------------------------------------------- the tests
@pytest.mark.parametrize("dtype", gr.DTYPES, ids=gr.dtype_name)
@pytest.mark.parametrize("case", gr.CASES, ids=gr.case_name)
def test_default_paths_per_frame_pair_and_element(ctx, case, dtype):
    j = Judge(label(case, dtype), "defaults")
    run_entries(ctx, j, case, dtype, ALL)
    j.finish()


@pytest.mark.parametrize("dtype", gr.DTYPES, ids=gr.dtype_name)
def test_frames_as_rows_of_a_wider_device_matrix(ctx, dtype):
    import torch
    case = gr.WIDE_CASE
    C, D, T, _ = case
    x = gr.frames(case, dtype)
    wide = torch.full((T, D + 5), 1e30, dtype=torch.from_numpy(x).dtype, device="cuda")    # the filler must never be read as a feature
    wide[:, :D] = torch.from_numpy(x).cuda()
    xv = wide[:, :D]
    torch.cuda.synchronize()
    assert xv.stride(0) == D + 5
    j = Judge(label(case, dtype, " ldx=D+5"), "defaults")
    run_entries(ctx, j, case, dtype, ALL, x=xv)
    with options(ctx, {"stats_z": 0}):
        j.path = "stats_z 0"
        run_entries(ctx, j, case, dtype, ("em", "tv"), x=xv)
    j.finish()


@pytest.mark.parametrize("case", gr.PATH_CASES, ids=gr.case_name)
@pytest.mark.parametrize("path", list(PATHS), ids=lambda p: p.replace(" ", "_"))
def test_option_paths_per_frame_pair_and_element(ctx, path, case):
    opts, entries, floor = PATHS[path]
    j = Judge(label(case, np.float32), path)
    with options(ctx, opts):
        run_entries(ctx, j, case, np.float32, entries, floor)
    j.finish()


@pytest.mark.parametrize("case", gr.PATH_CASES, ids=gr.case_name)
def test_paths_documented_as_bitwise_equal_are(ctx, case):
    """glds, short_calls and assume_finite for the log-likelihoods; the workgroup shapes of k_stats_z ("bit-identical by construction")"""
    j = Judge(label(case, np.float32), "bitwise")
    x = gr.frames(case, np.float32)
    g = ctx.gmm(*gr.model(case))
    base = g.llk(x, -1e9, 1e9)
    for k, v in (("glds", 0), ("short_calls", 0), ("assume_finite", 1)):
        with options(ctx, {k: v}):
            j.same_bits("llk %s %d" % (k, v), g.llk(x, -1e9, 1e9), base, "the default path")
    ub = gr.ragged_bounds(case[2])
    em, (N, F) = g.em_accumulate(x, weight=0.5), g.tv_stats(x, ub)
    for waves in (4, 16):
        with options(ctx, {"z_waves": waves}):
            j.same_bits("em z_waves %d" % waves, g.em_accumulate(x, weight=0.5), em, "z_waves 8")
            N2, F2 = g.tv_stats(x, ub)
            j.same_bits("tv N z_waves %d" % waves, N2, N, "z_waves 8")
            j.same_bits("tv F z_waves %d" % waves, F2, F, "z_waves 8")
    g.close()
    j.finish()


def chunk_plan(C):
    """-> (z_scratch_mb, T): the smallest scratch whose chunk (z_chunk_frames, capi_gmm_util.h: at least 4096 frames, a multiple of 64)
    the library accepts, and a frame count one ragged piece beyond it"""
    nct = ((C + 15) // 16 + 1) // 2 * 2
    per_frame = nct * 16 * 8 + nct * 2 + 16
    mb = 1
    frames = lambda m: int(((m << 20) // per_frame) / 1.2) // 64 * 64
    while frames(mb) < 4096:
        mb += 1
    return mb, frames(mb) + 203


@pytest.mark.parametrize("case", gr.PATH_CASES, ids=gr.case_name)
def test_stored_likelihood_path_in_chunks(ctx, case):
    """a scratch that holds one chunk of ~4100 frames: two launches of k_stats_z per call, EM sums carried from chunk to chunk,
    utterances dealt to chunks"""
    C, D, _, spread = case
    mb, T = chunk_plan(C)
    long_case = (C, D, T, spread)
    j = Judge(label(long_case, np.float32), "z_scratch_mb %d" % mb)
    ref = gr.reference(long_case, "float32")
    x = gr.frames(long_case, np.float32)
    g = ctx.gmm(*gr.model(long_case))
    with options(ctx, {"z_scratch_mb": mb, "timing": 1}):
        acc = g.em_accumulate(x, weight=0.5)
        n_em = ctx.kernel_launches("k_stats_z")
        N, F = g.tv_stats(x, gr.ragged_bounds(T))
        n_tv = ctx.kernel_launches("k_stats_z")
    assert n_em >= 2 and n_tv >= 2, (n_em, n_tv)
    check_acc(j, "em w=0.5", g, acc, ref, (0.5,))
    Nr, Fr, Nb, Fb = ref.utt_stats(gr.ragged_bounds(T))
    j("tv(b) N", "(u, c)", N, Nr, Nb)
    j("tv(b) F", "(u, c, d)", F.reshape(Fr.shape), Fr, Fb)
    g.close()
    j.finish()


BATCH_SHIFTS = (0, 11, 12)


@pytest.mark.parametrize("dtype", gr.DTYPES, ids=gr.dtype_name)
@pytest.mark.parametrize("case", gr.BATCH_CASES, ids=gr.case_name)
def test_a_model_per_segment(ctx, case, dtype):
    """GmmBatch.llk / tv_stats: three models, four segments whose bounds cut 16-frame blocks (one empty), frames before the first
    and after the last segment that belong to none"""
    C, D, T, _ = case
    models = [gr.model(case, s) for s in BATCH_SHIFTS]
    refs = [gr.reference(case, gr.dtype_name(dtype), s) for s in BATCH_SHIFTS]
    b = ctx.gmm_batch(3, C, D).load(np.stack([m[0] for m in models]), np.stack([m[1] for m in models]), np.stack([m[2] for m in models]))
    x = gr.frames(case, dtype)
    sb = np.array([3, T // 4 + 5, T // 4 + 5, 2 * T // 3 + 1, T - 1], np.int64)
    sm = np.array([1, 2, 0, 2], np.int32)
    j = Judge(label(case, dtype), "batch")
    llk, ssum = b.llk(x, sb, sm, -1e9, 1e9)
    N, F, sl = b.tv_stats(x, sb, sm)
    if not (np.isnan(llk[:sb[0]]).all() and np.isnan(llk[sb[-1]:]).all()):
        j.note("batch llk", "a frame outside every segment was written")
    for s, m in enumerate(sm):
        lo, hi, r = int(sb[s]), int(sb[s + 1]), refs[m]
        want, bar = r.llk_sum(lo, hi)
        j("batch llk seg %d" % s, "(t - %d)" % lo, llk[lo:hi], r.llk[lo:hi], r.B[lo:hi])
        j("batch llk seg_sum %d" % s, "()", ssum[s], want, bar)
        j("batch tv seg_llk %d" % s, "()", sl[s, 0], want, bar)
        if sl[s, 1] != hi - lo:
            j.note("batch tv seg_llk %d" % s, "frame count %r, expected %d" % (sl[s, 1], hi - lo))
        if hi > lo:
            q = r.sums(lo, hi, keys=("occ", "sx"))
            j("batch tv N seg %d" % s, "(c)", N[s], q["occ"], q["occ_b"])
            j("batch tv F seg %d" % s, "(c, d)", F[s].reshape(C, D), q["sx"], q["sx_b"])
        else:
            j("batch tv N seg %d" % s, "(c)", N[s], 0.0, 0.0)
            j("batch tv F seg %d" % s, "(c * D + d)", F[s], 0.0, 0.0)
    b.close()
    j.finish()


def test_closing_a_context_closes_the_model_handles_that_outlive_it():
    """A failing test keeps its Gmm alive in the traceback until after the module's context is closed; gmmiv_gmm_destroy reads the
    handle's context, so such a handle used to be destroyed against freed memory when it was finally collected.  Context.close()
    closes its models first; closing them again afterwards does nothing."""
    import ctypes as ct
    from lia_ral_amd import capi
    c = capi.Context(0)
    case = gr.CASES[3]
    g = c.gmm(*gr.model(case))
    b = c.gmm_batch(2, case[0], case[1])
    assert np.isfinite(g.llk(gr.frames(case, np.float32), -1e9, 1e9)).all()
    c.close()
    closed = not g._h and not b._h
    if not closed:                       # never hand a handle of a destroyed context to the library: drop it instead
        g._h, b._h = ct.c_void_p(), ct.c_void_p()
    assert closed
    g.close(); b.close(); c.close()
