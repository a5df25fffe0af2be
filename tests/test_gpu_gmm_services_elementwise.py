"""The small GMM-side entry points that were judged per array or through the workspace history alone, now per element or exactly,
each on the device inputs the library itself produced, so that every bar is rounding alone:

gmmiv_tv_stats_lines           every line row has the BITS of 0.0 + r_1 + r_2 .. in list order over the rows gmmiv_tv_stats returns
                               for the same files (k_merge_rows is a left fold) and lies inside the sum of the files' bars
                               (gmm_ref.Reference.utt_stats) + (k + 1) u sum |r_i|; a file twice on a line, a file on several lines,
                               a line without files (zeros), a line of the empty file; device outputs between guard bands; 65 537
                               lines in one call (the launcher splits gridDim.y at 65 535).
gmmiv_segment_means            against long double, bar (n + 8) u sum |v| / n per (row, segment): an empty segment (exactly 0), one
                               frame, 8192 and 8193 frames (the piece size), 20 000 frames; ld > n; a row alone has its bits.
gmmiv_em_get                   w, mean, cov per element on a device accumulator: 2u |w|, 2u |mean|, 6u (|sxx / occ| + mean^2); a
                               Gaussian of occupancy 0 keeps prev_mean / prev_cov bit for bit and gets weight 0.
gmmiv_variance_control         exact: the numpy clamp, floor test first, both counts; values on both bounds, a dimension whose floor
                               lies above its ceiling, counts = NULL, in place on a device tensor between guard bands.
gmmiv_count_unusable_frames    exact counts on both branches of k_flag_frames (dense 16-byte float rows / generic), values on both
                               sides of the 1e18 bound, padding columns, a misaligned view; "screened_frames" agrees, and a frame
                               the count calls usable comes back from gmmiv_llk with the reference's log-likelihood.

With SERVICES_ERRORS_JSON set to a path the largest ratio per (case, path, entry, kind) is written there
(profiles/r24/gmm_services_errors.json)."""
import json
import os
import time

import numpy as np
import pytest

import gmm_ref as gr
from conftest import make_gmm
from elementwise_judge import Guarded, Judge

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300), pytest.mark.skipif(not gr.HAVE_LONGDOUBLE, reason=gr.SKIP_MESSAGE)]

LD = gr.LD
U = gr.U
RATIOS = {}
JUDGED = [0]


class CountingJudge(Judge):
    def __call__(self, entry, kind, ratios):
        JUDGED[0] += int(np.asarray(ratios).size)
        super().__call__(entry, kind, ratios)


@pytest.fixture(scope="module")
def ctx():
    from lia_ral_amd import capi
    t0 = time.time()
    c = capi.Context(0)
    yield c
    c.close()
    path = os.environ.get("SERVICES_ERRORS_JSON")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump({"max_ratio": float("%.4g" % max(RATIOS.values())), "judged_elements": JUDGED[0], "module_seconds": round(time.time() - t0, 1),
                       "entries": {" | ".join(k): float("%.4g" % v) for k, v in sorted(RATIOS.items())}}, f, indent=1)


# ---------------------------------------------------------------- gmmiv_tv_stats_lines
LINE_CASES = ((37, 17, 300, 2.0), (129, 60, 256, 2.0))
EMPTY_FILE = 1                                                # gmm_ref.ragged_bounds: file 1 is empty
LINES = ([0], [0, 2, 3], [2, 2], [3], [], [EMPTY_FILE], [3, 4], [4, 3, 0, 2], [EMPTY_FILE, 4])     # file 3 stands on four lines


def fold(rows, files):
    """0.0 + r_1 + r_2 .. in list order, the additions of k_merge_rows"""
    s = np.zeros(rows.shape[1])
    for f in files:
        s = s + rows[f]
    return s


def judge_lines(j, N, F, Nf, Ff, stats, lines):
    Nr, Fr, Nb, Fb = stats
    Fr, Fb = Fr.reshape(Ff.shape), Fb.reshape(Ff.shape)
    for l, files in enumerate(lines):
        k = len(files)
        for name, got, rows, want, bar in (("N", N[l], Nf, Nr, Nb), ("F", F[l], Ff, Fr, Fb)):
            j.same_bits("%s line %d" % (name, l), got, fold(rows, files), "the fold over the file rows")
            w = sum((want[f] for f in files), np.zeros(rows.shape[1], LD))
            b = sum((bar[f] for f in files), np.zeros(rows.shape[1])) + (k + 1) * U * sum((np.abs(rows[f]) for f in files), np.zeros(rows.shape[1]))
            j("%s line %d" % (name, l), "(c[, d])", gr.ratio(got.astype(LD) - w, b))
        if not files and (np.any(N[l] != 0.0) or np.any(F[l] != 0.0)):
            j.note("line %d" % l, "a line without files is not a row of zeros")


@pytest.mark.parametrize("dtype", gr.DTYPES, ids=gr.dtype_name)
@pytest.mark.parametrize("case", LINE_CASES, ids=gr.case_name)
def test_tv_stats_lines_rows_are_the_fold_of_their_file_rows(ctx, case, dtype):
    C, D, T, _ = case
    ref = gr.reference(case, gr.dtype_name(dtype))
    x = gr.frames(case, dtype)
    fb = gr.ragged_bounds(T)
    assert fb[EMPTY_FILE + 1] == fb[EMPTY_FILE] and len(fb) == 6
    g = ctx.gmm(*gr.model(case))
    j = CountingJudge("%s %s" % (gr.case_name(case), gr.dtype_name(dtype)), "host outputs", RATIOS)
    Nf, Ff = g.tv_stats(x, fb)
    stats = ref.utt_stats(fb)
    N, F = g.tv_stats_lines(x, fb, LINES)
    judge_lines(j, N, F, Nf, Ff, stats, LINES)
    j.path = "device outputs"
    L = len(LINES)
    Nd, Fd = Guarded((L, C), fill=None), Guarded((L, C * D), fill=None)
    g.tv_stats_lines(x, fb, LINES, Nd.view, Fd.view)
    ctx.sync()
    j.same_bits("N", Nd.read(j, "N"), N, "the host-output call")
    j.same_bits("F", Fd.read(j, "F"), F, "the host-output call")
    g.close()
    j.finish()


def test_tv_stats_lines_beyond_one_grid_of_lines(ctx):
    """65 537 lines of two files each over 70 files of two frames (C = 1, D = 1): tvk_merge_rows launches 65 535 + 2 rows"""
    case = (1, 1, 140, 2.0)
    nfiles, nlines = 70, 65537
    x = gr.frames(case, np.float64)
    fb = np.arange(0, 2 * nfiles + 1, 2, dtype=np.int64)
    g = ctx.gmm(*gr.model(case))
    a, b = np.arange(nlines) % nfiles, (7 * np.arange(nlines) + 3) % nfiles
    lines = np.stack([a, b], 1).tolist()
    Nf, Ff = g.tv_stats(x, fb)
    N, F = g.tv_stats_lines(x, fb, lines)
    j = CountingJudge(gr.case_name(case) + " float64", "65537 lines", RATIOS)
    j.same_bits("N", N[:, 0], (0.0 + Nf[a, 0]) + Nf[b, 0], "the fold over the file rows")
    j.same_bits("F", F[:, 0], (0.0 + Ff[a, 0]) + Ff[b, 0], "the fold over the file rows")
    Nr, Fr, Nb, Fb = gr.reference(case, "float64").utt_stats(fb)
    for l in (65534, 65535, 65536):
        wn, wf = Nr[a[l], 0] + Nr[b[l], 0], Fr[a[l], 0, 0] + Fr[b[l], 0, 0]
        bn = Nb[a[l], 0] + Nb[b[l], 0] + 3 * U * (abs(Nf[a[l], 0]) + abs(Nf[b[l], 0]))
        bf = Fb[a[l], 0, 0] + Fb[b[l], 0, 0] + 3 * U * (abs(Ff[a[l], 0]) + abs(Ff[b[l], 0]))
        j("N line %d" % l, "()", gr.ratio(np.array([N[l, 0]]).astype(LD) - wn, bn))
        j("F line %d" % l, "()", gr.ratio(np.array([F[l, 0]]).astype(LD) - wf, bf))
    assert nlines > 65535
    g.close()
    j.finish()


# ---------------------------------------------------------------- gmmiv_segment_means
SEG_BOUNDS = np.array([0, 0, 1, 8193, 16386, 36386], np.int64)      # empty, 1 frame, 8192 (one piece), 8193 (a piece + 1), 20 000


def test_segment_means_per_row_and_segment(ctx):
    import torch
    n, nrows = int(SEG_BOUNDS[-1]), 5
    ld = n + 7
    rng = np.random.default_rng(31)
    v = rng.normal(0.0, 1.0, (nrows, ld)) * np.array([1.0, 1e-3, 50.0, 1.0, 1e6])[:, None]
    v[3] = -70.0 + rng.normal(0.0, 3.0, ld)                     # log-likelihood-like values
    v[:, n:] = 1e300                                            # behind the last segment: never read
    vd = torch.from_numpy(v).cuda()
    got = ctx.segment_means(vd[:, :n], SEG_BOUNDS)
    assert vd[:, :n].stride(0) == ld
    j = CountingJudge("segment_means 5 x %d, ld %d" % (n, ld), "defaults", RATIOS)
    vl = v.astype(LD)
    want, bar = np.zeros(got.shape, LD), np.zeros(got.shape)
    for s in range(len(SEG_BOUNDS) - 1):
        lo, hi = int(SEG_BOUNDS[s]), int(SEG_BOUNDS[s + 1])
        if hi > lo:
            want[:, s] = vl[:, lo:hi].sum(1) / LD(hi - lo)
            bar[:, s] = (hi - lo + 8) * U * np.abs(v[:, lo:hi]).sum(1) / (hi - lo)
    j("mean", "(row, segment)", gr.ratio(got.astype(LD) - want, bar))
    if np.any(got[:, 0] != 0.0):
        j.note("mean", "the empty segment is not exactly 0")
    for r in range(nrows):
        j.same_bits("row %d alone" % r, ctx.segment_means(vd[r:r + 1, :n], SEG_BOUNDS)[0], got[r], "the row inside the call")
    j.finish()


# ---------------------------------------------------------------- gmmiv_em_get
EM_GET_CASES = ((37, 17, 300, 2.0), (40, 61, 66, 2.0))


@pytest.mark.parametrize("case", EM_GET_CASES, ids=gr.case_name)
def test_em_get_per_element_on_the_device_accumulator(ctx, case):
    import torch
    C, D, T, _ = case
    g = ctx.gmm(*gr.model(case))
    acc = torch.zeros(g.em_acc_len(), dtype=torch.float64, device="cuda")
    g.em_accumulate(gr.frames(case, np.float32), acc=acc)
    ctx.sync()
    empty = (3, C - 1)
    for c in empty:
        acc[c] = 0.0                                            # the statistics rows stay: they must not be read
    torch.cuda.synchronize()
    a = g.split_acc(acc.cpu().numpy())
    rng = np.random.default_rng(C)
    prev_mean, prev_cov = rng.normal(0, 1, (C, D)), np.exp(rng.normal(0, 0.5, (C, D)))
    w, mean, cov = g.em_get(acc, prev_mean, prev_cov)
    j = CountingJudge(gr.case_name(case) + " float32", "defaults", RATIOS)
    live = np.setdiff1d(np.arange(C), empty)
    assert np.all(a["occ"][live] > 0)
    occ = a["occ"].astype(LD)[live, None]
    wl = a["occ"].astype(LD) / LD(a["count"])
    ml = a["sx"].astype(LD)[live] / occ
    ql = a["sxx"].astype(LD)[live] / occ
    j("w", "(c)", gr.ratio(w.astype(LD) - wl, 2 * U * np.abs(wl.astype(np.float64))))
    j("mean", "(c, d)", gr.ratio(mean[live].astype(LD) - ml, 2 * U * np.abs(ml.astype(np.float64))))
    j("cov", "(c, d)", gr.ratio(cov[live].astype(LD) - (ql - ml * ml), 6 * U * (np.abs(ql) + ml * ml).astype(np.float64)))
    for c in empty:
        j.same_bits("mean of the empty Gaussian %d" % c, mean[c], prev_mean[c], "prev_mean")
        j.same_bits("cov of the empty Gaussian %d" % c, cov[c], prev_cov[c], "prev_cov")
        if w[c] != 0.0:
            j.note("w", "the empty Gaussian %d has weight %r" % (c, w[c]))
    g.close()
    j.finish()


# ---------------------------------------------------------------- gmmiv_variance_control
def clamp_np(cov, flooring, ceiling, cs):
    """varianceControl in numpy: the floor test first, then the ceiling test on what the floor left -> (cov, [floored, ceiled])"""
    out = cov.copy()
    lo, hi = flooring * cs[None, :], ceiling * cs[None, :]
    f = out <= lo
    out = np.where(f, lo, out)
    c = out >= hi
    out = np.where(c, hi, out)
    return out, np.array([f.sum(), c.sum()], np.int64)


def test_variance_control_is_the_exact_clamp(ctx):
    C, D, flooring, ceiling = 9, 6, 0.5, 2.0
    rng = np.random.default_rng(7)
    cs = np.exp(rng.normal(0, 0.3, D))
    cs[4] = -1.0                                                # flooring cs > ceiling cs: everything lands on the ceiling
    cov = np.exp(rng.normal(0, 1.0, (C, D)))
    cov[0, 0], cov[1, 0] = flooring * cs[0], ceiling * cs[0]    # exactly on both bounds: both count
    cov[2, 1], cov[3, 1] = np.nextafter(flooring * cs[1], 9.0), np.nextafter(ceiling * cs[1], 0.0)     # one step inside: neither
    cov[5, 4] = -3.0                                            # below the floor of the reversed dimension: floored AND ceiled
    want, counts = clamp_np(cov, flooring, ceiling, cs)
    assert counts[0] >= 3 and counts[1] >= 3 and want[2, 1] == cov[2, 1] and want[3, 1] == cov[3, 1] and np.all(want[:, 4] == -2.0)
    j = CountingJudge("variance_control 9 x 6", "host", RATIOS)
    got, n = ctx.variance_control(cov.copy(), flooring, ceiling, cs, C, D)
    j.same_bits("cov", got, want, "the numpy clamp")
    if n.tolist() != counts.tolist():
        j.note("counts", "%r, expected %r" % (n.tolist(), counts.tolist()))
    got, n = ctx.variance_control(cov.copy(), flooring, ceiling, cs, C, D, count=False)
    j.same_bits("cov, counts NULL", got, want, "the numpy clamp")
    assert n is None
    j.path = "device, in place"
    gd = Guarded((C, D), init=cov)
    _, n = ctx.variance_control(gd.view, flooring, ceiling, cs, C, D)
    ctx.sync()
    j.same_bits("cov", gd.read(j, "cov"), want, "the numpy clamp")
    if n.tolist() != counts.tolist():
        j.note("counts", "%r, expected %r" % (n.tolist(), counts.tolist()))
    j.finish()


# ---------------------------------------------------------------- gmmiv_count_unusable_frames
def boundary(dtype):
    """-> (the largest usable value, the smallest unusable one) of the dtype: |x| <= 1e18 is usable"""
    big = dtype(1e18)
    return big, np.nextafter(big, dtype(np.inf))


def planted(T, D, dtype, seed):
    """frames with every kind of value on both sides of the bound -> (x, the exact count by the rule |x| <= 1e18)"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (T, D)).astype(dtype)
    big, nxt = boundary(dtype)
    values = [np.nan, np.inf, -np.inf, big, -big, nxt, -nxt]
    for k, v in enumerate(values):
        if T:
            x[(37 * k + 5) % T, (11 * k) % D] = v                # T = 1: all of them in the one frame
    if T > 200:
        x[100, 0], x[100, D - 1] = np.nan, np.inf                 # two bad values in one frame: counted once
        x[T - 1, D - 1] = -np.inf                                 # the last element of the matrix
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(x.astype(np.float64)) <= 1e18)
    return x, int(bad.any(1).sum())


@pytest.mark.parametrize("dtype", gr.DTYPES, ids=gr.dtype_name)
@pytest.mark.parametrize("D", (1, 3, 4, 60, 61))
def test_count_unusable_frames_is_exact_on_both_branches(ctx, D, dtype):
    import torch
    big, nxt = boundary(dtype)
    assert abs(float(big)) <= 1e18 < abs(float(nxt))
    bad = []
    for T in (0, 1, 255, 1025):
        x, want = planted(T, D, dtype, 100 * D + T)
        got = ctx.count_unusable_frames(x)
        if got != want:
            bad.append("D %d T %d: %d, expected %d" % (D, T, got, want))
    for v, want in ((big, 0), (-big, 0), (nxt, 1), (-nxt, 1), (np.nan, 1), (np.inf, 1)):     # one frame, one value
        x = np.zeros((1, D), dtype)
        x[0, D - 1] = v
        got = ctx.count_unusable_frames(x)
        if got != want:
            bad.append("D %d one frame with %r: %d, expected %d" % (D, v, got, want))
    # a wider device matrix: bad values in the padding columns are not features
    T = 255
    x, want = planted(T, D, dtype, 7)
    wide = torch.full((T, D + 4), float("nan"), dtype=torch.from_numpy(x).dtype, device="cuda")
    wide[:, :D] = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    got = ctx.count_unusable_frames(wide[:, :D])
    if got != want:
        bad.append("D %d ldx D + 4: %d, expected %d" % (D, got, want))
    # a dense view that starts one element (4 bytes for float32) off its 16-byte alignment
    flat = torch.zeros(T * D + 1, dtype=torch.from_numpy(x).dtype, device="cuda")
    flat[1:] = torch.from_numpy(x).cuda().reshape(-1)
    view = flat[1:].view(T, D)
    torch.cuda.synchronize()
    assert view.data_ptr() % 16 != 0
    got = ctx.count_unusable_frames(view)
    if got != want:
        bad.append("D %d misaligned: %d, expected %d" % (D, got, want))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", gr.DTYPES, ids=gr.dtype_name)
def test_a_frame_the_count_calls_usable_is_evaluated(ctx, dtype):
    """a model whose variance in one dimension is 1e34 gives a frame with the largest usable value there an ordinary likelihood:
    gmmiv_llk must return the reference's value for it, and count in "screened_frames" exactly the frames the count names"""
    C, D, T, WIDE = 3, 4, 255, 2
    w, mean, iv = make_gmm(C, D, seed=5)
    iv[:, WIDE] = 1e-34
    big, nxt = boundary(dtype)
    x = np.random.default_rng(9).normal(0, 1, (T, D)).astype(dtype)
    usable_at, unusable_at = (3, 64, 200), (4, 65, 254)
    for t, v in zip(usable_at, (big, -big, big)):
        x[t, WIDE] = v
    for t, v in zip(unusable_at, (nxt, np.nan, -nxt)):
        x[t, WIDE] = v
    n = ctx.count_unusable_frames(x)
    assert n == len(unusable_at)
    g = ctx.gmm(w, mean, iv)
    ctx.set_option("screened_frames", 0)
    got = g.llk(x, -1e9, 1e9)
    assert ctx.set_option("screened_frames", 0) == n
    keep = np.setdiff1d(np.arange(T), unusable_at)
    ref = gr.Reference(w, mean, iv, x[keep])
    j = CountingJudge("3x4x255 variance 1e34 %s" % gr.dtype_name(dtype), "defaults", RATIOS)
    j("llk of the usable frames", "frames", gr.ratio(got[keep].astype(LD) - ref.llk, ref.B))
    if not np.all(got[list(usable_at)] > -1e6):
        j.note("llk", "a frame with the largest usable value came back as %r" % got[list(usable_at)].tolist())
    g.close()
    j.finish()
