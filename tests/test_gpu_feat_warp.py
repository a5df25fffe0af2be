"""gmmiv_feat_warp_hist / gmmiv_feat_warp_apply (include/ext/gmmiv_feat_warp.h) on the device against tests/warp_ref.py.

What is demanded: bounds equal to the restatement's order statistics; count and every warped value with the BITS of the fp64
restatement of the reference's loops, and each under a derived bar against the long double one; status exact; degenerate columns
copied through; and the suite-wide rules applied here to the two entry points (their header is not under include/ yet): a used
context's bits, frames beyond 2^31 elements from the pointer; device inputs that arrive late on the stream are
tests/test_gpu_zz_feat_warp_stream.py.

The bars (u = 2^-53).  count = (m / n) / (b1 - b0): three roundings, 4 u relative.  A warped value, where the fp64 and the long double
restatements take the same bins (idxW, idxD): the source area sum tw carries (idxW + 10) u tw (a density of 3 u, a width, a product, idxW
additions, the interpolated last bin), the target prefix (idxD + 6) u T; both are divided by the target bin's area I and scaled by its
width w, the interval I = (area + td) - td cancels and adds the prefix errors once more:
    bar = 2 [ w ((e_tw + 2 e_td) / I + |ph| (2 e_td + 3 u I) / I + 3 u |ph|) + 2 u (|lower| + |value|) ]
Where the two restatements take different target bins (tw within rounding of a prefix value) the as-written back-off jumps by
w |area[j + 1] - area[j]| / area[j] at the edge; that, doubled and maximised over the table, is added for those values only."""
import os

import numpy as np
import pytest

import warp_ref as W
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from lia_ral_amd import capi                    # noqa: E402
from lia_ral_amd import feat_warp as fw         # noqa: E402  (fails here without the feature)

U53 = 2.0 ** -53
_S = {}


def ctx():
    import torch
    if "ctx" not in _S:
        _S["ctx"] = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    return _S["ctx"]


def new_ctx():
    """a context of its own (workspace, options, timers) on torch's current stream: no test of this file creates a stream (DESIGN.md
    section 9, item 7; the late-input test, which needs a private stream, is tests/test_gpu_zz_feat_warp_stream.py)"""
    import torch
    return capi.Context(0, torch.cuda.current_stream().cuda_stream)


def target():
    if "t" not in _S:
        _S["t"] = W.read_histo(os.path.join(GOLDEN, "table_gaussN.histo"))
    return _S["t"]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize])


def make(D, lens, dtype, seed, pad=3, gap=2):
    """units of the given lengths, each cut into two runs (three frames apart) when it has two frames; ldx = D + pad; a frame row
    is N(c, (1 + c / 7)^2) per column c -> (buffer [T, D + pad], runs [., 3])"""
    rng = np.random.default_rng(seed)
    runs, cur = [], 1
    for u, n in enumerate(lens):
        a = n // 3 if n >= 2 else n
        for part in (a, n - a):
            if part:
                runs.append((cur, part, u))
                cur += part + gap
    T = cur + 1
    x = (rng.standard_normal((T, D + pad)) * (1 + np.arange(D + pad) / 7.0) + np.arange(D + pad)).astype(dtype)
    return x, np.array(runs, np.int64)


def run_dev(x, D, runs, U, nb, force=False, out_dtype=None, in_place=False, c=None, tables="host"):
    """-> (out [T, ld] numpy, bounds, count, status)"""
    import torch
    c = c or ctx()
    tb, tc = target()
    xd = dev(x)
    r = dev(runs) if tables == "device" else runs
    torch.cuda.synchronize()                    # a private context's stream is not ordered with torch's
    b, cn, st = fw.warp_hist(c, xd[:, :D], r, U, nb, force_select=force)
    if in_place:
        od = xd
    else:
        od = torch.full(x.shape, -77.0, dtype=torch.float64 if (out_dtype or x.dtype) == np.float64 else torch.float32, device="cuda")
    tbd, tcd = (dev(tb), dev(tc)) if tables == "device" else (tb, tc)
    torch.cuda.synchronize()
    fw.warp_apply(c, xd[:, :D], r, U, b, cn, st, tbd, tcd, out=od[:, :D])
    c.sync()
    torch.cuda.synchronize()
    return od.cpu().numpy(), b, cn, st


def value_bar(x, b, cn, tb, tc):
    """the bar of the module docstring for one column -> (bar [n], long double values)"""
    ld = np.longdouble
    bl, cl, _ = W.histo(x, len(cn), ld)
    y64, iw64, j64, _ = W.warp_column(x, b, cn, tb, tc, detail=True)
    yl, iw, j, tw = W.warp_column(x, bl, cl, tb.astype(ld), tc.astype(ld), ld, detail=True)
    ta = (tc * np.diff(tb)).astype(np.float64)
    T = np.concatenate([[0.0], np.cumsum(ta)])
    w, I = np.diff(tb)[j], ta[j]
    tw, yl64 = tw.astype(np.float64), yl.astype(np.float64)
    e_tw, e_td = (iw + 10) * U53 * np.abs(tw), (j + 6) * U53 * T[np.minimum(j + 1, len(ta))]
    ph = np.abs((yl64 - tb[j]) / w)
    bar = 2 * (w * ((e_tw + 2 * e_td) / I + ph * (2 * e_td + 3 * U53 * I) / I + 3 * U53 * ph) + 2 * U53 * (np.abs(tb[j]) + np.abs(yl64)))
    jump = 2 * np.max(np.diff(tb)[:-1] * np.abs(np.diff(ta)) / np.minimum(ta[1:], ta[:-1]))
    return bar + np.where(j != j64, jump, 0.0), yl64, float(np.mean(j != j64))


def check(x, D, runs, U, nb, got, judge=True):
    """got = run_dev(...) of an out-of-place or in-place call on x; the restatement is computed here"""
    out, b, cn, st = got
    tb, tc = target()
    ro, rb, rc, rs = W.warp_units(x[:, :D], runs, U, nb, tb, tc, out_dtype=out.dtype)
    assert np.array_equal(st, rs), "status"
    assert np.array_equal(b, rb, equal_nan=True), "bounds"
    ok = rs == 0
    assert np.array_equal(bits(cn[ok]), bits(rc[ok])) and np.array_equal(cn[~ok], rc[~ok], equal_nan=True), "count"
    rows = np.concatenate([W.unit_rows(runs, u) for u in range(U)]) if len(runs) else np.zeros(0, np.int64)
    assert np.array_equal(bits(out[rows, :D]), bits(ro[rows])), "warped values: %d differ" % np.sum(bits(out[rows, :D]) != bits(ro[rows]))
    worst = 0.0
    if judge and out.dtype == np.float64:
        for u in range(U):
            ur = W.unit_rows(runs, u)
            for c in range(D):
                if rs[u, c]:
                    assert np.array_equal(bits(out[ur, c].astype(x.dtype)), bits(x[ur, c])), "a degenerate column is copied through"
                    continue
                cl = W.histo(x[ur, c], nb, np.longdouble)[1]
                assert np.all(np.abs(cn[u, c] - cl) <= 4 * U53 * np.abs(cl))
                bar, yl, flipped = value_bar(x[ur, c], b[u, c], cn[u, c], tb, tc)
                ratio = np.abs(out[ur, c] - yl) / bar
                worst = max(worst, float(ratio.max()))
                assert np.all(ratio <= 1.0), (u, c, float(ratio.max()))
    return rows, worst


# ------------------------------------------------------------------------------------------------------------------- the shapes
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("D,nb", [(1, 2), (3, 40), (33, 2), (33, 40), (3, 2), (1, 40)])
def test_against_the_restatement(D, nb, f64):
    dtype = np.float64 if f64 else np.float32
    lens = [nb - 1, nb, nb + 1, 2 * nb - 1, 1000, 0, 1]
    x, runs = make(D, lens, dtype, 100 + D + nb)
    U = len(lens)
    got = run_dev(x, D, runs, U, nb, out_dtype=np.float64)
    rows, worst = check(x, D, runs, U, nb, got)
    print("D %d nbBin %d %s: worst |device - long double| / bar = %.3f" % (D, nb, dtype.__name__, worst))
    out = got[0]
    other = np.setdiff1d(np.arange(len(x)), rows)
    assert np.all(out[other] == -77.0) and np.all(out[:, D:] == -77.0)       # nothing outside the runs and the D columns is written
    st = got[3]
    assert st[0].all() and st[5].all() and st[6].all() and not st[4].any()    # n < nbBin, no frames, one frame: DEGENERATE; 1000 frames: not


@pytest.mark.parametrize("f64", [False, True])
def test_either_side_of_the_lds_sort_limit_and_the_forced_select(f64):
    dtype, cap = (np.float64, fw.WARP_SORT_CAP[capi.F64]) if f64 else (np.float32, fw.WARP_SORT_CAP[capi.F32])
    D, nb = 3, 40
    lens = [cap, cap + 1, 1000, 77]
    x, runs = make(D, lens, dtype, 5)
    a = run_dev(x, D, runs, 4, nb, out_dtype=np.float64)
    check(x, D, runs, 4, nb, a, judge=False)
    # every unit through the radix select, and through a device table (1024 threads, the full LDS): the same bits
    for kw in (dict(force=True), dict(tables="device")):
        g = run_dev(x, D, runs, 4, nb, out_dtype=np.float64, **kw)
        for p, q in zip(a, g):
            assert np.array_equal(bits(p), bits(q)), kw


def test_a_unit_does_not_depend_on_the_list_or_its_place():
    D, nb = 3, 40
    lens = [1000, 130, 41, 2000]
    x, runs = make(D, lens, np.float32, 9)
    out, b, cn, st = run_dev(x, D, runs, 4, nb)
    for u in (3, 1):                                    # alone, as unit 0 of a list of one
        ru = runs[runs[:, 2] == u].copy()
        ru[:, 2] = 0
        o1, b1, c1, s1 = run_dev(x, D, ru, 1, nb)
        rows = W.unit_rows(ru, 0)
        assert np.array_equal(bits(b1[0]), bits(b[u])) and np.array_equal(bits(c1[0]), bits(cn[u])) and np.array_equal(s1[0], st[u])
        assert np.array_equal(bits(o1[rows, :D]), bits(out[rows, :D]))
    # the units in reverse order of ids (the frames stay): unit u becomes 3 - u
    rr = np.concatenate([runs[runs[:, 2] == u] for u in (3, 2, 1, 0)])
    rr[:, 2] = 3 - rr[:, 2]
    o2, b2, c2, s2 = run_dev(x, D, rr, 4, nb)
    assert np.array_equal(bits(b2[::-1]), bits(b)) and np.array_equal(bits(c2[::-1]), bits(cn)) and np.array_equal(bits(o2), bits(out))


def test_ties_a_constant_column_and_nan():
    D, nb, n = 4, 10, 100
    x, runs = make(D, [n], np.float64, 3)
    rows = W.unit_rows(runs, 0)
    col = np.arange(100.0) * 0.25 - 7
    col[30:41] = col[30]                                # d[30] == d[40]: exactly one bin without width
    x[rows, 1] = np.random.default_rng(1).permutation(col)
    x[rows, 2] = 2.5                                    # constant
    got = run_dev(x, D, runs, 1, nb, in_place=True)
    out, b, cn, st = got
    assert list(st[0]) == [0, 1, 1, 0] and np.sum(np.diff(b[0, 1]) == 0) == 1 and np.all(np.diff(b[0, 2]) == 0)
    assert np.array_equal(bits(out[rows, 1]), bits(x[rows, 1])) and np.all(out[rows, 2] == 2.5)
    check(x, D, runs, 1, nb, (out, b, cn, st))          # the neighbours (columns 0 and 3) carry the restatement's bits
    # NaN: +NaN sorts above +inf into the last bound, -NaN below -inf into the first; the column is DEGENERATE and copied through
    for sign, where in ((1.0, nb), (-1.0, 0)):
        xn = x.copy()
        xn[rows[17], 0] = np.copysign(np.nan, sign)
        o, bn, cnn, stn = run_dev(xn, D, runs, 1, nb, in_place=True)
        assert list(stn[0]) == [1, 1, 1, 0] and np.isnan(bn[0, 0, where]) and np.sum(np.isnan(bn[0, 0])) == 1
        assert np.array_equal(bits(o[rows, 0]), bits(xn[rows, 0]))
        assert np.array_equal(bits(o[rows, 3]), bits(out[rows, 3])) and np.array_equal(bits(bn[0, 3]), bits(b[0, 3]))
        fo = run_dev(xn, D, runs, 1, nb, in_place=True, force=True)
        assert np.array_equal(bits(fo[1]), bits(bn)) and np.array_equal(fo[3], stn)
    xi = x.copy()
    xi[rows[5], 3], xi[rows[6], 3] = np.inf, -np.inf    # infinite bounds: a width is inf (its area would be 0 x inf) -- DEGENERATE, copied through
    gi = run_dev(xi, D, runs, 1, nb, in_place=True)
    assert list(gi[3][0]) == [0, 1, 1, 1] and np.array_equal(bits(gi[0][rows, 3]), bits(xi[rows, 3]))
    check(xi, D, runs, 1, nb, gi)


@pytest.mark.parametrize("f64", [False, True])
def test_in_place_out_of_place_and_one_rounding(f64):
    dtype = np.float64 if f64 else np.float32
    D, nb = 5, 40
    x, runs = make(D, [700, 333], dtype, 21)
    ip = run_dev(x, D, runs, 2, nb, in_place=True)
    op = run_dev(x, D, runs, 2, nb, out_dtype=dtype)
    o64 = run_dev(x, D, runs, 2, nb, out_dtype=np.float64)
    o32 = run_dev(x, D, runs, 2, nb, out_dtype=np.float32)
    rows = np.concatenate([W.unit_rows(runs, u) for u in range(2)])
    assert np.array_equal(bits(ip[0][rows, :D]), bits(op[0][rows, :D]))
    assert np.array_equal(bits(o32[0][rows, :D]), bits(o64[0][rows, :D].astype(np.float32)))       # rounded once, from the fp64 result
    assert np.array_equal(ip[0][:, D:], x[:, D:]) and np.array_equal(np.delete(ip[0], rows, 0), np.delete(x, rows, 0))
    check(x, D, runs, 2, nb, o64)


def test_overlap_is_refused_on_the_device_too():
    import torch
    D, nb = 3, 4
    x, runs = make(D, [50], np.float32, 2, pad=0)
    xd = dev(x)
    b, cn, st = fw.warp_hist(ctx(), xd, runs, 1, nb)
    tb, tc = target()
    with pytest.raises(capi.GmmivError, match="overlaps x without being x"):
        fw.warp_apply(ctx(), xd, runs, 1, b, cn, st, tb, tc, out=xd[1:])
    with pytest.raises(capi.GmmivError, match="same dtype and stride"):
        fw.warp_apply(ctx(), xd, runs, 1, b, cn, st, tb, tc, out=torch.as_strided(xd, (len(x) * D // (D + 1), D), (D + 1, 1)))
    with pytest.raises(capi.GmmivError, match="run 1 of unit 0 overlaps"):
        fw.warp_hist(ctx(), xd, np.array([[0, 10, 0], [5, 10, 0]]), 1, nb)


def test_the_kernel_timers():
    c = new_ctx()
    c.set_option("timing", 1)
    x, runs = make(3, [500], np.float32, 4)
    run_dev(x, 3, runs, 1, 40, c=c)
    assert c.kernel_ms("k_warp_hist") > 0 and c.kernel_ms("k_warp_apply") > 0 and c.kernel_launches("k_warp_hist") == 1
    c.close()


# ------------------------------------------------------------------------------------------------------------ suite-wide rules
def test_a_used_context_gives_a_fresh_contexts_bits():
    """the programme of tests/ws_history.py's NaN calls first (they leave NaN in the shared staging slots), then the two entry points"""
    import ws_history as wh
    D, nb = 33, 40
    x, runs = make(D, [1000, 41, 300], np.float32, 31)
    first = new_ctx()
    fresh = run_dev(x, D, runs, 3, nb, c=first)
    first.close()
    used = new_ctx()
    ok = wh.nan_calls(used)
    assert all(ok.values()), ok
    for kw in (dict(), dict(tables="device"), dict(force=True)):
        got = run_dev(x, D, runs, 3, nb, c=used, **kw)
        for p, q in zip(fresh, got):
            assert np.array_equal(bits(p), bits(q)), kw
    used.close()


@pytest.mark.parametrize("f64", [False, True])
def test_frames_beyond_2_31_elements_from_the_base(f64):
    """the far buffer of tests/far_addr.py (skipped with its reason when the device has no room): runs on either side of every
    threshold, in place and into a second far view is not possible (one window), so in place; the dense twin gives the bits"""
    import far_addr as fa
    dtype = np.float64 if f64 else np.float32
    D, nb = 3, 4
    far = fa.FarBuffer()
    try:
        fruns, frames = fa.far_runs(dtype, D)
        druns, dframes = fa.compact(fruns)
        view = far.dense(dtype, D, frames)
        rng = np.random.default_rng(77)
        data = [rng.standard_normal((n, D)).astype(dtype) for _, n in fruns]
        units = np.arange(len(fruns)) // 2                                  # two runs per unit: a unit straddles what its runs straddle
        U = int(units[-1]) + 1
        ft = np.array([(f, n, u) for (f, n), u in zip(fruns, units)], np.int64)
        dt = np.array([(f, n, u) for (f, n), u in zip(druns, units)], np.int64)
        xd = np.zeros((dframes, D), dtype)
        for (f, n), d in zip(druns, data):
            xd[f:f + n] = d
        dense = run_dev(xd, D, dt, U, nb, in_place=True)
        cells = [view[f:f + n] for f, n in fruns]
        tb, tc = target()

        def call():
            b, cn, st = fw.warp_hist(ctx(), view, ft, U, nb)
            fw.warp_apply(ctx(), view, ft, U, b, cn, st, tb, tc)
            ctx().sync()
            return b, cn, st
        (b, cn, st), got = far.run("feat_warp", call, inputs=list(zip(cells, data)), outputs=cells)
        fa.same_bits("bounds", b, dense[1])
        fa.same_bits("count", cn, dense[2])
        assert np.array_equal(st, dense[3]) and not st.all()
        for (f, n), g in zip(druns, got):
            fa.same_bits("warped frames", g, dense[0][f:f + n])
    finally:
        far.close()


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("segmental", [False, True])
@pytest.mark.parametrize("add01", [False, True])
def test_feat_warp_on_three_files(segmental, add01):
    """feat_warp (NormFeat.cpp:362-368 / 465-483 on resident frames): three files in one buffer, fileMode (a unit per file) and
    segmentalMode (a unit per segment), warpAdd01Norm on and off -- the warp against the restatement in bits, the 0/1 step against the
    moments / apply pair run on the restatement's frames."""
    import torch
    D, nb = 12, 40
    segs = [[(0, 900)], [(10, 400), (500, 450)], [(0, 300), (320, 90), (500, 200)]]
    first = [0, 1000, 2000]
    rng = np.random.default_rng(8)
    x = (rng.gamma(2.0, 1.5, (2800, D)) - 1).astype(np.float32)            # skewed: the warp has work to do
    file_runs = np.array([(first[f] + b, n, f) for f, ss in enumerate(segs) for b, n in ss], np.int64)
    runs = file_runs.copy()
    if segmental:
        runs[:, 2] = np.arange(len(runs))
    U = int(runs[-1, 2]) + 1
    tb, tc = target()
    xd = dev(x)
    out, st = fw.feat_warp(ctx(), xd, runs, U, tb, tc, nb, add01=add01, add01_runs=file_runs, add01_groups=3)
    torch.cuda.synchronize()
    assert out is xd and not st.any()
    want = W.warp_units(x, runs, U, nb, tb, tc)[0]
    if add01:
        wd = dev(want)
        acc = torch.zeros((3, 2 * D + 1), dtype=torch.float64, device="cuda")
        ctx().frame_moments_groups(wd, file_runs, 3, acc)
        mean, std = ctx().frame_moments_stats(acc, D)
        ctx().feat_norm_apply(wd, file_runs, mean, std, out=wd)
        torch.cuda.synchronize()
        want = wd.cpu().numpy()
    got = out.cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    rows = np.concatenate([np.arange(f, f + n) for f, n, _ in file_runs])
    sel = got[rows].astype(np.float64)
    assert abs(np.mean(sel)) < 0.05 and abs(np.std(sel) - 1) < 0.06         # Gaussianised (40 bins squeeze the tails: std 0.96, see the CPU test)
    assert np.array_equal(np.delete(got, rows, 0), np.delete(x, rows, 0))   # unselected frames keep their values
