"""TurnDetection on resident frames (include/gmmiv_turn.h: gmmiv_turn_curve, gmmiv_turn_pick, gmmiv_turn_segments).

  * every position's value against the long double restatement under its own bar (tests/turn_ref.py; nothing in it is fitted to an
    output), all three criteria, status bits exact, on the smallest shapes at which the kernel can go wrong: tiles of P - 1, P, P + 1 and
    2 P + 1 positions, runs of 0, 1, 2 and 2-or-3 positions, f32 and f64, a padded stride and a column slice, a file without runs,
    tables on the host and on the device;
  * a position's bits do not depend on its place in the tile, its run, its file or the call;
  * a constant column, a NaN feature, a clamp that bites;
  * gmmiv_turn_pick exactly on integer curves, and on random curves but for the positions whose margin is inside the rounding;
  * gmmiv_turn_segments: counts, fill, too little room, count-only;
  * a table of 2049 runs in 5 files (three chunks of the tile scan, a file of 600 runs, runs without positions on either side of the
    chunk borders): every position under its bar, every run's decisions, every file's segments;
  * device tables whose content arrives late on the context's stream;
  * the chain end to end through host_capi against the host twin, the true change points and the label files.
Largest |difference| / bar measured on an MI355X over the 20 670 judged values: 0.006; over the 15 990 of the 2049-run table (2026-10-21,
parent 32904a4, profiles/r29/turn_table_scale.json): 0.0033, its largest logcov_ratio 0.090 against the 1.4 the bar allows.  The bar is
derived, not fitted: a ratio above 1 fails the test."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import turn_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_STATE = {}
GUARD = 1e30                       # between the runs and in the padding columns: a read of it would wreck a value


def ctx():
    if "ctx" not in _STATE:
        import torch
        from lia_ral_amd import capi
        _STATE["ctx"] = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    return _STATE["ctx"]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def layout(lens_per_file, rng, gaps=(0, 1, 7)):
    """run table of the files' run lengths, guard frames in the gaps -> (runs [nrun, 3], T)"""
    runs, pos = [], 2
    for f, lens in enumerate(lens_per_file):
        for n in lens:
            runs.append((pos, n, f))
            pos += n + int(rng.choice(gaps))
        pos += 2
    return np.array(runs, np.int64).reshape(-1, 3), pos


def fill(runs, T, D, rng):
    """float32-representable frames on the runs (both dtypes then share one reference), GUARD elsewhere"""
    x = np.full((T, D), GUARD, np.float64)
    for b, n, _ in runs:
        x[b:b + n] = tr.draw_frames(rng, n, D, np.float32)
    return x


def case(D, W, S):
    """the run table of a shape: three files, the middle one without a run -> dict(runs, x, pos_off, ref [npos] of value_ld(GLR))"""
    key = ("case", D, W, S)
    if key not in _STATE:
        from lia_ral_amd import capi
        P = capi.turn_tile_positions(D, W, S)
        assert P >= 2
        rng = np.random.default_rng(7000 * D + 70 * W + S)
        L = lambda n: 2 * W + (n - 1) * S + 1                               # the shortest run of n positions
        lens = [[2 * W, 2 * W + 1, L(P + 1), 2 * W + 2, 5], [], [2 * W + S + 1, L(P - 1), L(P), L(2 * P + 1), 1]]
        runs, T = layout(lens, rng)
        x = fill(runs, T, D, rng)
        po = capi.plan_turn_positions(runs, 3, W, S)
        want = [tr.positions_as_written(int(n), W, S) for n in runs[:, 1]]
        assert list(np.diff(po)) == want and want[2] == P + 1 and want[8] == 2 * P + 1 and want[0] == 0 and want[1] == 1
        ref = []
        for (b, n, _), k in zip(runs, want):
            ref += [tr.value_ld(x[b + i * S:b + i * S + 2 * W], W, tr.GLR) for i in range(k)]
        assert max(tr.logcov_ratio(x[b + i * S:b + i * S + 2 * W], W) for (b, n, _), k in zip(runs, want) for i in range(k)) <= 1.4
        _STATE[key] = dict(runs=runs, x=x, pos_off=po, ref=ref, P=P, T=T)
    return _STATE[key]


def judge(value, status, ref, D, W, S, crit, what):
    """every position under its own bar, status exact -> the largest |difference| / bar"""
    worst = 0.0
    pen = tr.LD(0.5 * (2 * D + 1)) * np.log(tr.LD(2 * W))
    for p, r in enumerate(ref):
        assert int(status[p]) == r["status"], "%s: position %d: status %d, the restatement has %d" % (what, p, status[p], r["status"])
        if r["status"] & tr.BAD_COV:
            assert np.isnan(value[p]), "%s: position %d has a bad covariance and the value %r" % (what, p, value[p])
            continue
        g = r["value"]
        want = g if crit == "GLR" else (-g if crit == "DGLR" else -g - pen)
        ratio = float(abs(tr.LD(value[p]) - want)) / tr.bar(r, D, W, S)
        print("%s %s position %d: value %.17g |difference| / bar %.3g" % (what, crit, p, value[p], ratio))
        assert ratio <= 1.0, "%s: position %d: %r against %r, %.3g bars" % (what, p, value[p], float(want), ratio)
        worst = max(worst, ratio)
    return worst


SHAPES = [(D, W, S) for D in (1, 3, 17, 60, 64) for (W, S) in ((4, 1), (4, 3), (5, 5), (8, 3), (50, 5))]


@pytest.mark.parametrize("f64", [0, 1], ids=["f32_slice_device_tables", "f64_padded_host_tables"])
@pytest.mark.parametrize("D,W,S", SHAPES, ids=["D%d_W%d_S%d" % s for s in SHAPES])
def test_every_position_against_long_double_under_its_own_bar(D, W, S, f64):
    """f64: a padded stride (ldx = D + 3) and host tables; f32: columns [2, 2 + D) of a wider matrix and device tables"""
    import torch
    c = ctx()
    k = case(D, W, S)
    runs, po, ref = k["runs"], k["pos_off"], k["ref"]
    lead, pad = (0, 3) if f64 else (2, 5)
    wide = np.full((k["T"], lead + D + pad), GUARD, np.float64 if f64 else np.float32)
    wide[:, lead:lead + D] = k["x"]
    xd = dev(wide)
    view = xd[:, lead:lead + D]
    npos = int(po[-1])
    for crit in ("GLR", "DGLR", "BIC"):
        if f64:
            v, st = c.turn_curve(view, runs, 3, po, W, S, crit)
        else:
            v = torch.full((npos,), -7.0, dtype=torch.float64, device="cuda")
            st = torch.full((npos,), -7, dtype=torch.int32, device="cuda")
            c.turn_curve(view, dev(runs), 3, dev(po), W, S, crit, value=v, status=st, npos=npos)
            c.sync()
            v, st = v.cpu().numpy(), st.cpu().numpy()
        judge(v, st, ref, D, W, S, crit, "D %d W %d S %d %s" % (D, W, S, "f64" if f64 else "f32"))
    assert torch.equal(xd.cpu(), torch.from_numpy(wide)), "the frames are read only"


def test_a_window_that_does_not_fit_the_lds_is_refused():
    import torch
    from lia_ral_amd import capi
    assert capi.turn_tile_positions(60, 50, 5) >= 8 and capi.turn_tile_positions(60, 400, 5) == 0 and capi.turn_tile_positions(0, 50, 5) == 0
    runs = np.array([[0, 900, 0]], np.int64)
    po = capi.plan_turn_positions(runs, 1, 400, 5)
    with pytest.raises(capi.GmmivError, match="do not fit the LDS"):
        ctx().turn_curve(torch.zeros((900, 60), device="cuda"), runs, 1, po, 400, 5)


# ---------------------------------------------------------------------------------------------------------------- invariance
@pytest.mark.parametrize("D,W,S", [(17, 8, 3), (60, 50, 5), (3, 4, 1)])
def test_a_position_does_not_depend_on_its_tile_its_run_its_file_or_the_call(D, W, S):
    from lia_ral_amd import capi
    c = ctx()
    P = capi.turn_tile_positions(D, W, S)
    rng = np.random.default_rng(11 * D + W)
    F = tr.draw_frames(rng, 2 * W, D, np.float32)
    slots = [0, P // 2, P - 1, P, 2 * P + 1]                                 # first, middle, last of a tile; the next tiles
    lens = [[slot * S + 2 * W + 3 * S + 1 for slot in slots[:3]], [7], [slot * S + 2 * W + 1 for slot in slots[3:]]]
    runs, T = layout(lens, rng)
    x = fill(runs, T, D, rng)
    where = []
    po = capi.plan_turn_positions(runs, 3, W, S)
    planted = [r for r in range(len(runs)) if runs[r, 1] > 7]
    for r, slot in zip(planted, slots):
        b = int(runs[r, 0])
        x[b + slot * S:b + slot * S + 2 * W] = F
        where.append(int(po[r]) + slot)
    got = []
    for f64 in (0, 1):
        v, st = c.turn_curve(dev(x.astype(np.float64 if f64 else np.float32)), runs, 3, po, W, S, "BIC")
        got += [v[p] for p in where]
        assert not st[where].any()                                          # (a window over the seam of two draws may well be clamped)
    # another call: the frames alone, one run, one file
    v1, _ = c.turn_curve(dev(np.concatenate([F, F[:1]])), np.array([[0, 2 * W + 1, 0]], np.int64), 1, np.array([0, 1], np.int64), W, S, "BIC")
    got.append(v1[0])
    assert all(same_bits(g, got[0]) for g in got), got
    r = tr.value_ld(F, W, tr.BIC)
    assert abs(tr.LD(got[0]) - r["value"]) <= tr.bar(r, D, W, S)


# ---------------------------------------------------------------------------------------------------------------- degenerate
def _one_run(D, W, S, npos, seed):
    rng = np.random.default_rng(seed)
    L = 2 * W + (npos - 1) * S + 1
    return tr.draw_frames(rng, L, D, np.float32).astype(np.float64), np.array([[0, L, 0]], np.int64), np.array([0, npos], np.int64)


def _refs(x, W, S, npos, crit=tr.GLR, **kw):
    return [tr.value_ld(x[i * S:i * S + 2 * W], W, crit, **kw) for i in range(npos)]


def test_a_constant_column_gives_nan_and_the_flag_and_leaves_the_neighbours_alone():
    D, W, S, npos = 5, 8, 4, 20
    x, runs, po = _one_run(D, W, S, npos, 5)
    k = 9
    x[k * S:k * S + W, 2] = 1.0                                             # c1 of position 9 = c2 of position 7
    ref = _refs(x, W, S, npos)
    assert [p for p, r in enumerate(ref) if r["status"]] == [k - W // S, k]
    v, st = ctx().turn_curve(dev(x), runs, 1, po, W, S, "GLR")
    judge(v, st, ref, D, W, S, "GLR", "constant column")


def test_a_nan_feature_goes_through_the_moments():
    D, W, S, npos = 3, 5, 5, 12
    x, runs, po = _one_run(D, W, S, npos, 6)
    x[33, 1] = np.nan
    ref = _refs(x, W, S, npos)
    bad = [p for p, r in enumerate(ref) if r["status"]]
    assert bad == [p for p in range(npos) if p * S <= 33 < p * S + 2 * W] and 0 < len(bad) < npos
    v, st = ctx().turn_curve(dev(x), runs, 1, po, W, S, "DGLR")
    judge(v, st, ref, D, W, S, "DGLR", "NaN feature")


@pytest.mark.parametrize("bound", ["min_llk", "max_llk"])
def test_the_clamp_acts_on_exactly_the_planted_positions(bound):
    D, W, S, npos = 12, 50, 5, 30
    x, runs, po = _one_run(D, W, S, npos, 8)
    row = 2 * W + 40
    x[row] = np.float32(x[row] + 60.0)                                      # far out in every column: q = 49 D / 2 -> llk below -200
    kw = dict(min_llk=-200.0, max_llk=200.0)
    if bound == "max_llk":                                                  # a ceiling between the best frames of a third of the positions and of the rest
        x, runs, po = _one_run(D, W, S, npos, 9)
        tops = [r["max_l"] for r in _refs(x, W, S, npos)]                   # (overlapping positions share windows, and with them their best frame)
        uniq = sorted(set(tops))
        lo, hi = uniq[2 * len(uniq) // 3 - 1], uniq[2 * len(uniq) // 3]
        assert hi - lo > 1e-9
        kw = dict(min_llk=-1e6, max_llk=0.5 * (lo + hi))
    ref = _refs(x, W, S, npos, **kw)
    acted = [p for p, r in enumerate(ref) if r["status"] == tr.CLAMPED]
    if bound == "min_llk":
        assert acted == [p for p in range(npos) if p * S <= row < p * S + 2 * W] and 0 < len(acted) < npos
    else:
        assert acted == [p for p in range(npos) if tops[p] > kw["max_llk"]] and 0 < len(acted) < npos, acted
    v, st = ctx().turn_curve(dev(x), runs, 1, po, W, S, "GLR", **kw)
    judge(v, st, ref, D, W, S, "GLR", "clamp " + bound)


# ---------------------------------------------------------------------------------------------------------------- pick
def exact_curves():
    rng = np.random.default_rng(3)
    nan_mid = [4.0, 9, 2, 7, float("nan"), 8, 1, 6, 3, 9, 0]
    curves = [[5.0], [5.0, 9], [1.0, 8, 2], [0.0, 8, 0], [3.0] * 9, [1.0, 4, 4, 4, 1, 1, 6, 6, 2, 2, 7, 0], list(map(float, range(1, 40))),
              list(map(float, range(40, 1, -1))), nan_mid, [0.0, 4, 8, 4, 0, 4, 8, 4, 0]]
    curves += [list(rng.integers(-50, 50, n).astype(np.float64)) for n in (4, 17, 255, 256, 257, 300, 1000)]
    return curves


def run_pick(curves, alpha, device_tables=False):
    import torch
    po = np.concatenate([[0], np.cumsum([len(c) for c in curves])]).astype(np.int64)
    v = np.concatenate([np.asarray(c, np.float64) for c in curves])
    if not device_tables:
        return po, ctx().turn_pick(v, po, alpha)
    n, nr = len(v), len(curves)
    out = (torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"),
           torch.zeros((nr, 2), dtype=torch.float64, device="cuda"), torch.zeros(nr, dtype=torch.int64, device="cuda"))
    ctx().turn_pick(dev(v), dev(po), alpha, *out)
    ctx().sync()
    return po, tuple(o.cpu().numpy() for o in out)


@pytest.mark.parametrize("device_tables", [False, True])
def test_pick_on_exact_curves_equals_the_loop_as_written(device_tables):
    """integer curves, alpha a power of two: the smoothed values and both sums are exact in any order"""
    curves = exact_curves() + [[]]                                          # and a run without positions
    for alpha in (0.5, 0.25, 2.0):
        po, (sm, dec, rs, nt) = run_pick(curves, alpha, device_tables)
        for r, cv in enumerate(curves):
            lo, hi = int(po[r]), int(po[r + 1])
            if not cv:
                assert np.isnan(rs[r]).all() and nt[r] == 0
                continue
            wsm, wdec, mean, std = tr.pick_as_written(cv, alpha)
            assert same_bits(sm[lo:hi], wsm), (r, sm[lo:hi], wsm)
            assert same_bits(rs[r], [mean, std]), (r, rs[r], mean, std)
            assert (dec[lo:hi] == wdec).all() and nt[r] == wdec.sum(), (r, alpha, dec[lo:hi], wdec)
    assert any(tr.pick_as_written(cv, 0.5)[1].any() for cv in curves if cv)


def random_curves():
    rng = np.random.default_rng(17)
    return [list(np.cumsum(rng.normal(0, 1, n)) * 0.3 + rng.normal(0, 1, n)) for n in (3, 50, 256, 700, 1200)]


def test_pick_on_random_curves_but_for_margins_inside_the_rounding():
    curves, alpha = random_curves(), 0.7
    po, (sm, dec, rs, nt) = run_pick(curves, alpha)
    left_out = total = 0
    for r, cv in enumerate(curves):
        lo, hi = int(po[r]), int(po[r + 1])
        wsm, wdec, mean, std = tr.pick_as_written(cv, alpha)
        assert same_bits(sm[lo:hi], wsm)                                    # the smoothing has one order
        n = len(cv)
        assert abs(rs[r, 0] - mean) <= 4 * n * tr.U * np.abs(wsm).mean() and abs(rs[r, 1] - std) <= 16 * n * tr.U * (np.abs(wsm).max() ** 2) / max(std, 1e-300)
        mar, wid = tr.pick_margins(wsm, alpha, float(std), n)
        keep = mar > wid
        left_out += int((~keep).sum())
        total += n
        assert (dec[lo:hi][keep] == wdec[keep]).all()
    assert left_out <= 0.01 * total, (left_out, total)


# ---------------------------------------------------------------------------------------------------------------- segments
def seg_table():
    rng = np.random.default_rng(23)
    W, S = 6, 4
    lens = [[3, 13, 14, 40, 12], [], [100, 2 * W + 1], [61]]
    runs, T = layout(lens, rng)
    n = [tr.positions_as_written(int(L), W, S) for L in runs[:, 1]]
    po = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    dec = (rng.random(int(po[-1])) < 0.3).astype(np.uint8)
    dec[int(po[3])] = 1                                                     # a caller's array: the first and the last position may be set
    dec[int(po[4]) - 1] = 1
    want = [[] for _ in lens]
    for r, (b, L, f) in enumerate(runs):
        want[f] += tr.segments_as_written(int(b), int(L), W, S, dec[int(po[r]):int(po[r + 1])])
    return W, S, runs, po, dec, want


@pytest.mark.parametrize("device_tables", [False, True])
def test_segments_counts_fill_and_too_little_room(device_tables):
    import torch
    W, S, runs, po, dec, want = seg_table()
    nf = len(want)
    c = ctx()
    up = dev if device_tables else (lambda a: a)
    cnt = c.turn_segments(up(runs), nf, up(po), up(dec), W, S, seg_count=up(np.full(nf, -1, np.int64)), npos=len(dec))        # count only
    c.sync()
    cnt = cnt.cpu().numpy() if device_tables else cnt
    assert list(cnt) == [len(w) for w in want] and cnt[1] == 0 and cnt[0] > 5
    # the fill: file 0 gets two entries too few, file 2 three too many; guard bands around the whole
    room = cnt.copy()
    room[0] -= 2
    room[2] += 3
    off = np.concatenate([[0], np.cumsum(room)]).astype(np.int64) + 4
    off[0] = 4
    tot = int(off[-1]) + 4
    sb, sl = np.full(tot, -9, np.int64), np.full(tot, -9, np.int64)
    if device_tables:
        dsb, dsl = dev(sb), dev(sl)
        c.turn_segments(dev(runs), nf, dev(po), dev(dec), W, S, seg_off=dev(off), seg_begin=dsb, seg_len=dsl, npos=len(dec))
        c.sync()
        sb, sl = dsb.cpu().numpy(), dsl.cpu().numpy()
    else:
        # a host seg_off counts from 0: the guard bands are the slices around what the call is given
        offh = off - 4
        c.turn_segments(runs, nf, po, dec, W, S, seg_off=offh, seg_begin=sb[4:4 + int(offh[-1])], seg_len=sl[4:4 + int(offh[-1])])
    for f in range(nf):
        lo, hi = int(off[f]), int(off[f + 1])
        k = min(hi - lo, len(want[f]))
        assert [(int(a), int(b)) for a, b in zip(sb[lo:lo + k], sl[lo:lo + k])] == want[f][:k], f
        assert (sb[lo + k:hi] == -9).all() and (sl[lo + k:hi] == -9).all(), "file %d: the room no segment fills keeps its values" % f
    assert (sb[:4] == -9).all() and (sb[int(off[-1]):] == -9).all() and (sl[:4] == -9).all() and (sl[int(off[-1]):] == -9).all()


# ---------------------------------------------------------------------------------------------------------------- table scale
SCALE = (3, 4, 3)                  # D, W, S
SCALE_FILES = (700, 600, 748, 0, 1)
# kinds of run by the positions they hold: the shortest runs of 0 (L = 5), 0 (L = 2 W), 1, 2 and P + 1 positions.  A cycle of ten: runs
# 1023 and 2048 (index 3 and 8) have positions, runs 0, 1024 and 2047 (index 0, 4 and 7) have none; 9 -> 0 and 7 .. are runs without
# positions in a row; one run of P + 1 in ten keeps the long double restatement to about 8 000 positions
SCALE_CYCLE = ("0a", "2", "0b", "P+1", "0a", "1", "2", "0b", "1", "0b")


def scale_table():
    """2049 runs in 5 files -- two full chunks of k_turn_tiles and a chunk of one; file 1 has 600 runs (more than two strides of
    k_turn_segments), file 3 none, file 4 the last run alone -> dict(runs, T, x, pos_off, ref, P, ratio)"""
    if "scale" not in _STATE:
        from lia_ral_amd import capi
        D, W, S = SCALE
        P = capi.turn_tile_positions(D, W, S)
        assert P >= 2
        L = {"0a": 5, "0b": 2 * W, "1": 2 * W + 1, "2": 2 * W + S + 1, "P+1": 2 * W + P * S + 1}
        rng = np.random.default_rng(2049)
        lens, k = [], 0
        for n in SCALE_FILES:
            lens.append([L[SCALE_CYCLE[(k + i) % len(SCALE_CYCLE)]] for i in range(n)])
            k += n
        assert k == 2049
        runs, T = layout(lens, rng)
        x = fill(runs, T, D, rng)
        po = capi.plan_turn_positions(runs, len(SCALE_FILES), W, S)
        want = [tr.positions_as_written(int(n), W, S) for n in runs[:, 1]]
        assert list(np.diff(po)) == want and sorted(set(want)) == [0, 1, 2, P + 1]
        assert want[1023] > 0 and want[1024] == 0 and want[2047] == 0 and want[2048] > 0 and want[0] == 0
        assert [int((runs[:, 2] == f).sum()) for f in range(5)] == list(SCALE_FILES) and runs[2048, 2] == 4
        ref, ratio = [], 0.0
        for (b, n, _), k in zip(runs, want):
            for i in range(k):
                w = x[b + i * S:b + i * S + 2 * W]
                ref.append(tr.value_ld(w, W, tr.GLR))
                ratio = max(ratio, tr.logcov_ratio(w, W))
        assert ratio <= 1.4, ratio                                          # the derived bar applies (turn_ref: sum |log cov| <= 1.4 sum (1 + kappa))
        print("table scale: %d runs, %d positions, largest logcov_ratio %.3f" % (len(runs), len(ref), ratio))
        _STATE["scale"] = dict(runs=runs, T=T, x=x, pos_off=po, ref=ref, P=P, ratio=ratio, want=want)
    return _STATE["scale"]


def test_a_table_of_2049_runs_is_judged_per_position_run_and_file():
    """the table-scale paths of turn_detect.hip: the chunked scan with its carry (k_turn_tiles), the binary search over tile_off with
    its ties (k_turn_curve), the stride over a file's runs (k_turn_segments).  A wrong carry or tie puts right values at wrong
    positions: every position is judged, every run's decisions and every file's segments are compared.
    The table cannot both end with a run without positions and have positions in run 2048, its last: the full table ends with
    positions, and its first 2048 runs -- exactly two chunks, ending with a run without -- are run as a table of their own"""
    import torch
    c = ctx()
    D, W, S = SCALE
    k = scale_table()
    runs, po, ref = k["runs"], k["pos_off"], k["ref"]
    nf, npos, nrun = len(SCALE_FILES), int(po[-1]), len(runs)
    G = 64
    worst, values = 0.0, {}
    for f64 in (0, 1):
        xd = dev(k["x"].astype(np.float64 if f64 else np.float32))
        v = torch.full((npos + 2 * G,), -7.0, dtype=torch.float64, device="cuda")
        st = torch.full((npos + 2 * G,), -7, dtype=torch.int32, device="cuda")
        if f64:                                                             # host tables; the outputs stay on the device between their guard bands
            c.turn_curve(xd, runs, nf, po, W, S, "GLR", value=v[G:G + npos], status=st[G:G + npos], npos=npos)
        else:
            c.turn_curve(xd, dev(runs), nf, dev(po), W, S, "GLR", value=v[G:G + npos], status=st[G:G + npos], npos=npos)
        c.sync()
        v, st = v.cpu().numpy(), st.cpu().numpy()
        what = "2049 runs %s" % ("f64 host tables" if f64 else "f32 device tables")
        assert (v[:G] == -7.0).all() and (v[G + npos:] == -7.0).all() and (st[:G] == -7).all() and (st[G + npos:] == -7).all(), what + ": a guard band was written"
        assert (st[G:G + npos] != -7).all() and not (v[G:G + npos] == -7.0).any(), what + ": a position was not written"
        worst = max(worst, judge(v[G:G + npos], st[G:G + npos], ref, D, W, S, "GLR", what))
        values[f64] = v[G:G + npos]
    print("table scale: largest |difference| / bar over %d judged values: %.3g; largest logcov_ratio %.3f" % (2 * npos, worst, k["ratio"]))
    # the first 2048 runs alone: two full chunks and no third, the last run without positions; a position's bits do not depend on the call
    n2 = int(po[2048])
    v2, st2 = c.turn_curve(dev(k["x"]), runs[:2048], nf, po[:2049], W, S, "GLR")
    assert k["want"][2047] == 0 and same_bits(v2, values[1][:n2]) and not st2.any()
    # pick: an integer curve over the same CSR, alpha a power of two -- exact in any order
    rng = np.random.default_rng(4)
    curve = rng.integers(-50, 50, npos).astype(np.float64)
    sm, dec, rs, nt = c.turn_pick(curve, po, 0.5)
    turns = 0
    for r in range(nrun):
        lo, hi = int(po[r]), int(po[r + 1])
        if hi == lo:
            assert np.isnan(rs[r]).all() and nt[r] == 0, r
            continue
        wsm, wdec, mean, std = tr.pick_as_written(curve[lo:hi], 0.5)
        assert same_bits(sm[lo:hi], wsm) and same_bits(rs[r], [mean, std]), r
        assert (dec[lo:hi] == wdec).all() and nt[r] == wdec.sum(), r
        turns += int(wdec.sum())
    assert turns > 100
    # segments of those decisions: count, then fill
    want = [[] for _ in range(nf)]
    for r, (b, L, f) in enumerate(runs):
        want[f] += tr.segments_as_written(int(b), int(L), W, S, dec[int(po[r]):int(po[r + 1])])
    cnt = c.turn_segments(runs, nf, po, dec, W, S)
    assert list(cnt) == [len(w) for w in want] and cnt[1] > 600 and cnt[3] == 0 and cnt[4] >= 1
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    sb, sl = np.full(int(off[-1]) + 4, -9, np.int64), np.full(int(off[-1]) + 4, -9, np.int64)
    c.turn_segments(runs, nf, po, dec, W, S, seg_off=off, seg_begin=sb, seg_len=sl)
    for f in range(nf):
        got = [(int(a), int(b)) for a, b in zip(sb[int(off[f]):int(off[f + 1])], sl[int(off[f]):int(off[f + 1])])]
        assert got == want[f], "file %d: first difference at segment %d" % (f, next(i for i, (g, w) in enumerate(zip(got, want[f])) if g != w))
    assert (sb[int(off[-1]):] == -9).all() and (sl[int(off[-1]):] == -9).all()
    # and with every table on the device: the same counts and segments
    dcnt = dev(np.full(nf, -3, np.int64))
    dsb, dsl = dev(np.full(len(sb), -9, np.int64)), dev(np.full(len(sl), -9, np.int64))
    c.turn_segments(dev(runs), nf, dev(po), dev(dec), W, S, seg_off=dev(off), seg_begin=dsb, seg_len=dsl, seg_count=dcnt, npos=npos)
    c.sync()
    assert (dcnt.cpu().numpy() == cnt).all() and (dsb.cpu().numpy() == sb).all() and (dsl.cpu().numpy() == sl).all()
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------- stream order
def test_device_tables_written_late_on_the_stream():
    """every array a device pointer: the three calls only enqueue, and read their inputs in stream order -- they hold poison when the
    calls are made and become right behind a spin kernel on the context's stream (the helpers of tests/stream_order.py)"""
    import torch
    from lia_ral_amd import capi
    import stream_order as so
    D, W, S = 17, 8, 3
    k = case(D, W, S)
    runs, po = k["runs"], k["pos_off"]
    npos = int(po[-1])
    c = capi.Context(0)                                                     # a private stream
    be = so.TorchBackend(capi.lib, c)
    true = [dev(k["x"]), dev(runs), dev(po)]

    def outputs(fill):
        return dict(value=torch.full((npos,), fill, dtype=torch.float64, device="cuda"), status=torch.full((npos,), int(fill), dtype=torch.int32, device="cuda"),
                    sm=torch.full((npos,), fill, dtype=torch.float64, device="cuda"), dec=torch.full((npos,), 9, dtype=torch.uint8, device="cuda"),
                    rs=torch.full((len(runs), 2), fill, dtype=torch.float64, device="cuda"), nt=torch.full((len(runs),), -3, dtype=torch.int64, device="cuda"),
                    cnt=torch.full((3,), -3, dtype=torch.int64, device="cuda"))

    def chain(x, r, p, o):
        c.turn_curve(x, r, 3, p, W, S, "DGLR", value=o["value"], status=o["status"], npos=npos)
        c.turn_pick(o["value"], p, 0.5, o["sm"], o["dec"], o["rs"], o["nt"], npos=npos)
        c.turn_segments(r, 3, p, o["dec"], W, S, seg_count=o["cnt"], npos=npos)

    ref = outputs(-7.0)
    torch.cuda.synchronize()
    chain(true[0], true[1], true[2], ref)
    c.sync()
    live = [t.clone() for t in true]
    got = outputs(-5.0)
    torch.cuda.synchronize()
    for t, src in zip(live, true):                                          # poison: -(a) - 1 for the floats, zeros for the tables
        be.write_now(t, so.poison(src))
    be.spin(so.SPIN_CYCLES)
    for t, src in zip(live, true):
        be.enqueue_copy(t, src)
    ev = be.mark()
    assert be.probe(live[0]) == so.poison(true[0]).flatten()[0].item()      # the restoring copies wait behind the spin
    chain(live[0], live[1], live[2], got)
    busy = be.busy(ev)
    c.sync()
    torch.cuda.synchronize()
    assert busy, "the calls returned after the stream had drained: they did not only enqueue"
    for name in ref:
        a, b = ref[name].cpu().numpy(), got[name].cpu().numpy()
        assert same_bits(a, b) if a.dtype == np.float64 else (a == b).all(), name
    # and the device tables give the bits of the host tables
    v, st = ctx().turn_curve(dev(k["x"]), runs, 3, po, W, S, "DGLR")
    assert same_bits(v, ref["value"].cpu().numpy()) and (st == ref["status"].cpu().numpy()).all()
    assert ref["cnt"].cpu().numpy().sum() >= len(runs)
    c.close()


# ---------------------------------------------------------------------------------------------------------------- end to end
def talk():
    """three files of two alternating "speakers", D = 12: one segment, two segments with a gap, one segment and a short one"""
    if "talk" not in _STATE:
        files = [tr.speakers(n, 12, 40 + k) for k, n in enumerate((1500, 1260, 930))]
        segs = [(np.array([0]), np.array([1500])), (np.array([10, 700]), np.array([650, 560])), (np.array([0, 905]), np.array([900, 25]))]
        _STATE["talk"] = (files, segs)
    return _STATE["talk"]


def test_end_to_end_against_the_host_twin_and_the_true_change_points(tmp_path):
    import struct
    from lia_ral_amd import host_capi as h
    files, segs = talk()
    xs = [f[0] for f in files]
    W, S, alpha = 50, 5, 0.7
    got = h.turn_detection_batch(xs, segs)                                  # the reference's defaults
    twin = h.turn_detection_batch(xs, segs, twin=True)
    left = total = 0
    for f, (g, t) in enumerate(zip(got, twin)):
        exact = True
        for cg, ct in zip(g["curves"], t["curves"]):
            n = len(ct["value"])
            assert len(cg["value"]) == n
            if n == 0:
                continue
            mar, wid = tr.pick_margins(ct["smoothed"], alpha, ct["std"], n)
            keep = mar > wid
            left += int((~keep).sum())
            total += n
            exact = exact and bool(keep.all())
            assert (cg["dec"][keep] == ct["dec"][keep]).all()
            assert np.allclose(cg["value"], ct["value"], rtol=0, atol=1e-6)
        if exact:
            assert g["begin"].tolist() == t["begin"].tolist() and g["length"].tolist() == t["length"].tolist(), f
        # every true change point inside an input segment (a window's width from its ends) is found within W frames
        for b, n in zip(*segs[f]):
            for cp in files[f][1]:
                if b + 2 * W <= cp <= b + n - 2 * W:
                    assert min(abs(int(v) - cp) for v in g["begin"]) <= W, (f, cp, g["begin"])
        # the pieces tile the input segments
        assert int(g["length"].sum()) == int(segs[f][1].sum())
    assert total > 500 and left <= 0.01 * total
    # the same list through files
    d = str(tmp_path) + os.sep
    for k, x in enumerate(xs):
        with open(d + "f%d.prm" % k, "wb") as fo:
            fo.write(struct.pack("<4I", 2, x.shape[1], len(x), 0))
            fo.write(x.tobytes())
        with open(d + "f%d.lbl" % k, "w") as fo:
            for b, n in zip(*segs[k]):
                fo.write("%g %g talk\n" % (int(b) * 0.01, (int(b) + int(n) - 1) * 0.01))
            fo.write("0 0.05 music\n")                                      # another label: not selected
    names = ["f0", "f1", "f2"]
    out = h.turn_detection_files(names, feature_path=d, label_path=d, label="talk", save_path=d, save_ext=".turn.lbl")
    for k, name in enumerate(names):
        assert out[k][0].tolist() == got[k]["begin"].tolist() and out[k][1].tolist() == got[k]["length"].tolist()
        lines = open(d + name + ".turn.lbl").read().split("\n")[:-1]
        assert lines == ["%g %g talk" % (int(b) * 0.01, (int(b) + int(n) - 1) * 0.01) for b, n in zip(got[k]["begin"], got[k]["length"])]
        back = [(int(round(float(l.split()[0]) * 100)), int(round(float(l.split()[1]) * 100))) for l in lines]
        assert back == [(int(b), int(b) + int(n) - 1) for b, n in zip(got[k]["begin"], got[k]["length"])]
    with pytest.raises(h.HostError, match="DELTABIC"):
        h.turn_detection_batch(xs, segs, "DELTABIC")
