"""NormFeat's default mode (gmmiv_frame_moments_groups / _stats / gmmiv_feat_norm_apply, liagpu::normFeat) and the online mode of
NormFeatWindowMode (gmmiv_feat_norm_online) on resident frames.

The references are the tools' loops restated here as sequential fp64 numpy (NormFeat.cpp:340-370, :448-464; GeneralTools.cpp:670-682;
NormFeatWindowMode.cpp:85-137, :243-296).  Bounds, none of them fitted to the library's output:
  * sums of a group of n frames: |S - S_seq| <= (n - 1) 2^-53 sum|x| (any order of n - 1 additions against any other);
  * mean / std from the library's own accumulator and computeZeroOne from given mean / std: bit for bit (every operation is one IEEE
    operation rounded on its own);
  * two passes: the sum bounds propagated through mean, variance, std and (x - mean) / std, plus one f32 ulp per pass (_pass_ref);
  * online mode: W' 2^-53 (max|x| / c_t + |out_t|) per element with the reference's c_t (max over the file, per dimension), plus one
    ulp of an f32 output -- the recurrences forget a rounding error at the rate they forget a frame, W' errors are alive at a time."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
_STATE = {}


def ctx():
    """one context for the module, on torch's current stream (the tensors below are written and read by torch on that stream)"""
    if "ctx" not in _STATE:
        import torch
        from lia_ral_amd import capi
        _STATE["ctx"] = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    return _STATE["ctx"]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def seqsum(a):
    """sequential fp64 sum over the rows (cumsum adds left to right)"""
    return np.cumsum(a, axis=0)[-1] if len(a) else np.zeros(a.shape[1])


# ---- the run table of tests (1) - (3): lengths 1, 2, 63, 64, 65, 257, 5000; a group of one run, a group of three non-adjacent runs, an
# empty group between two others, a group of two runs, a group of one
LENS = {"a": 5000, "b": 1, "c": 63, "d": 257, "e": 2, "f": 64, "g": 65}
ORDER_IN_BUFFER = "cagbfed"                      # where the runs lie in the buffer (not the table's order), 3 frames between them
TABLE = [("a", 0), ("b", 1), ("c", 1), ("d", 1), ("e", 3), ("f", 3), ("g", 4)]
NGROUPS = 5


def run_table():
    if "runs" not in _STATE:
        first, pos = {}, 2
        for name in ORDER_IN_BUFFER:
            first[name] = pos
            pos += LENS[name] + 3
        _STATE["runs"] = (np.array([[first[n], LENS[n], g] for n, g in TABLE], np.int64), pos)
    return _STATE["runs"]


def frames(D, f64, pad, grid=False):
    """(x [T, D + pad] with 1e30 in the padding columns, its fp64 values [T, D]) -- once per shape"""
    key = ("x", D, f64, pad, grid)
    if key not in _STATE:
        runs, T = run_table()
        rng = np.random.default_rng(100 * D + 10 * pad + f64)
        if grid:
            v = rng.integers(-64, 65, (T, D)) / 8.0
        else:
            v = rng.normal(rng.uniform(-3, 3, D), rng.uniform(0.5, 2, D), (T, D))
        x = np.full((T, D + pad), 1e30, np.float64 if f64 else np.float32)
        x[:, :D] = v
        _STATE[key] = (x, x[:, :D].astype(np.float64))
    return _STATE[key]


def group_rows(runs, g):
    return np.concatenate([np.arange(b, b + n) for b, n, gg in runs if gg == g] or [np.zeros(0, np.int64)])


# ---- (1) grouped moments ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("f64", [0, 1])
@pytest.mark.parametrize("D", [1, 3, 34, 60, 61])
def test_grouped_moments_against_the_sequential_sum(D, f64, pad):
    import torch
    c = ctx()
    runs, T = run_table()
    x, x64 = frames(D, f64, pad)
    xd = dev(x)[:, :D]
    acc = torch.zeros((NGROUPS, 2 * D + 1), dtype=torch.float64, device="cuda")
    c.frame_moments_groups(xd, runs, NGROUPS, acc)
    a1 = acc.cpu().numpy()
    for g in range(NGROUPS):
        rows = group_rows(runs, g)
        X = x64[rows]
        n = len(rows)
        assert a1[g, 2 * D] == n                                                    # n is exact
        if n == 0:
            assert not a1[g].any()                                                  # the empty group keeps its zeros
            continue
        es, ess = np.abs(a1[g, :D] - seqsum(X)), np.abs(a1[g, D:2 * D] - seqsum(X * X))
        print("D %d f64 %d pad %d group %d n %d: sum err / bound %.3f, sumsq %.3f" % (D, f64, pad, g, n, (es / ((n - 1) * U * np.abs(X).sum(0) + 1e-300)).max(),
                                                                                       (ess / ((n - 1) * U * (X * X).sum(0) + 1e-300)).max()))
        assert (es <= (n - 1) * U * np.abs(X).sum(0)).all() and (ess <= (n - 1) * U * (X * X).sum(0)).all()
    # the same group alone and among others: a bitwise-equal row (host accumulator this time)
    alone = runs[runs[:, 2] == 1].copy()
    alone[:, 2] = 0
    assert np.array_equal(c.frame_moments_groups(xd, alone, 1), a1[1:2])
    # a device table gives the same bits as the host table
    acc_d = torch.zeros_like(acc)
    c.frame_moments_groups(xd, dev(runs), NGROUPS, acc_d)
    assert np.array_equal(acc_d.cpu().numpy(), a1)
    # a second call doubles acc exactly
    c.frame_moments_groups(xd, runs, NGROUPS, acc)
    assert np.array_equal(acc.cpu().numpy(), 2.0 * a1)
    # one group over all frames against gmmiv_frame_moments (two orders: the same bound); runs of any length are allowed
    whole = c.frame_moments_groups(xd, np.array([[0, T, 0]], np.int64), 1)[0]
    fm = c.frame_moments(dev(np.ascontiguousarray(x[:, :D])))
    assert whole[2 * D] == T == fm[2 * D]
    assert (np.abs(whole[:D] - fm[:D]) <= (T - 1) * U * np.abs(x64).sum(0)).all()
    assert (np.abs(whole[D:2 * D] - fm[D:2 * D]) <= (T - 1) * U * (x64 * x64).sum(0)).all()


@pytest.mark.parametrize("f64", [0, 1])
@pytest.mark.parametrize("D", [1, 34, 60, 61])
def test_grouped_moments_of_frames_on_a_grid_are_exact(D, f64):
    """integers / 8: every partial sum is exact in fp64, whatever the order"""
    runs, T = run_table()
    x, x64 = frames(D, f64, 0, grid=True)
    acc = ctx().frame_moments_groups(dev(x), runs, NGROUPS)
    ref = np.zeros_like(acc)
    for g in range(NGROUPS):
        X = x64[group_rows(runs, g)]
        ref[g] = np.concatenate([X.sum(0), (X * X).sum(0), [len(X)]])
    assert np.array_equal(acc, ref)


# ---- (2) stats ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 34, 61])
def test_stats_are_the_four_numpy_operations_on_the_accumulator(D):
    runs, T = run_table()
    x, _ = frames(D, 0, 0)
    c = ctx()
    acc = c.frame_moments_groups(dev(x), runs, NGROUPS)
    mean, std = c.frame_moments_stats(acc, D)
    with np.errstate(all="ignore"):
        n = acc[:, 2 * D:]
        m = acc[:, :D] / n
        s = np.sqrt(acc[:, D:2 * D] / n - m * m)
    assert np.array_equal(mean, m, equal_nan=True) and np.array_equal(std, s, equal_nan=True)
    assert np.isnan(mean[2]).all() and np.isnan(std[2]).all()                       # the empty group
    assert np.isfinite(mean[[0, 1, 3, 4]]).all()
    md, sd = c.frame_moments_stats(dev(acc), D)                                     # device accumulator -> device results, the same bits
    assert np.array_equal(md.cpu().numpy(), m, equal_nan=True) and np.array_equal(sd.cpu().numpy(), s, equal_nan=True)


# ---- (3) apply ----------------------------------------------------------------------------------------------------------------
def apply_ref(x64, runs, mean, std, out_dtype):
    out = {}
    for b, n, g in runs:
        v = x64[b:b + n]
        if mean is not None:
            v = v - mean[g]
        if std is not None:
            v = v / std[g]
        out[(b, n)] = v.astype(out_dtype)
    return out


@pytest.mark.parametrize("which", ["both", "no_mean", "no_std"])
@pytest.mark.parametrize("mode", ["f32_in_place", "f32_to_f64", "f64_to_f32"])
@pytest.mark.parametrize("D,pad", [(60, 0), (34, 0), (34, 3), (61, 3), (3, 1)])
def test_apply_is_one_subtraction_and_one_division(D, pad, mode, which):
    import torch
    from lia_ral_amd import capi
    c = ctx()
    runs, T = run_table()
    f64 = mode == "f64_to_f32"
    x, x64 = frames(D, int(f64), pad)
    rng = np.random.default_rng(D)
    mean = None if which == "no_mean" else rng.normal(0, 2, (NGROUPS, D))
    std = None if which == "no_std" else rng.uniform(0.5, 2, (NGROUPS, D))
    if mean is not None:
        mean[2] = np.nan                                                            # the empty group's rows are used by no frame
    odt = np.float64 if mode == "f32_to_f64" else np.float32
    xd_full = dev(x)
    if mode == "f32_in_place":
        before = x
        od_full = xd_full
    else:
        before = np.full((T, D + pad), -7.0, odt)
        od_full = dev(before)
    c.feat_norm_apply(xd_full[:, :D], runs, mean, std, out=od_full[:, :D], ngroups=NGROUPS)
    got = od_full.cpu().numpy()
    ref = apply_ref(x64, runs, mean, std, odt)
    touched = np.zeros(T, bool)
    for (b, n), v in ref.items():
        assert np.array_equal(got[b:b + n, :D], v), (b, n)
        touched[b:b + n] = True
    assert got[~touched].tobytes() == before[~touched].tobytes()                    # frames outside the runs
    assert got[:, D:].tobytes() == before[:, D:].tobytes()                          # padding columns
    if mode != "f32_in_place":
        assert np.array_equal(xd_full.cpu().numpy(), x)                             # the input is not written
    if mode == "f32_in_place" and which == "both" and pad == 0:
        # a shifted overlap (out = x moved by one row) is refused, like gmmiv_feat_compensate's
        flat = torch.zeros((T + 1) * D, dtype=torch.float32, device="cuda")
        with pytest.raises(capi.GmmivError, match="out overlaps x"):
            c.feat_norm_apply(flat[:T * D].view(T, D), runs, mean, std, out=flat[D:].view(T, D), ngroups=NGROUPS)
        with pytest.raises(capi.GmmivError, match="out overlaps x"):                # the same pointer with another dtype
            c.feat_norm_apply(flat[:T * D].view(T, D), runs, mean, std, out=_alias_f64(flat, T, D), ngroups=NGROUPS)


def _alias_f64(flat, T, D):
    """a float64 matrix [T/2, D] that starts at the first byte of `flat`"""
    import torch
    return flat.view(torch.float64)[:(T // 2) * D].view(T // 2, D)


def test_apply_on_the_energy_column_slice():
    """the recipe's energy pass: column 16 of 34, D = 1, ldx = 34, in place; the other 33 columns keep their bytes"""
    c = ctx()
    runs, T = run_table()
    x, x64 = frames(34, 0, 0)
    xd = dev(x)
    col = xd[:, 16:17]
    acc = c.frame_moments_groups(col, runs, NGROUPS)
    X = x64[:, 16:17]
    for g in (0, 1, 3, 4):
        rows = group_rows(runs, g)
        assert (np.abs(acc[g, 0] - seqsum(X[rows])) <= (len(rows) - 1) * U * np.abs(X[rows]).sum(0)).all() and acc[g, 2] == len(rows)
    mean, std = c.frame_moments_stats(acc, 1)
    c.feat_norm_apply(col, runs, mean, std, out=col)
    got = xd.cpu().numpy()
    ref = x.copy()
    for (b, n), v in apply_ref(X, runs, mean, std, np.float32).items():
        ref[b:b + n, 16:17] = v
    assert got.tobytes() == ref.tobytes()


# ---- (4) KAT-4 end to end -----------------------------------------------------------------------------------------------------
def read_prm(path):
    b = open(path, "rb").read()
    h = struct.unpack("<4I", b[:16])
    return h, np.frombuffer(b[16:], np.float32).reshape(h[2], -1) if h[2] else np.zeros((0, 0), np.float32)


def test_kat4_through_norm_feat_and_norm_feat_files(golden_dir, tmp_path):
    from lia_ral_amd import host_capi as h
    k = np.load(os.path.join(golden_dir, "kat4_normfeat.npz"))
    cluster = [(int(b), int(n)) for b, n in zip(k["seg_begin"], k["seg_len"])]
    rows = np.concatenate([np.arange(b, b + n) for b, n in cluster])
    x = np.ascontiguousarray(k["x"], np.float32)
    out = h.norm_feat(x, [cluster])                                                 # file mode is the default
    diff = np.abs(out[rows].astype(np.float64) - k["x_norm"][rows].astype(np.float64))
    print("KAT-4: median %.3g max %.3g" % (np.median(diff), diff.max()))
    assert np.median(diff) < float(k["median_tol"]) and diff.max() < float(k["max_tol"])
    rest = np.setdiff1d(np.arange(len(x)), rows)
    assert out[rest].tobytes() == x[rest].tobytes()                                 # unselected frames: bit-identical
    # the same through files: the reference's own test1.prm, a label file with two inclusive segments
    src = os.path.join(golden_dir, "ref_files", "test1.prm")
    d = str(tmp_path) + os.sep
    with open(d + "test1.prm", "wb") as f:
        f.write(open(src, "rb").read())
    with open(d + "test1.lbl", "w") as f:
        f.write("0 0.1 speech\n0.3 0.4 speech\n0.45 0.48 other\n")
    hdr, xin = read_prm(src)
    mem = h.norm_feat(xin, [cluster])
    h.norm_feat_files(["test1"], feature_path=d, save_ext=".norm.prm", label_path=d, label="speech")
    hdr_o, got = read_prm(d + "test1.norm.prm")
    assert hdr_o == hdr and got.tobytes() == mem.tobytes()
    h.norm_feat_files(["test1"], feature_path=d, save_ext=".sel.prm", label_path=d, label="speech", write_all_features=False)
    hdr_s, sel = read_prm(d + "test1.sel.prm")
    assert hdr_s[2] == 22 and sel.shape == (22, 34) and sel.tobytes() == mem[rows].tobytes()
    # a non-contiguous mask: two column slices, the masked columns alone are written
    h.norm_feat_files(["test1"], feature_path=d, save_ext=".mask.prm", label_path=d, label="speech", mask="0-15,17-32")
    hdr_m, msk = read_prm(d + "test1.mask.prm")
    cols = list(range(16)) + list(range(17, 33))
    assert msk.shape == (50, 32) and msk.tobytes() == np.ascontiguousarray(mem[:, cols]).tobytes()


# ---- (5) segmental, then file -------------------------------------------------------------------------------------------------
def _pass_ref(x, dx):
    """one NormFeat pass over the frames x [n, D] of one group, sequential fp64; dx >= |library's input - x|.  -> (float32 output,
    bound on |library's float32 output - it|): the sum bounds (n - 1) 2^-53 sum|x| carried through mean, variance, std and
    (|dmean| + |out| |dstd|) / std, one ulp of the float32 output on top"""
    n = len(x)
    ax, e2 = np.abs(x), 2 * np.abs(x) * dx + dx * dx
    s, ss = seqsum(x), seqsum(x * x)
    ds = dx.sum(0) + (n - 1) * U * (ax + dx).sum(0)
    dss = e2.sum(0) + (n - 1) * U * (x * x + e2).sum(0)
    mean = s / n
    dmean = ds / n + U * np.abs(mean)
    var = ss / n - mean * mean
    dvar = dss / n + 2 * np.abs(mean) * dmean + dmean * dmean + 3 * U * (ss / n + mean * mean)
    std = np.sqrt(var)
    dstd = dvar / std + U * std                                                     # |sqrt a - sqrt b| <= |a - b| / sqrt a
    out = (x - mean) / std
    dout = (dx + dmean + np.abs(out) * dstd) / (std - dstd) + 2 * U * np.abs(out)
    o32 = out.astype(np.float32)
    return o32, dout + np.spacing(np.abs(o32)).astype(np.float64)


def test_segmental_then_file_against_the_two_pass_restatement():
    from lia_ral_amd import host_capi as h
    rng = np.random.default_rng(7)
    D = 34
    src_first = [0, 700]
    T = 700 + 5300
    clusters = [[(3, 40), (60, 1 + 64), (300, 257)], [(0, 63), (100, 4500), (4700, 2)]]   # one segment above the 4096-frame cut
    x = rng.normal(rng.uniform(-3, 3, D), rng.uniform(0.5, 2, D), (T, D)).astype(np.float32)
    got = h.norm_feat(x, clusters, src_first=src_first, segmental_mode=True, file_mode=True)
    ref = x.copy()
    err = np.zeros((T, D))
    for s, cl in enumerate(clusters):                                               # pass 1: every segment on its own
        for b, n in cl:
            r = slice(src_first[s] + b, src_first[s] + b + n)
            ref[r], err[r] = _pass_ref(x[r].astype(np.float64), np.zeros((n, D)))
    for s, cl in enumerate(clusters):                                               # pass 2: the source's selected frames together
        rows = np.concatenate([np.arange(src_first[s] + b, src_first[s] + b + n) for b, n in cl])
        ref[rows], err[rows] = _pass_ref(ref[rows].astype(np.float64), err[rows])
    sel = np.zeros(T, bool)
    for s, cl in enumerate(clusters):
        for b, n in cl:
            sel[src_first[s] + b:src_first[s] + b + n] = True
    assert got[~sel].tobytes() == x[~sel].tobytes()
    ok = np.isfinite(ref)                                                           # the 2-frame segment: std of pass 1 may be 0 in a column
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    print("segmental + file: max err %.3g, max err / bound %.3g" % (d[ok].max(), (d[ok] / np.maximum(err[ok], 1e-300)).max()))
    assert np.array_equal(np.isfinite(got), ok)
    assert (d[ok] <= err[ok]).all()
    # segmental mode alone: pass 1 only
    got1 = h.norm_feat(x, clusters, src_first=src_first, segmental_mode=True)
    ref1, err1 = x.copy(), np.zeros((T, D))
    for s, cl in enumerate(clusters):
        for b, n in cl:
            r = slice(src_first[s] + b, src_first[s] + b + n)
            ref1[r], err1[r] = _pass_ref(x[r].astype(np.float64), np.zeros((n, D)))
    assert (np.abs(got1.astype(np.float64) - ref1) <= err1).all()
    # cmsOnly / varOnly on the file pass; both together are refused like NormFeat.cpp:261
    cms = h.norm_feat(x, clusters, src_first=src_first, cms_only=True)
    var = h.norm_feat(x, clusters, src_first=src_first, var_only=True)
    full = h.norm_feat(x, clusters, src_first=src_first)
    for s, cl in enumerate(clusters):
        rows = np.concatenate([np.arange(src_first[s] + b, src_first[s] + b + n) for b, n in cl])
        X = x[rows].astype(np.float64)
        o, e = _pass_ref(X, np.zeros_like(X))
        assert (np.abs(full[rows] - o.astype(np.float64)) <= e).all()
        mean, std = seqsum(X) / len(X), np.sqrt(seqsum(X * X) / len(X) - (seqsum(X) / len(X)) ** 2)
        assert (np.abs(cms[rows] - (X - mean)) <= e * std + np.spacing(np.abs(cms[rows])).astype(np.float64)).all()
        assert (np.abs(var[rows] - X / std) <= e + np.spacing(np.abs(var[rows])).astype(np.float64)).all()
    with pytest.raises(RuntimeError, match="cmsOnly and varOnly"):
        h.norm_feat(x, clusters, src_first=src_first, cms_only=True, var_only=True)


# ---- (6) online mode ----------------------------------------------------------------------------------------------------------
def online_ref(x, W, L):
    """normFeatOnlineMode on one file x [n, D] (fp64), as written: -> (out, c_t, W')"""
    n, D = x.shape
    L = min(L, W)
    Wp = W - L + n if n < L else W
    head = x[:min(L, n)]
    s, ss = seqsum(head), seqsum(head * head)                                       # W' - len(head) zero vectors add nothing
    with np.errstate(all="ignore"):
        m = s / Wp
        c = np.sqrt(ss / Wp - m * m)
        out, ct_ = np.empty_like(x), np.empty_like(x)
        bw = (float(Wp) - 1) / float(Wp)
        for k in range(1, n + 1):
            f = x[k - 1]
            beta = 1.0 if k < L else bw
            m = beta * m + (1 - beta) * f
            c = np.sqrt(c * c * beta + (1 - beta) * (f * f))
            out[k - 1] = (f - m) / c
            ct_[k - 1] = c
    return out, ct_, Wp


def online_data(n, D, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(rng.uniform(-3, 3, D), rng.uniform(0.5, 2, D), (n, D)).astype(np.float32)


def online_check(got, x, W, L, f32_out, tag):
    ref, c_t, Wp = online_ref(x.astype(np.float64), W, L)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), tag                               # 0 / 0 where the reference has it (a window of one frame)
    if not fin.any():
        return
    with np.errstate(all="ignore"):
        bound = Wp * U * (np.abs(x).max(0).astype(np.float64) / c_t + np.abs(ref))
        if f32_out:
            bound = bound + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        d = np.abs(got.astype(np.float64) - ref)
    print("%s: max err / bound %.3f" % (tag, (d[fin] / bound[fin]).max()))
    assert (d[fin] <= bound[fin]).all(), tag


ONLINE = [(1, 300, 300), (50, 300, 200), (299, 300, 300), (300, 300, 300), (301, 300, 300), (777, 300, 100), (5000, 300, 0), (3000, 64, 7),
          (20, 1, 0)]


@pytest.mark.parametrize("D", [1, 34, 60])
@pytest.mark.parametrize("n,W,L", ONLINE)
def test_online_mode_against_the_sequential_loop(n, W, L, D):
    c = ctx()
    x = online_data(n, D, 1000 * D + n + W + L)
    fb = np.array([0, n], np.int64)
    o64 = c.feat_norm_online(dev(x), fb, W, L, out_dtype=1)                         # float32 frames, float64 output
    online_check(o64.cpu().numpy(), x, W, L, False, "n %d W %d L %d D %d f64 out" % (n, W, L, D))
    xd = dev(x)
    c.feat_norm_online(xd, fb, W, L, out=xd)                                        # in place
    online_check(xd.cpu().numpy(), x, W, L, True, "n %d W %d L %d D %d f32 in place" % (n, W, L, D))


@pytest.mark.parametrize("D", [34, 60])
def test_online_mode_on_a_batch_does_not_mix_the_sources(D):
    """an empty source, sources below / at / above the scan's chunk length (1024 frames) and one of several chunks in ONE call: every
    source against the reference, bitwise equal to the same source alone, and the same bits from a device table"""
    c = ctx()
    W, L = 300, 100
    lens = [777, 0, 1024, 1025, 2500, 1, 0]
    fb = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x = online_data(int(fb[-1]), D, 31 + D)
    got = c.feat_norm_online(dev(x), fb, W, L).cpu().numpy()
    got_dev = c.feat_norm_online(dev(x), dev(fb), W, L).cpu().numpy()
    assert got.tobytes() == got_dev.tobytes()
    for f, n in enumerate(lens):
        if n == 0:
            continue
        xs = np.ascontiguousarray(x[fb[f]:fb[f + 1]])
        online_check(got[fb[f]:fb[f + 1]], xs, W, L, True, "batch D %d source %d (n %d)" % (D, f, n))
        alone = c.feat_norm_online(dev(xs), np.array([0, n], np.int64), W, L).cpu().numpy()
        assert alone.tobytes() == got[fb[f]:fb[f + 1]].tobytes(), f
    # the host layer: every source of a FeatureBuffer
    from lia_ral_amd import host_capi as h
    assert h.norm_feat_online(x, src_first=fb[:-1], window_duration=W, init_with_delay=L).tobytes() == got.tobytes()
