"""The batched EnergyDetector on the GPU (include/gmmiv.h: gmmiv_energy_train, gmmiv_energy_select; liagpu::energyDetectorBatch).

The list, its 80-bit results and the bar of every file come from tests/energy_ref.py (the module docstring there derives the bar); the
staging boundary is asked from the library.  Every figure is printed before it is asserted; ENERGY_ERRORS_JSON=<path> also writes the
error-to-bar ratios of test 1 to that file (profiles/rNN/energy_errors.json is such a run)."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import energy_ref as er  # noqa: E402
from test_oracle_kat import energy_select_frames, kat6_normalised  # noqa: E402

pytestmark = pytest.mark.gpu
Q = ("w", "mean", "cov", "threshold")


@pytest.fixture(scope="module")
def ctx():
    import torch
    from lia_ral_amd import capi
    c = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref():
    from lia_ral_amd import capi
    return er.reference(capi.energy_stage_frames(capi.F32), capi.energy_stage_frames(capi.F64))


_RUN = {}


def run_group(ctx, g):
    """one train + count + fill on the group's buffer, once per group -> energy_detect's dict (host arrays)"""
    import torch
    if g["name"] not in _RUN:
        xd = torch.from_numpy(g["buf"].copy()).cuda()
        col = xd[:, g["col"]:g["col"] + 1]
        _RUN[g["name"]] = ctx.energy_detect(col, g["runs"], len(g["files"]), C=g["C"], nb_train_it=g["nb_it"], variance_flooring=er.FLOORING,
                                            variance_ceiling=er.CEILING, alpha=g["alpha"])
    return _RUN[g["name"]]


def split(model, C):
    return dict(w=model[:C], mean=model[C:2 * C], cov=model[2 * C:3 * C])


def file_out(r, f, C):
    d = split(r["model"][f], C)
    d["threshold"] = r["threshold"][f]
    return d


def segs_of(r, f):
    a, b = int(r["seg_off"][f]), int(r["seg_off"][f + 1])
    return [(int(x), int(y)) for x, y in zip(r["seg_begin"][a:b], r["seg_len"][a:b])]


# ---- (1) every file against the 80-bit chain ---------------------------------------------------------------------------------------
def test_every_file_within_its_bar_of_the_80_bit_chain(ctx, ref):
    rows, worst = [], 0.0
    failures = []
    for g in ref:
        r = run_group(ctx, g)
        column = g["buf"][:, g["col"]]
        for f, fr in enumerate(g["ref"]):
            rat = er.ratios(file_out(r, f, g["C"]), fr["r80"], fr["bar"])
            b, l = er.file_runs(g["runs"], f)
            want = energy_select_frames(column, float(fr["r80"]["threshold"]), b, l)
            above = int(sum(int(np.sum(column[int(bb):int(bb) + int(ll)] > float(fr["r80"]["threshold"]))) for bb, ll in zip(b, l)))
            rows.append(dict(group=g["name"], file=f, n=len(fr["x"]), C=g["C"], nb_train_it=g["nb_it"], dtype=np.dtype(g["dtype"]).name, ratios=rat))
            print("%s[%d] n=%d: err / bar w %.3g mean %.3g cov %.3g threshold %.3g; %d segments" % (g["name"], f, len(fr["x"]), rat["w"], rat["mean"], rat["cov"],
                                                                                                   rat["threshold"], len(want)))
            worst = max(worst, max(rat.values()))
            if max(rat.values()) > 1.0:
                failures.append((g["name"], f, len(fr["x"]), rat))
            assert int(r["status"][f]) == fr["r80"]["status"], (g["name"], f, int(r["status"][f]), fr["r80"]["status"])
            assert segs_of(r, f) == want, (g["name"], f)
            assert int(r["n_above"][f]) == above, (g["name"], f)
    print("largest error / bar over %d files: %.3g" % (len(rows), worst))
    if os.environ.get("ENERGY_ERRORS_JSON"):
        with open(os.environ["ENERGY_ERRORS_JSON"], "w") as fo:
            json.dump(dict(what="gmmiv_energy_train against tests/energy_ref.py: |device - 80-bit| / bar per file and output", worst=worst, files=rows), fo, indent=1)
    assert not failures, failures


# ---- (2) selectFrames on the device against the rule, on the device's own threshold -----------------------------------------------------
def test_device_segments_equal_select_frames_on_the_devices_own_threshold(ctx, ref):
    for g in ref:
        r = run_group(ctx, g)
        column = g["buf"][:, g["col"]]
        for f in range(len(g["files"])):
            b, l = er.file_runs(g["runs"], f)
            assert segs_of(r, f) == energy_select_frames(column, float(r["threshold"][f]), b, l), (g["name"], f)


PATTERNS = {
    # name: (column values, input segments (begin, length), threshold)
    "all in": ([1, 2, 3, 4, 5, 6], [(0, 6)], 0.5),
    "none in": ([1, 2, 3, 4, 5, 6], [(0, 6)], 6.0),
    "alternating": ([1, 0] * 300 + [1], [(0, 601)], 0.5),
    "alternating, out first": ([0, 1] * 300, [(0, 600)], 0.5),
    "a run reaches the segment's end": ([0, 0, 1, 1, 1, 9, 9, 0, 1, 1], [(0, 5), (7, 3)], 0.5),
    "a single frame in at a segment's end": ([0, 0, 0, 1, 0, 0, 1], [(0, 4), (4, 3)], 0.5),
    "a run stopped by the segment boundary": ([1, 1, 1, 1, 1, 1], [(0, 3), (3, 3)], 0.5),
    "a value equal to the threshold": ([0.5, 0.75, 0.5, 0.75, 0.75, 0.5], [(0, 6)], 0.5),
    "equal to the threshold everywhere": ([0.5] * 7, [(0, 7)], 0.5),
    "NaN out, +Inf in": ([np.nan, np.inf, 1e30, -np.inf, np.nan, 2.0], [(0, 6)], 1.0),
    "a NaN threshold": ([1, 2, 3], [(0, 3)], np.nan),
    "segments in another order than the buffer": ([1, 1, 0, 0, 1, 1, 0, 1], [(4, 4), (0, 3)], 0.5),
    "longer than a workgroup pass": ([1] * 255 + [0] + [1] * 300 + [0, 0] + [1] * 513, [(0, 700), (700, 371)], 0.5),
}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_select_patterns_count_and_fill_agree(ctx, dtype):
    import torch
    names = list(PATTERNS)
    cols, runs, th, t0 = [], [], [], 0
    for f, k in enumerate(names):
        v, segs, t = PATTERNS[k]
        cols.append(np.asarray(v, dtype))
        runs += [(t0 + b, n, f) for b, n in segs]
        th.append(t)
        t0 += len(v)
    col = np.concatenate(cols)
    runs = np.array(runs, np.int64)
    xd = torch.from_numpy(col.reshape(-1, 1).copy()).cuda()
    above, cnt = ctx.energy_select(xd, runs, len(names), np.array(th))
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    sb, sl = np.full(int(off[-1]), -1, np.int64), np.full(int(off[-1]), -1, np.int64)
    above2, cnt2, sb, sl = ctx.energy_select(xd, runs, len(names), np.array(th), seg_off=off, seg_begin=sb, seg_len=sl)
    assert np.array_equal(above, above2) and np.array_equal(cnt, cnt2)
    for f, k in enumerate(names):
        b, l = er.file_runs(runs, f)
        want = energy_select_frames(col, th[f], b, l)
        got = [(int(x), int(y)) for x, y in zip(sb[off[f]:off[f + 1]], sl[off[f]:off[f + 1]])]
        print("%-45s %s" % (k, got[:4]))
        assert got == want and int(cnt[f]) == len(want), k
        assert int(above[f]) == int(sum(np.sum(col[int(bb):int(bb) + int(ll)] > th[f]) for bb, ll in zip(b, l))), k
    worst = PATTERNS["alternating"]
    assert int(cnt[names.index("alternating")]) == len(worst[0]) // 2 + 1          # the worst case: one segment per two frames + one per input segment
    # room for fewer segments than there are: the surplus is not written
    short = off.copy(); short[1:] = np.minimum(short[1:], 1)
    sb2, sl2 = np.full(2, -1, np.int64), np.full(2, -1, np.int64)
    ctx.energy_select(xd, runs, len(names), np.array(th), seg_off=short, seg_begin=sb2, seg_len=sl2)
    assert (int(sb2[0]), int(sl2[0])) == (0, 7) and sb2[1] == -1 and sl2[1] == -1


# ---- (3) a file's bits do not depend on its place or its neighbours ------------------------------------------------------------------
def _train_bits(ctx, files, C, nb_it, alpha, dtype=np.float32):
    import torch
    runs, t0 = [], 3
    for f, x in enumerate(files):
        if len(x):
            runs.append((t0, len(x), f))
        t0 += len(x) + 2
    col = np.full(t0, 0.125, dtype)
    for (b, n, f) in runs:
        col[b:b + n] = files[f]
    xd = torch.from_numpy(col.reshape(-1, 1)).cuda()
    model, th, st = ctx.energy_train(xd, np.array(runs, np.int64).reshape(-1, 3), len(files), C=C, nb_train_it=nb_it, alpha=alpha)
    return [(model[f].tobytes(), th[f].tobytes(), int(st[f])) for f in range(len(files))]


def test_independence_of_position_and_neighbours(ctx, ref):
    a = ref[0]
    from lia_ral_amd import capi
    picks = [1, 3, 9, 10, 12, 13]                                   # 3, 64, 1000, 5000 frames, the boundary and one past it
    xs = {f: a["ref"][f]["x"] for f in picks}
    other = [er.energy_like(n, 900 + n) for n in (7, 700, capi.energy_stage_frames(capi.F32) + 5, 0)]
    kw = dict(C=a["C"], nb_it=a["nb_it"], alpha=a["alpha"])
    alone = {f: _train_bits(ctx, [xs[f]], **kw)[0] for f in picks}
    together = _train_bits(ctx, [xs[f] for f in picks], **kw)
    mixed_files = [other[2], xs[13], other[3], xs[12], other[0], xs[10], xs[9], other[1], xs[3], xs[1]]
    mixed = _train_bits(ctx, mixed_files, **kw)
    where = {13: 1, 12: 3, 10: 5, 9: 6, 3: 8, 1: 9}
    r = run_group(ctx, a)
    for i, f in enumerate(picks):
        in_list = (r["model"][f].tobytes(), r["threshold"][f].tobytes(), int(r["status"][f]))
        assert alone[f] == together[i] == mixed[where[f]] == in_list, f


# ---- (4) against the per-file path ------------------------------------------------------------------------------------------------
def test_batch_equals_the_per_file_path(ref):
    from lia_ral_amd import host_capi as h
    a = ref[0]
    picks = [2, 3, 4, 5, 7, 9, 10]                                   # 63, 64, 0, 65, 256, 1000, 5000 frames
    energies, segs = [], []
    for f in picks:
        x = a["ref"][f]["x"]
        lens = er.split_runs(len(x), a["files"][f][2], 77 + f)
        gap = 3
        col = np.full(len(x) + gap * len(lens) + 1, -5.0, np.float32)       # the input segments are not adjacent in the file
        b, o = [], 0
        for i, ln in enumerate(lens):
            b.append(o + gap * (i + 1)); col[b[-1]:b[-1] + ln] = x[o:o + ln]; o += ln
        energies.append(col); segs.append((np.array(b), np.array(lens)))
    kw = dict(C=a["C"], nb_train_it=a["nb_it"], variance_flooring=er.FLOORING, variance_ceiling=er.CEILING, alpha=a["alpha"])
    got = h.energy_detector_batch(energies, segs, **kw)
    for i, f in enumerate(picks):
        fr = a["ref"][f]
        if len(fr["x"]) == 0:
            assert got[i]["status"] == er.EMPTY and len(got[i]["begin"]) == 0 and np.isnan(got[i]["threshold"])
            continue
        one = h.energy_detector(energies[i], segs[i][0], segs[i][1], **kw)
        assert list(got[i]["begin"]) == list(one["begin"]) and list(got[i]["length"]) == list(one["length"]), f
        d = abs(got[i]["threshold"] - one["threshold"])
        print("file %d (n = %d): |batch - per-file threshold| = %.3g, the sum of both bars %.3g" % (f, len(fr["x"]), d, 2 * fr["bar"]["threshold"]))
        assert d <= 2 * float(fr["bar"]["threshold"]), f
        assert er.ratios(dict(w=got[i]["w"], mean=got[i]["mean"], cov=got[i]["cov"], threshold=got[i]["threshold"]), fr["r80"], fr["bar"])["threshold"] <= 1.0


# ---- (5) KAT-6 -----------------------------------------------------------------------------------------------------------------------
def test_kat6_inside_a_batch_and_through_files(ref, golden_dir, tmp_path):
    import struct
    from lia_ral_amd import host_capi as h
    k = np.load(os.path.join(golden_dir, "kat6_energydetector_assumed.npz"))
    e = kat6_normalised(k)
    kw = dict(C=len(k["init_w"]), nb_train_it=int(k["nb_train_it"]), variance_flooring=float(k["variance_flooring"]), variance_ceiling=float(k["variance_ceiling"]),
              alpha=float(k["alpha"]))
    nb = [er.energy_like(300, 5), er.energy_like(40, 6)]
    got = h.energy_detector_batch([nb[0], e, nb[1]], [([0], [300]), (k["seg_begin"], k["seg_len"]), ([2, 20], [10, 20])], **kw)
    assert [(int(b), int(n)) for b, n in zip(got[1]["begin"], got[1]["length"])] == [tuple(int(v) for v in k["expected_seg"])]
    # through files: the normalised column as a one-column .prm, the golden's input label segments
    d = str(tmp_path) + os.sep
    for name, col in (("n0", nb[0]), ("test1", e), ("n1", nb[1])):
        wide = np.full((len(col), 3), 1e30, np.float32); wide[:, 1] = col
        with open(d + name + ".prm", "wb") as fo:
            fo.write(struct.pack("<4I", 2, 3, len(col), 0)); fo.write(wide.tobytes())
    with open(d + "n0.lbl", "w") as fo:
        fo.write("0 2.99 speech\n")
    with open(d + "n1.lbl", "w") as fo:
        fo.write("0.02 0.11 speech\n0.2 0.39 speech\n")
    with open(d + "test1.lbl", "w") as fo:
        for b, n in zip(k["seg_begin"], k["seg_len"]):
            fo.write("%g %g speech\n" % (int(b) * 0.01, (int(b) + int(n) - 1) * 0.01))
    th, st = h.energy_detector_files(["n0", "test1", "n1"], feature_path=d, label_path=d, save_path=d, save_ext=".enr.lbl", mask="1", **kw)
    assert open(d + "test1.enr.lbl").read().split("\n")[0] == str(k["expected_label"])
    assert open(d + "test1.enr.lbl").read().count("\n") == 1
    assert th[1] == got[1]["threshold"] and th[0] == got[0]["threshold"] and list(st) == [g["status"] for g in got]
    want0 = ["%g %g speech" % (int(b) * 0.01, (int(b) + int(n) - 1) * 0.01) for b, n in zip(got[0]["begin"], got[0]["length"])]
    assert open(d + "n0.enr.lbl").read().split("\n")[:-1] == want0


# ---- (6) degenerate inputs -----------------------------------------------------------------------------------------------------------
def degenerate_files():
    base = er.energy_like(500, 71)
    bad = base.copy(); bad[[3, 77, 250, 499]] = [np.nan, np.inf, -np.inf, 1e30]
    far = (er.energy_like(200, 72) * np.float32(0.01) + np.float32(60.0)).astype(np.float32)   # every logit of iteration 1 below -745: (60 - 2)^2 / 2 = 1682
    return [("neighbour before", er.energy_like(300, 73)), ("NaN, Inf, -Inf and 1e30 inside", bad), ("a constant file", np.full(100, 0.75, np.float32)),
            ("neighbour between", er.energy_like(1000, 74)), ("one frame", np.array([0.5], np.float32)),
            ("every frame a zero-likelihood frame in iteration 1", far), ("neighbour after", er.energy_like(64, 75))]


def test_degenerate_inputs_follow_the_documented_rules(ctx):
    import torch
    files = degenerate_files()
    C, nb_it, alpha = 3, 10, 0.25
    runs, t0 = [], 0
    for f, (_, x) in enumerate(files):
        runs.append((t0, len(x), f)); t0 += len(x)
    col = np.concatenate([x for _, x in files])
    runs = np.array(runs, np.int64)
    xd = torch.from_numpy(col.reshape(-1, 1).copy()).cuda()
    r = ctx.energy_detect(xd, runs, len(files), C=C, nb_train_it=nb_it, alpha=alpha)
    torch.cuda.synchronize()
    for f, (name, x) in enumerate(files):
        r80 = er.chain(x, C, nb_it, alpha)
        bar = er.bars(x, C, nb_it, alpha, r80, degenerate=True)
        rat = er.ratios(file_out(r, f, C), r80, bar)
        print("%-52s status %d (80-bit %d) threshold %r: err / bar %s" % (name, int(r["status"][f]), r80["status"], float(r["threshold"][f]), {q: "%.3g" % rat[q] for q in Q}))
        assert int(r["status"][f]) == r80["status"], name
        assert max(rat.values()) <= 1.0, (name, rat)
        b, l = er.file_runs(runs, f)
        assert segs_of(r, f) == energy_select_frames(col, float(r["threshold"][f]), b, l), name
    st = {name: int(r["status"][f]) for f, (name, _) in enumerate(files)}
    assert st["a constant file"] & er.NONFINITE and st["one frame"] & er.NONFINITE          # globalCov = 0: every variance floored to 0
    assert st["every frame a zero-likelihood frame in iteration 1"] & er.NONFINITE         # count = 0: weights 0 / 0
    assert not st["NaN, Inf, -Inf and 1e30 inside"] & (er.FLOORED | er.CEILED)             # globalCov is NaN: no comparison holds
    # the neighbours keep the bits they have alone
    for name, x in files:
        if name.startswith("neighbour"):
            f = [n for n, _ in files].index(name)
            assert _train_bits(ctx, [x], C, nb_it, alpha)[0] == (r["model"][f].tobytes(), r["threshold"][f].tobytes(), int(r["status"][f])), name


# ---- (7) device pointers throughout: both calls only enqueue ------------------------------------------------------------------------
def test_device_pointers_only_enqueue(ref):
    import time
    import torch
    from lia_ral_amd import capi
    g = ref[0]
    nf = len(g["files"])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = capi.Context(0, s.cuda_stream)
        xd = torch.from_numpy(g["buf"].copy()).cuda()
        runs = torch.from_numpy(g["runs"].copy()).cuda()
        model = torch.zeros((nf, 3 * g["C"]), dtype=torch.float64, device="cuda"); th = torch.zeros(nf, dtype=torch.float64, device="cuda")
        st = torch.zeros(nf, dtype=torch.int32, device="cuda")
        above = torch.zeros(nf, dtype=torch.int64, device="cuda"); cnt = torch.zeros(nf, dtype=torch.int64, device="cuda")
        kw = dict(C=g["C"], nb_train_it=g["nb_it"], variance_flooring=er.FLOORING, variance_ceiling=er.CEILING, alpha=g["alpha"])
        c.energy_train(xd, runs, nf, model=model, threshold=th, status=st, **kw)
        c.energy_select(xd, runs, nf, th, n_above=above, seg_count=cnt)
        torch.cuda.synchronize()                                      # warm-up: workspaces, the LDS attribute
        off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(cnt, 0)])
        sb = torch.zeros(int(off[-1]), dtype=torch.int64, device="cuda"); sl = torch.zeros_like(sb)
        model.zero_(); th.zero_()
        torch.cuda._sleep(int(2.0e9))                                 # ~1 s of spinning on this stream
        t0 = time.perf_counter()
        c.energy_train(xd, runs, nf, model=model, threshold=th, status=st, **kw)
        c.energy_select(xd, runs, nf, th, n_above=above, seg_count=cnt)
        c.energy_select(xd, runs, nf, th, seg_off=off, seg_begin=sb, seg_len=sl, n_above=above, seg_count=cnt)
        dt = time.perf_counter() - t0
        still_busy = not s.query()
        torch.cuda.synchronize()
        assert still_busy and dt < 0.25, (still_busy, dt)
        # the device table gives the bits of the host table (table order, the whole staging budget: neither changes a sum)
        hc = capi.Context(0, s.cuda_stream)
        hm, ht, hs = hc.energy_train(xd, g["runs"], nf, **kw)
        torch.cuda.synchronize()
        assert model.cpu().numpy().tobytes() == hm.tobytes() and th.cpu().numpy().tobytes() == ht.tobytes() and np.array_equal(st.cpu().numpy(), hs)
        det = hc.energy_detect(xd, g["runs"], nf, **kw)
        assert np.array_equal(sb.cpu().numpy(), det["seg_begin"]) and np.array_equal(sl.cpu().numpy(), det["seg_len"])
        hc.close(); c.close()
