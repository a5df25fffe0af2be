"""Batched ComputeTest on the GPU: gmmiv_llr_trials (the trial kernel, its fallbacks, the chunking) against the oracle, against the
per-frame entry points bit for bit, against the composition it replaces, and the host layer (computeTestBatch, compute_test_ndx).

Tolerances: per-frame values of these kernels agree with the oracle to 1e-9 absolute (test_gpu_gmm.py), so do means of them; an LLR is
the difference of two.  Two summation orders of the same n values of magnitude <= L differ by at most 2 n 2^-53 L in the mean.

These thresholds see neither the order of the sums nor an error below 1e-9: tests/test_gpu_trials_elementwise.py holds the results
to the bits of the documented summation order and judges every trial, segment and frame against long double under its own bar.
"""
import ctypes as ct
import os
import struct

import numpy as np
import pytest

import models_ref as mr
import trials_ref as tr
from conftest import make_frames, make_gmm

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def ctx():
    from lia_ral_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


_cache = {}


def case(ctx, C, D, dtype=np.float32, per_model=False, layout="piece"):
    """world handle, batch, frames and segment layout of a shape -- built once per module"""
    from lia_ral_amd import capi
    key = (C, D, np.dtype(dtype).name, per_model, layout)
    if key not in _cache:
        world = make_gmm(C, D, seed=C + D)
        models = tr.make_models(world, per_model)
        sb, T = tr.piece_layout(capi.TRIAL_PIECE) if layout == "piece" else (mr.seg_layout()[0], mr.seg_layout()[2])
        x = make_frames(*world, T, seed=T + D, dtype=dtype)
        batch = ctx.gmm_batch(tr.N_MODELS, C, D).load(*models)
        _cache[key] = dict(world=world, models=models, sb=sb, T=T, x=x, g=ctx.gmm(*world), batch=batch, ref={})
    return _cache[key]


def frame_ref(cs, ctop, complete, lo=-200.0, hi=200.0):
    key = (ctop, complete, lo, hi)
    if key not in cs["ref"]:
        cs["ref"][key] = tr.frame_ref(cs["world"], cs["models"], cs["x"], ctop, complete, lo, hi)
    return cs["ref"][key]


SHAPES = [(128, 60, 1), (128, 60, 10), (128, 60, 16), (37, 14, 1), (37, 14, 10), (37, 14, 16), (2, 2, 1), (2, 2, 2),
          (33, 13, 10),     # odd vectSize: the any-shape path
          (128, 60, 17)]    # topDistribsCount > 16: the any-shape path


@pytest.mark.parametrize("C,D,ctop", SHAPES)
@pytest.mark.parametrize("complete", [True, False])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_against_oracle(ctx, C, D, ctop, complete, dtype):
    for per_model in (False, True):
        for layout in ("piece", "models"):
            cs = case(ctx, C, D, dtype, per_model, layout)
            ts, tm = tr.trial_list(len(cs["sb"]) - 1, skip=3)
            llr, cm, wm = cs["batch"].llr_trials(cs["g"], cs["x"], cs["sb"], ts, tm, ctop, complete)
            rl, rc, rw = tr.ref_llr(*frame_ref(cs, ctop, complete), cs["sb"], ts, tm)
            e = (np.max(np.abs(cm - rc)), np.max(np.abs(wm - rw)), np.max(np.abs(llr - rl)))
            print("C %d D %d ctop %d complete %d per_model %d %s: client %.2e world %.2e llr %.2e" % (C, D, ctop, complete, per_model, layout, *e))
            assert e[0] < 1e-9 and e[1] < 1e-9 and e[2] < 2e-9
            assert np.array_equal(llr, cm - wm[ts])


@pytest.mark.parametrize("C,D,ctop", [(128, 60, 10), (37, 14, 16), (2, 2, 2), (33, 13, 10), (128, 60, 17)])
@pytest.mark.parametrize("complete", [True, False])
@pytest.mark.parametrize("per_model", [False, True])
def test_per_frame_bits(ctx, C, D, ctop, complete, per_model):
    """one-frame segments: every sum has one term, so the means ARE the per-frame values of the single-model entry points"""
    cs = case(ctx, C, D, np.float32, per_model)
    T = 70
    x = cs["x"][:T]
    sb = np.arange(T + 1)
    ts = np.tile(np.arange(T, dtype=np.int32), tr.N_MODELS)
    tm = np.repeat(np.arange(tr.N_MODELS, dtype=np.int32), T)
    llr, cm, wm = cs["batch"].llr_trials(cs["g"], x, sb, ts, tm, ctop, complete)
    d = cs["g"].llk_determine_top(x, ctop, complete)
    assert np.array_equal(wm, d["llk"])
    for g in range(tr.N_MODELS):
        one = ctx.gmm(*tr.model_of(cs["models"], g))
        assert np.array_equal(cm[g * T:(g + 1) * T], one.llk_use_top(x, d["idx"], d["nontop_llk"], complete)), g
        one.close()
    assert np.array_equal(llr, cm - wm[ts])


@pytest.mark.parametrize("C,D,ctop", [(128, 60, 10), (37, 14, 16), (33, 13, 10), (128, 60, 17)])
@pytest.mark.parametrize("layout", ["piece", "models"])
def test_against_the_composition(ctx, C, D, ctop, layout):
    """determine_top + llk_use_top_multi + segment_means on the same frames: the same per-frame values in another summation order"""
    import torch
    from lia_ral_amd import capi
    cs = case(ctx, C, D, np.float32, False, layout)
    sb = cs["sb"]
    ts, tm = tr.trial_list(len(sb) - 1)
    llr, cm, wm = cs["batch"].llr_trials(cs["g"], cs["x"], sb, ts, tm, ctop, True, -200.0, 200.0)
    d = cs["g"].llk_determine_top(cs["x"], ctop, True, -200.0, 200.0)
    clients = [ctx.gmm(*tr.model_of(cs["models"], g)) for g in range(tr.N_MODELS)]
    rows = capi.Gmm.llk_use_top_multi(clients, cs["x"], d["idx"], d["nontop_llk"], True, -200.0, 200.0)
    means = ctx.segment_means(torch.from_numpy(np.vstack([d["llk"][None], rows])).cuda(), sb)       # [1 + G, nseg]
    for c in clients:
        c.close()
    n = (sb[1:] - sb[:-1]).astype(float)
    bound = 2 * n * U * 200.0
    assert np.all(np.abs(wm - means[0]) <= bound)
    assert np.all(np.abs(cm - means[1 + tm, ts]) <= bound[ts])
    assert np.all(np.abs(llr - (means[1 + tm, ts] - means[0, ts])) <= 2 * bound[ts])


@pytest.mark.parametrize("C,D,ctop", [(128, 60, 10), (33, 13, 10)])
def test_independence(ctx, C, D, ctop):
    """a trial's result depends on its segment's frames and its model only"""
    import torch
    cs = case(ctx, C, D)
    sb, x, g, b = cs["sb"], cs["x"], cs["g"], cs["batch"]
    ts, tm = tr.trial_list(len(sb) - 1, skip=3)                  # segment 3 has no trial
    base = b.llr_trials(g, x, sb, ts, tm, ctop)
    same = lambda r, sel=slice(None): all(np.array_equal(p[sel] if i < 2 else p, q) for i, (p, q) in enumerate(zip(base, r)))
    assert same(b.llr_trials(g, x, sb, ts, tm, ctop))            # two consecutive calls
    perm = np.random.default_rng(5).permutation(len(ts))         # the list shuffled
    assert same(b.llr_trials(g, x, sb, ts[perm], tm[perm], ctop), perm)
    for i in range(len(ts)):                                     # each trial alone
        assert same(b.llr_trials(g, x, sb, ts[i:i + 1], tm[i:i + 1], ctop), slice(i, i + 1)), i
    dup = np.concatenate([np.arange(len(ts)), [2, 2]])           # a duplicated trial
    assert same(b.llr_trials(g, x, sb, ts[dup], tm[dup], ctop), dup)
    full_ts = np.concatenate([ts, [3]]).astype(np.int32); full_tm = np.concatenate([tm, [1]]).astype(np.int32)
    r = b.llr_trials(g, x, sb, full_ts, full_tm, ctop)           # with a trial for the segment that had none
    assert all(np.array_equal(p, q[:len(ts)]) for p, q in zip(base[:2], r[:2])) and np.array_equal(base[2], r[2])
    xd = torch.from_numpy(x).cuda()                              # device tensors for x and the outputs
    o = [torch.full((len(ts),), 7.0, dtype=torch.float64, device="cuda") for _ in range(2)] + [torch.full((len(sb) - 1,), 7.0, dtype=torch.float64, device="cuda")]
    torch.cuda.synchronize()                                     # the fills ran on torch's stream, the call runs on the context's
    b.llr_trials(g, xd, sb, ts, tm, ctop, llr=o[0], client_mean=o[1], world_mean=o[2])
    ctx.sync()                                                   # device outputs: the call only enqueues on the context's stream
    assert same([t.cpu().numpy() for t in o])
    prev = ctx.set_option("trials_scratch_mb", 0)                # every segment a chunk of its own
    try:
        assert same(b.llr_trials(g, x, sb, ts, tm, ctop))
    finally:
        ctx.set_option("trials_scratch_mb", prev)
    ctx.set_option("glds", 0)
    try:
        assert same(b.llr_trials(g, x, sb, ts, tm, ctop))
    finally:
        ctx.set_option("glds", 1)


def test_edges(ctx):
    cs = case(ctx, 128, 60)
    sb, x, g, b = cs["sb"], cs["x"], cs["g"], cs["batch"]
    lw, lc = frame_ref(cs, 10, True)
    # an empty segment gives zeros
    llr, cm, wm = b.llr_trials(g, x, sb, [0, 0, 1], [1, 4, 1], 10)
    assert sb[1] == sb[0] and llr[0] == 0 and cm[1] == 0 and wm[0] == 0 and llr[2] != 0
    # no trial: llr is not touched, world_mean is filled
    keep = np.full(3, 7.0)
    _, _, wm0 = b.llr_trials(g, x, sb, [], [], 10, llr=keep, client_mean=keep.copy())
    assert np.all(keep == 7.0) and np.max(np.abs(wm0 - tr.ref_llr(lw, lc, sb, [], [])[2])) < 1e-9
    # no segment, no frame
    assert len(b.llr_trials(g, x[:0], [0], [], [], 10)[2]) == 0
    llr, cm, wm = b.llr_trials(g, x[:0], [0, 0], [0], [2], 10)
    assert llr[0] == 0 and cm[0] == 0 and wm[0] == 0
    # a NaN frame and a frame 50 sigma away inside the longest segment: both passes give min_llk there, the frames count in n_s
    s = len(sb) - 2
    bad = [int(sb[s]) + 5, int(sb[s]) + 200]
    xb = x.copy()
    xb[bad[0], 7] = np.nan
    xb[bad[1]] = (cs["world"][1][0] + 50.0 / np.sqrt(cs["world"][2][0])).astype(np.float32)
    llr, cm, wm = b.llr_trials(g, xb, sb, [s, s], [0, 3], 10, True, -150.0, 200.0)
    lw2, lc2 = tr.frame_ref(cs["world"], cs["models"], x, 10, True, -150.0, 200.0)
    n = int(sb[s + 1] - sb[s])
    rest = np.setdiff1d(np.arange(sb[s], sb[s + 1]), bad)
    assert abs(wm[s] - (lw2[rest].sum() + 2 * -150.0) / n) < 1e-9
    for i, m in enumerate([0, 3]):
        assert abs(cm[i] - (lc2[m][rest].sum() + 2 * -150.0) / n) < 1e-9
    assert np.max(np.abs(llr - (cm - wm[s]))) == 0


def test_argument_errors(ctx):
    import torch
    from lia_ral_amd import capi
    cs = case(ctx, 128, 60)
    sb, x, g, b = cs["sb"], cs["x"], cs["g"], cs["batch"]
    other = ctx.gmm_batch(2, 64, 60).load(*[a[:64] for a in cs["world"]])
    with pytest.raises(capi.GmmivError, match="the world model is 128 x 60"):
        other.llr_trials(g, x, sb, [1], [0], 10)
    other.close()
    for ctop in (0, 65, 129):
        with pytest.raises(capi.GmmivError, match="topDistribsCount"):
            b.llr_trials(g, x, sb, [1], [0], ctop)
    small = case(ctx, 2, 2)
    with pytest.raises(capi.GmmivError, match="topDistribsCount"):
        small["batch"].llr_trials(small["g"], small["x"], small["sb"], [1], [0], 3)       # more than the model has
    for ts, tm, what in [([len(sb) - 1], [0], "trial_seg"), ([-1], [0], "trial_seg"), ([1], [tr.N_MODELS], "trial_model"), ([1], [-1], "trial_model")]:
        with pytest.raises(capi.GmmivError, match=what):
            b.llr_trials(g, x, sb, ts, tm, 10)
    with pytest.raises(capi.GmmivError, match="non-decreasing"):
        b.llr_trials(g, x, [0, 10, 5], [0], [0], 10)
    with pytest.raises(capi.GmmivError, match="out of range"):
        b.llr_trials(g, x, [0, len(x) + 1], [0], [0], 10)
    # a table on the device
    dsb = torch.from_numpy(np.asarray(sb)).cuda()
    hts = np.array([1], np.int32); htm = np.array([0], np.int32)
    dts = torch.from_numpy(hts).cuda()
    out = np.empty(1)
    p = lambda a: ct.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else ct.c_void_p(a.ctypes.data)
    for tabs in [(dsb, hts, htm), (np.asarray(sb), dts, htm), (np.asarray(sb), hts, dts)]:
        rc = capi.lib.gmmiv_llr_trials(ctx._h, g._h, b._h, p(x), capi.F32, ct.c_int64(len(x)), ct.c_int64(x.shape[1]), p(tabs[0]), ct.c_int64(len(sb) - 1),
                                       p(tabs[1]), p(tabs[2]), ct.c_int64(1), 10, capi.TOP_COMPLETE, ct.c_double(-200.0), ct.c_double(200.0), p(out), None, None)
        assert rc != 0 and b"host arrays" in capi.lib.gmmiv_last_error()


def test_kat1_through_the_batch(ctx, golden_dir):
    """ComputeTest golden LLRs (test1.validate.res): the two labelled segments against [test1, wld]"""
    k = np.load(os.path.join(golden_dir, "kat1_computetest.npz"))
    world = ctx.gmm(k["w"], k["mean_world"], k["covinv"])
    C, D = k["mean_world"].shape
    batch = ctx.gmm_batch(2, C, D).load(np.stack([k["w_client"], k["w"]]), np.stack([k["mean_client"], k["mean_world"]]),
                                        np.stack([k["covinv_client"], k["covinv"]]))
    b0, b1 = (int(v) for v in k["seg_begin"]); n0, n1 = (int(v) for v in k["seg_len"])
    assert b0 + n0 <= b1
    sb = [b0, b0 + n0, b1, b1 + n1]                              # the gap between the two is a segment nobody asks for
    llr, _, _ = batch.llr_trials(world, k["x"], sb, [0, 0, 2, 2], [0, 1, 0, 1], int(k["top_c"]), True, float(k["min_llk"]), float(k["max_llk"]))
    assert np.allclose(llr[[0, 2]], k["expected_llr"], atol=float(k["abs_tol"]), rtol=0), llr
    assert np.all(np.abs(llr[[1, 3]]) < 1e-12)
    batch.close(); world.close()


def _host_lines():
    C, D = 64, 20
    world = make_gmm(C, D, seed=21)
    models = tr.make_models(world, False, seed=22)
    x = make_frames(*world, 900, seed=23)
    hm = lambda m: (m[0], m[1], 1.0 / m[2])                      # the host layer takes variances
    seg_begin = [[0, 150], [300, 460], [600, 700]]
    seg_len = [[140, 131], [128, 100], [1, 190]]
    clients = [[0, 3], [4, 1, 2], [3]]
    return x, seg_begin, seg_len, hm(world), [hm(tr.model_of(models, g)) for g in range(tr.N_MODELS)], clients


@pytest.mark.parametrize("segmental", [True, False])
def test_host_batch_equals_the_loop(segmental):
    from lia_ral_amd import host_capi as h
    x, sbeg, slen, world, models, clients = _host_lines()
    got = h.compute_test_batch(x, sbeg, slen, world, models, clients, segmental=segmental)
    ref = h.compute_test_batch(x, sbeg, slen, world, models, clients, segmental=segmental, loop=True)
    for l in range(3):
        one = h.compute_test(x, sbeg[l], slen[l], world, [models[g] for g in clients[l]], segmental=segmental)
        assert np.array_equal(ref[l], one)                       # the loop is computeTestLLR line by line
        n = np.array(slen[l], float) if segmental else np.array([float(sum(slen[l]))])
        assert got[l].shape == ref[l].shape == (len(n), len(clients[l]))
        assert np.all(np.abs(got[l] - ref[l]) <= (4 * n * U * 200.0)[:, None]), (l, got[l] - ref[l])
    # one client with another Gaussian count: the per-line loop itself
    small = tuple(a[:48] for a in models[1])
    small = (small[0] / small[0].sum(), small[1], small[2])
    mixed = models[:1] + [small] + models[2:]
    a = h.compute_test_batch(x, sbeg, slen, world, mixed, clients, segmental=segmental)
    b = h.compute_test_batch(x, sbeg, slen, world, mixed, clients, segmental=segmental, loop=True)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))


def test_ndx_reproduces_the_lines_of_compute_test_files(tmp_path, golden_dir):
    """a two-line ndx on the golden test1.prm / label file, two clients with real scores (KAT-1's test1 model and a second model with
    its means moved): every result line must be the text compute_test_files writes, and every LLR must lie within the summation-order
    bound of compute_test_files' LLR (4 n_s 2^-53 L for a difference of two means of n_s values of magnitude <= L = 200)"""
    from lia_ral_amd import host_capi as h
    ref = os.path.join(golden_dir, "ref_files")
    k = np.load(os.path.join(golden_dir, "kat1_computetest.npz"))

    def write_raw(path, w, mean, covinv):
        C, D = mean.shape
        with open(path, "wb") as f:
            f.write(struct.pack("<II", C, D)); f.write(w.astype("<f8").tobytes())
            for c in range(C):
                det = float(np.prod(1.0 / covinv[c])); cst = (2 * np.pi) ** (-D / 2) / np.sqrt(det)
                f.write(struct.pack("<ddB", cst, det, 0)); f.write(covinv[c].astype("<f8").tobytes()); f.write(mean[c].astype("<f8").tobytes())

    mdir = str(tmp_path) + os.sep
    write_raw(mdir + "wld.gmm", k["w"], k["mean_world"], k["covinv"])
    write_raw(mdir + "spk1.gmm", k["w_client"], k["mean_client"], k["covinv_client"])
    moved = k["mean_client"] + np.random.default_rng(31).normal(0.0, 0.2, k["mean_client"].shape) / np.sqrt(k["covinv_client"])
    write_raw(mdir + "spk2.gmm", k["w_client"], moved, k["covinv_client"])
    ndx = str(tmp_path / "trials.ndx")
    with open(ndx, "w") as f:
        f.write("test1 spk1 spk2\n\ntest1 spk2\n")
    args = dict(mask="0-15,17-32", label="male", top_c=10, complete=True, gender="M")
    llr, lines = h.compute_test_ndx(mdir + "wld.gmm", ndx, mdir, ref + os.sep, os.path.join(ref, "computetest_"), **args)
    want, want_llr = [], []
    for names in (["spk1", "spk2"], ["spk2"]):
        l, ls = h.compute_test_files(mdir + "wld.gmm", [mdir + n + ".gmm" for n in names], names, os.path.join(ref, "test1.prm"),
                                     os.path.join(ref, "computetest_test1.lbl"), test_name="test1", **args)
        want += ls
        want_llr += l.ravel().tolist()
    print("\n".join("%s | %s" % p for p in zip(lines, want)))
    assert len(lines) == 6 and len(llr) == 6
    assert lines == want
    n = np.array([k["seg_len"][0]] * 2 + [k["seg_len"][1]] * 2 + list(k["seg_len"]), float)      # [segment][client] per line
    print("LLR(ndx) - LLR(files):", llr - np.array(want_llr))
    assert np.all(np.abs(llr - np.array(want_llr)) <= 4 * n * U * 200.0)
    assert np.all(np.abs(llr) > 0.1)                             # real scores, not rounding noise
    assert np.allclose(llr[[0, 2]], k["expected_llr"], atol=float(k["abs_tol"]), rtol=0)
    assert llr[1] == llr[4] and llr[3] == llr[5]                 # the same (file, segment, model) trial on both lines
