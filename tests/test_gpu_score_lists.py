"""Score normalisation on lists (include/gmmiv.h, "score normalisation on lists") on the device.

The contract needs no tolerance: the (mean, std) of a distribution of a list are the bits gmmiv_score_cohort_stats (axis 0) returns
for a one-row matrix of the same values -- whatever the distribution's neighbours, the table order, pos or the alignment of its
first slot.  Against the numpy restatement of the reference (tests/score_lists_ref.py) integer scores are exact and real scores
stay within the bound derived in tests/test_gpu_score_norm.py, restated for lists in score_lists_ref: no new constant.

One list serves most tests: distributions of the lengths LENS in shuffled order (neighbours differ in class), about 10^5 scores.
LENS holds the smallest shapes at which the kernels can go wrong: the candidate cut-off 64, every thread-count step of the select
launcher (512, 1024, 2048, 4096 scores), the wave / workgroup step of the streaming pass (4096), the LDS staging limit 16384 on both
sides, and a distribution that is re-read per pass (40000).  At 1, 2, 3 and 8 scores discardH or discardL truncates to 0."""
import numpy as np
import pytest

import score_lists_ref as sr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

LENS = [1, 2, 3, 8, 63, 64, 65, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 16384, 16385, 40000]
MODES = [(0, 0.0, 0.0), (0, 0.1, 0.05), (1, 0.0, 0.0), (1, 0.25, 0.25)]
NPRE = 37


def same(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def same_value(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module")
def ctx():
    import torch
    from lia_ral_amd import capi
    c = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


class Lists:
    """the shared list: values per distribution, pre ids per slot, and the dense call's answer per (mode, pre)"""

    def __init__(self, ctx):
        rng = np.random.default_rng(1805)
        self.lens = np.array(LENS)[rng.permutation(len(LENS))]
        self.vals = [rng.normal(-2.0, 1.5, n) for n in self.lens]
        self.pre_id = [rng.integers(0, NPRE, n).astype(np.int32) for n in self.lens]
        self.pre_mean, self.pre_std = rng.normal(-2.0, 0.3, NPRE), rng.uniform(0.5, 2.0, NPRE)
        self.dense = {}
        for mode, pH, pL in MODES:
            for pre in (False, True):
                res = [ctx.score_cohort_stats(v[None, :], 0, pre_mean=self.pre_mean[i] if pre else None,
                                              pre_std=self.pre_std[i] if pre else None, mean_mode=mode, percent_h=pH, percent_l=pL)
                       for v, i in zip(self.vals, self.pre_id)]
                self.dense[(mode, pH, pL, pre)] = (np.array([r[0][0] for r in res]), np.array([r[1][0] for r in res]))

    def table(self, off0):
        off = np.concatenate([[off0], off0 + np.cumsum(self.lens)]).astype(np.int64)
        scores = np.concatenate([np.full(off0, np.nan)] + self.vals)       # slots before off[0]: never read
        pre_id = np.concatenate([np.full(off0, -1, np.int32)] + self.pre_id)
        return off, scores, pre_id


@pytest.fixture(scope="module")
def lists(ctx):
    return Lists(ctx)


# ---- 1. bitwise against the dense call ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off0", [4, 7])            # an even and an odd first slot: the 16-byte and the 8-byte loads of the streaming pass
def test_bitwise_against_the_dense_call(ctx, lists, off0):
    rng = np.random.default_rng(off0)
    off, scores, pre_id = lists.table(off0)
    total = len(scores)
    perm = rng.permutation(total).astype(np.int64)  # pos: slot k holds shuffled[perm[k]]
    shuffled = np.empty(total)
    shuffled[perm] = scores
    for mode, pH, pL in MODES:
        for pre in (False, True):
            kw = dict(mean_mode=mode, percent_h=pH, percent_l=pL)
            if pre:
                kw.update(pre_id=pre_id, pre_mean=lists.pre_mean, pre_std=lists.pre_std)
            want = lists.dense[(mode, pH, pL, pre)]
            m, s = ctx.score_list_stats(off, scores, **kw)
            assert same(m, want[0]) and same(s, want[1]), ("in place", off0, mode, pH, pL, pre, np.flatnonzero(m != want[0]), lists.lens)
            m, s = ctx.score_list_stats(off, shuffled, pos=perm, **kw)
            assert same(m, want[0]) and same(s, want[1]), ("pos", off0, mode, pH, pL, pre, np.flatnonzero(m != want[0]), lists.lens)


def test_device_arrays_give_the_bits_of_host_arrays(ctx, lists):
    import torch
    off, scores, pre_id = lists.table(3)
    d = lambda a: torch.from_numpy(a).cuda()
    sc, pid, pm, ps = d(scores), d(pre_id), d(lists.pre_mean), d(lists.pre_std)
    pos = d(np.arange(len(scores), dtype=np.int64))
    for mode, pH, pL in MODES:
        m = torch.empty(len(LENS), dtype=torch.float64, device="cuda"); s = torch.empty_like(m)
        ctx.score_list_stats(off, sc, pos=pos, pre_id=pid, pre_mean=pm, pre_std=ps, mean_mode=mode, percent_h=pH, percent_l=pL, out_mean=m, out_std=s)
        torch.cuda.synchronize()
        want = lists.dense[(mode, pH, pL, True)]
        assert same(m.cpu().numpy(), want[0]) and same(s.cpu().numpy(), want[1]), (mode, pH, pL)


# ---- 2. exact against the reference ---------------------------------------------------------------------------------------------
def test_integer_scores_are_exact(ctx):
    rng = np.random.default_rng(77)
    lens = np.array(LENS)[rng.permutation(len(LENS))]
    vals = [rng.integers(-3, 4, n).astype(np.float64) for n in lens]       # small integers, negative values, long runs of ties
    vals.append(np.full(300, 7.0)); vals.append(np.full(5000, -3.0))        # constant distributions
    off = np.concatenate([[0], np.cumsum([len(v) for v in vals])])
    for mode, pH, pL in MODES:
        m, s = ctx.score_list_stats(off, np.concatenate(vals), mean_mode=mode, percent_h=pH, percent_l=pL)
        ref = [sr.ref_mean_std(v, mode, pH, pL) for v in vals]
        assert same_value(m, [r[0] for r in ref]) and same_value(s, [r[1] for r in ref]), (mode, pH, pL)
        if (pH, pL) != (0.0, 0.0):                                         # ties across both thresholds in the long distributions
            v = np.sort(vals[int(np.argmax(lens))])[::-1]
            dH, dL = int(len(v) * pH), int(len(v) * pL)
            assert v[dH - 1] == v[dH] and v[len(v) - dL - 1] == v[len(v) - dL]


def test_key_mapping_on_zeros_denormals_and_huge_values(ctx):
    rng = np.random.default_rng(11)
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 1e300, -1e300, 1e300, -1e300, 2.2250738585072014e-308])
    vals = []
    for L in (64, 1000, 20000, 65, 513):
        r = np.concatenate([special, rng.integers(-50, 51, L - len(special)).astype(np.float64)])
        rng.shuffle(r)
        vals.append(r)
    off = np.concatenate([[0], np.cumsum([len(v) for v in vals])])
    x = np.concatenate(vals)
    for mode, pH, pL in MODES:
        m, s = ctx.score_list_stats(off, x, mean_mode=mode, percent_h=pH, percent_l=pL)
        for d, v in enumerate(vals):
            rm, rs, kept = sr.ref_mean_std(v, mode, pH, pL)
            if mode == 1:
                assert same_value(m[d], rm), (d, pH, pL, m[d], rm)         # the selected order statistic / the score at n / 2
            if (pH, pL) != (0.0, 0.0):                                     # both discards remove the two +-1e300
                assert int(len(v) * pH) >= 2 and int(len(v) * pL) >= 2
                bm, bs = sr.bounds(rm, rs, kept, mode)
                assert abs(m[d] - rm) <= bm and abs(s[d] - rs) <= bs, (d, mode, m[d], rm, bm, s[d], rs, bs)


# ---- 3. real-valued scores within the derived bound -----------------------------------------------------------------------------
def test_real_scores_within_the_derived_bound(ctx, lists):
    off, scores, pre_id = lists.table(0)
    for mode, pH, pL in MODES:
        for pre in (False, True):
            kw = dict(pre_id=pre_id, pre_mean=lists.pre_mean, pre_std=lists.pre_std) if pre else {}
            m, s = ctx.score_list_stats(off, scores, mean_mode=mode, percent_h=pH, percent_l=pL, **kw)
            for d, (v, pid) in enumerate(zip(lists.vals, lists.pre_id)):
                if pre:
                    v = (v - lists.pre_mean[pid]) / lists.pre_std[pid]      # the same two IEEE operations
                rm, rs, kept = sr.ref_mean_std(v, mode, pH, pL)
                bm, bs = sr.bounds(rm, rs, kept, mode)
                if mode == 1:
                    assert same_value(m[d], rm), (d, mode, pH, pL, pre)    # selection is exact
                em, es = abs(m[d] - rm), abs(s[d] - rs)
                assert em <= bm and es <= bs, (len(v), mode, pH, pL, pre, em, bm, es, bs)


# ---- 4. a distribution's result depends on nothing but the distribution ---------------------------------------------------------
def test_independence_of_neighbours_table_order_and_grouping(ctx, lists):
    off, scores, _ = lists.table(2)
    nd = len(LENS)
    # the table reversed: distribution j of the second list is distribution nd - 1 - j of the first, through pos
    rlens = lists.lens[::-1]
    roff = np.concatenate([[0], np.cumsum(rlens)]).astype(np.int64)
    rpos = np.concatenate([np.arange(off[nd - 1 - j], off[nd - j]) for j in range(nd)]).astype(np.int64)
    for mode, pH, pL in MODES:
        kw = dict(mean_mode=mode, percent_h=pH, percent_l=pL)
        m, s = ctx.score_list_stats(off, scores, **kw)
        m2, s2 = ctx.score_list_stats(off, scores, **kw)
        assert same(m, m2) and same(s, s2), ("repeat", mode, pH, pL)
        mr, sr_ = ctx.score_list_stats(roff, scores, pos=rpos, **kw)
        assert same(mr[::-1], m) and same(sr_[::-1], s), ("reversed", mode, pH, pL)
        for d in range(nd):
            m1, s1 = ctx.score_list_stats(off[d:d + 2], scores, **kw)      # alone: ndist = 1, its own off
            assert same(m1, m[d:d + 1]) and same(s1, s[d:d + 1]), ("alone", lists.lens[d], mode, pH, pL)


# ---- 5. the list normalisation is exact -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 100003])
def test_normalize_list_is_exact(ctx, n):
    import torch
    rng = np.random.default_rng(n)
    R, C = 5, 11
    x = rng.normal(-2.0, 1.5, n)
    rid, cid = rng.integers(0, R, n).astype(np.int32), rng.integers(0, C, n).astype(np.int32)      # ids with repeats
    rm, cm = rng.normal(-2.0, 0.5, R), rng.normal(-2.0, 0.5, C)
    rs, cs = rng.uniform(0.3, 3.0, R), rng.uniform(0.3, 3.0, C)
    cs[C // 3] = 0.0                                                        # a constant cohort: Inf / NaN in the same places
    with np.errstate(invalid="ignore", divide="ignore"):
        z = lambda v: (v - rm[rid]) / rs[rid]
        t = lambda v: (v - cm[cid]) / cs[cid]
        refs = {0: (z(x), None), 1: (t(x), None), 2: (z(t(x)), t(x)), 3: (t(z(x)), z(x))}
    d = lambda a: torch.from_numpy(a).cuda()
    for order in range(4):
        ref, ref_first = refs[order]
        got, first = x.copy(), np.full(n, 99.0)
        out = ctx.score_normalize_list(got, order, rid, rm, rs, cid, cm, cs, first_out=first)
        assert out is got and same_value(got, ref), (n, order)              # in place
        assert same_value(first, ref_first) if order >= 2 else np.all(first == 99.0)
        need_r, need_c = order != 1, order != 0                             # only what the order needs
        got2 = ctx.score_normalize_list(x.copy(), order, rid if need_r else None, rm if need_r else None, rs if need_r else None,
                                        cid if need_c else None, cm if need_c else None, cs if need_c else None)
        assert same_value(got2, ref)
        xd, fd = d(x), torch.full((n,), 99.0, dtype=torch.float64, device="cuda")
        ctx.score_normalize_list(xd, order, d(rid), d(rm), d(rs), d(cid), d(cm), d(cs), first_out=fd)
        torch.cuda.synchronize()
        assert same(xd.cpu().numpy(), got) and same(fd.cpu().numpy(), first), (n, order)


# ---- 6. errors enqueue nothing --------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_untouched(ctx):
    import torch
    from lia_ral_amd import capi
    sc = torch.arange(10, dtype=torch.float64, device="cuda")
    m = torch.full((3,), 99.0, dtype=torch.float64, device="cuda"); s = torch.full_like(m, 99.0)
    with pytest.raises(capi.GmmivError, match="distribution 1 has 0 scores"):
        ctx.score_list_stats([0, 4, 4, 10], sc, out_mean=m, out_std=s)
    with pytest.raises(capi.GmmivError, match="distribution 1: empty kept range, 2 scores"):
        ctx.score_list_stats([0, 5, 7, 10], sc, percent_h=0.5, percent_l=0.5, out_mean=m, out_std=s)
    pid = np.zeros(10, np.int32); pid[9] = 2
    with pytest.raises(capi.GmmivError, match=r"distribution 2: pre_id\[9\] = 2 outside \[0, 2\)"):
        ctx.score_list_stats([0, 5, 7, 10], sc, pre_id=pid, pre_mean=np.zeros(2), pre_std=np.ones(2), out_mean=m, out_std=s)
    pos = np.arange(10); pos[0] = 10
    with pytest.raises(capi.GmmivError, match=r"distribution 0: pos\[0\] = 10 outside \[0, 10\)"):
        ctx.score_list_stats([0, 5, 7, 10], sc, pos=pos, out_mean=m, out_std=s)
    x = torch.full((4,), 99.0, dtype=torch.float64, device="cuda")
    with pytest.raises(capi.GmmivError, match=r"row_id\[3\] = 5"):
        ctx.score_normalize_list(x, capi.NORM_Z, np.array([0, 1, 1, 5], np.int32), np.zeros(2), np.ones(2))
    torch.cuda.synchronize()
    assert bool((m == 99.0).all()) and bool((s == 99.0).all()) and bool((x == 99.0).all())
    m0, s0 = ctx.score_list_stats([3], sc)                                  # no distribution: a no-op
    assert len(m0) == 0 and len(s0) == 0
    assert len(ctx.score_normalize_list(np.zeros(0), capi.NORM_Z, np.zeros(0, np.int32), np.zeros(1), np.ones(1))) == 0


# ---- 7. the four chains end to end through the host layer, from files to files --------------------------------------------------
def _write(path, lines):
    with open(path, "w") as f:
        f.write("".join("%s %s 0 %s %.17g\n" % l for l in lines))
    return str(path)


def _parse(path):
    out = []
    for line in open(path):
        g, name, dec, seg, sc = line.split()
        assert dec == "0"
        out.append((g, name, seg, float(sc)))
    return out


def _e2e_lists(rng, ragged):
    M, S, Nz, Nt = 7, 9, 11, 5
    ms, ss = ["m%d" % i for i in range(M)], ["s%d" % i for i in range(S)]
    imps, cs = ["i%d" % i for i in range(Nz)], ["c%d" % i for i in range(Nt)]
    pairs = [(m, s) for m in ms for s in ss]
    if ragged:                                                              # 40 % of the pairs, every model and segment at least once
        keep = set(rng.choice(len(pairs), int(0.4 * len(pairs)), replace=False).tolist())
        keep |= {i * S + (i % S) for i in range(M)} | {(j % M) * S + j for j in range(S)}
        pairs = [pairs[i] for i in sorted(keep)]
        rng.shuffle(pairs)
    sc = lambda: float(rng.normal(-1.0, 2.0))
    test = [("F" if i % 3 == 0 else "M", m, s, sc()) for i, (m, s) in enumerate(pairs)]

    def cohort(rows, cols, drop, twice):
        l = [("M", r, c, sc()) for r in rows for c in cols if (r, c) not in drop]
        if ragged:
            l.append(("M", twice[0], twice[1], sc()))                       # a pair listed twice is two scores
            rng.shuffle(l)
        return l
    drop = lambda rows, cols: {(rows[1], cols[2]), (rows[3], cols[5 % len(cols)])} if ragged else set()
    zl = cohort(ms, imps, drop(ms, imps), (ms[0], imps[1]))                 # two models lack different impostor segments
    tl = cohort(cs, ss, drop(cs, ss), (cs[2], ss[4]))
    ztl = cohort(cs, imps, drop(cs, imps), (cs[4], imps[7]))
    ids = imps[:3] + imps[4:10] + cs[:2] + cs[3:]                           # 9 of 11 impostor segments, 4 of 5 cohort models
    return test, zl, tl, ztl, ids


@pytest.mark.parametrize("use_ids", [False, True])
def test_chains_end_to_end_from_files_to_files(tmp_path, use_ids):
    import os
    from lia_ral_amd import host_capi
    rng = np.random.default_rng(31)
    test, zl, tl, ztl, ids = _e2e_lists(rng, ragged=True)
    f = {k: _write(tmp_path / (k + ".nist"), v) for k, v in (("test", test), ("z", zl), ("t", tl), ("zt", ztl))}
    idf = None
    if use_ids:
        idf = str(tmp_path / "ids.lst")
        open(idf, "w").write("\n".join(ids) + "\n")
    with pytest.raises(host_capi.HostError, match="not a full cross product"):      # what the dense driver makes of these lists
        host_capi.compute_norm_files(f["test"], str(tmp_path / "dense"), "ztnorm", znorm_nist_file=f["z"], tnorm_nist_file=f["t"],
                                     ztnorm_nist_file=f["zt"])
    exts = {"znorm": (".znorm", None), "tnorm": (".tnorm", None), "ztnorm": (".ztnorm", ".tnorm"), "tznorm": (".tznorm", ".znorm")}
    for nt in ("znorm", "tnorm", "ztnorm", "tznorm"):
        for mode, pH, pL in ((0, 0.0, 0.0), (1, 0.2, 0.1)):
            base = str(tmp_path / ("out_%s_%d" % (nt, mode)))
            host_capi.compute_norm_list_files(f["test"], base, nt, znorm_nist_file=f["z"], tnorm_nist_file=f["t"], ztnorm_nist_file=f["zt"],
                                              impostor_id_list=idf, mean_mode=mode, percent_h=pH, percent_l=pL)
            ref = sr.chain_ref(test, zl, tl, ztl, nt, mode, pH, pL, set(ids) if use_ids else None)
            got = _parse(base + exts[nt][0])
            assert [g[:3] for g in got] == [t[:3] for t in test]            # test-list order
            for g, r in zip(got, ref):
                assert abs(g[3] - r[0]) <= r[1], (nt, mode, use_ids, g, r)
            if exts[nt][1]:
                first = _parse(base + exts[nt][1])                          # both files of the two-stage types
                assert [g[:3] for g in first] == [t[:3] for t in test]
                for g, r in zip(first, ref):
                    assert abs(g[3] - r[2]) <= r[3], (nt, mode, use_ids, "first", g, r)
            else:
                assert not any(os.path.exists(base + e) for e in (".znorm", ".tnorm", ".ztnorm", ".tznorm") if e != exts[nt][0])


def test_on_a_cross_product_the_list_driver_agrees_with_the_dense_driver(tmp_path):
    from lia_ral_amd import host_capi
    rng = np.random.default_rng(32)
    test, zl, tl, ztl, _ = _e2e_lists(rng, ragged=False)
    f = {k: _write(tmp_path / (k + ".nist"), v) for k, v in (("test", test), ("z", zl), ("t", tl), ("zt", ztl))}
    exts = {"znorm": (".znorm",), "tnorm": (".tnorm",), "ztnorm": (".ztnorm", ".tnorm"), "tznorm": (".tznorm", ".znorm")}
    for nt in ("znorm", "tnorm", "ztnorm", "tznorm"):
        for mode, pH, pL in ((0, 0.0, 0.0), (1, 0.2, 0.1)):
            kw = dict(znorm_nist_file=f["z"], tnorm_nist_file=f["t"], ztnorm_nist_file=f["zt"], mean_mode=mode, percent_h=pH, percent_l=pL)
            host_capi.compute_norm_list_files(f["test"], str(tmp_path / "list"), nt, **kw)
            host_capi.compute_norm_files(f["test"], str(tmp_path / "dense"), nt, **kw)
            ref = sr.chain_ref(test, zl, tl, ztl, nt, mode, pH, pL)
            for k, e in enumerate(exts[nt]):
                a, b = _parse(str(tmp_path / "list") + e), _parse(str(tmp_path / "dense") + e)
                assert [g[:3] for g in a] == [g[:3] for g in b] == [t[:3] for t in test]
                for ga, gb, r in zip(a, b, ref):
                    y, by = (r[0], r[1]) if k == 0 else (r[2], r[3])
                    assert abs(ga[3] - y) <= by and abs(gb[3] - y) <= by, (nt, mode, e, ga, gb, r)


# ---- 8. no growth -----------------------------------------------------------------------------------------------------------------
def test_scratch_is_the_formula_and_does_not_grow():
    import torch
    from lia_ral_amd import capi
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    nd, n = 20000, 100
    sc = torch.randn(nd * n, dtype=torch.float64, device="cuda")
    off = np.arange(nd + 1, dtype=np.int64) * n
    pos = torch.arange(nd * n, dtype=torch.int64, device="cuda")
    pid = torch.zeros(nd * n, dtype=torch.int32, device="cuda")
    pre = (torch.zeros(4, dtype=torch.float64, device="cuda"), torch.ones(4, dtype=torch.float64, device="cuda"))
    m = torch.empty(nd, dtype=torch.float64, device="cuda"); s = torch.empty_like(m)

    def run():
        ctx.score_list_stats(off, sc, out_mean=m, out_std=s)
        ctx.score_list_stats(off, sc, pos=pos, pre_id=pid, pre_mean=pre[0], pre_std=pre[1], mean_mode=1, percent_h=0.05, percent_l=0.2,
                             out_mean=m, out_std=s)
        ctx.score_normalize_list(sc[:nd], capi.NORM_Z, pid[:nd], pre[0], pre[1])
    run()
    torch.cuda.synchronize()
    ws = [ctx.workspace_bytes(i) for i in range(64)]
    formula = capi.list_scratch_bytes(nd)                                   # GMMIV_SCORE_LIST_SCRATCH_BYTES(nd) = 12 nd + 8
    assert sum(ws) == ctx.workspace_bytes() and formula <= ctx.workspace_bytes() <= formula + formula // 8, (ws, formula)
    run()
    torch.cuda.synchronize()
    assert ws == [ctx.workspace_bytes(i) for i in range(64)]                # the second call allocated nothing
    ctx.close()
