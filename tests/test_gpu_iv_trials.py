"""The i-vector scoring rules on a list of trials (include/gmmiv_iv_trials.h: gmmiv_score_cosine_trials / _mahalanobis_trials /
_twocov_trials / _plda_trials on k_score_trials), judged TRIAL BY TRIAL against the long-double scores and the bars of
tests/backend_ref.py, never by array:
  every trial of every list            |got - ref[m, s]| <= bar[m, s]
  against the dense rule's cell        |list - dense[m, s]| <= 2 bar[m, s]   (both lie within one bar of the same reference)
  bit for bit (array_equal)            the shuffled list, every other list, a trial scored alone, the duplicated list, both anchor
                                       sides, pieces of 4 and the default, host arrays against device tensors
dims: a row of one pair, a tail lane, exactly 64 pairs, one more, more than two passes; counts up to 34 x 130.  Then: the argument
checks that need a device pointer, a history case (a used context gives the bits of a fresh one and allocates nothing on a repeated
call), the resident chain into gmmiv_score_list_stats / gmmiv_score_normalize_list, and the host layer (ivTestTrials, enrollMean, the
ndx tool)."""
import contextlib

import numpy as np
import pytest

import backend_ref as br
import iv_trials_ref as ir
import score_lists_ref as sr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300), pytest.mark.skipif(not br.HAVE_LONGDOUBLE, reason=br.SKIP_MESSAGE)]

SENTINEL = -1.2345678e300


@pytest.fixture(scope="module")
def ctx():
    from lia_ral_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def options(ctx, opts):
    """set, run, restore: both options of the list calls default to 0"""
    try:
        for k, v in opts.items():
            assert ctx.set_option(k, v) == 0, k
        yield
    finally:
        for k, v in opts.items():
            assert ctx.set_option(k, 0) == v, k


def dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def run_dense(ctx, rule, p, which="FTJF"):
    if rule == "cosine":
        return ctx.score_cosine(p["m"], p["s"])
    if rule == "mahalanobis":
        return ctx.score_mahalanobis(p["m"], p["s"], p["Mah"])
    if rule == "twocov":
        return ctx.score_twocov(p["m"], p["s"], p["G"], p["H"])
    return ctx.score_plda(p["msum"], p["nsess"], p["s"], p[which])


def run_list(ctx, rule, p, tm, ts, m=None, s=None, out=None, which="FTJF"):
    """one list call; m, s: None (the case's host arrays) or device tensors; out: None (a host array pre-filled with a sentinel)"""
    if m is None:
        m, s = (p["msum"] if rule == "plda" else p["m"]), p["s"]
    if out is None:
        out = np.full(len(tm), SENTINEL)
    if rule == "cosine":
        return ctx.score_cosine_trials(m, s, tm, ts, out=out)
    if rule == "mahalanobis":
        return ctx.score_mahalanobis_trials(m, s, p["Mah"], tm, ts, out=out)
    if rule == "twocov":
        return ctx.score_twocov_trials(m, s, p["G"], p["H"], tm, ts, out=out)
    return ctx.score_plda_trials(m, p["nsess"], s, p[which], tm, ts, out=out)


class Failures:
    def __init__(self):
        self.bad = []

    def judge(self, what, got, key, rule, tm, ts, which="FTJF", scale=1.0, against=None):
        """per trial: |got_i - against_i| <= scale bar[m_i, s_i]; against: None = the long-double reference"""
        ref, bar = ir.reference(key, rule, which)
        want = ref[tm, ts] if against is None else br.ld(against)
        got = np.asarray(got, np.float64)
        r = np.where(np.isfinite(got), np.abs(br.ld(got) - want) / (scale * bar[tm, ts]), np.inf)
        print("%-60s worst ratio %.3f of %g bar over %d trials" % (what, float(r.max()), scale, len(tm)))
        if not np.all(r <= 1):
            i = int(np.argmax(r))
            self.bad.append("%s: trial %d = (model %d, segment %d): %.3g of the bar; %d of %d trials miss"
                            % (what, i, tm[i], ts[i], float(r[i]), int(np.sum(~(r <= 1))), len(tm)))

    def same_bits(self, what, got, want):
        got, want = np.asarray(got), np.asarray(want)
        if not np.array_equal(got, want):
            i = int(np.flatnonzero(got != want)[0])
            self.bad.append("%s: trial %d differs: %r against %r (%d of %d differ)" % (what, i, got[i], want[i], int(np.sum(got != want)), len(want)))

    def finish(self):
        assert not self.bad, "\n".join(self.bad)


def check_rule(ctx, f, key, rule, which="FTJF", tag=""):
    """every list of one case and rule: accuracy per trial, the dense cell, and the bit invariances"""
    import torch
    p = br.score_case(*key)
    M, S = p["M"], p["S"]
    name = "%s dim %d %dx%d%s " % (rule, key[0], M, S, tag)
    dense = run_dense(ctx, rule, p, which)
    tm, ts = ir.trial_list("full shuffled", M, S)
    base = run_list(ctx, rule, p, tm, ts, which=which)
    f.judge(name + "full shuffled", base, key, rule, tm, ts, which)
    f.judge(name + "full shuffled against the dense cell", base, key, rule, tm, ts, which, scale=2.0, against=dense[tm, ts])
    cell = np.full((M, S), np.nan)
    cell[tm, ts] = base                                                 # the bits of every pair
    for kind in ir.LISTS[1:]:
        lm, ls = ir.trial_list(kind, M, S)
        with options(ctx, {"iv_trials_piece": 4} if kind == "one model" else {}):
            got = run_list(ctx, rule, p, lm, ls, which=which)
        f.judge(name + kind, got, key, rule, lm, ls, which)
        f.judge(name + kind + " against the dense cell", got, key, rule, lm, ls, which, scale=2.0, against=dense[lm, ls])
        f.same_bits(name + kind + " against the shuffled list", got, cell[lm, ls])
    for opts in ({"iv_trials_anchor": 1}, {"iv_trials_anchor": 2}, {"iv_trials_piece": 4}, {"iv_trials_anchor": 2, "iv_trials_piece": 4}):
        with options(ctx, opts):
            f.same_bits(name + str(opts), run_list(ctx, rule, p, tm, ts, which=which), base)
    alone = range(len(tm)) if len(tm) <= 21 else np.random.default_rng(5).choice(len(tm), 6, replace=False)
    for i in alone:
        f.same_bits(name + "trial %d alone" % i, run_list(ctx, rule, p, tm[i:i + 1], ts[i:i + 1], which=which), base[i:i + 1])
    md, sd = dev(p["msum"] if rule == "plda" else p["m"]), dev(p["s"])
    buf = torch.full((len(tm) + 16,), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    run_list(ctx, rule, p, tm, ts, m=md, s=sd, out=buf[8:8 + len(tm)], which=which)
    ctx.sync()
    back = buf.cpu().numpy()
    f.same_bits(name + "device tensors", back[8:8 + len(tm)], base)
    assert np.all(back[:8] == SENTINEL) and np.all(back[8 + len(tm):] == SENTINEL), name + "wrote outside scores[ntrial]"


@pytest.mark.parametrize("dim,M,S", ir.cases(), ids=lambda v: str(v))
def test_list_rules_per_trial_and_bit_invariance(ctx, dim, M, S):
    f = Failures()
    for rule in ir.LIST_RULES:
        check_rule(ctx, f, ir.case_key(dim, M, S, rule), rule)
    f.finish()


@pytest.mark.parametrize("kind", ir.PLDA_KINDS)
@pytest.mark.parametrize("dim", (5, 40, 129))
def test_plda_session_patterns(ctx, dim, kind):
    """classes by the DISTINCT session count: runs, all distinct, an odd run at an odd index -- and a second FTJF on the same context"""
    f = Failures()
    key = (dim, len(br.PLDA_COUNTS[kind]), 7, "plda " + kind)
    check_rule(ctx, f, key, "plda", "FTJF", " " + kind)
    check_rule(ctx, f, key, "plda", "FTJF2", " " + kind + " second model")
    f.finish()


def test_checks_that_need_a_device_pointer(ctx):
    import torch
    from lia_ral_amd import capi
    p = br.score_case(5, 3, 7, "plain")
    tm, ts = ir.trial_list("full", 3, 7)
    out = np.full(len(tm), SENTINEL)
    for a, b in ((dev(tm), ts), (tm, dev(ts))):
        with pytest.raises(capi.GmmivError, match="trial_model and trial_seg must be host arrays"):
            ctx.score_cosine_trials(p["m"], p["s"], a, b, out=out)
    import ctypes as ct
    ns = dev(p["nsess"])
    rc = capi.lib.gmmiv_score_plda_trials(ctx._h, 5, ct.c_int64(3), ct.c_int64(7), capi._ptr(p["msum"]), ct.c_void_p(ns.data_ptr()),
                                          capi._ptr(p["s"]), capi._ptr(p["FTJF"]), capi._ptr(tm), capi._ptr(ts), ct.c_int64(len(tm)), capi._ptr(out))
    assert rc == -1 and b"nsess must be a host array" in capi.lib.gmmiv_last_error()
    with pytest.raises(capi.GmmivError, match=r"trial_seg\[2\] = 7 outside \[0, 7\)"):
        ctx.score_cosine_trials(p["m"], p["s"], [0, 1, 2], [0, 1, 7], out=out)
    assert np.all(out == SENTINEL)
    # nothing to do is valid: an empty list, with and without vectors
    for rule in ir.LIST_RULES:
        assert len(run_list(ctx, rule, p, tm[:0], ts[:0])) == 0
    assert len(ctx.score_cosine_trials(np.zeros((5, 0)), np.zeros((5, 0)), [], [])) == 0
    assert ctx.iv_trial_piece() == capi.IV_TRIAL_PIECE
    with options(ctx, {"iv_trials_piece": 4}):
        assert ctx.iv_trial_piece() == 4
    del torch


def test_a_used_context_gives_the_bits_of_a_fresh_one_and_allocates_nothing_twice():
    """the largest case, a PLDA call with another FTJF and a dense rule first, then the small cases: every score has the bits of the
    same call on a fresh context; a repeated call leaves every workspace slot as it is"""
    from lia_ral_amd import capi
    small = [(1, 1, 1), (5, 3, 7), (33, 2, 2), (129, 7, 5), (64, 7, 1)]

    def scores(c, dim, M, S):
        out = {}
        for rule in ir.LIST_RULES:
            p = br.score_case(*ir.case_key(dim, M, S, rule))
            for kind in ("full shuffled", "sparse"):
                tm, ts = ir.trial_list(kind, M, S)
                out[(rule, kind)] = run_list(c, rule, p, tm, ts)
        return out

    def slots(c):
        return [c.workspace_bytes(k) for k in range(256)]
    used = capi.Context(0)
    try:
        for rule in ir.LIST_RULES:
            p = br.score_case(*ir.case_key(257, 34, 130, rule))
            tm, ts = ir.trial_list("twice", 34, 130)
            run_list(used, rule, p, tm, ts, which="FTJF2")
            run_dense(used, rule, p)
        before = slots(used)
        p = br.score_case(257, 34, 130, "plain")
        tm, ts = ir.trial_list("twice", 34, 130)
        first = run_list(used, "plda", p, tm, ts, which="FTJF2")
        again = run_list(used, "plda", p, tm, ts, which="FTJF2")
        assert slots(used) == before and np.array_equal(first, again)
        f = Failures()
        for dim, M, S in small:
            got = scores(used, dim, M, S)
            fresh = capi.Context(0)
            try:
                want = scores(fresh, dim, M, S)
            finally:
                fresh.close()
            for k in want:
                f.same_bits("dim %d %dx%d %s %s on a used context" % ((dim, M, S) + k), got[k], want[k])
        assert slots(used) == before                                    # the small cases fit what the large one left
        f.finish()
    finally:
        used.close()


def test_resident_chain_into_the_list_normalisation(ctx):
    """scores stay on the device: list scores -> gmmiv_score_list_stats (a pos table grouped by model) -> gmmiv_score_normalize_list;
    against a numpy z-norm of the same list within the list calls' own bounds (tests/score_lists_ref.py)"""
    import torch
    from lia_ral_amd import capi
    key = (33, 33, 31, "plain")
    p = br.score_case(*key)
    tm, ts = ir.trial_list("sparse", 33, 31)
    models = np.unique(tm)
    pos = np.argsort(tm, kind="stable").astype(np.int64)               # the slots of a model are contiguous
    off = np.concatenate([[0], np.cumsum(np.bincount(tm, minlength=33)[models])]).astype(np.int64)
    row_id = np.searchsorted(models, tm).astype(np.int32)
    md, sd, d_pos, d_row = dev(p["m"]), dev(p["s"]), dev(pos), dev(row_id)
    sc = torch.empty(len(tm), dtype=torch.float64, device="cuda")
    mean = torch.empty(len(models), dtype=torch.float64, device="cuda")
    std = torch.empty(len(models), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    run_list(ctx, "mahalanobis", p, tm, ts, m=md, s=sd, out=sc)
    raw = torch.empty_like(sc)
    with torch.cuda.stream(ctx.torch_stream()):
        raw.copy_(sc)                                                   # a device copy, in stream order
    ctx.score_list_stats(off, sc, pos=d_pos, out_mean=mean, out_std=std)
    ctx.score_normalize_list(sc, capi.NORM_Z, row_id=d_row, row_mean=mean, row_std=std)
    ctx.sync()
    x, got, gm, gs = raw.cpu().numpy(), sc.cpu().numpy(), mean.cpu().numpy(), std.cpu().numpy()
    f = Failures()
    f.same_bits("the scores that went into the chain", x, run_list(ctx, "mahalanobis", p, tm, ts))
    for d, mdl in enumerate(models):
        idx = pos[off[d]:off[d + 1]]
        assert np.all(tm[idx] == mdl)
        m_ref, s_ref, kept = sr.ref_mean_std(x[idx], 0, 0.0, 0.0)
        dm, ds = sr.bounds(m_ref, s_ref, kept, 0)
        assert abs(gm[d] - m_ref) <= dm and abs(gs[d] - s_ref) <= ds, (mdl, gm[d], m_ref, dm, gs[d], s_ref, ds)
        if len(idx) < 2 or not s_ref > ds:
            continue                                                    # one score: std 0, the quotient is not a number on both sides
        y_ref = (x[idx] - m_ref) / s_ref
        bound = sr.norm_bound(y_ref, dm, ds, s_ref)
        assert np.all(np.abs(got[idx] - y_ref) <= bound), (mdl, np.max(np.abs(got[idx] - y_ref) / bound))
    f.finish()


# ---------------------------------------------------------------- the host layer
def _host_data(seed=2, dim=20, nspk=40):
    rng = np.random.default_rng(seed)
    sps = rng.integers(3, 7, nspk)
    cls = np.repeat(np.arange(nspk), sps)
    A = rng.normal(size=(dim, dim)) * 0.4 + np.eye(dim)
    dev_set = A @ ((rng.normal(size=(dim, nspk)) * 1.3)[:, cls] + rng.normal(size=(dim, int(sps.sum())))) + 0.5
    epm = np.array([1, 2, 1, 3, 2, 1, 2])
    enrol = A @ rng.normal(size=(dim, int(epm.sum()))) * 1.5 + 0.5
    test = A @ rng.normal(size=(dim, 9)) * 1.5 + 0.5
    rf, rg = 5, 3
    plda0 = (rng.normal(size=(dim, rf)), 0.3 * rng.normal(size=(dim, rg)), np.eye(dim) * 0.5 + 0.1 * A @ A.T)
    return dev_set, sps, enrol, epm, test, plda0


def _per_model(enrol, epm, mean):
    """ivTest step 4: the enrolment vectors of a model added in order, divided by their number for a mean"""
    out = np.empty((enrol.shape[0], len(epm)))
    s0 = 0
    for m, ns in enumerate(epm):
        a = np.zeros(enrol.shape[0])
        for e in range(ns):
            a = a + enrol[:, s0 + e]
        out[:, m] = a / float(ns) if mean else a
        s0 += ns
    return out


def _host_bars(scoring, m, s, mats, nsess):
    """the bars of tests/backend_ref.py (score_reference) for vectors and matrices that are not one of its cases"""
    dim = m.shape[0]
    if scoring == "cosine":
        nm, ns = np.sqrt(np.sum(m * m, 0)), np.sqrt(np.sum(s * s, 0))
        return (2 * (dim + 8) + 4) * br.u * (np.abs(m).T @ np.abs(s)) / (nm[:, None] * ns[None, :])
    if scoring == "mahalanobis":
        Q = mats["Mah"]
        return br.score_bar(dim, 0.5 * (br.abs_cross(Q, m, s) + br.abs_cross(Q.T, m, s)), 0.5 * br.abs_cols(Q, m), 0.5 * br.abs_cols(Q, s))
    if scoring == "2cov":
        G, H = mats["G"], mats["H"]
        GH = np.abs(G) + np.abs(H)
        return br.score_bar(dim, br.abs_cross(G, m, s) + br.abs_cross(G.T, m, s), br.abs_cols(GH, m), br.abs_cols(GH, s))
    FTJF = mats["FTJF"]
    kn = lambda n: (np.linalg.inv(n * FTJF + np.eye(dim)), -np.linalg.slogdet(n * FTJF + np.eye(dim))[1])
    kappa = float(np.linalg.cond((int(nsess.max()) + 1) * FTJF + np.eye(dim)))
    bar = np.empty((m.shape[1], s.shape[1]), br.LD)
    (K1, a1) = kn(1)
    for L in sorted(set(int(v) for v in nsess)):
        rows = np.flatnonzero(nsess == L)
        (KL, aL), (KL1, aL1) = kn(L), kn(L + 1)
        k1, kl, kl1 = np.abs(K1), np.abs(KL), np.abs(KL1)
        mr = m[:, rows]
        S_q = 0.5 * (br.abs_cross(kl1, mr, s) + br.abs_cross(kl1.T, mr, s)) + 0.5 * br.abs_cols(kl1 + kl, mr)[:, None] + 0.5 * br.abs_cols(kl1 + k1, s)[None, :]
        S_c = (abs(aL1) + abs(aL) + abs(a1)) / 2
        bar[rows] = (2 * (dim + 8) + br.PLDA_C_K * dim * kappa) * br.u * br.ld(S_q) + br.PLDA_C_LOGDET * dim * br.u * max(S_c, 1.0)
    return bar


@pytest.mark.parametrize("scoring", ["cosine", "mahalanobis", "2cov", "plda", "plda enrollMean"])
def test_iv_test_trials_gives_the_cells_of_iv_test(ctx, scoring):
    """liagpu::ivTestTrials against liagpu::ivTest on a small development set, per trial within 2 bars.  Without ivNorm and PLDA EM
    iterations every input of the rule can be rebuilt through the C ABI, which gives the vectors the bars are made of -- and, for
    enrollMean, gmmiv_score_plda on the means with nsess = 1, whose bits the dense ivTest must return."""
    from lia_ral_amd import host_capi as host
    dev_set, sps, enrol, epm, test, plda0 = _host_data()
    mode = "enrollMean" if scoring.endswith("enrollMean") else "native"
    scoring = scoring.split()[0]
    kw = dict(scoring=scoring, plda=plda0 if scoring == "plda" else None, plda_it=0, plda_scoring=mode)
    M, S = len(epm), test.shape[1]
    dense = host.iv_test(dev_set, sps, enrol, epm, test, **kw)
    assert dense.shape == (M, S)
    mats, nsess = {}, np.ones(M, np.int64)
    e, t = enrol, test
    if scoring == "mahalanobis":
        mats["Mah"] = ctx.dev_mahalanobis(dev_set, sps)
    elif scoring == "2cov":
        _, W, B = ctx.dev_cov_mat(dev_set, sps)
        mats["G"], mats["H"] = ctx.twocov_model(W, B)
    elif scoring == "plda":
        FTJ, mats["FTJF"] = ctx.plda_precompute(*plda0)
        e, t = ctx.iv_normalize(enrol, None, FTJ, False), ctx.iv_normalize(test, None, FTJ, False)
        if mode == "native":
            nsess = epm.astype(np.int64)
    m = _per_model(e, epm, mean=not (scoring == "plda" and mode == "native"))
    if scoring == "plda" and mode == "enrollMean":
        want = ctx.score_plda(m, nsess, t, mats["FTJF"])
        assert np.array_equal(dense, want)                              # pldaMeanScoring: the means, one session each
    bar = _host_bars(scoring, m, t, mats, nsess)                        # PLDA: on the sums, as score_reference takes them
    bad = []
    for kind in ("full shuffled", "sparse", "single"):
        tm, ts = ir.trial_list(kind, M, S)
        got = host.iv_test_trials(dev_set, sps, enrol, epm, test, tm, ts, **kw)
        r = np.abs(br.ld(got) - br.ld(dense[tm, ts])) / (2 * bar[tm, ts])
        print("%s %s %s: worst %.3f of 2 bars over %d trials" % (scoring, mode, kind, float(r.max()), len(tm)))
        if not np.all(r <= 1):
            i = int(np.argmax(r))
            bad.append("%s: trial %d = (%d, %d): %.3g of 2 bars" % (kind, i, tm[i], ts[i], float(r[i])))
    assert not bad, "\n".join(bad)


def test_iv_test_ndx_writes_the_lines_in_the_reference_order(ctx, tmp_path):
    """files in, file out: the vectors by id, an ndx with a duplicate, a targetIdList with a model that is never enrolled; the lines
    come segment-major with the model index ascending (IvTest.cpp:430-437) and carry the scores of ivTestTrials"""
    from lia_ral_amd import host_capi as host
    dev_set, sps, enrol, epm, test, _ = _host_data()
    dim = dev_set.shape[0]
    e_ids = ["e%d" % i for i in range(enrol.shape[1])]
    s_ids = ["seg%d" % i for i in range(test.shape[1])]
    d = str(tmp_path)
    host.io_vectors(d, e_ids + s_ids, ".y", "DB", np.concatenate([enrol.T, test.T]))
    starts = np.concatenate([[0], np.cumsum(epm)])
    names = ["spk%d" % m for m in range(len(epm))]
    with open(tmp_path / "ids.lst", "w") as f:
        for m, nme in enumerate(names):
            f.write(" ".join([nme] + e_ids[starts[m]:starts[m + 1]]) + "\n")
    lines = ["seg3 spk1 spk0 ghost", "seg0 spk4 spk3", "seg3 spk6 spk1", "seg8 spk2", "seg0 spk0"]
    with open(tmp_path / "t.ndx", "w") as f:
        f.write("\n".join(lines) + "\n")
    out = tmp_path / "res.txt"
    r = host.iv_test_ndx(dev_set, sps, str(tmp_path / "t.ndx"), d, str(out), target_id_list=str(tmp_path / "ids.lst"), scoring="mahalanobis",
                         gender="F", threshold=-1e9)
    nx = r["ndx"]
    assert nx["dropped"] == 1 and nx["segs"] == ["seg3", "seg0", "seg8"]
    # targetIdList sorted by element count, descending and stable: spk3 (3 sessions), then spk1, spk4, spk6 (2), then spk0, spk2, spk5
    assert nx["models"] == ["spk3", "spk1", "spk4", "spk6", "spk0", "spk2", "spk5"]
    want_pairs = sorted(set((nx["models"].index(mm), nx["segs"].index(l.split()[0])) for l in lines for mm in l.split()[1:] if mm != "ghost"),
                        key=lambda p: (p[1], p[0]))
    assert list(zip(r["line_model"].tolist(), r["line_seg"].tolist())) == want_pairs and len(want_pairs) == 7
    # the scores are those of ivTestTrials on the same vectors in the loader's order
    order = [names.index(n) for n in nx["models"]]
    enrol2 = np.concatenate([enrol[:, starts[m]:starts[m + 1]] for m in order], axis=1)
    test2 = test[:, [s_ids.index(s) for s in nx["segs"]]]
    direct = host.iv_test_trials(dev_set, sps, enrol2, epm[order], test2, r["line_model"], r["line_seg"], scoring="mahalanobis")
    assert np.array_equal(r["scores"], direct)
    got = [l.split() for l in open(out).read().splitlines()]
    assert [(g[0], g[1], g[2], g[3]) for g in got] == [("F", nx["models"][m], "1", nx["segs"][s]) for m, s in want_pairs]
    assert np.allclose([float(g[4]) for g in got], r["scores"], rtol=1e-5)      # the result line carries six significant digits
    assert dim == 20
