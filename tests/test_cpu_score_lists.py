"""Score normalisation on lists, the parts that need no GPU: the new C ABI symbols and their argument checks (made before the context
is looked at), the host planner of the length classes, the list loader of the host layer, the refusal of a test line without a
distribution, a self-check of the numpy reference (tests/score_lists_ref.py) and a source check of score_norm_lists.hip."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

import score_lists_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL = ct.c_void_p(0)


def _p(a):
    return ct.c_void_p(a.ctypes.data)


def _stats(off, scores, pos=None, pre_id=None, pre_mean=None, pre_std=None, mode=0, pH=0.0, pL=0.0, ctx=NULL):
    from lia_ral_amd import capi
    off = np.ascontiguousarray(off, np.int64)
    nd = len(off) - 1
    scores = np.ascontiguousarray(scores, np.float64)
    m, s = np.full(max(nd, 1), 99.0), np.full(max(nd, 1), 99.0)
    keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((pos, np.int64), (pre_id, np.int32), (pre_mean, np.float64),
                                                                            (pre_std, np.float64))]
    q = [NULL if a is None else _p(a) for a in keep]
    rc = capi.lib.gmmiv_score_list_stats(ctx, ct.c_int64(nd), _p(off), q[0], _p(scores), ct.c_int64(len(scores)), q[1], q[2], q[3],
                                         ct.c_int64(0 if keep[2] is None else len(keep[2])), int(mode), ct.c_double(pH), ct.c_double(pL),
                                         _p(m), _p(s))
    assert np.all(m == 99.0) and np.all(s == 99.0)                     # nothing was written
    return rc, capi.lib.gmmiv_last_error().decode()


def test_symbols_are_exported_and_refuse_a_null_context():
    from lia_ral_amd import capi, host_capi
    for name in ("gmmiv_score_list_stats", "gmmiv_score_normalize_list", "gmmiv_plan_score_lists", "gmmiv_score_list_class"):
        assert hasattr(capi.lib, name), name
    for name in ("liagpu_compute_norm_lists", "liagpu_compute_norm_list_files", "liagpu_norm_lists_load"):
        assert hasattr(host_capi.lib, name), name
    for name in ("score_list_stats", "score_normalize_list"):
        assert hasattr(capi.Context, name), name
    rc, msg = _stats([0, 3], np.arange(3.0))
    assert rc == -1 and "score_list_stats: ctx == NULL" in msg          # GMMIV_ERR_ARG, with a message
    x = np.zeros(4); ids = np.zeros(4, np.int32); v = np.ones(2)
    rc = capi.lib.gmmiv_score_normalize_list(NULL, ct.c_int64(4), _p(x), 0, _p(ids), _p(v), _p(v), ct.c_int64(2), NULL, NULL, NULL,
                                             ct.c_int64(0), NULL)
    assert rc == -1 and b"score_normalize_list: ctx == NULL" in capi.lib.gmmiv_last_error()
    hdr = open(os.path.join(ROOT, "include", "gmmiv.h")).read()
    assert "GMMIV_SCORE_LIST_SCRATCH_BYTES(ndist) ((size_t)12 * (size_t)(ndist) + (size_t)8)" in hdr
    assert "#define GMMIV_SCORE_LIST_CLASSES 7" in hdr
    assert capi.list_scratch_bytes(1000) == 12008 and capi.SCORE_LIST_CLASSES == 7


def test_bad_arguments_are_refused_with_a_message_naming_the_distribution():
    """the arguments are checked before the context: the checks run here, where there is no device to make one on"""
    sc = np.arange(10.0)
    rc, msg = _stats([0, 4, 3, 10], sc)
    assert rc == -1 and "off decreases at distribution 1" in msg
    rc, msg = _stats([0, 4, 4, 10], sc)
    assert rc == -1 and "distribution 1 has 0 scores" in msg and "empty impostor cohort" in msg
    rc, msg = _stats([0, 4, 6, 10], sc, pH=0.5, pL=0.5)                 # 4: 2 + 2; 2: 1 + 1
    assert rc == -1 and "distribution 0: empty kept range, 4 scores with 2 + 2 discarded" in msg
    rc, msg = _stats([0, 5, 7, 10], sc, pH=0.5, pL=0.5)                 # 5 keeps one, 2 keeps none
    assert rc == -1 and "distribution 1: empty kept range, 2 scores with 1 + 1 discarded" in msg
    rc, msg = _stats([-1, 4], sc)
    assert rc == -1 and "off[0]" in msg
    for kw in (dict(pH=1.0), dict(pL=-0.1), dict(pH=float("nan"))):
        rc, msg = _stats([0, 10], sc, **kw)
        assert rc == -1 and "must lie in [0, 1)" in msg
    rc, msg = _stats([0, 10], sc, mode=2)
    assert rc == -1 and "mean_mode 2" in msg
    one = np.ones(3)
    rc, msg = _stats([0, 10], sc, pre_id=np.zeros(10, np.int32))
    assert rc == -1 and "pre_id goes with pre_mean and pre_std" in msg
    rc, msg = _stats([0, 10], sc, pre_mean=one, pre_std=one)
    assert rc == -1 and "pre_id goes with pre_mean and pre_std" in msg
    rc, msg = _stats([0, 10], sc, pre_id=np.zeros(10, np.int32), pre_mean=one)
    assert rc == -1 and "pre_mean and pre_std go together" in msg
    pid = np.zeros(10, np.int32); pid[7] = 3
    rc, msg = _stats([0, 4, 10], sc, pre_id=pid, pre_mean=one, pre_std=one)
    assert rc == -1 and "distribution 1: pre_id[7] = 3 outside [0, 3)" in msg
    pos = np.arange(10); pos[2] = 10
    rc, msg = _stats([0, 4, 10], sc, pos=pos)
    assert rc == -1 and "distribution 0: pos[2] = 10 outside [0, 10)" in msg
    pos[2] = -1
    rc, msg = _stats([3, 4, 10], sc, pos=pos)                           # slots before off[0] are not looked at
    assert rc == -1 and "ctx == NULL" in msg
    rc, msg = _stats([0, 4, 11], sc)
    assert rc == -1 and "beyond nscores = 10" in msg
    # the list normalisation
    from lia_ral_amd import capi
    x = np.full(4, 99.0); v = np.ones(2)
    call = lambda order, rid, cid: capi.lib.gmmiv_score_normalize_list(
        NULL, ct.c_int64(4), _p(x), order, NULL if rid is None else _p(rid), _p(v), _p(v), ct.c_int64(2), NULL if cid is None else _p(cid),
        _p(v), _p(v), ct.c_int64(2), NULL)
    ok, bad = np.array([0, 1, 1, 0], np.int32), np.array([0, 1, 2, 0], np.int32)
    assert call(7, ok, ok) == -1 and b"unknown order 7" in capi.lib.gmmiv_last_error()
    assert call(2, ok, None) == -1 and b"order 2 needs col_id" in capi.lib.gmmiv_last_error()
    assert call(0, None, ok) == -1 and b"order 0 needs row_id" in capi.lib.gmmiv_last_error()
    assert call(0, bad, None) == -1 and b"row_id[2] = 2 outside [0, 2)" in capi.lib.gmmiv_last_error()
    assert call(3, ok, bad) == -1 and b"col_id[2] = 2 outside [0, 2)" in capi.lib.gmmiv_last_error()
    assert call(1, None, bad) == -1 and b"col_id[2]" in capi.lib.gmmiv_last_error()
    assert np.all(x == 99.0)


def test_planner_bins_by_length_alone():
    from lia_ral_amd import capi
    rng = np.random.default_rng(4)
    lens = np.array([1, 2, 3, 8, 63, 64, 65, 511, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 40000, 512, 4097, 1])
    # the launch shapes of the dense call: 8 scores per thread in 64 .. 1024 threads, rows up to 16384 scores staged; a wave up to 4096
    for n in lens:
        k, thr, stage = capi.score_list_class(n, False)
        want = 64
        while want < (n + 7) // 8 and want < 1024:
            want *= 2
        assert thr == want and (stage >= n if n <= 16384 else stage == 0) and stage <= 16384, (n, k, thr, stage)
        assert stage == 0 or stage < 2 * n or n <= 512, (n, stage)      # a class stages at most twice what its shortest member needs
        k, thr, stage = capi.score_list_class(n, True)
        assert (k, thr, stage) == ((0, 64, 0) if n <= 4096 else (1, 256, 0))
    for streaming in (False, True):
        perm = rng.permutation(len(lens))
        results = []
        for order_of in (np.arange(len(lens)), perm):
            L = lens[order_of]
            off = np.concatenate([[5], 5 + np.cumsum(L)])
            cls, order, cb, used = capi.plan_score_lists(off, streaming)
            assert sorted(order.tolist()) == list(range(len(L)))           # every distribution exactly once
            assert cb[0] == 0 and cb[-1] == len(L) and np.all(np.diff(cb) >= 0)
            assert used == int(np.sum(np.diff(cb) > 0)) == len(set(cls.tolist()))
            for k in range(capi.SCORE_LIST_CLASSES):
                members = order[cb[k]:cb[k + 1]]
                assert np.all(cls[members] == k) and np.all(np.diff(members) > 0)   # table order inside a class
            for d, n in enumerate(L):
                assert cls[d] == capi.score_list_class(n, streaming)[0]    # a function of the length alone
            results.append(dict(zip(order_of.tolist(), cls.tolist())))
        assert results[0] == results[1]                                    # a shuffled table: the same class per distribution
    with pytest.raises(capi.GmmivError):
        capi.plan_score_lists([0, 4, 3], False)
    with pytest.raises(capi.GmmivError):
        capi.plan_score_lists([-2, 4], True)
    cls, order, cb, used = capi.plan_score_lists([7], False)               # no distribution
    assert len(cls) == 0 and used == 0 and np.all(cb == 0)


def _write(path, lines):
    with open(path, "w") as f:
        f.write("".join(l + "\n" for l in lines))
    return str(path)


def _nist(lines):
    return ["%s %s 0 %s %.17g" % l for l in lines]


def _lists():
    """3 models x 2 test segments (sparse), 4 impostor segments, 3 cohort models; ragged, one pair twice"""
    test = [("M", "m1", "s1", 0.5), ("F", "m3", "s2", -1.25), ("M", "m1", "s2", 2.0), ("M", "m2", "s1", 0.125)]
    zl = [("M", "m2", "i1", 1.0), ("M", "m1", "i3", 2.0), ("M", "m1", "i1", 3.0), ("M", "m2", "i4", 4.0), ("M", "m3", "i2", 5.0),
          ("M", "m1", "i3", 6.0), ("M", "m3", "i1", 7.0), ("M", "m2", "i2", 8.0), ("M", "m1", "i2", 9.0)]      # m1 lacks i4, (m1, i3) twice
    tl = [("M", "c1", "s1", 1.5), ("M", "c2", "s1", 2.5), ("M", "c3", "s2", 3.5), ("M", "c1", "s2", 4.5), ("M", "c3", "s1", 5.5)]  # s2 lacks c2
    ztl = [("M", c, i, 10.0 * a + b) for a, c in enumerate(("c1", "c2", "c3")) for b, i in enumerate(("i1", "i2", "i3", "i4"))][:-1]
    return test, zl, tl, ztl


def test_list_loader_keeps_file_order_duplicates_and_the_selection(tmp_path):
    """host only: runs before (and without) a device"""
    from lia_ral_amd import host_capi
    test, zl, tl, ztl = _lists()
    f = {k: _write(tmp_path / (k + ".nist"), _nist(v)) for k, v in (("test", test), ("z", zl), ("t", tl), ("zt", ztl))}
    # the dense loader refuses exactly this list
    with pytest.raises(host_capi.HostError, match="not a full cross product"):
        host_capi.compute_norm_files(f["test"], str(tmp_path / "o"), "znorm", znorm_nist_file=f["z"])
    L = host_capi.load_compute_norm_lists(f["test"], "znorm", znorm_nist_file=f["z"])
    z = L["z"]
    assert z["keys"] == ["m2", "m1", "m3"]                                 # order of first appearance
    assert z["off"].tolist() == [0, 3, 7, 9]
    assert z["scores"].tolist() == [1.0, 4.0, 8.0, 2.0, 3.0, 6.0, 9.0, 5.0, 7.0]    # file order inside a distribution, (m1, i3) twice
    assert z["other"] is None and L["line_seg"] is None
    assert L["x"].tolist() == [0.5, -1.25, 2.0, 0.125] and L["line_model"].tolist() == [1, 2, 1, 0]
    assert L["t"]["keys"] == [] and L["t"]["off"].tolist() == [0]
    # the same through the reference restatement
    d = sr.get_all_scores(zl, "name")
    assert list(d) == z["keys"] and [v[0] for v in d.values()] == [[1.0, 4.0, 8.0], [2.0, 3.0, 6.0, 9.0], [5.0, 7.0]]
    # impostorIDList looks at the OTHER field
    ids = _write(tmp_path / "ids.lst", ["i1 i3", "c1", "c3"])
    L = host_capi.load_compute_norm_lists(f["test"], "znorm", znorm_nist_file=f["z"], impostor_id_list=ids)
    assert L["z"]["keys"] == ["m2", "m1", "m3"] and L["z"]["off"].tolist() == [0, 1, 4, 5]
    assert L["z"]["scores"].tolist() == [1.0, 2.0, 3.0, 6.0, 7.0]
    L = host_capi.load_compute_norm_lists(f["test"], "tnorm", tnorm_nist_file=f["t"], impostor_id_list=ids)
    assert L["t"]["keys"] == ["s1", "s2"] and L["t"]["scores"].tolist() == [1.5, 5.5, 3.5, 4.5] and L["line_seg"].tolist() == [0, 1, 1, 0]
    assert L["line_model"] is None
    # ztnorm: zt by impostor segment, z carries the zt distribution of every slot's segment
    L = host_capi.load_compute_norm_lists(f["test"], "ztnorm", znorm_nist_file=f["z"], tnorm_nist_file=f["t"], ztnorm_nist_file=f["zt"])
    assert L["zt"]["keys"] == ["i1", "i2", "i3", "i4"] and L["zt"]["off"].tolist() == [0, 3, 6, 9, 11]
    assert L["zt"]["scores"].tolist() == [0.0, 10.0, 20.0, 1.0, 11.0, 21.0, 2.0, 12.0, 22.0, 3.0, 13.0]
    assert L["z"]["other"].tolist() == [0, 3, 1, 2, 0, 2, 1, 1, 0] and L["t"]["other"] is None
    # tznorm: zt by cohort model, t carries the zt distribution of every slot's model
    L = host_capi.load_compute_norm_lists(f["test"], "tznorm", znorm_nist_file=f["z"], tnorm_nist_file=f["t"], ztnorm_nist_file=f["zt"])
    assert L["zt"]["keys"] == ["c1", "c2", "c3"] and L["zt"]["off"].tolist() == [0, 4, 8, 11]
    assert L["t"]["keys"] == ["s1", "s2"] and L["t"]["other"].tolist() == [0, 1, 2, 2, 0] and L["z"]["other"] is None
    # field positions: score first, then segment, model, gender, decision
    swapped = lambda lines: ["%.17g %s %s %s 0" % (sc, s, m, g) for g, m, s, sc in lines]
    L2 = host_capi.load_compute_norm_lists(_write(tmp_path / "t2.nist", swapped(test)), "znorm",
                                           znorm_nist_file=_write(tmp_path / "z2.nist", swapped(zl)), fields=(3, 2, 4, 1, 0))
    assert L2["z"]["keys"] == z["keys"] and L2["z"]["scores"].tolist() == z["scores"].tolist() and L2["x"].tolist() == [0.5, -1.25, 2.0, 0.125]


def test_a_missing_distribution_is_named_before_a_device_is_opened(tmp_path):
    from lia_ral_amd import host_capi
    test, zl, tl, ztl = _lists()
    out = str(tmp_path / "out")
    f = {k: _write(tmp_path / (k + ".nist"), _nist(v)) for k, v in (("z", zl), ("t", tl), ("zt", ztl))}
    t_bad_m = _write(tmp_path / "t1.nist", _nist(test + [("M", "m9", "s1", 0.0)]))
    t_bad_s = _write(tmp_path / "t2.nist", _nist(test + [("M", "m1", "s9", 0.0)]))
    with pytest.raises(host_capi.HostError, match=r"not found for id \[m9\]"):
        host_capi.compute_norm_list_files(t_bad_m, out, "znorm", znorm_nist_file=f["z"])
    with pytest.raises(host_capi.HostError, match=r"not found for seg \[s9\]"):
        host_capi.compute_norm_list_files(t_bad_s, out, "tnorm", tnorm_nist_file=f["t"])
    with pytest.raises(host_capi.HostError, match=r"not found for seg \[s9\]"):
        host_capi.compute_norm_list_files(t_bad_s, out, "ztnorm", znorm_nist_file=f["z"], tnorm_nist_file=f["t"], ztnorm_nist_file=f["zt"])
    # a cohort line whose second field has no first-stage distribution (:483)
    z_bad = _write(tmp_path / "zb.nist", _nist(zl + [("M", "m1", "i7", 1.0)]))
    t_ok = _write(tmp_path / "t0.nist", _nist(test))
    with pytest.raises(host_capi.HostError, match=r"distribution for \[i7\] not found"):
        host_capi.compute_norm_list_files(t_ok, out, "ztnorm", znorm_nist_file=z_bad, tnorm_nist_file=f["t"], ztnorm_nist_file=f["zt"])
    with pytest.raises(KeyError, match="i7"):
        sr.chain_ref(test, zl + [("M", "m1", "i7", 1.0)], tl, ztl, "ztnorm", 0, 0.0, 0.0)
    # ... unless impostorIDList leaves that line out
    ids = _write(tmp_path / "ids.lst", ["i1", "i2", "i3", "i4", "c1", "c2", "c3"])
    L = host_capi.load_compute_norm_lists(t_ok, "ztnorm", znorm_nist_file=z_bad, tnorm_nist_file=f["t"], ztnorm_nist_file=f["zt"], impostor_id_list=ids)
    assert L["z"]["off"].tolist() == [0, 3, 7, 9]
    with pytest.raises(host_capi.HostError, match="unknown normalization mode"):
        host_capi.compute_norm_list_files(t_ok, out, "snorm", znorm_nist_file=f["z"])
    assert not any(os.path.exists(out + e) for e in (".znorm", ".tnorm", ".ztnorm", ".tznorm"))


def test_reference_list_chains_equal_matrix_chains_on_a_cross_product():
    rng = np.random.default_rng(12)
    M, S, Nt, Nz = 5, 6, 7, 8
    names = lambda p, n: ["%s%d" % (p, i) for i in range(n)]
    ms, ss, cs, is_ = names("m", M), names("s", S), names("c", Nt), names("i", Nz)
    for integer in (True, False):
        gen = (lambda shape: rng.integers(-20, 21, shape).astype(np.float64)) if integer else (lambda shape: rng.normal(-1.0, 2.0, shape))
        X, Z, T, ZT = gen((M, S)), gen((M, Nz)), gen((Nt, S)), gen((Nt, Nz))
        lines = lambda A, r, c: [("M", r[i], c[j], A[i, j]) for i in range(len(r)) for j in range(len(c))]
        test, zl, tl, ztl = lines(X, ms, ss), lines(Z, ms, is_), lines(T, cs, ss), lines(ZT, cs, is_)
        for mode, pH, pL in ((0, 0.0, 0.0), (0, 0.2, 0.15), (1, 0.0, 0.0), (1, 0.25, 0.25)):
            def stat(A, axis, pre=None):                                   # plain numpy on matrices, one distribution per row / column
                D = A if axis == 0 else A.T
                if pre is not None:
                    D = (D - pre[0][None, :]) / pre[1][None, :]
                r = [sr.ref_mean_std(row, mode, pH, pL) for row in D]
                return np.array([v[0] for v in r]), np.array([v[1] for v in r])
            col, row = (lambda v: v[:, None]), (lambda v: v[None, :])
            with np.errstate(invalid="ignore", divide="ignore"):
                want = {}
                mz, sz = stat(Z, 0); want["znorm"] = ((X - col(mz)) / col(sz), None)
                mt, st = stat(T, 1); want["tnorm"] = ((X - row(mt)) / row(st), None)
                ma, sa = stat(ZT, 1); mz2, sz2 = stat(Z, 0, (ma, sa)); x1 = (X - row(mt)) / row(st)
                want["ztnorm"] = ((x1 - col(mz2)) / col(sz2), x1)
                ma, sa = stat(ZT, 0); mt2, st2 = stat(T, 1, (ma, sa)); x1 = (X - col(mz)) / col(sz)
                want["tznorm"] = ((x1 - row(mt2)) / row(st2), x1)
            for nt in ("znorm", "tnorm", "ztnorm", "tznorm"):
                got = sr.chain_ref(test, zl, tl, ztl, nt, mode, pH, pL)
                y = np.array([g[0] for g in got]).reshape(M, S)
                assert np.array_equal(y, want[nt][0], equal_nan=True), (integer, nt, mode, pH, pL)
                if want[nt][1] is not None:
                    assert np.array_equal(np.array([g[2] for g in got]).reshape(M, S), want[nt][1], equal_nan=True)
                else:
                    assert all(g[2] is None for g in got)
    # integer scores: the statistics are exact (sums of small integers in any order), here against exact integer arithmetic
    v = [3, -7, 12, 12, 0, -7, 5, 9]
    mu, sd, kept = sr.ref_mean_std(v, 0, 0.25, 0.25)                        # drops 12 12 and -7 -7
    assert kept.tolist() == [9.0, 5.0, 3.0, 0.0] and mu == 17.0 / 4 and sd == np.sqrt(115.0 / 4 - (17.0 / 4) ** 2)
    mu, sd, _ = sr.ref_mean_std(v, 1, 0.0, 0.0)                             # the quirk: position n / 2 in input order
    assert mu == 0.0 and sd == 55.0 / 8
    mu, sd, _ = sr.ref_mean_std(v, 1, 0.25, 0.25)
    assert mu == 3.0 and sd == (6 + 2 + 0 + 3) / 4.0


def test_list_kernel_source_has_no_floating_point_atomic():
    """determinism is structural: the only atomics are integer adds of 1 into the LDS histograms and the LDS candidate counters"""
    src = open(os.path.join(ROOT, "lia_ral_amd", "csrc", "score_norm_lists.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "unsafeAtomicAdd" not in code and "atomicAdd_system" not in code and "__hip_atomic" not in code
    calls = re.findall(r"atomic\w*\s*\(([^;]*);", code)
    assert calls, "the radix select counts with LDS atomics"
    for c in calls:
        assert re.match(r"&hist\[[^\]]*\], 1u\)", c.strip()) or re.match(r"&s_nc\[[^\]]*\], 1\)", c.strip()), c
    assert re.search(r"unsigned \*hist = \(unsigned \*\)sbuf;", code) and re.search(r"__shared__ u64 sbuf\[", code)
    assert re.search(r"__shared__ int s_nc\[", code)
    assert "#pragma clang fp contract(off)" in src
    for k in ("k_norm_select_lists", "k_norm_listsum", "k_norm_apply_list"):
        assert re.search(r"__global__[^;{]*\b%s\b" % k, code), k
    mk = open(os.path.join(ROOT, "lia_ral_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "score_norm_lists.hip" in srcs and "capi_score_lists.hip" in srcs
