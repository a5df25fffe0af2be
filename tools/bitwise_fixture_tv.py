#!/usr/bin/env python3
"""The i-vector half of the C API (capi_tv.hip, capi_iv_score.hip, capi_backend.hip) on every branch of its host-side dispatch, as
BITS.  A sibling of tools/bitwise_fixture.py and tools/bitwise_fixture_em.py, with the same two modes:
  tools/bitwise_fixture_tv.py write out.json     compute with the library capi loads (GMMIV_LIB_PATH selects another build), store digests
  tools/bitwise_fixture_tv.py check ref.json     compute again and compare the digests, key by key
tests/golden/r05_bitwise.json pins the default T-matrix EM path at even orders and two scoring rules; this one pins the rest, at the
smallest shapes at which each branch exists: the batched SPD work packed (order 34), unpacked + GEMM-built (order 33, and "chol_gemm" 1),
across batches and super-batches (tv_batch 3, tv_acc_mb 0), host and device accumulators; tv_update_t by substitution, by the explicit
inverse (D = 65, tv_mstep_solve 0, odd order) and over two chunks of systems; both routes of tv_min_divergence; the approximate
extractors and statistics steps; both routes of tv_orthonormalize_t; JFA; iv_normalize; the five scoring rules, apply_trials and
score_plda with odd and even operand counts; gmmiv_dgemm plain, split-K and with an epilogue; the PldaDev statistics, sym_eigen, EFR,
LDA, PLDA EM and pre-computation and the two-covariance model at even and odd dimensions.
tests/golden/tv_capi_bitwise.json was written by the library before the batched SPD work got its one owner (SpdBatch, capi_tv_util.h)
and before the host linear algebra moved to host_linalg.cpp (tests/test_gpu_tv_capi_bitwise.py).
The inputs come from numpy's generator and element-wise arithmetic only (no BLAS / LAPACK call, whose bits depend on the CPU)."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

N_KEYS = 256  # what compute() returns; tests/test_gpu_tv_capi_bitwise.py asserts that the golden has them all
ACC = ("A", "Cmx", "Rm", "r", "meanW", "W")


def spd(rng, n, scale=0.05):
    """symmetric, strictly diagonally dominant (so positive definite) for n <= 14; element-wise arithmetic only"""
    a = rng.normal(size=(n, n)) * scale
    return (a + a.T) / 2 + np.eye(n)


def tv_problem(C, D, R, U, seed):
    rng = np.random.default_rng(seed)
    N = rng.uniform(0.5, 40.0, (U, C))
    return dict(N=N, F=rng.normal(size=(U, C * D)) * np.repeat(N, D, axis=1), Tm=0.05 * rng.normal(size=(R, C * D)),
                invvar=rng.uniform(0.5, 2.0, C * D), means=rng.normal(size=C * D), C=C, D=D, R=R, U=U)


def compute():
    import torch
    from lia_ral_amd import capi
    out = {}
    ctx = capi.Context(0)

    class options:  # set for a block, put back after it
        def __init__(self, **kv):
            self.kv = kv

        def __enter__(self):
            self.prev = {k: ctx.set_option(k, v) for k, v in self.kv.items()}

        def __exit__(self, *exc):
            for k, v in self.prev.items():
                ctx.set_option(k, v)

    def on_device(a):
        """the context runs on a stream of its own: a tensor is complete before a call reads it (and torch.cuda.synchronize() comes
        between a call and the first look at a tensor it wrote)"""
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        torch.cuda.synchronize()
        return t

    def start_acc(p, seed, device=False):
        """accumulators that are not zero: the E-step adds to them"""
        rng = np.random.default_rng(seed)
        C, D, R = p["C"], p["D"], p["R"]
        acc = dict(A=rng.normal(size=(C, R * (R + 1) // 2)), Cmx=rng.normal(size=(R, C * D)), Rm=rng.normal(size=(R, R)), r=rng.normal(size=R),
                   meanW=rng.normal(size=R))
        return {k: on_device(v) for k, v in acc.items()} if device else acc

    def estep(tag, p, device_too=True):
        """tv_tett, tv_estimate_w, tv_estimate_a_and_c -> the host accumulators with A, Rm, r, meanW started at zero (what the M-step takes)"""
        C, D = p["C"], p["D"]
        te = ctx.tv_tett(p["Tm"], p["invvar"], C, D)
        out["tett_" + tag] = te
        out["W_" + tag] = ctx.tv_estimate_w(p["N"], p["F"], p["Tm"], p["invvar"], te, C, D)
        acc = ctx.tv_estimate_a_and_c(p["N"], p["F"], p["Tm"], p["invvar"], te, C, D)
        for f in ACC:
            out["estep_%s_%s" % (f, tag)] = np.asarray(acc[f]).copy()
        add = ctx.tv_estimate_a_and_c(p["N"], p["F"], p["Tm"], p["invvar"], te, C, D, acc=start_acc(p, 5))
        for f in ACC:
            out["estep_add_%s_%s" % (f, tag)] = np.asarray(add[f]).copy()
        if device_too:
            dev = ctx.tv_estimate_a_and_c(p["N"], p["F"], p["Tm"], p["invvar"], te, C, D, acc=start_acc(p, 5, device=True))
            torch.cuda.synchronize()
            for f in ACC[:-1]:
                out["estep_dev_%s_%s" % (f, tag)] = dev[f].cpu().numpy()
            out["estep_dev_W_" + tag] = np.asarray(dev["W"]).copy()
        return acc

    # ---- E-step at C = 6, D = 5, U = 7: packed, unpacked + GEMM-built, chol_gemm, batches and super-batches of 3 + 3 + 1
    p34, p33 = tv_problem(6, 5, 34, 7, 34), tv_problem(6, 5, 33, 7, 33)
    acc34 = estep("R34", p34)
    acc33 = estep("R33", p33)
    with options(chol_gemm=1):
        estep("R34_cholgemm", p34)
    with options(tv_batch=3, tv_acc_mb=0):
        estep("R34_b3", p34)
        estep("R33_b3", p33)
    p66 = tv_problem(6, 66, 34, 1, 66)
    out["tett_D66"] = ctx.tv_tett(p66["Tm"], p66["invvar"], 6, 66)
    with options(tv_tett_direct=0):
        out["tett_R34_gemm"] = ctx.tv_tett(p34["Tm"], p34["invvar"], 6, 5)
        out["tett_R33_gemm"] = ctx.tv_tett(p33["Tm"], p33["invvar"], 6, 5)

    # ---- tv_update_t on those accumulators
    def update_t(tag, acc, p):
        out["update_t_" + tag] = ctx.tv_update_t(acc["A"], acc["Cmx"], p["C"], p["D"])

    update_t("R34", acc34, p34)
    update_t("R33", acc33, p33)
    with options(tv_mstep_solve=0):
        update_t("R34_inverse", acc34, p34)
    with options(chol_gemm=1):
        update_t("R34_cholgemm", acc34, p34)
    p65 = tv_problem(2, 65, 34, 7, 65)
    update_t("R34_D65", estep("R34_D65", p65, device_too=False), p65)
    p300 = tv_problem(300, 2, 6, 7, 300)
    update_t("C300", estep("C300", p300, device_too=False), p300)

    # ---- tv_min_divergence: on the device, on the host (option, and odd order)
    def min_div(tag, acc, p):
        Rm, r, means, Tm = acc["Rm"].copy(), acc["r"].copy(), p["means"].copy(), p["Tm"].copy()
        ctx.tv_min_divergence(Rm, r, acc["meanW"] / p["U"], means, Tm, p["U"], p["C"], p["D"])
        for f, v in (("Rm", Rm), ("r", r), ("means", means), ("Tm", Tm)):
            out["md_%s_%s" % (f, tag)] = v

    min_div("R34", acc34, p34)
    min_div("R33", acc33, p33)
    with options(tv_md_device=0):
        min_div("R34_host", acc34, p34)

    # ---- approximate extractors and statistics steps, batches of 3 + 3 + 1
    def approx(tag, p, batch):
        C, D, R, U = p["C"], p["D"], p["R"], p["U"]
        rng = np.random.default_rng(1000 + R + D)
        weight = rng.uniform(0.5, 1.5, C); weight /= weight.sum()
        Q = rng.normal(size=(R, R)) / np.sqrt(R)
        with options(tv_batch=batch):
            Fn = ctx.tv_norm_statistics(p["N"], p["F"].copy(), p["means"], p["invvar"], C, D)
            Tn = ctx.tv_norm_t(p["Tm"].copy(), p["invvar"], C, D)
            Wm = ctx.tv_weighted_cov(Tn, weight, C, D)
            Dm = ctx.tv_approximate_tctc(Tn, Q, C, D)
            out["norm_statistics_" + tag], out["norm_t_" + tag], out["weighted_cov_" + tag], out["approximate_tctc_" + tag] = Fn, Tn, Wm, Dm
            out["w_ubm_weight_" + tag] = ctx.tv_estimate_w_ubm_weight(p["N"], Fn, Tn, Wm, C, D, out=rng.normal(size=(U, R)))
            out["w_eigen_" + tag] = ctx.tv_estimate_w_eigen(p["N"], Fn, Tn, Dm, Q, C, D, out=rng.normal(size=(U, R)))
            out["subtract_m_plus_tw_" + tag] = ctx.tv_subtract_m_plus_tw(p["N"], p["F"].copy(), p["means"], p["Tm"], rng.normal(size=(U, R)), C, D)

    approx("R34", p34, 3)
    approx("R33", p33, 3)
    # (beyond the smallest shapes: K = C D >= 2048, where the K range of F T^T and T T^T is split, and a last batch of 1 row after one of
    #  130 -- the full batch decides into how many layers)
    approx("splitk", tv_problem(64, 40, 34, 131, 64), 130)
    for D in (6, 5):  # the one-pass kernel, and its copy fallback at an odd vectSize
        p = tv_problem(6, D, 4, 7, D)
        out["subtract_m_to_D%d" % D] = ctx.tv_subtract_m_to(p["N"], p["F"], np.empty_like(p["F"]), p["means"], 6, D)
        out["subtract_m_D%d" % D] = ctx.tv_subtract_m(p["N"], p["F"].copy(), p["means"], 6, D)

    # ---- tv_orthonormalize_t: through the Cholesky factor of the Gram matrix, and step by step (a zero row has no factor)
    Tm = np.random.default_rng(6).normal(size=(6, 30))
    out["orthonormalize"] = ctx.tv_orthonormalize_t(Tm.copy())
    Tm[3] = 0.0
    out["orthonormalize_zero_row"] = ctx.tv_orthonormalize_t(Tm.copy())

    # ---- JFA at C = 6, D = 5, R = 3, 7 speakers
    C, D, R, nspk = 6, 5, 3, 7
    rng = np.random.default_rng(77)
    p = tv_problem(C, D, R, 9, 77)
    owner = np.array([0, 1, 1, 2, 3, 4, 5, 5, 6])
    Dm, Z, Y = rng.uniform(0.1, 1.0, C * D), rng.normal(size=(nspk, C * D)), rng.normal(size=(nspk, R))
    out["jfa_subtract"] = ctx.jfa_subtract(p["N"], p["F"].copy(), C, D, owner=owner, nfact=nspk, means=p["means"], T=p["Tm"], W=Y, Dm=Dm, Z=Z)
    out["jfa_subtract_means_only"] = ctx.jfa_subtract(p["N"], p["F"].copy(), C, D, means=p["means"])
    sess_begin = np.array([0, 1, 3, 4, 5, 6, 8, 9])
    out["jfa_subtract_sessions"] = ctx.jfa_subtract_sessions(sess_begin, p["N"], rng.normal(size=(nspk, C * D)), p["Tm"], rng.normal(size=(9, R)), C, D)
    Ns, Fs = p["N"][:nspk], p["F"][:nspk]
    out["jfa_estimate_z"] = ctx.jfa_estimate_z(Ns, Fs, p["invvar"], Dm, C, D)
    out["jfa_estimate_z_tau"] = ctx.jfa_estimate_z(Ns, Fs, p["invvar"], Dm, C, D, tau=14.0)
    Dn = Dm.copy()
    out["jfa_estimate_z_and_d_Z"] = ctx.jfa_estimate_z_and_d(Ns, Fs, p["invvar"], Dn, C, D)
    out["jfa_estimate_z_and_d_D"] = Dn

    # ---- iv_normalize: 12 -> 8 with mean, rotation and length norm; and with none of the three
    rng = np.random.default_rng(12)
    X = rng.normal(size=(12, 9))
    out["iv_normalize"] = ctx.iv_normalize(X, mean=rng.normal(size=12), M=rng.normal(size=(8, 12)), length_norm=True)
    out["iv_normalize_none"] = ctx.iv_normalize(X, length_norm=False)
    out["iv_normalize_mean_only"] = ctx.iv_normalize(X, mean=rng.normal(size=12), length_norm=True)

    # ---- scoring at dim 12: each operand once odd (copied to an even stride) and once even
    dim = 12
    for M, S in ((7, 10), (8, 9)):
        rng = np.random.default_rng(100 * M + S)
        tag = "%dx%d" % (M, S)
        models, segs = rng.normal(size=(dim, M)), rng.normal(size=(dim, S))
        G, H = spd(rng, dim), spd(rng, dim)
        out["score_cosine_" + tag] = ctx.score_cosine(models, segs)
        out["score_mahalanobis_" + tag] = ctx.score_mahalanobis(models, segs, G)
        out["score_twocov_" + tag] = ctx.score_twocov(models, segs, G, H)
        out["score_twocov_mix_part_" + tag] = ctx.score_twocov_mix_part(models, segs, G, rng.normal(size=(M, S)))
        out["score_apply_trials_" + tag] = ctx.score_apply_trials(rng.integers(0, 2, (M, S)).astype(np.uint8), rng.normal(size=(M, S)), fill=-1.5)
        nsess = [1, 1, 1, 2, 2, 3, 1, 1][:M]  # runs of odd and even length
        out["score_plda_" + tag] = ctx.score_plda(models, nsess, segs, spd(rng, dim))

    # ---- gmmiv_dgemm: plain, split-K chosen by the library (nz = 0, K = 4096), with an epilogue
    rng = np.random.default_rng(8)
    dev = lambda *shape: on_device(rng.normal(size=shape))

    def dgemm(*args, **kw):
        Cm = ctx.dgemm(*args, **kw)
        torch.cuda.synchronize()
        return Cm.cpu().numpy()

    out["dgemm_plain"] = dgemm(False, False, 1.5, dev(20, 30), dev(30, 10), 0.5, dev(20, 10))
    out["dgemm_nz0"] = dgemm(False, True, 1.0, dev(20, 4096), dev(10, 4096), 0.0, dev(20, 10), nz=0)
    out["dgemm_epilogue"] = dgemm(True, False, 1.0, dev(30, 20), dev(30, 10), 0.0, dev(20, 10), epi_mode=2, rv=dev(20), cv=dev(10), br=0.5, bc=-0.5, cst=0.25)

    # ---- back end: PldaDev statistics at an even and an odd dimension, 40 speakers
    for dim in (10, 11):
        rng = np.random.default_rng(dim)
        sps = rng.integers(2, 5, 40)
        X = rng.normal(size=(dim, int(sps.sum()))) + np.repeat(rng.normal(size=(dim, 40)), sps, axis=1)
        tag = "dim%d" % dim
        for f, v in zip(("mean", "spk_means"), ctx.dev_means(X, sps)):
            out["dev_means_%s_%s" % (f, tag)] = v
        for f, v in zip(("Sigma", "W", "B"), ctx.dev_cov_mat(X, sps)):
            out["dev_cov_mat_%s_%s" % (f, tag)] = v
        for f, v in zip(("SB", "SW"), ctx.dev_scatter_mat(X, sps)):
            out["dev_scatter_mat_%s_%s" % (f, tag)] = v
        out["dev_mahalanobis_" + tag] = ctx.dev_mahalanobis(X, sps)
        out["dev_wccn_chol_" + tag] = ctx.dev_wccn_chol(X, sps)
        W, B = spd(rng, dim), spd(rng, dim)
        for f, v in zip(("G", "H"), ctx.twocov_model(W, B)):
            out["twocov_model_%s_%s" % (f, tag)] = v
    rng = np.random.default_rng(1212)
    W, B = spd(rng, 12, 0.04), spd(rng, 12, 0.04)
    for f, v in zip(("vect", "val"), ctx.sym_eigen(B)):
        out["sym_eigen_" + f] = v
    for f, v in zip(("vect", "val"), ctx.sym_eigen(B, rank=5)):
        out["sym_eigen_rank5_" + f] = v
    out["dev_efr_matrix"] = ctx.dev_efr_matrix(W)
    for f, v in zip(("mat", "val"), ctx.dev_lda(W, B, 5)):
        out["dev_lda_" + f] = v
    for dim, rf, rg, nspk in ((8, 3, 2, 8), (8, 3, 0, 8)):
        rng = np.random.default_rng(10 * rf + rg)
        sps = rng.integers(2, 5, nspk)
        X = rng.normal(size=(dim, int(sps.sum()))) + np.repeat(rng.normal(size=(dim, nspk)), sps, axis=1) + 0.2
        start = (rng.normal(size=(dim, rf)), 0.5 * rng.normal(size=(dim, rg)), spd(rng, dim), 0.1 * rng.normal(size=dim))
        for where in ("host", "device"):
            Xw = X.copy() if where == "host" else on_device(X)
            F, G, Sigma, Delta = (a.copy() for a in start)
            for it in range(2):
                ctx.plda_em_iteration(Xw, sps, F, G, Sigma, Delta)
            torch.cuda.synchronize()
            tag = "rg%d_%s" % (rg, where)
            for f, v in (("X", Xw if where == "host" else Xw.cpu().numpy()), ("F", F), ("G", G), ("Sigma", Sigma), ("Delta", Delta)):
                out["plda_em_%s_%s" % (f, tag)] = v
    for dim, rf, rg in ((10, 4, 3), (11, 4, 0), (12, 4, 14)):  # rg > dim: the second inverse is the larger one
        rng = np.random.default_rng(100 * dim + rg)
        F, G = rng.normal(size=(dim, rf)), (0.5 * rng.normal(size=(dim, rg)) if rg else None)
        for f, v in zip(("FTJ", "FTJF"), ctx.plda_precompute(F, G, spd(rng, dim))):
            out["plda_precompute_%s_%dx%dx%d" % (f, dim, rf, rg)] = v
    ctx.close()
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


def digests(arrs):
    import hashlib
    return {k: {"sha256": hashlib.sha256(v.tobytes()).hexdigest(), "shape": list(v.shape), "dtype": str(v.dtype)} for k, v in arrs.items()}


if __name__ == "__main__":
    import json
    mode, path = sys.argv[1], sys.argv[2]
    got = digests(compute())
    if mode == "write":
        json.dump({"arrays": got}, open(path, "w"), indent=0, sort_keys=True)
        print("wrote the digests of %d arrays to %s" % (len(got), path))
    else:
        ref = json.load(open(path))["arrays"]
        bad = [k for k in ref if got.get(k) != ref[k]] + [k for k in got if k not in ref]
        print("%d arrays, %d differ: %s" % (len(ref), len(bad), bad[:20]))
        sys.exit(1 if bad else 0)
