"""MLLR mean adaptation on the device (gmmiv_mllr_adapt_models, k_mllr_solve) and end to end (adaptModelBatch with "MLLR").

Every system (client g, dimension p) is judged on its own against the 80-bit reference of tests/mllr_ref.py; the bar is
spd_ref.accept: err <= 16 max(err of the double restatement on the same system, 64 u).  References are computed once per shape and
shared read-only."""
import functools

import numpy as np
import pytest

import mllr_ref
import spd_ref
from conftest import make_frames, make_gmm

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not spd_ref.HAVE_LONGDOUBLE, reason=spd_ref.SKIP_MESSAGE)]

# D + 1 and D + 2 on both sides of 16 / 32 / 64, C not a multiple of 4, the production shape once
SHAPES = [(1, 5, 1), (3, 9, 2), (2, 16, 3), (3, 64, 14), (3, 70, 15), (2, 67, 32), (2, 130, 31), (3, 256, 60), (2, 130, 62), (1, 2048, 60)]
ILL = [(32, 1.0, 5.0), (60, 1.0, 5.0), (32, 10.0, -20.0), (60, 10.0, -20.0)]     # (D, scale, shift) of the a-priori means, C = 256


@pytest.fixture(scope="module")
def ctx():
    from lia_ral_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def case(G, C, D, scale=1.0, shift=0.0, keep_systems=False):
    k = mllr_ref.generate(G, C, D, seed=1000 * G + 10 * C + D, scale=scale, shift=shift)
    ref = [mllr_ref.exact(k["mean0"], k["cov0"], k["N"][g], k["m"][g], keep_systems) for g in range(G)]
    res = [mllr_ref.restate(k["mean0"], k["cov0"], k["N"][g], k["m"][g]) for g in range(G)]
    return k, ref, res


def run(ctx, k, sel=None):
    from lia_ral_amd import capi
    N, F = (k["N"], k["F"]) if sel is None else (k["N"][sel], k["F"][sel])
    W, means, status = capi.mllr_adapt(ctx, N, F, k["mean0"], k["cov0"])
    C, D = k["mean0"].shape
    return W, means.reshape(len(N), C, D), status


@pytest.mark.parametrize("G,C,D", SHAPES)
def test_every_system_of_every_shape(ctx, G, C, D):
    k, ref, res = case(G, C, D)
    W, means, status = run(ctx, k)
    assert np.array_equal(status, np.zeros(G, np.int32))
    failures, worst = [], 0.0
    for g in range(G):
        worst = max(worst, mllr_ref.check_client(W[g], means[g], ref[g][0], ref[g][1], res[g][0], res[g][1], "(%d, %d, %d) g=%d" % (G, C, D, g), failures))
    print("(%d, %d, %d): worst err / bar = %.3g over %d systems" % (G, C, D, worst, G * D))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("D,scale,shift", ILL)
def test_ill_conditioned_inputs_by_backward_error(ctx, D, scale, shift):
    """a-priori means far from the origin: cond_2 G in the millions.  The forward error of a correct solve scatters far around the
    restatement's there, so each system is judged by eta = ||z - G w^|| / (||G||_2 ||w^|| + ||z||), G and z formed in 80-bit:
    eta <= 16 max(eta of the restatement, 64 u).  The adapted means: spd_ref.accept against the restatement's mean error."""
    G, C = 2, 256
    k, ref, res = case(G, C, D, scale, shift, True)
    W, means, status = run(ctx, k)
    assert np.array_equal(status, np.zeros(G, np.int32))
    failures, worst, conds = [], 0.0, []
    for g in range(G):
        Wr, mr, Gs, z = ref[g]
        for p in range(D):
            Gd = Gs[p].astype(np.float64)
            n2 = np.linalg.norm(Gd, 2)
            if p % 16 == 0:
                conds.append(np.linalg.cond(Gd))
            eta, eta0 = spd_ref.backward_error(Gs[p], n2, W[g, p], z[p]), spd_ref.backward_error(Gs[p], n2, res[g][0][p], z[p])
            worst = max(worst, eta / spd_ref.bar(eta0))
            if not spd_ref.accept(eta, eta0):
                failures.append("g=%d p=%d: eta %.3e, restatement %.3e, bar %.3e" % (g, p, eta, eta0, spd_ref.bar(eta0)))
        e, e0 = mllr_ref.mean_error(means[g], mr), mllr_ref.mean_error(res[g][1], mr)
        print("D=%d scale=%g shift=%g g=%d: mean error %.3e, restatement %.3e" % (D, scale, shift, g, e, e0))
        if not spd_ref.accept(e, e0):
            failures.append("g=%d means: error %.3e, restatement %.3e, bar %.3e" % (g, e, e0, spd_ref.bar(e0)))
    print("D=%d scale=%g shift=%g: cond_2 G up to %.2e, worst eta / bar = %.3g" % (D, scale, shift, max(conds), worst))
    assert not failures, "\n".join(failures)


def test_failure_status_leaves_the_neighbours_alone(ctx):
    """a client without a single occupied Gaussian between two good ones: an exact zero pivot.  status = [0, != 0, 0]; the failed
    client has W = [0 | I] and the a-priori means, bit for bit; its neighbours are what a batch without it gives"""
    k, _, _ = case(3, 70, 15)
    C, D = k["mean0"].shape
    N = k["N"].copy(); F = k["F"].copy()
    N[1] = 0.0
    bad = dict(k, N=N, F=F)
    W, means, status = run(ctx, bad)
    assert status[0] == 0 and status[2] == 0 and status[1] != 0
    assert np.array_equal(means[1], k["mean0"])
    assert np.array_equal(W[1], np.concatenate([np.zeros((D, 1)), np.eye(D)], axis=1))
    W2, means2, status2 = run(ctx, k, [0, 2])
    assert np.array_equal(status2, np.zeros(2, np.int32))
    assert np.array_equal(W[[0, 2]], W2) and np.array_equal(means[[0, 2]], means2)


def test_a_clients_bits_do_not_depend_on_the_batch(ctx):
    """alone, first or last of seven, on a second call, through GmmBatch, with torch device tensors: the same bits"""
    import torch
    from lia_ral_amd import capi
    k, _, _ = case(3, 256, 60)
    C, D = k["mean0"].shape
    W1, m1, s1 = run(ctx, k, [1])
    sel = [1, 0, 2, 0, 2, 0, 1]
    W7, m7, s7 = run(ctx, k, sel)
    for pos in (0, 6):
        assert np.array_equal(W7[pos], W1[0]) and np.array_equal(m7[pos], m1[0])
    W7b, m7b, s7b = run(ctx, k, sel)
    assert np.array_equal(W7, W7b) and np.array_equal(m7, m7b) and np.array_equal(s7, s7b)
    b = ctx.gmm_batch(7, C, D)
    Wg, mg, sg = b.mllr_adapt(k["N"][sel], k["F"][sel], k["mean0"], k["cov0"])
    b.close()
    assert np.array_equal(Wg, W7) and np.array_equal(mg.reshape(7, C, D), m7)
    dev = lambda a: torch.from_numpy(np.array(a)).to("cuda")
    Wt, mt, st = capi.mllr_adapt(ctx, dev(k["N"][sel]), dev(k["F"][sel]), dev(k["mean0"]), dev(k["cov0"]))
    ctx.sync()
    assert Wt.is_cuda and mt.is_cuda and st.is_cuda and st.dtype == torch.int32
    assert np.array_equal(Wt.cpu().numpy(), W7) and np.array_equal(mt.cpu().numpy().reshape(7, C, D), m7) and np.array_equal(st.cpu().numpy(), s7)


def test_vectsize_63_is_refused_with_a_message(ctx):
    from lia_ral_amd import capi
    k = mllr_ref.generate(1, 70, 63, seed=1)
    with pytest.raises(capi.GmmivError, match="-3.*vectSize 63"):
        capi.mllr_adapt(ctx, k["N"], k["F"], k["mean0"], k["cov0"])


# ---- end to end: liagpu::adaptModelBatch("MLLR") against the adaptModel loop ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def enroll_case(C, D, n_clients=5, frames=400):
    w, mean, iv = make_gmm(C, D, seed=C + D)
    x = make_frames(w, mean, iv, n_clients * frames, seed=11)
    sb = np.arange(n_clients) * frames
    sl = np.full(n_clients, frames)
    cb = np.arange(n_clients + 1)
    return (w, mean, 1.0 / iv), x, cb, sb, sl


def loop(h, case_, method, nb_it):
    world, x, cb, sb, sl = case_
    return [h.train_target_ex(x, sb[i:i + 1], sl[i:i + 1], world, method=method, nb_it=nb_it) for i in range(len(sb))]


def max_cond(h, case_):
    """the largest cond_2 G_p over clients and dimensions, G_p formed with numpy from the loop's ML estimate of the first iteration"""
    world, x, cb, sb, sl = case_
    C, D = world[1].shape
    Xi = np.concatenate([np.ones((C, 1)), world[1]], axis=1)
    kappa, ml = 0.0, []
    for i in range(len(sb)):
        w, m, c = h.train_target_ex(x, sb[i:i + 1], sl[i:i + 1], world, method="none", nb_it=1)    # an unknown MAPAlgo: the ML estimate
        ml.append((w, m))
        for p in range(D):
            kappa = max(kappa, np.linalg.cond(Xi.T @ ((w / world[2][:, p])[:, None] * Xi)))
    return kappa, ml


def rel(a, ref):
    return float(np.max(np.abs(a - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("C,D", [(64, 20), (64, 13)])
def test_train_target_batch_mllr_against_the_loop(C, D):
    """nb_it = 1: the two paths differ by the summation order of the statistics rows (1e-13), which the solve
    amplifies by at most cond_2 G: bar 16 kappa 1e-13.  nb_it = 2: one more EM pass amplifies that difference by a factor nobody fixed
    in advance; the batch-against-loop error of the "MAPOccDep" path at the same shape and iteration count is measured here (it is what
    the code did before MLLR existed) and the MLLR bar is 16 kappa x that error.
    Measured on an MI355X: (64, 20) kappa 76.2, nb_it = 1 error 3.6e-15 (bar 1.2e-10); nb_it = 2 MAPOccDep 2.2e-16, MLLR 3.7e-15 (bar 2.7e-13).
    (64, 13) kappa 32.8, nb_it = 1 error 2.3e-15 (bar 5.2e-11); nb_it = 2 MAPOccDep 3.7e-16, MLLR 1.9e-15 (bar 1.9e-13)."""
    from lia_ral_amd import host_capi as h
    cs = enroll_case(C, D)
    world, x, cb, sb, sl = cs
    kappa, ml = max_cond(h, cs)
    for nb_it in (1, 2):
        ref = loop(h, cs, "MLLR", nb_it)
        w, mean, cov, Wm = h.train_target_batch(x, cb, sb, sl, world, method="MLLR", nb_it=nb_it, return_mllr=True)
        e = max(rel(mean[i], ref[i][1]) for i in range(len(sb)))
        if nb_it == 1:
            bar = 16 * kappa * 1e-13
            W0 = Wm[0]
        else:
            refm = loop(h, cs, "MAPOccDep", 2)
            bm = h.train_target_batch(x, cb, sb, sl, world, method="MAPOccDep", nb_it=2)
            e_map = max(rel(bm[1][i], refm[i][1]) for i in range(len(sb)))
            bar = 16 * kappa * e_map
            print("(%d, %d) nb_it = 2: MAPOccDep batch against loop %.3e" % (C, D, e_map))
        print("(%d, %d) nb_it = %d: kappa = %.3e, MLLR batch against loop %.3e, bar %.3e" % (C, D, nb_it, kappa, e, bar))
        assert e <= bar
        for i in range(len(sb)):
            assert np.array_equal(w[i], world[0]) and np.array_equal(cov[i], world[2])
            assert np.array_equal(ref[i][0], world[0]) and np.array_equal(ref[i][2], world[2])
    # return_mllr: client 0's W of the first iteration is what computeMLLR gives on its ML estimate, to the bar of the per-system test
    w_ml, m_ml = ml[0]
    occ = w_ml * float(sl[0])
    m_in = np.where((occ == 0)[:, None], np.nan, m_ml)
    W_ref, m_ref = mllr_ref.exact(world[1], world[2], occ, m_in)
    W_np, m_np = mllr_ref.restate(world[1], world[2], occ, m_in)
    W_host, _ = h.compute_mllr(world, (w_ml, m_ml), float(sl[0]))
    failures = []
    mllr_ref.check_client(W0, m_ref, W_ref, m_ref, W_np, m_np, "return_mllr", failures)
    mllr_ref.check_client(W_host, m_ref, W_ref, m_ref, W_np, m_np, "compute_mllr", failures)
    assert not failures, "\n".join(failures)


def test_vectsize_64_takes_the_per_client_loop():
    """(C, D) = (16, 64): no device entry for this width, adaptModelBatch runs adaptModel client after client -- the same bits.  (With
    16 Gaussians for 65 unknowns the systems are rank deficient: the shape checks the routing, not the numbers.)"""
    from lia_ral_amd import host_capi as h
    cs = enroll_case(16, 64, 3, 200)
    world, x, cb, sb, sl = cs
    ref = loop(h, cs, "MLLR", 1)
    w, mean, cov = h.train_target_batch(x, cb, sb, sl, world, method="MLLR", nb_it=1)
    for i in range(len(sb)):
        assert np.array_equal(mean[i], ref[i][1], equal_nan=True) and np.array_equal(w[i], ref[i][0]) and np.array_equal(cov[i], ref[i][2])
