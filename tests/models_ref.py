"""Shared by test_cpu_gmm_models.py / test_gpu_gmm_models.py: the segment layout of the batched-model tests, a numpy restatement of
the batched MAP formula (gmmiv_map_adapt_models) and the enrolment loop assembled from the oracle's EM accumulator + that formula."""
import numpy as np

# a model used twice, an empty segment, boundaries off every multiple of 4 / 16 / 32 / 256; 9 leading and 5 trailing frames of nobody
SEG_LEN = [70, 0, 131, 64, 1, 3, 17, 259, 300]
SEG_MODEL = [0, 1, 2, 2, 4, 0, 3, 1, 4]
LEAD, TRAIL = 9, 5
N_MODELS = 5


def seg_layout():
    sb = LEAD + np.concatenate([[0], np.cumsum(SEG_LEN)]).astype(np.int64)
    return sb, np.asarray(SEG_MODEL, np.int32), int(sb[-1]) + TRAIL


def relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


def map_adapt_np(N, F, count, w0, mean0, cur, method, mean=True, weight=False, reg=(16.0, 16.0, 16.0), alpha_mean=0.75):
    """N [G, C], F [G, C, D], count [G], a-priori (w0 [C], mean0 [C, D]), cur [G, C, D] -> (means [G, C, D], weights [G, C]): the ML
    estimate of em_get (w = N / count, mean = F / N, N = 0: cur and weight 0) followed by the mean / weight branches of computeMAP, every
    operation in the order of liatools_gpu.cpp's computeMAP*."""
    N = np.asarray(N, np.float64); G, C = N.shape
    F = np.asarray(F, np.float64).reshape(G, C, -1)
    cur = np.broadcast_to(np.asarray(cur, np.float64).reshape(-1, C, F.shape[2]), F.shape)
    means = np.empty_like(F); weights = np.empty_like(N)
    for g in range(G):
        cnt = float(count[g])
        w = N[g] / cnt if cnt > 0 else np.zeros(C)
        with np.errstate(invalid="ignore", divide="ignore"):
            ml = np.where(N[g][:, None] > 0, F[g] / N[g][:, None], cur[g])
        n = float(int(cnt))                                  # the reference passes an unsigned long
        known = method in ("MAPOccDep", "MAPModelBased", "MAPConst", "MAPConst2")
        wt = w0.copy() if known else w
        if not known:
            m = ml
        elif not mean:
            m = mean0.copy()
        elif method in ("MAPOccDep", "MAPModelBased"):
            alpha = w * n
            a = (alpha / (alpha + reg[0]))[:, None]
            m = (1 - a) * mean0 + a * ml
        elif method == "MAPConst":
            m = (alpha_mean * mean0) + ((1 - alpha_mean) * ml)
        else:
            m = ((alpha_mean * w0[:, None] * mean0) + ((1 - alpha_mean) * w[:, None] * ml)) / (w0 * alpha_mean + w * (1 - alpha_mean))[:, None]
        if weight and method in ("MAPOccDep", "MAPModelBased"):
            alpha = w * n
            a = alpha / (alpha + reg[2])
            wt = a * w + (1 - a) * w0
            s = 0.0
            for v in wt:                                      # left to right like the reference's loop
                s += v
            wt = wt / s
        means[g] = m; weights[g] = wt
    return means, weights
