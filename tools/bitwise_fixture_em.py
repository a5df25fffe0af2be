#!/usr/bin/env python3
"""The readers of the stored likelihoods and running exponents (k_llk_mfma in WZ mode -> k_stats_z, k_post_from_z, k_topc_from_z)
at boundary shapes, as BITS.  A sibling of tools/bitwise_fixture.py, with the same two modes:
  tools/bitwise_fixture_em.py write out.json     compute with the library capi loads (GMMIV_LIB_PATH selects another build), store digests
  tools/bitwise_fixture_em.py check ref.json     compute again and compare the digests, key by key
Covered: the EM accumulator at vectSize 1, 13, 33, 60, 64, 80 and frame counts that end inside a 16-frame block, a 64-frame tile
and a segment, several frame chunks per call (small z_scratch_mb), f32 / f64 / row-strided features, the workgroup shapes and
stream depths of k_stats_z (z_waves 4 / 16, z_depth_em 4) and posterior pruning; the N / F rows of tv_stats (both N / F shapes);
the posterior vectors of gmmiv_occ; DETERMINE_TOP through the stored likelihoods (topc_fused 0); the compensated frames of
gmmiv_feat_compensate (one chunk, and a chunk plus a tail); gmmiv_llk_models / _tv_stats_models / _em_stats_models on segments that
start inside a 16-frame block, are empty, 17 frames long and four tiles long.
tests/golden/em_readers_bitwise.json was written by the library before the EM statistics kernel read x^2 from LDS and before the
running exponents were stored four to a 16-byte word (tests/test_gpu_em_readers_bitwise.py); its featcomp_ and models_ entries by the
library before the likelihood scratch got its one reserve function (gmmiv_z_reserve)."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

# frame counts: 16-frame block, 64-frame tile and 64-frame-aligned segment boundaries fall inside the last chunk
FRAMES = (1, 15, 17, 100, 1000, 4103, 6007, 12345)


def compute():
    import torch
    from conftest import make_frames, make_gmm
    from lia_ral_amd import capi
    out = {}
    ctx = capi.Context(0)

    def opt(key, value):
        return ctx.set_option(key, value)

    # EM accumulator, every vectSize, one chunk (default scratch) and several chunks
    for C, D in ((64, 1), (96, 13), (128, 33), (128, 60), (64, 64), (32, 80)):
        w, mean, iv = make_gmm(C, D, seed=C * 7 + D)
        g = ctx.gmm(w, mean, iv)
        for T in FRAMES:
            x = make_frames(w, mean, iv, T, seed=T + D)
            k = "%dx%dx%d" % (C, D, T)
            out["em_" + k] = g.em_accumulate(x)
            if T >= 4103:
                prev = opt("z_scratch_mb", 6)  # ~4900-frame chunks at 128 Gaussians (>= 4096 frames keep the chunked path)
                out["em_chunked_" + k] = g.em_accumulate(x)
                opt("z_scratch_mb", prev)
        g.close()

    # the default EM shape (2048 x 60): f32, f64, row-strided, chunked, the other kernel shapes and pruning
    C, D = 2048, 60
    w, mean, iv = make_gmm(C, D, seed=11)
    g = ctx.gmm(w, mean, iv)
    for T in (777, 12345):
        x = make_frames(w, mean, iv, T, seed=T)
        k = "%dx%dx%d" % (C, D, T)
        out["em_" + k] = g.em_accumulate(x)
        out["em_w_" + k] = g.em_accumulate(x, weight=0.37)
        out["em_f64_" + k] = g.em_accumulate(x.astype(np.float64))
        wide = torch.zeros((T, D + 3), dtype=torch.float32, device="cuda")
        wide[:, :D] = torch.from_numpy(x).cuda()
        acc = torch.zeros(g.em_acc_len(), dtype=torch.float64, device="cuda")
        g.em_accumulate(wide[:, :D], acc=acc)
        torch.cuda.synchronize()
        out["em_strided_" + k] = acc.cpu().numpy()
        for key, val in (("z_waves", 4), ("z_waves", 16), ("z_depth_em", 4), ("prune_log2", 20), ("z_scratch_mb", 100)):
            prev = opt(key, val)
            out["em_%s%d_%s" % (key, val, k)] = g.em_accumulate(x)
            opt(key, prev)
        out["occ_" + k] = g.occ(x[:300] if T > 300 else x)
        lens = [300, 0, 1, 17, T - 318]
        ub = np.concatenate([[0], np.cumsum(lens)])
        N, F = g.tv_stats(x, ub)
        out["N_" + k], out["F_" + k] = N, F
        for key, val in (("z_tv4", 0), ("z_depth_tv", 4)):
            prev = opt(key, val)
            N, F = g.tv_stats(x, ub)
            out["N_%s%d_%s" % (key, val, k)], out["F_%s%d_%s" % (key, val, k)] = N, F
            opt(key, prev)
        prev = opt("topc_fused", 0)
        d = g.llk_determine_top(x, 10)
        for f in ("idx", "lk", "nontop_llk", "nontop_w", "llk"):
            out["topz_%s_%s" % (f, k)] = d[f]
        opt("topc_fused", prev)
    g.close()

    # posterior vectors, N / F and top-C through the stored likelihoods at smaller models and odd frame counts
    for C, D, T in ((128, 60, 1000), (96, 13, 4103), (64, 33, 17), (64, 1, 100)):
        w, mean, iv = make_gmm(C, D, seed=C + 3 * D)
        g = ctx.gmm(w, mean, iv)
        x = make_frames(w, mean, iv, T, seed=T)
        k = "%dx%dx%d" % (C, D, T)
        out["occ_" + k] = g.occ(x)
        lens = [T // 3, 0, T - T // 3]
        N, F = g.tv_stats(x, np.concatenate([[0], np.cumsum(lens)]))
        out["N_" + k], out["F_" + k] = N, F
        prev = opt("topc_fused", 0)
        d = g.llk_determine_top(x, min(10, C))
        out["topz_idx_" + k], out["topz_llk_" + k] = d["idx"], d["llk"]
        opt("topc_fused", prev)
        g.close()

    # feature compensation through the stored likelihoods: one chunk, and a 4928-frame chunk plus a 1079-frame tail
    C, D = 128, 60
    w, mean, iv = make_gmm(C, D, seed=C * 7 + D)
    g = ctx.gmm(w, mean, iv)
    offset = np.random.default_rng(5).standard_normal((C, D))
    out["featcomp_%dx%dx1000" % (C, D)] = g.feat_compensate(make_frames(w, mean, iv, 1000, seed=1000 + D), offset)
    prev = opt("z_scratch_mb", 6)
    out["featcomp_chunked_%dx%dx6007" % (C, D)] = g.feat_compensate(make_frames(w, mean, iv, 6007, seed=6007 + D), offset)
    opt("z_scratch_mb", prev)
    g.close()

    # a model per segment: a first block that starts inside a 16-frame block, an empty segment, a 17-frame segment and a segment
    # over four 256-frame tiles
    G = 3
    models = [make_gmm(C, D, seed=40 + m) for m in range(G)]
    b = ctx.gmm_batch(G, C, D).load(*(np.stack([m[i] for m in models]) for i in range(3)))
    x = make_frames(*models[0], 1400, seed=1400)
    sb, sm = [5, 305, 305, 322, 1322], [0, 2, 2, 1]
    llk, seg_sum = b.llk(x, sb, sm)
    out["models_llk"], out["models_llk_seg_sum"] = llk[sb[0]:sb[-1]], seg_sum  # frames outside the segments are not written
    for f, v in zip(("N", "F", "seg_llk"), b.tv_stats(x, sb, sm)):
        out["models_tv_" + f] = v
    for f, v in zip(("N", "F", "S", "seg_llk"), b.em_stats(x, sb, sm)):
        out["models_em_" + f] = v
    b.close()
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
        bad = [k for k in ref if got.get(k) != ref[k]]
        print("%d arrays, %d differ: %s" % (len(ref), len(bad), bad[:20]))
        sys.exit(1 if bad else 0)
