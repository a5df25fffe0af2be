#!/usr/bin/env python3
"""The GMM half of the C API (capi_gmm.hip, capi_feat.hip, capi_models.hip) on every branch of its host-side dispatch, as BITS and
as LAUNCH COUNTS.  A sibling of tools/bitwise_fixture_em.py and tools/bitwise_fixture_tv.py, with the same two modes:
  tools/bitwise_fixture_gmm_capi.py write out.json    compute with the library capi loads (GMMIV_LIB_PATH selects another build), store digests
  tools/bitwise_fixture_gmm_capi.py check ref.json    compute again and compare digests and launch counts, key by key
tests/golden/em_readers_bitwise.json pins the stored-likelihood readers at boundary shapes and r05_bitwise.json the default top-C path
at the workload's shape; this one pins the rest of the dispatch, at the smallest shapes at which each branch exists:
gmmiv_llk_determine_top fused (topDistribsCount 1 / 10 / 16, PARTIAL / COMPLETE, 1 / 255 / 257 / 1000 frames, with and without the
optional outputs, several fused chunks), fused with exact ties, with redone frames, redone whole, through the stored likelihoods (one chunk and two),
the direct kernel, the any-shape kernel (topDistribsCount 65, vectSize 81, 4800 Gaussians); gmmiv_topgauss_compute; gmmiv_feat_map on
a frame with an unusable value; gmmiv_tv_stats cut into pieces and not, over several chunks of whole utterances, with an utterance
longer than a chunk, at vectSize 81, and per ndx line; gmmiv_em_accumulate / _occ / _llk / _llk_use_top_multi on their second paths;
the four *_models calls with chunks bounded by frames and by models, on the per-segment walk (a long segment, vectSize 81, stats_z 0),
and gmmiv_feat_compensate_models into a host output with padding columns between untouched frames, in place on the device and with a
shared offset.
Next to the digests, the launch counts that kernel_launches reports after each call under "timing" 1 (which launch of a call restarts a
kernel's timer is host-side bookkeeping that no result depends on).
tests/golden/gmm_capi_bitwise.json was written by the library before capi_gmm.hip was split into capi_ctx.hip, capi_gmm.hip and
capi_feat.hip and before the per-chunk likelihood stage of capi_models.hip got its one function (tests/test_gpu_gmm_capi_bitwise.py)."""
import ctypes as ct
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

N_KEYS = 322  # what compute() returns; tests/test_gpu_gmm_capi_bitwise.py asserts that the golden has them all
KERNELS = ("k_llk_mfma", "k_gmm_pack", "k_stats_z", "k_stats_mfma", "k_feat_comp", "k_topc_rank", "k_topc_from_z", "k_topc_determine",
           "k_posteriors")
TOP_FIELDS = ("idx", "lk", "nontop_lk", "nontop_llk", "nontop_w", "llk")


def compute():
    """-> (arrays, launches): launches[call] = {kernel: count} as the context reports them right after the call (and the frames that
    a gmmiv_llk_determine_top call handed to its slower paths, "topc_fallbacks")"""
    import torch
    from conftest import make_frames, make_gmm
    from lia_ral_amd import capi
    out, launches = {}, {}
    ctx = capi.Context(0)
    ctx.set_option("timing", 1)

    class options:  # set for a block, put back after it
        def __init__(self, **kv):
            self.kv = kv

        def __enter__(self):
            self.prev = {k: ctx.set_option(k, v) for k, v in self.kv.items()}

        def __exit__(self, *exc):
            for k, v in self.prev.items():
                ctx.set_option(k, v)

    def counted(tag):
        assert tag not in launches, tag
        launches[tag] = {k: int(ctx.kernel_launches(k)) for k in KERNELS}

    def top(tag, g, x, ctop, complete=True, optional=True):
        """gmmiv_llk_determine_top with every output, or (optional=False) with idx and llk alone; + the fallback count of the call"""
        T = x.shape[0]
        idx, llk = np.empty((T, ctop), np.int32), np.empty(T)
        rest = [np.empty((T, ctop)), np.empty(T), np.empty(T), np.empty(T)] if optional else [None] * 4
        ctx.set_option("topc_fallbacks", 0)
        capi._chk(capi.lib.gmmiv_llk_determine_top(ctx._h, g._h, capi._ptr(x), capi.F32, ct.c_int64(T), ct.c_int64(x.shape[1]), ctop,
                                                   1 if complete else 0, ct.c_double(-200.0), ct.c_double(200.0), capi._ptr(idx), *(capi._ptr(a) for a in rest),
                                                   capi._ptr(llk)))
        counted("top_" + tag)
        launches["top_" + tag]["topc_fallbacks"] = int(ctx.set_option("topc_fallbacks", 0))
        for f, v in zip(TOP_FIELDS, [idx] + rest + [llk]):
            if v is not None:
                out["top_%s_%s" % (f, tag)] = v

    # ---- gmmiv_llk_determine_top ---------------------------------------------------------------------------------------------------
    wA = make_gmm(129, 60, seed=129)
    gA = ctx.gmm(*wA)
    xA = make_frames(*wA, 6007, seed=6007)
    wB = make_gmm(64, 13, seed=64)
    gB = ctx.gmm(*wB)
    xB = make_frames(*wB, 1000, seed=1013)
    for ctop in (1, 10, 16):        # the fused path
        for complete in (True, False):
            for T in (1, 255, 257, 1000):
                top("fused_c%d_%s_%d" % (ctop, "complete" if complete else "partial", T), gA, xA[:T], ctop, complete)
    top("fused_D13_c10_257", gB, xB[:257], 10)
    for T in (1, 257):
        top("fused_bare_c10_%d" % T, gA, xA[:T], 10, optional=False)
    with options(z_scratch_mb=2):   # fused chunks of 256 frames
        top("fused_chunks_c10_1000", gA, xA[:1000], 10)
        top("fused_chunks_bare_c16_1000", gA, xA[:1000], 16, complete=False, optional=False)
    # three pairs of identical Gaussians: exact ties inside the selection, resolved by k_topc_rank itself
    w, mean, iv = make_gmm(512, 60, seed=31, spread=0.5)
    for a, b in ((7, 300), (8, 9), (100, 511)):
        mean[b] = mean[a]; iv[b] = iv[a]; w[b] = w[a]
    w /= w.sum()
    g = ctx.gmm(w, mean, iv)
    top("fused_ties_c10_4000", g, make_frames(w, mean, iv, 4000, seed=32), 10)
    g.close()
    # (redone frames: 35 of the 1000 above at topDistribsCount 16, in the first chunk and in later ones)
    # 100 identical Gaussians: more than 64 logits tie at the threshold of the frames drawn from them; 509 of 700 frames fail, more than
    # n / 8 + 64, so the call is redone whole -- through the stored likelihoods, which flag it on to the direct kernel
    w, mean, iv = make_gmm(256, 60, seed=21)
    mean[100:200] = mean[100]; iv[100:200] = iv[100]; w[100:200] = w[100]; w /= w.sum()
    g = ctx.gmm(w, mean, iv)
    top("fused_whole_c10_700", g, make_frames(w, mean, iv, 700, seed=22), 10)
    g.close()
    # ... with most of the weight on them (968 of 1000 frames fail)
    w, mean, iv = make_gmm(128, 60, seed=33)
    mean[28:] = mean[28]; iv[28:] = iv[28]; w[:] = 1.0 / 128
    g = ctx.gmm(w, mean, iv)
    top("fused_whole_c10_1000", g, make_frames(w, mean, iv, 1000, seed=34), 10)
    g.close()
    top("z_c20_1000", gA, xA[:1000], 20)                     # no fused path beyond 16: the stored likelihoods
    top("z_bare_c20_257", gA, xA[:257], 20, optional=False)
    with options(topc_fused=0, z_scratch_mb=8):               # ... in two chunks (5248 frames + the rest)
        top("z_chunks_c10_6007", gA, xA, 10)
    with options(topc_z=0):                                   # the direct kernel
        top("direct_c20_1000", gA, xA[:1000], 20)
        with options(topc_fused=0):
            top("direct_c10_partial_257", gA, xA[:257], 10, complete=False)
    top("big_c65_257", gA, xA[:257], 65)                      # the any-shape kernel: by topDistribsCount,
    w81 = make_gmm(64, 81, seed=81)
    g81 = ctx.gmm(*w81)
    x81 = make_frames(*w81, 300, seed=381)
    top("D81_c10_300", g81, x81, 10)                          # (vectSize 81: no MFMA instantiation)
    wide = make_gmm(4800, 2, seed=48)
    g = ctx.gmm(*wide)
    top("C4800_c10_257", g, make_frames(*wide, 257, seed=482), 10)  # and by logit rows that exceed LDS
    g.close()

    # ---- gmmiv_topgauss_compute: a fixed count, a fraction of the likelihood -------------------------------------------------------
    for tag, cap, top_gauss in (("fixed5", 10, 5.0), ("mass", 16, 0.9)):
        T = 1000
        idx, count, snsw, snsl, llk, ncap = np.empty((T, cap), np.int32), np.empty(T, np.int32), np.empty(T), np.empty(T), np.empty(T), ct.c_int64()
        capi._chk(capi.lib.gmmiv_topgauss_compute(ctx._h, gA._h, capi._ptr(xA), capi.F32, ct.c_int64(T), ct.c_int64(60), cap, ct.c_double(top_gauss), 1,
                                                  ct.c_double(-200.0), ct.c_double(200.0), capi._ptr(idx), capi._ptr(count), capi._ptr(snsw), capi._ptr(snsl),
                                                  capi._ptr(llk), ct.byref(ncap)))
        counted("topgauss_" + tag)
        for f, v in (("idx", idx), ("count", count), ("snsw", snsw), ("snsl", snsl), ("llk", llk), ("n_capped", np.array([ncap.value], np.int64))):
            out["topgauss_%s_%s" % (f, tag)] = v

    # ---- gmmiv_feat_map: the top-1 selection on a zeroed index array, 37 Gaussians (padded to 48), one frame with an unusable value ---
    w37 = make_gmm(37, 13, seed=37)
    g = ctx.gmm(*w37)
    x = make_frames(*w37, 300, seed=337)
    x[17, 3] = np.nan
    rng = np.random.default_rng(38)
    ci_mean, ci_cov = rng.normal(size=(37, 13)), rng.uniform(0.5, 2.0, (37, 13))
    out["featmap_out"], out["featmap_best"] = g.feat_map(w37[1], 1.0 / w37[2], ci_mean, ci_cov, x)
    counted("featmap")
    g.close()

    # ---- gmmiv_tv_stats ---------------------------------------------------------------------------------------------------------------
    def tv(tag, g, x, ub):
        out["tv_N_" + tag], out["tv_F_" + tag] = g.tv_stats(x, ub)
        counted("tv_" + tag)

    ub = [0, 1000, 1000, 1700, 3000]
    tv("split", gA, xA[:3000], ub)                            # one chunk of at most 16 utterances, cut into pieces
    with options(tv_stats_split=0):
        tv("nosplit", gA, xA[:3000], ub)
    lens = np.random.default_rng(100).integers(10, 80, 200)  # about 100 utterances fit a chunk: cut to 64
    lens[37] = 0
    ub200 = np.concatenate([[3], 3 + np.cumsum(lens)])
    xB2 = make_frames(*wB, int(ub200[-1]) + 5, seed=100)
    assert xB2.shape[0] >= 6000
    with options(z_scratch_mb=3):                             # 4864-frame chunks at 64 Gaussians
        tv("chunks_200utt", gB, xB2, ub200)
        tv("long_utt", gB, xB2[:6000], [0, 5000, 6000])       # an utterance longer than the chunk: k_stats_mfma
    tv("D81", g81, x81, [0, 100, 100, 300])
    out["tvlines_N"], out["tvlines_F"] = gA.tv_stats_lines(xA[:3000], ub, [[0, 1], [1], [3, 0]])
    counted("tvlines")

    # ---- the other single-model calls -----------------------------------------------------------------------------------------------
    with options(stats_z=0):
        out["em_nostatsz_1000"] = gA.em_accumulate(xA[:1000])
        counted("em_nostatsz_1000")
        out["em_nostatsz_6007"] = gA.em_accumulate(xA, weight=0.37)
        counted("em_nostatsz_6007")
    out["em_D81"] = g81.em_accumulate(x81)
    counted("em_D81")
    with options(topc_z=0):
        out["occ_notopcz"] = gA.occ(xA[:257])
        counted("occ_notopcz")
    sums = np.array([1.5, 2.0])
    out["llk"] = gA.llk(xA[:1000], sums=sums)
    out["llk_sums"] = sums
    counted("llk")
    clients = [ctx.gmm(*make_gmm(129, 60, seed=200 + i)) for i in range(3)]
    d = gA.llk_determine_top(xA[:1000], 10)
    out["usetop_multi"] = capi.Gmm.llk_use_top_multi(clients, xA[:1000], d["idx"], d["nontop_llk"])
    counted("usetop_multi")
    with options(topc_use_lanes=1):
        out["usetop_multi_lanes1"] = capi.Gmm.llk_use_top_multi(clients, xA[:1000], d["idx"], d["nontop_llk"])
        counted("usetop_multi_lanes1")
    for g in clients:
        g.close()

    # ---- the four *_models calls ---------------------------------------------------------------------------------------------------
    def models(tag, b, x, sb, sm, offsets):
        llk, seg_sum = b.llk(x, sb, sm)
        counted("models_llk_" + tag)
        out["models_llk_" + tag], out["models_llk_seg_sum_" + tag] = llk, seg_sum
        for f, v in zip(("N", "F", "seg_llk"), b.tv_stats(x, sb, sm)):
            out["models_tv_%s_%s" % (f, tag)] = v
        counted("models_tv_" + tag)
        for f, v in zip(("N", "F", "S", "seg_llk"), b.em_stats(x, sb, sm)):
            out["models_em_%s_%s" % (f, tag)] = v
        counted("models_em_" + tag)
        # a host output with three padding columns, between frames of no segment: the whole matrix, the untouched bytes with it
        whole = np.full((x.shape[0], x.shape[1] + 3), 7.0, np.float32)
        b.feat_compensate(x, sb, sm, offsets, out=whole[:, :x.shape[1]])
        counted("models_featcomp_" + tag)
        out["models_featcomp_" + tag] = whole

    G, C, D = 3, 129, 60
    ms = [make_gmm(C, D, seed=40 + m) for m in range(G)]
    b = ctx.gmm_batch(G, C, D).load(*(np.stack([m[i] for m in ms]) for i in range(3)))
    offs = np.random.default_rng(5).standard_normal((G, C, D))
    x = make_frames(*ms[0], 1400, seed=1400)
    # a first segment that starts inside a 16-frame block, an empty segment, a model used twice
    sb, sm = [5, 305, 305, 322, 700, 1100, 1390], [0, 2, 2, 1, 0, 1]
    models("default", b, x, sb, sm, offs)
    with options(z_scratch_mb=1):                             # chunks bounded by frames (512)
        models("by_frames", b, x, sb, sm, offs)
        models("walk_long_segment", b, x, [5, 305, 305, 322, 1322], [0, 2, 2, 1], offs)  # a segment longer than the chunk
    with options(models_scratch_mb=0):                        # chunks bounded by models (one per chunk)
        models("by_models", b, x, sb, sm, offs)
    with options(stats_z=0):
        models("walk_nostatsz", b, x, sb, sm, offs)
    # in place on the device; a shared offset
    xd = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    b.feat_compensate(xd, sb, sm, offs, out=xd)
    counted("models_featcomp_inplace")
    ctx.sync()
    out["models_featcomp_inplace"] = xd.cpu().numpy()
    xd = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    with options(z_scratch_mb=1):                             # ... across chunk boundaries inside a 16-frame block
        b.feat_compensate(xd, sb, sm, offs, out=xd)
    counted("models_featcomp_inplace_by_frames")
    ctx.sync()
    out["models_featcomp_inplace_by_frames"] = xd.cpu().numpy()
    out["models_featcomp_shared_offset"] = b.feat_compensate(x, sb, sm, offs[1])
    counted("models_featcomp_shared_offset")
    with options(z_scratch_mb=1):
        out["models_featcomp_shared_offset_by_frames"] = b.feat_compensate(x, sb, sm, offs[1], out_dtype=capi.F64)
        counted("models_featcomp_shared_offset_by_frames")
    b.close()
    ms = [make_gmm(64, 81, seed=90 + m) for m in range(2)]
    b = ctx.gmm_batch(2, 64, 81).load(*(np.stack([m[i] for m in ms]) for i in range(3)))
    models("walk_D81", b, x81, [5, 100, 100, 290], [1, 0, 1], np.random.default_rng(6).standard_normal((2, 64, 81)))
    b.close()
    ctx.close()
    return {k: np.ascontiguousarray(v) for k, v in out.items()}, launches


def digests(arrs):
    import hashlib
    return {k: {"sha256": hashlib.sha256(v.tobytes()).hexdigest(), "shape": list(v.shape), "dtype": str(v.dtype)} for k, v in arrs.items()}


if __name__ == "__main__":
    import json
    mode, path = sys.argv[1], sys.argv[2]
    arrs, launches = compute()
    got = digests(arrs)
    if mode == "write":
        json.dump({"arrays": got, "launches": launches}, open(path, "w"), indent=0, sort_keys=True)
        print("wrote the digests of %d arrays and the launch counts of %d calls to %s" % (len(got), len(launches), path))
    else:
        ref = json.load(open(path))
        bad = [k for k in ref["arrays"] if got.get(k) != ref["arrays"][k]] + [k for k in got if k not in ref["arrays"]]
        bad += ["launches of " + k for k in ref["launches"] if launches.get(k) != ref["launches"][k]] + ["launches of " + k for k in launches if k not in ref["launches"]]
        print("%d arrays, %d calls, %d differ: %s" % (len(ref["arrays"]), len(ref["launches"]), len(bad), bad[:20]))
        sys.exit(1 if bad else 0)
