// capi_host.cpp -- flat C entry points over liatools_gpu (used by the Python tests / tools; a C++
// caller includes liatools_gpu.h directly).  Every function returns 0 or -1 (+ liagpu_last_error()),
// mirroring the reference tools' "catch, print, carry on" drivers.
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include <memory>

#include "liatools_gpu.h"
#include "io.h"

using namespace liagpu;

static thread_local std::string g_err;
#define GUARD(...)                                          \
    try { __VA_ARGS__; return 0; }                              \
    catch (const std::exception &e) { g_err = e.what(); return -1; }

static SegCluster make_cluster(const long *begin, const long *len, long n)
{
    SegCluster c(n);
    for (long i = 0; i < n; ++i) { c[i].begin = (unsigned long)begin[i]; c[i].length = (unsigned long)len[i]; c[i].source = 0; }
    return c;
}
static MixtureGD make_mixture(int C, int D, const double *w, const double *mean, const double *cov)
{
    MixtureGD m(C, D);
    m.weights().assign(w, w + C);
    m.means().assign(mean, mean + (size_t)C * D);
    m.covs().assign(cov, cov + (size_t)C * D);
    m.computeAll();
    return m;
}

extern "C" {

const char *liagpu_last_error(void) { return g_err.c_str(); }
int liagpu_train_world_timed(int device, const float *x, long T, int D, const long *seg_begin, const long *seg_len, long nseg,
                             int C, double *w, double *mean, double *cov, int nbTrainIt, double baggedFrameProbability,
                             double initVarFloor, double finalVarFloor, double initVarCeil, double finalVarCeil,
                             long initRand, double *global_mean_out, double *global_cov_out, double *llk_it_out, double *it_ms_out);
int liagpu_compute_test_timed(int device, const float *x, long T, int D, const long *seg_begin, const long *seg_len, long nseg,
                              int C, const double *w_world, const double *mean_world, const double *cov_world, int nClients,
                              const double *w_cl, const double *mean_cl, const double *cov_cl, int topDistribsCount,
                              int complete, double minLLK, double maxLLK, int segmentalMode, double *llr_out, int reps, double *ms_out);
int liagpu_iv_extract_timed(int device, const float *x, long T, int D, const long *utt_begin, long U, int C, const double *w,
                            const double *mean, const double *cov, int R, const double *Tmat, double *W_out, double *N_out,
                            double *F_out, int reps, double *ms_out);

// TrainWorld: computeMeanCov -> trainModelStream (TrainWorld.cpp:101-191 minus file I/O and mixtureInit)
int liagpu_train_world(int device, const float *x, long T, int D, const long *seg_begin, const long *seg_len, long nseg,
                       int C, double *w, double *mean, double *cov, int nbTrainIt, double baggedFrameProbability,
                       double initVarFloor, double finalVarFloor, double initVarCeil, double finalVarCeil,
                       long initRand, double *global_mean_out, double *global_cov_out, double *llk_it_out)
{
    return liagpu_train_world_timed(device, x, T, D, seg_begin, seg_len, nseg, C, w, mean, cov, nbTrainIt, baggedFrameProbability, initVarFloor,
                                    finalVarFloor, initVarCeil, finalVarCeil, initRand, global_mean_out, global_cov_out, llk_it_out, nullptr);
}

// the same, with the wall time of every iteration in it_ms_out[nbTrainIt] (nullable): what bench.py's host_layer block reports
int liagpu_train_world_timed(int device, const float *x, long T, int D, const long *seg_begin, const long *seg_len, long nseg,
                             int C, double *w, double *mean, double *cov, int nbTrainIt, double baggedFrameProbability,
                             double initVarFloor, double finalVarFloor, double initVarCeil, double finalVarCeil,
                             long initRand, double *global_mean_out, double *global_cov_out, double *llk_it_out, double *it_ms_out)
{
    GUARD({
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        SegCluster segs = make_cluster(seg_begin, seg_len, nseg);
        std::vector<double> gm, gc;
        std::vector<double> itMs;
        computeMeanCov(fs, segs, gm, gc);
        if (global_mean_out) memcpy(global_mean_out, gm.data(), D * sizeof(double));
        if (global_cov_out) memcpy(global_cov_out, gc.data(), D * sizeof(double));
        MixtureGD world = make_mixture(C, D, w, mean, cov);
        TrainCfg cfg;
        cfg.nbTrainIt = nbTrainIt; cfg.baggedFrameProbability = baggedFrameProbability;
        cfg.initVarianceFlooring = initVarFloor; cfg.finalVarianceFlooring = finalVarFloor;
        cfg.initVarianceCeiling = initVarCeil; cfg.finalVarianceCeiling = finalVarCeil;
        cfg.initRand = (unsigned long)initRand;
        if (it_ms_out) cfg.iterationMs = &itMs;
        std::vector<double> llk = trainModelStream(cfg, fs, segs, gc, world);
        memcpy(w, world.weights().data(), C * sizeof(double));
        memcpy(mean, world.means().data(), (size_t)C * D * sizeof(double));
        memcpy(cov, world.covs().data(), (size_t)C * D * sizeof(double));
        if (llk_it_out) memcpy(llk_it_out, llk.data(), llk.size() * sizeof(double));
        if (it_ms_out) memcpy(it_ms_out, itMs.data(), itMs.size() * sizeof(double));
    })
}

// TrainWorld (TrainWorld.cpp:101-191) with NO initial model ("World model init from scratch", :175-178): global mean / covariance
// (or use01: 0 / 1, :158-169), mixtureInit with C components, trainModelStream.  w / mean / cov [C], [C x D], [C x D] are outputs only.
int liagpu_train_world_scratch(int device, const float *x, long T, int D, const long *seg_begin, const long *seg_len, long nseg,
                               int C, double nbFrameToSelect, int use01, double *w, double *mean, double *cov, int nbTrainIt,
                               double baggedFrameProbability, double initVarFloor, double finalVarFloor, double initVarCeil,
                               double finalVarCeil, long initRand, double *global_cov_out, double *llk_it_out)
{
    GUARD({
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        SegCluster segs = make_cluster(seg_begin, seg_len, nseg);
        std::vector<double> gm(D, 0.0), gc(D, 1.0);                    // initialize01
        if (!use01) computeMeanCov(fs, segs, gm, gc);
        if (global_cov_out) memcpy(global_cov_out, gc.data(), D * sizeof(double));
        MixtureGD world((unsigned long)C, (unsigned long)D);
        MixtureInitCfg icfg;
        icfg.nbFrameToSelect = nbFrameToSelect;
        mixtureInit(fs, segs, 1.0, world, gc, icfg);
        TrainCfg cfg;
        cfg.nbTrainIt = nbTrainIt; cfg.baggedFrameProbability = baggedFrameProbability;
        cfg.initVarianceFlooring = initVarFloor; cfg.finalVarianceFlooring = finalVarFloor;
        cfg.initVarianceCeiling = initVarCeil; cfg.finalVarianceCeiling = finalVarCeil;
        cfg.initRand = (unsigned long)initRand;
        std::vector<double> llk = trainModelStream(cfg, fs, segs, gc, world);
        memcpy(w, world.weights().data(), C * sizeof(double));
        memcpy(mean, world.means().data(), (size_t)C * D * sizeof(double));
        memcpy(cov, world.covs().data(), (size_t)C * D * sizeof(double));
        if (llk_it_out) memcpy(llk_it_out, llk.data(), llk.size() * sizeof(double));
    })
}

// TrainWorld over nStream input streams ("inputStreamList" / "weightStreamList", TrainWorld.cpp:123-137): computeMeanCov over all
// streams, trainModelStream(fsTab, segTab, weightTab) with componentReduction / normalizeModel.  weight == NULL: 1 / nStream.
// opts[5] = {componentReduction, targetMixtureDistribCount, normalizeModel, normalizeModelMeanOnly, normalizeModelNbIt}.
// w / mean / cov hold the C initial components on entry and the *C_out final ones (<= C) on return.
int liagpu_train_world_streams(int device, int nStream, const float *const *x, const long *T, int D, const long *const *seg_begin,
                               const long *const *seg_len, const long *nseg, const double *weight, int C, double *w, double *mean,
                               double *cov, int nbTrainIt, double baggedFrameProbability, double initVarFloor, double finalVarFloor,
                               double initVarCeil, double finalVarCeil, long initRand, const long *opts, long *C_out,
                               double *global_mean_out, double *global_cov_out, double *llk_it_out)
{
    GUARD({
        if (nStream <= 0) throw Exception("TrainWorld error:no input stream");
        GpuServer srv(device);
        std::vector<std::unique_ptr<FeatureBuffer> > fsTab;
        std::vector<SegCluster> segTab(nStream);
        std::vector<TrainStream> streams(nStream);
        for (int i = 0; i < nStream; ++i) {
            fsTab.emplace_back(new FeatureBuffer(srv, x[i], (unsigned long)T[i], (unsigned long)D));
            segTab[i] = make_cluster(seg_begin[i], seg_len[i], nseg[i]);
        }
        for (int i = 0; i < nStream; ++i) {
            streams[i].fs = fsTab[i].get(); streams[i].segs = &segTab[i];
            streams[i].weight = weight ? weight[i] : 1.0 / (double)nStream;
        }
        std::vector<double> gm, gc;
        computeMeanCov(streams, gm, gc);
        if (global_mean_out) memcpy(global_mean_out, gm.data(), D * sizeof(double));
        if (global_cov_out) memcpy(global_cov_out, gc.data(), D * sizeof(double));
        MixtureGD world = make_mixture(C, D, w, mean, cov);
        TrainCfg cfg;
        cfg.nbTrainIt = nbTrainIt; cfg.baggedFrameProbability = baggedFrameProbability;
        cfg.initVarianceFlooring = initVarFloor; cfg.finalVarianceFlooring = finalVarFloor;
        cfg.initVarianceCeiling = initVarCeil; cfg.finalVarianceCeiling = finalVarCeil;
        cfg.initRand = (unsigned long)initRand;
        if (opts) {
            cfg.componentReduction = opts[0] != 0; cfg.targetDistribCount = (unsigned long)opts[1];
            cfg.normalizeModel = opts[2] != 0; cfg.normalizeModelMeanOnly = opts[3] != 0; cfg.normalizeModelNbIt = (unsigned long)opts[4];
        }
        std::vector<double> llk = trainModelStream(cfg, streams, gc, world);
        const unsigned long Co = world.getDistribCount();
        if (C_out) *C_out = (long)Co;
        memcpy(w, world.weights().data(), Co * sizeof(double));
        memcpy(mean, world.means().data(), (size_t)Co * D * sizeof(double));
        memcpy(cov, world.covs().data(), (size_t)Co * D * sizeof(double));
        if (llk_it_out) memcpy(llk_it_out, llk.data(), llk.size() * sizeof(double));
    })
}

// mixtureInit over nStream input streams (TrainTools.cpp:674-766, the call of TrainWorld.cpp:177): w / mean / cov [C], [C x D], [C x D] out;
// counts [C] (nullable) = frames picked per component over all streams.  weight == NULL: 1 / nStream.
int liagpu_mixture_init_streams(int device, int nStream, const float *const *x, const long *T, int D, const long *const *seg_begin,
                                const long *const *seg_len, const long *nseg, const double *weight, int C, const double *global_cov,
                                double nbFrameToSelect, long minLen, long maxLen, double *w, double *mean, double *cov, long *counts)
{
    GUARD({
        if (nStream <= 0) throw Exception("mixtureInit: no input stream");
        GpuServer srv(device);
        std::vector<std::unique_ptr<FeatureBuffer> > fsTab;
        std::vector<SegCluster> segTab(nStream);
        std::vector<TrainStream> streams(nStream);
        for (int i = 0; i < nStream; ++i) {
            fsTab.emplace_back(new FeatureBuffer(srv, x[i], (unsigned long)T[i], (unsigned long)D));
            segTab[i] = make_cluster(seg_begin[i], seg_len[i], nseg[i]);
        }
        for (int i = 0; i < nStream; ++i) {
            streams[i].fs = fsTab[i].get(); streams[i].segs = &segTab[i];
            streams[i].weight = weight ? weight[i] : 1.0 / (double)nStream;
        }
        MixtureGD world((unsigned long)C, (unsigned long)D);
        MixtureInitCfg cfg;
        cfg.nbFrameToSelect = nbFrameToSelect; cfg.baggedMinimalLength = (unsigned long)minLen; cfg.baggedMaximalLength = (unsigned long)maxLen;
        std::vector<unsigned long> cnt;
        mixtureInit(streams, world, std::vector<double>(global_cov, global_cov + D), cfg, &cnt);
        memcpy(w, world.weights().data(), C * sizeof(double));
        memcpy(mean, world.means().data(), (size_t)C * D * sizeof(double));
        memcpy(cov, world.covs().data(), (size_t)C * D * sizeof(double));
        if (counts) for (int c = 0; c < C; ++c) counts[c] = (long)cnt[c];
    })
}

// meanLikelihood over several feature servers (GeneralTools.cpp:599-607), optionally weighted by one decision value per server (:610-624)
int liagpu_mean_llk_streams(int device, int nStream, const float *const *x, const long *T, int D, const long *const *seg_begin,
                            const long *const *seg_len, const long *nseg, const double *decision, int C, const double *w, const double *mean,
                            const double *cov, double minLLK, double maxLLK, double *out)
{
    GUARD({
        GpuServer srv(device);
        std::vector<std::unique_ptr<FeatureBuffer> > fsTab;
        std::vector<SegCluster> segTab(nStream);
        std::vector<TrainStream> streams(nStream);
        for (int i = 0; i < nStream; ++i) {
            fsTab.emplace_back(new FeatureBuffer(srv, x[i], (unsigned long)T[i], (unsigned long)D));
            segTab[i] = make_cluster(seg_begin[i], seg_len[i], nseg[i]);
        }
        for (int i = 0; i < nStream; ++i) { streams[i].fs = fsTab[i].get(); streams[i].segs = &segTab[i]; }
        MixtureGD model = make_mixture(C, D, w, mean, cov);
        DeviceMixture dm(srv, model);
        *out = decision ? meanLikelihood(streams, dm, std::vector<double>(decision, decision + nStream), minLLK, maxLLK)
                        : meanLikelihood(streams, dm, minLLK, maxLLK);
    })
}

// selectComponent(nbTop) + reduceModel + normalizeWeights, then (optionally) normalizeMixture to N(0, 1): the model edits of
// TrainTools.cpp:1078-1098 on their own (host arithmetic only -- no device is touched)
int liagpu_model_reduce_normalize(int C, int D, double *w, double *mean, double *cov, long nbTop, int normalize, int meanOnly, long nbIt,
                                  long *order_out)
{
    GUARD({
        MixtureGD m = make_mixture(C, D, w, mean, cov);
        if (order_out) {
            const std::vector<unsigned long> o = sortByWeight(m);
            for (int i = 0; i < C; ++i) order_out[i] = (long)o[i];
        }
        if (nbTop > 0 && nbTop < C) {
            std::vector<bool> sel;
            const unsigned long n = selectComponent(sel, (unsigned long)nbTop, m);
            MixtureGD out(n, (unsigned long)D);
            (void)reduceModel(sel, m, out);
            normalizeWeights(out);
            m = out;
        }
        if (normalize) normalizeMixture(m, std::vector<double>(), std::vector<double>(), true, (unsigned long)nbIt, meanOnly != 0);
        const unsigned long Co = m.getDistribCount();
        memcpy(w, m.weights().data(), Co * sizeof(double));
        memcpy(mean, m.means().data(), (size_t)Co * D * sizeof(double));
        memcpy(cov, m.covs().data(), (size_t)Co * D * sizeof(double));
    })
}

// mixtureInit (TrainTools.cpp:674-766 multi-stream form with one stream when single_stream == 0, :619-672 when 1): the
// start-from-scratch model of TrainWorld.  param = nbFrameToSelect (multi) or baggedFrameProbabilityInit (single).
// w / mean / cov [C], [C x D], [C x D] out; counts [C] (nullable) = frames picked per component.
int liagpu_mixture_init(int device, const float *x, long T, int D, const long *seg_begin, const long *seg_len, long nseg, int C,
                        int single_stream, double param, double stream_weight, long min_len, long max_len, const double *global_cov,
                        double *w, double *mean, double *cov, long *counts)
{
    GUARD({
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        SegCluster segs = make_cluster(seg_begin, seg_len, nseg);
        MixtureGD world((unsigned long)C, (unsigned long)D);
        MixtureInitCfg cfg;
        cfg.baggedMinimalLength = (unsigned long)min_len; cfg.baggedMaximalLength = (unsigned long)max_len;
        std::vector<unsigned long> cnt;
        const std::vector<double> gc(global_cov, global_cov + D);
        if (single_stream) { cfg.baggedFrameProbabilityInit = param; mixtureInitSingleStream(fs, world, segs, gc, cfg, &cnt); }
        else { cfg.nbFrameToSelect = param; mixtureInit(fs, segs, stream_weight, world, gc, cfg, &cnt); }
        memcpy(w, world.weights().data(), C * sizeof(double));
        memcpy(mean, world.means().data(), (size_t)C * D * sizeof(double));
        memcpy(cov, world.covs().data(), (size_t)C * D * sizeof(double));
        if (counts) for (int k = 0; k < C; ++k) counts[k] = (long)cnt[k];
    })
}

// TVAcc::verifyEMLK (AccumulateTVStat.cpp:1654-1688) on given i-vectors: file f = frames [file_begin[f], file_begin[f+1]) of x,
// its speaker model = UBM with means m + T^T W[row_of_file[f]]; llk_out [nfiles] = getLLK per file, *total = their sum.
// supervectors_out (nullable) [nfiles x C*D] = getMplusTW of each file's row.
int liagpu_tv_verify_emlk(int device, const float *x, long T, int D, const long *file_begin, long nfiles, const long *row_of_file, int C,
                          const double *w, const double *mean, const double *cov, int R, const double *Tmat, long U, const double *W,
                          long max_llk_computed, double minLLK, double maxLLK, double *llk_out, double *total, double *supervectors_out)
{
    GUARD({
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        TVAcc tv(srv, make_mixture(C, D, w, mean, cov), (unsigned long)R, (unsigned long)U);
        tv.loadT(std::vector<double>(Tmat, Tmat + (size_t)R * C * D));
        memcpy(tv.getW().data(), W, (size_t)U * R * sizeof(double));
        std::vector<SegCluster> segs(nfiles);
        std::vector<unsigned long> rows(nfiles);
        for (long f = 0; f < nfiles; ++f) {
            Seg s; s.begin = (unsigned long)file_begin[f]; s.length = (unsigned long)(file_begin[f + 1] - file_begin[f]);
            segs[f].push_back(s);
            rows[f] = (unsigned long)row_of_file[f];
        }
        std::vector<double> per;
        *total = tv.verifyEMLK(fs, segs, rows, (unsigned long)max_llk_computed, minLLK, maxLLK, &per);
        for (size_t f = 0; f < per.size(); ++f) llk_out[f] = per[f];
        if (supervectors_out) {
            std::vector<double> Sp;
            tv.getMplusTW(Sp, rows);
            memcpy(supervectors_out, Sp.data(), Sp.size() * sizeof(double));
        }
    })
}

// accumulateStatLLK over a cluster (AccumulateStat.cpp:69-94): getMeanLLK of the selected frames, clamped per frame
int liagpu_mean_llk(int device, const float *x, long T, int D, const long *seg_begin, const long *seg_len, long nseg, int C,
                    const double *w, const double *mean, const double *cov, double minLLK, double maxLLK, double *out)
{
    GUARD({
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        DeviceMixture dm(srv, make_mixture(C, D, w, mean, cov));
        *out = accumulateStatLLK(fs, dm, make_cluster(seg_begin, seg_len, nseg), minLLK, maxLLK);
    })
}

// TrainTarget (TrainTarget.cpp:73-278 minus file I/O): client = MAP-adapt(world) on the selected frames
int liagpu_train_target(int device, const float *x, long T, int D, const long *seg_begin, const long *seg_len, long nseg,
                        int C, const double *w, const double *mean, const double *cov, int nbTrainIt, double meanReg,
                        double *w_out, double *mean_out, double *cov_out)
{
    GUARD({
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        SegCluster segs = make_cluster(seg_begin, seg_len, nseg);
        MixtureGD world = make_mixture(C, D, w, mean, cov);
        MixtureGD client = world;
        MAPCfg cfg;
        cfg.nbTrainIt = nbTrainIt; cfg.meanReg = meanReg;
        adaptModel(fs, segs, world, client, cfg);
        memcpy(w_out, client.weights().data(), C * sizeof(double));
        memcpy(mean_out, client.means().data(), (size_t)C * D * sizeof(double));
        memcpy(cov_out, client.covs().data(), (size_t)C * D * sizeof(double));
    })
}

static MAPCfg make_map_cfg(const char *method, int nbTrainIt, double baggedP, int flags, const double *reg, double alphaMean, const long *norm)
{
    MAPCfg cfg;
    cfg.method = method ? method : "MAPOccDep";
    cfg.nbTrainIt = (unsigned long)nbTrainIt; cfg.baggedFrameProbability = baggedP;
    cfg.meanAdapt = (flags & 1) != 0; cfg.varAdapt = (flags & 2) != 0; cfg.weightAdapt = (flags & 4) != 0;
    cfg.batchVariances = (flags & 8) != 0; // adaptModelBatch only
    if (reg) { cfg.meanReg = reg[0]; cfg.varReg = reg[1]; cfg.weightReg = reg[2]; }
    cfg.meanAlpha = alphaMean;
    if (norm) { cfg.normalizeModel = norm[0] != 0; cfg.normalizeModelMeanOnly = norm[1] != 0; cfg.normalizeModelNbIt = (unsigned long)norm[2]; }
    return cfg;
}

// TrainTarget with every MAPCfg parameter (TrainTools.cpp:95-147): method = MAPAlgo, flags bit 0 / 1 / 2 = meanAdapt / varAdapt /
// weightAdapt (bit 3, batched calls only: MAPCfg::batchVariances), reg[3] = MAPRegFactorMean / Var / Weight, alphaMean = MAPAlphaMean, norm[3] = normalizeModel, MeanOnly, NbIt (nullable)
int liagpu_train_target_ex(int device, const float *x, long T, int D, const long *seg_begin, const long *seg_len, long nseg, int C,
                           const double *w, const double *mean, const double *cov, const char *method, int nbTrainIt, double baggedP,
                           int flags, const double *reg, double alphaMean, const long *norm, double *w_out, double *mean_out, double *cov_out)
{
    GUARD({
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        SegCluster segs = make_cluster(seg_begin, seg_len, nseg);
        MixtureGD world = make_mixture(C, D, w, mean, cov);
        MixtureGD client = world;
        adaptModel(fs, segs, world, client, make_map_cfg(method, nbTrainIt, baggedP, flags, reg, alphaMean, norm));
        memcpy(w_out, client.weights().data(), C * sizeof(double));
        memcpy(mean_out, client.means().data(), (size_t)C * D * sizeof(double));
        memcpy(cov_out, client.covs().data(), (size_t)C * D * sizeof(double));
    })
}

// TrainTarget for MANY clients in one call (adaptModelBatch): client i owns the segments [client_begin[i], client_begin[i + 1]) of the
// seg_begin / seg_len lists and starts from the world model; w_out [nclients x C], mean_out / cov_out [nclients x C * D]
// liagpu_train_target_batch_w: the same with mllr_out (nullable) [nclients x D x (D+1)] = the last iteration's MLLR transform of every
// client (method "MLLR"; left untouched for the other methods)
int liagpu_train_target_batch_w(int device, const float *x, long T, int D, const long *client_begin, long nclients, const long *seg_begin,
                                const long *seg_len, int C, const double *w, const double *mean, const double *cov, const char *method, int nbTrainIt,
                                double baggedP, int flags, const double *reg, double alphaMean, const long *norm, double *w_out, double *mean_out,
                                double *cov_out, double *mllr_out);
int liagpu_train_target_batch(int device, const float *x, long T, int D, const long *client_begin, long nclients, const long *seg_begin,
                              const long *seg_len, int C, const double *w, const double *mean, const double *cov, const char *method, int nbTrainIt,
                              double baggedP, int flags, const double *reg, double alphaMean, const long *norm, double *w_out, double *mean_out,
                              double *cov_out)
{
    return liagpu_train_target_batch_w(device, x, T, D, client_begin, nclients, seg_begin, seg_len, C, w, mean, cov, method, nbTrainIt, baggedP, flags, reg,
                                       alphaMean, norm, w_out, mean_out, cov_out, nullptr);
}
int liagpu_train_target_batch_w(int device, const float *x, long T, int D, const long *client_begin, long nclients, const long *seg_begin,
                                const long *seg_len, int C, const double *w, const double *mean, const double *cov, const char *method, int nbTrainIt,
                                double baggedP, int flags, const double *reg, double alphaMean, const long *norm, double *w_out, double *mean_out,
                                double *cov_out, double *mllr_out)
{
    GUARD({
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        MixtureGD world = make_mixture(C, D, w, mean, cov);
        std::vector<SegCluster> sel;
        for (long i = 0; i < nclients; ++i) sel.push_back(make_cluster(seg_begin + client_begin[i], seg_len + client_begin[i], client_begin[i + 1] - client_begin[i]));
        std::vector<MixtureGD> clients((size_t)nclients, world);
        std::vector<MatrixD> Wm;
        adaptModelBatch(fs, sel, world, clients, make_map_cfg(method, nbTrainIt, baggedP, flags, reg, alphaMean, norm), mllr_out ? &Wm : nullptr);
        for (size_t i = 0; i < Wm.size(); ++i)
            if (!Wm[i].v.empty()) memcpy(mllr_out + i * (size_t)D * (D + 1), Wm[i].v.data(), Wm[i].v.size() * sizeof(double));
        for (long i = 0; i < nclients; ++i) {
            memcpy(w_out + (size_t)i * C, clients[i].weights().data(), C * sizeof(double));
            memcpy(mean_out + (size_t)i * C * D, clients[i].means().data(), (size_t)C * D * sizeof(double));
            memcpy(cov_out + (size_t)i * C * D, clients[i].covs().data(), (size_t)C * D * sizeof(double));
        }
    })
}

// tools/bench_enroll.py: enrolment of nclients clients of frames_per_client frames each (client i = frames [i n, (i + 1) n)) from the world
// model, timed on the host around the whole adaptation (features resident, the stream drained before and after): which = 0
// adaptModelBatch, 1 = adaptModel client after client.  ms_out[reps]: every repetition (the caller drops warm-ups); after them one more pass
// with the context's kernel timers on: kernel_ms[0..2] = k_llk_mfma, k_stats_z, k_gmm_pack of the LAST call of that pass (-1: not run).
// warm_clients > 0: only that many clients in the first repetition.  mean0_out (nullable): the adapted means of client 0.
// liagpu_bench_enroll_method (tools/bench_mllr.py): the same with the MAPAlgo given (NULL: "MAPOccDep"); kernel_ms[5] then also holds
// [3] = k_mllr_solve, [4] = k_mllr_pack of the last call
int liagpu_bench_enroll_method(int device, const float *x, long T, int D, long nclients, long frames_per_client, int C, const double *w, const double *mean,
                               const double *cov, const char *method, int nbTrainIt, int which, int reps, long warm_clients, double *ms_out,
                               double *kernel_ms, double *mean0_out);
int liagpu_bench_enroll(int device, const float *x, long T, int D, long nclients, long frames_per_client, int C, const double *w, const double *mean,
                        const double *cov, int nbTrainIt, int which, int reps, long warm_clients, double *ms_out, double *kernel_ms, double *mean0_out)
{
    double km[5];
    const int rc = liagpu_bench_enroll_method(device, x, T, D, nclients, frames_per_client, C, w, mean, cov, nullptr, nbTrainIt, which, reps, warm_clients, ms_out,
                                              km, mean0_out);
    if (!rc) memcpy(kernel_ms, km, 3 * sizeof(double));
    return rc;
}
// liagpu_bench_enroll_flags (tools/bench_enroll_var.py): the same with the MAPCfg flags of liagpu_train_target_ex (bit 1 varAdapt, bit 3
// batchVariances, ...); cov0_out (nullable): the adapted variances of client 0
int liagpu_bench_enroll_flags(int device, const float *x, long T, int D, long nclients, long frames_per_client, int C, const double *w, const double *mean,
                              const double *cov, const char *method, int nbTrainIt, int flags, int which, int reps, long warm_clients, double *ms_out,
                              double *kernel_ms, double *mean0_out, double *cov0_out);
int liagpu_bench_enroll_method(int device, const float *x, long T, int D, long nclients, long frames_per_client, int C, const double *w, const double *mean,
                               const double *cov, const char *method, int nbTrainIt, int which, int reps, long warm_clients, double *ms_out,
                               double *kernel_ms, double *mean0_out)
{
    return liagpu_bench_enroll_flags(device, x, T, D, nclients, frames_per_client, C, w, mean, cov, method, nbTrainIt, 1, which, reps, warm_clients, ms_out,
                                     kernel_ms, mean0_out, nullptr);
}
int liagpu_bench_enroll_flags(int device, const float *x, long T, int D, long nclients, long frames_per_client, int C, const double *w, const double *mean,
                              const double *cov, const char *method, int nbTrainIt, int flags, int which, int reps, long warm_clients, double *ms_out,
                              double *kernel_ms, double *mean0_out, double *cov0_out)
{
    GUARD({
        if (nclients * frames_per_client > T) throw Exception("bench_enroll: not enough frames");
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        MixtureGD world = make_mixture(C, D, w, mean, cov);
        std::vector<SegCluster> sel((size_t)nclients);
        for (long i = 0; i < nclients; ++i) {
            Seg s;
            s.begin = (unsigned long)(i * frames_per_client); s.length = (unsigned long)frames_per_client;
            sel[(size_t)i].push_back(s);
        }
        MAPCfg cfg;
        cfg.nbTrainIt = (unsigned long)nbTrainIt;
        if (method) cfg.method = method;
        cfg.meanAdapt = (flags & 1) != 0; cfg.varAdapt = (flags & 2) != 0; cfg.weightAdapt = (flags & 4) != 0; cfg.batchVariances = (flags & 8) != 0;
        std::vector<MixtureGD> clients;
        auto run = [&](long n) {
            clients.assign((size_t)n, world);
            if (which == 0) {
                std::vector<SegCluster> part(sel.begin(), sel.begin() + n);
                adaptModelBatch(fs, part, world, clients, cfg);
            } else {
                for (long i = 0; i < n; ++i) adaptModel(fs, sel[(size_t)i], world, clients[(size_t)i], cfg);
            }
            srv.sync();
        };
        for (int r = 0; r < reps; ++r) {
            srv.sync();
            const auto t0 = std::chrono::steady_clock::now();
            run(r == 0 && warm_clients > 0 && warm_clients < nclients ? warm_clients : nclients);
            ms_out[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        (void)gmmiv_ctx_set_option(srv.ctx(), "timing", 1);
        run(nclients);
        kernel_ms[0] = gmmiv_ctx_kernel_ms(srv.ctx(), "k_llk_mfma");
        kernel_ms[1] = gmmiv_ctx_kernel_ms(srv.ctx(), "k_stats_z");
        kernel_ms[2] = gmmiv_ctx_kernel_ms(srv.ctx(), "k_gmm_pack");
        kernel_ms[3] = gmmiv_ctx_kernel_ms(srv.ctx(), "k_mllr_solve");
        kernel_ms[4] = gmmiv_ctx_kernel_ms(srv.ctx(), "k_mllr_pack");
        (void)gmmiv_ctx_set_option(srv.ctx(), "timing", 0);
        if (mean0_out) memcpy(mean0_out, clients[0].means().data(), (size_t)C * D * sizeof(double));
        if (cov0_out) memcpy(cov0_out, clients[0].covs().data(), (size_t)C * D * sizeof(double));
    })
}

// computeMAP on its own (TrainTools.cpp:543-556; host arithmetic only -- no device is touched): w / mean / cov = the ML estimate in, the
// adapted model out
int liagpu_compute_map(int C, int D, const double *w0, const double *mean0, const double *cov0, double *w, double *mean, double *cov,
                       double frameCount, const char *method, int flags, const double *reg, double alphaMean)
{
    GUARD({
        MixtureGD init = make_mixture(C, D, w0, mean0, cov0), client = make_mixture(C, D, w, mean, cov);
        computeMAP(init, client, (unsigned long)frameCount, make_map_cfg(method, 1, 1.0, flags, reg, alphaMean, nullptr));
        memcpy(w, client.weights().data(), C * sizeof(double));
        memcpy(mean, client.means().data(), (size_t)C * D * sizeof(double));
        memcpy(cov, client.covs().data(), (size_t)C * D * sizeof(double));
    })
}

// computeMLLR on its own (TrainTools.cpp:788-866; host arithmetic only -- no device is touched): w / mean = the ML estimate in (cov is not
// read), the adapted model out (weights and variances of the init model, covInv_out (nullable) = what computeAll() made of them);
// W_out [D x (D+1)]
int liagpu_compute_mllr(int C, int D, const double *w0, const double *mean0, const double *cov0, double *w, double *mean, double *cov,
                        double *covinv_out, double frameCount, double *W_out)
{
    GUARD({
        MixtureGD init = make_mixture(C, D, w0, mean0, cov0), client = make_mixture(C, D, w, mean, cov0);
        const MatrixD W = computeMLLR(init, client, (unsigned long)frameCount);
        memcpy(W_out, W.v.data(), W.v.size() * sizeof(double));
        memcpy(w, client.weights().data(), C * sizeof(double));
        memcpy(mean, client.means().data(), (size_t)C * D * sizeof(double));
        memcpy(cov, client.covs().data(), (size_t)C * D * sizeof(double));
        if (covinv_out) memcpy(covinv_out, client.covInvs().data(), (size_t)C * D * sizeof(double));
    })
}

// TopGauss (TopGauss.cpp): compute on the selected frames, write the nbGaussian file, read it back into a fresh object, get() on
// it with `ubm` and (when given) a second model.  out[0] = compute's mean llk, out[1] = get(ubm), out[2] = get(model2),
// out[3] = frames capped; counts_out[T] / snsw_out[T] / snsl_out[T] (nullable) = what was stored; *nbgcnt_out = total entries.
int liagpu_topgauss(int device, const float *x, long T, int D, const long *seg_begin, const long *seg_len, long nseg, int C,
                    const double *w, const double *mean, const double *cov, const double *mean2, double topGauss, int topDistribsCount,
                    int complete, double minLLK, double maxLLK, const char *path, double *out, long *counts_out, long *idx_out,
                    double *snsw_out, double *snsl_out, long *nbgcnt_out)
{
    GUARD({
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        SegCluster segs = make_cluster(seg_begin, seg_len, nseg);
        MixtureGD ubm = make_mixture(C, D, w, mean, cov);
        DeviceMixture dubm(srv, ubm);
        TopGauss tg;
        out[0] = tg.compute(dubm, fs, segs, topGauss, topDistribsCount, complete != 0, minLLK, maxLLK);
        out[3] = (double)tg.nbCapped();
        tg.write(path);
        TopGauss back;
        back.read(path);
        if (back.nt() != tg.nt() || back.nbgcnt() != tg.nbgcnt() || back.nbg() != tg.nbg() || back.idx() != tg.idx() || back.snsw() != tg.snsw() ||
            back.snsl() != tg.snsl())
            throw Exception("TopGauss: the file does not read back as written");
        out[1] = back.get(dubm, fs, segs, complete != 0, minLLK, maxLLK);
        out[2] = 0.0;
        if (mean2) {
            MixtureGD m2 = make_mixture(C, D, w, mean2, cov);
            DeviceMixture d2(srv, m2);
            out[2] = back.get(d2, fs, segs, complete != 0, minLLK, maxLLK);
        }
        if (nbgcnt_out) *nbgcnt_out = (long)back.nbgcnt();
        for (unsigned long t = 0; t < back.nt(); ++t) {
            if (counts_out) counts_out[t] = (long)back.nbg()[t];
            if (snsw_out) snsw_out[t] = back.snsw()[t];
            if (snsl_out) snsl_out[t] = back.snsl()[t];
        }
        if (idx_out) for (unsigned long i = 0; i < back.nbgcnt(); ++i) idx_out[i] = (long)back.idx()[i];
    })
}

// ComputeTest for one test file: world + nClients models (same C, D), covariances given as covInv
int liagpu_compute_test(int device, const float *x, long T, int D, const long *seg_begin, const long *seg_len, long nseg,
                        int C, const double *w_world, const double *mean_world, const double *cov_world, int nClients,
                        const double *w_cl, const double *mean_cl, const double *cov_cl, int topDistribsCount,
                        int complete, double minLLK, double maxLLK, int segmentalMode, double *llr_out)
{
    return liagpu_compute_test_timed(device, x, T, D, seg_begin, seg_len, nseg, C, w_world, mean_world, cov_world, nClients, w_cl, mean_cl, cov_cl,
                                     topDistribsCount, complete, minLLK, maxLLK, segmentalMode, llr_out, 1, nullptr);
}

// the same, computeTestLLR run `reps` times on the resident features and models: ms_out[reps] = wall time of each run (bench.py host_layer)
int liagpu_compute_test_timed(int device, const float *x, long T, int D, const long *seg_begin, const long *seg_len, long nseg,
                              int C, const double *w_world, const double *mean_world, const double *cov_world, int nClients,
                              const double *w_cl, const double *mean_cl, const double *cov_cl, int topDistribsCount,
                              int complete, double minLLK, double maxLLK, int segmentalMode, double *llr_out, int reps, double *ms_out)
{
    GUARD({
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        SegCluster segs = make_cluster(seg_begin, seg_len, nseg);
        MixtureGD world = make_mixture(C, D, w_world, mean_world, cov_world);
        DeviceMixture dworld(srv, world);
        std::vector<DeviceMixture *> cl;
        const size_t CD = (size_t)C * D;
        for (int i = 0; i < nClients; ++i)
            cl.push_back(new DeviceMixture(srv, make_mixture(C, D, w_cl + (size_t)i * C, mean_cl + i * CD, cov_cl + i * CD)));
        std::vector<double> out;
        try {
            for (int r = 0; r < (reps > 0 ? reps : 1); ++r) {
                srv.sync();
                const auto t0 = std::chrono::steady_clock::now();
                out = computeTestLLR(fs, segs, dworld, cl, topDistribsCount, complete != 0, minLLK, maxLLK, segmentalMode != 0);
                srv.sync();
                if (ms_out) ms_out[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            }
        }
        catch (...) { for (auto p : cl) delete p; throw; }
        for (auto p : cl) delete p;
        memcpy(llr_out, out.data(), out.size() * sizeof(double));
    })
}

// ComputeTest with worldDecime and the WindowLLR mode (ComputeTest.cpp:154-207, UnsupervisedTools.cpp:70-145).
// win_out receives up to max_win rows [idxBegin, idxEnd, llr(client 0..nClients-1)]; *n_win = rows produced.
int liagpu_compute_test_ex(int device, const float *x, long T, int D, const long *seg_begin, const long *seg_len, long nseg, int C,
                           const double *w_world, const double *mean_world, const double *cov_world, int nClients, const double *w_cl,
                           const double *mean_cl, const double *cov_cl, int topDistribsCount, int complete, double minLLK, double maxLLK,
                           int segmentalMode, long worldDecime, long windowSize, long windowDec, double *llr_out, double *win_out,
                           long max_win, long *n_win)
{
    GUARD({
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        SegCluster segs = make_cluster(seg_begin, seg_len, nseg);
        MixtureGD world = make_mixture(C, D, w_world, mean_world, cov_world);
        DeviceMixture dworld(srv, world);
        std::vector<DeviceMixture *> cl;
        const size_t CD = (size_t)C * D;
        for (int i = 0; i < nClients; ++i)
            cl.push_back(new DeviceMixture(srv, make_mixture(C, D, w_cl + (size_t)i * C, mean_cl + i * CD, cov_cl + i * CD)));
        std::vector<double> out;
        std::vector<WindowOut> wins;
        try {
            out = computeTestLLR(fs, segs, dworld, cl, topDistribsCount, complete != 0, minLLK, maxLLK, segmentalMode != 0,
                                 (unsigned long)worldDecime, (unsigned long)windowSize, (unsigned long)windowDec, &wins);
        } catch (...) { for (auto p : cl) delete p; throw; }
        for (auto p : cl) delete p;
        memcpy(llr_out, out.data(), out.size() * sizeof(double));
        long nw = 0;
        for (const WindowOut &o : wins) {
            if (nw >= max_win) break;
            double *row = win_out + (size_t)nw * (2 + nClients);
            row[0] = (double)o.idxBegin; row[1] = (double)o.idxEnd;
            for (int i = 0; i < nClients; ++i) row[2 + i] = o.llr[i];
            ++nw;
        }
        if (n_win) *n_win = (long)wins.size();
    })
}

// IvExtractor (IvExtractor.cpp:70-148): stats -> substractM -> estimateTETt -> estimateW
int liagpu_iv_extract(int device, const float *x, long T, int D, const long *utt_begin, long U, int C, const double *w,
                      const double *mean, const double *cov, int R, const double *Tmat, double *W_out, double *N_out,
                      double *F_out)
{
    return liagpu_iv_extract_timed(device, x, T, D, utt_begin, U, C, w, mean, cov, R, Tmat, W_out, N_out, F_out, 1, nullptr);
}

// the same, the extraction run `reps` times on the resident features: ms_out[reps x 4] = wall time of computeAndAccumulateTVStat,
// substractM, estimateTETt (first run only: T does not change during extraction, IvExtractor.cpp:136) and estimateW (bench.py host_layer)
int liagpu_iv_extract_timed(int device, const float *x, long T, int D, const long *utt_begin, long U, int C, const double *w,
                            const double *mean, const double *cov, int R, const double *Tmat, double *W_out, double *N_out,
                            double *F_out, int reps, double *ms_out)
{
    GUARD({
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        MixtureGD ubm = make_mixture(C, D, w, mean, cov);
        TVAcc tv(srv, ubm, (unsigned long)R, (unsigned long)U);
        std::vector<SegCluster> lines(U);
        for (long u = 0; u < U; ++u) {
            Seg s; s.begin = (unsigned long)utt_begin[u]; s.length = (unsigned long)(utt_begin[u + 1] - utt_begin[u]); s.source = 0;
            if (s.length) lines[u].push_back(s);
        }
        tv.loadT(std::vector<double>(Tmat, Tmat + (size_t)R * C * D));
        auto lap = [&](std::chrono::steady_clock::time_point &t0) {
            srv.sync();
            const auto t1 = std::chrono::steady_clock::now();
            const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
            t0 = t1;
            return ms;
        };
        for (int r = 0; r < (reps > 0 ? reps : 1); ++r) {
            double ms[4] = {0.0, 0.0, 0.0, 0.0};
            srv.sync();
            auto t0 = std::chrono::steady_clock::now();
            tv.computeAndAccumulateTVStat(fs, lines);
            ms[0] = lap(t0);
            if (r == 0) {
                if (N_out) memcpy(N_out, tv.getN().data(), tv.getN().size() * sizeof(double));
                if (F_out) memcpy(F_out, tv.getF().data(), tv.getF().size() * sizeof(double));
                t0 = std::chrono::steady_clock::now();
            }
            tv.substractM();
            ms[1] = lap(t0);
            if (r == 0) { tv.estimateTETt(); ms[2] = lap(t0); }
            tv.estimateW();
            ms[3] = lap(t0);
            if (ms_out) memcpy(ms_out + 4 * r, ms, sizeof(ms));
        }
        memcpy(W_out, tv.getW().data(), tv.getW().size() * sizeof(double));
    })
}

// IvExtractorUbmWeigth / IvExtractorEigenDecomposition (IvExtractor.cpp:150-250, 254-360): the approximate
// extractors.  mode 1 = ubmWeight, 2 = eigenDecomposition.  Q_out [R x R] / D_out [C x R] (mode 2) and Wcov_out
// [R x R] receive the intermediate matrices when given.
int liagpu_iv_extract_approx(int device, int mode, const float *x, long T, int D, const long *utt_begin, long U, int C, const double *w,
                             const double *mean, const double *cov, int R, const double *Tmat, double *W_out, double *Wcov_out,
                             double *Q_out, double *D_out)
{
    GUARD({
        if (mode != 1 && mode != 2) throw Exception("iv_extract_approx: mode must be 1 (ubmWeight) or 2 (eigenDecomposition)");
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        MixtureGD ubm = make_mixture(C, D, w, mean, cov);
        TVAcc tv(srv, ubm, (unsigned long)R, (unsigned long)U);
        std::vector<SegCluster> lines(U);
        for (long u = 0; u < U; ++u) {
            Seg s; s.begin = (unsigned long)utt_begin[u]; s.length = (unsigned long)(utt_begin[u + 1] - utt_begin[u]); s.source = 0;
            if (s.length) lines[u].push_back(s);
        }
        tv.loadT(std::vector<double>(Tmat, Tmat + (size_t)R * C * D));
        tv.normTMatrix();
        std::vector<double> Wc, Q, ev, Dm;
        tv.getWeightedCov(Wc, std::vector<double>(w, w + C));
        if (Wcov_out) memcpy(Wcov_out, Wc.data(), Wc.size() * sizeof(double));
        if (mode == 2) {
            computeEigenProblem(Wc, (unsigned long)R, Q, ev, (unsigned long)R);
            tv.approximateTcTc(Dm, Q);
            if (Q_out) memcpy(Q_out, Q.data(), Q.size() * sizeof(double));
            if (D_out) memcpy(D_out, Dm.data(), Dm.size() * sizeof(double));
        }
        tv.computeAndAccumulateTVStat(fs, lines);
        tv.normStatistics();
        if (mode == 1) tv.estimateWUbmWeight(Wc);
        else { std::fill(tv.getW().begin(), tv.getW().end(), 0.0); tv.estimateWEigenDecomposition(Dm, Q); }
        memcpy(W_out, tv.getW().data(), tv.getW().size() * sizeof(double));
    })
}

// PldaDev::sphericalNuisanceNormalization (PldaTools.cpp:1822-1929): EFR (sph_norm 0) / sphNorm (1) training on a
// development set X [dim x n] (normalised in place); mats [nb_it x dim x dim], means [nb_it x dim].  Optional
// outputs after the last iteration: the WCCN Cholesky factor, the Mahalanobis matrix and lda_rank LDA rows.
int liagpu_backend_train(int device, int dim, long n, double *X, long nspk, const long *sps, int sph_norm, int nb_it, double *mats,
                         double *means, double *wccn, double *mahalanobis, int lda_rank, double *lda)
{
    GUARD({
        GpuServer srv(device);
        PldaDev dev(srv, (unsigned long)dim, std::vector<double>(X, X + (size_t)dim * n), std::vector<unsigned long>(sps, sps + nspk));
        std::vector<std::vector<double> > M, mu;
        dev.sphericalNuisanceNormalization((unsigned long)nb_it, sph_norm != 0, M, mu);
        for (int it = 0; it < nb_it; ++it) {
            memcpy(mats + (size_t)it * dim * dim, M[it].data(), (size_t)dim * dim * sizeof(double));
            memcpy(means + (size_t)it * dim, mu[it].data(), (size_t)dim * sizeof(double));
        }
        memcpy(X, dev.getData().data(), (size_t)dim * n * sizeof(double));
        std::vector<double> t;
        if (wccn) { dev.computeWccnChol(t); memcpy(wccn, t.data(), t.size() * sizeof(double)); }
        if (mahalanobis) { dev.computeMahalanobis(t); memcpy(mahalanobis, t.data(), t.size() * sizeof(double)); }
        if (lda && lda_rank > 0) { dev.computeLDA(t, (unsigned long)lda_rank); memcpy(lda, t.data(), t.size() * sizeof(double)); }
    })
}

// PLDA training (LIA_SpkDet/PLDA/src/PLDA.cpp:80-95): nb_it EM iterations from given F, G, Sigma; X is left centred by
// the accumulated minimum-divergence shifts like the reference's _Dev.
int liagpu_plda_train(int device, int dim, long n, double *X, long nspk, const long *sps, int rf, int rg, int nb_it, double *F, double *G,
                      double *Sigma, double *Delta, double *original_mean)
{
    GUARD({
        GpuServer srv(device);
        PldaDev dev(srv, (unsigned long)dim, std::vector<double>(X, X + (size_t)dim * n), std::vector<unsigned long>(sps, sps + nspk));
        PldaModel plda(dev, (unsigned long)rf, (unsigned long)rg, std::vector<double>(F, F + (size_t)dim * rf),
                       std::vector<double>(G, G + (size_t)dim * rg), std::vector<double>(Sigma, Sigma + (size_t)dim * dim));
        for (int it = 0; it < nb_it; ++it) plda.em_iteration();
        memcpy(F, plda.getF().data(), plda.getF().size() * sizeof(double));
        memcpy(G, plda.getG().data(), plda.getG().size() * sizeof(double));
        memcpy(Sigma, plda.getSigma().data(), plda.getSigma().size() * sizeof(double));
        memcpy(Delta, plda.getDelta().data(), plda.getDelta().size() * sizeof(double));
        if (original_mean) memcpy(original_mean, plda.getOriginalMean().data(), (size_t)dim * sizeof(double));
        memcpy(X, dev.getData().data(), (size_t)dim * n * sizeof(double));
    })
}

// IvTest (IvTest.cpp:73-471).  scoring: 0 cosine, 1 mahalanobis, 2 2cov, 3 plda.  dev [dim x nDev] with sessions grouped by
// speaker; enrol [dim x nEnrol] grouped by model; test [dim x nTest]; scores [nModels x nTest].
// pldaScoring: 0 native, 1 enrollMean.  trialModel == NULL: the dense matrix [nModels x nTest]; else one score per listed trial.
static void iv_test_impl(int device, int dim, long nDev, const double *dev, long nspk, const long *sps, long nModels, const long *enrolPerModel,
                         const double *enrol, long nTest, const double *test, int ivNorm, int ivNormIt, int sphNorm, int lda, int ldaRank,
                         int wccn, int scoring, int rf, int rg, int pldaIt, const double *F, const double *G, const double *Sigma, int pldaScoring,
                         long ntrial, const int32_t *trialModel, const int32_t *trialSeg, double *scores)
{
    {
        static const char *names[] = {"cosine", "mahalanobis", "2cov", "plda"};
        if (scoring < 0 || scoring > 3) throw Exception("Scoring option is invalid, must be: cosine OR mahalanobis OR 2cov OR plda");
        GpuServer srv(device);
        PldaDev pd(srv, (unsigned long)dim, std::vector<double>(dev, dev + (size_t)dim * nDev), std::vector<unsigned long>(sps, sps + nspk));
        IvTestCfg cfg;
        cfg.ivNorm = ivNorm != 0; cfg.ivNormIterationNb = (unsigned long)ivNormIt; cfg.sphNorm = sphNorm != 0;
        cfg.LDA = lda != 0; cfg.ldaRank = (unsigned long)ldaRank; cfg.WCCN = wccn != 0; cfg.scoring = names[scoring];
        cfg.pldaRankF = (unsigned long)rf; cfg.pldaRankG = (unsigned long)rg; cfg.pldaNbIt = (unsigned long)pldaIt;
        if (pldaScoring != 0 && pldaScoring != 1) throw Exception("pldaScoring must be: native OR enrollMean");
        cfg.pldaScoring = pldaScoring ? "enrollMean" : "native";
        std::vector<unsigned long> epm(enrolPerModel, enrolPerModel + nModels);
        unsigned long nEnrol = 0;
        for (unsigned long e : epm) nEnrol += e;
        const unsigned long d2 = cfg.ivNorm && cfg.LDA ? 0 : 0; (void)d2;
        std::vector<double> f, g, s;
        if (scoring == 3) {
            // the PLDA matrices live in the space AFTER normalisation / LDA: their leading dimension is that space's
            const unsigned long pd_dim = cfg.ivNorm && cfg.LDA ? cfg.ldaRank : (unsigned long)dim;
            f.assign(F, F + pd_dim * rf); g.assign(G, G + pd_dim * rg); s.assign(Sigma, Sigma + pd_dim * pd_dim);
        }
        std::vector<double> out;
        if (trialModel)
            out = ivTestTrials(srv, cfg, pd, std::vector<double>(enrol, enrol + (size_t)dim * nEnrol), epm, std::vector<double>(test, test + (size_t)dim * nTest),
                               (unsigned long)nTest, std::vector<int32_t>(trialModel, trialModel + ntrial), std::vector<int32_t>(trialSeg, trialSeg + ntrial), f, g, s);
        else
            out = ivTest(srv, cfg, pd, std::vector<double>(enrol, enrol + (size_t)dim * nEnrol), epm,
                         std::vector<double>(test, test + (size_t)dim * nTest), (unsigned long)nTest, f, g, s);
        memcpy(scores, out.data(), out.size() * sizeof(double));
    }
}
int liagpu_iv_test(int device, int dim, long nDev, const double *dev, long nspk, const long *sps, long nModels, const long *enrolPerModel,
                   const double *enrol, long nTest, const double *test, int ivNorm, int ivNormIt, int sphNorm, int lda, int ldaRank,
                   int wccn, int scoring, int rf, int rg, int pldaIt, const double *F, const double *G, const double *Sigma, double *scores)
{
    GUARD(iv_test_impl(device, dim, nDev, dev, nspk, sps, nModels, enrolPerModel, enrol, nTest, test, ivNorm, ivNormIt, sphNorm, lda, ldaRank, wccn,
                       scoring, rf, rg, pldaIt, F, G, Sigma, 0, 0, nullptr, nullptr, scores))
}
// IvTest on a list of trials (liagpu::ivTestTrials): trial i = (trialModel[i], trialSeg[i]), scores [ntrial] in list order.  pldaScoring:
// 0 native, 1 enrollMean.  trialModel == NULL runs the dense liagpu::ivTest with that pldaScoring: scores [nModels x nTest].
int liagpu_iv_test_trials(int device, int dim, long nDev, const double *dev, long nspk, const long *sps, long nModels, const long *enrolPerModel,
                          const double *enrol, long nTest, const double *test, int ivNorm, int ivNormIt, int sphNorm, int lda, int ldaRank,
                          int wccn, int scoring, int rf, int rg, int pldaIt, const double *F, const double *G, const double *Sigma, int pldaScoring,
                          long ntrial, const int32_t *trialModel, const int32_t *trialSeg, double *scores)
{
    GUARD({
        if (ntrial < 0 || (trialModel && !trialSeg)) throw Exception("liagpu_iv_test_trials: bad trial list");
        iv_test_impl(device, dim, nDev, dev, nspk, sps, nModels, enrolPerModel, enrol, nTest, test, ivNorm, ivNormIt, sphNorm, lda, ldaRank, wccn, scoring,
                     rf, rg, pldaIt, F, G, Sigma, pldaScoring, ntrial, trialModel, trialSeg, scores);
    })
}
// loadIvTestNdx (host only): the counts in dims = {models, segments, trials, dropped, enrolment sessions, maxSessions}; with text != NULL the
// tables as text (cap bytes): one line "M <id> <session> ..." per model, "S <id>" per segment, "T <model index> <segment index>" per trial
int liagpu_iv_test_ndx_load(const char *ndx, const char *targetIdList, long *dims, char *text, long cap)
{
    GUARD({
        const IvTestNdx nx = loadIvTestNdx(ndx, targetIdList ? targetIdList : "");
        size_t nsess = 0;
        for (const auto &v : nx.sessions) nsess += v.size();
        dims[0] = (long)nx.models.size(); dims[1] = (long)nx.segs.size(); dims[2] = (long)nx.trialModel.size(); dims[3] = (long)nx.dropped;
        dims[4] = (long)nsess; dims[5] = (long)nx.maxSessions;
        if (text) {
            std::ostringstream o;
            for (size_t m = 0; m < nx.models.size(); ++m) {
                o << "M " << nx.models[m];
                for (const std::string &e : nx.sessions[m]) o << " " << e;
                o << "\n";
            }
            for (const std::string &e : nx.segs) o << "S " << e << "\n";
            for (size_t i = 0; i < nx.trialModel.size(); ++i) o << "T " << nx.trialModel[i] << " " << nx.trialSeg[i] << "\n";
            const std::string t = o.str();
            if ((long)t.size() + 1 > cap) throw Exception("liagpu_iv_test_ndx_load: text buffer too small");
            memcpy(text, t.c_str(), t.size() + 1);
        }
    })
}
// IvTest from files on an ndx (liagpu::ivTestFiles): the development set as arrays, the enrolment and test vectors from
// <vector_path>/<id><vector_ext> (matrix format fmt), the result lines into out_path in the order of IvTest.cpp:430-437.  With
// line_model / line_seg / scores (cap entries each, nullable) the trial and the score of every line; *n_lines = their number.
int liagpu_iv_test_ndx(int device, int dim, long nDev, const double *dev, long nspk, const long *sps, const char *ndx, const char *targetIdList,
                       const char *vector_path, const char *vector_ext, const char *fmt, const char *out_path, const char *gender, double threshold,
                       int ivNorm, int ivNormIt, int sphNorm, int lda, int ldaRank, int wccn, int scoring, int rf, int rg, int pldaIt, const double *F,
                       const double *G, const double *Sigma, int pldaScoring, long cap, int32_t *line_model, int32_t *line_seg, double *scores,
                       long *n_lines)
{
    GUARD({
        static const char *names[] = {"cosine", "mahalanobis", "2cov", "plda"};
        if (scoring < 0 || scoring > 3) throw Exception("Scoring option is invalid, must be: cosine OR mahalanobis OR 2cov OR plda");
        if (pldaScoring != 0 && pldaScoring != 1) throw Exception("pldaScoring must be: native OR enrollMean");
        GpuServer srv(device);
        PldaDev pd(srv, (unsigned long)dim, std::vector<double>(dev, dev + (size_t)dim * nDev), std::vector<unsigned long>(sps, sps + nspk));
        IvTestFilesCfg cfg;
        cfg.test.ivNorm = ivNorm != 0; cfg.test.ivNormIterationNb = (unsigned long)ivNormIt; cfg.test.sphNorm = sphNorm != 0;
        cfg.test.LDA = lda != 0; cfg.test.ldaRank = (unsigned long)ldaRank; cfg.test.WCCN = wccn != 0; cfg.test.scoring = names[scoring];
        cfg.test.pldaRankF = (unsigned long)rf; cfg.test.pldaRankG = (unsigned long)rg; cfg.test.pldaNbIt = (unsigned long)pldaIt;
        cfg.test.pldaScoring = pldaScoring ? "enrollMean" : "native";
        cfg.ndxFilename = ndx; cfg.targetIdList = targetIdList ? targetIdList : ""; cfg.vectorFilesPath = vector_path; cfg.vectorFilesExtension = vector_ext;
        cfg.loadMatrixFormat = fmt; cfg.outputFilename = out_path ? out_path : ""; cfg.gender = gender ? gender : "M"; cfg.decisionThreshold = threshold;
        std::vector<double> f, g, s;
        if (scoring == 3) {
            const unsigned long pd_dim = cfg.test.ivNorm && cfg.test.LDA ? cfg.test.ldaRank : (unsigned long)dim;
            f.assign(F, F + pd_dim * rf); g.assign(G, G + pd_dim * rg); s.assign(Sigma, Sigma + pd_dim * pd_dim);
        }
        const IvTestFilesResult r = ivTestFiles(srv, cfg, pd, f, g, s);
        const long n = (long)r.scores.size();
        if (n_lines) *n_lines = n;
        if (line_model || line_seg || scores) {
            if (n > cap) throw Exception("liagpu_iv_test_ndx: output arrays too small");
            if (line_model) memcpy(line_model, r.lineModel.data(), (size_t)n * sizeof(int32_t));
            if (line_seg) memcpy(line_seg, r.lineSeg.data(), (size_t)n * sizeof(int32_t));
            if (scores) memcpy(scores, r.scores.data(), (size_t)n * sizeof(double));
        }
    })
}

// TotalVariability (TotalVariability.cpp:118-169): nbIt iterations on precomputed N, F
int liagpu_tv_train(int device, long U, int C, int D, const double *w, const double *mean, const double *cov, int R,
                    const double *N, const double *F, double *Tmat, int nbIt, int minDiv, double *mean_out)
{
    GUARD({
        GpuServer srv(device);
        MixtureGD ubm = make_mixture(C, D, w, mean, cov);
        TVAcc tv(srv, ubm, (unsigned long)R, (unsigned long)U);
        tv.loadT(std::vector<double>(Tmat, Tmat + (size_t)R * C * D));
        tv.setStats(N, F);         // one upload; everything below stays on the device until getT()
        tv.storeStats();
        for (int it = 0; it < nbIt; ++it) {
            if (it) tv.restoreStatsAndSubstractM(); // the reference reloads N and F from disk every iteration (:152-153) and centres
            else tv.substractM();                   // them in place: one device pass over F here
            tv.estimateTETt();
            tv.estimateAandC();
            tv.updateTestimate();
            if (minDiv) tv.minDivergence();
        }
        memcpy(Tmat, tv.getT().data(), tv.getT().size() * sizeof(double));
        if (mean_out) memcpy(mean_out, tv.getUbmMeans().data(), tv.getUbmMeans().size() * sizeof(double));
    })
}

// TVAcc::initT ("normal" law) for a UBM with the given inverse variances: seeds glibc with `seed` first (the reference never calls
// srand, i.e. seed 1) and fills Tmat [R x C*D]
int liagpu_tv_init_t(int device, int C, int D, const double *w, const double *mean, const double *cov, int R, unsigned seed, double *Tmat)
{
    GUARD({
        GpuServer srv(device);
        TVAcc tv(srv, make_mixture(C, D, w, mean, cov), (unsigned long)R, 1);
        srand(seed);
        tv.initT("normal");
        memcpy(Tmat, tv.getT().data(), (size_t)R * C * D * sizeof(double));
    })
}

// computeAndAccumulateTVStat with the file -> ndx-line map: file f = frames [file_begin[f], file_begin[f+1]) of x, line l lists the
// files line_files[line_off[l] .. line_off[l+1]); N [nlines x C], F [nlines x C*D]
int liagpu_tv_stats_lines(int device, const float *x, long T, int D, const long *file_begin, long nfiles, long nlines, const long *line_off,
                          const long *line_files, int C, const double *w, const double *mean, const double *cov, double *N, double *F)
{
    GUARD({
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        TVAcc tv(srv, make_mixture(C, D, w, mean, cov), 1, (unsigned long)nlines);
        std::vector<SegCluster> segs(nfiles);
        for (long f = 0; f < nfiles; ++f) { Seg s; s.begin = (unsigned long)file_begin[f]; s.length = (unsigned long)(file_begin[f + 1] - file_begin[f]); segs[f].push_back(s); }
        std::vector<std::vector<unsigned long> > lines(nlines);
        for (long l = 0; l < nlines; ++l)
            for (long p = line_off[l]; p < line_off[l + 1]; ++p) lines[l].push_back((unsigned long)line_files[p]);
        tv.computeAndAccumulateTVStat(fs, segs, lines);
        memcpy(N, tv.getN().data(), tv.getN().size() * sizeof(double));
        memcpy(F, tv.getF().data(), tv.getF().size() * sizeof(double));
    })
}

// One rank of a multi-GPU TotalVariability run (configs[3]: utterances sharded over the GPUs of a node, one process -- or host
// thread -- per GPU).  N, F: the statistics of THIS rank's U utterances; Tmat: the same initial matrix on every rank.  The
// ranks meet through `id_file` (rank 0 publishes the RCCL id there, gmmiv_comm_exchange_id_file); per iteration the only
// exchange is reduce-scatter(A, Cmx) / all-gather(T) / all-reduce(R, r, meanW) on device buffers (TVAcc::updateTestimate(comm)).
// U_total = utterances over all ranks (the session count of minDivergence).  times_ms (nullable, 4 x nbIt): wall-clock of
// estimateTETt / estimateAandC / updateTestimate (with its collectives) / minDivergence per iteration.
int liagpu_tv_train_dist2(int device, int world, int rank, const char *id_file, long U, long U_total, int C, int D, const double *w,
                          const double *mean, const double *cov, int R, const double *N, const double *F, double *Tmat, int nbIt,
                          int minDiv, int overlap, double *mean_out, double *times_ms);
int liagpu_tv_train_dist(int device, int world, int rank, const char *id_file, long U, long U_total, int C, int D, const double *w,
                         const double *mean, const double *cov, int R, const double *N, const double *F, double *Tmat, int nbIt,
                         int minDiv, double *mean_out, double *times_ms)
{
    return liagpu_tv_train_dist2(device, world, rank, id_file, U, U_total, C, D, w, mean, cov, R, N, F, Tmat, nbIt, minDiv, 0, mean_out, times_ms);
}
// the same with the exchange started early when overlap != 0 (TVAcc::setOverlap: the reduce-scatter of A from inside estimateAandC,
// the all-gather of T joined inside minDivergence); bitwise the results of overlap == 0
int liagpu_tv_train_dist2(int device, int world, int rank, const char *id_file, long U, long U_total, int C, int D, const double *w,
                          const double *mean, const double *cov, int R, const double *N, const double *F, double *Tmat, int nbIt,
                          int minDiv, int overlap, double *mean_out, double *times_ms)
{
    GUARD({
        GpuServer srv(device);
        gmmiv_comm *comm = nullptr;
        if (world > 1) {
            unsigned char id[GMMIV_COMM_ID_BYTES];
            srv.check(gmmiv_comm_exchange_id_file(id_file, rank, id, 300.0));
            srv.check(gmmiv_comm_create(srv.ctx(), world, rank, id, &comm));
        }
        struct CommGuard { gmmiv_comm *c; ~CommGuard() { gmmiv_comm_destroy(c); } } guard{comm};
        MixtureGD ubm = make_mixture(C, D, w, mean, cov);
        TVAcc tv(srv, ubm, (unsigned long)R, (unsigned long)U);
        tv.loadT(std::vector<double>(Tmat, Tmat + (size_t)R * C * D));
        tv.setStats(N, F);
        tv.storeStats();
        if (overlap) tv.setOverlap(comm);
        auto now = [&]() { srv.check(gmmiv_ctx_sync(srv.ctx())); return std::chrono::steady_clock::now(); };
        auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        for (int it = 0; it < nbIt; ++it) {
            if (it) tv.restoreStatsAndSubstractM();
            else tv.substractM();
            auto t0 = now();
            tv.estimateTETt();
            auto t1 = now();
            tv.estimateAandC();
            auto t2 = now();
            tv.updateTestimate(comm, (unsigned long)U_total);
            auto t3 = now();
            if (minDiv) tv.minDivergence();
            else tv.finishT();
            auto t4 = now();
            if (times_ms) { times_ms[4 * it] = ms(t0, t1); times_ms[4 * it + 1] = ms(t1, t2); times_ms[4 * it + 2] = ms(t2, t3); times_ms[4 * it + 3] = ms(t3, t4); }
        }
        memcpy(Tmat, tv.getT().data(), tv.getT().size() * sizeof(double));
        if (mean_out) memcpy(mean_out, tv.getUbmMeans().data(), tv.getUbmMeans().size() * sizeof(double));
    })
}

// One rank of a multi-GPU TrainWorld run: x = this rank's frames, global_cov = the variance-control reference (replicated);
// per iteration ONE gmmiv_allreduce_f64 of the flat EM accumulator on the device (trainModelStream(..., comm)).
int liagpu_train_world_dist(int device, int world, int rank, const char *id_file, const float *x, long T, int D, const long *seg_begin,
                            const long *seg_len, long nseg, int C, double *w, double *mean, double *cov, int nbTrainIt,
                            double initVarFloor, double finalVarFloor, double initVarCeil, double finalVarCeil, const double *global_cov,
                            double *llk_it_out)
{
    GUARD({
        GpuServer srv(device);
        gmmiv_comm *comm = nullptr;
        unsigned char id[GMMIV_COMM_ID_BYTES] = {0};
        if (world > 1) srv.check(gmmiv_comm_exchange_id_file(id_file, rank, id, 300.0));
        srv.check(gmmiv_comm_create(srv.ctx(), world, rank, id, &comm));
        struct CommGuard { gmmiv_comm *c; ~CommGuard() { gmmiv_comm_destroy(c); } } guard{comm};
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        SegCluster segs = make_cluster(seg_begin, seg_len, nseg);
        MixtureGD model = make_mixture(C, D, w, mean, cov);
        TrainCfg cfg;
        cfg.nbTrainIt = nbTrainIt;
        cfg.initVarianceFlooring = initVarFloor; cfg.finalVarianceFlooring = finalVarFloor;
        cfg.initVarianceCeiling = initVarCeil; cfg.finalVarianceCeiling = finalVarCeil;
        std::vector<double> llk = trainModelStream(cfg, fs, segs, std::vector<double>(global_cov, global_cov + D), model, comm);
        memcpy(w, model.weights().data(), C * sizeof(double));
        memcpy(mean, model.means().data(), (size_t)C * D * sizeof(double));
        memcpy(cov, model.covs().data(), (size_t)C * D * sizeof(double));
        if (llk_it_out) memcpy(llk_it_out, llk.data(), llk.size() * sizeof(double));
    })
}

// EigenVoice / EigenChannel / EstimateDMatrix on given statistics (task 0 / 1 / 2; EigenVoice.cpp:71-160,
// EigenChannel.cpp:71-165, EstimateDMatrix.cpp:103-210 minus the file I/O).  V, U, Dm: initial matrices in, trained out
// (only the task's own matrix changes); Y, X, Z: the factors of the last estimate (outputs, may be NULL).
int liagpu_jfa_train(int device, int task, long nspk, const long *sessPerSpk, int C, int D, const double *w, const double *mean,
                     const double *cov, int rankEV, int rankEC, const double *N, const double *N_h, const double *F_X, const double *F_X_h,
                     double *V, double *U, double *Dm, const double *Z0, int nbIt, int orthoV, double *Y, double *X, double *Z)
{
    GUARD({
        GpuServer srv(device);
        MixtureGD ubm = make_mixture(C, D, w, mean, cov);
        std::vector<unsigned long> sps(sessPerSpk, sessPerSpk + nspk);
        JFAAcc jfa(srv, ubm, (unsigned long)rankEV, (unsigned long)rankEC, sps);
        const size_t SV = (size_t)C * D, nsess = jfa.getNSessions();
        jfa.setStats(std::vector<double>(N, N + (size_t)nspk * C), std::vector<double>(N_h, N_h + nsess * C),
                     std::vector<double>(F_X, F_X + (size_t)nspk * SV), std::vector<double>(F_X_h, F_X_h + nsess * SV));
        jfa.loadEV(std::vector<double>(V, V + (size_t)rankEV * SV));
        jfa.loadEC(std::vector<double>(U, U + (size_t)rankEC * SV));
        jfa.loadD(std::vector<double>(Dm, Dm + SV));
        if (Z0) jfa.getZ().assign(Z0, Z0 + (size_t)nspk * SV);
        if (task == 0) eigenVoice(jfa, (unsigned long)nbIt, orthoV != 0);
        else if (task == 1) eigenChannel(jfa, (unsigned long)nbIt);
        else if (task == 2) estimateDMatrix(jfa, (unsigned long)nbIt);
        else throw Exception("liagpu_jfa_train: task must be 0 (EigenVoice), 1 (EigenChannel) or 2 (EstimateDMatrix)");
        memcpy(V, jfa.getV().data(), jfa.getV().size() * sizeof(double));
        memcpy(U, jfa.getU().data(), jfa.getU().size() * sizeof(double));
        memcpy(Dm, jfa.getD().data(), SV * sizeof(double));
        if (Y) memcpy(Y, jfa.getY().data(), jfa.getY().size() * sizeof(double));
        if (X) memcpy(X, jfa.getX().data(), jfa.getX().size() * sizeof(double));
        if (Z) memcpy(Z, jfa.getZ().data(), jfa.getZ().size() * sizeof(double));
    })
}

// ComputeTest, JFA dot-product scoring (ComputeTest.cpp:303-358) for nTest segments given their statistics (N == N_h, F == F_h:
// one session each) and the client supervectors [nClients x SV]; scores [nTest x nClients]
int liagpu_jfa_dot_product(int device, long nTest, int C, int D, const double *w, const double *mean, const double *cov, int rankEV,
                           int rankEC, const double *N, const double *F, const double *V, const double *U, const double *Dm,
                           long nClients, const double *clientSV, double *scores)
{
    GUARD({
        GpuServer srv(device);
        MixtureGD ubm = make_mixture(C, D, w, mean, cov);
        std::vector<unsigned long> sps((size_t)nTest, 1ul);
        JFAAcc jfa(srv, ubm, (unsigned long)rankEV, (unsigned long)rankEC, sps);
        const size_t SV = (size_t)C * D;
        const std::vector<double> Nv(N, N + (size_t)nTest * C), Fv(F, F + (size_t)nTest * SV);
        jfa.setStats(Nv, Nv, Fv, Fv);
        jfa.loadEV(std::vector<double>(V, V + (size_t)rankEV * SV));
        jfa.loadEC(std::vector<double>(U, U + (size_t)rankEC * SV));
        jfa.loadD(std::vector<double>(Dm, Dm + SV));
        std::vector<double> sc = computeTestDotProduct(srv, jfa, std::vector<double>(clientSV, clientSV + (size_t)nClients * SV), (unsigned long)nClients);
        memcpy(scores, sc.data(), sc.size() * sizeof(double));
    })
}

// Baum-Welch statistics of a TVAcc that lives on ONE server from the frames of a FeatureBuffer that lives on ANOTHER (the
// reference hands any FeatureServer to any accumulator, AccumulateTVStat.cpp:281-351).  The accumulator's server also owns a clean
// buffer (x_own): the screening decision of the call must follow the buffer that is READ -- a dirty x there must not poison N / F.
// unusable_out[2] = unusable frames of (the accumulator's own buffer, the foreign buffer) as counted at upload.
int liagpu_tv_stats_cross_server(int device, const float *x_own, long T_own, const float *x, long T, int D, const long *utt_begin, long U,
                                 int C, const double *w, const double *mean, const double *cov, double *N_out, double *F_out,
                                 long *unusable_out, long *assume_finite_after)
{
    GUARD({
        GpuServer srvAcc(device), srvFeat(device);
        FeatureBuffer own(srvAcc, x_own, (unsigned long)T_own, (unsigned long)D);
        FeatureBuffer fs(srvFeat, x, (unsigned long)T, (unsigned long)D);
        MixtureGD ubm = make_mixture(C, D, w, mean, cov);
        TVAcc tv(srvAcc, ubm, 2, (unsigned long)U);
        std::vector<SegCluster> lines(U);
        for (long u = 0; u < U; ++u) {
            Seg s; s.begin = (unsigned long)utt_begin[u]; s.length = (unsigned long)(utt_begin[u + 1] - utt_begin[u]); s.source = 0;
            if (s.length) lines[u].push_back(s);
        }
        tv.computeAndAccumulateTVStat(fs, lines);
        memcpy(N_out, tv.getN().data(), tv.getN().size() * sizeof(double));
        memcpy(F_out, tv.getF().data(), tv.getF().size() * sizeof(double));
        if (unusable_out) { unusable_out[0] = (long)own.unusableFrames(); unusable_out[1] = (long)fs.unusableFrames(); }
        // the option is the user's again once the call has returned (it was 0 before: never set)
        if (assume_finite_after) *assume_finite_after = gmmiv_ctx_set_option(srvAcc.ctx(), "assume_finite", 0);
    })
}

// JFA statistics from frames (JFAAcc::computeAndAccumulateJFAStat, :515-577): sessions = utterance ranges, grouped by speaker
int liagpu_jfa_stats(int device, const float *x, long T, int D, const long *sess_begin, long nspk, const long *sessPerSpk, int C,
                     const double *w, const double *mean, const double *cov, double *N, double *N_h, double *F_X, double *F_X_h)
{
    GUARD({
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        MixtureGD ubm = make_mixture(C, D, w, mean, cov);
        std::vector<unsigned long> sps(sessPerSpk, sessPerSpk + nspk);
        JFAAcc jfa(srv, ubm, 1, 1, sps);
        std::vector<SegCluster> segs(jfa.getNSessions());
        for (unsigned long h = 0; h < jfa.getNSessions(); ++h) {
            Seg s; s.begin = (unsigned long)sess_begin[h]; s.length = (unsigned long)(sess_begin[h + 1] - sess_begin[h]); s.source = 0;
            segs[h].push_back(s);
        }
        jfa.computeAndAccumulateJFAStat(fs, segs);
        memcpy(N, jfa.getN().data(), jfa.getN().size() * sizeof(double));
        memcpy(N_h, jfa.getN_h().data(), jfa.getN_h().size() * sizeof(double));
        memcpy(F_X, jfa.getF_X().data(), jfa.getF_X().size() * sizeof(double));
        memcpy(F_X_h, jfa.getF_X_h().data(), jfa.getF_X_h().size() * sizeof(double));
    })
}

// Host arithmetic of JFAAcc::getUX / getSpeakerModel for ONE session (no device is opened): ux [SV], sp [SV] = m + V y + D z + U x
int liagpu_jfa_session_model_host(long SV, int rankEV, int rankEC, const double *means, const double *V, const double *y, const double *Dm,
                                  const double *z, const double *U, const double *x, double *ux, double *sp)
{
    GUARD({
        jfaUX(U, x, (unsigned long)rankEC, (unsigned long)SV, ux);
        jfaSessionSupervector(means, V, y, (unsigned long)rankEV, Dm, z, ux, (unsigned long)SV, sp);
    })
}

static std::vector<SegCluster> clusters_from(const long *clu_off, long nclu, const long *seg_begin, const long *seg_len)
{
    std::vector<SegCluster> out((size_t)nclu);
    for (long h = 0; h < nclu; ++h)
        for (long k = clu_off[h]; k < clu_off[h + 1]; ++k) {
            Seg s; s.begin = (unsigned long)seg_begin[k]; s.length = (unsigned long)seg_len[k]; s.source = 0;
            out[(size_t)h].push_back(s);
        }
    return out;
}

// JFAAcc::normalizeFeatures on the frames x [T x D] (rewritten in place): session h owns the segments clu_off[h] .. clu_off[h + 1]
// of (seg_begin, seg_len).  Y [nspk x rankEV], X [nsess x rankEC], Z [nspk x SV] are the factors; ux_out / model_out (nullable):
// getUX / the means of getSpeakerModel of every session, [nsess x SV].
int liagpu_jfa_normalize_features(int device, float *x, long T, int D, long nspk, const long *sessPerSpk, const long *clu_off,
                                  const long *seg_begin, const long *seg_len, int C, const double *w, const double *mean, const double *cov,
                                  int rankEV, int rankEC, const double *V, const double *U, const double *Dm, const double *Y, const double *X,
                                  const double *Z, double *ux_out, double *model_out)
{
    GUARD({
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        MixtureGD ubm = make_mixture(C, D, w, mean, cov);
        std::vector<unsigned long> sps(sessPerSpk, sessPerSpk + nspk);
        JFAAcc jfa(srv, ubm, (unsigned long)rankEV, (unsigned long)rankEC, sps);
        const size_t SV = (size_t)C * D, nsess = jfa.getNSessions();
        jfa.loadEV(std::vector<double>(V, V + (size_t)rankEV * SV));
        jfa.loadEC(std::vector<double>(U, U + (size_t)rankEC * SV));
        jfa.loadD(std::vector<double>(Dm, Dm + SV));
        jfa.getY().assign(Y, Y + (size_t)nspk * rankEV);
        jfa.getX().assign(X, X + nsess * rankEC);
        jfa.getZ().assign(Z, Z + (size_t)nspk * SV);
        for (size_t h = 0; h < nsess && (ux_out || model_out); ++h) {
            if (ux_out) { std::vector<double> ux; jfa.getUX(ux, (unsigned long)h); memcpy(ux_out + h * SV, ux.data(), SV * sizeof(double)); }
            if (model_out) { MixtureGD m = ubm; jfa.getSpeakerModel(m, (unsigned long)h); memcpy(model_out + h * SV, m.means().data(), SV * sizeof(double)); }
        }
        jfa.normalizeFeatures(fs, clusters_from(clu_off, (long)nsess, seg_begin, seg_len));
        fs.download(x);
    })
}

// The same with the choice of the path: batched = 0 JFAAcc::normalizeFeatures (the per-session loop), 1 JFAAcc::normalizeFeaturesBatch
int liagpu_jfa_normalize_features_batch(int device, float *x, long T, int D, long nspk, const long *sessPerSpk, const long *clu_off,
                                        const long *seg_begin, const long *seg_len, int C, const double *w, const double *mean, const double *cov,
                                        int rankEV, int rankEC, const double *V, const double *U, const double *Dm, const double *Y, const double *X,
                                        const double *Z, int batched)
{
    GUARD({
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        MixtureGD ubm = make_mixture(C, D, w, mean, cov);
        std::vector<unsigned long> sps(sessPerSpk, sessPerSpk + nspk);
        JFAAcc jfa(srv, ubm, (unsigned long)rankEV, (unsigned long)rankEC, sps);
        const size_t SV = (size_t)C * D, nsess = jfa.getNSessions();
        jfa.loadEV(std::vector<double>(V, V + (size_t)rankEV * SV));
        jfa.loadEC(std::vector<double>(U, U + (size_t)rankEC * SV));
        jfa.loadD(std::vector<double>(Dm, Dm + SV));
        jfa.getY().assign(Y, Y + (size_t)nspk * rankEV);
        jfa.getX().assign(X, X + nsess * rankEC);
        jfa.getZ().assign(Z, Z + (size_t)nspk * SV);
        const std::vector<SegCluster> clusters = clusters_from(clu_off, (long)nsess, seg_begin, seg_len);
        if (batched) jfa.normalizeFeaturesBatch(fs, clusters);
        else jfa.normalizeFeatures(fs, clusters);
        fs.download(x);
    })
}

// Timing of the two paths on resident frames (tools/bench_feat_comp_models.py): nsess sessions of frames_per_session frames each, one
// speaker per session with y = z = 0, session model m + U x_h.  which = 0: normalizeFeaturesBatch, 1: normalizeFeatures (the
// per-session loop).  ms_out[reps]: host clock around one call with the stream drained before and after (the caller drops warm-ups;
// every repetition rewrites the frames the previous one left, which changes no amount of work); then one more pass with the kernel
// timers on: kernel_ms[0..2] = k_gmm_pack, k_llk_mfma, k_feat_comp and kernel_ms[3] = launches of k_feat_comp, all of the LAST library
// call of the pass (the whole batch for which = 0, the last session alone for which = 1).
int liagpu_jfa_normalize_features_bench(int device, const float *x, long nsess, long frames_per_session, int D, int C, const double *w,
                                        const double *mean, const double *cov, int rankEC, const double *U, const double *X, int which, int reps,
                                        double *ms_out, double *kernel_ms)
{
    GUARD({
        if (which != 0 && which != 1) throw Exception("jfa_normalize_features_bench: which must be 0 (batch) or 1 (per-session loop)");
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)(nsess * frames_per_session), (unsigned long)D);
        MixtureGD ubm = make_mixture(C, D, w, mean, cov);
        JFAAcc jfa(srv, ubm, 1, (unsigned long)rankEC, std::vector<unsigned long>((size_t)nsess, 1));
        jfa.loadEC(std::vector<double>(U, U + (size_t)rankEC * C * D));
        jfa.getX().assign(X, X + (size_t)nsess * rankEC);
        std::vector<SegCluster> sel((size_t)nsess);
        for (long h = 0; h < nsess; ++h) {
            Seg s;
            s.begin = (unsigned long)(h * frames_per_session); s.length = (unsigned long)frames_per_session; s.source = 0;
            sel[(size_t)h].push_back(s);
        }
        auto run = [&]() {
            if (which == 0) jfa.normalizeFeaturesBatch(fs, sel);
            else jfa.normalizeFeatures(fs, sel);
            srv.sync();
        };
        for (int r = 0; r < reps; ++r) {
            srv.sync();
            const auto t0 = std::chrono::steady_clock::now();
            run();
            ms_out[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        (void)gmmiv_ctx_set_option(srv.ctx(), "timing", 1);
        run();
        kernel_ms[0] = gmmiv_ctx_kernel_ms(srv.ctx(), "k_gmm_pack");
        kernel_ms[1] = gmmiv_ctx_kernel_ms(srv.ctx(), "k_llk_mfma");
        kernel_ms[2] = gmmiv_ctx_kernel_ms(srv.ctx(), "k_feat_comp");
        kernel_ms[3] = (double)gmmiv_ctx_kernel_launches(srv.ctx(), "k_feat_comp");
        (void)gmmiv_ctx_set_option(srv.ctx(), "timing", 0);
    })
}

// liagpu::featureMapping on the frames x [T x D] (rewritten in place) over the cluster (seg_begin, seg_len)[nseg]
int liagpu_feature_mapping(int device, float *x, long T, int D, const long *seg_begin, const long *seg_len, long nseg, int C, const double *w_cd,
                           const double *mean_cd, const double *cov_cd, const double *w_ci, const double *mean_ci, const double *cov_ci)
{
    GUARD({
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        MixtureGD cd = make_mixture(C, D, w_cd, mean_cd, cov_cd), ci = make_mixture(C, D, w_ci, mean_ci, cov_ci);
        const long off[2] = {0, nseg};
        featureMapping(ci, cd, fs, clusters_from(off, 1, seg_begin, seg_len)[0]);
        fs.download(x);
    })
}

// liagpu::normFeat on the frames x [T x D] (rewritten in place): source s = frames [src_first[s], src_first[s + 1]) (src_first has
// nsrc + 1 entries), its cluster the segments clu_off[s] .. clu_off[s + 1] of (seg_begin, seg_len), begins counted from the source's
// first frame.  ext_mean / ext_std: NULL or [ncols] (ncols = 0: all columns from first_col).
int liagpu_norm_feat(int device, float *x, long T, int D, long nsrc, const long *src_first, const long *clu_off, const long *seg_begin,
                     const long *seg_len, int segmentalMode, int fileMode, int cmsOnly, int varOnly, const double *ext_mean, const double *ext_std,
                     int first_col, int ncols)
{
    GUARD({
        GpuServer srv(device);
        std::vector<unsigned long> first(src_first, src_first + nsrc);
        if (nsrc < 1 || src_first[nsrc] != T) throw Exception("norm_feat: src_first must end at the frame count");
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D, first);
        NormFeatCfg cfg;
        cfg.segmentalMode = segmentalMode != 0; cfg.fileMode = fileMode != 0; cfg.cmsOnly = cmsOnly != 0; cfg.varOnly = varOnly != 0;
        const int nc = ncols ? ncols : D - first_col;
        if (ext_mean && ext_std) { cfg.extMean.assign(ext_mean, ext_mean + nc); cfg.extStd.assign(ext_std, ext_std + nc); }
        normFeat(fs, clusters_from(clu_off, nsrc, seg_begin, seg_len), cfg, (unsigned long)first_col, (unsigned long)ncols);
        fs.download(x);
    })
}

// liagpu::normFeatOnlineMode on the frames x [T x D] (rewritten in place), sources as above
int liagpu_norm_feat_online(int device, float *x, long T, int D, long nsrc, const long *src_first, long windowDuration, long initWithDelay)
{
    GUARD({
        GpuServer srv(device);
        std::vector<unsigned long> first(src_first, src_first + nsrc);
        if (nsrc < 1 || src_first[nsrc] != T) throw Exception("norm_feat_online: src_first must end at the frame count");
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D, first);
        normFeatOnlineMode(fs, windowDuration, initWithDelay);
        fs.download(x);
    })
}

// liagpu::normFeatFiles: names [n] are joined with the paths / extensions like the reference's FeatureServer does
int liagpu_norm_feat_files(int device, int n, const char **names, const char *feature_path, const char *load_ext, const char *save_path,
                           const char *save_ext, const char *label_path, const char *label_ext, const char *label, double frameLength,
                           const char *mask, int writeAllFeatures, int segmentalMode, int fileMode, int cmsOnly, int varOnly)
{
    GUARD({
        GpuServer srv(device);
        NormFeatFilesCfg cfg;
        cfg.norm.segmentalMode = segmentalMode != 0; cfg.norm.fileMode = fileMode != 0; cfg.norm.cmsOnly = cmsOnly != 0; cfg.norm.varOnly = varOnly != 0;
        cfg.featureFilesPath = feature_path ? feature_path : ""; cfg.loadFeatureFileExtension = load_ext ? load_ext : "";
        cfg.saveFeatureFilePath = save_path ? save_path : ""; cfg.saveFeatureFileExtension = save_ext ? save_ext : "";
        cfg.labelFilesPath = label_path ? label_path : ""; cfg.labelFilesExtension = label_ext ? label_ext : "";
        cfg.labelSelectedFrames = label ? label : ""; cfg.frameLength = frameLength; cfg.featureServerMask = mask ? mask : "";
        cfg.writeAllFeatures = writeAllFeatures != 0;
        normFeatFiles(srv, std::vector<std::string>(names, names + n), cfg);
    })
}

// liagpu::normFeat with windowMode on the frames x [T x D] (rewritten in place), sources and clusters as liagpu_norm_feat takes them;
// fileMode != 0 applies the file pass afterwards
int liagpu_norm_feat_window(int device, float *x, long T, int D, long nsrc, const long *src_first, const long *clu_off, const long *seg_begin,
                            const long *seg_len, double windowDuration, double windowComp, double frameLength, int fileMode, int cmsOnly, int varOnly,
                            int first_col, int ncols)
{
    GUARD({
        GpuServer srv(device);
        std::vector<unsigned long> first(src_first, src_first + nsrc);
        if (nsrc < 1 || src_first[nsrc] != T) throw Exception("norm_feat_window: src_first must end at the frame count");
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D, first);
        NormFeatCfg cfg;
        cfg.windowMode = true; cfg.windowDuration = windowDuration; cfg.windowComp = windowComp; cfg.frameLength = frameLength;
        cfg.fileMode = fileMode != 0; cfg.cmsOnly = cmsOnly != 0; cfg.varOnly = varOnly != 0;
        normFeat(fs, clusters_from(clu_off, nsrc, seg_begin, seg_len), cfg, (unsigned long)first_col, (unsigned long)ncols);
        fs.download(x);
    })
}

// liagpu::normFeatFiles with windowMode (the other arguments as liagpu_norm_feat_files)
int liagpu_norm_feat_files_window(int device, int n, const char **names, const char *feature_path, const char *load_ext, const char *save_path,
                                  const char *save_ext, const char *label_path, const char *label_ext, const char *label, double frameLength,
                                  const char *mask, int writeAllFeatures, int fileMode, int cmsOnly, int varOnly, double windowDuration, double windowComp)
{
    GUARD({
        GpuServer srv(device);
        NormFeatFilesCfg cfg;
        cfg.norm.windowMode = true; cfg.norm.windowDuration = windowDuration; cfg.norm.windowComp = windowComp;
        cfg.norm.fileMode = fileMode != 0; cfg.norm.cmsOnly = cmsOnly != 0; cfg.norm.varOnly = varOnly != 0;
        cfg.featureFilesPath = feature_path ? feature_path : ""; cfg.loadFeatureFileExtension = load_ext ? load_ext : "";
        cfg.saveFeatureFilePath = save_path ? save_path : ""; cfg.saveFeatureFileExtension = save_ext ? save_ext : "";
        cfg.labelFilesPath = label_path ? label_path : ""; cfg.labelFilesExtension = label_ext ? label_ext : "";
        cfg.labelSelectedFrames = label ? label : ""; cfg.frameLength = frameLength; cfg.featureServerMask = mask ? mask : "";
        cfg.writeAllFeatures = writeAllFeatures != 0;
        normFeatFiles(srv, std::vector<std::string>(names, names + n), cfg);
    })
}

// liagpu::normFeat with warp on the frames x [T x D] (rewritten in place), sources and clusters as liagpu_norm_feat takes them; the
// target table (nbin_t, tbounds [nbin_t + 1], tcount [nbin_t]) or, with nbin_t == 0, the file histo_path (NULL: the refusal of the
// rand()-made default target).  windowMode != 0 is passed on to be refused by name.
int liagpu_norm_feat_warp(int device, float *x, long T, int D, long nsrc, const long *src_first, const long *clu_off, const long *seg_begin,
                          const long *seg_len, int segmentalMode, int fileMode, int windowMode, int cmsOnly, int varOnly, long warpBinCount,
                          int warpAdd01Norm, int nbin_t, const double *tbounds, const double *tcount, const char *histo_path, int first_col, int ncols)
{
    GUARD({
        GpuServer srv(device);
        std::vector<unsigned long> first(src_first, src_first + nsrc);
        if (nsrc < 1 || src_first[nsrc] != T) throw Exception("norm_feat_warp: src_first must end at the frame count");
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D, first);
        NormFeatCfg cfg;
        cfg.warp = true; cfg.warpBinCount = (unsigned long)warpBinCount; cfg.warpAdd01Norm = warpAdd01Norm != 0;
        cfg.segmentalMode = segmentalMode != 0; cfg.fileMode = fileMode != 0; cfg.windowMode = windowMode != 0;
        cfg.cmsOnly = cmsOnly != 0; cfg.varOnly = varOnly != 0;
        if (nbin_t > 0) { cfg.warpTarget.bounds.assign(tbounds, tbounds + nbin_t + 1); cfg.warpTarget.count.assign(tcount, tcount + nbin_t); }
        if (histo_path) cfg.warpGaussHistoFilename = histo_path;
        normFeat(fs, clusters_from(clu_off, nsrc, seg_begin, seg_len), cfg, (unsigned long)first_col, (unsigned long)ncols);
        fs.download(x);
    })
}

// liagpu::featWarpHost (no device): runs [nrun x 3] = (first frame, length, unit); status (nullable) [nunits x D]
int liagpu_feat_warp_host(float *x, long ld, int D, const long *runs, long nrun, long nunits, long nbBin, int nbin_t, const double *tbounds,
                          const double *tcount, int *status)
{
    GUARD({
        Histo t;
        t.bounds.assign(tbounds, tbounds + nbin_t + 1); t.count.assign(tcount, tcount + nbin_t);
        std::vector<int64_t> r(runs, runs + 3 * nrun);
        std::vector<int> st;
        featWarpHost(x, (unsigned long)ld, D, r, nunits, (unsigned long)nbBin, t, status ? &st : nullptr);
        if (status) std::copy(st.begin(), st.end(), status);
    })
}

// .histo files: nbin = liagpu_histo_bins(path) (< 0: error), then liagpu_histo_read fills bounds [nbin + 1] and count [nbin]
long liagpu_histo_bins(const char *path)
{
    long n = -1;
    const int rc = [&]() -> int { GUARD({ n = (long)readHistoFile(path).count.size(); }) }();
    return rc ? -1 : n;
}
int liagpu_histo_read(const char *path, double *bounds, double *count)
{
    GUARD({
        const Histo h = readHistoFile(path);
        std::copy(h.bounds.begin(), h.bounds.end(), bounds);
        std::copy(h.count.begin(), h.count.end(), count);
    })
}
int liagpu_histo_write(const char *path, int nbin, const double *bounds, const double *count)
{
    GUARD({
        Histo h;
        h.bounds.assign(bounds, bounds + nbin + 1); h.count.assign(count, count + nbin);
        writeHistoFile(path, h);
    })
}

// liagpu::normFeatFiles with warp (the other arguments as liagpu_norm_feat_files); histo_path NULL or "": the refusal of the default target
int liagpu_norm_feat_files_warp(int device, int n, const char **names, const char *feature_path, const char *load_ext, const char *save_path,
                                const char *save_ext, const char *label_path, const char *label_ext, const char *label, double frameLength,
                                const char *mask, int writeAllFeatures, int segmentalMode, int fileMode, int windowMode, int cmsOnly, int varOnly,
                                long warpBinCount, int warpAdd01Norm, const char *histo_path)
{
    GUARD({
        GpuServer srv(device);
        NormFeatFilesCfg cfg;
        cfg.norm.warp = true; cfg.norm.warpBinCount = (unsigned long)warpBinCount; cfg.norm.warpAdd01Norm = warpAdd01Norm != 0;
        cfg.norm.warpGaussHistoFilename = histo_path ? histo_path : "";
        cfg.norm.segmentalMode = segmentalMode != 0; cfg.norm.fileMode = fileMode != 0; cfg.norm.windowMode = windowMode != 0;
        cfg.norm.cmsOnly = cmsOnly != 0; cfg.norm.varOnly = varOnly != 0;
        cfg.featureFilesPath = feature_path ? feature_path : ""; cfg.loadFeatureFileExtension = load_ext ? load_ext : "";
        cfg.saveFeatureFilePath = save_path ? save_path : ""; cfg.saveFeatureFileExtension = save_ext ? save_ext : "";
        cfg.labelFilesPath = label_path ? label_path : ""; cfg.labelFilesExtension = label_ext ? label_ext : "";
        cfg.labelSelectedFrames = label ? label : ""; cfg.frameLength = frameLength; cfg.featureServerMask = mask ? mask : "";
        cfg.writeAllFeatures = writeAllFeatures != 0;
        normFeatFiles(srv, std::vector<std::string>(names, names + n), cfg);
    })
}

// ComputeTest from FILES for one ndx line (test file + client list): RAW models, .prm features with
// featureServerMask, .lbl selection.  Writes the NIST-style result lines (segmental mode) into out_text
// and the LLRs into llr_out[nseg x nClients].  ComputeTest.cpp:129-215 + the format readers of io.h.
int liagpu_compute_test_files(int device, const char *world_path, int nClients, const char **client_paths,
                              const char **client_names, const char *prm_path, const char *lbl_path, const char *mask,
                              const char *label, double frameLength, int topDistribsCount, int complete, double minLLK,
                              double maxLLK, const char *gender, const char *testName, double threshold, double *llr_out,
                              long max_llr, char *out_text, long out_cap)
{
    GUARD({
        GpuServer srv(device);
        MixtureGD world = readMixtureRAW(world_path);
        FeatureFile ff = readFeatureFile(prm_path, mask ? mask : "");
        if (ff.vectSize != world.getVectSize()) throw Exception("vectSize of features and world model differ");
        FeatureBuffer fs(srv, ff.data.data(), ff.nFrames, ff.vectSize);
        SegCluster segs = selectSegments(readLabelFile(lbl_path), label, frameLength);
        DeviceMixture dworld(srv, world);
        std::vector<DeviceMixture *> cl;
        std::vector<double> out;
        try {
            for (int i = 0; i < nClients; ++i) cl.push_back(new DeviceMixture(srv, readMixtureRAW(client_paths[i])));
            out = computeTestLLR(fs, segs, dworld, cl, topDistribsCount, complete != 0, minLLK, maxLLK, true);
        } catch (...) { for (auto p : cl) delete p; throw; }
        for (auto p : cl) delete p;
        if ((long)out.size() > max_llr) throw Exception("llr_out too small");
        memcpy(llr_out, out.data(), out.size() * sizeof(double));
        std::string text;
        for (size_t s = 0; s < segs.size(); ++s)
            for (int i = 0; i < nClients; ++i)   // frameIdxToTime(begin), frameIdxToTime(begin + length) (ComputeTest.cpp:186)
                text += resultLine(out[s * nClients + i], client_names[i], testName, gender, threshold, true,
                                   frameIdxToTime(segs[s].begin, frameLength), frameIdxToTime(segs[s].begin + segs[s].length, frameLength)) + "\n";
        if ((long)text.size() + 1 > out_cap) throw Exception("out_text too small");
        memcpy(out_text, text.c_str(), text.size() + 1);
    })
}

// ---- ComputeTest for a whole trial list (computeTestBatch) ------------------------------------------------------------------------------
// the lists of an ndx in flat form: line l owns the segments [line_seg_off[l], line_seg_off[l + 1]) of seg_begin / seg_len and the clients
// line_clients[line_cl_off[l] .. line_cl_off[l + 1]) (indices into the nModels models).  Checked before any device is touched.
static void check_lines(long nlines, const long *line_seg_off, const long *line_cl_off, const long *line_clients, int nModels)
{
    if (nlines < 0 || !line_seg_off || !line_cl_off) throw Exception("compute_test_batch: bad line tables");
    if (line_seg_off[0] != 0 || line_cl_off[0] != 0) throw Exception("compute_test_batch: the offset tables must start at 0");
    for (long l = 0; l < nlines; ++l) {
        if (line_seg_off[l + 1] < line_seg_off[l] || line_cl_off[l + 1] < line_cl_off[l]) throw Exception("compute_test_batch: the offset tables must be non-decreasing");
        for (long k = line_cl_off[l]; k < line_cl_off[l + 1]; ++k)
            if (line_clients[k] < 0 || line_clients[k] >= nModels)
                throw Exception("compute_test_batch: line " + std::to_string(l) + " names client " + std::to_string(line_clients[k]) + " of " + std::to_string(nModels));
    }
}

// ComputeTestJFA for a whole trial list (computeTestJFABatch): the tables of liagpu_compute_test_batch, every client model of the world's
// shape, U [rankEC x C*D].  which = 0: computeTestJFABatch; 1: the composition of the existing calls on one accumulator -- the same
// JFAAcc steps, JFAAcc::normalizeFeatures (the per-session loop) on this call's own copy of the frames, computeTestBatch on the
// rewritten buffer (the lines' selections must not share frames).  llr_out: one LLR per line and client, line after line; comp_out
// (nullable) [sum of the selections x D]: the compensated frames, line after line; x_out (nullable) [nlines x rankEC]: the channel factors.
int liagpu_compute_test_jfa(int device, const float *x, long T, int D, long nlines, const long *line_seg_off, const long *seg_begin, const long *seg_len,
                            int C, const double *w_world, const double *mean_world, const double *cov_world, int rankEC, const double *U, int nModels,
                            const double *w_cl, const double *mean_cl, const double *cov_cl, const long *line_cl_off, const long *line_clients,
                            int topDistribsCount, int complete, double minLLK, double maxLLK, int which, double *llr_out, long max_llr, long *n_llr,
                            float *comp_out, double *x_out)
{
    GUARD({
        check_lines(nlines, line_seg_off, line_cl_off, line_clients, nModels);
        if (which != 0 && which != 1) throw Exception("compute_test_jfa: which must be 0 (batch) or 1 (composition of the existing calls)");
        if (rankEC < 1 || !U || nModels < 1) throw Exception("compute_test_jfa: U with at least one eigenchannel and at least one client model are needed");
        if (line_cl_off[nlines] > max_llr) throw Exception("compute_test_jfa: llr_out too small");
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        MixtureGD world = make_mixture(C, D, w_world, mean_world, cov_world);
        DeviceMixture dworld(srv, world);
        const size_t SV = (size_t)C * D;
        std::vector<MixtureGD> models;
        for (int g = 0; g < nModels; ++g) models.push_back(make_mixture(C, D, w_cl + (size_t)g * C, mean_cl + g * SV, cov_cl + g * SV));
        DeviceMixtureBatch batch(srv, models);
        const std::vector<double> Um(U, U + (size_t)rankEC * SV);
        std::vector<SegCluster> sel((size_t)nlines);
        std::vector<std::vector<unsigned long>> cl((size_t)nlines);
        for (long l = 0; l < nlines; ++l) {
            sel[(size_t)l] = make_cluster(seg_begin + line_seg_off[l], seg_len + line_seg_off[l], line_seg_off[l + 1] - line_seg_off[l]);
            cl[(size_t)l].assign(line_clients + line_cl_off[l], line_clients + line_cl_off[l + 1]);
        }
        std::vector<std::vector<double>> out;
        std::vector<float> comp;
        std::vector<double> xf;
        if (which == 0)
            out = computeTestJFABatch(fs, sel, world, Um, (unsigned long)rankEC, dworld, batch, cl, topDistribsCount, complete != 0, minLLK, maxLLK,
                                      comp_out ? &comp : nullptr, x_out ? &xf : nullptr);
        else if (nlines > 0) {
            JFAAcc jfa(srv, world, 1, (unsigned long)rankEC, std::vector<unsigned long>((size_t)nlines, 1));
            jfa.loadEC(Um);
            jfa.computeAndAccumulateJFAStat(fs, sel);
            jfa.estimateUEUT();
            jfa.estimateAndInverseL_EC();
            jfa.substractMplusVYplusDZ();
            jfa.estimateX();
            xf = jfa.getX();
            jfa.normalizeFeatures(fs, sel);
            out = computeTestBatch(fs, sel, dworld, batch, cl, topDistribsCount, complete != 0, minLLK, maxLLK, false);
            if (comp_out) {
                std::vector<float> all((size_t)T * D); // the rewritten buffer, its selected rows line after line
                fs.download(all.data());
                for (const SegCluster &c : sel)
                    for (const Seg &s : c) comp.insert(comp.end(), all.begin() + (size_t)s.begin * D, all.begin() + (size_t)(s.begin + s.length) * D);
            }
        }
        long k = 0;
        for (const auto &o : out) { memcpy(llr_out + k, o.data(), o.size() * sizeof(double)); k += (long)o.size(); }
        if (n_llr) *n_llr = k;
        if (comp_out && !comp.empty()) memcpy(comp_out, comp.data(), comp.size() * sizeof(float));
        if (x_out && !xf.empty()) memcpy(x_out, xf.data(), xf.size() * sizeof(double));
    })
}

// models: nModels client models laid out one after the other, model g with model_C[g] Gaussians (model_C == NULL: all have C), covariances
// as in liagpu_compute_test.  which = 0: computeTestBatch; 1: the computeTestLLR loop line by line, every model resident as its own
// DeviceMixture.  llr_out: the lines' results one after the other, each [seg or 0][client]; *n_llr = their total.
int liagpu_compute_test_batch(int device, const float *x, long T, int D, long nlines, const long *line_seg_off, const long *seg_begin, const long *seg_len,
                              int C, const double *w_world, const double *mean_world, const double *cov_world, int nModels, const int *model_C,
                              const double *w_cl, const double *mean_cl, const double *cov_cl, const long *line_cl_off, const long *line_clients,
                              int topDistribsCount, int complete, double minLLK, double maxLLK, int segmentalMode, int which, double *llr_out, long max_llr,
                              long *n_llr)
{
    GUARD({
        check_lines(nlines, line_seg_off, line_cl_off, line_clients, nModels);
        if (which != 0 && which != 1) throw Exception("compute_test_batch: which must be 0 (batch) or 1 (per-line loop)");
        long need = 0;
        for (long l = 0; l < nlines; ++l) need += (segmentalMode ? line_seg_off[l + 1] - line_seg_off[l] : 1) * (line_cl_off[l + 1] - line_cl_off[l]);
        if (need > max_llr) throw Exception("compute_test_batch: llr_out too small");
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        MixtureGD world = make_mixture(C, D, w_world, mean_world, cov_world);
        DeviceMixture dworld(srv, world);
        std::vector<MixtureGD> models;
        size_t ow = 0, om = 0;
        for (int g = 0; g < nModels; ++g) {
            const int Cg = model_C ? model_C[g] : C;
            models.push_back(make_mixture(Cg, D, w_cl + ow, mean_cl + om, cov_cl + om));
            ow += (size_t)Cg; om += (size_t)Cg * D;
        }
        std::vector<SegCluster> sel((size_t)nlines);
        std::vector<std::vector<unsigned long>> cl((size_t)nlines);
        for (long l = 0; l < nlines; ++l) {
            sel[(size_t)l] = make_cluster(seg_begin + line_seg_off[l], seg_len + line_seg_off[l], line_seg_off[l + 1] - line_seg_off[l]);
            cl[(size_t)l].assign(line_clients + line_cl_off[l], line_clients + line_cl_off[l + 1]);
        }
        std::vector<std::vector<double>> out;
        if (which == 0)
            out = computeTestBatch(fs, sel, dworld, models, cl, topDistribsCount, complete != 0, minLLK, maxLLK, segmentalMode != 0);
        else {
            std::vector<std::unique_ptr<DeviceMixture>> dm;
            for (const MixtureGD &m : models) dm.emplace_back(new DeviceMixture(srv, m));
            for (long l = 0; l < nlines; ++l) {
                std::vector<DeviceMixture *> c;
                for (unsigned long g : cl[(size_t)l]) c.push_back(dm[g].get());
                out.push_back(computeTestLLR(fs, sel[(size_t)l], dworld, c, topDistribsCount, complete != 0, minLLK, maxLLK, segmentalMode != 0));
            }
        }
        long k = 0;
        for (const auto &o : out) { memcpy(llr_out + k, o.data(), o.size() * sizeof(double)); k += (long)o.size(); }
        if (n_llr) *n_llr = k;
    })
}

// the lines of an ndx: test name + client names; empty lines skipped
static void read_ndx(const char *ndx_path, std::vector<std::string> &tests, std::vector<std::vector<std::string>> &clients)
{
    std::ifstream in(ndx_path);
    if (!in) throw Exception(std::string("cannot open the ndx file ") + ndx_path);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string tok;
        if (!(ls >> tok)) continue;
        tests.push_back(tok);
        clients.emplace_back();
        while (ls >> tok) clients.back().push_back(tok);
    }
}

// What liagpu_compute_test_ndx will produce for this ndx, from the ndx and the label files alone (host only, no device, no feature or
// model file is opened): *n_llr = the number of scores (selected segments x clients, over all lines), *text_bytes = an upper bound of the
// size of the result text including its terminator.  The caller sizes llr_out / out_text with them.
int liagpu_compute_test_ndx_count(const char *ndx_path, const char *label_path, const char *label_ext, const char *label, double frameLength,
                                  const char *gender, long *n_llr, long *text_bytes)
{
    GUARD({
        std::vector<std::string> tests;
        std::vector<std::vector<std::string>> cl;
        read_ndx(ndx_path, tests, cl);
        long n = 0, bytes = 1;
        const size_t fixed = strlen(gender ? gender : "") + 96; // separators, the decision, two times and a score of at most 24 characters each
        for (size_t l = 0; l < tests.size(); ++l) {
            const size_t nseg = selectSegments(readLabelFile(std::string(label_path) + tests[l] + label_ext), label, frameLength).size();
            n += (long)(nseg * cl[l].size());
            for (const std::string &id : cl[l]) bytes += (long)(nseg * (fixed + id.size() + tests[l].size()));
        }
        *n_llr = n;
        *text_bytes = bytes;
    })
}

// ComputeTest from FILES for a whole ndx (segmental mode, like liagpu_compute_test_files): every line of ndx_path is a test file name
// followed by the ids of its clients.  Test file <feature_path><name><feature_ext> with the selection of <label_path><name><label_ext>,
// client model <model_path><id><model_ext> (RAW; each distinct id is read once).  All lines are scored in one computeTestBatch; out_text
// receives the result lines in the format of liagpu_compute_test_files, line after line, llr_out the LLRs in the same order.
int liagpu_compute_test_ndx(int device, const char *world_path, const char *ndx_path, const char *model_path, const char *model_ext,
                            const char *feature_path, const char *feature_ext, const char *label_path, const char *label_ext, const char *mask,
                            const char *label, double frameLength, int topDistribsCount, int complete, double minLLK, double maxLLK, const char *gender,
                            double threshold, double *llr_out, long max_llr, long *n_llr, char *out_text, long out_cap)
{
    GUARD({
        std::vector<std::string> tests, ids;
        std::vector<std::vector<std::string>> names;
        read_ndx(ndx_path, tests, names);
        std::map<std::string, unsigned long> idOf;
        std::vector<std::vector<unsigned long>> cl(tests.size());
        for (size_t l = 0; l < tests.size(); ++l)
            for (const std::string &tok : names[l]) {
                auto it = idOf.find(tok);
                if (it == idOf.end()) { it = idOf.emplace(tok, (unsigned long)ids.size()).first; ids.push_back(tok); }
                cl[l].push_back(it->second);
            }
        MixtureGD world = readMixtureRAW(world_path);
        std::vector<MixtureGD> models;
        for (const std::string &id : ids) models.push_back(readMixtureRAW(std::string(model_path) + id + model_ext));
        // the frames of all test files, one source per line
        std::vector<float> frames;
        std::vector<unsigned long> first;
        std::vector<SegCluster> sel(tests.size());
        for (size_t l = 0; l < tests.size(); ++l) {
            FeatureFile ff = readFeatureFile(std::string(feature_path) + tests[l] + feature_ext, mask ? mask : "");
            if (ff.vectSize != world.getVectSize()) throw Exception("vectSize of features and world model differ (" + tests[l] + ")");
            first.push_back((unsigned long)(frames.size() / ff.vectSize));
            frames.insert(frames.end(), ff.data.begin(), ff.data.end());
            sel[l] = selectSegments(readLabelFile(std::string(label_path) + tests[l] + label_ext), label, frameLength, (unsigned long)l);
        }
        std::string text;
        long k = 0;
        if (!tests.empty()) {
            GpuServer srv(device);
            FeatureBuffer fs(srv, frames.data(), (unsigned long)(frames.size() / world.getVectSize()), world.getVectSize(), first);
            DeviceMixture dworld(srv, world);
            const std::vector<std::vector<double>> out = computeTestBatch(fs, sel, dworld, models, cl, topDistribsCount, complete != 0, minLLK, maxLLK, true);
            for (size_t l = 0; l < tests.size(); ++l) {
                const size_t nc = cl[l].size();
                if (k + (long)out[l].size() > max_llr) throw Exception("llr_out too small");
                memcpy(llr_out + k, out[l].data(), out[l].size() * sizeof(double));
                k += (long)out[l].size();
                for (size_t s = 0; s < sel[l].size(); ++s)
                    for (size_t i = 0; i < nc; ++i)
                        text += resultLine(out[l][s * nc + i], ids[cl[l][i]], tests[l], gender, threshold, true, frameIdxToTime(sel[l][s].begin, frameLength),
                                           frameIdxToTime(sel[l][s].begin + sel[l][s].length, frameLength)) + "\n";
            }
        }
        if (n_llr) *n_llr = k;
        if ((long)text.size() + 1 > out_cap) throw Exception("out_text too small");
        memcpy(out_text, text.c_str(), text.size() + 1);
    })
}

// tools/bench_computetest.py: nlines test segments of frames_per_line frames each (line l = frames [l n, (l + 1) n)), every line scored against
// clients_per_line of the nModels client models (line_clients [nlines x clients_per_line]); the models are the world's with the means
// mean_cl [nModels x C*D].  Timed on the host around the whole scoring (features and -- for the loop -- the models resident, the stream
// drained before and after): which = 0 computeTestBatch on a resident DeviceMixtureBatch, 1 = computeTestLLR line after line on resident
// DeviceMixtures, 2 = computeTestBatch from the host models (their upload is inside the timed region).  ms_out[reps]; then one more pass with the kernel timers on: kernel_ms[0..4] = k_llk_mfma,
// k_topc_rank, k_topc_use, k_trial_reduce of the LAST call of that pass (-1: not run) and [4] = the trial piece in effect.  llr_out
// [nlines x clients_per_line].  trial_piece > 0 sets the context's "trials_piece" knob (A/B runs).
int liagpu_bench_computetest(int device, const float *x, long T, int D, long nlines, long frames_per_line, int C, const double *w, const double *mean,
                             const double *cov, int nModels, const double *mean_cl, long clients_per_line, const long *line_clients, int topDistribsCount,
                             int complete, int which, int reps, long trial_piece, double *ms_out, double *kernel_ms, double *llr_out)
{
    GUARD({
        if (nlines * frames_per_line > T) throw Exception("bench_computetest: not enough frames");
        for (long k = 0; k < nlines * clients_per_line; ++k)
            if (line_clients[k] < 0 || line_clients[k] >= nModels) throw Exception("bench_computetest: client index out of range");
        GpuServer srv(device);
        FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D);
        MixtureGD world = make_mixture(C, D, w, mean, cov);
        DeviceMixture dworld(srv, world);
        if (trial_piece > 0) (void)gmmiv_ctx_set_option(srv.ctx(), "trials_piece", trial_piece);
        const size_t CD = (size_t)C * D;
        std::vector<MixtureGD> models((size_t)nModels, world);
        for (int g = 0; g < nModels; ++g) memcpy(models[(size_t)g].means().data(), mean_cl + (size_t)g * CD, CD * sizeof(double));
        std::vector<SegCluster> sel((size_t)nlines);
        std::vector<std::vector<unsigned long>> cl((size_t)nlines);
        for (long l = 0; l < nlines; ++l) {
            Seg s;
            s.begin = (unsigned long)(l * frames_per_line); s.length = (unsigned long)frames_per_line;
            sel[(size_t)l].push_back(s);
            cl[(size_t)l].assign(line_clients + l * clients_per_line, line_clients + (l + 1) * clients_per_line);
        }
        std::vector<std::unique_ptr<DeviceMixture>> dm;
        std::unique_ptr<DeviceMixtureBatch> db;
        if (which == 1)
            for (const MixtureGD &m : models) dm.emplace_back(new DeviceMixture(srv, m));
        if (which == 0) db.reset(new DeviceMixtureBatch(srv, models));
        std::vector<std::vector<double>> out;
        auto run = [&]() {
            if (which == 0)
                out = computeTestBatch(fs, sel, dworld, *db, cl, topDistribsCount, complete != 0, -200.0, 200.0, false);
            else if (which == 2)
                out = computeTestBatch(fs, sel, dworld, models, cl, topDistribsCount, complete != 0, -200.0, 200.0, false);
            else {
                out.assign((size_t)nlines, std::vector<double>());
                for (long l = 0; l < nlines; ++l) {
                    std::vector<DeviceMixture *> c;
                    for (unsigned long g : cl[(size_t)l]) c.push_back(dm[g].get());
                    out[(size_t)l] = computeTestLLR(fs, sel[(size_t)l], dworld, c, topDistribsCount, complete != 0, -200.0, 200.0, false);
                }
            }
            srv.sync();
        };
        for (int r = 0; r < reps; ++r) {
            srv.sync();
            const auto t0 = std::chrono::steady_clock::now();
            run();
            ms_out[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        (void)gmmiv_ctx_set_option(srv.ctx(), "timing", 1);
        run();
        kernel_ms[0] = gmmiv_ctx_kernel_ms(srv.ctx(), "k_llk_mfma");
        kernel_ms[1] = gmmiv_ctx_kernel_ms(srv.ctx(), "k_topc_rank");
        kernel_ms[2] = gmmiv_ctx_kernel_ms(srv.ctx(), "k_topc_use");
        kernel_ms[3] = gmmiv_ctx_kernel_ms(srv.ctx(), "k_trial_reduce");
        kernel_ms[4] = (double)(trial_piece > 0 ? trial_piece : GMMIV_TRIAL_PIECE);
        (void)gmmiv_ctx_set_option(srv.ctx(), "timing", 0);
        for (long l = 0; l < nlines; ++l) memcpy(llr_out + l * clients_per_line, out[(size_t)l].data(), (size_t)clients_per_line * sizeof(double));
    })
}

// EnergyDetector on one energy column (EnergyDetector.cpp:190-285, thresholdMode meanStd): energy [T] float32 (featureServerMask picks
// the column, vectSize 1), selected segments; out_begin / out_len [max_out] <- the output segments (frames of the SELECTION), model_out
// [3 * C] <- weights | means | covariances, *threshold_out <- the threshold.
int liagpu_energy_detector(int device, const float *energy, long T, const long *seg_begin, const long *seg_len, long nseg, int C, int nbTrainIt,
                           double varianceFlooring, double varianceCeiling, double alpha, long *out_begin, long *out_len, long max_out,
                           long *n_out, double *model_out, double *threshold_out)
{
    GUARD({
        GpuServer srv(device);
        FeatureBuffer fs(srv, energy, (unsigned long)T, 1);
        SegCluster segs = make_cluster(seg_begin, seg_len, nseg);
        EnergyDetectorCfg cfg;
        cfg.nbTrainIt = (unsigned long)nbTrainIt; cfg.mixtureDistribCount = (unsigned long)C;
        cfg.varianceFlooring = varianceFlooring; cfg.varianceCeiling = varianceCeiling; cfg.alpha = alpha;
        MixtureGD model(C, 1);
        double th = 0.0;
        SegCluster out = energyDetector(fs, segs, cfg, &model, &th);
        if ((long)out.size() > max_out) throw Exception("out_begin too small");
        for (size_t i = 0; i < out.size(); ++i) { out_begin[i] = (long)out[i].begin; out_len[i] = (long)out[i].length; }
        *n_out = (long)out.size();
        if (model_out)
            for (int c = 0; c < C; ++c) { model_out[c] = model.weight(c); model_out[C + c] = model.getMean(c, 0); model_out[2 * C + c] = model.getCov(c, 0); }
        if (threshold_out) *threshold_out = th;
    })
}

// liagpu::energyDetectorBatch on nfiles energy columns laid end to end: energy [T] float32, file f = frames [file_begin[f], file_begin[f + 1]),
// its input segments seg_begin / seg_len [seg_off[f], seg_off[f + 1]) (frames of the FILE).  out_off [nfiles + 1], out_begin / out_len
// [max_out] <- the output segments in CSR form (frames of each file's SELECTION); model_out [nfiles x 3 C] (w | mean | cov), threshold_out
// [nfiles], status_out [nfiles] (all nullable).
int liagpu_energy_detector_batch(int device, const float *energy, long T, const long *file_begin, long nfiles, const long *seg_off, const long *seg_begin,
                                 const long *seg_len, int C, int nbTrainIt, double varianceFlooring, double varianceCeiling, double alpha, long *out_off,
                                 long *out_begin, long *out_len, long max_out, double *model_out, double *threshold_out, int *status_out)
{
    GUARD({
        GpuServer srv(device);
        if (nfiles < 0 || (nfiles > 0 && (file_begin[0] != 0 || file_begin[nfiles] != T))) throw Exception("file_begin must run from 0 to T");
        std::vector<unsigned long> first((size_t)(nfiles > 0 ? nfiles : 1), 0);
        for (long f = 0; f < nfiles; ++f) first[(size_t)f] = (unsigned long)file_begin[f];
        FeatureBuffer fs(srv, energy, (unsigned long)T, 1, first);
        std::vector<SegCluster> sel((size_t)nfiles);
        for (long f = 0; f < nfiles; ++f) sel[(size_t)f] = make_cluster(seg_begin + seg_off[f], seg_len + seg_off[f], seg_off[f + 1] - seg_off[f]);
        if (nfiles == 0) sel.resize(fs.getSourceCount());
        EnergyDetectorCfg cfg;
        cfg.nbTrainIt = (unsigned long)nbTrainIt; cfg.mixtureDistribCount = (unsigned long)C;
        cfg.varianceFlooring = varianceFlooring; cfg.varianceCeiling = varianceCeiling; cfg.alpha = alpha;
        std::vector<MixtureGD> models;
        std::vector<double> th;
        std::vector<int> st;
        std::vector<SegCluster> out = energyDetectorBatch(fs, sel, cfg, &models, &th, &st);
        long k = 0;
        for (long f = 0; f < nfiles; ++f) {
            out_off[f] = k;
            for (const Seg &g : out[(size_t)f]) {
                if (k >= max_out) throw Exception("out_begin too small");
                out_begin[k] = (long)g.begin; out_len[k] = (long)g.length; ++k;
            }
            if (model_out)
                for (int c = 0; c < C; ++c) {
                    model_out[f * 3 * C + c] = models[(size_t)f].weight(c); model_out[f * 3 * C + C + c] = models[(size_t)f].getMean(c, 0);
                    model_out[f * 3 * C + 2 * C + c] = models[(size_t)f].getCov(c, 0);
                }
            if (threshold_out) threshold_out[f] = th[(size_t)f];
            if (status_out) status_out[f] = st[(size_t)f];
        }
        out_off[nfiles > 0 ? nfiles : 0] = k;
    })
}

// liagpu::energyDetectorFiles: names [n] are joined with the paths / extensions; threshold_out / status_out [n] (nullable)
int liagpu_energy_detector_files(int device, int n, const char **names, const char *feature_path, const char *load_ext, const char *label_path,
                                 const char *label_ext, const char *label, const char *save_path, const char *save_ext, const char *label_out,
                                 const char *mask, double frameLength, int C, int nbTrainIt, double varianceFlooring, double varianceCeiling, double alpha,
                                 double *threshold_out, int *status_out)
{
    GUARD({
        GpuServer srv(device);
        EnergyDetectorFilesCfg cfg;
        cfg.energy.nbTrainIt = (unsigned long)nbTrainIt; cfg.energy.mixtureDistribCount = (unsigned long)C;
        cfg.energy.varianceFlooring = varianceFlooring; cfg.energy.varianceCeiling = varianceCeiling; cfg.energy.alpha = alpha;
        cfg.featureFilesPath = feature_path ? feature_path : ""; cfg.loadFeatureFileExtension = load_ext ? load_ext : "";
        cfg.labelFilesPath = label_path ? label_path : ""; cfg.labelFilesExtension = label_ext ? label_ext : "";
        cfg.labelSelectedFrames = label ? label : ""; cfg.saveLabelFilePath = save_path ? save_path : "";
        cfg.saveLabelFileExtension = save_ext ? save_ext : ""; cfg.labelOutputFrames = label_out ? label_out : "";
        cfg.featureServerMask = mask ? mask : ""; cfg.frameLength = frameLength;
        std::vector<double> th;
        std::vector<int> st;
        energyDetectorFiles(srv, std::vector<std::string>(names, names + n), cfg, &th, &st);
        for (int k = 0; k < n; ++k) {
            if (threshold_out) threshold_out[k] = th[(size_t)k];
            if (status_out) status_out[k] = st[(size_t)k];
        }
    })
}

namespace {
TurnDetectionCfg turn_cfg(const char *crit, long winSize, long winStep, double alpha, double minLLK, double maxLLK)
{
    TurnDetectionCfg cfg;
    cfg.clusteringCrit = crit ? crit : "";
    if (winSize < 1 || winStep < 1) throw Exception("winSize and winStep must be >= 1");
    cfg.winSize = (unsigned long)winSize; cfg.winStep = (unsigned long)winStep; cfg.alpha = alpha; cfg.minLLK = minLLK; cfg.maxLLK = maxLLK;
    return cfg;
}
// out_off [nfiles + 1], out_begin / out_len [max_out] <- the clusters in CSR form; curve_off [nseg + 1] (nullable), value / smoothed / dec
// [max_pos], stats [nseg x 2] <- the curves of the input segments in table order
void turn_put(const std::vector<SegCluster> &out, const std::vector<std::vector<TurnCurve> > &curves, long *out_off, long *out_begin, long *out_len, long max_out,
              long *curve_off, double *value, double *smoothed, unsigned char *dec, double *stats, long max_pos)
{
    long k = 0, p = 0, q = 0;
    for (size_t f = 0; f < out.size(); ++f) {
        out_off[f] = k;
        for (const Seg &g : out[f]) {
            if (k >= max_out) throw Exception("out_begin too small");
            out_begin[k] = (long)g.begin; out_len[k] = (long)g.length; ++k;
        }
        if (curve_off)
            for (const TurnCurve &c : curves[f]) {
                curve_off[q] = p;
                if (p + (long)c.value.size() > max_pos) throw Exception("value too small");
                for (size_t i = 0; i < c.value.size(); ++i, ++p) { value[p] = c.value[i]; smoothed[p] = c.smoothed[i]; dec[p] = c.dec[i]; }
                stats[2 * q] = c.mean; stats[2 * q + 1] = c.std;
                ++q;
            }
    }
    out_off[out.size()] = k;
    if (curve_off) curve_off[q] = p;
}
} // namespace

// liagpu::turnDetectionBatch (twin == 0) or the host-only loop twin liagpu::turnDetection per file (twin != 0; no GPU is touched) on nfiles
// frame matrices laid end to end: x [T x D] float32, file f = frames [file_begin[f], file_begin[f + 1]), its input segments seg_begin /
// seg_len [seg_off[f], seg_off[f + 1]) (frames of the FILE).  Outputs: see turn_put; the output segments count frames of the file.
int liagpu_turn_detection_batch(int device, int twin, const float *x, long T, int D, const long *file_begin, long nfiles, const long *seg_off, const long *seg_begin,
                                const long *seg_len, const char *crit, long winSize, long winStep, double alpha, double minLLK, double maxLLK, long *out_off,
                                long *out_begin, long *out_len, long max_out, long *curve_off, double *value, double *smoothed, unsigned char *dec, double *stats,
                                long max_pos)
{
    GUARD({
        const TurnDetectionCfg cfg = turn_cfg(crit, winSize, winStep, alpha, minLLK, maxLLK);
        if (nfiles < 0 || D < 1 || (nfiles > 0 && (file_begin[0] != 0 || file_begin[nfiles] != T))) throw Exception("file_begin must run from 0 to T");
        std::vector<SegCluster> sel((size_t)nfiles), out;
        for (long f = 0; f < nfiles; ++f) sel[(size_t)f] = make_cluster(seg_begin + seg_off[f], seg_len + seg_off[f], seg_off[f + 1] - seg_off[f]);
        std::vector<std::vector<TurnCurve> > curves;
        if (twin) {
            out.resize((size_t)nfiles); curves.resize((size_t)nfiles);
            for (long f = 0; f < nfiles; ++f) {
                out[(size_t)f] = turnDetection(x + (size_t)file_begin[f] * D, (unsigned long)(file_begin[f + 1] - file_begin[f]), (unsigned long)D, sel[(size_t)f], cfg, &curves[(size_t)f]);
                for (Seg &g : out[(size_t)f]) g.source = (unsigned long)f;
            }
        } else if (nfiles > 0) {
            GpuServer srv(device);
            std::vector<unsigned long> first((size_t)nfiles, 0);
            for (long f = 0; f < nfiles; ++f) first[(size_t)f] = (unsigned long)file_begin[f];
            FeatureBuffer fs(srv, x, (unsigned long)T, (unsigned long)D, first);
            out = turnDetectionBatch(fs, sel, cfg, &curves);
        }
        turn_put(out, curves, out_off, out_begin, out_len, max_out, curve_off, value, smoothed, dec, stats, max_pos);
    })
}

// liagpu::turnDetectionFiles: names [n] are joined with the paths / extensions; out_off [n + 1], out_begin / out_len [max_out] <- the output
// segments (what the label files were written from)
int liagpu_turn_detection_files(int device, int n, const char **names, const char *feature_path, const char *load_ext, const char *label_path,
                                const char *label_ext, const char *label, const char *save_path, const char *save_ext, const char *mask, double frameLength,
                                const char *crit, long winSize, long winStep, double alpha, double minLLK, double maxLLK, long *out_off, long *out_begin,
                                long *out_len, long max_out)
{
    GUARD({
        TurnDetectionFilesCfg cfg;
        cfg.turn = turn_cfg(crit, winSize, winStep, alpha, minLLK, maxLLK);
        (void)turnCriterion(cfg.turn.clusteringCrit);
        GpuServer srv(device);
        cfg.featureFilesPath = feature_path ? feature_path : ""; cfg.loadFeatureFileExtension = load_ext ? load_ext : "";
        cfg.labelFilesPath = label_path ? label_path : ""; cfg.labelFilesExtension = label_ext ? label_ext : "";
        cfg.labelSelectedFrames = label ? label : ""; cfg.saveLabelFilePath = save_path ? save_path : "";
        cfg.saveLabelFileExtension = save_ext ? save_ext : ""; cfg.featureServerMask = mask ? mask : ""; cfg.frameLength = frameLength;
        const std::vector<SegCluster> out = turnDetectionFiles(srv, std::vector<std::string>(names, names + n), cfg);
        turn_put(out, std::vector<std::vector<TurnCurve> >(), out_off, out_begin, out_len, max_out, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
    })
}

// selectFrames alone (EnergyDetector.cpp:118-157; host only, no GPU): energy [T], threshold, selected segments -> output segments
int liagpu_select_frames(const float *energy, long T, double threshold, const long *seg_begin, const long *seg_len, long nseg, long *out_begin,
                         long *out_len, long max_out, long *n_out, long *count_out)
{
    GUARD({
        std::vector<float> e(energy, energy + T);
        SegCluster segs = make_cluster(seg_begin, seg_len, nseg), out;
        const unsigned long cnt = selectFrames(e, threshold, segs, out);
        if ((long)out.size() > max_out) throw Exception("out_begin too small");
        for (size_t i = 0; i < out.size(); ++i) { out_begin[i] = (long)out[i].begin; out_len[i] = (long)out[i].length; }
        *n_out = (long)out.size();
        if (count_out) *count_out = (long)cnt;
    })
}

// GmmTokenizer driven from its files (LIA_Utils/GmmTokenizer/src/GmmTokenizer.cpp:169-207 symbols, :120-164 confusion matrix): RAW world
// model, .prm features (masked), .lbl segments with the selected label.  symbols_out [max_symbols] <- one best-Gaussian index per selected
// frame (*n_symbols of them; skipped when symbols_out is NULL); confusion_out [C x C] (nullable, zeroed here) <- the nBest = topDistribsCount
// confusion counts; matrix_path (nullable / "") <- the same matrix as a DT file, like mce_matrix.save (:160).
int liagpu_gmm_tokenizer_files(int device, const char *world_path, const char *prm_path, const char *lbl_path, const char *mask,
                               const char *label, double frameLength, int topDistribsCount, double minLLK, double maxLLK,
                               long *symbols_out, long max_symbols, long *n_symbols, long *confusion_out, long *dims,
                               const char *matrix_path)
{
    GUARD({
        GpuServer srv(device);
        MixtureGD world = readMixtureRAW(world_path);
        FeatureFile ff = readFeatureFile(prm_path, mask ? mask : "");
        if (ff.vectSize != world.getVectSize()) throw Exception("vectSize of features and world model differ");
        FeatureBuffer fs(srv, ff.data.data(), ff.nFrames, ff.vectSize);
        SegCluster segs = selectSegments(readLabelFile(lbl_path), label, frameLength);
        DeviceMixture dworld(srv, world);
        const unsigned long C = world.getDistribCount();
        if (dims) { dims[0] = (long)C; dims[1] = (long)world.getVectSize(); dims[2] = (long)totalFrame(segs); }
        if (symbols_out) {
            std::vector<unsigned long> stream;
            computeSymbols(segs, fs, dworld, stream, topDistribsCount, minLLK, maxLLK);
            if ((long)stream.size() > max_symbols) throw Exception("symbols_out too small");
            for (size_t i = 0; i < stream.size(); ++i) symbols_out[i] = (long)stream[i];
            if (n_symbols) *n_symbols = (long)stream.size();
        }
        if (confusion_out || (matrix_path && *matrix_path)) {
            std::vector<unsigned long> mce((size_t)C * C, 0);
            computeConfusionMatrix(segs, fs, dworld, (unsigned long)topDistribsCount, mce, minLLK, maxLLK);
            if (confusion_out) for (size_t i = 0; i < mce.size(); ++i) confusion_out[i] = (long)mce[i];
            if (matrix_path && *matrix_path) {
                MatrixD m; m.rows = C; m.cols = C; m.v.assign(mce.begin(), mce.end());
                writeMatrixDT(matrix_path, m);
            }
        }
    })
}

// XML mixture round trip + DB / DT matrices + per-id vector files (CPU tests; no GPU involved).
// xml_in -> xml_out (re-written) and raw_out (the same model as a RAW file); dims = {C, D}; first = {weight 0, covInv(0,0), mean(0,0)}
int liagpu_io_xml(const char *xml_in, const char *xml_out, const char *raw_out, long *dims, double *first)
{
    GUARD({
        MixtureGD m = readMixture(xml_in);
        dims[0] = (long)m.getDistribCount(); dims[1] = (long)m.getVectSize();
        first[0] = m.weight(0); first[1] = m.getCovInv(0, 0); first[2] = m.getMean(0, 0);
        writeMixtureXML(xml_out, m);
        if (raw_out && *raw_out) {
            writeMixtureRAW(raw_out, m);
            MixtureGD r = readMixture(raw_out);        // sniffed as RAW
            if (r.getDistribCount() != m.getDistribCount() || r.getMean(0, 0) != m.getMean(0, 0)) throw Exception("RAW re-read differs");
        }
    })
}
// width of the extents writeMatrixDB puts in a DB header (4 or 8 bytes; anything else only queries); returns the previous one
int liagpu_io_db_header_bytes(int bytes) { return setMatrixDBHeaderBytes(bytes); }
// matrix file -> matrix file in another format; dims = {rows, cols}
int liagpu_io_matrix_convert(const char *in, const char *fmt_in, const char *out, const char *fmt_out, long *dims)
{
    GUARD({
        const MatrixD m = readMatrix(in, fmt_in);
        dims[0] = (long)m.rows; dims[1] = (long)m.cols;
        writeMatrix(out, m, fmt_out);
    })
}
// W [n x rank] -> one vector file per id under dir (saveWbyFile), read back as columns (PldaTest::load): back [rank x n]
int liagpu_io_vectors(const char *dir, int n, const char **ids, const char *ext, const char *fmt, int rank, const double *W, double *back)
{
    GUARD({
        std::vector<std::string> v(ids, ids + n);
        saveVectorsById(std::string(dir) + "/", v, ext, std::vector<double>(W, W + (size_t)n * rank), (unsigned long)rank, fmt);
        unsigned long dim = 0;
        const std::vector<double> cols = loadVectorsById(dir, v, ext, dim, fmt);
        if (dim != (unsigned long)rank) throw Exception("vector files: dimension changed on the way");
        memcpy(back, cols.data(), cols.size() * sizeof(double));
    })
}

// format round trips used by the CPU tests (no GPU involved)
int liagpu_io_roundtrip(const char *raw_in, const char *raw_out, const char *prm_in, const char *prm_out, const char *mask,
                        long *dims /* C, D, nFrames, vectSize */, double *first_mean, float *first_frame)
{
    GUARD({
        MixtureGD m = readMixtureRAW(raw_in);
        writeMixtureRAW(raw_out, m);
        FeatureFile f = readFeatureFile(prm_in, "");
        writeFeatureFile(prm_out, f);
        FeatureFile fm = readFeatureFile(prm_in, mask);
        dims[0] = (long)m.getDistribCount(); dims[1] = (long)m.getVectSize(); dims[2] = (long)fm.nFrames; dims[3] = (long)fm.vectSize;
        for (unsigned long d = 0; d < m.getVectSize(); ++d) first_mean[d] = m.getMean(0, d);
        for (unsigned long d = 0; d < fm.vectSize; ++d) first_frame[d] = fm.data[d];
    })
}

int liagpu_label_segments(const char *lbl_path, const char *label, double frameLength, long *begin, long *len, long cap, long *n)
{
    GUARD({
        SegCluster c = selectSegments(readLabelFile(lbl_path), label, frameLength);
        if ((long)c.size() > cap) throw Exception("segment buffer too small");
        for (size_t i = 0; i < c.size(); ++i) { begin[i] = (long)c[i].begin; len[i] = (long)c[i].length; }
        *n = (long)c.size();
    })
}

// ComputeNorm on resident matrices (liagpu::computeNorm).  normType: 0 znorm, 1 tnorm, 2 ztnorm, 3 tznorm.  Every array may be a
// host or a device pointer; imp_models [Nt] / imp_segs [Nz]: host bytes or NULL.  Returns when the results are complete.
int liagpu_compute_norm(int device, int normType, int meanMode, double percentH, double percentL, long M, long S, long Nt, long Nz,
                        double *X, const double *Z, const double *T, const double *ZT, const unsigned char *imp_models,
                        const unsigned char *imp_segs, double *first_out)
{
    GUARD({
        static const char *names[] = {"znorm", "tnorm", "ztnorm", "tznorm"};
        ComputeNormCfg cfg;
        cfg.normType = normType >= 0 && normType <= 3 ? names[normType] : "?";
        cfg.meanMode = meanMode; cfg.percentH = percentH; cfg.percentL = percentL;
        if (imp_models) cfg.impModels.assign(imp_models, imp_models + Nt);
        if (imp_segs) cfg.impSegs.assign(imp_segs, imp_segs + Nz);
        GpuServer srv(device);
        computeNorm(srv, cfg, (unsigned long)M, (unsigned long)S, (unsigned long)Nt, (unsigned long)Nz, X, Z, T, ZT, first_out);
        srv.sync();
    })
}

// ComputeNorm on files (liagpu::computeNormFiles).  fields: fieldGender, fieldName, fieldDecision, fieldSeg, fieldLLR.  The lists
// are read and checked BEFORE a device is opened: a list that is not a full cross product fails without one.
int liagpu_compute_norm_files(int device, const char *normType, int meanMode, double percentH, double percentL, const char *testNistFile,
                              const char *znormNistFile, const char *tnormNistFile, const char *ztnormNistFile, const char *impostorIDList,
                              const char *outputFileBaseName, const int *fields)
{
    GUARD({
        ComputeNormFilesCfg cfg;
        cfg.norm.normType = normType; cfg.norm.meanMode = meanMode; cfg.norm.percentH = percentH; cfg.norm.percentL = percentL;
        cfg.testNistFile = testNistFile; cfg.znormNistFile = znormNistFile ? znormNistFile : "";
        cfg.tnormNistFile = tnormNistFile ? tnormNistFile : ""; cfg.ztnormNistFile = ztnormNistFile ? ztnormNistFile : "";
        cfg.impostorIDList = impostorIDList ? impostorIDList : ""; cfg.outputFileBaseName = outputFileBaseName;
        if (fields) { cfg.fields.fieldGender = fields[0]; cfg.fields.fieldName = fields[1]; cfg.fields.fieldDecision = fields[2];
                      cfg.fields.fieldSeg = fields[3]; cfg.fields.fieldLLR = fields[4]; }
        ComputeNormTables t = loadComputeNormTables(cfg);
        GpuServer srv(device);
        computeNormFiles(srv, cfg, t);
    })
}

// ComputeNorm on score lists (liagpu::computeNormLists).  normType as liagpu_compute_norm.  x [n] is normalised in place; line_model /
// line_seg [n]; per list (z, t, zt): ndist, off (HOST, ndist + 1), scores, nscores, pos (nullable), other (nullable), an unused list
// has ndist 0.  Every array but the offsets may be a host or a device pointer.  Returns when the results are complete.
int liagpu_compute_norm_lists(int device, int normType, int meanMode, double percentH, double percentL, long n, double *x,
                              const int32_t *line_model, const int32_t *line_seg, const long *ndist, const int64_t *const *off,
                              const double *const *scores, const long *nscores, const int64_t *const *pos, const int32_t *const *other,
                              double *first_out)
{
    GUARD({
        static const char *names[] = {"znorm", "tnorm", "ztnorm", "tznorm"};
        ComputeNormCfg cfg;
        cfg.normType = normType >= 0 && normType <= 3 ? names[normType] : "?";
        cfg.meanMode = meanMode; cfg.percentH = percentH; cfg.percentL = percentL;
        ScoreListView v[3];
        for (int i = 0; i < 3; ++i) {
            v[i].ndist = (unsigned long)ndist[i]; v[i].off = off[i]; v[i].scores = scores[i]; v[i].nscores = (unsigned long)nscores[i];
            v[i].pos = pos[i]; v[i].other = other[i];
        }
        GpuServer srv(device);
        computeNormLists(srv, cfg, (unsigned long)n, x, line_model, line_seg, v[0], v[1], v[2], first_out);
        srv.sync();
    })
}

namespace {
ComputeNormFilesCfg normFilesCfg(const char *normType, int meanMode, double percentH, double percentL, const char *testNistFile,
                                 const char *znormNistFile, const char *tnormNistFile, const char *ztnormNistFile, const char *impostorIDList,
                                 const char *outputFileBaseName, const int *fields)
{
    ComputeNormFilesCfg cfg;
    cfg.norm.normType = normType; cfg.norm.meanMode = meanMode; cfg.norm.percentH = percentH; cfg.norm.percentL = percentL;
    cfg.testNistFile = testNistFile; cfg.znormNistFile = znormNistFile ? znormNistFile : "";
    cfg.tnormNistFile = tnormNistFile ? tnormNistFile : ""; cfg.ztnormNistFile = ztnormNistFile ? ztnormNistFile : "";
    cfg.impostorIDList = impostorIDList ? impostorIDList : ""; cfg.outputFileBaseName = outputFileBaseName ? outputFileBaseName : "";
    if (fields) { cfg.fields.fieldGender = fields[0]; cfg.fields.fieldName = fields[1]; cfg.fields.fieldDecision = fields[2];
                  cfg.fields.fieldSeg = fields[3]; cfg.fields.fieldLLR = fields[4]; }
    return cfg;
}
} // namespace

// ComputeNorm on files, as lists (liagpu::computeNormListFiles): the arguments of liagpu_compute_norm_files, no cross product asked
// for.  The lists are read and checked BEFORE a device is opened: a test line without a distribution fails without one.
int liagpu_compute_norm_list_files(int device, const char *normType, int meanMode, double percentH, double percentL, const char *testNistFile,
                                   const char *znormNistFile, const char *tnormNistFile, const char *ztnormNistFile, const char *impostorIDList,
                                   const char *outputFileBaseName, const int *fields)
{
    GUARD({
        const ComputeNormFilesCfg cfg = normFilesCfg(normType, meanMode, percentH, percentL, testNistFile, znormNistFile, tnormNistFile,
                                                     ztnormNistFile, impostorIDList, outputFileBaseName, fields);
        ComputeNormLists t = loadComputeNormLists(cfg);
        GpuServer srv(device);
        computeNormListFiles(srv, cfg, t);
    })
}

// liagpu::loadComputeNormLists for callers and tests (host only): *out is a handle to the loaded lists; _sizes fills
// { test lines, then per list z, t, zt: distributions, slots, 1 if `other` is present, bytes of the keys joined by '\n' };
// _get copies list `which` (0 z, 1 t, 2 zt) and _lines the test list (each pointer may be NULL); _free releases the handle.
int liagpu_norm_lists_load(const char *normType, const char *testNistFile, const char *znormNistFile, const char *tnormNistFile,
                           const char *ztnormNistFile, const char *impostorIDList, const int *fields, void **out)
{
    GUARD({
        const ComputeNormFilesCfg cfg = normFilesCfg(normType, 0, 0.0, 0.0, testNistFile, znormNistFile, tnormNistFile, ztnormNistFile,
                                                     impostorIDList, nullptr, fields);
        *out = new ComputeNormLists(loadComputeNormLists(cfg));
    })
}
static const ScoreList &normListOf(const ComputeNormLists *t, int which)
{
    if (which < 0 || which > 2) throw Exception("norm_lists: list 0 (z), 1 (t) or 2 (zt)");
    return which == 0 ? t->z : (which == 1 ? t->t : t->zt);
}
static std::string joinedKeys(const ScoreList &l)
{
    std::string k;
    for (size_t i = 0; i < l.keys.size(); ++i) { k += l.keys[i]; k += '\n'; }
    return k;
}
int liagpu_norm_lists_sizes(const void *h, long *sz)
{
    GUARD({
        const ComputeNormLists *t = (const ComputeNormLists *)h;
        sz[0] = (long)t->test.size();
        for (int w = 0; w < 3; ++w) {
            const ScoreList &l = normListOf(t, w);
            sz[1 + 4 * w] = (long)l.keys.size(); sz[2 + 4 * w] = (long)l.scores.size(); sz[3 + 4 * w] = l.other.empty() ? 0 : 1;
            sz[4 + 4 * w] = (long)joinedKeys(l).size();
        }
    })
}
int liagpu_norm_lists_get(const void *h, int which, int64_t *off, double *scores, int32_t *other, char *keys)
{
    GUARD({
        const ScoreList &l = normListOf((const ComputeNormLists *)h, which);
        if (off) memcpy(off, l.off.data(), l.off.size() * sizeof(int64_t));
        if (scores) memcpy(scores, l.scores.data(), l.scores.size() * sizeof(double));
        if (other) memcpy(other, l.other.data(), l.other.size() * sizeof(int32_t));
        if (keys) { const std::string k = joinedKeys(l); memcpy(keys, k.data(), k.size()); }
    })
}
int liagpu_norm_lists_lines(const void *h, double *x, int32_t *line_model, int32_t *line_seg)
{
    GUARD({
        const ComputeNormLists *t = (const ComputeNormLists *)h;
        if (x) memcpy(x, t->x.data(), t->x.size() * sizeof(double));
        if (line_model) memcpy(line_model, t->lineModel.data(), t->lineModel.size() * sizeof(int32_t));
        if (line_seg) memcpy(line_seg, t->lineSeg.data(), t->lineSeg.size() * sizeof(int32_t));
    })
}
void liagpu_norm_lists_free(void *h) { delete (ComputeNormLists *)h; }

// resultLine / parseResultLine round trip for the tests: writes the line into `line` (cap bytes) and parses `parse_in` (or the
// line just written when NULL) with the given field positions into name / seg / gender (each cap bytes), decision and llr.
int liagpu_result_line(double llr, const char *client, const char *test, const char *gender, double threshold, int withTimes, double start,
                       double end, const char *parse_in, const int *fields, char *line, char *name, char *seg, char *gender_out, long cap,
                       int *decision, double *llr_out)
{
    GUARD({
        const std::string l = resultLine(llr, client, test, gender, threshold, withTimes != 0, start, end);
        ResultFields f;
        if (fields) { f.fieldGender = fields[0]; f.fieldName = fields[1]; f.fieldDecision = fields[2]; f.fieldSeg = fields[3]; f.fieldLLR = fields[4]; }
        const ResultLine r = parseResultLine(parse_in ? std::string(parse_in) : l, f);
        auto put = [&](char *dst, const std::string &v) {
            if ((long)v.size() + 1 > cap) throw Exception("result line buffer too small");
            memcpy(dst, v.c_str(), v.size() + 1);
        };
        put(line, l); put(name, r.name); put(seg, r.seg); put(gender_out, r.gender);
        *decision = r.decision; *llr_out = r.llr;
    })
}

} // extern "C"
