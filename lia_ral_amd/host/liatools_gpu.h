// liatools_gpu.h -- C++ host side above the C ABI (include/gmmiv.h): the LIA_SpkTools driver
// functions of the hot path, same names / argument meaning / error behaviour as the reference,
// with the per-frame ALIZE calls replaced by batched calls into libgmmiv (HIP, gfx950).
//
// The ALIZE container types are not available (alize-core is external to LIA_RAL), so minimal
// stand-ins carry the same information: Seg/SegCluster (begin, length, source), FeatureBuffer
// (a FeatureServer with featureServerBufferSize = ALL_FEATURES, resident in HBM), MixtureGD
// (weights, means, covariances + computeAll()).  Errors throw liagpu::Exception, which a tool
// driver catches and prints exactly like `catch (Exception& e) { cout << e.toString(); }`
// (LIA_SpkDet/TrainWorld/src/TrainWorld.cpp:187-190).
#pragma once
#include <math.h>
#include <stdint.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/gmmiv.h"
#include "../../include/gmmiv_iv_trials.h"
#include "../../include/gmmiv_feat_window.h"
#include "../../include/gmmiv_turn.h"

namespace liagpu {

struct Exception : std::runtime_error {
    explicit Exception(const std::string &m) : std::runtime_error(m) {}
    std::string toString() const { return std::string("[gmmiv::Exception] ") + what(); }
};

// SegTools.cpp:265-271: a label "begin_s end_s" selects frames begin..end INCLUSIVE (length = end-begin+1)
struct Seg {
    unsigned long begin = 0, length = 0;
    unsigned long source = 0; // index of the feature file in the FeatureBuffer
    unsigned long labelCode = 0; // Seg::labelCode(): the multi-cluster baggedSegments tags a segment with the component it was drawn for
};
typedef std::vector<Seg> SegCluster;
unsigned long totalFrame(const SegCluster &c);
unsigned long timeToFrameIdx(double time, double frameLength);   // SegTools.cpp:135-142
double frameIdxToTime(unsigned long idx, double frameLength);    // SegTools.cpp:143-148
Seg segFromLabel(double begin_s, double end_s, double frameLength, unsigned long source = 0);

class GpuServer; // context owner (the StatServer/MixtureServer pair of the reference)

// A Matrix<double> / DoubleVector of the reference that LIVES ON THE DEVICE.  The accumulator classes below (EMAcc, TVAcc,
// JFAAcc, PldaDev) keep their statistics, matrices and accumulators in these: the C ABI is called with device pointers, so
// nothing crosses PCIe between the steps of a training loop -- at BASELINE's T-matrix configuration one rank holds F (6.1 GB),
// TETt and A (1.3 GB each); staging them per call would cost more than the compute.  A host copy exists only while somebody
// looks at it: host() downloads when the device copy is newer and assumes the caller may write (the next dev() uploads it
// again), chost() is the read-only view.  All copies / memsets are enqueued on the context's stream, i.e. in order with the
// kernels of the C ABI calls; only transfers that involve host memory wait for the stream.
class DVec {
  public:
    DVec() = default;
    explicit DVec(GpuServer &srv) : _srv(&srv) {}
    ~DVec();
    DVec(const DVec &) = delete;
    DVec &operator=(const DVec &) = delete;
    void bind(GpuServer &srv) { _srv = &srv; }
    size_t size() const { return _n; }
    bool empty() const { return _n == 0; }
    void assign(size_t n, double v = 0.0);            // vector::assign: n elements equal to v (device-side for v == 0)
    void set(const double *h, size_t n);              // upload
    void set(const std::vector<double> &h) { set(h.data(), h.size()); }
    void copyFrom(const DVec &o);                     // device-to-device (storeAccs / restoreAccs)
    void swap(DVec &o);
    double *dev();                                    // read-write device view (uploads a modified host copy first)
    const double *cdev() const;                       // read-only device view
    std::vector<double> &host();                      // read-write host view (downloads if the device copy is newer)
    const std::vector<double> &chost() const;         // read-only host view
    void get(double *h, size_t n, size_t offset = 0) const; // download a range without keeping a host copy

  private:
    void sync() const;
    void *st() const;
    void reserve(size_t n);
    GpuServer *_srv = nullptr;
    mutable double *_d = nullptr;
    size_t _n = 0, _cap = 0;
    mutable std::vector<double> _h;
    mutable bool _hostValid = false;  // _h mirrors the device copy
    mutable bool _hostDirty = false;  // _h may have been written through host(): the device copy is stale
};

// FeatureServer(ALL_FEATURES): all frames of all sources, float32 like SPro files, device resident.
class FeatureBuffer {
  public:
    FeatureBuffer(GpuServer &srv, const float *frames, unsigned long nFrames, unsigned long vectSize,
                  const std::vector<unsigned long> &sourceFirstFrame = std::vector<unsigned long>(1, 0));
    ~FeatureBuffer();
    unsigned long getVectSize() const { return _d; }
    unsigned long getFeatureCount() const { return _n; }
    unsigned long getFirstFeatureIndexOfASource(unsigned long s) const { return _first.at(s); }
    unsigned long getSourceCount() const { return _first.size(); }
    unsigned long getFeatureCountOfASource(unsigned long s) const { return (s + 1 < _first.size() ? _first[s + 1] : _n) - _first.at(s); }
    const float *device() const { return _dev; }
    unsigned long unusableFrames() const { return _unusable; } // frames with a NaN / infinite / absurd value, counted once at upload
    // device matrix [n x D] of the frames selected by the cluster, in cluster order.  The selection is ENQUEUED on the server's
    // stream (run table from pinned memory + k_gather_runs) and the pointer is valid in stream order: every gmmiv call of the same
    // server that follows sees the frames; the host does not wait.  A cluster that is one contiguous run is returned in place.
    // The matrix is overwritten by the next select() -- also in stream order, after the kernels that still read it.
    const float *select(const SegCluster &c, unsigned long &nSelected);
    // The same selection for a call that REWRITES the frames (normalizeFeatures, featureMapping) -- and scatter(), its inverse:
    // the rows of `selected` (what select / selectForUpdate returned for this cluster) go back to the cluster's frames, in stream
    // order (k_scatter_runs; nothing to do when the cluster was one contiguous run and was handed out in place).  This is the
    // reference's writeFeature (AccumulateJFAStat.cpp:4675, GeneralTools.cpp:800).  Frames outside the cluster are not touched.
    float *selectForUpdate(const SegCluster &c, unsigned long &nSelected) { return const_cast<float *>(select(c, nSelected)); }
    void scatter(const SegCluster &c, const float *selected);
    float *mutableDevice() { return _dev; }             // the resident frames as a mutable device view
    void download(float *frames) const;                 // all frames back to the host (waits for the stream)
    GpuServer &server() { return _srv; }

  private:
    unsigned long buildRuns(const SegCluster &c, unsigned long &nSelected, unsigned long &firstFrame, size_t &nPieces);
    GpuServer &_srv;
    float *_dev = nullptr, *_sel = nullptr;
    unsigned long _n, _d, _selCap = 0, _unusable = 0;
    std::vector<unsigned long> _first;
    int64_t *_hRuns = nullptr, *_dRuns = nullptr; // run table: pinned host copy, device copy
    size_t _runsCap = 0, _dRunsCap = 0;
    void *_runsCopied = nullptr;                  // hipEvent_t: the last upload of the pinned table has completed
};

// MixtureGD / DistribGD: weight(c), getMean/getCov/getCovInv, setMean/setCov, computeAll()
class MixtureGD {
  public:
    MixtureGD(unsigned long distribCount, unsigned long vectSize);
    unsigned long getDistribCount() const { return _c; }
    unsigned long getVectSize() const { return _d; }
    double &weight(unsigned long c) { return _w[c]; }
    double weight(unsigned long c) const { return _w[c]; }
    double getMean(unsigned long c, unsigned long i) const { return _mean[c * _d + i]; }
    double getCov(unsigned long c, unsigned long i) const { return _cov[c * _d + i]; }
    double getCovInv(unsigned long c, unsigned long i) const { return _covInv[c * _d + i]; }
    void setMean(unsigned long c, double v, unsigned long i) { _mean[c * _d + i] = v; }
    void setCov(unsigned long c, double v, unsigned long i) { _cov[c * _d + i] = v; }
    // a model file stores covInv: keep the file's bits (1 / (1 / v) need not round back to v)
    void setCovInv(unsigned long c, double v, unsigned long i) { _covInv[c * _d + i] = v; _cov[c * _d + i] = 1.0 / v; }
    void computeAll(); // covInv = 1/cov (cst, det are derived on the device)
    std::vector<double> &weights() { return _w; }
    std::vector<double> &means() { return _mean; }
    std::vector<double> &covs() { return _cov; }
    const std::vector<double> &covInvs() const { return _covInv; }
    const std::vector<double> &weights_c() const { return _w; }
    const std::vector<double> &means_c() const { return _mean; }
    const std::vector<double> &covs_c() const { return _cov; }

  private:
    unsigned long _c, _d;
    std::vector<double> _w, _mean, _cov, _covInv;
};

// Owns the gmmiv context (one per GPU).  createAndStoreMixtureStat() -> EMAcc / LLKAcc below.
class GpuServer {
  public:
    explicit GpuServer(int device = 0);
    ~GpuServer();
    gmmiv_ctx *ctx() { return _ctx; }
    void *stream() { return gmmiv_ctx_stream(_ctx); } // hipStream_t of the context: the host layer's own copies are ordered on it
    void sync() { check(gmmiv_ctx_sync(_ctx)); }
    // grow-only device workspace of the host layer itself (slot 0..7): the per-file buffers of computeTestLLR live here instead of
    // a hipMalloc / hipFree pair -- two device synchronisations -- per test file.  Contents do not survive a growth.
    void *workspace(int slot, size_t bytes);
    void check(int rc) const; // throws Exception(gmmiv_last_error()) on rc != 0

  private:
    gmmiv_ctx *_ctx = nullptr;
    void *_ws[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t _wsBytes[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// Scope of ONE frame-consuming call of the C ABI on `srv`'s context with frames of `fs`: the per-call screening pass is skipped
// (assume_finite) iff that buffer was found free of unusable frames at upload, or the user had set the option; the previous
// value comes back at scope exit.  The decision follows the buffer actually read, which may belong to another server.
class FiniteScope {
  public:
    FiniteScope(GpuServer &srv, const FeatureBuffer &fs);
    ~FiniteScope();
    FiniteScope(const FiniteScope &) = delete;
    FiniteScope &operator=(const FiniteScope &) = delete;

  private:
    gmmiv_ctx *_ctx;
    long _prev;
};

// Device copy of a MixtureGD
class DeviceMixture {
  public:
    DeviceMixture(GpuServer &srv, const MixtureGD &m);
    ~DeviceMixture();
    void update(const MixtureGD &m);
    gmmiv_gmm *handle() const { return _g; }
    GpuServer &server() { return _srv; }
    unsigned long getDistribCount() const { return _c; }
    unsigned long getVectSize() const { return _d; }

  private:
    GpuServer &_srv;
    gmmiv_gmm *_g = nullptr;
    unsigned long _c = 0, _d = 0;
};

// MixtureStat in EM mode: resetEM / computeAndAccumulateEM (batched) / getEM / getEMFeatureCount / addAccEM
class EMAcc {
  public:
    EMAcc(DeviceMixture &dm, const MixtureGD &model);
    void resetEM();
    double getEMFeatureCount() const;   // sum of the frame weights (2 doubles come back from the device)
    double getAccumulatedLLK() const;
    MixtureGD getEM() const; // ML weights / means / covariances; occ == 0 keeps the model's values
    void setModel(const MixtureGD &model) { _model = model; } // the model the next getEM() falls back to (createAndStoreMixtureStat(*world) of the next iteration)
    void addAccEM(const EMAcc &o);
    std::vector<double> &flat() { return _acc.host(); } // host view of the flat accumulator (downloaded on demand)
    DVec &acc() { return _acc; }                         // the device-resident accumulator = the all-reduce payload
    DeviceMixture &mixture() { return _dm; }

  private:
    DeviceMixture &_dm;
    MixtureGD _model;
    DVec _acc;
};

// FrameAccGD
struct FrameAccGD {
    std::vector<double> acc; // [sum | sumsq | n]
    unsigned long vectSize = 0;
    unsigned long getCount() const { return acc.empty() ? 0 : (unsigned long)acc.back(); }
    std::vector<double> getMeanVect() const;
    std::vector<double> getCovVect() const; // biased: sumsq/n - mean^2
};

// ---- AccumulateStat.h --------------------------------------------------------------------------
// accumulateStatEM (AccumulateStat.cpp:103-152): returns sum_t log lk_t over the cluster
double accumulateStatEM(FeatureBuffer &fs, EMAcc &emAcc, const SegCluster &selectedSegments);
double accumulateStatEM(FeatureBuffer &fs, EMAcc &emAcc, const SegCluster &selectedSegments, double weight);
// accumulateStatLLK (AccumulateStat.cpp:69-94): mean clamped llk over the cluster (getMeanLLK)
double accumulateStatLLK(FeatureBuffer &fs, DeviceMixture &m, const SegCluster &selectedSegments, double minLLK,
                         double maxLLK);
// MixtureStat in LLK mode: resetLLK / computeAndAccumulateLLK(f, weight) (batched) / getMeanLLK = sum w llk / sum w -- the accumulator the
// meanLikelihood family drives over one cluster, over several streams (GeneralTools.cpp:589-607) and over weighted feature servers
// (`decision[nbFs]` as the frame weight: AccumulateStat.cpp:344-379, GeneralTools.cpp:610-624)
struct LLKAcc {
    double sumLLK = 0.0, sumWeight = 0.0;
    void resetLLK() { sumLLK = sumWeight = 0.0; }
    double getMeanLLK() const { return sumWeight > 0.0 ? sumLLK / sumWeight : 0.0; }
    double getAccumulatedLLK() const { return sumLLK; }
    double getAccumulatedLLKFeatureCount() const { return sumWeight; }
};
void accumulateStatLLK(LLKAcc &llkAcc, FeatureBuffer &fs, DeviceMixture &m, const SegCluster &selectedSegments, double weight, double minLLK,
                       double maxLLK);
struct TrainStream;
double meanLikelihood(const std::vector<TrainStream> &streams, DeviceMixture &model, double minLLK, double maxLLK);                  // :599-607
double meanLikelihood(const std::vector<TrainStream> &streams, DeviceMixture &model, const std::vector<double> &decision, double minLLK,
                      double maxLLK);                                                                                                  // :610-624
// accumulateStatFrame (AccumulateStat.cpp:387-410)
void accumulateStatFrame(FrameAccGD &frameAcc, FeatureBuffer &fs, const SegCluster &selectedSegments);

// ---- TrainTools.h ------------------------------------------------------------------------------
struct TrainCfg { // TrainTools.cpp:67-93
    double initVarianceFlooring = 0.0, initVarianceCeiling = 10.0, finalVarianceFlooring = 0.0, finalVarianceCeiling = 10.0;
    unsigned long nbTrainIt = 1;
    double baggedFrameProbability = 1.0;
    unsigned long baggedMinimalLength = 3, baggedMaximalLength = 7, initRand = 0;
    // componentReduction / targetMixtureDistribCount (:86-91): after every iteration keep the nbTop heaviest components, nbTop going
    // linearly from the initial count to the target (TrainTools.cpp:1078-1097)
    bool componentReduction = false;
    unsigned long targetDistribCount = 0;
    // normalizeModel (:76-84): after every iteration move the mixture to global mean 0 / variance 1 (normalizeMixture, :287-315);
    // normalizeModelNbIt only applies with normalizeModelMeanOnly
    bool normalizeModel = false, normalizeModelMeanOnly = false;
    unsigned long normalizeModelNbIt = 1;
    // not a reference parameter: when set, receives the wall time (ms) of every iteration, measured from the end of the previous
    // iteration's model update to the end of this one's (what bench.py's host_layer block reports)
    std::vector<double> *iterationMs = nullptr;
};
double setItParameter(double begin, double end, int nbIt, int it);                                 // :560-564
void varianceControl(MixtureGD &model, double flooring, double ceiling, const std::vector<double> &covSignal); // :567-587
unsigned long computeMeanCov(FeatureBuffer &fs, const SegCluster &seg, std::vector<double> &mean, std::vector<double> &cov); // :593-611
// GeneralTools.cpp:455-510 with glibc rand() (baggedFrame :309-314); caller seeds with srand()
void baggedSegments(const SegCluster &selectedSegments, SegCluster &baggedFrameSegment, double baggedProbability,
                    unsigned long minimumLength, unsigned long maximumLength);
// The multi-selection form (GeneralTools.cpp:330-390): ONE walk over the input segments, nbBagged independent draws per chunk;
// a chunk drawn for component idx is appended with labelCode = idx (rand() order: chunk-major, component-minor)
void baggedSegments(const SegCluster &selectedSegments, SegCluster &baggedSeg, unsigned long nbBagged, double baggedProbability,
                    unsigned long minimumLength, unsigned long maximumLength);
// mixtureInit: the start-from-scratch model of TrainWorld (random picking of frames per component; means = the picked
// frames' means, covariances = globalCov, equal weights).  glibc srand / rand in the reference's order, like baggedSegments.
//   multi-stream form, TrainTools.cpp:674-766 -- the one TrainWorld.cpp:177 calls -- for ONE stream of weight streamWeight:
//     p = nbFrameToSelect * weight / totalFrame (folded into several bagging passes when > 1, :700-708 -- as written that fold
//     only terminates for p >= ~4.9; for 1 < p < 4.9 the reference spins forever and this layer throws instead), seed
//     srand((stream + 1) * 100 + baggedIt + 1), one multi-selection baggedSegments pass per iteration;
//   single-stream form, TrainTools.cpp:619-672: p = baggedFrameProbabilityInit / distribCount, seed
//     srand((indg + 1) * (baggedIt + 1)) and one plain baggedSegments pass PER COMPONENT.
// A component that drew no frame has no mean: Exception (FrameAccGD::getMeanVect on an empty accumulator is undefined in
// the reference).  frameCount (optional) receives the frames picked per component.
struct MixtureInitCfg { unsigned long baggedMinimalLength = 3, baggedMaximalLength = 7; double nbFrameToSelect = 50; double baggedFrameProbabilityInit = 0.0; };
struct TrainStream;
// all input streams (fsTab / segTab / weightTab), the form TrainWorld.cpp:177 calls; the one-stream overload below forwards here
void mixtureInit(const std::vector<TrainStream> &streams, MixtureGD &world, const std::vector<double> &globalCov, const MixtureInitCfg &cfg,
                 std::vector<unsigned long> *frameCount = nullptr);
void mixtureInit(FeatureBuffer &fs, const SegCluster &selectedSegments, double streamWeight, MixtureGD &world,
                 const std::vector<double> &globalCov, const MixtureInitCfg &cfg, std::vector<unsigned long> *frameCount = nullptr);
void mixtureInitSingleStream(FeatureBuffer &fs, MixtureGD &world, const SegCluster &selectedSegments, const std::vector<double> &globalCov,
                             const MixtureInitCfg &cfg, std::vector<unsigned long> *frameCount = nullptr);
// trainModelStream (TrainTools.cpp:1030-1110), single stream; returns the per-iteration mean llk
// ("llkPreviousIt").  allReduce, when given, sums the flat accumulator over ranks (RCCL/xGMI).
// Multi-GPU: frames sharded per rank, ONE all-reduce of the flat EM accumulator per iteration, the collective twin of
// MixtureStat::addAccEM (AccumulateStat.cpp:286-292).  The default is the C ABI's own RCCL communicator (comm, on the device
// accumulator); AllReduceFn is the hook for another transport (it gets the HOST view of the accumulator).
typedef void (*AllReduceFn)(double *buf, size_t n, void *user);
// one input stream of TrainWorld ("inputStreamList" / "weightStreamList", TrainWorld.cpp:123-137): fsTab[i], segTab[i], weightTab[i].
// Every stream's FeatureBuffer lives on the same GpuServer.  weightTab defaults to 1 / nbStream (reserveMem, TrainWorld.cpp:85).
struct TrainStream { FeatureBuffer *fs = nullptr; const SegCluster *segs = nullptr; double weight = 1.0; };
// The stream form (TrainTools.cpp:1030-1110): per iteration and stream, baggedProba = p * nbTotalFrame * weight / totalFrame(stream)
// (folded into nbBaggedIt passes when > 1), seed ((trainIt+1+initRand)*200) + ((stream+1)*20) + (baggedIt+1), ONE accumulator over
// all streams; then getEM, varianceControl, componentReduction, normalizeModel.  `world` may come back with fewer components.
// The host prepares the selection of the next pass while the kernels of the current one run (rand() order unchanged: every pass
// seeds the generator itself).
std::vector<double> trainModelStream(const TrainCfg &cfg, const std::vector<TrainStream> &streams, const std::vector<double> &globalCov,
                                     MixtureGD &world, AllReduceFn allReduce = nullptr, void *user = nullptr, gmmiv_comm *comm = nullptr);
// component selection and model normalisation used by it (TrainTools.cpp:186-227, :240-315; TabWeight: GeneralTools.h:145-183)
std::vector<unsigned long> sortByWeight(const MixtureGD &model);     // TabWeight::_sortByWeight: qsort, heaviest first
unsigned long selectComponent(std::vector<bool> &selectCompA, unsigned long nbTop, const MixtureGD &inputM); // the nbTop heaviest
unsigned long selectComponent(std::vector<bool> &selectCompA, double wFactor, const MixtureGD &inputM);      // weight >= wFactor
double reduceModel(const std::vector<bool> &selectCompA, const MixtureGD &inputM, MixtureGD &outputM);        // returns the kept weight
void normalizeWeights(MixtureGD &outputM);
void mixtureFusion(const MixtureGD &mixt, std::vector<double> &mean, std::vector<double> &cov, double &wres);
void normalizeMixture(MixtureGD &mixt, const std::vector<double> &meanSignal, const std::vector<double> &covSignal, bool zeroOne,
                      unsigned long nbIt, bool meanOnly);
// global mean / covariance over several streams (computeMeanCov(config, fsTab, segTab, nbStream, ...), TrainTools.cpp:593-601)
unsigned long computeMeanCov(const std::vector<TrainStream> &streams, std::vector<double> &mean, std::vector<double> &cov);
std::vector<double> trainModelStream(const TrainCfg &cfg, FeatureBuffer &fs, const SegCluster &selectedSegments,
                                     const std::vector<double> &globalCov, MixtureGD &world, gmmiv_comm *comm);
std::vector<double> trainModelStream(const TrainCfg &cfg, FeatureBuffer &fs, const SegCluster &selectedSegments,
                                     const std::vector<double> &globalCov, MixtureGD &world,
                                     AllReduceFn allReduce = nullptr, void *user = nullptr, gmmiv_comm *comm = nullptr);

// ---- TrainTarget: MAP adaptation (TrainTools.cpp:445-489 computeMAPOccDep, :871-904 adaptModel) ----
struct MatrixD { unsigned long rows = 0, cols = 0; std::vector<double> v; }; // row-major; io.h reads / writes it (DT, DB)
struct MAPCfg { // MAPCfg::MAPCfg, TrainTools.cpp:95-147
    std::string method = "MAPOccDep"; // MAPAlgo: MAPOccDep, MAPModelBased (regulation factors), MAPConst, MAPConst2 (constant alpha), MLLR
    unsigned long nbTrainIt = 1;
    double baggedFrameProbability = 1.0;
    bool meanAdapt = true, varAdapt = false, weightAdapt = false;
    double meanReg = 16.0, varReg = 16.0, weightReg = 16.0; // MAPRegFactorMean / Var / Weight
    double meanAlpha = 0.75;                                  // MAPAlphaMean: a-priori probability of the init model (MAPConst / MAPConst2)
    bool normalizeModel = false, normalizeModelMeanOnly = false; // :125-135, applied after every iteration's MAP step (:898)
    unsigned long normalizeModelNbIt = 1;
    // adaptModelBatch only: keep varAdapt / normalizeModel / an unknown MAPAlgo's ML estimate on the device too (second-order statistics
    // per client, gmmiv_em_stats_models + gmmiv_map_adapt_models_full + gmmiv_normalize_models).  Off: those run the per-client loop.
    bool batchVariances = false;
    // MLLR only: when set, the transform W [D x (D+1)] is saved there (DT matrix) after every iteration.  The reference writes
    // "MLLR_matrix.mat" into the working directory unconditionally (TrainTools.cpp:892-893); a library does not.
    std::string mllrMatrixFile;
};
void computeMAPOccDep(const MixtureGD &initModel, MixtureGD &client, const MAPCfg &cfg, double frameCount);              // :445-489
void computeModelBasedMAPOccDep(const MixtureGD &initModel, MixtureGD &client, const MAPCfg &cfg, double frameCount);    // :491-536 (the same arithmetic)
void computeMAPConst(const MixtureGD &initModel, MixtureGD &client, const MAPCfg &cfg);                                  // :356-384 (means only)
void computeMAPConst2(const MixtureGD &initModel, MixtureGD &client, const MAPCfg &cfg);                                 // :390-420 (means only, weight-balanced)
// computeMAP (:543-556): dispatch on cfg.method; an unknown method leaves the client as it is (the reference prints a warning)
void computeMAP(const MixtureGD &initModel, MixtureGD &client, unsigned long frameCount, const MAPCfg &cfg);
// computeMLLR (:788-866), host arithmetic in the reference's order: outM holds the ML estimate (weights, means) of this iteration and
// comes back with means W [1; mean_in] and inM's weights and variances (copyVar -> computeAll(), copyWeight).  Row p of the returned
// W [D x (D+1)] is G_p^-1 z_p with occ_j = outM.weight(j) * frameCount; the inverse is a Gauss-Jordan elimination with partial
// pivoting in double.  meanAdapt / varAdapt / weightAdapt are not consulted.  Throws on a zero or non-finite pivot (a client
// without frames, fewer than D + 1 occupied Gaussians).
MatrixD computeMLLR(const MixtureGD &inM, MixtureGD &outM, unsigned long frameCount);
// client model = MAP(aprioriModel, EM estimate on the selected frames), nbTrainIt times; mapCfg.method == "MLLR" takes computeMLLR
// instead of computeMAP (:888-894), to which "MLLR" stays an unknown mapAlgo
void adaptModel(FeatureBuffer &fs, const SegCluster &selectedSegments, const MixtureGD &aprioriModel,
                MixtureGD &clientMixture, const MAPCfg &mapCfg);
// The same for many clients at once (the client loop of TrainTarget.cpp:150-270): client i = adaptModel(fs, selectedPerClient[i],
// aprioriModel, clientMixtures[i], mapCfg) called client after client in that order -- same bagging draws, results to the last bits of
// another summation order -- with ONE statistics pass per iteration for all clients (gmmiv_tv_stats_models, a model per client) and the
// MAP step on the device (gmmiv_map_adapt_models).  varAdapt, normalizeModel and an unknown MAPAlgo run the per-client loop, unless
// mapCfg.batchVariances is set: then they stay on the device as well (gmmiv_em_stats_models, gmmiv_map_adapt_models_full,
// gmmiv_normalize_models, gmmiv_gmm_batch_load_cov per iteration); a client whose MAP step leaves a variance that is not positive and
// finite gets its model as computed, as adaptModel gives it, and the first such client is named on stderr after the last iteration.
// "MLLR": the same loop with gmmiv_mllr_adapt_models as the adaptation step (varAdapt is ignored, as computeMLLR ignores it;
// normalizeModel, clients of another shape and vectSize > 62 run the per-client loop).  The statuses are read once, after the last
// iteration: a client whose system failed throws an Exception naming the first such client, as the per-client loop would.
// mllrW (optional): the last iteration's W of every client.  A configuration with mllrMatrixFile set runs the per-client loop (one
// file, rewritten client after client, iteration after iteration).
void adaptModelBatch(FeatureBuffer &fs, const std::vector<SegCluster> &selectedPerClient, const MixtureGD &aprioriModel,
                     std::vector<MixtureGD> &clientMixtures, const MAPCfg &mapCfg, std::vector<MatrixD> *mllrW = nullptr);

// ---- ComputeTest (LIA_SpkDet/ComputeTest/src/ComputeTest.cpp:129-215) -----------------------------
// LLR of each client against the world for one test file: per segment when segmentalMode, else one
// per file.  out[(seg or 0) * nClients + i] = mean llk_client - mean llk_world.
std::vector<double> computeTestLLR(FeatureBuffer &fs, const SegCluster &selectedSegments, DeviceMixture &world,
                                   std::vector<DeviceMixture *> &clients, int topDistribsCount, bool complete,
                                   double minLLK, double maxLLK, bool segmentalMode);
// The same for a whole ndx in one device pass (gmmiv_llr_trials): line l scores the selection selectedPerLine[l] against the models
// clientModels[clientsPerLine[l][..]].  Element l of the result is what computeTestLLR(fs, selectedPerLine[l], world, <those clients>, ...)
// returns, layout [seg or 0][client] -- to the last bits of another summation order (pieces of GMMIV_TRIAL_PIECE frames instead of
// gmmiv_segment_means' pieces).  The selections of all lines are gathered once, line after line (the way adaptModelBatch lays out its
// clients'); the models go into one gmmiv_gmm_batch, weights and covInv as ONE shared row when every client has the same.  Clients of
// another shape than the world run the per-line computeTestLLR loop.
std::vector<std::vector<double>> computeTestBatch(FeatureBuffer &fs, const std::vector<SegCluster> &selectedPerLine, DeviceMixture &world,
                                                  const std::vector<MixtureGD> &clientModels,
                                                  const std::vector<std::vector<unsigned long>> &clientsPerLine, int topDistribsCount,
                                                  bool complete, double minLLK, double maxLLK, bool segmentalMode);
// Device copies of MANY MixtureGD of one shape (what DeviceMixture is for one): a gmmiv_gmm_batch.  A caller that scores several trial
// lists against the same client set builds it once and passes it to the overload below; the overload above builds one per call (the
// upload of 1000 models of 2048 x 60 is 1 GB across PCIe).  Throws when the models differ in shape.
class DeviceMixtureBatch {
  public:
    DeviceMixtureBatch(GpuServer &srv, const std::vector<MixtureGD> &models);
    ~DeviceMixtureBatch();
    DeviceMixtureBatch(const DeviceMixtureBatch &) = delete;
    DeviceMixtureBatch &operator=(const DeviceMixtureBatch &) = delete;
    gmmiv_gmm_batch *handle() const { return _b; }
    size_t size() const { return _g; }
    unsigned long getDistribCount() const { return _c; }
    unsigned long getVectSize() const { return _d; }

  private:
    gmmiv_gmm_batch *_b = nullptr;
    size_t _g = 0;
    unsigned long _c = 0, _d = 0;
};
// the batch must have the world's shape
std::vector<std::vector<double>> computeTestBatch(FeatureBuffer &fs, const std::vector<SegCluster> &selectedPerLine, DeviceMixture &world,
                                                  DeviceMixtureBatch &clientModels, const std::vector<std::vector<unsigned long>> &clientsPerLine,
                                                  int topDistribsCount, bool complete, double minLLK, double maxLLK, bool segmentalMode);
// WindowLLR (LIA_SpkTools/src/UnsupervisedTools.cpp:70-145): sliding window over the per-frame LLRs of ComputeTest
// (ComputeTest.cpp:165-178).  One WindowOut per position at which the window is full.
struct WindowLLR {
    WindowLLR(unsigned long size, unsigned long dec, unsigned long nClient);
    void dec(unsigned long idxFrame);                        // :119-135
    void accLLR(unsigned long clientIdx, double llr);        // :136-139
    double getLLR(unsigned long clientIdx) const { return _acc[clientIdx] / (double)_size; }
    bool isEnd() const { return _count == _size; }
    unsigned long getIdxBegin() const { return _idx[_bIdx]; }
    unsigned long getIdxEnd() const { return _idx[(_bIdx + _count - 1) % _size]; }
    unsigned long _size, _dec, _nClient, _bIdx, _count;
    std::vector<unsigned long> _idx;
    std::vector<double> _acc, _llr; // _llr [size x nClient]
};
struct WindowOut { unsigned long idxBegin, idxEnd; std::vector<double> llr; /* one per client */ };
// The full frame loop of ComputeTest.cpp:154-207: worldDecime (DETERMINE_TOP_DISTRIBS on every worldDecime-th frame
// of a segment, USE_TOP_DISTRIBS with the last top set on the others) and the optional windowed LLRs
// (windowSize == 0: off).  Returns the same file / segment LLRs as computeTestLLR.
std::vector<double> computeTestLLR(FeatureBuffer &fs, const SegCluster &selectedSegments, DeviceMixture &world,
                                   std::vector<DeviceMixture *> &clients, int topDistribsCount, bool complete,
                                   double minLLK, double maxLLK, bool segmentalMode, unsigned long worldDecime,
                                   unsigned long windowSize, unsigned long windowDec, std::vector<WindowOut> *windows);

// ---- TopGauss.h (LIA_SpkTools/src/TopGauss.cpp) -----------------------------------------------------
// The per-frame Gaussian selection the factor-analysis tools compute once per feature file and cache on disk.
class TopGauss {
  public:
    // compute (:136-198): DETERMINE_TOP_DISTRIBS on every selected frame with a list of topDistribsCount entries (any count up to the model's), then
    // topGauss >= 1: the (unsigned long)topGauss heaviest Gaussians of every frame; topGauss < 1: Gaussians until their cumulative
    // likelihood passes topGauss * exp(llk) -- a variable count per frame.  Returns getMeanLLK() of the DETERMINE pass.
    double compute(DeviceMixture &ubm, FeatureBuffer &fs, const SegCluster &selectedSegments, double topGauss, int topDistribsCount,
                   bool complete, double minLLK, double maxLLK);
    // get (:275-316): mean llk of `ubm` (any model with the UBM's component order) on the stored selection (USE_TOP_DISTRIBS with
    // setTopDistribIndexVector(index, snsw, snsl) per frame)
    double get(DeviceMixture &ubm, FeatureBuffer &fs, const SegCluster &selectedSegments, bool complete, double minLLK, double maxLLK) const;
    // write / read (:200-224 / :76-98), the reference's binary layout on LP64: _nt, _nbgcnt (unsigned long, 8 bytes, native order),
    // _nbg[_nt] (unsigned long), _idx[_nbgcnt] (unsigned long), _snsw[_nt], _snsl[_nt] (double)
    void write(const std::string &path) const;
    void read(const std::string &path);
    unsigned long frameToIdx(unsigned long f) const; // :68-74
    unsigned long nt() const { return _nt; }
    unsigned long nbgcnt() const { return _nbgcnt; }
    unsigned long nbCapped() const { return _capped; } // frames whose likelihood mass was not reached within topDistribsCount entries
    const std::vector<unsigned long> &nbg() const { return _nbg; }
    const std::vector<unsigned long> &idx() const { return _idx; }
    const std::vector<double> &snsw() const { return _snsw; }
    const std::vector<double> &snsl() const { return _snsl; }

  private:
    unsigned long _nt = 0, _nbgcnt = 0, _capped = 0;
    std::vector<unsigned long> _nbg, _idx;
    std::vector<double> _snsw, _snsl;
};

// ---- GmmTokenizer (LIA_Utils/GmmTokenizer/src/GmmTokenizer.cpp): the two consumers of getTopDistribIndexVector() that ship golden
// outputs (test/test1.sym.ref, test/mce_matrix.mat.ref -- KAT-5 of tests/golden) ------------------------------------------------
// computeSymbols (:99-126): DETERMINE_TOP_DISTRIBS with a list of topDistribsCount entries on every selected frame, v[0].idx appended
// to `stream` -- one symbol per frame, in cluster order.
void computeSymbols(const SegCluster &selectedSegments, FeatureBuffer &fs, DeviceMixture &world, std::vector<unsigned long> &stream,
                    int topDistribsCount = 1, double minLLK = -200.0, double maxLLK = 200.0);
// computeConfusionMatrix (:69-97): mce_matrix(v[0].idx, v[i].idx)++ for i < nBest on every selected frame; mce_matrix is
// [distribCount x distribCount], row-major, ACCUMULATED into (the caller sizes and zeroes it, like mce_matrix.setDimensions at :144).
// nBest = topDistribsCount there (:132), so the list length and the loop bound are one number.
void computeConfusionMatrix(const SegCluster &selectedSegments, FeatureBuffer &fs, DeviceMixture &world, unsigned long nBest,
                            std::vector<unsigned long> &mce_matrix, double minLLK = -200.0, double maxLLK = 200.0);

// ---- EnergyDetector (LIA_SpkDet/EnergyDetector/src/EnergyDetector.cpp): a two / three-Gaussian model of the energy coefficient trained
// by FULL EM (weights, means AND variances) from a FIXED init -- no rand() -- then a threshold on that coefficient.  The one reference tool
// whose output (test/test1.validate.enr.lbl, KAT-6 of tests/golden, "assumed") depends on the variance estimate of getEM.
struct EnergyDetectorCfg {
    unsigned long nbTrainIt = 10, mixtureDistribCount = 3;
    double varianceFlooring = 0.5, varianceCeiling = 10.0, alpha = 0.0;
    std::string thresholdMode = "meanStd"; // :199-203; "weight" needs alize-core's Histo (not in the LIA_RAL tree): Exception
};
void energyMixtureInit(MixtureGD &world);                    // :163-183: means from -2 in steps of 4 / (distribCount - 1), covariances 1, equal weights
unsigned long findMaxEnergyDistrib(const MixtureGD &mixt);   // :83-93
// selectFrames (:118-157): segments of consecutive frames of `selectedSeg` whose coefficient 0 exceeds the threshold; begin / length count
// frames of the SELECTION (the reference's `ind`), and a run that reaches the end of an input segment is one frame longer than a run that
// ends inside it (:144 vs :151 -- reproduced as written).  energy[t] = coefficient 0 of frame t of the file.  Returns the frames above.
unsigned long selectFrames(const std::vector<float> &energy, double threshold, const SegCluster &selectedSeg, SegCluster &outputSeg);
// energyDetector (:190-285): globalMeanCov -> energyMixtureInit -> nbTrainIt x (accumulateStatEM, getEM, varianceControl) -> threshold
// = mean - alpha * sqrt(cov) of the highest-mean component -> selectFrames.  energyModel / threshold (optional) receive the trained model
// and the threshold.
SegCluster energyDetector(FeatureBuffer &fs, const SegCluster &selectedSegments, const EnergyDetectorCfg &cfg, MixtureGD *energyModel = nullptr,
                          double *threshold = nullptr);

// The same for ALL sources of the buffer in one device pass (gmmiv_energy_train + gmmiv_energy_select): selectedPerFile[s] is the cluster
// of input label segments of source s (Seg::begin counts from the source's first frame; Seg::source is ignored), the result [s] the output
// segments of source s (begin / length count frames of ITS selection, Seg::source = s).  One train call, a counting and a filling select
// call, and two downloads (the per-file results and counts; the segments) whatever the number of files.  models / thresholds / status
// (optional, one entry per source) receive the trained models, the thresholds and the GMMIV_ENERGY_* bit sets.  A buffer of vectSize > 1
// or a model of more than GMMIV_ENERGY_MAX_C Gaussians runs energyDetector per file; thresholdMode "weight" is the Exception it is there.
std::vector<SegCluster> energyDetectorBatch(FeatureBuffer &fs, const std::vector<SegCluster> &selectedPerFile, const EnergyDetectorCfg &cfg,
                                            std::vector<MixtureGD> *models = nullptr, std::vector<double> *thresholds = nullptr,
                                            std::vector<int> *status = nullptr);

// ---- NormFeat (LIA_SpkDet/NormFeat/src/NormFeat.cpp:231-518), the default mode: mean / std of the selected frames per segment
// (segmentalMode, :340-370) and / or per file (fileMode, :448-464; the mode when neither is set, :243), then computeZeroOne
// (GeneralTools.cpp:670-682) on those frames, in place in the resident buffer.  Both set: segmental first, then file (:272).
// cmsOnly: the std is replaced by 1 (:358); varOnly: the mean by 0 (:359); both: refused (:261).  extMean / extStd (both vectSize long,
// or both empty): externalStatsFilename's vectors replace the computed ones (:347-350, :451-453).
// windowMode (:372-447, include/gmmiv_feat_window.h): every selected segment by the statistics of a window of about windowDuration
// seconds of selected speech around it, blended with the file's by windowComp and how full the window is; frameLength turns frame
// indices into the truncated milliseconds the windows are counted in.  segmentalMode with it is refused (:241), ext vectors are
// ignored by it like the reference does, fileMode with it applies the file pass afterwards (:272, :448); alone it is NOT followed by
// the file pass (:243).  One plan on the host (gmmiv_plan_norm_windows) and one launch for all sources; a source is one workgroup, so
// a single long source runs on one compute unit.  A cluster whose segments overlap or are out of order is refused.
// warp (:362-368, :465-483, include/ext/gmmiv_feat_warp.h): every column of a unit -- a segment in segmentalMode, a source's selected
// cluster in fileMode -- through its own warpBinCount-bin histogram onto the target table of warpGaussHistoFilename (a Histo::save
// file; warpTarget, when not empty, is used instead of reading the file).  cmsOnly, varOnly and ext vectors with it are refused
// (:262-264).  warpAdd01Norm (:475-483): the mean / std pass over every source's cluster afterwards.  A column whose histogram has a bin
// without width is copied through (GMMIV_WARP_DEGENERATE).  Not built, refused with a message: warp with windowMode (its histograms
// read frames an earlier window has rewritten), and the rand()-made default target (a target must be named).  The segments of a
// cluster must be in increasing order and must not overlap.  Two launches for all sources.
struct Histo {                                 // alize-core's Histo as Histo::save writes it: bounds [nbBin + 1], count [nbBin]
    std::vector<double> bounds, count;
    bool empty() const { return count.empty(); }
};
struct NormFeatCfg {
    bool segmentalMode = false, fileMode = false, cmsOnly = false, varOnly = false;
    std::vector<double> extMean, extStd;
    bool windowMode = false;
    double windowDuration = 5, windowComp = 1, frameLength = 0.01;
    bool warp = false, warpAdd01Norm = false;
    unsigned long warpBinCount = 40;
    std::string warpGaussHistoFilename;
    Histo warpTarget;
};
// The host-only twin of warp's per-unit loop (tests and tools/bench_feat_warp.py; one core, no device): x [. x ld] float32, in place on
// the first D columns of the frames of runs [nrun x 3] = (first frame, length, unit), unit ids non-decreasing.  Per unit and column:
// the values sorted (the order of include/ext/gmmiv_feat_warp.h), the histogram, then warping() (ScoreWarp.cpp:168-206) loop for loop.
// status (optional) [nunits x D] receives 0 or GMMIV_WARP_DEGENERATE; such a column is left as it is.
void featWarpHost(float *x, unsigned long ld, int D, const std::vector<int64_t> &runs, int64_t nunits, unsigned long nbBin, const Histo &target,
                  std::vector<int> *status = nullptr);
// ALL sources of the buffer in one batch: selectedPerSource[s] is the cluster of selected segments of source s (Seg::begin counts
// from the source's first frame; Seg::source is ignored).  A pass is three enqueues on the whole batch -- gmmiv_frame_moments_groups,
// gmmiv_frame_moments_stats, gmmiv_feat_norm_apply, one group per segment or per source, runs cut at 4096 frames, all with device
// pointers; the host waits once, at the end of the pass, because its run table is uploaded from pageable memory.  Between the passes the frames are float32 (the resident type; the reference's writeFeature into its
// float buffer).  Segments of a cluster must not overlap (a label file's do not).  firstCol / nCols: the pass works on that column
// slice only (featureServerMask; nCols = 0: all columns from firstCol); ext vectors are then nCols long.
void normFeat(FeatureBuffer &fs, const std::vector<SegCluster> &selectedPerSource, const NormFeatCfg &cfg, unsigned long firstCol = 0,
              unsigned long nCols = 0);
// NormFeatWindowMode's normFeatOnlineMode (NormFeatWindowMode.cpp:165-311) on EVERY frame of every source (the tool uses no labels):
// running mean / std with the forgetting factor (windowDuration - 1) / windowDuration, started from windowDuration - initWithDelay zero
// vectors and the source's first initWithDelay frames (0: the tool without the parameter).  One enqueue (gmmiv_feat_norm_online).
void normFeatOnlineMode(FeatureBuffer &fs, long windowDuration = 300, long initWithDelay = 0);

// ---- TurnDetection (LIA_SpkSeg/TurnDetection/src/TurnDetection.cpp:101-287; the criterion of ClusteringCriterion.cpp:104-139, :807-927): every
// input segment longer than 2 winSize frames is walked by two adjacent windows of winSize frames in steps of winStep; a one-Gaussian model
// per window and of both, the criterion GLR / DGLR / BIC from their accumulated log-likelihoods; the curve is smoothed, and a position whose
// value stands out by alpha standard deviations from the minima to its left and right cuts the segment (include/gmmiv_turn.h has the rule).
// clusteringCrit "DELTABIC" (a split of the merged Gaussian and two EM iterations per position) is refused with a message.
struct TurnDetectionCfg {
    std::string clusteringCrit = "DGLR";
    unsigned long winSize = 50, winStep = 5;
    double alpha = 0.7, minLLK = -200.0, maxLLK = 200.0;
};
struct TurnCurve {                        // of one input segment; empty for a segment that is copied through
    std::vector<double> value, smoothed;
    std::vector<unsigned char> dec;
    double mean = NAN, std = NAN;
};
int turnCriterion(const std::string &clusteringCrit);   // GMMIV_TURN_*; throws on DELTABIC and on an unknown name
// The loop twin, HOST ONLY, one cluster: frames [nFrames x vectSize] float32, Seg::begin counts frames of that matrix.  The arithmetic is
// the reference's, in its order: FrameAccGD sums frame by frame, det = prod cov, cst = (2 pi)^(-D/2) / sqrt(det), lk = cst exp(-m / 2),
// log, the clamp (a likelihood that is 0 or not finite gives minLLK), accumulated frame by frame; then :184-279 as written.
SegCluster turnDetection(const float *frames, unsigned long nFrames, unsigned long vectSize, const SegCluster &cluster, const TurnDetectionCfg &cfg,
                         std::vector<TurnCurve> *curves = nullptr);
// ALL sources of the buffer in one device pass (gmmiv_turn_curve, gmmiv_turn_pick, a counting and a filling gmmiv_turn_segments):
// perFile[s] is the cluster of input segments of source s (Seg::begin counts from the source's first frame; Seg::source is ignored), the
// result [s] its output segments (begin from the source's first frame, Seg::source = s, Seg::labelCode = the input segment's).
// curves (optional) [s][segment] receives the curves and decisions.
std::vector<SegCluster> turnDetectionBatch(FeatureBuffer &fs, const std::vector<SegCluster> &perFile, const TurnDetectionCfg &cfg,
                                           std::vector<std::vector<TurnCurve> > *curves = nullptr);

// ---- AccumulateTVStat.h ----------------------------------------------------------------------------
class TVAcc {
  public:
    // ndx lines = statistics rows; row u owns the frames of segs[u] (TVAcc::_init, :129-196)
    TVAcc(GpuServer &srv, const MixtureGD &ubm, unsigned long rankT, unsigned long nSpeakers);
    void computeAndAccumulateTVStat(FeatureBuffer &fs, const std::vector<SegCluster> &segsPerLine); // :281-351
    // the same with the reference's file -> line map (TVTranslate::locIndices, :318-346): segsPerFile[f] = selected segments of
    // feature file f, filesOfLine[l] = the files listed on ndx line l (a file may be listed on several lines: it is evaluated
    // once and its statistics are added to each)
    void computeAndAccumulateTVStat(FeatureBuffer &fs, const std::vector<SegCluster> &segsPerFile,
                                    const std::vector<std::vector<unsigned long> > &filesOfLine);
    // initT, randomInitLaw "normal" (:729-748): T(i,j) = boxMuller(0,1) * (sum_k invvar_k) * 0.001 with the Box-Muller chain of
    // ScoreWarp.cpp:68-81 on glibc rand() (no srand: the caller's seed state, 1 by default); NaN / Inf draws are redrawn.  The
    // "uniform" law calls Matrix::randomInit of alize-core (not in the LIA_RAL tree): not reproduced, throws.
    void initT(const std::string &randomInitLaw = "normal");
    void substractM();                 // :1088-1105
    void estimateTETt();               // :777-805
    void estimateW();                  // :2114-2169
    void estimateAandC();              // :1702-1795
    void updateTestimate();            // :974-1005
    void minDivergence();              // :2056-2099
    void orthonormalizeT();            // :1548-1596
    // approximate extractors (IvExtractor modes ubmWeight / eigenDecomposition, IvExtractor.cpp:150-360)
    void normStatistics();             // :1225-1242
    void substractMplusTW();           // :1379-1399
    void normTMatrix();                // :1600-1609
    void getWeightedCov(std::vector<double> &W, const std::vector<double> &weight);       // :2837-2855, W [R x R]
    void approximateTcTc(std::vector<double> &D, const std::vector<double> &Q);            // :3116-3136, D [C x R] accumulated
    void estimateWUbmWeight(const std::vector<double> &W);                                 // :2348-2396 (zeroes _W first)
    void estimateWEigenDecomposition(const std::vector<double> &D, const std::vector<double> &Q); // :2566-2609 (accumulates into _W)
    void resetTmpAcc();                // :620-629
    void loadT(const std::vector<double> &T);
    void setStats(const std::vector<double> &N, const std::vector<double> &F);   // loadN / loadF (upload, no host copy kept)
    void setStats(const double *N, const double *F);
    // TotalVariability reloads N and F from disk at every iteration because substractM works in place
    // (TotalVariability.cpp:152-153); here the pristine statistics are kept on the device instead
    void storeStats();
    void restoreStats();
    void restoreStatsAndSubstractM();  // both steps of an iteration's start in one pass over F (gmmiv_tv_subtract_m_to)
    // Multi-GPU form of updateTestimate for utterance-sharded statistics: reduce-scatter of A / Cmx by blocks
    // of Gaussians, T_c = A_c^-1 Cmx_c on the rank's own Gaussians, all-gather of T; R, r and meanW (sums) are all-reduced
    // for minDivergence, whose session count becomes the global one.  comm == NULL or one rank: plain updateTestimate.
    void updateTestimate(gmmiv_comm *comm, unsigned long nSessionsAllRanks);
    // Overlapped exchange (option; bitwise the results of the serial order): with a communicator set here, estimateAandC()
    // accumulates A in the reduce-scatter's (block-padded) send buffer and BEGINS that reduce-scatter from the "tv_a_ready" hook of
    // gmmiv_tv_estimate_a_and_c -- it runs on the communicator's side stream under the Cmx GEMM -- and updateTestimate(comm, n)
    // leaves the all-gather of T in flight for minDivergence(), which joins it from the "md_factored" hook (after R is factored).
    // A caller that skips minDivergence() calls finishT() before anything reads T.  comm == NULL: serial order again.
    void setOverlap(gmmiv_comm *comm);
    void finishT();
    // The EM sanity check of TotalVariability (TotalVariability.cpp:132 `if (_checkLLK) tvAcc.verifyEMLK(config)`):
    //   getMplusTW (:964-971)      Sp = ubm_means + T^T w_spk  -- for a LIST of rows at once: one device pass, Sp [rows x svSize]
    //   getSpeakerModel (:1533-1545) the UBM with those means (svToModel, SuperVectors.cpp:79-85: means only)
    //   getLLK (:1626-1651)        mean clamped log-likelihood of the selected frames under a model (computeAndAccumulateLLK loop)
    //   verifyEMLK (:1654-1688)    sum over the first maxLLKcomputed files of getLLK(file's segments, speaker model of its row);
    //                              rowOfFile[f] = the statistics row (ndx line) file f belongs to; perFile (optional) = each llk
    void getMplusTW(std::vector<double> &Sp, const std::vector<unsigned long> &rows);
    void getSpeakerModel(MixtureGD &mixture, unsigned long spk);
    double getLLK(const SegCluster &selectedSegments, const MixtureGD &model, FeatureBuffer &fs, double minLLK = -200.0, double maxLLK = 200.0);
    double verifyEMLK(FeatureBuffer &fs, const std::vector<SegCluster> &segsPerFile, const std::vector<unsigned long> &rowOfFile,
                      unsigned long maxLLKcomputed, double minLLK = -200.0, double maxLLK = 200.0, std::vector<double> *perFile = nullptr);
    // all host views below download on demand (and re-upload before the next device step, they may be written through)
    std::vector<double> &getT() { return _T.host(); }
    std::vector<double> &getW() { return _W.host(); }
    std::vector<double> &getN() { return _statN.host(); }
    std::vector<double> &getF() { return _statF.host(); }
    std::vector<double> &getUbmMeans() { return _ubm_means.host(); }
    DVec &deviceT() { return _T; }
    DVec &deviceW() { return _W; }
    unsigned long getRankT() const { return _rankT; }

  private:
    GpuServer &_srv;
    MixtureGD _ubm;
    DeviceMixture _dubm;
    unsigned long _rankT, _n_speakers, _n_distrib, _vectSize, _svSize, _n_sessions_global;
    DVec _ubm_means, _ubm_invvar, _statN, _statF, _cN, _cF, _T, _W, _TETt, _A, _Cmx, _R, _r, _meanW;
    // overlapped exchange
    gmmiv_comm *_ovComm = nullptr;
    DVec _aMine, _tAll, _tMine;
    bool _aBegun = false, _tPending = false;
    static void hookAReady(void *self);
    static void hookMdFactored(void *self);
    void gatherIntoT();
};

// ---- AccumulateJFAStat.h: JFAAcc, M_{s,h} = m + V y_s + U x_h + D z_s (AccumulateJFAStat.cpp) ---------------------------
// Statistics rows: _matN / _F_X per speaker (ndx line), _N_h / _F_X_h per session (ndx element); sessions are grouped by
// speaker in ndx order.  L matrices are never stored: estimateAndInverseL_E{V,C} only mark the step, the build + inverse
// happens inside the estimate* call that consumes it, on the device (one workgroup per system).
class JFAAcc {
  public:
    JFAAcc(GpuServer &srv, const MixtureGD &ubm, unsigned long rankEV, unsigned long rankEC,
           const std::vector<unsigned long> &sessionsPerSpeaker);                          // _init, :168-300
    void computeAndAccumulateJFAStat(FeatureBuffer &fs, const std::vector<SegCluster> &segsPerSession); // :515-577
    void setStats(const std::vector<double> &N, const std::vector<double> &N_h, const std::vector<double> &F_X,
                  const std::vector<double> &F_X_h);                                       // loadN / loadN_h / loadF_X / loadF_X_h, :1025-1068
    void storeAccs();                  // :3777-3784
    void restoreAccs();                // :3786-3793
    void resetTmpAcc();                // :863-897
    void loadEV(const std::vector<double> &V);      // :949-968
    void loadEC(const std::vector<double> &U);      // :983-995
    void loadD(const std::vector<double> &D);       // :1016-1023
    void initD(double regulationFactor);            // initDType "MAP", :1214-1218
    void estimateVEVT();               // :1266-1352
    void estimateUEUT();               // :1425-1508
    void estimateAndInverseL_EV() {}   // :1970-1996 (fused into estimateYandV / estimateY)
    void estimateAndInverseL_EC() {}   // :2137-2163 (fused into estimateXandU / estimateX)
    void estimateYandV();              // :2467-2511
    void estimateY();                  // :2867-2957
    void estimateXandU();              // :3040-3083
    void estimateX();                  // :3262-3351
    void estimateZandD();              // :3480-3516
    void estimateZ();                  // :3550-3573
    void estimateZMAP(double tau);     // :3576-3594
    void updateVestimate();            // :3597-3619
    void updateUestimate();            // :3622-3644
    void substractMplusDZ();           // :3805-3822   _F_X   -= N   (m + D z)
    void substractMplusVY();           // :3988-4005   _F_X   -= N   (m + V y)
    void substractUX();                // :4152-4172   _F_X   -= sum_h N_h (U x_h)
    void substractMplusVYplusDZ();     // :4400-4422   _F_X_h -= N_h (m + V y + D z) of the session's speaker
    void substractMplusUX();           // :4336-4364   _F_X   -= sum_h N_h (m + U x_h)
    void substractMplusDZByChannel();  // :3948-3976   _F_X_h -= N_h (m + D z) of the session's speaker
    void orthonormalizeV();            // :4700-4777
    void getMplusVYplusDZ(std::vector<double> &Sp, unsigned long spk); // :1926-1935
    void getUX(std::vector<double> &ux, unsigned long session);        // :1803-1816 (ux += U(j, i) X(session, j); the index overload
                                                                       // :1788-1800 assigns instead of adding and keeps only the last j)
    void getSpeakerModel(MixtureGD &mixture, unsigned long session);   // :4605-4619: the means of m + V y + D z + U x_h
    // normalizeFeatures (:4623-4686) / substractUXfromFeatures (:4689-4697): o'_t = o_t - sum_c P(c | o_t) (U x_h)_c on the frames of every
    // session's cluster, with the full posterior of the session model.  The offsets U x_h and the session supervectors of ALL sessions
    // come from one product each; per session: the session model is set, the cluster's frames are selected, compensated in one call
    // of gmmiv_feat_compensate and scattered back -- one library call per session, not one per label segment.
    void normalizeFeatures(FeatureBuffer &fs, const std::vector<SegCluster> &segsPerSession);
    // The same for ALL sessions in one device pass (opt-in): the session models as one gmmiv_gmm_batch loaded from the device rows, the
    // selections of all sessions gathered once, session after session (the way adaptModelBatch / computeTestBatch lay theirs out), one
    // gmmiv_feat_compensate_models, one scatter.  A frame gets the bits normalizeFeatures gives it.  If the clusters of two sessions
    // share a frame the per-session loop depends on the order of the sessions and a single gather does not: such a list runs
    // normalizeFeatures.
    void normalizeFeaturesBatch(FeatureBuffer &fs, const std::vector<SegCluster> &segsPerSession);
    // the core of it on frames that are already gathered: rows [sessBegin[h], sessBegin[h + 1]) of x [n x vectSize] (device, float32)
    // are session h's; out (device) may be x or a matrix that does not overlap it.  fs: the buffer the frames came from (screening).
    void compensateSessions(const FeatureBuffer &fs, const float *x, unsigned long n, const std::vector<int64_t> &sessBegin, float *out);
    std::vector<double> &getV() { return _V.host(); }
    std::vector<double> &getU() { return _matU.host(); }
    std::vector<double> &getD() { return _D.host(); }
    std::vector<double> &getY() { return _Y.host(); }
    std::vector<double> &getX() { return _matX.host(); }
    std::vector<double> &getZ() { return _Z.host(); }
    std::vector<double> &getN() { return _matN.host(); }
    std::vector<double> &getN_h() { return _N_h.host(); }
    std::vector<double> &getF_X() { return _F_X.host(); }
    std::vector<double> &getF_X_h() { return _F_X_h.host(); }
    unsigned long getNSpeakers() const { return _n_speakers; }
    unsigned long getNSessions() const { return _n_sessions; }

  private:
    GpuServer &_srv;
    MixtureGD _ubm;
    DeviceMixture _dubm;
    unsigned long _rankEV, _rankEC, _n_speakers, _n_sessions, _n_distrib, _vectSize, _svSize;
    std::vector<int64_t> _sess_begin, _owner;
    DVec _ubm_means, _ubm_invvar, _matN, _N_h, _F_X, _F_X_h, _cN, _cN_h, _cF_X, _cF_X_h;
    DVec _V, _matU, _D, _Y, _matX, _Z, _vEvT, _uEuT, _Aev, _Cev, _Aec, _Cec, _mdR, _mdr, _mdmw; // _md*: minimum-divergence sums, unused by JFA
};
// host arithmetic of getUX / getSpeakerModel (no device): ux[i] = sum_j U[j][i] x[j] in the reference's order; sp = (m + vy + D z) + ux
void jfaUX(const double *U, const double *x, unsigned long rankEC, unsigned long svSize, double *ux);
void jfaSessionSupervector(const double *means, const double *V, const double *y, unsigned long rankEV, const double *Dm, const double *z,
                           const double *ux, unsigned long svSize, double *sp);
// featureMapping (GeneralTools.cpp:762-811, NormFeat.cpp:619): every frame of the cluster through its best Gaussian of the
// channel-dependent model cd to the same Gaussian of the channel-independent model ci, in place in the buffer
void featureMapping(MixtureGD &ci, MixtureGD &cd, FeatureBuffer &fs, const SegCluster &selectedSegments);
// the three training tools around it (statistics and initial matrices already in the accumulator)
void eigenVoice(JFAAcc &jfaAcc, unsigned long nbIt, bool orthonormalizeV);   // EigenVoice.cpp:114-147
void eigenChannel(JFAAcc &jfaAcc, unsigned long nbIt);                        // EigenChannel.cpp:118-160
void estimateDMatrix(JFAAcc &jfaAcc, unsigned long nbIt);                     // EstimateDMatrix.cpp:143-206
// ComputeTest in the JFA framework, dot-product scoring (ComputeTest.cpp:303-358): every statistics row of jfaAcc is one test
// segment (one session, y = z = 0); returns scores[nTest x nClients] = <client supervector, channel-compensated mean statistics>
std::vector<double> computeTestDotProduct(GpuServer &srv, JFAAcc &jfaAcc, const std::vector<double> &clientSV, unsigned long nClients);
// ComputeTest in the JFA framework, LLR scoring (ComputeTestJFA, ComputeTest.cpp:376-569) for a WHOLE ndx: per line the channel factor
// of the test file is estimated (statistics, estimateUEUT, substractMplusVYplusDZ, estimateX -- one speaker with one session per line,
// y = z = 0, so V and D play no part, as in the reference, where they multiply zero factors), its selected frames are compensated
// (o_t - sum_c gamma_tc (U x)_c under the model m + U x) and scored like computeTestBatch scores them: worldDecime = 1, one LLR per
// line and client.  All lines go through one statistics pass, one batched solve, one gmmiv_feat_compensate_models and one
// gmmiv_llr_trials.  fs is NOT rewritten: the compensation works on a copy of the gathered frames.  U [rankEC x C*D]; compensated
// (nullable): the compensated frames of all lines, line after line [n x D]; channelFactors (nullable): x of every line [L x rankEC].
std::vector<std::vector<double>> computeTestJFABatch(FeatureBuffer &fs, const std::vector<SegCluster> &selectedPerLine, const MixtureGD &world,
                                                     const std::vector<double> &U, unsigned long rankEC, DeviceMixture &dworld,
                                                     DeviceMixtureBatch &clientModels, const std::vector<std::vector<unsigned long>> &clientsPerLine,
                                                     int topDistribsCount, bool complete, double minLLK, double maxLLK,
                                                     std::vector<float> *compensated = nullptr, std::vector<double> *channelFactors = nullptr);

// ---- PldaTools.h: PldaDev, the development set of the i-vector back-end (PldaTools.cpp:274-2005) -------------
// _data [vectSize x n_sessions] (one i-vector per column), sessions grouped by speaker.
class PldaDev {
  public:
    PldaDev(GpuServer &srv, unsigned long vectSize, const std::vector<double> &data, const std::vector<unsigned long> &sessionPerSpeaker);
    unsigned long getVectSize() const { return _vectSize; }
    unsigned long getSpeakerNumber() const { return _session_per_speaker.size(); }
    unsigned long getSessionNumber() const { return _n_sessions; }
    unsigned long getSpeakerSessionNumber(unsigned long spk) const { return _session_per_speaker.at(spk); }
    std::vector<double> &getData() { return _data.host(); }   // host view, downloaded on demand
    DVec &deviceData() { return _data; }
    const std::vector<double> &getMean() const { return _mean; }
    const std::vector<double> &getSpeakerMeans() const { return _speaker_means; } // [vectSize x n_speakers]
    void computeAll();                                   // :353-387
    void lengthNorm();                                   // :436-463
    void center(const std::vector<double> &mu);          // :466-474
    void centerPerSpeaker();                             // :488-495 (means are NOT recomputed, like the reference)
    void rotateLeft(const std::vector<double> &M, unsigned long rows); // :498-513, M [rows x vectSize]
    void computeCovMat(std::vector<double> &Sigma, std::vector<double> &W, std::vector<double> &B);   // :527-566
    void computeWccnChol(std::vector<double> &WCCN);     // :1124-1176
    void computeMahalanobis(std::vector<double> &M);     // :1366-1378
    void computeScatterMat(std::vector<double> &SB, std::vector<double> &SW);                          // :1610-1644
    void computeLDA(std::vector<double> &ldaMat, unsigned long ldaRank, bool scatterMatrices = false);  // :1381-1413, [rank x vectSize]
    // :1822-1929: nbIt iterations of {covariances, EFR (Sigma) or sphNorm (W) matrix, center, rotate, lengthNorm};
    // the matrices and means of every iteration are returned instead of being written to files
    void sphericalNuisanceNormalization(unsigned long nbIt, bool sphNorm, std::vector<std::vector<double> > &mats,
                                        std::vector<std::vector<double> > &means);
    // one PldaModel::em_iteration on this set (used by PldaModel; the data is centred by Delta in place)
    void emIteration(unsigned long rankF, unsigned long rankG, std::vector<double> &F, std::vector<double> &G, std::vector<double> &Sigma,
                     std::vector<double> &Delta, const std::vector<int64_t> &sessionsPerSpeaker);
    // :1931-2005: apply stored matrices / means
    void applySphericalNuisanceNormalization(const std::vector<std::vector<double> > &mats, const std::vector<std::vector<double> > &means);

  private:
    std::vector<int64_t> sps64() const;
    GpuServer &_srv;
    unsigned long _vectSize, _n_sessions;
    DVec _data;                                   // [vectSize x n_sessions], device resident
    std::vector<double> _mean, _speaker_means;
    std::vector<unsigned long> _session_per_speaker;
};

// PldaModel in training mode (PldaTools.cpp:2043-2120, 2329-2343, 2790-2815).  The reference draws F and G at
// random when pldaLoadInitMatrices is false (initF / initG, glibc rand()); here they are always given, like its
// pldaLoadInitMatrices branch.
class PldaModel {
  public:
    PldaModel(PldaDev &dev, unsigned long rankF, unsigned long rankG, const std::vector<double> &F, const std::vector<double> &G,
              const std::vector<double> &Sigma);
    void em_iteration();                                        // :2329-2343
    std::vector<double> &getF() { return _F; }                  // [vectSize x rankF]
    std::vector<double> &getG() { return _G; }                  // [vectSize x rankG]
    std::vector<double> &getSigma() { return _Sigma; }          // [vectSize x vectSize]
    std::vector<double> &getDelta() { return _Delta; }          // minimum-divergence mean shift
    const std::vector<double> &getOriginalMean() const { return _originalMean; }
    unsigned long getRankF() const { return _rankF; }
    unsigned long getRankG() const { return _rankG; }

  private:
    PldaDev &_Dev;
    unsigned long _rankF, _rankG, _vectSize;
    std::vector<double> _F, _G, _Sigma, _Delta, _originalMean;
};

// ---- IvTest (LIA_SpkDet/IvTest/src/IvTest.cpp:73-471): normalisation estimated on a development set, applied to the
// enrolment and test vectors, then one of the four scoring rules.  Everything the reference exchanges through matrix
// files between the steps is kept in memory.
struct IvTestCfg {
    bool ivNorm = false;                  // ivNorm
    unsigned long ivNormIterationNb = 1;  // ivNormIterationNb
    bool sphNorm = false;                 // ivNormEfrMode == "sphNorm" (else EFR)
    bool LDA = false;                     // LDA
    unsigned long ldaRank = 0;            // ldaRank
    bool WCCN = false;                    // wccn (cosine scoring only)
    std::string scoring = "cosine";       // cosine | mahalanobis | 2cov | plda
    unsigned long pldaRankF = 0, pldaRankG = 0, pldaNbIt = 0; // pldaEigenVoiceNumber / pldaEigenChannelNumber / pldaNbIt
    // pldaScoring (IvTest.cpp:397-406): "native" scores the SUM of a model's vectors with its session count (pldaNativeScoring),
    // "enrollMean" their MEAN as one session (pldaMeanScoring, PldaTools.cpp:4612-4709).  Anything else is an Exception.
    std::string pldaScoring = "native";
};
// dev: development set (modified: normalised in place like the reference's PldaDev).
// enrol [dim x nEnrol] one enrolment vector per column, enrolPerModel[m] consecutive columns per model (cosine,
// mahalanobis and 2cov score the MEAN of a model's vectors, plda their sum with the session count, PldaTools.cpp:4206-4221);
// test [dim x nTest].  pldaF / pldaG / pldaSigma: initial matrices of the PLDA EM (ignored for the other rules).
// Returns scores [nModels x nTest].
std::vector<double> ivTest(GpuServer &srv, const IvTestCfg &cfg, PldaDev &dev, std::vector<double> enrol,
                           const std::vector<unsigned long> &enrolPerModel, std::vector<double> test, unsigned long nTest,
                           const std::vector<double> &pldaF, const std::vector<double> &pldaG, const std::vector<double> &pldaSigma);
// The same on a LIST of trials: trial i is model trialModel[i] against test vector trialSeg[i], in any order (include/gmmiv_iv_trials.h).
// Steps 1-4 (normalisation, back-end matrices, projection, one vector per model) are those of ivTest; only the listed pairs are
// scored, as cosineDistance / mahalanobisDistance do under _trials (PldaTools.cpp:3871, :3889).  Returns one score per trial, in list
// order: the cell [trialModel[i]][trialSeg[i]] of ivTest's matrix to the last bits of another summation order.
std::vector<double> ivTestTrials(GpuServer &srv, const IvTestCfg &cfg, PldaDev &dev, std::vector<double> enrol,
                                 const std::vector<unsigned long> &enrolPerModel, std::vector<double> test, unsigned long nTest,
                                 const std::vector<int32_t> &trialModel, const std::vector<int32_t> &trialSeg, const std::vector<double> &pldaF,
                                 const std::vector<double> &pldaG, const std::vector<double> &pldaSigma);

// ---- ComputeNorm (LIA_SpkDet/ComputeNorm/src/ComputeNorm.cpp:491-760) on resident score matrices ------------------------------
// The reference reads NIST result lines and keeps one DistribNorm per name; here the same four chains run on dense matrices
// that stay on the device (include/gmmiv.h, "score normalisation"):
//   X  [M  x S ]  the test scores (model m against test segment s), normalised IN PLACE
//   Z  [M  x Nz]  znormNistFile: the models against the impostor segments
//   T  [Nt x S ]  tnormNistFile: the t-norm cohort models against the test segments
//   ZT [Nt x Nz]  ztnormNistFile: the cohort models against the impostor segments
// normType "znorm" (:562-595) needs Z; "tnorm" (:530-561) T; "ztnorm" (:596-667) and "tznorm" (:668-751) all three.
// impostorIDList (selectImp, :436-445) is a list of COHORT-side names: impModels[Nt] flags the cohort models, impSegs[Nz] the
// impostor segments that are in it (empty vector: no selection).  Every pointer may be a host or a device pointer.
struct ComputeNormCfg {
    std::string normType = "znorm";     // znorm | tnorm | ztnorm | tznorm
    int meanMode = 0;                   // 0 mean / std, 1 median / mean absolute deviation
    double percentH = 0.0, percentL = 0.0; // share of the highest / lowest scores discarded
    std::vector<unsigned char> impModels, impSegs;
};
// firstOut: NULL, or [M x S] -- the t-normed scores of "ztnorm", the z-normed scores of "tznorm" (the reference writes both files)
void computeNorm(GpuServer &srv, const ComputeNormCfg &cfg, unsigned long M, unsigned long S, unsigned long Nt, unsigned long Nz,
                 double *X, const double *Z, const double *T, const double *ZT, double *firstOut = nullptr);

// ---- ComputeNorm on score LISTS: sparse trial lists and per-entity cohorts of different lengths -----------------------------------
// What the reference does by name (one DistribNorm per name, ComputeNorm.cpp:104-118, filled line by line, :446-489; two lookups per
// test line, :542-554, :576-589, :634-658, :717-742), by index: a list holds one distribution per value of its key field as a CSR
// table over a score array (include/gmmiv.h, "score normalisation on lists").  The impostorIDList selection is applied when a list
// is BUILT (loadComputeNormLists, io.h): cfg.impModels / cfg.impSegs are not looked at here.
//   z  znormNistFile:  a distribution per MODEL (its impostor-segment scores)       lineModel[i] names the one of test line i
//   t  tnormNistFile:  a distribution per TEST SEGMENT (its cohort-model scores)     lineSeg[i] names the one of test line i
//   zt ztnormNistFile: per IMPOSTOR SEGMENT for "ztnorm" (:618), per COHORT MODEL for "tznorm" (:697): the first-stage statistics
// `other` (by slot) names the zt distribution of the slot's second field; "ztnorm" needs it on z (:629), "tznorm" on t (:704).
struct ScoreListView {
    unsigned long ndist = 0;
    const int64_t *off = nullptr;    // HOST, ndist + 1
    const double *scores = nullptr;  // host or device
    unsigned long nscores = 0;
    const int64_t *pos = nullptr;    // host or device, by slot; NULL: slot k holds scores[k]
    const int32_t *other = nullptr;  // host or device, by slot
};
// x [n]: the scores of the test lines, normalised IN PLACE (host or device); firstOut: NULL, or [n] -- the t-normed scores of "ztnorm",
// the z-normed scores of "tznorm".  lineModel / lineSeg: host or device; the one a normType does not use may be NULL.
void computeNormLists(GpuServer &srv, const ComputeNormCfg &cfg, unsigned long n, double *x, const int32_t *lineModel, const int32_t *lineSeg,
                      const ScoreListView &z, const ScoreListView &t, const ScoreListView &zt, double *firstOut = nullptr);

// TVAcc::computeEigenProblem (AccumulateTVStat.cpp:2997-3102) for the SYMMETRIC matrices it is used on (the weighted
// covariance W): cyclic Jacobi on the host, eigenvalues sorted descending, eigenVect[k*rank + j] = component k of
// the j-th eigenvector (the reference's Eigen / LAPACK solver returns its own column order and sign; any orthonormal
// eigenbasis gives the same approximate i-vectors).  eigenVal [rank] holds the diagonal.
void computeEigenProblem(const std::vector<double> &EP, unsigned long n, std::vector<double> &eigenVect,
                         std::vector<double> &eigenVal, unsigned long rank);

} // namespace liagpu
