// io.h -- on-disk formats either side of the hot path, decoded from the
// reference's own fixtures; host-only, little-endian.
//   * feature files (.prm as shipped under LIA_SpkDet/*/test): 16-byte header of four u32
//     (2, base dimension, frame count, flags) + frames x dim float32; `featureServerMask`
//     ("0-15,17-32") selects columns like ALIZE's FeatureServer does
//     (LIA_SpkDet/ComputeTest/test/ComputeTest.cfg:28-29)
//   * label files (.lbl): "begin_s end_s label" per line; frame = time / frameLength and the end
//     frame is INCLUSIVE (LIA_SpkTools/src/SegTools.cpp:265-271)
//   * RAW mixture files (saveMixtureFileFormat RAW): u32 C, u32 D, f64 w[C], then per Gaussian
//     f64 cst, f64 det, u8 flag, f64 covInv[D], f64 mean[D]
//   * DT matrices (text): "rows cols" then the values, row-major (ComputeTest/test/zero.mat)
//   * score lines of the NIST-style result file (LIA_SpkTools/src/IOFormat.cpp:112-122), e.g.
//     "M test1 1 test3 0 0.26 5.06601" (LIA_SpkDet/ComputeTest/test/test1.validate.res)
#pragma once
#include <string>
#include <vector>

#include "liatools_gpu.h"

namespace liagpu {

std::vector<int> parseFeatureMask(const std::string &mask);             // "0-15,17-32" -> column list
struct FeatureFile {
    unsigned long nFrames = 0, vectSize = 0; // after masking
    unsigned baseDim = 0, flags = 0;
    std::vector<float> data;                 // [nFrames x vectSize]
};
FeatureFile readFeatureFile(const std::string &path, const std::string &mask = "");
void writeFeatureFile(const std::string &path, const FeatureFile &f);   // unmasked layout, same header

struct LabelSeg { double begin_s, end_s; std::string label; };
std::vector<LabelSeg> readLabelFile(const std::string &path);
SegCluster selectSegments(const std::vector<LabelSeg> &lab, const std::string &labelSelectedFrames, double frameLength,
                          unsigned long source = 0);

// Histo::save files (NormFeat/test/*.histo): a line nbBin, nbBin lines "lowerBound count", the last upper bound; written with the
// default ostream precision (%g), which is the precision of the reference's files.
Histo readHistoFile(const std::string &path);
void writeHistoFile(const std::string &path, const Histo &h);

MixtureGD readMixtureRAW(const std::string &path);
void writeMixtureRAW(const std::string &path, const MixtureGD &m);
// XML mixture files (saveMixtureFileFormat XML; fixture LIA_SpkDet/TrainWorld/test/wld.validate):
//   <MixtureGD version="1" id="#1" distribCount="C" vectSize="D"> / <DistribGD i weight cst det> / <covInv i>v</covInv> ... <mean i>v</mean>
// numbers carry 19 significant digits (%.19g).  weight / covInv / mean round-trip bit for bit; cst / det are recomputed from the
// covariances like DistribGD::computeAll does and agree with the file to rounding.
MixtureGD readMixtureXML(const std::string &path);
void writeMixtureXML(const std::string &path, const MixtureGD &m, const std::string &id = "#1");
MixtureGD readMixture(const std::string &path); // XML when the file starts with '<', else RAW

// (struct MatrixD { rows, cols, v } lives in liatools_gpu.h: computeMLLR returns one)
MatrixD readMatrixDT(const std::string &path);
void writeMatrixDT(const std::string &path, const MatrixD &m);
// DB matrices (saveMatrixFormat DB, the binary twin of DT written by alize-core's Matrix<double>::save): rows, cols, then
// rows * cols float64, little-endian.  The two extents are `unsigned long` members written with their own size: 8 bytes each
// from an LP64 build (Linux), 4 bytes each from a 32-bit / Windows build.  readMatrixDB accepts BOTH (the width is the one that
// makes the file size come out exactly); writeMatrixDB writes this platform's `unsigned long` width unless
// setMatrixDBHeaderBytes(4 | 8) says otherwise (returns the previous width).  alize-core is not part of the LIA_RAL tree and
// no DB file ships with it, so this layout is NOT pinned by a reference file; DT is (ComputeTest/test/zero.mat).
MatrixD readMatrixDB(const std::string &path);
void writeMatrixDB(const std::string &path, const MatrixD &m);
int setMatrixDBHeaderBytes(int bytes);
MatrixD readMatrix(const std::string &path, const std::string &format);   // "DT" | "DB" (loadMatrixFormat)
void writeMatrix(const std::string &path, const MatrixD &m, const std::string &format);
// Per-id vector files: TVAcc::saveWbyFile (AccumulateTVStat.cpp:2799-2822) writes row `session` of W as a 1 x rankT matrix to
// <saveVectorFilesPath><id><vectorFilesExtension>; PldaTest::load (PldaTools.cpp:3552-3588) reads <testVectorFilesPath>/<id><ext>
// back as column k of _models / _segments.
void saveVectorsById(const std::string &dir, const std::vector<std::string> &ids, const std::string &ext, const std::vector<double> &W,
                     unsigned long rank, const std::string &format = "DB");
// -> [dim x ids.size()] one vector per COLUMN (the layout of PldaTest::_models / _segments); dim from the first file
std::vector<double> loadVectorsById(const std::string &dir, const std::vector<std::string> &ids, const std::string &ext, unsigned long &dim,
                                    const std::string &format = "DB");

// gender, client id, decision ('1'/'0' by threshold), test file, [start end,] score
std::string resultLine(double llr, const std::string &clientName, const std::string &testName, const std::string &gender,
                       double threshold, bool withTimes = false, double start = 0.0, double end = 0.0);

// A NIST-style result line as the tools write it (resultLine above; outputResultLine of the reference): five fields separated
// by blanks, their POSITIONS configurable like the reference's fieldGender / fieldName / fieldDecision / fieldSeg / fieldLLR
// (ComputeNorm.cpp:520-524; a line written with start / end times has its score at position 6).
struct ResultFields { int fieldGender = 0, fieldName = 1, fieldDecision = 2, fieldSeg = 3, fieldLLR = 4; };
struct ResultLine { std::string gender, name, seg; int decision = 0; double llr = 0.0; };
ResultLine parseResultLine(const std::string &line, const ResultFields &f = ResultFields());   // throws on a missing field
std::vector<ResultLine> readResultFile(const std::string &path, const ResultFields &f = ResultFields()); // empty lines skipped

// ComputeNorm driven by files (ComputeNorm.cpp:491-760).  The lists must be FULL CROSS PRODUCTS -- every model of the test list
// against every test segment, every entity against the same cohort: that is what makes them dense matrices.  A ragged list (an
// entity whose cohort differs from the others') is refused with a message; the reference's per-name DistribNorm would accept it.
struct ComputeNormFilesCfg {
    ComputeNormCfg norm;                 // normType, meanMode, percentH, percentL (the masks are built from impostorIDList)
    std::string testNistFile, znormNistFile, tnormNistFile, ztnormNistFile, impostorIDList; // impostorIDList "": no selection
    std::string outputFileBaseName;
    std::string znormFilesExtension = ".znorm", tnormFilesExtension = ".tnorm", ztnormFilesExtension = ".ztnorm",
                tznormFilesExtension = ".tznorm";
    ResultFields fields;
};
struct ComputeNormTables {               // the lists as dense matrices, in order of first appearance
    std::vector<ResultLine> test;        // the test list, line by line (output order)
    std::vector<std::string> models, segs, cohortModels, impSegs;
    std::vector<double> X, Z, T, ZT;     // [models x segs], [models x impSegs], [cohortModels x segs], [cohortModels x impSegs]
    std::vector<unsigned long> lineRow, lineCol; // cell of X of each test line
    ComputeNormCfg norm;                 // cfg.norm with impModels / impSegs filled from impostorIDList
};
ComputeNormTables loadComputeNormTables(const ComputeNormFilesCfg &cfg);                 // host only
void computeNormFiles(GpuServer &srv, const ComputeNormFilesCfg &cfg, ComputeNormTables &tables); // normalise + write the output files
void computeNormFiles(GpuServer &srv, const ComputeNormFilesCfg &cfg);

// ComputeNorm driven by files, on LISTS: no cross product is asked for.  The four NIST files become CSR lists with the reference's
// semantics (getAllScores / getAllScoresFirstNormed, ComputeNorm.cpp:446-489): a distribution per value of the key field, its scores
// in FILE ORDER (the unsorted "median" of meanMode 1 without discards is the score at position n / 2 of that order), a line enters
// only if its OTHER field passes impostorIDList when one is given, a (model, segment) pair listed twice is two scores, names are
// indexed in order of first appearance.  A test line whose model or segment has no distribution, and a selected cohort line whose
// other field has no first-stage distribution, is an Exception that names it (the reference prints "... not found ..." and exits).
struct ScoreList {
    std::vector<std::string> keys;       // one per distribution
    std::vector<int64_t> off;            // keys.size() + 1
    std::vector<double> scores;          // by slot
    std::vector<int32_t> other;          // by slot: the first-stage distribution of the line's other field (second-stage list only)
};
struct ComputeNormLists {
    std::vector<ResultLine> test;        // the test list, line by line (output order)
    std::vector<double> x;               // its scores
    std::vector<int32_t> lineModel, lineSeg; // distribution of z / of t of each test line (empty when the normType does not use it)
    ScoreList z, t, zt;                  // znormNistFile by model; tnormNistFile by test segment; ztnormNistFile by impostor segment
                                         // ("ztnorm") or by cohort model ("tznorm")
    ComputeNormCfg norm;
};
ComputeNormLists loadComputeNormLists(const ComputeNormFilesCfg &cfg);                      // host only
void computeNormListFiles(GpuServer &srv, const ComputeNormFilesCfg &cfg, ComputeNormLists &lists); // normalise + write the output files
void computeNormListFiles(GpuServer &srv, const ComputeNormFilesCfg &cfg);

// IvTest driven by an ndx (PldaTest::load, PldaTools.cpp:3467-3620; the inputVectorFilename mode -- all against all -- stays with
// liagpu::ivTest).  Every line of the ndx is "segment model model ...".
//   without a targetIdList: a model is one vector, named by the ndx; models and segments are indexed in order of first appearance
//   with one:               its lines "model session session ..." define the models, read in DESCENDING order of their element count
//                           (XList::sortByElementNumber("descend"); the order of lines of equal count is alize-core's and cannot be
//                           read in the LIA_RAL tree: ASSUMED stable, i.e. file order).  A model named on several lines is one model
//                           with the sessions of all of them.  A trial whose model has no enrolment session is DROPPED and counted
//                           (the reference prints a warning and then indexes _trials with -1).
// The trial list has duplicates removed -- _trials is a matrix of flags -- and keeps the order of first appearance.
struct IvTestNdx {
    std::vector<std::string> models, segs;                 // ids, by index
    std::vector<std::vector<std::string> > sessions;       // the enrolment sessions of every model (the model's own id without a targetIdList)
    std::vector<int32_t> trialModel, trialSeg;             // the trials, duplicates removed
    unsigned long dropped = 0;                             // trials of the ndx whose model has no enrolment session
    unsigned long maxSessions = 1;                         // _n_enrollSessions_max
};
IvTestNdx loadIvTestNdx(const std::string &ndx, const std::string &targetIdList = ""); // host only
// IvTest from files: the vectors <vectorFilesPath>/<id><vectorFilesExtension> of the enrolment sessions and of the segments
// (loadVectorsById), the development set as it is given, liagpu::ivTestTrials on the ndx's trials, and the ASCII result file in the order
// of IvTest.cpp:430-437: segment-major, model index ascending, one resultLine per trial.  Returns the scores in that order.
struct IvTestFilesCfg {
    IvTestCfg test;
    std::string ndxFilename, targetIdList, vectorFilesPath, vectorFilesExtension = ".y", loadMatrixFormat = "DB";
    std::string outputFilename, gender = "M";
    double decisionThreshold = 0.0;
};
struct IvTestFilesResult {
    IvTestNdx ndx;
    std::vector<int32_t> lineModel, lineSeg;               // the trial of every output line
    std::vector<double> scores;                            // its score
};
IvTestFilesResult ivTestFiles(GpuServer &srv, const IvTestFilesCfg &cfg, PldaDev &dev, const std::vector<double> &pldaF = std::vector<double>(),
                              const std::vector<double> &pldaG = std::vector<double>(), const std::vector<double> &pldaSigma = std::vector<double>());

// NormFeat driven by files (NormFeat.cpp:302-509): every feature file <featureFilesPath><name><loadFeatureFileExtension> of the list is
// loaded at its full width into ONE resident buffer (the files must share their dimension), the clusters come from
// <labelFilesPath><name><labelFilesExtension> (labelFilesExtension "": no label files, every frame is selected), liagpu::normFeat runs
// once on the whole batch -- on the columns of featureServerMask: a contiguous mask is one column slice, a non-contiguous one a call per
// contiguous piece -- and <saveFeatureFilePath><name><saveFeatureFileExtension> receives the masked columns of all frames
// (writeAllFeatures, :489-495) or of the selected frames only, in cluster order (:497-498).
struct NormFeatFilesCfg {
    NormFeatCfg norm;
    std::string featureFilesPath, loadFeatureFileExtension = ".prm", saveFeatureFilePath, saveFeatureFileExtension = ".norm.prm";
    std::string labelFilesPath, labelFilesExtension = ".lbl", labelSelectedFrames = "speech", featureServerMask;
    double frameLength = 0.01;
    bool writeAllFeatures = true;
};
void normFeatFiles(GpuServer &srv, const std::vector<std::string> &names, const NormFeatFilesCfg &cfg);

// EnergyDetector driven by files (EnergyDetectorMain.cpp:104-131, EnergyDetector.cpp:200-279): every feature file
// <featureFilesPath><name><loadFeatureFileExtension> of the list is loaded through featureServerMask -- which picks the energy column --
// into ONE resident buffer, the input clusters come from <labelFilesPath><name><labelFilesExtension> (labelFilesExtension "": every frame
// of the file), liagpu::energyDetectorBatch runs once on the whole list, and <saveLabelFilePath><name><saveLabelFileExtension> receives one
// line "begin_s end_s labelOutputFrames" per output segment (outputLabelFile, SegTools.cpp:106-118: frameIdxToTime of begin and of
// begin + length - 1).  thresholds / status (optional): one entry per name.
struct EnergyDetectorFilesCfg {
    EnergyDetectorCfg energy;
    std::string featureFilesPath, loadFeatureFileExtension = ".prm", labelFilesPath, labelFilesExtension = ".lbl", labelSelectedFrames = "speech";
    std::string saveLabelFilePath, saveLabelFileExtension = ".enr.lbl", labelOutputFrames = "speech", featureServerMask;
    double frameLength = 0.01;
};
void energyDetectorFiles(GpuServer &srv, const std::vector<std::string> &names, const EnergyDetectorFilesCfg &cfg, std::vector<double> *thresholds = nullptr,
                         std::vector<int> *status = nullptr);

// TurnDetection driven by files (TurnDetection.cpp:292-349): every feature file of the list goes into ONE resident buffer, the input clusters
// come from <labelFilesPath><name><labelFilesExtension> (labelFilesExtension "": every frame of the file), liagpu::turnDetectionBatch runs
// once on the whole list, and <saveLabelFilePath><name><saveLabelFileExtension> receives one line "begin_s end_s label" per output segment,
// the label string of the input segment kept on its pieces (labelSelectedFrames: the cluster holds the segments of that label).
struct TurnDetectionFilesCfg {
    TurnDetectionCfg turn;
    std::string featureFilesPath, loadFeatureFileExtension = ".prm", labelFilesPath, labelFilesExtension = ".lbl", labelSelectedFrames = "speech";
    std::string saveLabelFilePath, saveLabelFileExtension = ".turn.lbl", featureServerMask;
    double frameLength = 0.01;
};
std::vector<SegCluster> turnDetectionFiles(GpuServer &srv, const std::vector<std::string> &names, const TurnDetectionFilesCfg &cfg);

} // namespace liagpu
