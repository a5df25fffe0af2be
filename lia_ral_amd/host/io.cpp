// io.cpp -- see io.h
#include "io.h"

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <map>
#include <sstream>

namespace liagpu {

static std::vector<unsigned char> slurp(const std::string &path)
{
    std::ifstream f(path.c_str(), std::ios::binary);
    if (!f) throw Exception("cannot open file [" + path + "]");
    return std::vector<unsigned char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

std::vector<int> parseFeatureMask(const std::string &mask)
{
    std::vector<int> cols;
    std::stringstream ss(mask);
    std::string tok;
    while (std::getline(ss, tok, ',')) {
        if (tok.empty()) continue;
        const size_t dash = tok.find('-');
        int a, b;
        if (dash == std::string::npos) a = b = atoi(tok.c_str());
        else { a = atoi(tok.substr(0, dash).c_str()); b = atoi(tok.substr(dash + 1).c_str()); }
        if (a < 0 || b < a) throw Exception("bad featureServerMask [" + mask + "]");
        for (int c = a; c <= b; ++c) cols.push_back(c);
    }
    return cols;
}

FeatureFile readFeatureFile(const std::string &path, const std::string &mask)
{
    const std::vector<unsigned char> b = slurp(path);
    if (b.size() < 16) throw Exception("feature file too short [" + path + "]");
    uint32_t h[4];
    memcpy(h, b.data(), 16);
    FeatureFile f;
    f.baseDim = h[1]; f.flags = h[3];
    const unsigned long n = h[2];
    if (n == 0) return f;
    if ((b.size() - 16) % (4 * n)) throw Exception("feature file size does not match its frame count [" + path + "]");
    const unsigned long dim = (b.size() - 16) / (4 * n);
    std::vector<int> cols = parseFeatureMask(mask);
    if (cols.empty()) for (unsigned long c = 0; c < dim; ++c) cols.push_back((int)c);
    for (int c : cols) if ((unsigned long)c >= dim) throw Exception("featureServerMask selects a column beyond vectSize");
    f.nFrames = n; f.vectSize = cols.size();
    f.data.resize(n * cols.size());
    const float *src = (const float *)(b.data() + 16);
    for (unsigned long t = 0; t < n; ++t)
        for (size_t k = 0; k < cols.size(); ++k) f.data[t * cols.size() + k] = src[t * dim + cols[k]];
    return f;
}

void writeFeatureFile(const std::string &path, const FeatureFile &f)
{
    std::ofstream o(path.c_str(), std::ios::binary);
    if (!o) throw Exception("cannot write [" + path + "]");
    const uint32_t h[4] = {2u, f.baseDim, (uint32_t)f.nFrames, f.flags};
    o.write((const char *)h, 16);
    o.write((const char *)f.data.data(), f.data.size() * sizeof(float));
}

Histo readHistoFile(const std::string &path)
{
    std::ifstream in(path.c_str());
    if (!in) throw Exception("cannot read [" + path + "]");
    long nb = 0;
    in >> nb;
    if (!in || nb < 1) throw Exception("[" + path + "] is not a histo file (bin count)");
    Histo h;
    h.bounds.resize((size_t)nb + 1); h.count.resize((size_t)nb);
    for (long i = 0; i < nb; ++i) in >> h.bounds[(size_t)i] >> h.count[(size_t)i];
    in >> h.bounds[(size_t)nb];
    if (!in) throw Exception("[" + path + "] is not a histo file (" + std::to_string(nb) + " bins announced)");
    return h;
}

void writeHistoFile(const std::string &path, const Histo &h)
{
    if (h.empty() || h.bounds.size() != h.count.size() + 1) throw Exception("writeHistoFile: bounds must be one longer than count");
    std::ofstream o(path.c_str(), std::ios::out | std::ios::trunc);
    if (!o) throw Exception("cannot write [" + path + "]");
    o << h.count.size() << "\n";
    for (size_t i = 0; i < h.count.size(); ++i) o << h.bounds[i] << "\t" << h.count[i] << "\n";
    o << h.bounds.back() << "\n";
}

std::vector<LabelSeg> readLabelFile(const std::string &path)
{
    std::ifstream f(path.c_str());
    if (!f) throw Exception("cannot open label file [" + path + "]");
    std::vector<LabelSeg> out;
    std::string line;
    while (std::getline(f, line)) {
        std::stringstream ss(line);
        LabelSeg s;
        if (ss >> s.begin_s >> s.end_s >> s.label) out.push_back(s);
    }
    return out;
}

SegCluster selectSegments(const std::vector<LabelSeg> &lab, const std::string &labelSelectedFrames, double frameLength,
                          unsigned long source)
{
    SegCluster c;
    for (const LabelSeg &l : lab)
        if (l.label == labelSelectedFrames) c.push_back(segFromLabel(l.begin_s, l.end_s, frameLength, source));
    return c;
}

MixtureGD readMixtureRAW(const std::string &path)
{
    const std::vector<unsigned char> b = slurp(path);
    if (b.size() < 8) throw Exception("mixture file too short [" + path + "]");
    uint32_t C, D;
    memcpy(&C, b.data(), 4);
    memcpy(&D, b.data() + 4, 4);
    const size_t rec = 17 + 16 * (size_t)D, want = 8 + 8 * (size_t)C + C * rec;
    if (C == 0 || D == 0 || b.size() != want) {
        char msg[256];
        snprintf(msg, sizeof(msg), "RAW mixture [%s]: %zu bytes, expected %zu for %u x %u (text-mode damaged file?)", path.c_str(),
                 b.size(), want, C, D);
        throw Exception(msg);
    }
    MixtureGD m(C, D);
    memcpy(m.weights().data(), b.data() + 8, 8 * (size_t)C);
    for (uint32_t c = 0; c < C; ++c) {
        const unsigned char *p = b.data() + 8 + 8 * (size_t)C + c * rec + 17; // skip cst, det, flag (recomputed)
        std::vector<double> civ(D), mu(D);
        memcpy(civ.data(), p, 8 * (size_t)D);
        memcpy(mu.data(), p + 8 * (size_t)D, 8 * (size_t)D);
        for (uint32_t d = 0; d < D; ++d) { m.setMean(c, mu[d], d); m.setCov(c, 1.0 / civ[d], d); }
    }
    m.computeAll();
    return m;
}

void writeMixtureRAW(const std::string &path, const MixtureGD &m)
{
    std::ofstream o(path.c_str(), std::ios::binary);
    if (!o) throw Exception("cannot write [" + path + "]");
    const uint32_t C = (uint32_t)m.getDistribCount(), D = (uint32_t)m.getVectSize();
    o.write((const char *)&C, 4);
    o.write((const char *)&D, 4);
    for (uint32_t c = 0; c < C; ++c) { const double w = m.weight(c); o.write((const char *)&w, 8); }
    for (uint32_t c = 0; c < C; ++c) {
        double det = 1.0;
        for (uint32_t d = 0; d < D; ++d) det *= m.getCov(c, d);
        const double cst = pow(2.0 * M_PI, -0.5 * D) / sqrt(det); // DistribGD::computeAll
        const unsigned char flag = 0;
        o.write((const char *)&cst, 8);
        o.write((const char *)&det, 8);
        o.write((const char *)&flag, 1);
        for (uint32_t d = 0; d < D; ++d) { const double v = m.getCovInv(c, d); o.write((const char *)&v, 8); }
        for (uint32_t d = 0; d < D; ++d) { const double v = m.getMean(c, d); o.write((const char *)&v, 8); }
    }
}

// ---- XML mixtures ---------------------------------------------------------------------------------------------------------
namespace {
// value of attribute `name` inside the tag text [b, e)
std::string xmlAttr(const std::string &t, size_t b, size_t e, const char *name, const std::string &path)
{
    const std::string key = std::string(name) + "=\"";
    const size_t p = t.find(key, b);
    if (p == std::string::npos || p >= e) throw Exception("XML mixture [" + path + "]: attribute " + name + " missing");
    const size_t q = t.find('"', p + key.size());
    if (q == std::string::npos || q > e) throw Exception("XML mixture [" + path + "]: unterminated attribute " + name);
    return t.substr(p + key.size(), q - p - key.size());
}
} // namespace

MixtureGD readMixtureXML(const std::string &path)
{
    const std::vector<unsigned char> raw = slurp(path);
    const std::string t(raw.begin(), raw.end());
    size_t pos = t.find("<MixtureGD");
    if (pos == std::string::npos) throw Exception("XML mixture [" + path + "]: no <MixtureGD> element");
    size_t end = t.find('>', pos);
    if (end == std::string::npos) throw Exception("XML mixture [" + path + "]: truncated header");
    const unsigned long C = strtoul(xmlAttr(t, pos, end, "distribCount", path).c_str(), nullptr, 10);
    const unsigned long D = strtoul(xmlAttr(t, pos, end, "vectSize", path).c_str(), nullptr, 10);
    if (!C || !D) throw Exception("XML mixture [" + path + "]: distribCount / vectSize must be positive");
    MixtureGD m(C, D);
    pos = end;
    for (unsigned long c = 0; c < C; ++c) {
        pos = t.find("<DistribGD", pos);
        if (pos == std::string::npos) throw Exception("XML mixture [" + path + "]: fewer <DistribGD> elements than distribCount");
        end = t.find('>', pos);
        if (strtoul(xmlAttr(t, pos, end, "i", path).c_str(), nullptr, 10) != c) throw Exception("XML mixture [" + path + "]: distributions out of order");
        m.weight(c) = strtod(xmlAttr(t, pos, end, "weight", path).c_str(), nullptr);
        const size_t close = t.find("</DistribGD>", end);
        if (close == std::string::npos) throw Exception("XML mixture [" + path + "]: unterminated <DistribGD>");
        for (int what = 0; what < 2; ++what) {
            const std::string tag = what == 0 ? "<covInv i=\"" : "<mean i=\"";
            size_t p = end;
            for (unsigned long d = 0; d < D; ++d) {
                p = t.find(tag, p);
                if (p == std::string::npos || p > close) throw Exception("XML mixture [" + path + "]: a distribution has fewer than vectSize entries");
                const unsigned long idx = strtoul(t.c_str() + p + tag.size(), nullptr, 10);
                const size_t v = t.find('>', p);
                if (idx >= D || v == std::string::npos) throw Exception("XML mixture [" + path + "]: bad entry index");
                const double val = strtod(t.c_str() + v + 1, nullptr);
                if (what == 0) m.setCovInv(c, val, idx); else m.setMean(c, val, idx);
                p = v;
            }
        }
        pos = close;
    }
    return m; // no computeAll(): the covInv bits of the file are kept
}

void writeMixtureXML(const std::string &path, const MixtureGD &m, const std::string &id)
{
    FILE *f = fopen(path.c_str(), "w");
    if (!f) throw Exception("cannot write [" + path + "]");
    const unsigned long C = m.getDistribCount(), D = m.getVectSize();
    fprintf(f, "<MixtureGD version=\"1\" id=\"%s\" distribCount=\"%lu\" vectSize=\"%lu\">\n", id.c_str(), C, D);
    for (unsigned long c = 0; c < C; ++c) {
        double det = 1.0;
        for (unsigned long d = 0; d < D; ++d) det *= m.getCov(c, d);
        const double cst = pow(2.0 * M_PI, -0.5 * D) / sqrt(det); // DistribGD::computeAll
        fprintf(f, "\t<DistribGD i=\"%lu\" weight=\"%.19g\" cst=\"%.19g\" det=\"%.19g\">\n", c, m.weight(c), cst, det);
        for (unsigned long d = 0; d < D; ++d) fprintf(f, "\t\t<covInv i=\"%lu\">%.19g</covInv>\n", d, m.getCovInv(c, d));
        for (unsigned long d = 0; d < D; ++d) fprintf(f, "\t\t<mean i=\"%lu\">%.19g</mean>\n", d, m.getMean(c, d));
        fprintf(f, "\t</DistribGD>\n");
    }
    fprintf(f, "</MixtureGD>\n");
    fclose(f);
}

MixtureGD readMixture(const std::string &path)
{
    std::ifstream f(path.c_str(), std::ios::binary);
    if (!f) throw Exception("cannot open [" + path + "]");
    char c = 0;
    while (f.get(c) && (c == ' ' || c == '\n' || c == '\r' || c == '\t')) {}
    return c == '<' ? readMixtureXML(path) : readMixtureRAW(path);
}

// ---- DB matrices and per-id vector files ------------------------------------------------------------------------------------
// Header width: alize-core's Matrix<T> keeps its extents in `unsigned long` members and (to the best of what can be told
// without its sources -- alize-core is not in the LIA_RAL tree and no DB file ships with it) writes them with sizeof(member):
// 2 x 8 bytes from an LP64 build (Linux / macOS), 2 x 4 bytes from an ILP32 or LLP64 build (32-bit, Windows).  The reader
// takes whichever width makes the file size come out exactly (ambiguity is impossible: with the wide header the upper halves
// are zero, which read as a 0-column matrix under the narrow interpretation -- only an empty matrix satisfies both, and both
// readings agree on it); the writer uses this platform's `unsigned long` like an upstream build here would, or the width
// asked for (setMatrixDBHeaderBytes(4 | 8)) when a file is meant for a build of the other kind.
static int g_db_header_bytes = (int)sizeof(unsigned long);
int setMatrixDBHeaderBytes(int bytes)
{
    const int prev = g_db_header_bytes;
    if (bytes == 4 || bytes == 8) g_db_header_bytes = bytes;
    return prev;
}
MatrixD readMatrixDB(const std::string &path)
{
    const std::vector<unsigned char> b = slurp(path);
    if (b.size() < 8) throw Exception("DB matrix too short [" + path + "]");
    uint64_t r = 0, c = 0;
    size_t hdr = 0;
    if (b.size() >= 16) { // LP64 writer: two 8-byte extents
        uint64_t r8, c8;
        memcpy(&r8, b.data(), 8);
        memcpy(&c8, b.data() + 8, 8);
        if (r8 <= (1ull << 40) && c8 <= (1ull << 40) && (r8 == 0 || c8 <= (~(size_t)0 - 16) / 8 / r8) && b.size() == 16 + 8 * (size_t)r8 * (size_t)c8) { r = r8; c = c8; hdr = 16; }
    }
    if (!hdr) {           // ILP32 / LLP64 writer: two 4-byte extents
        uint32_t r4, c4;
        memcpy(&r4, b.data(), 4);
        memcpy(&c4, b.data() + 4, 4);
        if (b.size() == 8 + 8 * (size_t)r4 * c4) { r = r4; c = c4; hdr = 8; }
    }
    if (!hdr) {
        uint32_t r4, c4;
        memcpy(&r4, b.data(), 4);
        memcpy(&c4, b.data() + 4, 4);
        char msg[320];
        snprintf(msg, sizeof(msg), "DB matrix [%s]: %zu bytes fit neither an 8-byte-extent header nor a 4-byte one (%u x %u would need %zu)",
                 path.c_str(), b.size(), r4, c4, 8 + 8 * (size_t)r4 * c4);
        throw Exception(msg);
    }
    MatrixD m;
    m.rows = (unsigned long)r; m.cols = (unsigned long)c;
    m.v.resize((size_t)r * c);
    if (!m.v.empty()) memcpy(m.v.data(), b.data() + hdr, 8 * m.v.size());
    return m;
}
void writeMatrixDB(const std::string &path, const MatrixD &m)
{
    std::ofstream o(path.c_str(), std::ios::binary);
    if (!o) throw Exception("cannot write [" + path + "]");
    if (g_db_header_bytes == 8) {
        const uint64_t r = (uint64_t)m.rows, c = (uint64_t)m.cols;
        o.write((const char *)&r, 8);
        o.write((const char *)&c, 8);
    } else {
        const uint32_t r = (uint32_t)m.rows, c = (uint32_t)m.cols;
        o.write((const char *)&r, 4);
        o.write((const char *)&c, 4);
    }
    if (!m.v.empty()) o.write((const char *)m.v.data(), 8 * m.v.size());
}
MatrixD readMatrix(const std::string &path, const std::string &format)
{
    if (format == "DT") return readMatrixDT(path);
    if (format == "DB") return readMatrixDB(path);
    throw Exception("unknown matrix format [" + format + "]");
}
void writeMatrix(const std::string &path, const MatrixD &m, const std::string &format)
{
    if (format == "DT") writeMatrixDT(path, m);
    else if (format == "DB") writeMatrixDB(path, m);
    else throw Exception("unknown matrix format [" + format + "]");
}

void saveVectorsById(const std::string &dir, const std::vector<std::string> &ids, const std::string &ext, const std::vector<double> &W,
                     unsigned long rank, const std::string &format)
{
    if (W.size() != ids.size() * rank) throw Exception("saveVectorsById: W must hold one row of `rank` values per id");
    for (size_t s = 0; s < ids.size(); ++s) { // one 1 x rank matrix per id, in list order (saveWbyFile: session++)
        MatrixD y;
        y.rows = 1; y.cols = rank;
        y.v.assign(W.begin() + s * rank, W.begin() + (s + 1) * rank);
        writeMatrix(dir + ids[s] + ext, y, format);
    }
}
std::vector<double> loadVectorsById(const std::string &dir, const std::vector<std::string> &ids, const std::string &ext, unsigned long &dim,
                                    const std::string &format)
{
    dim = 0;
    std::vector<double> out;
    for (size_t k = 0; k < ids.size(); ++k) {
        const MatrixD v = readMatrix(dir + "/" + ids[k] + ext, format);
        if (k == 0) { dim = v.cols; out.assign((size_t)dim * ids.size(), 0.0); } // _vectSize = tmpVect.cols() of the first file
        if (v.rows < 1 || v.cols != dim) throw Exception("vector file [" + ids[k] + ext + "]: expected 1 x " + std::to_string(dim));
        for (unsigned long i = 0; i < dim; ++i) out[i * ids.size() + k] = v.v[i]; // _models(k, m) = tmpVect(0, k)
    }
    return out;
}

MatrixD readMatrixDT(const std::string &path)
{
    std::ifstream f(path.c_str());
    if (!f) throw Exception("cannot open matrix [" + path + "]");
    MatrixD m;
    if (!(f >> m.rows >> m.cols)) throw Exception("bad DT matrix header [" + path + "]");
    m.v.resize(m.rows * m.cols);
    for (double &x : m.v)
        if (!(f >> x)) throw Exception("DT matrix truncated [" + path + "]");
    return m;
}

void writeMatrixDT(const std::string &path, const MatrixD &m)
{
    FILE *f = fopen(path.c_str(), "w");
    if (!f) throw Exception("cannot write [" + path + "]");
    fprintf(f, "%lu %lu\n", m.rows, m.cols);
    for (unsigned long i = 0; i < m.rows; ++i) {
        for (unsigned long j = 0; j < m.cols; ++j) fprintf(f, "%.17g ", m.v[i * m.cols + j]);
        fprintf(f, "\n");
    }
    fclose(f);
}

std::string resultLine(double llr, const std::string &clientName, const std::string &testName, const std::string &gender,
                       double threshold, bool withTimes, double start, double end)
{
    std::ostringstream o;
    o << gender << " " << clientName << " " << (llr > threshold ? 1 : 0) << " " << testName << " ";
    if (withTimes) o << start << " " << end << " ";
    o << llr;
    return o.str();
}

// ---- NIST result lines in, ComputeNorm on files -----------------------------------------------------------------------------
ResultLine parseResultLine(const std::string &line, const ResultFields &f)
{
    std::vector<std::string> tok;
    std::istringstream in(line);
    for (std::string t; in >> t;) tok.push_back(t);
    auto at = [&](int i, const char *what) -> const std::string & {
        if (i < 0 || (size_t)i >= tok.size()) throw Exception(std::string("result line [") + line + "] has no field " + std::to_string(i) + " (" + what + ")");
        return tok[(size_t)i];
    };
    ResultLine r;
    r.gender = at(f.fieldGender, "fieldGender");
    r.name = at(f.fieldName, "fieldName");
    r.seg = at(f.fieldSeg, "fieldSeg");
    if (f.fieldDecision >= 0 && (size_t)f.fieldDecision < tok.size()) r.decision = atoi(tok[(size_t)f.fieldDecision].c_str());
    const std::string &v = at(f.fieldLLR, "fieldLLR");
    char *end = nullptr;
    r.llr = strtod(v.c_str(), &end);
    if (end == v.c_str()) throw Exception("result line [" + line + "]: field " + std::to_string(f.fieldLLR) + " is not a score");
    return r;
}

std::vector<ResultLine> readResultFile(const std::string &path, const ResultFields &f)
{
    std::ifstream in(path.c_str());
    if (!in) throw Exception("cannot read [" + path + "]");
    std::vector<ResultLine> out;
    for (std::string line; std::getline(in, line);) {
        if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
        out.push_back(parseResultLine(line, f));
    }
    return out;
}

namespace {
unsigned long indexOf(std::vector<std::string> &names, std::map<std::string, unsigned long> &idx, const std::string &n, bool grow,
                      const std::string &path, const char *what)
{
    auto it = idx.find(n);
    if (it != idx.end()) return it->second;
    if (!grow) throw Exception("[" + path + "]: " + what + " [" + n + "] does not occur in the other lists: not a full cross product");
    idx[n] = names.size();
    names.push_back(n);
    return names.size() - 1;
}
// rows / cols: the names seen so far (fixed == true: the list must use exactly these); -> dense [rows x cols]
std::vector<double> denseFromLines(const std::vector<ResultLine> &lines, const std::string &path, std::vector<std::string> &rows,
                                   bool rowsFixed, std::vector<std::string> &cols, bool colsFixed, std::vector<unsigned long> *lineRow,
                                   std::vector<unsigned long> *lineCol)
{
    std::map<std::string, unsigned long> ri, ci;
    for (size_t i = 0; i < rows.size(); ++i) ri[rows[i]] = i;
    for (size_t i = 0; i < cols.size(); ++i) ci[cols[i]] = i;
    std::vector<unsigned long> lr(lines.size()), lc(lines.size());
    for (size_t l = 0; l < lines.size(); ++l) {
        lr[l] = indexOf(rows, ri, lines[l].name, !rowsFixed, path, "model");
        lc[l] = indexOf(cols, ci, lines[l].seg, !colsFixed, path, "segment");
    }
    const size_t R = rows.size(), C = cols.size();
    if (lines.size() != R * C)
        throw Exception("[" + path + "]: " + std::to_string(lines.size()) + " lines for " + std::to_string(R) + " models x " + std::to_string(C) +
                        " segments: not a full cross product (ragged cohorts are not supported)");
    std::vector<double> out(R * C);
    std::vector<bool> seen(R * C, false);
    for (size_t l = 0; l < lines.size(); ++l) {
        const size_t k = lr[l] * C + lc[l];
        if (seen[k]) throw Exception("[" + path + "]: model [" + lines[l].name + "] meets segment [" + lines[l].seg + "] twice: not a full cross product");
        seen[k] = true;
        out[k] = lines[l].llr;
    }
    if (lineRow) *lineRow = lr;
    if (lineCol) *lineCol = lc;
    return out;
}
} // namespace

ComputeNormTables loadComputeNormTables(const ComputeNormFilesCfg &cfg)
{
    ComputeNormTables t;
    t.norm = cfg.norm;
    const std::string &nt = cfg.norm.normType;
    const bool zn = nt == "znorm", tn = nt == "tnorm", two = nt == "ztnorm" || nt == "tznorm";
    if (!zn && !tn && !two) throw Exception("unknown normalization mode:" + nt);
    t.test = readResultFile(cfg.testNistFile, cfg.fields);
    t.X = denseFromLines(t.test, cfg.testNistFile, t.models, false, t.segs, false, &t.lineRow, &t.lineCol);
    if (zn || two) t.Z = denseFromLines(readResultFile(cfg.znormNistFile, cfg.fields), cfg.znormNistFile, t.models, true, t.impSegs, false, nullptr, nullptr);
    if (tn || two) t.T = denseFromLines(readResultFile(cfg.tnormNistFile, cfg.fields), cfg.tnormNistFile, t.cohortModels, false, t.segs, true, nullptr, nullptr);
    if (two) t.ZT = denseFromLines(readResultFile(cfg.ztnormNistFile, cfg.fields), cfg.ztnormNistFile, t.cohortModels, true, t.impSegs, true, nullptr, nullptr);
    if (!cfg.impostorIDList.empty()) { // selectMode 1 (:511-514): a cohort-side name enters only if the list has it
        std::ifstream in(cfg.impostorIDList.c_str());
        if (!in) throw Exception("cannot read [" + cfg.impostorIDList + "]");
        std::map<std::string, int> ids;
        for (std::string w; in >> w;) ids[w] = 1;
        t.norm.impModels.assign(t.cohortModels.size(), 0);
        t.norm.impSegs.assign(t.impSegs.size(), 0);
        for (size_t i = 0; i < t.cohortModels.size(); ++i) t.norm.impModels[i] = ids.count(t.cohortModels[i]) ? 1 : 0;
        for (size_t i = 0; i < t.impSegs.size(); ++i) t.norm.impSegs[i] = ids.count(t.impSegs[i]) ? 1 : 0;
    }
    return t;
}

void computeNormFiles(GpuServer &srv, const ComputeNormFilesCfg &cfg, ComputeNormTables &t)
{
    const std::string &nt = t.norm.normType;
    const bool two = nt == "ztnorm" || nt == "tznorm";
    std::vector<double> first(two ? t.X.size() : 0);
    computeNorm(srv, t.norm, t.models.size(), t.segs.size(), t.cohortModels.size(), t.impSegs.size(), t.X.data(),
                t.Z.empty() ? nullptr : t.Z.data(), t.T.empty() ? nullptr : t.T.data(), t.ZT.empty() ? nullptr : t.ZT.data(),
                two ? first.data() : nullptr);
    srv.sync();
    auto write = [&](const std::string &ext, const std::vector<double> &v) {
        const std::string path = cfg.outputFileBaseName + ext;
        std::ofstream out(path.c_str(), std::ios::out | std::ios::trunc);
        if (!out) throw Exception("cannot write [" + path + "]");
        out.precision(17);
        const size_t S = t.segs.size();
        for (size_t l = 0; l < t.test.size(); ++l) { // decision 0 like the reference (:497)
            const double sc = v[t.lineRow[l] * S + t.lineCol[l]];
            out << t.test[l].gender << " " << t.test[l].name << " 0 " << t.test[l].seg << " " << sc << "\n";
        }
    };
    if (nt == "znorm") write(cfg.znormFilesExtension, t.X);
    else if (nt == "tnorm") write(cfg.tnormFilesExtension, t.X);
    else if (nt == "ztnorm") { write(cfg.ztnormFilesExtension, t.X); write(cfg.tnormFilesExtension, first); }   // :656-657
    else { write(cfg.tznormFilesExtension, t.X); write(cfg.znormFilesExtension, first); }                        // :738-739
}

void computeNormFiles(GpuServer &srv, const ComputeNormFilesCfg &cfg)
{
    ComputeNormTables t = loadComputeNormTables(cfg);
    computeNormFiles(srv, cfg, t);
}

// ---- ComputeNorm on files, as lists -------------------------------------------------------------------------------------------
namespace {
// getAllScores (:446-462) / getAllScoresFirstNormed (:466-489): key = fieldOne, the filter and the first-stage lookup use fieldTwo
ScoreList buildScoreList(const std::vector<ResultLine> &lines, const std::string &path, bool keyIsSeg, const std::map<std::string, int> *ids,
                         const ScoreList *first)
{
    ScoreList l;
    std::map<std::string, unsigned long> ki, fi;
    if (first)
        for (size_t i = 0; i < first->keys.size(); ++i) fi[first->keys[i]] = i;
    std::vector<unsigned long> key(lines.size());
    std::vector<char> in(lines.size(), 0);
    std::vector<int64_t> cnt;
    for (size_t i = 0; i < lines.size(); ++i) {
        const std::string &one = keyIsSeg ? lines[i].seg : lines[i].name, &two = keyIsSeg ? lines[i].name : lines[i].seg;
        if (ids && !ids->count(two)) continue; // selectImp, :436-445
        if (first && !fi.count(two)) throw Exception("[" + path + "]: distribution for [" + two + "] not found (line of [" + one + "])"); // :483
        auto it = ki.find(one);
        if (it == ki.end()) { it = ki.insert(std::make_pair(one, (unsigned long)l.keys.size())).first; l.keys.push_back(one); cnt.push_back(0); }
        key[i] = it->second;
        in[i] = 1;
        cnt[it->second]++;
    }
    l.off.assign(l.keys.size() + 1, 0);
    for (size_t d = 0; d < l.keys.size(); ++d) l.off[d + 1] = l.off[d] + cnt[d];
    l.scores.resize((size_t)l.off.back());
    if (first) l.other.resize((size_t)l.off.back());
    std::vector<int64_t> at(l.off.begin(), l.off.end() - 1);
    for (size_t i = 0; i < lines.size(); ++i) { // file order inside a distribution
        if (!in[i]) continue;
        const int64_t k = at[key[i]]++;
        l.scores[(size_t)k] = lines[i].llr;
        if (first) l.other[(size_t)k] = (int32_t)fi[keyIsSeg ? lines[i].name : lines[i].seg];
    }
    return l;
}
} // namespace

ComputeNormLists loadComputeNormLists(const ComputeNormFilesCfg &cfg)
{
    ComputeNormLists t;
    t.norm = cfg.norm;
    t.norm.impModels.clear(); // the selection is applied here, line by line
    t.norm.impSegs.clear();
    const std::string &nt = cfg.norm.normType;
    const bool zn = nt == "znorm", tn = nt == "tnorm", ztn = nt == "ztnorm", tzn = nt == "tznorm";
    if (!zn && !tn && !ztn && !tzn) throw Exception("unknown normalization mode:" + nt);
    std::map<std::string, int> idsMap;
    const std::map<std::string, int> *ids = nullptr;
    if (!cfg.impostorIDList.empty()) { // selectMode 1 (:511-514)
        std::ifstream in(cfg.impostorIDList.c_str());
        if (!in) throw Exception("cannot read [" + cfg.impostorIDList + "]");
        for (std::string w; in >> w;) idsMap[w] = 1;
        ids = &idsMap;
    }
    t.test = readResultFile(cfg.testNistFile, cfg.fields);
    auto lines = [&](const std::string &path) { return readResultFile(path, cfg.fields); };
    if (zn) t.z = buildScoreList(lines(cfg.znormNistFile), cfg.znormNistFile, false, ids, nullptr);                 // :573
    else if (tn) t.t = buildScoreList(lines(cfg.tnormNistFile), cfg.tnormNistFile, true, ids, nullptr);             // :537
    else if (ztn) {
        t.zt = buildScoreList(lines(cfg.ztnormNistFile), cfg.ztnormNistFile, true, ids, nullptr);                    // :618
        t.t = buildScoreList(lines(cfg.tnormNistFile), cfg.tnormNistFile, true, ids, nullptr);                       // :623
        t.z = buildScoreList(lines(cfg.znormNistFile), cfg.znormNistFile, false, ids, &t.zt);                        // :629
    } else {
        t.z = buildScoreList(lines(cfg.znormNistFile), cfg.znormNistFile, false, ids, nullptr);                      // :690
        t.zt = buildScoreList(lines(cfg.ztnormNistFile), cfg.ztnormNistFile, false, ids, nullptr);                   // :697
        t.t = buildScoreList(lines(cfg.tnormNistFile), cfg.tnormNistFile, true, ids, &t.zt);                         // :704
    }
    std::map<std::string, int32_t> zi, ti;
    for (size_t i = 0; i < t.z.keys.size(); ++i) zi[t.z.keys[i]] = (int32_t)i;
    for (size_t i = 0; i < t.t.keys.size(); ++i) ti[t.t.keys[i]] = (int32_t)i;
    t.x.resize(t.test.size());
    if (!tn) t.lineModel.resize(t.test.size());
    if (!zn) t.lineSeg.resize(t.test.size());
    for (size_t l = 0; l < t.test.size(); ++l) { // the two lookups of every test line (:547, :582, :642-650, :725-732)
        t.x[l] = t.test[l].llr;
        if (!tn) {
            auto it = zi.find(t.test[l].name);
            if (it == zi.end()) throw Exception("[" + cfg.testNistFile + "]: znorm distribution not found for id [" + t.test[l].name + "]");
            t.lineModel[l] = it->second;
        }
        if (!zn) {
            auto it = ti.find(t.test[l].seg);
            if (it == ti.end()) throw Exception("[" + cfg.testNistFile + "]: tnorm distribution not found for seg [" + t.test[l].seg + "]");
            t.lineSeg[l] = it->second;
        }
    }
    return t;
}

void computeNormListFiles(GpuServer &srv, const ComputeNormFilesCfg &cfg, ComputeNormLists &t)
{
    const std::string &nt = t.norm.normType;
    const bool two = nt == "ztnorm" || nt == "tznorm";
    std::vector<double> first(two ? t.x.size() : 0);
    auto view = [](const ScoreList &l) {
        ScoreListView v;
        v.ndist = l.keys.size(); v.off = l.off.empty() ? nullptr : l.off.data(); v.scores = l.scores.data(); v.nscores = l.scores.size();
        v.other = l.other.empty() ? nullptr : l.other.data();
        return v;
    };
    computeNormLists(srv, t.norm, t.x.size(), t.x.data(), t.lineModel.empty() ? nullptr : t.lineModel.data(),
                     t.lineSeg.empty() ? nullptr : t.lineSeg.data(), view(t.z), view(t.t), view(t.zt), two ? first.data() : nullptr);
    srv.sync();
    auto write = [&](const std::string &ext, const std::vector<double> &v) {
        const std::string path = cfg.outputFileBaseName + ext;
        std::ofstream out(path.c_str(), std::ios::out | std::ios::trunc);
        if (!out) throw Exception("cannot write [" + path + "]");
        out.precision(17);
        for (size_t l = 0; l < t.test.size(); ++l) // test-list order; the line of computeNormFiles: decision 0 like the reference (:497), 17 digits
            out << t.test[l].gender << " " << t.test[l].name << " 0 " << t.test[l].seg << " " << v[l] << "\n";
    };
    if (nt == "znorm") write(cfg.znormFilesExtension, t.x);
    else if (nt == "tnorm") write(cfg.tnormFilesExtension, t.x);
    else if (nt == "ztnorm") { write(cfg.ztnormFilesExtension, t.x); write(cfg.tnormFilesExtension, first); }   // :656-657
    else { write(cfg.tznormFilesExtension, t.x); write(cfg.znormFilesExtension, first); }                        // :738-739
}

void computeNormListFiles(GpuServer &srv, const ComputeNormFilesCfg &cfg)
{
    ComputeNormLists t = loadComputeNormLists(cfg);
    computeNormListFiles(srv, cfg, t);
}

// ---- NormFeat from files ------------------------------------------------------------------------------
void normFeatFiles(GpuServer &srv, const std::vector<std::string> &names, const NormFeatFilesCfg &cfg)
{
    if (names.empty()) return;
    std::vector<FeatureFile> files;
    std::vector<unsigned long> first;
    std::vector<SegCluster> clusters;
    unsigned long total = 0, dim = 0;
    for (size_t k = 0; k < names.size(); ++k) {
        files.push_back(readFeatureFile(cfg.featureFilesPath + names[k] + cfg.loadFeatureFileExtension));
        const FeatureFile &f = files.back();
        if (f.nFrames) {
            if (dim && f.vectSize != dim) throw Exception("normFeatFiles: [" + names[k] + "] has another dimension than the files before it");
            dim = f.vectSize;
        }
        first.push_back(total);
        total += f.nFrames;
        SegCluster c;
        if (cfg.labelFilesExtension.empty()) { Seg all; all.begin = 0; all.length = f.nFrames; all.source = k; if (f.nFrames) c.push_back(all); }
        else c = selectSegments(readLabelFile(cfg.labelFilesPath + names[k] + cfg.labelFilesExtension), cfg.labelSelectedFrames, cfg.frameLength, k);
        for (const Seg &g : c)
            if (g.begin + g.length > f.nFrames) throw Exception("normFeatFiles: a segment of [" + names[k] + "] ends after the last frame of the file");
        if (cfg.norm.windowMode || cfg.norm.warp)
            for (size_t i = 1; i < c.size(); ++i)
                if (c[i].begin < c[i - 1].begin + c[i - 1].length)
                    throw Exception(std::string("normFeatFiles: ") + (cfg.norm.warp ? "warp" : "windowMode") + ": the selected segments of [" + names[k] + "] overlap or are not in increasing order");
        clusters.push_back(c);
    }
    if (!dim) throw Exception("normFeatFiles: no frames");
    std::vector<int> cols = parseFeatureMask(cfg.featureServerMask);
    if (cols.empty()) for (unsigned long c = 0; c < dim; ++c) cols.push_back((int)c);
    for (int c : cols) if ((unsigned long)c >= dim) throw Exception("featureServerMask selects a column beyond vectSize");
    NormFeatCfg norm = cfg.norm;
    if (norm.warp && norm.warpTarget.empty() && !norm.warpGaussHistoFilename.empty()) norm.warpTarget = readHistoFile(norm.warpGaussHistoFilename);
    std::vector<float> all((size_t)total * dim);
    for (size_t k = 0; k < files.size(); ++k)
        if (files[k].nFrames) memcpy(all.data() + (size_t)first[k] * dim, files[k].data.data(), files[k].data.size() * sizeof(float));
    {
        FeatureBuffer fs(srv, all.data(), total, dim, first);
        size_t done = 0;                                       // offset into the external vectors: they follow the mask's order
        for (size_t a = 0; a < cols.size();) {                 // one call per contiguous piece of the mask
            size_t b = a + 1;
            while (b < cols.size() && cols[b] == cols[b - 1] + 1) ++b;
            NormFeatCfg nc = norm;
            nc.frameLength = cfg.frameLength;                  // windowMode counts its windows in the label files' time base
            if (!nc.extMean.empty()) {
                if (nc.extMean.size() != cols.size() || nc.extStd.size() != cols.size()) throw Exception("normFeatFiles: external mean / std must have one value per masked column");
                nc.extMean.assign(cfg.norm.extMean.begin() + done, cfg.norm.extMean.begin() + done + (b - a));
                nc.extStd.assign(cfg.norm.extStd.begin() + done, cfg.norm.extStd.begin() + done + (b - a));
            }
            normFeat(fs, clusters, nc, (unsigned long)cols[a], (unsigned long)(b - a));
            done += b - a;
            a = b;
        }
        fs.download(all.data());
    }
    for (size_t k = 0; k < files.size(); ++k) {
        FeatureFile out;
        out.vectSize = cols.size(); out.baseDim = (unsigned)cols.size(); out.flags = files[k].flags;
        auto put = [&](unsigned long t) {
            const float *row = all.data() + (size_t)(first[k] + t) * dim;
            for (int c : cols) out.data.push_back(row[c]);
            ++out.nFrames;
        };
        if (cfg.writeAllFeatures) for (unsigned long t = 0; t < files[k].nFrames; ++t) put(t);
        else for (const Seg &g : clusters[k]) for (unsigned long t = 0; t < g.length; ++t) put(g.begin + t);
        if (cols.size() == dim) out.baseDim = files[k].baseDim;  // nothing masked: the header goes through unchanged
        writeFeatureFile((cfg.saveFeatureFilePath.empty() ? cfg.featureFilesPath : cfg.saveFeatureFilePath) + names[k] + cfg.saveFeatureFileExtension, out);
    }
}

void energyDetectorFiles(GpuServer &srv, const std::vector<std::string> &names, const EnergyDetectorFilesCfg &cfg, std::vector<double> *thresholds,
                         std::vector<int> *status)
{
    if (thresholds) thresholds->clear();
    if (status) status->clear();
    if (names.empty()) return;
    std::vector<unsigned long> first;
    std::vector<SegCluster> clusters;
    std::vector<float> all;
    unsigned long total = 0, dim = 0;
    for (size_t k = 0; k < names.size(); ++k) {
        const FeatureFile f = readFeatureFile(cfg.featureFilesPath + names[k] + cfg.loadFeatureFileExtension, cfg.featureServerMask);
        if (f.nFrames) {
            if (dim && f.vectSize != dim) throw Exception("energyDetectorFiles: [" + names[k] + "] has another dimension than the files before it");
            dim = f.vectSize;
        }
        first.push_back(total);
        total += f.nFrames;
        all.insert(all.end(), f.data.begin(), f.data.end());
        SegCluster c;
        if (cfg.labelFilesExtension.empty()) { Seg s; s.begin = 0; s.length = f.nFrames; s.source = k; if (f.nFrames) c.push_back(s); }
        else c = selectSegments(readLabelFile(cfg.labelFilesPath + names[k] + cfg.labelFilesExtension), cfg.labelSelectedFrames, cfg.frameLength, k);
        for (const Seg &g : c)
            if (g.begin + g.length > f.nFrames) throw Exception("energyDetectorFiles: a segment of [" + names[k] + "] ends after the last frame of the file");
        clusters.push_back(c);
    }
    if (!dim) throw Exception("energyDetectorFiles: no frames");
    std::vector<SegCluster> out;
    {
        FeatureBuffer fs(srv, all.data(), total, dim, first);
        out = energyDetectorBatch(fs, clusters, cfg.energy, nullptr, thresholds, status);
    }
    for (size_t k = 0; k < names.size(); ++k) {
        const std::string path = (cfg.saveLabelFilePath.empty() ? cfg.labelFilesPath : cfg.saveLabelFilePath) + names[k] + cfg.saveLabelFileExtension;
        std::ofstream o(path.c_str(), std::ios::out | std::ios::trunc);
        if (!o.good()) throw Exception("Can't create label file [" + path + "]");
        for (const Seg &g : out[k])
            o << frameIdxToTime(g.begin, cfg.frameLength) << " " << frameIdxToTime(g.begin + g.length - 1, cfg.frameLength) << " " << cfg.labelOutputFrames << std::endl;
    }
}

std::vector<SegCluster> turnDetectionFiles(GpuServer &srv, const std::vector<std::string> &names, const TurnDetectionFilesCfg &cfg)
{
    std::vector<SegCluster> out;
    if (names.empty()) return out;
    (void)turnCriterion(cfg.turn.clusteringCrit);                        // a refused criterion before any file is read
    std::vector<unsigned long> first;
    std::vector<SegCluster> clusters;
    std::vector<float> all;
    unsigned long total = 0, dim = 0;
    for (size_t k = 0; k < names.size(); ++k) {
        const FeatureFile f = readFeatureFile(cfg.featureFilesPath + names[k] + cfg.loadFeatureFileExtension, cfg.featureServerMask);
        if (f.nFrames) {
            if (dim && f.vectSize != dim) throw Exception("turnDetectionFiles: [" + names[k] + "] has another dimension than the files before it");
            dim = f.vectSize;
        }
        first.push_back(total);
        total += f.nFrames;
        all.insert(all.end(), f.data.begin(), f.data.end());
        SegCluster c;
        if (cfg.labelFilesExtension.empty()) { Seg s; s.begin = 0; s.length = f.nFrames; s.source = k; if (f.nFrames) c.push_back(s); }
        else c = selectSegments(readLabelFile(cfg.labelFilesPath + names[k] + cfg.labelFilesExtension), cfg.labelSelectedFrames, cfg.frameLength, k);
        for (const Seg &g : c)
            if (g.begin + g.length > f.nFrames) throw Exception("turnDetectionFiles: a segment of [" + names[k] + "] ends after the last frame of the file");
        clusters.push_back(c);
    }
    if (!dim) throw Exception("turnDetectionFiles: no frames");
    {
        FeatureBuffer fs(srv, all.data(), total, dim, first);
        out = turnDetectionBatch(fs, clusters, cfg.turn);
    }
    for (size_t k = 0; k < names.size(); ++k) {
        const std::string path = (cfg.saveLabelFilePath.empty() ? cfg.labelFilesPath : cfg.saveLabelFilePath) + names[k] + cfg.saveLabelFileExtension;
        std::ofstream o(path.c_str(), std::ios::out | std::ios::trunc);
        if (!o.good()) throw Exception("Can't create label file [" + path + "]");
        for (const Seg &g : out[k])
            o << frameIdxToTime(g.begin, cfg.frameLength) << " " << frameIdxToTime(g.begin + g.length - 1, cfg.frameLength) << " " << cfg.labelSelectedFrames << std::endl;
    }
    return out;
}

// ---- IvTest on an ndx ----------------------------------------------------------------------------------------------------------
namespace {
// the lines of an XList: blank-separated elements, empty lines skipped
std::vector<std::vector<std::string> > readListLines(const std::string &path, const char *what)
{
    std::ifstream in(path.c_str());
    if (!in) throw Exception(std::string("cannot open the ") + what + " [" + path + "]");
    std::vector<std::vector<std::string> > lines;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::vector<std::string> el;
        std::string tok;
        while (ls >> tok) el.push_back(tok);
        if (!el.empty()) lines.push_back(el);
    }
    return lines;
}
} // namespace

IvTestNdx loadIvTestNdx(const std::string &ndx, const std::string &targetIdList)
{
    IvTestNdx out;
    const std::vector<std::vector<std::string> > test = readListLines(ndx, "ndx file");
    std::map<std::string, int32_t> modelOf, segOf;
    const bool idList = !targetIdList.empty(); // PldaTools.cpp:3473
    if (idList) {
        std::vector<std::vector<std::string> > enrol = readListLines(targetIdList, "targetIdList");
        if (enrol.empty()) throw Exception("targetIdList [" + targetIdList + "] is empty");
        // enrollList.sortByElementNumber("descend") (:3487); lines of equal length keep file order (assumed, see io.h)
        std::stable_sort(enrol.begin(), enrol.end(), [](const std::vector<std::string> &a, const std::vector<std::string> &b) { return a.size() > b.size(); });
        out.maxSessions = (unsigned long)enrol[0].size() - 1; // :3495
        for (const std::vector<std::string> &l : enrol) {     // :3497-3511
            auto it = modelOf.find(l[0]);
            if (it == modelOf.end()) {
                it = modelOf.emplace(l[0], (int32_t)out.models.size()).first;
                out.models.push_back(l[0]);
                out.sessions.emplace_back();
            }
            for (size_t e = 1; e < l.size(); ++e) out.sessions[(size_t)it->second].push_back(l[e]);
        }
    }
    std::map<std::pair<int32_t, int32_t>, bool> seen;
    for (const std::vector<std::string> &l : test) { // :3520-3545 and :3606-3620 in one pass: the indices never change once given
        auto is = segOf.find(l[0]);
        if (is == segOf.end()) {
            is = segOf.emplace(l[0], (int32_t)out.segs.size()).first;
            out.segs.push_back(l[0]);
        }
        for (size_t e = 1; e < l.size(); ++e) {
            auto im = modelOf.find(l[e]);
            if (im == modelOf.end()) {
                if (idList) { ++out.dropped; continue; } // "WARNING: model ... has no enrollment session" (:3535)
                im = modelOf.emplace(l[e], (int32_t)out.models.size()).first;
                out.models.push_back(l[e]);
                out.sessions.push_back(std::vector<std::string>(1, l[e]));
            }
            if (seen.emplace(std::make_pair(im->second, is->second), true).second) {
                out.trialModel.push_back(im->second);
                out.trialSeg.push_back(is->second);
            }
        }
    }
    return out;
}

IvTestFilesResult ivTestFiles(GpuServer &srv, const IvTestFilesCfg &cfg, PldaDev &dev, const std::vector<double> &pldaF, const std::vector<double> &pldaG,
                              const std::vector<double> &pldaSigma)
{
    IvTestFilesResult r;
    r.ndx = loadIvTestNdx(cfg.ndxFilename, cfg.targetIdList);
    const IvTestNdx &nx = r.ndx;
    if (nx.models.empty() || nx.segs.empty()) throw Exception("ivTestFiles: the ndx [" + cfg.ndxFilename + "] names no model or no segment");
    std::vector<std::string> enrolIds;
    std::vector<unsigned long> enrolPerModel;
    for (const std::vector<std::string> &s : nx.sessions) {
        if (s.empty()) throw Exception("ivTestFiles: a model of the targetIdList has no enrolment session");
        enrolIds.insert(enrolIds.end(), s.begin(), s.end());
        enrolPerModel.push_back((unsigned long)s.size());
    }
    unsigned long dimE = 0, dimT = 0;
    std::vector<double> enrol = loadVectorsById(cfg.vectorFilesPath, enrolIds, cfg.vectorFilesExtension, dimE, cfg.loadMatrixFormat);
    std::vector<double> test = loadVectorsById(cfg.vectorFilesPath, nx.segs, cfg.vectorFilesExtension, dimT, cfg.loadMatrixFormat);
    if (dimE != dimT || dimE != dev.getVectSize()) throw Exception("ivTestFiles: the vector files and the development set differ in dimension");
    const std::vector<double> sc = ivTestTrials(srv, cfg.test, dev, enrol, enrolPerModel, test, (unsigned long)nx.segs.size(), nx.trialModel, nx.trialSeg,
                                                pldaF, pldaG, pldaSigma);
    // IvTest.cpp:430-437: for every segment, the models in index order
    std::vector<size_t> order(sc.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
        return nx.trialSeg[a] != nx.trialSeg[b] ? nx.trialSeg[a] < nx.trialSeg[b] : nx.trialModel[a] < nx.trialModel[b];
    });
    for (size_t i : order) {
        r.lineModel.push_back(nx.trialModel[i]);
        r.lineSeg.push_back(nx.trialSeg[i]);
        r.scores.push_back(sc[i]);
    }
    if (!cfg.outputFilename.empty()) {
        std::ofstream o(cfg.outputFilename.c_str(), std::ios::out | std::ios::trunc);
        if (!o.good()) throw Exception("Can't create the result file [" + cfg.outputFilename + "]");
        for (size_t k = 0; k < r.scores.size(); ++k)
            o << resultLine(r.scores[k], nx.models[(size_t)r.lineModel[k]], nx.segs[(size_t)r.lineSeg[k]], cfg.gender, cfg.decisionThreshold) << std::endl;
    }
    return r;
}

} // namespace liagpu
