// host_linalg.cpp -- see host_linalg.h.  The loop orders and expressions are part of the results (bit for bit): do not reorder.
#include "host_linalg.h"

#include <math.h>
#include <string.h>

bool host_cholesky_upper(int n, const std::vector<double> &a, std::vector<double> &ch)
{
    ch.assign((size_t)n * n, 0.0); // R = Ch^T Ch, Ch upper
    for (int i = 0; i < n; ++i)
        for (int j = i; j < n; ++j) {
            double s = a[(size_t)i * n + j];
            for (int k = 0; k < i; ++k) s -= ch[(size_t)k * n + i] * ch[(size_t)k * n + j];
            if (i == j) {
                if (!(s > 0.0)) return false;
                ch[(size_t)i * n + i] = sqrt(s);
            } else
                ch[(size_t)i * n + j] = s / ch[(size_t)i * n + i];
        }
    return true;
}

bool host_spd_inverse(int n, const std::vector<double> &a, std::vector<double> &inv, double *logdet)
{
    std::vector<double> u;
    if (!host_cholesky_upper(n, a, u)) return false;
    double ld = 0.0;
    for (int i = 0; i < n; ++i) ld += log(u[(size_t)i * n + i]);
    if (logdet) *logdet = 2.0 * ld;
    // Ui = U^-1 (upper), then A^-1 = Ui Ui^T
    std::vector<double> ui((size_t)n * n, 0.0);
    for (int c = 0; c < n; ++c) {
        ui[(size_t)c * n + c] = 1.0 / u[(size_t)c * n + c];
        for (int i = c - 1; i >= 0; --i) {
            double s = 0.0;
            for (int k = i + 1; k <= c; ++k) s += u[(size_t)i * n + k] * ui[(size_t)k * n + c];
            ui[(size_t)i * n + c] = -s / u[(size_t)i * n + i];
        }
    }
    inv.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = i; j < n; ++j) {
            double s = 0.0;
            for (int k = j; k < n; ++k) s += ui[(size_t)i * n + k] * ui[(size_t)j * n + k];
            inv[(size_t)i * n + j] = inv[(size_t)j * n + i] = s;
        }
    return true;
}

void host_sym_eigen(int n, const std::vector<double> &A, int rank, std::vector<double> &vect, std::vector<double> &val)
{
    std::vector<double> a(A), v((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) v[(size_t)i * n + i] = 1.0;
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0.0, dg = 0.0;
        for (int i = 0; i < n; ++i) {
            dg += a[(size_t)i * n + i] * a[(size_t)i * n + i];
            for (int j = i + 1; j < n; ++j) off += a[(size_t)i * n + j] * a[(size_t)i * n + j];
        }
        if (off <= 1e-30 * (dg + off)) break;
        for (int p = 0; p + 1 < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = a[(size_t)p * n + q];
                if (apq == 0.0) continue;
                const double th = (a[(size_t)q * n + q] - a[(size_t)p * n + p]) / (2.0 * apq);
                const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
                for (int k = 0; k < n; ++k) { const double x = a[(size_t)k * n + p], y = a[(size_t)k * n + q]; a[(size_t)k * n + p] = cs * x - sn * y; a[(size_t)k * n + q] = sn * x + cs * y; }
                for (int k = 0; k < n; ++k) { const double x = a[(size_t)p * n + k], y = a[(size_t)q * n + k]; a[(size_t)p * n + k] = cs * x - sn * y; a[(size_t)q * n + k] = sn * x + cs * y; }
                for (int k = 0; k < n; ++k) { const double x = v[(size_t)k * n + p], y = v[(size_t)k * n + q]; v[(size_t)k * n + p] = cs * x - sn * y; v[(size_t)k * n + q] = sn * x + cs * y; }
            }
    }
    std::vector<int> ord(n);
    for (int i = 0; i < n; ++i) ord[i] = i;
    for (int i = 1; i < n; ++i) { // stable insertion sort, descending
        const int o = ord[i];
        int j = i - 1;
        while (j >= 0 && a[(size_t)ord[j] * n + ord[j]] < a[(size_t)o * n + o]) { ord[j + 1] = ord[j]; --j; }
        ord[j + 1] = o;
    }
    vect.assign((size_t)n * rank, 0.0);
    val.assign(rank, 0.0);
    for (int j = 0; j < rank; ++j) {
        val[j] = a[(size_t)ord[j] * n + ord[j]];
        for (int k = 0; k < n; ++k) vect[(size_t)k * rank + j] = v[(size_t)k * n + ord[j]];
    }
}

void hmm(int M, int N, int K, const double *A, bool ta, const double *B, bool tb, double *Cm, bool accumulate)
{
    if (!accumulate) memset(Cm, 0, sizeof(double) * (size_t)M * N);
    for (int i = 0; i < M; ++i)
        for (int k = 0; k < K; ++k) {
            const double a = ta ? A[(size_t)k * M + i] : A[(size_t)i * K + k];
            if (a == 0.0) continue;
            double *cr = Cm + (size_t)i * N;
            if (!tb) { const double *br = B + (size_t)k * N; for (int j = 0; j < N; ++j) cr[j] += a * br[j]; }
            else for (int j = 0; j < N; ++j) cr[j] += a * B[(size_t)j * K + k];
        }
}

bool host_cholesky_lower(int n, const std::vector<double> &g, std::vector<double> &L, double *dmin, double *dmax)
{
    L.assign((size_t)n * n, 0.0);
    *dmin = __builtin_inf();
    *dmax = 0.0;
    for (int j = 0; j < n; ++j) {
        double d = g[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) d -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
        if (!(d > 0.0)) return false;
        const double ljj = sqrt(d);
        L[(size_t)j * n + j] = ljj;
        *dmin = ljj < *dmin ? ljj : *dmin;
        *dmax = ljj > *dmax ? ljj : *dmax;
        for (int i = j + 1; i < n; ++i) {
            double t = g[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) t -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
            L[(size_t)i * n + j] = t / ljj;
        }
    }
    return true;
}

void host_lower_inverse(int n, const std::vector<double> &L, std::vector<double> &Li)
{
    Li.assign((size_t)n * n, 0.0);
    for (int c = 0; c < n; ++c) {
        Li[(size_t)c * n + c] = 1.0 / L[(size_t)c * n + c];
        for (int i = c + 1; i < n; ++i) {
            double t = 0.0;
            for (int k = c; k < i; ++k) t += L[(size_t)i * n + k] * Li[(size_t)k * n + c];
            Li[(size_t)i * n + c] = -t / L[(size_t)i * n + i];
        }
    }
}

void host_upper_tsolve_cols(int n, const std::vector<double> &U, const std::vector<double> &B, std::vector<double> &X)
{
    X.resize((size_t)n * n);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            double v = B[(size_t)i * n + j];
            for (int k = 0; k < i; ++k) v -= U[(size_t)k * n + i] * X[(size_t)k * n + j];
            X[(size_t)i * n + j] = v / U[(size_t)i * n + i];
        }
}

void host_upper_rsolve_rows(int n, const std::vector<double> &U, const std::vector<double> &T, std::vector<double> &X)
{
    X.resize((size_t)n * n);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            double v = T[(size_t)j * n + i];
            for (int k = 0; k < i; ++k) v -= U[(size_t)k * n + i] * X[(size_t)j * n + k];
            X[(size_t)j * n + i] = v / U[(size_t)i * n + i];
        }
}

void host_upper_solve_vec(int n, const std::vector<double> &U, const std::vector<double> &vect, int rank, int j, std::vector<double> &out)
{
    for (int i = n - 1; i >= 0; --i) {
        double v = vect[(size_t)i * rank + j];
        for (int k = i + 1; k < n; ++k) v -= U[(size_t)i * n + k] * out[(size_t)j * n + k];
        out[(size_t)j * n + i] = v / U[(size_t)i * n + i];
    }
}
