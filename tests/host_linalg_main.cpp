// host_linalg_main.cpp -- runs the routines of lia_ral_amd/csrc/host_linalg.cpp on the cases of a file and writes what they return:
// the stand-alone program of tests/test_cpu_host_linalg.py, built plain and with -fsanitize=address,undefined.
//   host_linalg_main in.bin out.bin
// in : int32 count, then per case int32 op, n, rank and n*n doubles A (op 4, 5: n*n more, B)
// out: per case what the op produces (fixed sizes, zeros where a routine reports failure)
//   0 cholesky_upper        int32 ok, ch[n*n]
//   1 spd_inverse           int32 ok, inv[n*n], logdet
//   2 sym_eigen             vect[n*rank], val[rank]
//   3 cholesky_lower        int32 ok, dmin, dmax, L[n*n], Li[n*n] (lower_inverse)
//   4 the LDA substitutions U = cholesky_upper(A): int32 ok, U^-T B [n*n], U^-T B U^-1 [n*n], rows U^-1 B[:, j] [n*n]
//   5 hmm                   A B, A^T B, A B^T, A^T B^T, and A B accumulated onto A B  [5 * n*n]
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../lia_ral_amd/csrc/host_linalg.h"

static bool rd(FILE *f, void *p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }
static void wr(FILE *f, const void *p, size_t bytes) { fwrite(p, 1, bytes, f); }
static void wr(FILE *f, const std::vector<double> &v, size_t n)
{
    std::vector<double> o(v);
    o.resize(n, 0.0);
    wr(f, o.data(), n * sizeof(double));
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t count;
    if (!rd(in, &count, 4)) return 2;
    for (int32_t k = 0; k < count; ++k) {
        int32_t h[3];
        if (!rd(in, h, 12)) return 2;
        const int op = h[0], n = h[1], rank = h[2];
        const size_t nn = (size_t)n * n;
        std::vector<double> A(nn), B;
        if (!rd(in, A.data(), nn * 8)) return 2;
        if (op == 4 || op == 5) { B.resize(nn); if (!rd(in, B.data(), nn * 8)) return 2; }
        if (op == 0) {
            std::vector<double> ch;
            const int32_t ok = host_cholesky_upper(n, A, ch);
            wr(out, &ok, 4);
            wr(out, ok ? ch : std::vector<double>(), nn);
        } else if (op == 1) {
            std::vector<double> inv;
            double ld = 0.0;
            const int32_t ok = host_spd_inverse(n, A, inv, &ld);
            wr(out, &ok, 4);
            wr(out, inv, nn);
            wr(out, &ld, 8);
            std::vector<double> again;
            if (host_spd_inverse(n, A, again, nullptr) != (bool)ok) return 3; // the log det is optional
        } else if (op == 2) {
            std::vector<double> vect, val;
            host_sym_eigen(n, A, rank, vect, val);
            wr(out, vect, (size_t)n * rank);
            wr(out, val, rank);
        } else if (op == 3) {
            std::vector<double> L, Li;
            double dmin = 0.0, dmax = 0.0;
            const int32_t ok = host_cholesky_lower(n, A, L, &dmin, &dmax);
            if (ok) host_lower_inverse(n, L, Li);
            wr(out, &ok, 4);
            wr(out, &dmin, 8);
            wr(out, &dmax, 8);
            wr(out, L, nn);
            wr(out, Li, nn);
        } else if (op == 4) {
            std::vector<double> U, T1, Cm, rows(nn, 0.0);
            const int32_t ok = host_cholesky_upper(n, A, U);
            if (ok) {
                host_upper_tsolve_cols(n, U, B, T1);
                host_upper_rsolve_rows(n, U, T1, Cm);
                for (int j = 0; j < n; ++j) host_upper_solve_vec(n, U, B, n, j, rows);
            }
            wr(out, &ok, 4);
            wr(out, T1, nn);
            wr(out, Cm, nn);
            wr(out, rows, nn);
        } else if (op == 5) {
            std::vector<double> C(nn);
            for (int t = 0; t < 4; ++t) {
                hmm(n, n, n, A.data(), (t & 1) != 0, B.data(), (t & 2) != 0, C.data());
                wr(out, C, nn);
            }
            hmm(n, n, n, A.data(), false, B.data(), false, C.data());
            hmm(n, n, n, A.data(), false, B.data(), false, C.data(), true);
            wr(out, C, nn);
        } else {
            fprintf(stderr, "case %d: unknown op %d\n", (int)k, op);
            return 2;
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
