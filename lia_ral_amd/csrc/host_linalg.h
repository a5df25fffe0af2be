// host_linalg.h -- small dense fp64 routines on the host for the O(n^3)-once-per-call pieces of the i-vector back end (min-divergence
// factor, PLDA K_n, the Gram factor of orthonormalize_t, LDA, the PLDA pre-computation).  Plain C++: no HIP, no context, so the file
// compiles on its own (tests/host_linalg_main.cpp runs it under a sanitizer).  Row-major everywhere.  Internal: hidden from the ABI.
#pragma once
#include <vector>

#pragma GCC visibility push(hidden)
// a = Ch^T Ch, Ch upper; false: a is not positive definite
bool host_cholesky_upper(int n, const std::vector<double> &a, std::vector<double> &ch);
// SPD inverse + log det (nullable) through the Cholesky factor
bool host_spd_inverse(int n, const std::vector<double> &a, std::vector<double> &inv, double *logdet);
// cyclic Jacobi for a symmetric matrix: eigenvalues descending, vect[k*rank + j] = component k of vector j
void host_sym_eigen(int n, const std::vector<double> &A, int rank, std::vector<double> &vect, std::vector<double> &val);
// g = L L^T, L lower, column by column; dmin / dmax = the extremes of L's diagonal over the columns done; false: not positive definite
bool host_cholesky_lower(int n, const std::vector<double> &g, std::vector<double> &L, double *dmin, double *dmax);
// Li = L^-1 by forward substitution, column by column
void host_lower_inverse(int n, const std::vector<double> &L, std::vector<double> &Li);
// with U upper (W = U^T U): X = U^-T B column by column; X = T U^-1 row by row; x = U^-1 y for y = column j of vect [n x rank],
// written to row j of out [rank x n] -- the three substitutions of the symmetric form of W^-1 B (gmmiv_dev_lda)
void host_upper_tsolve_cols(int n, const std::vector<double> &U, const std::vector<double> &B, std::vector<double> &X);
void host_upper_rsolve_rows(int n, const std::vector<double> &U, const std::vector<double> &T, std::vector<double> &X);
void host_upper_solve_vec(int n, const std::vector<double> &U, const std::vector<double> &vect, int rank, int j, std::vector<double> &out);
#pragma GCC visibility pop
// C[M x N] (+)= op(A) op(B), op(A) is M x K; i-k-j order.  (C linkage, default visibility: the library has exported this name since
// the routine was written, and the list of exported names is not this file's to change.)
extern "C" void hmm(int M, int N, int K, const double *A, bool ta, const double *B, bool tb, double *Cm, bool accumulate = false);
