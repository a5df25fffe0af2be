// turn_detect.h -- launchers of turn_detect.hip (include/gmmiv_turn.h) and the tile shape both sides agree on.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define TURN_THREADS 256
#define TURN_MAX_TILE 32           // positions per tile, at most
#define TURN_LDS_BUDGET (159 * 1024) // bytes of the 160 KB a tile may take

// The LDS layout of a tile of P positions (doubles unless said otherwise); host and device compute it from (D, W, S, P) alone.
struct TurnShape {
    long W, S;
    int D, Dp, P;
    long nb, nb12, r1, r12; // blocks of a W-window / of the 2 W-window, length of their short last block (0: none)
    int ncap, cap_r1, cap_r12; // partial sums kept per block start: the full block, then the two short lengths that occur
    long R;                 // rows staged: 2 W + (P - 1) S
    long nA, nB;            // block starts j S (family A) and W + j S (family B, only when W % S != 0)
    long o_x, o_bs, o_mod, o_lc, o_lp, o_flag, bytes; // offsets in doubles; o_flag: 2 P ints (bad covariance | rule acted)
    __host__ __device__ long nblk() const { return 2 * nb + nb12; } // llk block partials per position: c1 | c2 | c12
};

// false when the numbers overflow or P < 1; s.bytes may exceed the budget (the caller compares)
static inline __host__ __device__ bool turn_shape(int D, long W, long S, int P, TurnShape &s)
{
    if (D < 1 || W < 1 || S < 1 || P < 1 || W > (1L << 24) || S > (1L << 24) || D > (1 << 20)) return false;
    s.W = W; s.S = S; s.D = D; s.Dp = D | 1; s.P = P;
    s.nb = (W + S - 1) / S; s.nb12 = (2 * W + S - 1) / S; s.r1 = W % S; s.r12 = (2 * W) % S;
    s.cap_r1 = s.r1 ? 1 : 0; s.cap_r12 = s.r12 ? 1 + s.cap_r1 : 0; s.ncap = 1 + (s.r1 ? 1 : 0) + (s.r12 ? 1 : 0);
    s.R = 2 * W + (long)(P - 1) * S;
    s.nA = (P - 1) + s.nb12; s.nB = s.r1 ? (P - 1) + s.nb : 0;
    long bs = (s.nA + s.nB) * s.ncap * 2 * s.Dp;
    const long lg = 3L * P * s.Dp; // the log covariances take the block sums' place once the models stand
    if (bs < lg) bs = lg;
    s.o_x = 0; s.o_bs = s.o_x + s.R * s.Dp; s.o_mod = s.o_bs + bs; s.o_lc = s.o_mod + 6L * P * s.Dp; s.o_lp = s.o_lc + 3L * P;
    s.o_flag = s.o_lp + (long)P * s.nblk();
    s.bytes = 8 * (s.o_flag + P);
    return true;
}

// positions gmmiv_plan_turn_positions gives a run of L frames
static inline __host__ __device__ long turn_run_positions(long L, long W, long S) { return L <= 2 * W ? 0 : (L - 2 * W + S - 1) / S; }

int gmmk_turn_tiles(hipStream_t st, const long *runs, long nrun, const long *pos_off, long W, long S, int P, long *tile_off);
int gmmk_turn_curve(hipStream_t st, int x_f64, const void *x, long ldx, int D, const long *runs, long nrun, const long *pos_off, long npos, long W, long S,
                    int P, long grid, const long *tile_off, int crit, double penalty, double min_llk, double max_llk, double *value, int *status);
int gmmk_turn_pick(hipStream_t st, const double *value, const long *pos_off, long nrun, long npos, double alpha, double *smoothed, unsigned char *dec,
                   double *run_stats, long *n_turns);
int gmmk_turn_segments(hipStream_t st, const long *runs, long nrun, long nfiles, const long *pos_off, long npos, const unsigned char *dec, long W, long S,
                       long *run_base, long *seg_count, const long *seg_off, long *seg_begin, long *seg_len);
