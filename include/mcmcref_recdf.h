/*
 * mcmcref_recdf.h -- the C ABI of libmcmcref_recdf.so, a companion library of libmcmcref_hip.so: the PER-CHAIN RANK-ECDF
 * UNIFORMITY TEST WITH SIMULTANEOUS BANDS of Saeilynoja, Buerkner and Vehtari (2022, "Graphical test for discrete
 * uniformity and its applications in goodness-of-fit evaluation and multiple sample comparison"), the test behind
 * bayesplot's mcmc_rank_ecdf and ArviZ's plot_ecdf(confidence_bands="simulated").  R-hat says THAT chains disagree; this
 * says which chain, where in the distribution, and whether more than C chains of n exchangeable draws do by chance.
 * Entries are prefixed mce_, constants MCE_.  This header takes from mcmcref_hip.h the return codes (MCR_OK, MCR_EINVAL,
 * MCR_EHIP, MCR_ENOMEM, MCR_ENODEVICE, MCR_ENONFINITE) and the dtype constants (MCR_F64, MCR_F32) and nothing else.  As
 * libmcmcref_std.so the library does not link against the main one: it holds a further copy of the main library's code (its
 * sort stage and summary pipeline, linked in as objects, no name of it exported), and an mce handle owns a context of
 * that copy.  Device addresses come from the caller; the caller orders its own work first (mcr_sync) -- an mce call runs
 * on streams its handle owns.  Calls on one handle are serialised by the caller.
 *
 * THE DEFINITION.  One parameter, C >= 1 chains of n >= 1 kept draws x[c][i], M = C n < 2^31 - 1 pooled draws, K evaluation
 * points, 2 <= K <= min(M, MCE_MAX_POINTS).  An f32 draw is widened to double first (exactly).  Thinning is the caller's
 * stride: there is no thin argument, a caller that keeps every T-th draw passes stride_n T and n = ceil(N / T).
 * Counts.  For k = 1 .. K-1:
 *     m_k     = floor(k M / K) in integer arithmetic (strictly increasing, >= 1, < M)
 *     t_k     = the m_k-th smallest pooled draw
 *     a[c][k] = #{ i : x[c][i] <= t_k } under IEEE comparison: ties go together, -0.0 == +0.0
 *     R[k]    = sum_c a[c][k]      (>= m_k; equal unless draws tie with t_k)
 *     tied    = #{ k : R[k] != m_k }: the calibration below is exact when this is 0 and approximate otherwise.  A
 *               reported output, not an error.
 * Pointwise table, a function of (M, n, K) alone (mce_table_host): for X ~ Hypergeometric(population M, m_k marked, n drawn)
 *     U[k][j] = min(P(X <= j), P(X >= j)),   j = 0 .. n
 * from weights w_j = pmf(j) / pmf(mode) by the recurrence w_{j+1} = w_j ((m_k - j)(n - j)) / ((j + 1)(M - m_k - n + j + 1))
 * upward from the mode and w_{j-1} = w_j (j (M - m_k - n + j)) / ((m_k - j + 1)(n - j + 1)) downward (w_mode = 1; mode =
 * floor((n + 1)(m_k + 1) / (M + 2)) clamped to the support), each tail summed from its END INWARD so that a small tail
 * keeps its relative accuracy, the smaller of the two divided by the sum of all weights.  0 outside the support: a count
 * that ties pushed past m_k has U = 0.  No special function, every step a rounded double operation: the table has the same bits wherever it is computed.
 * Statistic.
 *     u[c]    = min_k U[k][a[c][k]]        kmin[c] = the first k attaining it
 *     g       = min_c u[c]                 chain   = the first c attaining it
 *     dev[c]  = max_k |a[c][k] M - n R[k]|  as int64: the largest difference between the chain's ECDF and the pooled one,
 *               times n M (the caller divides)
 * Every min is exact and every count an integer: the device, the host definition, every layout, dtype route, alignment
 * and chunking give the SAME BITS.
 * Null sample, a function of (C, n, K, S, seed): for s = 0 .. S-1 the simulated draws are
 *     y[s][c][i] = (splitmix64(seed * 0x9E3779B97F4A7C15 + s M + c n + i) >> 11) * 2^-53     (64-bit wrapping arithmetic)
 *     splitmix64(x): z = x + 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *                    z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)
 * and g0[s] = g of y[s], by the same count and statistic code.  The caller assembles
 *     p = (1 + #{ s : g0[s] <= g }) / (S + 1)          and rejects at level alpha when p <= alpha.
 * Example.  C = 2, n = 4, K = 4: chain 0 = 1, 2, 3, 4, chain 1 = 5, 6, 7, 8.  M = 8, m = 2, 4, 6, t = 2, 4, 6.
 * a[0] = 2, 4, 4, a[1] = 0, 0, 2, R = 2, 4, 6, tied = 0.  X ~ Hypergeometric(8, m_k, 4): for m = 2 the pmf on 0, 1, 2 is
 * 3/14, 8/14, 3/14, so U[1][2] = U[1][0] = 3/14; for m = 4 the pmf on 0 .. 4 is 1, 16, 36, 16, 1 over 70, so
 * U[2][4] = U[2][0] = 1/70; m = 6 mirrors m = 2 (pmf on 2, 3, 4): U[3][4] = U[3][2] = 3/14.  u = 1/70, 1/70 with kmin = 2, 2;
 * g = 1/70 = 0.014285714285714, chain = 0; dev = max |2*8 - 4*2|, |4*8 - 4*4|, |4*8 - 4*6| = 16 for both chains: an ECDF
 * difference of 16 / 32 = 0.5 at the pooled median.
 * Layout of the outputs of one parameter: counts [C][K-1] and pooled [K-1] (column k - 1 holds point k); kmin holds k
 * itself, 1 .. K-1; the table is [K-1][n+1], U[k][j] at (k - 1)(n + 1) + j.
 */
#ifndef MCMCREF_RECDF_H
#define MCMCREF_RECDF_H

#include "mcmcref_hip.h"

#pragma GCC visibility push(default)
#ifdef __cplusplus
extern "C" {
#endif

#define MCE_VERSION 100
#define MCE_MAX_POINTS 1024       /* K, evaluation points */
#define MCE_MAX_TABLE 134217728   /* (K - 1)(n + 1), entries of the pointwise table (2^27: 1 GiB) */
#define MCE_HIST_BYTES 24576      /* LDS histogram of a count workgroup: floor(MCE_HIST_BYTES / (4 K)) chains at most */
#define MCE_SLICE_DRAWS 16384     /* ... and as many chains as keep it near this many draws */
#define MCE_KERNEL_FILL 0         /* mce_kernel_ms: the null sample's generator */
#define MCE_KERNEL_PIPE 1         /* ... the copy of the kept draws and the summary pipeline (the sort) */
#define MCE_KERNEL_COUNT 2        /* ... the count kernel */
#define MCE_KERNEL_STAT 3         /* ... the statistic kernel */
#define MCE_KERNELS 4

/* The library's version, MCE_VERSION. */
int mce_version(void);
/* A handle on HIP device `device`: a context of the library's own copy of the summary pipeline (streams, workspace
 * that only grows) and the uploaded table of the last (M, n, K).  MCR_ENODEVICE when the device cannot be used; then
 * mce_last_error(NULL) holds the message. */
int mce_init(int device, void** handle);
void mce_free(void* handle);
/* The message of the last failed call on the handle (NULL: of this thread's last failed call that takes no handle). */
const char* mce_last_error(void* handle);
/* Upper bound in bytes of the device workspace of one chunk of parameters or simulations.  A call cuts its parameters
 * into chunks under it; MCR_ENOMEM from a later call when one parameter alone does not fit. */
int mce_set_workspace_limit(void* handle, size_t bytes);
/* Parameters per chunk of a call of this shape under the handle's limit (mce_rank_ecdf_dev makes the same cut). */
int mce_plan(void* handle, int dtype, int64_t C, int64_t n, int64_t P, int64_t stride_c, int64_t stride_n, int64_t stride_p,
             int K, int64_t* params_per_chunk);
/* Simulations per chunk of mce_null_sample of this shape under the handle's limit. */
int mce_null_plan(void* handle, int64_t C, int64_t n, int K, int64_t S, int64_t* sims_per_chunk);

/* The test's statistics of every parameter p < P of a draw tensor in device memory: element (c, i, p) is at
 * draws_dev[c stride_c + i stride_n + p stride_p] (strides in elements, >= 0), dtype MCR_F64 or MCR_F32.  The outputs are
 * host arrays: counts [P][C][K-1], pooled [P][K-1], tied [P], u [P][C], kmin [P][C], dev [P][C], g [P], chain [P]; a NULL
 * output is skipped.
 * Per chunk: contiguous f64 [P][C][n] is read in place, anything else is copied to f64.  The summary pipeline sorts the
 * pooled draws as one chain of M (no diagnostics).  k_mce_count, a workgroup per (parameter, slice of chains), takes the
 * K - 1 thresholds from the sorted keys into LDS, streams its chains in time order with 16-byte loads, bins every draw by
 * a fixed-depth binary search into an LDS histogram [chains][K] and ends with a prefix over k; k_mce_stat, a workgroup
 * per parameter, pools the counts, looks the table up (cached on the handle per (M, n, K)) and takes the exact minima.
 * Synchronous.  MCR_ENONFINITE when a draw is NaN or infinite (the outputs are then unspecified).  MCR_EINVAL (the message
 * names the cause): a NULL handle or tensor pointer; a dtype other than the two; C, n or P < 1; C * n >= 2^31 - 1; K < 2,
 * K > C * n or K > MCE_MAX_POINTS; (K - 1)(n + 1) > MCE_MAX_TABLE; a negative stride.  After an error the handle stays usable. */
int mce_rank_ecdf_dev(void* handle, const void* draws_dev, int dtype, int64_t C, int64_t n, int64_t P, int64_t stride_c,
                      int64_t stride_n, int64_t stride_p, int K, int32_t* counts, int32_t* pooled, int32_t* tied, double* u,
                      int32_t* kmin, int64_t* dev, double* g, int32_t* chain);
/* The same on a tensor in host memory, which it uploads (the span the strides reach). */
int mce_rank_ecdf(void* handle, const void* draws, int dtype, int64_t C, int64_t n, int64_t P, int64_t stride_c, int64_t stride_n,
                  int64_t stride_p, int K, int32_t* counts, int32_t* pooled, int32_t* tied, double* u, int32_t* kmin, int64_t* dev,
                  double* g, int32_t* chain);
/* The null sample g0[S] (a host array, in simulation order) on the device: k_mce_null writes a chunk of simulations'
 * draws, which then go down the path of mce_rank_ecdf_dev.  The same bits under every chunking, and as
 * mce_null_sample_host.  S >= 1. */
int mce_null_sample(void* handle, int64_t C, int64_t n, int K, int64_t S, uint64_t seed, double* g0);

/* The definition on the host for one parameter: chains [C][n] doubles, the outputs as above with P = 1.  table: the
 * [K-1][n+1] table of mce_table_host(C n, n, K), or NULL (computed by the call).  No handle, no device; the same limits
 * and refusals (MCR_ENONFINITE leaves the outputs untouched). */
int mce_rank_ecdf_host(const double* chains, int64_t C, int64_t n, int K, const double* table, int32_t* counts, int32_t* pooled,
                       int32_t* tied, double* u, int32_t* kmin, int64_t* dev, double* g, int32_t* chain);
/* The null sample by the definition on the host. */
int mce_null_sample_host(int64_t C, int64_t n, int K, int64_t S, uint64_t seed, double* g0);
/* The pointwise table [K-1][n+1] of (M, n, K); 1 <= n <= M < 2^31 - 1, 2 <= K <= min(M, MCE_MAX_POINTS). */
int mce_table_host(int64_t M, int64_t n, int K, double* table);

/* Per-kernel times: when enabled (on != 0) every later mce_rank_ecdf* and mce_null_sample call brackets its kernels with
 * HIP events (and waits after every chunk); mce_kernel_ms writes the LAST call's totals over its chunks in milliseconds,
 * ms[MCE_KERNEL_FILL .. MCE_KERNEL_STAT] (cap >= MCE_KERNELS, else MCR_EINVAL; zeros when the last call was not timed). */
int mce_profile_enable(void* handle, int on);
int mce_kernel_ms(void* handle, double* ms, int cap);

#ifdef __cplusplus
}
#endif
#pragma GCC visibility pop

#endif
