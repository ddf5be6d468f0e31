/*
 * mcmcref_iess.h -- the C ABI of libmcmcref_iess.so, the companion library of libmcmcref_hip.so: the effective sample
 * size of an INDICATOR I(lower < x <= upper) of the draws, from bit-packed indicator chains.  Entries are prefixed mci_,
 * constants MCI_.  This header takes from mcmcref_hip.h the return codes (MCR_OK, MCR_EINVAL, MCR_EHIP, MCR_ENOMEM,
 * MCR_ENODEVICE) and the dtype constants (MCR_F64, MCR_F32) and nothing else; the library does not link against the main
 * one and uses none of its internals.  Device addresses come from the caller (for instance mcr_dev_alloc of a ctx on
 * the same device): both libraries run in one process on one HIP runtime, so an address is valid in both.  The caller
 * orders its own work first (mcr_sync) -- an mci call runs on a stream its handle owns.  Calls on one handle are
 * serialised by the caller.
 *
 * What it answers: how many effective draws stand behind a quantile (lower = -inf, upper = q: the Monte Carlo error of
 * an order statistic is governed by the autocorrelation of I(x <= q)), behind a tail probability P(x > 0), or behind a
 * bin of the local-efficiency plot of Vehtari et al. (2021).
 *
 * THE DEFINITION.  It is the ESS rule of the reference (diagnostics._ess: UNSPLIT chains, truncation at the first
 * negative rho) applied to the 0/1 chains of the indicator.  It is NOT Geyer's initial-sequence rule on split chains, so
 * the numbers differ from posterior::ess_quantile / ess_median / ess_tail exactly as this project's ess_bulk differs
 * from posterior::ess_bulk.
 *
 * One parameter, one request (lower, upper], C chains of N draws; n = N, m = C.
 *     b[c][t] = 1 iff lower < x[c][t] && x[c][t] <= upper        compared in double; an f32 draw is widened exactly
 * lower = -inf and upper = +inf are allowed; lower >= upper is a valid, empty indicator.  A NaN draw compares false and
 * counts as 0; non-finite draws are not looked for.  All of the following are integers, exact in 64 bits:
 *     k_c  = sum_t b[c][t]                  Ksum = sum_c k_c               (`ones`)
 *     Wnum = sum_c k_c (n - k_c)            Q    = m sum_c k_c^2 - Ksum^2
 * and, in double, each operation rounded once, no fused multiply-add, in exactly this order:
 *     W       = Wnum / (n * (n - 1)) / m                 (sum_t (b - mean_c)^2 = k_c (n - k_c) / n exactly)
 *     B       = Q / (m * n * (m - 1))   if m > 1, else 0 (= n sum_c (mean_c - mean_total)^2 / (m - 1))
 *     var_hat = ((n - 1) / n) * W + B / n
 * (integers are converted to double first; products of converted integers are taken left to right).  Per lag = 1 .. n - 1
 * and chain c, with integer counts
 *     S_c(lag) = sum_{i < n - lag} b_i b_{i+lag}     H_c(lag) = sum_{i < n - lag} b_i     T_c(lag) = sum_{i >= lag} b_i
 *     A_c(lag) = n^2 S_c - n k_c (H_c + T_c) + (n - lag) k_c^2        (|A_c| < 2^62 for n <= 2^20: a 64-bit integer)
 *     A(lag)   = sum_c A_c(lag)          (up to 2^71: kept as a hi/lo PAIR, int64 hi and uint64 lo, two's complement)
 *     rho(lag) = dbl(A(lag)) / (n * n * (n - lag)) / (m * var_hat)
 * dbl(A) = sign * (double(hi') * 2^64 + double(lo')) of the magnitude's halves hi', lo' (each conversion rounds to
 * nearest; exact whenever |A| < 2^53).  Then
 *     trunc = the first lag with A(lag) < 0, decided on the integer pair; n when there is none
 *     ESS   = (m * n) / (1 + 2 * R),       R = the sum of rho(lag) over 1 <= lag < trunc
 * R's order: lags are taken in blocks of MCI_LAG_BLOCK consecutive lags, block j holding lags j * MCI_LAG_BLOCK + 1 ..
 * (j + 1) * MCI_LAG_BLOCK.  A block's terms t[i] (i = lag - first lag of the block) are rho(lag) for lag < trunc and
 * lag <= n - 1, else +0.0; they are summed by the halving tree  for (s = MCI_LAG_BLOCK / 2; s >= 1; s /= 2) t[i] +=
 * t[i + s] for i < s;  and the block sums are added to R = +0.0 in ascending block order, up to the block that holds
 * trunc (or lag n - 1).  The host routine and the lag kernel compile this from one text (csrc/mci_core.hpp).
 * Edge rules:  n < 2: ESS = NaN, trunc = -1.   var_hat == 0: ESS = m n, trunc = 0.   A(lag) == 0 is not negative: the
 * walk goes on.  Example: one chain 1,1,1,0,0,0 has A(1) = 27 (rho = 0.6), A(2) = 0, A(3) = -27: trunc = 3, ESS = 30/11.
 * Every autocovariance is an exact rational of integer counts, so the one decision the rule turns on is taken without
 * rounding; there is no guard band.
 */
#ifndef MCMCREF_IESS_H
#define MCMCREF_IESS_H

#include "mcmcref_hip.h"

#pragma GCC visibility push(default)
#ifdef __cplusplus
extern "C" {
#endif

#define MCI_VERSION 100
#define MCI_MAX_REQUESTS 32   /* requests (lower, upper] of one call: 1 <= K <= 32 */
#define MCI_MAX_DRAWS 1048576 /* draws per chain, 2^20: A_c fits 64 bits */
#define MCI_LAG_BLOCK 256     /* lags of one step of the walk, one per thread; part of R's summation order */
#define MCI_LDS_WORDS 8192    /* the lag kernel stages a request's words in LDS when C * (ceil(N / 64) + 1) <= this */
#define MCI_KERNEL_PACK 0     /* mci_kernel_ms: index of the pack kernel's time */
#define MCI_KERNEL_LAG 1      /* ... of the lag kernel's */
#define MCI_KERNELS 2

/* The library's version, MCI_VERSION. */
int mci_version(void);
/* A handle on HIP device `device`: a stream and device workspace that only grows.  MCR_ENODEVICE when the
 * device cannot be used; then mci_last_error(NULL) holds the message. */
int mci_init(int device, void** handle);
void mci_free(void* handle);
/* The message of the last failed call on the handle (NULL: of this thread's last failed mci_init or
 * mci_indicator_ess_host). */
const char* mci_last_error(void* handle);
/* Upper bound in bytes of the device workspace of one chunk of parameters (default 1 GiB).  A call cuts its parameters
 * into chunks under it; MCR_ENOMEM from a later call when one parameter alone does not fit. */
int mci_set_workspace_limit(void* handle, size_t bytes);
/* Parameters per chunk of a call of this shape under the handle's limit (mci_indicator_ess_dev makes the same cut). */
int mci_indicator_plan(void* handle, int dtype, int64_t C, int64_t N, int64_t P, int K, int64_t* params_per_chunk);

/* The statistic for every parameter p < P and request k < K of a draw tensor in device memory: element (c, n, p) is at
 * draws_dev[c stride_c + n stride_n + p stride_p] (strides in elements, >= 0), dtype MCR_F64 or MCR_F32.  lower, upper
 * [P][K] and the outputs ess, trunc, ones [P][K] are on the host; a NULL output is skipped; ones = Ksum.
 * Two kernels per chunk.  k_pack reads every draw once for all K requests and writes bits[p][k][c][ceil(N / 64) + 1]
 * (bit t % 64 of word t / 64 is b[c][t]; the bits past N and the last word are zero) on one of two routes that give the
 * same words: stride_n == 1: a wave takes 64 consecutive draws and one ballot per request; otherwise a workgroup stages a
 * tile of 64 parameters x 64 draws in LDS (coalesced rows when stride_p == 1, the sampler's [C][N][P] layout; per-lane,
 * uncoalesced loads at any other strides) and a lane builds the words of its parameter.  k_c is not stored by it: k_lag,
 * one workgroup per (parameter, request), stages the words in LDS when they fit (MCI_LDS_WORDS; else reads them from
 * global memory), builds running popcounts over the words (they give k_c, H_c and T_c), and walks the lags in blocks of
 * MCI_LAG_BLOCK, one lag per thread: S_c = sum_w popcount(B[w] & funnel(B[w + q], B[w + q + 1], r)), lag = 64 q + r.  It
 * stops after the first block that holds a negative A.
 * A parameter's outputs have the same bits alone, at any place in a batch, under any chunking, on either route and entry.
 * Synchronous.  MCR_EINVAL (the message names the cause): a NULL handle, tensor or threshold pointer; a dtype other than
 * the two; C, N or P < 1; N > MCI_MAX_DRAWS; C * N >= 2^31 - 1; a negative stride; K < 1 or K > MCI_MAX_REQUESTS; a NaN
 * threshold.  After an error the handle stays usable. */
int mci_indicator_ess_dev(void* handle, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                          int64_t stride_n, int64_t stride_p, const double* lower, const double* upper, int K, double* ess,
                          int64_t* trunc, int64_t* ones);
/* The same on a tensor in host memory, which it uploads (the span the strides reach) to a cached device buffer. */
int mci_indicator_ess(void* handle, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                      int64_t stride_n, int64_t stride_p, const double* lower, const double* upper, int K, double* ess,
                      int64_t* trunc, int64_t* ones);
/* The definition on the host for one parameter: chains [C][N] doubles, lower / upper / outputs [K].  No handle, no
 * device; the same limits and refusals.  Same bits as the device. */
int mci_indicator_ess_host(const double* chains, int64_t C, int64_t N, const double* lower, const double* upper, int K,
                           double* ess, int64_t* trunc, int64_t* ones);

/* Per-kernel times: when enabled (on != 0) every later mci_indicator_ess* call brackets its kernels with HIP events;
 * mci_kernel_ms writes the LAST call's totals over its chunks in milliseconds, ms[MCI_KERNEL_PACK] and
 * ms[MCI_KERNEL_LAG] (cap >= MCI_KERNELS, else MCR_EINVAL; zeros when the last call was not timed). */
int mci_profile_enable(void* handle, int on);
int mci_kernel_ms(void* handle, double* ms, int cap);

#ifdef __cplusplus
}
#endif
#pragma GCC visibility pop

#endif
