/*
 * mcmcref_std.h -- the C ABI of libmcmcref_std.so, a companion library of libmcmcref_hip.so: R-hat and ESS in the
 * STAN CONVENTION -- split chains, Blom scores, Geyer's initial positive and monotone sequence -- as stansummary,
 * posterior::summarise_draws (rhat, ess_bulk, ess_tail, ess_mean, mcse_mean) and arviz.summary define them (Vehtari,
 * Gelman, Simpson, Carpenter, Buerkner 2021: "Rank-normalization, folding, and localization").  The main library's
 * numbers follow the reference's definitions instead (unsplit chains for ESS, truncation at the first negative rho, rank
 * offset (r - 0.5) / M); both are kept, for their two audiences.  Entries are prefixed mcs_, constants MCS_.  This header
 * takes from mcmcref_hip.h the return codes (MCR_OK, MCR_EINVAL, MCR_EHIP, MCR_ENOMEM, MCR_ENODEVICE, MCR_ENONFINITE) and
 * the dtype constants (MCR_F64, MCR_F32) and nothing else.  The library does not link against the main one: it holds a
 * second copy of the main library's code (its sort stage and summary pipeline, linked in as objects, no name of it
 * exported), and an mcs handle owns a context of that copy.  Device addresses come from the caller (for instance
 * mcr_dev_alloc of a ctx on the same device): one process, one HIP runtime, so an address is valid in both.  The caller
 * orders its own work first (mcr_sync) -- an mcs call runs on streams its handle owns.  Calls on one handle are serialised
 * by the caller.
 *
 * Agreement with posterior and ArviZ rests on THIS DEFINITION, written from the papers; no package output pins it.
 *
 * THE DEFINITION.  One parameter, C chains of N >= 2 draws.
 * Split and kept draws.  n = floor(N / 2), m = 2 C split chains; split chain k = 2 c + h (h = 0, 1) holds the draws
 * [h (N - n), h (N - n) + n) of chain c; S = m n kept draws.  For odd N the middle draw of each chain takes part in
 * NOTHING: not the ranks, not the median, not the quantiles (ArviZ's rank and median rule).  For even N the definition
 * coincides with posterior's and ArviZ's.  DEVIATION for odd N: both packages take the tail quantiles, and posterior
 * also the median, over all draws; here they are taken over the kept draws.
 * Series v[k][i], each over the kept draws, in double (an f32 draw is widened exactly):
 *     bulk   inv((r - 3/8) / (S + 1/4)), r the average rank of the draw among the kept draws (ties averaged; -0.0 and
 *            +0.0 tie), inv = AS241 PPND16 (Wichura 1988)
 *     fold   the same score of |x - med|, med = (s[S/2 - 1] + s[S/2]) / 2 of the ascending kept draws s (S is even)
 *     q05, q95   1.0 when x <= q, else 0.0; q the type-7 (numpy "linear") quantile of the kept draws: h = (S - 1) prob,
 *            lo = floor(h), g = h - lo, a = s[lo], b = s[min(lo + 1, S - 1)], q = g >= 0.5 ? b - (b - a)(1 - g) : a + (b - a) g
 *     raw    x itself (only with MCS_WANT_BASIC)
 * Every operation is rounded once, no fused multiply-add.  ONE summation order:
 *     sum64(u_0 .. u_{n-1}): lane l < 64 adds u_l, u_{l+64}, .. in ascending order from +0.0; the 64 lane sums meet in
 *            the halving tree  for (o = 32; o >= 1; o /= 2) a[l] += a[l + o] for l < o
 *     mean_k = sum64(v[k]) / n        d[k][i] = v[k][i] - mean_k        q_k = sum64(d[k]^2)        s2_k = q_k / (n - 1)
 *     sums over chains run in chain order k = 0 .. m - 1 from +0.0
 * R-hat of a series.  mean = (sum_k mean_k) / m,  W = (sum_k s2_k) / m,  V = (sum_k (mean_k - mean)^2) / (m - 1)
 *     rhat = sqrt((n V / W + (n - 1)) / n)
 * rhat_bulk = rhat(bulk), rhat_tail = rhat(fold), rhat = the larger as Python's max(rhat_bulk, rhat_tail) gives it;
 * rhat_basic = rhat(raw).
 * ESS of a series (Geyer 1992 as Stan applies it).
 *     gamma_k(t) = (sum_{i < n - t} d[k][i] d[k][i + t]) / n      one accumulator from +0.0, ascending i, each product
 *                  rounded before its addition: biased, with the chain's own mean
 *     gamma(t)   = (sum_k gamma_k(t)) / m
 *     mean_var   = gamma(0) n / (n - 1)         var_plus = gamma(0) + V
 *     rho_t      = 1 - (mean_var - gamma(t)) / var_plus
 * The walk, with rho_0 = 1 (as a constant), rho_1 by the formula, t = 0:
 *     1. while t < n - 5 and rho_t + rho_{t+1} > 0:  t += 2, compute rho_t and rho_{t+1}, store them when their sum
 *        is >= 0 (the stored values at a lag never stored are 0)
 *     2. max_t = t
 *     3. if the last even rho computed is > 0 it replaces the stored rho_{max_t}
 *     4. monotone pass: for t = 2, 4, .. <= max_t - 2, when rho_t + rho_{t+1} > rho_{t-2} + rho_{t-1} set both to
 *        (rho_{t-2} + rho_{t-1}) / 2
 *     5. tau = -1 + 2 (sum_{t < max_t} rho_t) + rho_{max_t}     the sum in ascending t from +0.0
 *     6. tau = max(tau, 1 / log10(S))
 *     7. ESS = S / tau
 * (The pass of step 4 looks one pair back only, so the routines settle the pair at t when the walk moves on to t + 2
 * and keep no array of rho: the same numbers in the same order.)
 * Outputs per parameter: rhat, rhat_bulk, rhat_tail; ess_bulk = ESS(bulk) with lag_bulk = max_t; ess_q05, ess_q95 with
 * lag_q05, lag_q95; ess_tail = the smaller of ess_q05 and ess_q95, NaN when either is NaN; margin = the smallest
 * |rho_t + rho_{t+1}| the bulk walk evaluated (t = 0 included): how far the walk's decisions were from a tie.  With
 * MCS_WANT_BASIC in flags: rhat_basic, ess_mean = ESS(raw) with lag_mean, and mcse_mean = sd / sqrt(ess_mean),
 * sd = sqrt((sum_k (q_k + n (mean_k - mean)^2)) / (S - 1)) of the raw series: the ddof-1 standard deviation of the kept
 * draws.  Without the flag those four are NaN, NaN, -1 and NaN.
 * Edge rules.  n < 4: every ESS is NaN, every lag -1, margin NaN (the R-hats follow the formula; n = 1 gives NaN).  A
 * series constant over all kept draws (min == max), or var_plus not > 0: its ESS and R-hat are NaN, its lag -1 -- heavy
 * ties can make an indicator constant.  m == 1 cannot happen after the split.  Non-finite draws: MCR_ENONFINITE, as the
 * pipeline reports them.
 * Example (raw series): one chain 1, 2, 3, 4, 5, 6, 7, 8, 1, 8, 2, 7, 3, 6, 4, 5 -- n = 8, m = 2, S = 16, both means
 * 4.5 -- has gamma(0) = 5.25, gamma(1) = -0.5, gamma(2) = 2.375, gamma(3) = -1.3125, mean_var = 6, var_plus = 5.25 (V = 0):
 * rho_1 = -5/21 = -0.238095238095238, rho_2 = 13/42 = 0.309523809523810, rho_3 = -11/28 = -0.392857142857143.  The walk
 * takes one step (1 + rho_1 > 0, 0 < n - 5 = 3) and stops at max_t = 2 with rho_2 + rho_3 = -1/12 < 0: the pair is not
 * stored, but rho_2 > 0 replaces the stored 0.  tau = -1 + 2 (1 + rho_1) + rho_2 = 5/6 = 0.833333333333333, above
 * 1 / log10(16) = 0.830482023721841: ess_mean = 16 / tau = 19.2, lag_mean = 2, and the walk's margin is 1/12.
 * Cost.  O(n max_t) products per chain and series: a converged series ends within the first block of lags, a run that
 * has not converged walks to n - 5, O(n^2).  There is no FFT tier.
 * Device and host: the host routine is this definition in C; the device computes the same sums in the same order, with
 * the device's inv, log10 and sqrt, which differ from libm's by an ulp or two in the tails: the two agree to 1e-9
 * relative, NOT in bits; the lags agree exactly whenever margin is well above that.
 */
#ifndef MCMCREF_STD_H
#define MCMCREF_STD_H

#include "mcmcref_hip.h"

#pragma GCC visibility push(default)
#ifdef __cplusplus
extern "C" {
#endif

#define MCS_VERSION 100
#define MCS_MAX_DRAWS 1048576 /* draws per chain, 2^20 */
#define MCS_LAG_BLOCK 256     /* lags of one step of the walk kernel, one per thread */
#define MCS_LDS_DRAWS 7680    /* the walk kernel stages a split chain's deviations in LDS when n <= this */
#define MCS_WANT_BASIC 1      /* flags: also the raw series (rhat_basic, ess_mean, lag_mean, mcse_mean) */
#define MCS_KERNEL_PIPE 0     /* mcs_kernel_ms: the copy of the kept draws and the summary pipeline */
#define MCS_KERNEL_SERIES 1   /* ... the series kernel */
#define MCS_KERNEL_WALK 2     /* ... the walk kernel */
#define MCS_KERNELS 3

/* The library's version, MCS_VERSION. */
int mcs_version(void);
/* A handle on HIP device `device`: a context of the library's own copy of the summary pipeline (streams, workspace
 * that only grows).  MCR_ENODEVICE when the device cannot be used; then mcs_last_error(NULL) holds the message. */
int mcs_init(int device, void** handle);
void mcs_free(void* handle);
/* The message of the last failed call on the handle (NULL: of this thread's last failed mcs_init or
 * mcs_diagnostics_host). */
const char* mcs_last_error(void* handle);
/* Upper bound in bytes of the device workspace of one chunk of parameters.  A call cuts its parameters into chunks
 * under it; MCR_ENOMEM from a later call when one parameter alone does not fit. */
int mcs_set_workspace_limit(void* handle, size_t bytes);
/* Parameters per chunk of a call of this shape under the handle's limit (mcs_diagnostics_dev makes the same cut). */
int mcs_plan(void* handle, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c, int64_t stride_n, int64_t stride_p,
             int flags, int64_t* params_per_chunk);

/* The diagnostics of every parameter p < P of a draw tensor in device memory: element (c, n, p) is at
 * draws_dev[c stride_c + n stride_n + p stride_p] (strides in elements, >= 0), dtype MCR_F64 or MCR_F32.  flags: 0 or
 * MCS_WANT_BASIC.  The outputs are host arrays [P]; a NULL output is skipped.
 * Per chunk: contiguous f64 [P][C][N] with an even N is read in place as [P][2 C][n]; anything else is copied to f64
 * kept draws (odd N: by a copy that skips each chain's middle draw).  The summary pipeline runs on the kept draws as one
 * chain of S draws and leaves the 5 % and 95 % quantiles and the tie-averaged rank codes of x and |x - med| in time order.
 * k_mcs_series, a wave per split chain, decodes the series (a Blom table of 2 S entries, cached per S), takes the chain
 * moments and writes the deviations; k_mcs_walk, a workgroup per (parameter, series), takes the lag products in blocks of
 * MCS_LAG_BLOCK lags, one lag per thread, the chains in chain order (staged in LDS when n <= MCS_LDS_DRAWS), pools them
 * and walks; it stops after the block in which the walk ends.
 * A parameter's outputs have the same bits alone, at any place in a batch, under any chunking, for every layout and
 * dtype route and on either entry.  Synchronous.  MCR_ENONFINITE when a draw is NaN or infinite (the outputs are then
 * unspecified).  MCR_EINVAL (the message names the cause): a NULL handle or tensor pointer; a dtype other than the two;
 * C or P < 1; N < 2; N > MCS_MAX_DRAWS; C * N >= 2^31 - 1; a negative stride; a flag other than MCS_WANT_BASIC.  After an
 * error the handle stays usable. */
int mcs_diagnostics_dev(void* handle, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                        int64_t stride_n, int64_t stride_p, int flags, double* rhat, double* rhat_bulk, double* rhat_tail,
                        double* ess_bulk, double* ess_tail, double* ess_q05, double* ess_q95, double* margin, double* rhat_basic,
                        double* ess_mean, double* mcse_mean, int64_t* lag_bulk, int64_t* lag_q05, int64_t* lag_q95,
                        int64_t* lag_mean);
/* The same on a tensor in host memory, which it uploads (the span the strides reach). */
int mcs_diagnostics(void* handle, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                    int64_t stride_n, int64_t stride_p, int flags, double* rhat, double* rhat_bulk, double* rhat_tail,
                    double* ess_bulk, double* ess_tail, double* ess_q05, double* ess_q95, double* margin, double* rhat_basic,
                    double* ess_mean, double* mcse_mean, int64_t* lag_bulk, int64_t* lag_q05, int64_t* lag_q95, int64_t* lag_mean);
/* The definition on the host for one parameter: chains [C][N] doubles, every output [1].  No handle, no device; the
 * same limits and refusals (MCR_ENONFINITE leaves the outputs untouched). */
int mcs_diagnostics_host(const double* chains, int64_t C, int64_t N, int flags, double* rhat, double* rhat_bulk, double* rhat_tail,
                         double* ess_bulk, double* ess_tail, double* ess_q05, double* ess_q95, double* margin, double* rhat_basic,
                         double* ess_mean, double* mcse_mean, int64_t* lag_bulk, int64_t* lag_q05, int64_t* lag_q95,
                         int64_t* lag_mean);

/* Per-phase times: when enabled (on != 0) every later mcs_diagnostics* call brackets its phases with HIP events (and
 * waits after every chunk); mcs_kernel_ms writes the LAST call's totals over its chunks in milliseconds,
 * ms[MCS_KERNEL_PIPE], ms[MCS_KERNEL_SERIES] and ms[MCS_KERNEL_WALK] (cap >= MCS_KERNELS, else MCR_EINVAL; zeros when the
 * last call was not timed). */
int mcs_profile_enable(void* handle, int on);
int mcs_kernel_ms(void* handle, double* ms, int cap);

#ifdef __cplusplus
}
#endif
#pragma GCC visibility pop

#endif
