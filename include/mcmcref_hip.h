/*
 * mcmcref_hip.h -- C ABI of libmcmcref_hip.so, the MI355X (gfx950) implementation of the
 * draw-vs-reference statistics hot path of StefanSko/mcmc-db (`mcmc_ref` 0.1.4).
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  A Python
 * host binds it with ctypes (mcmc-db_amd/mcmc_ref_hip/_ffi.py; the reference-side stub is
 * shown in INTEGRATION.md).  Each entry point names the reference interface it replaces
 * (file:line relative to the reference repo root).
 *
 * Conventions
 *   - every function returns MCR_OK (0) or a negative MCR_E* code and never throws/aborts;
 *     mcr_last_error(ctx) returns a human-readable message for the last failure on ctx.
 *   - the caller owns every host buffer; the library owns all device scratch in mcr_ctx.
 *   - one mcr_ctx == one GPU + its HIP streams ("lanes", see mcr_init).  Calls on one ctx must be
 *     serialised by the caller; different ctxs are independent (one process per GPU, one ctx per
 *     thread, or several ctxs in one thread).
 *   - tensors are described by element strides (stride_c, stride_n, stride_p), so both the
 *     Arrow column layout [P][C][N] and `Draws.to_numpy` layout [C][N][P] (src/mcmc_ref/draws.py:28-29)
 *     are accepted without a host-side copy.  Any non-negative strides are accepted, padded, sliced and thinned
 *     views included; zero or aliasing strides (broadcast views, parameters or chains sharing elements) are read as
 *     they are: the library only reads the draws.
 *   - dtype: MCR_F64 (the reference's only dtype) or MCR_F32 (widened to f64 on load).
 *   - NaN/Inf in the draws are rejected with MCR_ENONFINITE (the reference's behaviour for
 *     them is undefined: sort order with NaN).
 */
#ifndef MCMCREF_HIP_H
#define MCMCREF_HIP_H

#include <stddef.h>
#include <stdint.h>

#pragma GCC visibility push(default)
#ifdef __cplusplus
extern "C" {
#endif

#define MCR_VERSION 100 /* 0.1.0 */

#define MCR_OK 0
#define MCR_EINVAL (-1)         /* null pointer, negative size, unsupported dtype/quantile count */
#define MCR_EMINCHAINS (-2)     /* C < min_chains: "... require at least k chains; got m chain(s)"
                                   (src/mcmc_ref/diagnostics.py:25-28, 49-52, 65-68) */
#define MCR_EMINCHAINS_ARG (-3) /* min_chains < 1: "min_chains must be >= 1; got k" (diagnostics.py:88-90) */
#define MCR_ENONFINITE (-4)     /* NaN/Inf found in the draws */
#define MCR_EHIP (-5)           /* HIP runtime error (message has the hipError string) */
#define MCR_ENOMEM (-6)         /* host or device allocation failed */
#define MCR_ENODEVICE (-7)      /* no usable HIP device / bad device index */
#define MCR_ECOMM (-8)          /* RCCL error (multi-GPU gather) */
#define MCR_ELAYOUT (-9)        /* mcr_summarize_files: rows not in (chain, draw) order or chains of unequal length */
#define MCR_EFALLBACK (-10)     /* mcr_json_*: valid input for the caller's host reader, but outside the subset the device
                                   reader certifies; the message names the first reason and its byte offset.
                                   mcr_chain_layout_dev: the chain-id and draw-index ranges of the table need more than
                                   64 bits together, so no packed row key exists; the caller sorts on the host
                                   (np.lexsort) and takes mcr_gather_rows_dev */

#define MCR_F64 0
#define MCR_F32 1

#define MCR_MAX_QUANTILES 32

typedef struct mcr_ctx mcr_ctx;

/* Per-parameter results, struct-of-arrays, caller allocated.  Every non-NULL array has P
 * entries, except q (P * n_q, row-major [p][k]) and q_lo (n_q).  NULL members are skipped; when
 * every diagnostics member (rhat* / ess_* / lag_*) is NULL the rank / fold / autocovariance
 * kernels are not launched at all (Backend.stats-only call).
 *
 *  mean, std, q   Backend.stats(): pooled mean, population std (ddof=0), linear-interpolated
 *                 quantiles (src/mcmc_ref/backends.py:14-24, backends_arrow.py:36-51,
 *                 backends_numpy.py:40-47).  q_lo[k] = floor((M-1)*q_k): the order-statistic
 *                 index (integer, bit-exact gate).
 *  median         statistics.median of the pooled draws, the fold point (diagnostics.py:97).
 *                 Where the middle draws are zeros of mixed sign, the earlier ones in time order count as the
 *                 smaller, as in Python's sorted(); a median that only rounds to zero keeps the sign of the sum.
 *  rhat           split_rhat(): max(rhat_bulk, rhat_tail) with Python max() NaN ordering
 *                 (diagnostics.py:13-40); rhat_bulk / rhat_tail are its two operands.
 *  ess_bulk/tail  ess_bulk(), ess_tail() (diagnostics.py:43-73).
 *  lag_bulk/tail  number of autocorrelation terms accumulated before the first negative rho
 *                 (diagnostics.py:171-177) -- integer, bit-exact gate.
 */
typedef struct mcr_summary {
    double* mean;
    double* std;
    double* q;
    double* median;
    double* rhat;
    double* rhat_bulk;
    double* rhat_tail;
    double* ess_bulk;
    double* ess_tail;
    int64_t* lag_bulk;
    int64_t* lag_tail;
    int64_t* q_lo;
} mcr_summary;

/* Accumulated HIP-event time of one kernel since profiling was last reset. */
typedef struct mcr_kernel_time {
    char name[48];
    int64_t launches;
    double total_ms;
} mcr_kernel_time;

/* ---- lifecycle -------------------------------------------------------------------- */
int mcr_version(void);
int mcr_device_count(void);
/* Creates a context bound to HIP device `device` (own non-blocking streams, lazily grown
 * workspaces).  Fails with MCR_ENODEVICE when no GPU is present: there is no CPU fallback.
 * Environment read here: MCR_LANES (streams + workspaces that consecutive calls rotate over,
 * default 4, max MCR_MAX_INFLIGHT), MCR_WORKSPACE_MB (see mcr_set_workspace_limit).
 * Limits: C <= 256 chains, C * N < 2^31 pooled draws per parameter (rank codes are 32-bit),
 * any number of parameters (chunked through the workspace). */
int mcr_init(int device, mcr_ctx** out);
void mcr_free(mcr_ctx* ctx);
const char* mcr_last_error(const mcr_ctx* ctx); /* ctx may be NULL: last mcr_init failure */
/* Upper bound for device scratch (bytes); parameters are processed in chunks that fit.
 * Default: MCR_WORKSPACE_MB env or 8192 MiB. */
int mcr_set_workspace_limit(mcr_ctx* ctx, size_t bytes);

/* How the parameters of a call of this shape are cut into workspace chunks: parameters [k * n, (k + 1) * n) are
 * processed together, n = *params_per_chunk (a function of the shape, the strides' layout class, the workspace limit and
 * MCR_FFT).  The reference has no counterpart (its loop is per parameter, src/mcmc_ref/convert.py:140-147); tests and
 * bench.py use it to put oracle-checked parameters on both sides of every chunk edge. */
int mcr_plan_chunks(mcr_ctx* ctx, int64_t C, int64_t N, int64_t P, int64_t stride_c, int64_t stride_n, int64_t stride_p,
                    int diagnostics, int64_t* params_per_chunk);

/* mcr_plan_chunks for a ragged call (mcr_summarize_chains_enqueue) on contiguous parameters (stride_p == chain_off[C]).
 * 0 for a call without draws. */
int mcr_plan_chunks_chains(mcr_ctx* ctx, const int64_t* chain_off, int C, int64_t P, int diagnostics,
                           int64_t* params_per_chunk);

/* How many autocorrelation lags this context has re-derived the reference's way so far: no tier of the ESS walk takes
 * a `rho < 0` decision (src/mcmc_ref/diagnostics.py:171-177) on a value within MCR_RHO_BAND (default 1e-10) of zero --
 * segment records + mean correction below lag 256, tree sums or FFTs beyond; such a lag is recomputed with _autocorr's
 * own left-to-right sums and the chain's left-to-right mean (diagnostics.py:180-193) first.  A diagnostic: tests use it
 * to show that the guard ran.  Waits for the calls in flight. */
int mcr_rho_guard_count(mcr_ctx* ctx, int64_t* rederived);

/* How many 4096-draw tiles of f64 draws this context has sorted as (key, position) pairs so far, after their sort as
 * 64-bit records (upper 52 bits of the draw + tile slot) failed its order check: draws of one tile that agree in their
 * upper 52 bits and whose low bits order them against their slots.  A diagnostic: tests use it to show which path ran.
 * Waits for the calls in flight. */
int mcr_tile_fallback_count(mcr_ctx* ctx, int64_t* tiles);

/* ---- device memory plumbing (for device-resident benchmarking and pipelines) --------- */
int mcr_dev_alloc(mcr_ctx* ctx, size_t bytes, void** dptr);
int mcr_dev_free(mcr_ctx* ctx, void* dptr);
int mcr_memcpy_h2d(mcr_ctx* ctx, void* dptr, const void* hptr, size_t bytes);
int mcr_memcpy_d2h(mcr_ctx* ctx, void* hptr, const void* dptr, size_t bytes);
int mcr_sync(mcr_ctx* ctx);

/* ---- the hot path ------------------------------------------------------------------ */
/* Everything the reference computes per parameter over a (C chains x N draws x P params)
 * tensor, in one call: replaces the per-parameter Python loops of
 *   convert._compute_diagnostics            (src/mcmc_ref/convert.py:134-147)
 *   reference.diagnostics_for_model         (src/mcmc_ref/reference.py:92-104)
 *   Backend.stats                            (src/mcmc_ref/backends_arrow.py:36-51)
 * `draws` is a HOST pointer (copied to the device inside the call). Synchronous. */
int mcr_summarize(mcr_ctx* ctx, const void* draws, int dtype, int64_t C, int64_t N, int64_t P,
                  int64_t stride_c, int64_t stride_n, int64_t stride_p, int min_chains,
                  const double* quantiles, int n_q, mcr_summary* out);
/* Same with `draws` already resident in this ctx's device memory.  Synchronous. */
int mcr_summarize_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N,
                      int64_t P, int64_t stride_c, int64_t stride_n, int64_t stride_p,
                      int min_chains, const double* quantiles, int n_q, mcr_summary* out);
/* Asynchronous form: enqueues the whole pipeline on the ctx stream and returns; results
 * land in `out` (which must stay valid) when mcr_summarize_wait() returns.  At most
 * MCR_MAX_INFLIGHT enqueues may be outstanding per ctx. */
#define MCR_MAX_INFLIGHT 8
int mcr_summarize_enqueue(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N,
                          int64_t P, int64_t stride_c, int64_t stride_n, int64_t stride_p,
                          int min_chains, const double* quantiles, int n_q, mcr_summary* out);
int mcr_summarize_wait(mcr_ctx* ctx);
/* Waits for the OLDEST outstanding enqueue only and fills its `out`; later enqueues keep running, so a
 * caller can hold a rolling window of MCR_MAX_INFLIGHT calls without ever draining the device. */
int mcr_summarize_wait_one(mcr_ctx* ctx);

/* Many independent models in one call (BASELINE configs 2/3: the packaged corpus): every model is a
 * device-resident tensor of this ctx; the calls are pipelined through the lanes with a rolling window
 * of MCR_MAX_INFLIGHT, so small models overlap.  Replaces the per-model loop of
 * generate.generate_reference_corpus -> convert_file (src/mcmc_ref/generate.py:77-96).  outs[i] receives
 * model i.  Stops at the first failing model and returns its code (earlier models are delivered). */
typedef struct mcr_model_desc {
    const void* draws_dev;
    int dtype;
    int min_chains;
    int64_t C, N, P;
    int64_t stride_c, stride_n, stride_p;
} mcr_model_desc;
int mcr_summarize_models(mcr_ctx* ctx, const mcr_model_desc* models, int n_models, const double* quantiles,
                         int n_q, mcr_summary* outs);

/* diagnostics.split_rhat / ess_bulk / ess_tail for ONE parameter given as possibly ragged
 * chains (src/mcmc_ref/diagnostics.py:13-73): `pooled` holds the chains back to back, chain c
 * is pooled[chain_off[c] .. chain_off[c+1]), chain_off being C + 1 non-decreasing entries
 * starting at 0.  Host pointers.  out arrays have 1 entry.
 * Optional debug outputs (host, length chain_off[C], may be NULL): z_bulk / z_tail =
 * _rank_normalize(x) / _rank_normalize(_fold_chains(x)) (diagnostics.py:93-133), rank_bulk /
 * rank_tail = the average ranks (exact multiples of 0.5). */
int mcr_diagnose_chains(mcr_ctx* ctx, const double* pooled, const int64_t* chain_off, int C,
                        int min_chains, mcr_summary* out, double* z_bulk, double* z_tail,
                        double* rank_bulk, double* rank_tail);

/* Every statistic of P parameters whose chains differ in length, in ONE pipeline (the per-parameter loop of
 * convert._compute_diagnostics, src/mcmc_ref/convert.py:134-147, over chains `_chains_from_table` left ragged,
 * :150-161).  draws_dev: f64 device memory, parameter p at draws_dev[p * stride_p .. + M), M = chain_off[C], its chains
 * back to back in (chain, draw) order: chain c is [chain_off[c], chain_off[c + 1]).  chain_off is a HOST array of C + 1
 * non-decreasing entries starting at 0; it is copied by the call.  stride_p >= M; stride_p != M goes through one ingest
 * pass.  mean / std / q / q_lo / median are taken over the M pooled draws (Backend.stats); the diagnostics are
 * diagnostics.py's for ragged chains, exactly as mcr_diagnose_chains computes them (ranks over all pooled draws, n = the
 * shortest chain, halves of len / 2 per chain, a chain of one draw contributes no halves; diagnostics.py:13-85,
 * 154-193).  All diagnostics members NULL: Backend.stats only, no rank or autocovariance kernel is launched.
 * Slots, lanes, chunking under the workspace limit, mcr_summarize_wait / _wait_one: as mcr_summarize_enqueue, and calls
 * of both kinds may be in flight together.  Errors as mcr_diagnose_chains: MCR_EMINCHAINS_ARG, MCR_EMINCHAINS,
 * MCR_EINVAL (C > 256, M >= 2^31 - 1, a decreasing table), MCR_ENONFINITE at the wait; M == 0 or P == 0 gives NaN. */
int mcr_summarize_chains_enqueue(mcr_ctx* ctx, const double* draws_dev, int64_t stride_p, const int64_t* chain_off, int C,
                                 int64_t P, int min_chains, const double* quantiles, int n_q, mcr_summary* out);
/* mcr_summarize_chains_enqueue + mcr_summarize_wait */
int mcr_summarize_chains_dev(mcr_ctx* ctx, const double* draws_dev, int64_t stride_p, const int64_t* chain_off, int C,
                             int64_t P, int min_chains, const double* quantiles, int n_q, mcr_summary* out);

/* compare.compute_basic_stats (src/mcmc_ref/compare.py:58-64): mean and population std of n
 * host values; n == 0 gives NaN, NaN.  Also the streaming "moments" kernel (HBM-bound). */
int mcr_basic_stats(mcr_ctx* ctx, const void* values, int dtype, int64_t n, double* mean,
                    double* std);
/* Pooled mean / population std per parameter of a device-resident tensor (one HBM pass). */
int mcr_moments_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N,
                    int64_t P, int64_t stride_c, int64_t stride_n, int64_t stride_p,
                    double* mean, double* std);
/* compare.compare_stats inner arithmetic (src/mcmc_ref/compare.py:38-43) on n (ref, actual)
 * pairs: rel = |a-r| / max(|r|, 1e-12), pass = rel <= tol (NaN -> 0).  Host pointers. */
int mcr_compare(mcr_ctx* ctx, const double* ref, const double* actual, int64_t n, double tol,
                double* rel_error, uint8_t* passed);

/* ---- extensions (named in the north star, ABSENT from the reference: parity unpinned by it) ----- */
/* Two-sample Kolmogorov-Smirnov statistic and Wasserstein-1 distance per parameter between the
 * reference draws ref[P][Mr] and the actual draws act[P][Ma] (host pointers, row-major, finite).
 * Definitions follow scipy.stats.ks_2samp(...).statistic and scipy.stats.wasserstein_distance:
 * both samples are sorted on the device and compared in one merge-path pass.  SURVEY.md rows X1, X2. */
int mcr_two_sample(mcr_ctx* ctx, const double* ref, int64_t Mr, const double* act, int64_t Ma, int64_t P,
                   double* ks, double* w1);
/* Sliced two-sample check: both samples are projected onto K directions and every projected row goes through the
 * two-sample pass above, so a difference in the DEPENDENCE between parameters that no marginal shows is seen as a KS /
 * W1 along some direction.  ref[P][Mr], act[P][Ma] as in mcr_two_sample; dirs[K][P], center[P] (NULL = zeros), host.
 *     z[k][m] = sum_p dirs[k][p] * (x[p][m] - center[p])
 * in ONE fixed order: the accumulator starts at +0.0 and, for p = 0 .. P-1, d = x[p][m] - center[p] is rounded once
 * and acc = fma(dirs[k][p], d, acc).  z[k][m] therefore has the same bits whatever K is, wherever k stands in dirs,
 * however the directions are chunked to fit the workspace limit, for odd and even M and any 8-byte alignment of the
 * draws.  ks[k], w1[k]: mcr_two_sample's statistics of (z_ref[k], z_act[k]), the same kernels on the same values.
 * proj_ref[K][Mr] / proj_act[K][Ma]: the projected rows, copied out when not NULL (debug outputs).
 * MCR_EINVAL: a NULL pointer where one is needed, K < 0, P < 1 with K > 0, Mr or Ma < 1, K > 65535, mcr_two_sample's
 * length limits, a non-finite entry of dirs or center, summaries in flight.  MCR_ENONFINITE: non-finite draws, or a
 * projection that overflows.  K == 0: MCR_OK, nothing written.  Synchronous.  Parity unpinned by the reference. */
int mcr_sliced_two_sample(mcr_ctx* ctx, const double* ref, int64_t Mr, const double* act, int64_t Ma, int64_t P,
                          const double* dirs, const double* center, int64_t K, double* ks, double* w1,
                          double* proj_ref, double* proj_act);
/* The same with ref_dev / act_dev in this ctx's device memory; everything else on the host as above. */
int mcr_sliced_two_sample_dev(mcr_ctx* ctx, const double* ref_dev, int64_t Mr, const double* act_dev, int64_t Ma,
                              int64_t P, const double* dirs, const double* center, int64_t K, double* ks, double* w1,
                              double* proj_ref, double* proj_act);
/* Directions per workspace chunk of such a call under the current workspace limit (K when all fit at once; 0 for an
 * empty shape).  MCR_ENOMEM when the limit does not fit one direction. */
int mcr_sliced_plan(mcr_ctx* ctx, int64_t Mr, int64_t Ma, int64_t P, int64_t K, int64_t* dirs_per_chunk);
#define MCR_PROJ_TILE_M 512  /* draws per k_project workgroup (two per lane) */
#define MCR_PROJ_TILE_K 8    /* directions per k_project workgroup (accumulators in registers) */
#define MCR_PROJ_CHUNK_P 64  /* parameters whose weights and centers a k_project workgroup stages in LDS at a time */
/* Energy distance (Szekely and Rizzo, "Energy statistics: a class of statistics based on distances"): the direction-free
 * counterpart of the sliced check, a two-sample statistic of the JOINT distribution without a seed, a number of
 * directions or any tuning parameter.  ABSENT from the reference.
 *     E(X, Y) = 2 E|X - Y| - E|X - X'| - E|Y - Y'|
 * As a V-statistic it is non-negative; in the population it is zero only when the two distributions are equal; it is
 * rotation invariant.  ref[P][Mr], act[P][Ma]: f64, row-major, as for mcr_two_sample.  scale[P]: finite and >= 0, NULL
 * means all ones.  For two draws x and y of either sample, everything in IEEE double:
 *     1. the scaled value is u_p = x_p * scale_p, rounded once (scale == NULL: x_p itself);
 *     2. acc starts at +0.0;
 *     3. for p = 0 .. P-1 in order, t = u_p(x) - u_p(y), rounded once, and acc = fma(t, t, acc);
 *     4. d(x, y) = sqrt(acc), correctly rounded.
 * So d has the same bits wherever the pair sits in a tile, a launch or a chunk of parameters; d(x, y) = d(y, x) exactly;
 * d(x, x) = +0.0 exactly; a parameter with scale 0 drops out.  The three pair sums
 *     S_xy = sum_{i < Mr, j < Ma} d(ref_i, act_j)    S_xx = sum_{i, j < Mr} d(ref_i, ref_j)    S_yy = sum_{i, j < Ma} d(act_i, act_j)
 * (S_xx and S_yy include their zero diagonals) are each taken in an order that depends on (Mr, Ma, P) only: a call gives
 * the same bits on the host entry and on the device entry, on repeated calls, under any workspace limit, with or without
 * profiling.  out[0..5], in this order:
 *     A = S_xy / (double)(Mr Ma)     B = S_xx / (double)(Mr Mr)     C = S_yy / (double)(Ma Ma)      (one division each)
 *     E = (A - B) + (A - C)          H = E / (2 A), or 0 when A == 0                                 (in [0, 1])
 *     T = Mr Ma / (Mr + Ma) * E      (the test statistic of the energy two-sample test)
 * B and C are the V-statistic means; M / (M - 1) times either is the U-statistic mean over the M (M - 1) pairs i != j.
 * NO p-value is offered: a permutation test needs the pooled (Mr + Ma)^2 distance matrix, tens of gigabytes at these
 * sizes, and assumes independent draws, which MCMC output is not.  E is a distance to be thresholded, like sliced_w1.
 * Cost: O(M^2 P).  A call is refused when (Mr Ma + Mr (Mr + 1) / 2 + Ma (Ma + 1) / 2) P > MCR_ENERGY_MAX_WORK, and no
 * single launch carries more than MCR_ENERGY_LAUNCH_WORK pair-parameters: with J = ceil(Mr / TI) ceil(Ma / TJ) +
 * T(ceil(Mr / TI)) + T(ceil(Ma / TI)) tile jobs, T(n) = n (n + 1) / 2, a call is ceil(J / max(1, floor(MCR_ENERGY_LAUNCH_WORK
 * / (TI TJ P)))) launches of k_energy_pairs (the jobs spread evenly over them) and one of k_energy_reduce.  The
 * environment variable MCR_ENERGY_LAUNCH_WORK, read once at mcr_init, lowers the launch budget (tests; no bit changes).
 * MCR_EINVAL (the message names the cause): a NULL pointer, Mr or Ma < 1, P < 1, a negative or non-finite scale,
 * summaries in flight, work over the limit.  MCR_ENONFINITE: non-finite draws, or a squared distance that overflows.
 * MCR_ENOMEM (naming the need): the workspace limit does not fit the partials.  The context stays usable after every
 * error.  Synchronous.  Parity unpinned by the reference. */
int mcr_energy_distance(mcr_ctx* ctx, const double* ref, int64_t Mr, const double* act, int64_t Ma, int64_t P,
                        const double* scale, double* out6);
/* The same with ref_dev / act_dev in this ctx's device memory (any 8-byte alignment); scale and out6 on the host. */
int mcr_energy_distance_dev(mcr_ctx* ctx, const double* ref_dev, int64_t Mr, const double* act_dev, int64_t Ma, int64_t P,
                            const double* scale, double* out6);
/* The definition on the host, without a context: the same per-pair arithmetic bit for bit, the pair sums in long double
 * (rounded to double before the one division).  The same argument errors and work limit (codes only, no message). */
int mcr_energy_distance_host(const double* ref, int64_t Mr, const double* act, int64_t Ma, int64_t P, const double* scale,
                             double* out6);
/* Bytes of workspace such a call carves (one partial per tile job, the scales, the results). */
int mcr_energy_workspace(mcr_ctx* ctx, int64_t Mr, int64_t Ma, int64_t P, size_t* bytes);
#define MCR_ENERGY_TILE_I 128   /* draws x draws of a k_energy_pairs workgroup (TI, TJ) */
#define MCR_ENERGY_TILE_J 128
#define MCR_ENERGY_CHUNK_P 8    /* parameters a k_energy_pairs workgroup stages in LDS at a time */
#define MCR_ENERGY_MAX_WORK 17592186044416ll   /* 2^44 pair-parameters of a call */
#define MCR_ENERGY_LAUNCH_WORK 274877906944ll  /* 2^38 pair-parameters of a launch */
/* Nested R-hat: the convergence diagnostic for MANY SHORT chains (Margossian, Hoffman, Sountsov, Riou-Durand, Vehtari,
 * Gelman, "Nested R-hat: assessing the convergence of Markov chain Monte Carlo when running many short chains";
 * rhat_nested of the R package posterior).  ABSENT from the reference: it replaces no reference line, and split R-hat /
 * ESS keep their limit of 256 chains.  The C chains are grouped into K superchains of L chains each (chains of a
 * superchain share a starting point): superchain[c] is any int32 label, labels need be neither contiguous nor sorted,
 * every label must occur equally often (superchains are summed in the order of their first chain, so the labels are
 * names only).  For one kind of value v[c][n], in IEEE double, every variance two-pass:
 *     m_c  = (sum_n v[c][n]) / N                 q_c = sum_n (v[c][n] - m_c)^2
 *     mu_k = (sum_{c in k} m_c) / L              b_k = sum_{c in k} (m_c - mu_k)^2        w_k = sum_{c in k} q_c
 *     mu   = (sum_k mu_k) / K                    B   = sum_k (mu_k - mu)^2 / (K - 1)
 *     W    = (sum_k (b_k / (L - 1) + w_k / (L (N - 1)))) / K        (a term with L == 1 resp. N == 1 is 0)
 *     nrhat = sqrt(1 + B / W);  W == 0: 1.0 when B == 0, else inf;  NaN when K < 2 or C * N == 0
 * Three kinds, as for split R-hat: raw (v = the draws: the paper's definition), bulk (v = z of the pooled tie-averaged
 * ranks) and tail (the same of |x - median|); nrhat = max(nrhat_bulk, nrhat_tail) with Python's NaN ordering.  Chains
 * are not split.  between_* / within_* are B and W.  Every sum has one order that depends on (C, N, K) only: a
 * parameter's results have the same bits alone or in a batch, under any workspace limit, on either entry.
 * draws: host tensor addressed like mcr_summarize's (dtype, C, N, P, element strides; f32 is widened first).
 * Limits: C <= 1 048 576, C * N < 2^31 - 1.  MCR_EINVAL (message names the cause): superchains of unequal size, a NULL
 * superchain with C > 0, C over the limit, summaries in flight.  MCR_ENONFINITE: NaN / Inf draws.  The context stays
 * usable after every error.  Synchronous. */
typedef struct mcr_nested { /* P entries each, NULL members skipped */
    double *nrhat, *nrhat_bulk, *nrhat_tail, *nrhat_raw;
    double *between_bulk, *within_bulk, *between_tail, *within_tail, *between_raw, *within_raw;
} mcr_nested;
int mcr_nested_rhat(mcr_ctx* ctx, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                    int64_t stride_n, int64_t stride_p, const int32_t* superchain, mcr_nested* out);
/* The same on draws in this ctx's device memory; superchain and out stay on the host. */
int mcr_nested_rhat_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                        int64_t stride_n, int64_t stride_p, const int32_t* superchain, mcr_nested* out);
/* Parameters per workspace chunk of such a call with K superchains under the current workspace limit (0 for an empty
 * shape).  MCR_ENOMEM when the limit does not fit one parameter. */
int mcr_nested_plan(mcr_ctx* ctx, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c, int64_t stride_n,
                    int64_t stride_p, int64_t K, int64_t* params_per_chunk);
#define MCR_NESTED_MAX_CHAINS 1048576 /* chains of a mcr_nested_rhat call */
#define MCR_NESTED_BLOCK 512          /* draws of a chain k_chain_moments keeps in registers for its second pass */
/* Pareto k-hat: the tail diagnostic for the draws behind a mean and a std (Vehtari, Simpson, Gelman, Yao, Gabry, "Pareto
 * smoothed importance sampling"; pareto_khat(tail = "both") / pareto_diags of the R package posterior, with Zhang and
 * Stephens' (2009) profile fit, gpdfit).  ABSENT from the reference.  It estimates the shape k of a generalised Pareto
 * distribution fitted to each tail: k < 0.5 the variance is finite and the central limit theorem holds; 0.5 <= k < 0.7 the
 * mean estimate converges slowly and a std gate is not trustworthy; k >= 0.7 the estimate is unreliable; k >= 1 no mean
 * exists.
 * For one parameter, let x_(0) <= ... <= x_(M-1) be its M pooled draws in ascending order.  The chains are pooled and
 * their structure plays no part.  Everything is IEEE double.
 * Tail length.  Each parameter takes a requested length t_req >= 1 from the caller, or the default
 *     t_req = ceil(3 * sqrt(M / r_eff))  when M > 225,  else  floor(M / 5)
 * with r_eff = 1 when none is given.  mcr_pareto_tail_length(M, r_eff) computes the default on the host and needs no
 * device.  It works in integers: the smallest t with t^2 * r_eff >= 9 M (t^2 exact, the product rounded once; capped at
 * 2^31); it does not depend on how a floating-point sqrt rounds.  It returns 0 for M < 1 and MCR_EINVAL unless r_eff is
 * finite and > 0.  The effective length is
 *     t = min(max(t_req, 5), floor(M / 2))
 * If t < 5, that is M < 10, both tails give NaN.
 * Right tail.  Let cutoff = x_(M-t-1) and e_i = x_(M-t+i) - cutoff for i = 0 ... t-1.  The e_i are ascending and >= 0.
 * Left tail.  This is the right tail of -x.  Let cutoff' = x_(t) and e_i = x_(t) - x_(t-1-i).  This is the same
 * subtraction, so khat_left(x) and khat_right(-x) agree in bits.
 * Fit of one tail of n = t exceedances:
 *  1. If e_(n-1) == e_0, the tail is constant: khat = NaN.
 *  2. Let G = 30 + floor(sqrt(n)) and xstar = e_(floor(n/4 + 0.5) - 1).  If xstar == 0: khat = +inf.
 *     (From here on the e_i stand for 2^s e_i, the power of two that brings e_(n-1) into [1, 2), |s| <= 1000: an exact
 *     scaling.  The fit is scale-free in exact arithmetic, but log(-theta_j / k_j) below is not in floating point; read
 *     this way khat(x) and khat(2^m x) agree in bits.  Against the unscaled formulas the difference is rounding, ~1e-13.)
 *  3. For j = 1 ... G:   theta_j = 1/e_(n-1) + (1 - sqrt(G / (j - 0.5))) / 3 / xstar
 *                        k_j = (sum_i log1p(-theta_j e_i)) / n
 *                        l_j = n (log(-theta_j / k_j) - k_j - 1)
 *  4. Let w_j = exp(l_j - L), with L = m + log sum_j exp(l_j - m) and m = max_j l_j.  Then theta = sum_j theta_j w_j.
 *  5. Let k = (sum_i log1p(-theta e_i)) / n.  Then khat = (k n + 5) / (n + 10).  This is the weakly informative prior:
 *     mean 0.5, weight 10.
 *  6. If khat is NaN it becomes +inf.
 * Outputs per parameter: khat_left, khat_right, khat = max(khat_left, khat_right) with Python's max NaN ordering, as
 * for rhat, and ndraws_tail, the effective t as an int64.
 * Summation order.  Every sum over i and over j has one order that depends on n alone (for the j sums on G, itself a
 * function of n): 64 partial sums, partial l adding the terms l, l + 64, ... in order, joined by the tree 32, 16, ... 1.
 * A parameter's outputs therefore have the same bits alone or in a batch, at any place in the batch, under any workspace
 * limit, in either layout, on the host entry or the device entry.  f32 draws are widened first by the ingest pass, as
 * nested R-hat does; the answer is that of the f64 call on the widened tensor.
 * draws: host tensor addressed like mcr_summarize's.  ndraws_tail: P requested lengths, or NULL for the default.
 * Limits: any C, C * N < 2^31 - 1.  MCR_EINVAL (message names the cause): a negative dimension, a ndraws_tail entry < 1,
 * summaries in flight, negative strides.  MCR_ENONFINITE: NaN / Inf draws.  M == 0 gives NaN (ndraws_tail 0), P == 0
 * writes nothing.  The context stays usable after every error.  Synchronous.  A tail beyond MCR_PARETO_LDS_TAIL draws is
 * fitted from global memory, and every tail by ONE workgroup: beyond ~10^5 draws a tail takes milliseconds. */
typedef struct mcr_pareto { double *khat, *khat_left, *khat_right; int64_t* ndraws_tail; } mcr_pareto; /* P entries, NULL skipped */
int mcr_pareto_khat(mcr_ctx* ctx, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                    int64_t stride_n, int64_t stride_p, const int64_t* ndraws_tail /* P entries or NULL */, mcr_pareto* out);
/* The same on draws in this ctx's device memory; ndraws_tail and out stay on the host. */
int mcr_pareto_khat_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                        int64_t stride_n, int64_t stride_p, const int64_t* ndraws_tail, mcr_pareto* out);
/* Parameters per workspace chunk of such a call under the current workspace limit (0 for an empty shape).  MCR_ENOMEM
 * when the limit does not fit one parameter. */
int mcr_pareto_plan(mcr_ctx* ctx, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c, int64_t stride_n,
                    int64_t stride_p, int64_t* params_per_chunk);
int64_t mcr_pareto_tail_length(int64_t M, double r_eff);                 /* host only */
/* The same fit routine on an ascending host array (host only, no ctx; ndraws_tail 0 = the default, NULL outputs are
 * skipped).  It runs the device's text in the device's summation order, but with the host's libm: log1p, log and exp
 * are not the device's, so the results equal the device's to ~1e-13, not in bits.  MCR_EINVAL: M < 0, ndraws_tail < 0,
 * a NULL array.  Non-finite entries are not looked for. */
int mcr_pareto_fit_host(const double* sorted, int64_t M, int64_t ndraws_tail /* 0 = default */,
                        double* khat_left, double* khat_right, int64_t* t_eff);
#define MCR_PARETO_LDS_TAIL 8192      /* the longest tail k_pareto_fit stages in LDS */
/* Pareto-smoothed importance sampling (PSIS) and PSIS-LOO: the second half of the paper cited above (psislw / loo of
 * ArviZ, psis / loo of the R package loo).  ABSENT from the reference.  The largest importance ratios of a column are
 * replaced with the expected order statistics of the generalised Pareto distribution fitted to them and the weights are
 * normalised; from a (chains x draws x observations) tensor of pointwise log-likelihoods this gives elpd_loo, p_loo and a
 * k-hat per observation, the accepted way to compare two models fitted to the same data.
 * For one column of M = C * N pooled values v, everything in IEEE double (f32 is widened first by the ingest pass; the
 * answer is that of the f64 call on the widened tensor).  negate = 0: v are log importance ratios and x = v.  negate = 1
 * (LOO): v are log-likelihoods and x = -v; the negation is exact.  Let x_(0) <= ... <= x_(M-1) be x in ascending order
 * and y_(i) = x_(i) - x_(M-1).
 *  1. Tail length.  A requested length t_req >= 1 from the caller (ndraws_tail), or the default
 *         t_req = min((M + 4) / 5, T)        (integer division),  T the smallest t with t^2 * r_eff >= 9 M
 *     T by mcr_pareto_tail_length's integer bisection; that is ceil(min(M / 5, 3 sqrt(M / r_eff))), loo's and ArviZ's rule
 *     for EVERY M (not posterior's floor(M / 5) below 226 draws, which mcr_pareto_khat follows).  r_eff: per column, 1 when
 *     none is given, finite and > 0; it plays no part where ndraws_tail is given.  mcr_psis_tail_length(M, r_eff) computes
 *     the default on the host (0 for M < 1, MCR_EINVAL for a bad r_eff).  The effective length is t = min(t_req, M - 1).
 *  2. Cutoff and tail.  cut = max(y_(M-t-1), log(DBL_MIN)), log(DBL_MIN) read as the double -708.3964185322641.  The tail
 *     is the n values with y > cut, compared by value: with ties at the cutoff, or with the clamp active, n < t.  If
 *     t == 0 or n <= 4: khat = +inf, nothing is smoothed, the weights are the normalised raw ratios.
 *  3. Fit.  e_i = exp(y_(M-n+i)) - exp(cut), i = 0 ... n-1, ascending, fitted as mcr_pareto_khat fits a tail (rules 1-6
 *     above: the same text, scaling and summation order): khat, the regularised (k n + 5) / (n + 10) -- NaN (a constant
 *     tail) becoming +inf -- and sigma = -k / theta / 2^s from the UNregularised k of rule 5, theta of rule 4 and the scale
 *     of rule 2 (loo::gpdfit and ArviZ's _gpdfit do the same).  Unless khat is finite and sigma > 0 nothing is smoothed.
 *  4. Smoothing.  For tail index i let [s, e) be the maximal run of equal e_j that contains it, and p_i = (s + e) / (2 n):
 *     (i + 0.5) / n, ArviZ's, for a value that is alone.  q_i = sigma * expm1(-khat * log1p(-p_i)) / khat, or
 *     -sigma * log1p(-p_i) when |khat| < DBL_EPSILON.  The smoothed value is min(log(q_i + exp(cut)), 0).
 *     The run rule is the one deliberate departure from ArviZ and loo: they give tied ratios different weights
 *     according to argsort's order among them.  This library's sorts keep no order among equal keys, and a draw's weight
 *     must be a function of its value alone.
 *  5. Normalisation.  lw_(i) is the smoothed value of a tail index, else y_(i).  log_norm = m + log(sum_i exp(lw_(i) - m)),
 *     m = max_i lw_(i) (every log-sum-exp here: the maximum first, then the sum).  The log weight of a draw is
 *     lw - log_norm.
 *  6. Outputs per column: khat; ndraws_tail, the n actually used, an int64; with negate = 1 also
 *         lppd = logsumexp_i(-x_(i)) - log M,   elpd = logsumexp_i(lw_(i) - x_(i)) - log_norm,   p_loo = lppd - elpd
 *     (NaN with negate = 0); and, where log_weights is given, the P x M log weights in TIME order: element
 *     (p, c * N + n), contiguous in n.
 *  7. Summation order.  Every sum and every maximum over the M sorted values is 256 partial results, partial s taking the
 *     terms s, s + 256, ... in index order; each 64 consecutive partials are joined by the tree 32, 16, ... 1 and the four
 *     results r_0 ... r_3 as (r_0 + r_2) + (r_1 + r_3).  The order is a function of M alone and runs over the sorted
 *     values: it needs no positions and does not depend on the order among ties.  A column's outputs therefore have the
 *     same bits alone or anywhere in a batch, on the host or the device entry, in either layout or a strided view, under
 *     any workspace limit, for f32 against the widened f64, with or without log_weights, and for negate = 1 on v against
 *     negate = 0 on -v.
 * draws: host tensor addressed like mcr_summarize's.  r_eff, ndraws_tail: P entries each, or NULL.  out: P entries per
 * array, NULL skipped; log_weights is a HOST pointer in mcr_psis and a pointer into THIS ctx's device memory in
 * mcr_psis_dev (where every other array of out, r_eff and ndraws_tail stay on the host).
 * Limits: any C, C * N < 2^31 - 1.  MCR_EINVAL (message names the cause): a negative dimension, negate other than 0 / 1,
 * a ndraws_tail entry < 1, an r_eff entry that is not finite and > 0, summaries in flight, negative strides.
 * MCR_ENONFINITE: NaN / Inf values -- a log ratio of -inf (a weight of exactly zero) is refused like any other.  M == 0
 * gives NaN (ndraws_tail 0), P == 0 writes nothing.  The context stays usable after every error.  Synchronous.  ONE
 * workgroup handles a column (a tail beyond MCR_PARETO_LDS_TAIL is fitted from global memory): beyond ~10^5 draws a
 * column takes milliseconds.  k_psis_weights runs only where log_weights is given. */
typedef struct mcr_psis_out {
    double* khat; int64_t* ndraws_tail; double *lppd, *elpd, *p_loo;   /* P entries each, NULL skipped */
    double* log_weights;                                               /* [P][M], time order; NULL: not computed */
} mcr_psis_out;
int mcr_psis(mcr_ctx* ctx, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c, int64_t stride_n,
             int64_t stride_p, int negate, const double* r_eff /* P entries or NULL */,
             const int64_t* ndraws_tail /* P entries or NULL */, mcr_psis_out* out);
/* The same on draws in this ctx's device memory; out->log_weights is a device pointer too. */
int mcr_psis_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                 int64_t stride_n, int64_t stride_p, int negate, const double* r_eff, const int64_t* ndraws_tail,
                 mcr_psis_out* out);
/* Columns per workspace chunk of such a call under the current workspace limit (0 for an empty shape); host_weights: the
 * host entry with log_weights, whose chunk holds its weights too.  MCR_ENOMEM when the limit does not fit one column. */
int mcr_psis_plan(mcr_ctx* ctx, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c, int64_t stride_n,
                  int64_t stride_p, int host_weights, int64_t* params_per_chunk);
int64_t mcr_psis_tail_length(int64_t M, double r_eff);                   /* host only */
/* One column on the host (host only, no ctx, no device): M values in ANY order (sorted here), ndraws_tail 0 = the
 * default; NULL outputs are skipped; log_weights takes M entries in the order of `values`.  It runs the device's text in
 * the device's summation order, but with the host's libm, so the results equal the device's to rounding, not in bits.
 * MCR_EINVAL: M < 0 or >= 2^31 - 1, a NULL array, negate, ndraws_tail < 0, r_eff as above.  MCR_ENONFINITE: NaN / Inf. */
int mcr_psis_host(const double* values, int64_t M, int negate, double r_eff, int64_t ndraws_tail /* 0 = default */,
                  double* khat, int64_t* n_tail, double* lppd, double* elpd, double* p_loo, double* log_weights);
/* Highest-density intervals (HDI): the shortest interval that holds a given share of a parameter's draws (ArviZ's
 * unimodal hdi, the hdi_3% / hdi_97% columns of its summary; hdi of bayestestR).  ABSENT from the reference.  For a skewed
 * or bounded parameter it differs from the equal-tailed interval of the same share by a large part of its width.
 * For one parameter, let x_(0) <= ... <= x_(M-1) be its M pooled draws in ascending order.  The chains are pooled and
 * their structure plays no part.  Everything is IEEE double.  For each requested probability prob:
 *     inc = (int64) floor(prob * (double)M)        one rounded product, computed on the host
 *     W   = M - inc                                the number of windows
 *     w_i = x_(i + inc) - x_(i),  i = 0 ... W-1
 *     i*  = the smallest i with w_i = min_j w_j    (numpy.argmin: the first minimum)
 *     lo = x_(i*),  hi = x_(i* + inc),  index = i*
 * that is numpy.argmin(s[inc:] - s[:M - inc]) on s = numpy.sort(x).  The interval holds inc + 1 draws.  If W < 1 -- only
 * when the product rounds up to M -- lo = hi = NaN and index = -1.  A width that overflows to +inf is an ordinary value
 * of the comparison.
 * One answer.  The minimum over (w_i, i) in lexicographic order does not depend on the order of evaluation: a
 * parameter's outputs have the same bits alone or in a batch, at any place in the batch, under any workspace limit, in
 * either layout, on the host entry or the device entry, and for any split of the window range.  lo and hi are keys of
 * the sort: where the draws hold both -0.0 and +0.0 the sign of a zero endpoint is the sort's and is not specified.
 * f32 draws are widened first by the ingest pass; the answer is that of the f64 call on the widened tensor.
 * draws: host tensor addressed like mcr_summarize's.  probs: nprob probabilities, each finite with 0 < prob < 1, in any
 * order, repeats allowed.  out: [P][nprob] row-major arrays, NULL skipped.
 * Limits: any C, C * N < 2^31 - 1.  MCR_EINVAL (message names the cause): a negative dimension, nprob < 1 or >
 * MCR_HDI_MAX_PROBS, a probability outside (0, 1) or NaN, summaries in flight, negative strides.  MCR_ENONFINITE: NaN /
 * Inf draws.  M == 0 gives NaN and -1, P == 0 writes nothing.  The context stays usable after every error.  Synchronous.
 * k_hdi_window gives MCR_HDI_SLICE windows of a (parameter, probability) to one workgroup; k_hdi_pick takes the least of
 * the slices' candidates. */
typedef struct mcr_hdi_out { double *lo, *hi; int64_t* index; } mcr_hdi_out;   /* [P][nprob] each, NULL skipped */
int mcr_hdi(mcr_ctx* ctx, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c, int64_t stride_n,
            int64_t stride_p, const double* probs, int nprob, mcr_hdi_out* out);
/* The same on draws in this ctx's device memory; probs and out stay on the host. */
int mcr_hdi_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                int64_t stride_n, int64_t stride_p, const double* probs, int nprob, mcr_hdi_out* out);
/* Parameters per workspace chunk of such a call with nprob probabilities under the current workspace limit (0 for an
 * empty shape).  MCR_ENOMEM when the limit does not fit one parameter. */
int mcr_hdi_plan(mcr_ctx* ctx, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c, int64_t stride_n,
                 int64_t stride_p, int nprob, int64_t* params_per_chunk);
/* The same intervals of an ascending host array (host only, no ctx, no device): lo, hi, index take nprob entries, NULL
 * skipped.  The comparison of two windows is the device's text.  MCR_EINVAL: M < 0, a NULL array, nprob or a probability
 * as above.  Non-finite entries are not looked for. */
int mcr_hdi_sorted_host(const double* sorted, int64_t M, const double* probs, int nprob, double* lo, double* hi,
                        int64_t* index);
#define MCR_HDI_MAX_PROBS 16          /* probabilities of a mcr_hdi call */
#define MCR_HDI_SLICE 16384           /* windows k_hdi_window gives one workgroup */
/* Importance-weighted summaries: the mean, sd, standard error of the mean and quantiles of every parameter under ONE
 * weight per pooled draw, shared by all parameters (posterior::weight_draws + summarise_draws, loo::E_loo,
 * numpy.quantile(weights=)).  ABSENT from the reference.  It is what the log weights of mcr_psis are for: draws from an
 * approximation, reweighted towards the target.
 * Weights.  v[m], m = c * N + n, M = C * N entries.  Without MCR_W_LOG: w_m = v_m, every v_m finite and >= 0.  With it:
 * w_m = exp(v_m - max v), every v_m finite or -inf (-inf: the weight 0); NaN and +inf are refused.  A vector without a
 * positive weight is refused, and so is one whose S1 or S2 overflows.
 * Totals, once per call:   S1 = sum w     S2 = sum w^2     ess = S1^2 / S2   (Kish's effective sample size)
 * Per parameter, over its draws x_m in TIME order, in two passes:
 *     mean    = (sum w_m x_m) / S1
 *     d_m     = x_m - mean,  a_m = w_m d_m
 *     sd      = sqrt((sum a_m d_m) / S1)                 the population form, like mcr_summarize's std
 *     mean_se = sqrt(sum a_m a_m) / S1                   the standard error of a self-normalised importance-sampling mean
 * Per parameter and probability q, over the ascending order x_(0) <= ... <= x_(M-1) with u_j the weight of the draw
 * that stands at j:
 *     cum_j = the prefix sum of u up to and including j,    t = q * cum_(M-1)   (one rounded product)
 *     j*    = the first j with cum_j >= t and cum_j > 0,    quantile = x_(j*)
 * that is numpy.quantile(x, q, weights=w, method="inverted_cdf"), the only numpy method that takes weights; the clause
 * cum_j > 0 makes q = 0 skip leading zero weights.  Among tied draws every index gives the same value, and the value is
 * what is returned.  This is NOT the linear-interpolation quantile of mcr_summarize: with equal weights it is numpy's
 * unweighted inverted_cdf and differs from q5 / q50 / q95 by at most one spacing of the order statistics.
 * ONE association for every sum here -- S1, S2, the three moment sums, cum.  The indices are cut into blocks of
 * MCR_WEIGHTED_BLOCK consecutive ones.  A block's terms (+0 past the end) are the leaves of the balanced binary tree over
 * adjacent indices: node(0, i) = term i, node(L, i) = node(L-1, 2 i) + node(L-1, 2 i + 1); the block's sum is the root.
 * The blocks are added in ascending order from +0.  The in-block prefix of c leaves is the root of the same tree with
 * the leaves from c on replaced by +0 -- the tree's aligned nodes named by the binary digits of c, added from the
 * smallest to the largest; the root itself for a whole block, so that a block's sum is its last in-block prefix -- and
 * cum_j = (the sum of the blocks in front) + (the in-block prefix).  Every sum is monotone in its operands, so cum never
 * falls and stays where the weights are zero: the first block whose running sum satisfies the two conditions, then the
 * first j in that block, is the first j of all.  Every product is rounded before it is added.  A parameter's outputs therefore have the same bits alone
 * or at any place in a batch, under any workspace limit, for either position width of the sort, from the host or the
 * device entry, in either layout or a strided view, and for f32 draws against the widened f64 (the ingest pass widens
 * first).  mcr_weighted_host reproduces them bit for bit for linear weights; log weights go through the device's exp,
 * which need not be libm's, so out->weights returns the w_m the call formed, and a second call with those as linear
 * weights gives the same bits.
 * draws: host tensor addressed like mcr_summarize's.  weights: M entries, a HOST pointer in mcr_weighted_summary and a
 * pointer into THIS ctx's device memory in mcr_weighted_summary_dev; out->weights likewise.  probs: nq probabilities in
 * [0, 1], 0 <= nq <= MCR_WEIGHTED_MAX_Q; nq = 0 computes no quantile (the sort still runs: it counts the non-finite draws).
 * Every other array of out stays on the host, NULL skipped.
 * Limits: any C, C * N < 2^31 - 1.  MCR_EINVAL (message names the cause, the same on both entries): a negative dimension,
 * unknown flag bits, nq out of range, a probability outside [0, 1] or NaN, a weight vector refused as above (checked on
 * the device before any output is written: one small copy of the totals), summaries in flight, negative strides.
 * MCR_ENONFINITE: NaN / Inf draws.  M == 0 gives NaN, ess included, without a launch; P == 0 writes nothing.  The context
 * stays usable after every error.  Synchronous.
 * Kernels (mcr_weighted.hpp): k_weight_prepare once per call, k_weighted_moments and k_weighted_combine twice per chunk,
 * k_wq_blocks and k_wq_pick where nq > 0.  OUT OF SCOPE: weighted KS / W1 / HDI / k-hat, resampling, a weight vector
 * per parameter, ragged mcr_summarize_chains input. */
#define MCR_WEIGHTED_BLOCK 1024       /* consecutive indices of one summation tree (part of the summation order) */
#define MCR_WEIGHTED_MAX_Q 16         /* probabilities of a call */
#define MCR_W_LOG 1                   /* flags: the weight vector holds log weights */
typedef struct mcr_weighted_out {
    double *mean, *sd, *mean_se;      /* P entries each, NULL skipped */
    double *quantiles;                /* [P][nq] */
    double *ess, *weight_sum;         /* one entry each: S1^2 / S2 and S1 */
    double *weights;                  /* [M], the w_m as formed; NULL: not returned */
} mcr_weighted_out;
int mcr_weighted_summary(mcr_ctx* ctx, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                         int64_t stride_n, int64_t stride_p, const double* weights, int flags, const double* probs, int nq,
                         mcr_weighted_out* out);
/* The same on draws in this ctx's device memory; weights_dev and out->weights are device pointers too. */
int mcr_weighted_summary_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P,
                             int64_t stride_c, int64_t stride_n, int64_t stride_p, const double* weights_dev, int flags,
                             const double* probs, int nq, mcr_weighted_out* out);
/* Parameters per workspace chunk of such a call with nq probabilities under the current workspace limit (0 for an empty
 * shape).  MCR_ENOMEM when the limit does not fit one parameter. */
int mcr_weighted_plan(mcr_ctx* ctx, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c, int64_t stride_n,
                      int64_t stride_p, int nq, int64_t* params_per_chunk);
/* One parameter on the host (host only, no ctx, no device): M draws x in time order and their M weights; std::sort on
 * (value, position), then the association above.  quantiles takes nq entries, weights M; NULL outputs are skipped.
 * MCR_EINVAL: M < 0 or >= 2^31 - 1, a NULL array, flags, nq or a probability as above, a refused weight vector.
 * MCR_ENONFINITE: NaN / Inf draws.  M == 0 gives NaN. */
int mcr_weighted_host(const double* x, const double* weights_in, int64_t M, int flags, const double* probs, int nq,
                      double* mean, double* sd, double* mean_se, double* quantiles, double* ess, double* weight_sum,
                      double* weights);
/* Simulation-based calibration (SBC; Talts et al. 2018, Schad et al. 2021, the SBC R package): where the true value of
 * a parameter stands among the posterior draws of a fit to data simulated from it, for S simulations at once.  ABSENT
 * from the reference.  It checks a sampler when no reference posterior exists: over many simulations the rank is uniform
 * exactly when the sampler is right.
 * Input: S simulations, each a (C, N, P) draw tensor addressed like mcr_summarize's, simulation s starting stride_s
 * elements behind simulation s - 1; f64 or f32 (f32 draws are widened first by the ingest pass: the answer is that of the
 * f64 call on the widened tensor).  truth[S][P]: the values the data were simulated from, HOST doubles in both entries.
 * Thinning is no argument: a thinned tensor is the same tensor with a larger stride_n and a smaller N.
 * For every (s, p), with x_0 ... x_{L-1} the L = C * N draws of that simulation and parameter, chain after chain, and
 * t = truth[s][p], everything in IEEE double:
 *     n_less  = #{i : x_i < t}        n_equal = #{i : x_i == t}        (-0.0 == +0.0; a NaN draw is in neither)
 *     mean    = (sum x_i) / L
 *     sd      = sqrt((sum (x_i - mean)^2) / L)      the population form, like mcr_summarize's std, in two passes; the
 *                                                   difference and its square are rounded one after the other
 * The rank of t is n_less plus, by the method's convention, a uniform draw from 0 .. n_equal (the caller's: see
 * mcmc_ref_hip.sbc).  ONE association for both sums, that of the weighted summaries above: the indices i are cut into
 * blocks of MCR_WEIGHTED_BLOCK consecutive ones; a block's terms (+0 past the end) are the leaves of the balanced binary
 * tree over adjacent indices, node(0, i) = term i, node(k, i) = node(k-1, 2 i) + node(k-1, 2 i + 1), the block's sum is the
 * root; the blocks are added in ascending order from +0.  It is defined on the indices of the row, not on addresses, so
 * an (s, p)'s outputs have the same bits alone or at any place in a batch, under any workspace limit, for aligned or
 * misaligned rows, in any layout or strided view, from the host or the device entry, and mcr_sbc_ranks_host reproduces
 * them bit for bit.
 * out: HOST arrays of [S][P] entries each, NULL skipped.
 * Limits: S * P < 2^31, C * N < 2^31 - 1.  MCR_EINVAL (message names the cause; nothing has been uploaded or written): a
 * negative dimension, S * P >= 2^31, C * N >= 2^31 - 1, a NULL or non-finite entry of truth, negative strides, summaries in
 * flight.  MCR_ENONFINITE: NaN / Inf draws, with their number in the message; the outputs are written all the same.
 * L == 0 gives the counts 0 and NaN mean and sd without a launch; S == 0 or P == 0 writes nothing.  The context stays usable
 * after every error.  Synchronous; the result table comes back in one copy.
 * Kernels (mcr_sbc.hpp): k_sbc_ranks, a wave per (s, p).  When the draws are f64 and every simulation is [P][C][N]
 * contiguous with stride_s = P * C * N, it reads the caller's memory: one launch, no copy.  Otherwise the simulations are
 * cut into workspace chunks (mcr_sbc_plan), one k_ingest (its grid's z runs over the chunk's simulations) and one k_sbc_ranks
 * per chunk, all on the stream without a host synchronisation in between. */
typedef struct mcr_sbc_out {
    int64_t *n_less, *n_equal;        /* [S][P] each, NULL skipped */
    double  *mean, *sd;
} mcr_sbc_out;
int mcr_sbc_ranks(mcr_ctx* ctx, const void* draws, int dtype, int64_t S, int64_t C, int64_t N, int64_t P, int64_t stride_s,
                  int64_t stride_c, int64_t stride_n, int64_t stride_p, const double* truth, mcr_sbc_out* out);
/* The same on draws in this ctx's device memory; truth and out stay on the host. */
int mcr_sbc_ranks_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t S, int64_t C, int64_t N, int64_t P,
                      int64_t stride_s, int64_t stride_c, int64_t stride_n, int64_t stride_p, const double* truth,
                      mcr_sbc_out* out);
/* Simulations per workspace chunk of such a call under the current workspace limit: S when the call reads the caller's
 * memory, 0 for an empty shape.  MCR_ENOMEM when the limit does not fit one simulation's ingest copy; MCR_EINVAL for a
 * shape the call would refuse (S < 0, S * P >= 2^31). */
int mcr_sbc_plan(mcr_ctx* ctx, int dtype, int64_t S, int64_t C, int64_t N, int64_t P, int64_t stride_s, int64_t stride_c,
                 int64_t stride_n, int64_t stride_p, int64_t* sims_per_chunk);
/* The definition on the host (host only, no ctx, no device): x is [S][P][L] contiguous doubles.  MCR_EINVAL: a NULL array,
 * a negative size, S * P >= 2^31, L >= 2^31 - 1, a non-finite entry of truth (nothing is written).  MCR_ENONFINITE: NaN / Inf
 * draws (the outputs are written).  L == 0 gives 0 and NaN. */
int mcr_sbc_ranks_host(const double* x, int64_t S, int64_t P, int64_t L, const double* truth, mcr_sbc_out* out);
/* The uniformity of the ranks (host only, no ctx).  ranks[S][P], each in 0 .. L; B bins, 2 <= B <= L + 1; S >= 1.
 *     bin(r)      = floor(r * B / (L + 1))
 *     expected[b] = S * #{r in 0 .. L : bin(r) == b} / (L + 1)      exact also when B does not divide L + 1
 *     counts[p][b] = #{s : bin(ranks[s][p]) == b}
 *     chi2[p]     = sum_b (counts[p][b] - expected[b])^2 / expected[b]   in bin order, B - 1 degrees of freedom
 *     pvalue[p]   = mcr_chi2_sf(chi2[p], B - 1)
 *     ecdf_dev[p] = max over r in 0 .. L of |#{s : ranks[s][p] <= r} / S - (r + 1) / (L + 1)|, formed as the integer maximum of
 *                   |#{...} (L + 1) - (r + 1) S| and divided once by S (L + 1), as the two-sample KS is
 * Outputs: counts [P][B], expected [B], chi2, pvalue, ecdf_dev [P]; NULL skipped.  MCR_EINVAL: a NULL ranks, S < 1, P < 0,
 * L < 0, B outside 2 .. L + 1, a rank outside 0 .. L (outputs of earlier parameters have been written). */
int mcr_sbc_uniformity(const int64_t* ranks, int64_t S, int64_t P, int64_t L, int64_t B, int64_t* counts, double* expected,
                       double* chi2, double* pvalue, double* ecdf_dev);
/* The survival function of the chi-square distribution with dof > 0 degrees of freedom at x >= 0: the regularised upper
 * incomplete gamma function Q(dof / 2, x / 2), by the series of P below x / 2 < dof / 2 + 1 and by the continued fraction
 * of Q above.  NaN for dof <= 0, x < 0 or NaN. */
double mcr_chi2_sf(double x, double dof);
/* Autocorrelation functions and autocorrelation times: the autocorrelation of the RAW draws of every (parameter, chain)
 * up to a maximum lag, the within-chain pooled autocorrelation per parameter, and the integrated autocorrelation time
 * with Sokal's automatic window (posterior::autocorrelation, ArviZ's autocorr / plot_autocorr, emcee's integrated_time).
 * ABSENT from the reference, whose only use of the time order is inside its ESS.  The ESS kernels here are not involved:
 * they work on rank-normalised z, sum over chains, divide by n - lag and stop at the truncation lag.
 * For one parameter and one chain x_0 ... x_{N-1}, maximum lag L, everything in IEEE double:
 *     m     = (sum_i x_i) / N
 *     d_i   = x_i - m
 *     S_l   = sum_{i=0}^{N-l-1} d_i * d_{i+l}            l = 0 ... L
 *     gamma_l = S_l / N                                  (flag MCR_ACF_UNBIASED: S_l / (N - l))
 *     rho_l = gamma_l / gamma_0                          gamma_0 == 0 (a constant chain, or N == 1): every rho_l = NaN
 * The biased form is the FFT-based arviz.autocorr / posterior::autocovariance, computed by direct sums; the unbiased one
 * is the per-chain cov / (n - lag) of the reference's _autocorr (diagnostics.py:186-191).
 * Integrated autocorrelation time, with the caller's window constant window_c (emcee's c; 5 is the usual value):
 *     tau_W  = 2 (rho_0 + ... + rho_W) - 1               W = 0 ... L, a running sum left to right
 *     window = the smallest W with W >= window_c * tau_W, or -1 when no W <= L satisfies it
 *     tau    = tau_window, or tau_L when window == -1    (then a lower bound: the ACF has not decayed within L)
 * NaN rho gives tau = NaN and window = -1.  This differs from emcee in one place: emcee returns the last index when no
 * window is found; here that case is -1, so that it cannot be mistaken for a found window.
 * Pooled over the C chains of a parameter (within-chain correlation: the chains are NOT concatenated):
 *     gamma-bar_l = (sum_c gamma_{l,c}) / C in chain order c = 0 ... C-1,  rho-bar_l = gamma-bar_l / gamma-bar_0 (NaN
 *     when that is 0); tau_pooled and window_pooled follow the same rule on rho-bar.
 * One order of summation, a function of (N, l) and C alone:
 *     m      lane j of 64 adds x_j, x_{j+64}, ... in index order; the 64 sums meet pairwise, v_j += v_{j+o} for j < o,
 *            o = 32, 16, ... 1; m = v_0 / N.
 *     S_l    the draws are cut into blocks of MCR_ACF_BLOCK consecutive i.  Block b: acc = +0, then
 *            acc = fma(d_i, d_{i+l}, acc) for i = b B ... min(b B + B, N - l) - 1 ascending (an explicit fma on the device
 *            and on the host).  S_l = ((0 + acc_0) + acc_1) + ... over all ceil(N / B) blocks in block order.
 *     pooled, tau: left to right from +0, as written above.
 * A (parameter, chain)'s outputs therefore have the same bits alone or at any place in a batch, under any workspace
 * limit, in either layout, for aligned or misaligned rows, from the host or the device entry.  f32 draws are widened
 * first by the ingest pass; the answer is that of the f64 call on the widened tensor.
 * draws: host tensor addressed like mcr_summarize's.  out stays on the host; NULL members are skipped.  Synchronous.
 * Limits: any C, C * N < 2^31 - 1, max_lag <= MCR_ACF_MAX_LAG: the products are direct, O(N * max_lag).  Larger lags, the
 * full ACF by the FFT tier, and the ACF of the rank-normalised z codes are OUT OF SCOPE.
 * MCR_EINVAL (message names the cause): a negative dimension, max_lag < 0, max_lag > N - 1 (when N >= 1), max_lag >
 * MCR_ACF_MAX_LAG, unknown flag bits, window_c not finite or <= 0, negative strides, summaries in flight.
 * MCR_ENONFINITE: NaN / Inf draws.  C * N == 0 fills NaN and -1, P == 0 writes nothing.  The context stays usable after
 * every error.  The workspace is chunked over parameters (mcr_autocorr_plan reports the chunk).
 * Kernels (mcr_acf.hpp): k_acf_mean, k_acf_products (the dense lag products, LDS-staged, 4 lags x 4 draws per thread and
 * step), k_acf_finish (per chain), k_acf_pool (per parameter). */
#define MCR_ACF_MAX_LAG   4096        /* the largest max_lag of a call */
#define MCR_ACF_BLOCK     512         /* consecutive draws of one fma chain (part of the summation order) */
#define MCR_ACF_UNBIASED  1           /* flags */
typedef struct mcr_acf_out {          /* NULL members are skipped; L = max_lag */
    double  *acf;                     /* [P][C][L+1] */
    double  *var;                     /* [P][C]   gamma_0 */
    double  *tau;                     /* [P][C] */
    int64_t *window;                  /* [P][C] */
    double  *acf_pooled;              /* [P][L+1] */
    double  *tau_pooled;              /* [P] */
    int64_t *window_pooled;           /* [P] */
} mcr_acf_out;
int mcr_autocorr(mcr_ctx* ctx, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                 int64_t stride_n, int64_t stride_p, int64_t max_lag, int flags, double window_c, mcr_acf_out* out);
/* The same on draws in this ctx's device memory; out stays on the host. */
int mcr_autocorr_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                     int64_t stride_n, int64_t stride_p, int64_t max_lag, int flags, double window_c, mcr_acf_out* out);
/* Parameters per workspace chunk of such a call under the current workspace limit (0 for an empty shape).  MCR_ENOMEM
 * when the limit does not fit one parameter; MCR_EINVAL for a max_lag the call would refuse. */
int mcr_autocorr_plan(mcr_ctx* ctx, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c, int64_t stride_n,
                      int64_t stride_p, int64_t max_lag, int64_t* params_per_chunk);
/* The same quantities of one parameter's chains in host memory, chains[C][N] row-major (host only, no ctx, no device);
 * out as above with P = 1.  It runs the device's text in the device's summation order and uses only +, -, *, / and fma:
 * its results equal the device's IN BITS (unlike mcr_pareto_fit_host, which goes through libm).  MCR_EINVAL as above
 * (without a message), MCR_ENONFINITE for NaN / Inf draws. */
int mcr_autocorr_host(const double* chains, int64_t C, int64_t N, int64_t max_lag, int flags, double window_c,
                      mcr_acf_out* out);
/* Population covariance matrix (ddof = 0, like compare.py:63) of P parameters over M pooled draws,
 * draws[P][M] host row-major -> cov[P][P].  The one dense contraction of the path: fp64 MFMA
 * (v_mfma_f64_16x16x4f64; LDS-staged 64 x 64 tiles, upper triangle, split over the draw axis).
 * numpy.cov(x, ddof=0).  SURVEY.md row X3. */
int mcr_covariance(mcr_ctx* ctx, const double* draws, int64_t M, int64_t P, double* cov);
/* The same on device-resident buffers of this ctx (draws_dev [P][M], cov_dev [P][P]); P <= 8192. */
int mcr_covariance_dev(mcr_ctx* ctx, const double* draws_dev, int64_t M, int64_t P, double* cov_dev);

/* ---- measurement ------------------------------------------------------------------- */
/* When on, every kernel launch is bracketed by HIP events on the ctx stream. */
int mcr_profile_enable(mcr_ctx* ctx, int on);
int mcr_profile_reset(mcr_ctx* ctx);
/* Synchronises, resolves the events and fills up to `max` entries; *n = entries available. */
int mcr_profile_get(mcr_ctx* ctx, mcr_kernel_time* out, int max, int* n);
/* Fills a device buffer with the synthetic stress tensor of SURVEY.md 8(d) C4 (iid
 * N(p, sigma_p), counter-based, layout [P][C][N]) without touching the host. */
int mcr_fill_synthetic(mcr_ctx* ctx, void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P,
                       uint64_t seed);

/* What this device's HBM delivers, measured: best of `iters` passes of a read-only streaming kernel over `bytes`
 * (read_gbps) and of a device-to-device copy (copy_gbps = bytes read + written per second); either may be NULL.
 * bench.py prints it as `peak_measured` beside the 8 TB/s specification peak. */
int mcr_hbm_probe(mcr_ctx* ctx, size_t bytes, int iters, double* read_gbps, double* copy_gbps);
/* The same for the parameter block [p0, p0 + P) of that tensor: draws_dev receives P * C * N elements that equal the
 * corresponding slice of the whole tensor (a rank of a P-split model generates only its own columns). */
int mcr_fill_synthetic_at(mcr_ctx* ctx, void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t p0,
                          uint64_t seed);

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU: one process per GPU, models / parameter blocks sharded with no data-path
 * exchange, and ONE collective at the end -- an RCCL all-gather of fixed-size per-parameter summary
 * records over xGMI.  The reference has no counterpart (it is single-process); this replaces the loop
 * over models of generate.generate_reference_corpus (src/mcmc_ref/generate.py:77-96) being run on N
 * devices.  librccl is loaded on first use (dlopen); failures return MCR_ECOMM.
 * Ranks must agree on a 128-byte id: rank 0 calls mcr_comm_unique_id and hands the bytes to the others
 * by any means (mcmc_ref_hip.shard uses a file keyed on MASTER_ADDR / MASTER_PORT), then every rank
 * calls mcr_comm_init (collective).  All buffers are host pointers; calls are synchronous.
 * EVERY collective has a deadline: ncclCommInitRank runs on a helper thread the caller watches, and the
 * waits for all-gather / all-reduce / barrier poll the communicator's stream and ncclCommGetAsyncError
 * against MCR_COMM_TIMEOUT_S (default 300).  A peer that never arrives or dies -- the reference's loop
 * simply continues past a failed recipe, src/mcmc_ref/generate.py:77-96 -- ends the call with MCR_ECOMM
 * naming the call and the rank after that time instead of blocking for ever; the communicator is
 * aborted (ncclCommAbort) and every later call on it fails at once.  A collective that fails or
 * times out leaves the caller's output buffer unwritten: the result is copied out only after the wait.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mcr_comm mcr_comm;
#define MCR_COMM_ID_BYTES 128
#define MCR_RECORD_DOUBLES 16 /* one per-parameter summary record = 128 bytes */
int mcr_comm_unique_id(void* id, size_t len);
int mcr_comm_init(mcr_ctx* ctx, const void* id, int world, int rank, mcr_comm** out);
void mcr_comm_free(mcr_comm* comm);
int mcr_comm_world(const mcr_comm* comm);
int mcr_comm_rank(const mcr_comm* comm);
int mcr_comm_has_deadline(const mcr_comm* comm); /* 1 for any communicator: every wait is bounded */
/* ncclAllGather: every rank sends `count` doubles and receives world * count doubles in rank order. */
int mcr_comm_all_gather(mcr_comm* comm, const double* send, int64_t count, double* recv);
/* ncclAllReduce in place over n doubles; op: 0 = sum, 1 = max, 2 = min (max-over-ranks clock, all-valid flag). */
int mcr_comm_all_reduce(mcr_comm* comm, double* vals, int64_t n, int op);
/* Drains this context's lanes, then synchronises the ranks. */
int mcr_comm_barrier(mcr_comm* comm);

/* ------------------------------------------------------------------------------------------------
 * Parquet ingest: draws file -> device tensor.
 * Replaces pq.read_table / pq.ParquetFile + to_numpy on the way into the statistics
 * (src/mcmc_ref/store.py:79-95 open_draws, src/mcmc_ref/convert.py:61-65, backends_numpy.py:35):
 * footer and page headers are parsed on the host, page payloads are Snappy-decompressed and
 * PLAIN / RLE_DICTIONARY decoded by HIP kernels straight into device memory.
 * Supported: flat schemas; INT32 / INT64 / FLOAT / DOUBLE columns, REQUIRED or OPTIONAL without
 * nulls; UNCOMPRESSED / SNAPPY; data pages v1 and v2; any number of row groups and pages.
 * Anything else fails with MCR_EINVAL and a message naming the feature.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mcr_parquet mcr_parquet;

#define MCR_PQ_F64 0 /* out_dev is double[num_rows]  (ints and floats are converted to double) */
#define MCR_PQ_I64 1 /* out_dev is int64_t[num_rows] (INT32 / INT64 columns only: chain, draw) */

/* Physical types as in parquet.thrift (mcr_parquet_column_type). */
#define MCR_PQ_BOOLEAN 0
#define MCR_PQ_INT32 1
#define MCR_PQ_INT64 2
#define MCR_PQ_INT96 3
#define MCR_PQ_FLOAT 4
#define MCR_PQ_DOUBLE 5
#define MCR_PQ_BYTE_ARRAY 6
#define MCR_PQ_FIXED_LEN_BYTE_ARRAY 7

typedef struct {
    const mcr_parquet* file;
    int column;    /* index into the file's (flat) schema */
    int out_kind;  /* MCR_PQ_F64 or MCR_PQ_I64 */
    void* out_dev; /* device pointer, num_rows 8-byte elements, rows in file order */
} mcr_parquet_request;

/* Parses the metadata of a Parquet file image held in host memory.  `bytes` must stay valid and
 * unchanged until mcr_parquet_close (the image is not copied).  Needs no device: ctx may be NULL
 * (the message of a failure is then read with mcr_last_error(NULL)). */
int mcr_parquet_open(mcr_ctx* ctx, const void* bytes, size_t len, mcr_parquet** out);
void mcr_parquet_close(mcr_parquet* f);
int64_t mcr_parquet_num_rows(const mcr_parquet* f);
int mcr_parquet_num_columns(const mcr_parquet* f);
const char* mcr_parquet_column_name(const mcr_parquet* f, int column); /* NULL if out of range */
int mcr_parquet_column_type(const mcr_parquet* f, int column);         /* -1 if out of range */
/* Page table as parsed from the page headers (introspection / tests).  info[10] = {column, page
 * type, value encoding, codec, payload file offset, compressed size, uncompressed size, values,
 * first row, page index of the chunk's dictionary page or -1}. */
int mcr_parquet_num_pages(const mcr_parquet* f);
int mcr_parquet_page_info(const mcr_parquet* f, int page, int64_t* info);

/* Decodes the requested columns (of one or many files) with ONE upload + two kernel launches;
 * synchronous on return.  Requests may mix files, columns and output kinds. */
int mcr_parquet_decode(mcr_ctx* ctx, const mcr_parquet_request* reqs, int n_reqs);

/* dst[p][k] = src[p][order[k]]: puts rows that are not stored in (chain, draw) order into the
 * order `_chains_from_table` produces (src/mcmc_ref/convert.py:150-161).  order is a host array. */
int mcr_gather_rows_dev(mcr_ctx* ctx, const double* src_dev, int64_t P, int64_t M, const int64_t* order,
                        double* dst_dev);

/* The row order of `_chains_from_table` (src/mcmc_ref/convert.py:150-161) from the decoded id columns, on the device:
 * order = np.lexsort((draw, chain)) -- chain id ascending, draw ascending within a chain, rows with equal (chain, draw)
 * in file order -- by a stable LSD radix sort of the packed key (chain - min chain) << bits(draw range) | (draw - min
 * draw), one 8-bit pass per significant key byte.  chain_dev / draw_dev: int64 device columns of M rows (M < 2^31 - 1).
 * *in_order = 1: the rows are in that order already; no sort runs and order_dev is not written (it may be NULL).
 * Otherwise order_dev (device, M entries) receives the order.  chain_ids / counts (host, cap entries): the distinct chain
 * ids ascending and their row counts, *n_chains of them; more than cap distinct ids is MCR_EINVAL.  Ranges that do not
 * fit one 64-bit key: MCR_EFALLBACK.  Synchronous; uses the current lane's workspace, so no summary may be in flight.
 * MCR_LAYOUT_SPAN: rows per workgroup of a sort pass. */
#define MCR_LAYOUT_SPAN 2048
int mcr_chain_layout_dev(mcr_ctx* ctx, const int64_t* chain_dev, const int64_t* draw_dev, int64_t M, int64_t* order_dev,
                         int64_t* chain_ids, int64_t* counts, int cap, int* n_chains, int* in_order);
/* Step one of mcr_chain_layout_dev for MANY tables in one round trip (a corpus pass reads dozens of files, nearly all in
 * order): per table t, in_order[t], n_chains[t] (the number of maximal runs of equal chain id in file order) and --
 * meaningful when in_order[t] is 1 -- chain_ids / counts at [t * cap, t * cap + min(n_chains[t], cap)).  A table that is
 * not in order is then sorted by its own mcr_chain_layout_dev call; one with n_chains[t] > cap has only its first cap
 * chains reported.  Never sorts, never answers MCR_EFALLBACK. */
typedef struct mcr_id_columns {
    const int64_t* chain_dev;
    const int64_t* draw_dev;
    int64_t rows;
} mcr_id_columns;
int mcr_chain_layout_many_dev(mcr_ctx* ctx, const mcr_id_columns* tables, int n_tables, int64_t* chain_ids, int64_t* counts,
                              int cap, int* n_chains, int* in_order);
/* mcr_gather_rows_dev with the order in device memory (what mcr_chain_layout_dev wrote): dst[p][k] = src[p][order[k]].
 * An entry outside [0, M) is not read: MCR_EINVAL. */
int mcr_gather_rows_order_dev(mcr_ctx* ctx, const double* src_dev, int64_t P, int64_t M, const int64_t* order_dev,
                              double* dst_dev);

/* ------------------------------------------------------------------------------------------------
 * Parquet writing: device columns -> draws file image.
 * Replaces `pq.write_table(table, draws_path)` (src/mcmc_ref/convert.py:64): every data page is
 * formed (definition levels + PLAIN values), Snappy-compressed and measured (min / max) by one HIP
 * workgroup, the host writes page headers and the footer from the pages' sizes, and one kernel
 * packs everything into the file image that one copy brings to pinned host memory.
 * Written: a flat schema of OPTIONAL leaves without nulls, INT32 / INT64 / DOUBLE, data pages v1 of
 * MCR_PQW_PAGE_ROWS rows, PLAIN values, RLE levels, SNAPPY with copy offsets <= 65535, no
 * dictionary pages, row groups of row_group_rows rows, Statistics (null_count 0, min_value /
 * max_value; a zero minimum is -0.0 and a zero maximum +0.0; none for a chunk with a NaN),
 * created_by "mcmc-ref-hip version <major.minor.patch of MCR_VERSION>".  The same columns give the
 * same bytes.
 * A column is `rows` elements of a source: device memory through an element stride, or generated.
 * f64 -> DOUBLE keeps the bits; f64 -> INT64 / INT32 and i64 -> INT64 / INT32 are checked: a value
 * that is no integer or outside the type's range ends the call with MCR_EINVAL naming the column
 * and the first such row.  Also MCR_EINVAL: rows <= 0 or >= 2^31, an empty or repeated name, a
 * type other than the three, an integer source written as DOUBLE, stride < 1.
 * ---------------------------------------------------------------------------------------------- */
#define MCR_PQW_PAGE_ROWS 8192         /* rows per data page: 64 KiB of 8-byte values */
#define MCR_PQW_ROW_GROUP_ROWS 1048576 /* rows per row group when row_group_rows is 0 (pyarrow's default) */

#define MCR_PQW_F64 0 /* src_dev: double, element r at src_dev[r * stride] */
#define MCR_PQW_I64 1 /* src_dev: int64_t, same addressing */
#define MCR_PQW_SEQ 2 /* no memory: value(r) = (r / seq_div) % seq_mod.  chain of a rectangular model: div = N;
                         draw: mod = N; row number: div = 1, mod = INT64_MAX; zeros: mod = 1 */
typedef struct mcr_pq_column {
    const char* name;
    int type;     /* MCR_PQ_INT32, MCR_PQ_INT64 or MCR_PQ_DOUBLE */
    int src_kind; /* MCR_PQW_* */
    const void* src_dev;
    int64_t stride;
    int64_t seq_div, seq_mod;
} mcr_pq_column;
typedef struct mcr_pq_image mcr_pq_image;

/* Synchronous; uses the current lane's workspace, so no summary may be in flight (as mcr_chain_layout_dev).
 * *out owns the image (pinned host memory) until mcr_pq_image_free. */
int mcr_parquet_write_dev(mcr_ctx* ctx, const mcr_pq_column* cols, int n_cols, int64_t rows, int64_t row_group_rows,
                          mcr_pq_image** out);
/* The same file format from HOST columns (src_dev points to host memory), without a device: ctx may be NULL.  Page
 * headers, footer, levels and statistics come from the same code, the pages from a scalar restatement of the
 * compressor that shares the token emission; its sequential match finder sees every earlier element, so the bytes
 * may differ from the device's.  Both are valid files with equal contents. */
int mcr_parquet_write_host(mcr_ctx* ctx, const mcr_pq_column* cols, int n_cols, int64_t rows, int64_t row_group_rows,
                           mcr_pq_image** out);
const void* mcr_pq_image_data(const mcr_pq_image* image);
size_t mcr_pq_image_size(const mcr_pq_image* image);
int mcr_pq_image_pages(const mcr_pq_image* image); /* data pages of the file */
void mcr_pq_image_free(mcr_pq_image* image);

/* ------------------------------------------------------------------------------------------------
 * CSV writing: device columns -> text image.
 * Replaces `pyarrow.csv.write_csv(table, out)` of the reference's `draws` command
 * (src/mcmc_ref/cli.py:100-127), byte for byte, for float64 / int64 columns without nulls.
 * A double is nan, [-]inf, [-]0, or the shortest digits d1..dn that read back to it (the closest
 * such string), v = d1.d2..dn x 10^e: positional without exponent when -6 <= e <= 9 (0.000001,
 * 1500000000, 12345.678), d1[.d2..dn]e[+-]E otherwise (1e+10, 1.2e-7, 5e-324); never more than 25
 * bytes.  Integers are plain decimal.  Separator ',', '\n' after every row.
 * Columns are addressed as for mcr_parquet_write_dev; `type` says only integer (MCR_PQ_INT32 and
 * MCR_PQ_INT64 print alike, the full int64 range) or MCR_PQ_DOUBLE (printed from its 64 bits, never
 * through a float32).  An f64 source declared integer is checked: a value that is no integer ends
 * the call with MCR_EINVAL naming the column and the first such row.
 * `rows` is the row count of the source.  Without a row list the rows 0 .. rows - 1 are written;
 * with one, its n_index entries select and order them (repeats allowed, n_index may be 0: the header
 * alone).  MCR_EINVAL, with the reason in the message: rows < 0 or >= 2^31, n_index < 0 or >= 2^31,
 * n_cols < 1, stride < 1, an integer source declared DOUBLE, a list entry outside 0 .. rows - 1.
 * A table whose worst-case text (26 bytes per field) exceeds the workspace limit is written in row
 * ranges appended to the one image.
 * ---------------------------------------------------------------------------------------------- */
#define MCR_CSVW_TILE_FIELDS 2048 /* fields per k_csvw_format workgroup: whole rows when n_cols <= this, else a row is cut */
#define MCR_CSVW_FIELD_MAX 26     /* the longest field and its separator */
#define MCR_CSVW_HEADER_QUOTED 0  /* "name" with an inner quote doubled: pyarrow's default */
#define MCR_CSVW_HEADER_PLAIN 1   /* the names as they are (MCR_EINVAL for a name with a quote, comma, CR or LF) */
#define MCR_CSVW_HEADER_NONE 2
typedef struct mcr_text_image mcr_text_image;

/* Synchronous; uses the current lane's workspace, so no summary may be in flight.  index_dev: device memory.
 * *out owns the image (pinned host memory) until mcr_text_image_free. */
int mcr_csv_write_dev(mcr_ctx* ctx, const mcr_pq_column* cols, int n_cols, int64_t rows, const int64_t* index_dev,
                      int64_t n_index, int header, mcr_text_image** out);
/* The same from HOST columns and a host row list, without a device: ctx may be NULL.  The same formatter walks the
 * same tiles: the bytes are identical to the device's. */
int mcr_csv_write_host(mcr_ctx* ctx, const mcr_pq_column* cols, int n_cols, int64_t rows, const int64_t* index,
                       int64_t n_index, int header, mcr_text_image** out);
const void* mcr_text_image_data(const mcr_text_image* image);
size_t mcr_text_image_size(const mcr_text_image* image);
void mcr_text_image_free(mcr_text_image* image);
/* The grammar for one value (host, like mcr_parse_double): writes len <= 25 bytes, no terminator. */
int mcr_format_double(double v, char* out26, int* len);

/* Stable selection (the reference's `ds.field("chain").isin(chains)`, src/mcmc_ref/store.py:79-95): the indices of
 * the rows of chain_dev[0 .. M) whose value is in chains[0 .. n_chains) (host memory), in order, into
 * rows_dev[0 .. *n_selected) (device memory, room for M).  An empty list selects nothing; repeats are harmless.
 * Synchronous; uses the current lane's workspace. */
#define MCR_SELECT_BLOCK_ROWS 256 /* rows per k_select_rows workgroup */
int mcr_select_rows_dev(mcr_ctx* ctx, const int64_t* chain_dev, int64_t M, const int64_t* chains, int n_chains,
                        int64_t* rows_dev, int64_t* n_selected);

/* ------------------------------------------------------------------------------------------------
 * Many draws files -> statistics in ONE call (the per-model loop of reference.stats /
 * diagnostics_for_model, src/mcmc_ref/reference.py:30-104, over a list of
 * draws/<model>.draws.parquet files): mmap + footer parse on the host, one batched GPU decode, the
 * chain / draw bookkeeping of convert._chains_from_table, same-shape neighbours summarised as one
 * tensor, results in a host-side set.  Parameters = every numeric column except `chain` and `draw`,
 * in schema order.  Files whose rows are not in (chain, draw) order, or whose chains differ in
 * length while diagnostics are requested, end the call with MCR_ELAYOUT (use mcr_parquet_decode +
 * mcr_chain_layout_dev + mcr_gather_rows_order_dev + mcr_summarize_chains_dev for those).  diagnostics = 0: Backend.stats only
 * (pooled mean / std / quantiles; any chain structure).
 * ---------------------------------------------------------------------------------------------- */
typedef struct mcr_fileset mcr_fileset;
#define MCR_FS_MEAN 0
#define MCR_FS_STD 1
#define MCR_FS_Q 2 /* [P][n_q] */
#define MCR_FS_MEDIAN 3
#define MCR_FS_RHAT 4
#define MCR_FS_ESS_BULK 5
#define MCR_FS_ESS_TAIL 6
#define MCR_FS_RHAT_BULK 7
#define MCR_FS_RHAT_TAIL 8
#define MCR_FS_LAG_BULK 9 /* truncation lags as doubles */
#define MCR_FS_LAG_TAIL 10
#define MCR_FS_FIELDS 11
int mcr_summarize_files(mcr_ctx* ctx, const char* const* paths, int n_paths, int min_chains,
                        const double* quantiles, int n_q, int diagnostics, mcr_fileset** out);
int mcr_fileset_size(const mcr_fileset* fs);
int64_t mcr_fileset_params(const mcr_fileset* fs, int file);
int64_t mcr_fileset_chains(const mcr_fileset* fs, int file);
int64_t mcr_fileset_draws(const mcr_fileset* fs, int file); /* draws per chain (of the first chain when they differ) */
const char* mcr_fileset_param_name(const mcr_fileset* fs, int file, int64_t param);
const double* mcr_fileset_field(const mcr_fileset* fs, int file, int field); /* P doubles (MCR_FS_Q: P * n_q) */
/* The whole set in two blocks, for callers that turn it into dictionaries (the shape reference.stats /
 * diagnostics_for_model return, src/mcmc_ref/reference.py:30-104) without a call per file and field:
 * mcr_fileset_export writes one row of 10 + n_q doubles per parameter, files and parameters in order -- mean, std,
 * median, rhat, ess_bulk, ess_tail, rhat_bulk, rhat_tail, lag_bulk, lag_tail, q[0 .. n_q) -- and returns the number of
 * rows of the set (at most cap_rows are written; rows may be NULL to ask); mcr_fileset_names writes the parameters'
 * names in the same order, each terminated by NUL, and returns the bytes that takes (written only if they fit cap). */
int64_t mcr_fileset_export(const mcr_fileset* fs, double* rows, int64_t cap_rows);
int64_t mcr_fileset_names(const mcr_fileset* fs, char* buf, int64_t cap);
/* Where the host-clock time of the mcr_summarize_files call that built `fs` went, in milliseconds (the path it replaces,
 * pq.read_table + the per-parameter loops of src/mcmc_ref/store.py:79-95 / reference.py:30-104, is host-bound, so the
 * split is part of the measurement): ms[MCR_FS_PH_*]; returns MCR_FS_PHASES (at most `cap` entries are written). */
#define MCR_FS_PH_OPEN 0    /* open + fstat of every file, staging buffers */
#define MCR_FS_PH_READ 1    /* MCR_IO_THREADS host threads (default 8): pread of the whole file images into pinned memory,
                               footer + page-header parse from there; uploads issued behind them in >= 2 MB pieces */
#define MCR_FS_PH_PLAN 2    /* request list, page table, table uploads */
#define MCR_FS_PH_DECODE 3  /* wait for the uploads + Snappy / page decode kernels + the chain / draw layout kernel */
#define MCR_FS_PH_STATS 4   /* the statistics pipeline of every job (enqueue, kernels, result copies) */
#define MCR_FS_PH_COLLECT 5 /* results into the set */
#define MCR_FS_PH_CLOSE 6   /* close, free of the parsed metadata */
#define MCR_FS_PH_TOTAL 7
#define MCR_FS_PHASES 8
int mcr_fileset_phases(const mcr_fileset* fs, double* ms, int cap);
/* How many tensors (kernel pipelines) the files of the set were summarised as: files of one (chains, draws) shape that sit
 * next to each other in the call's arena -- ordered by the chain count the footers' column statistics suggest -- are one. */
int mcr_fileset_jobs(const mcr_fileset* fs);
void mcr_fileset_free(mcr_fileset* fs);

/* ------------------------------------------------------------------------------------------------
 * CmdStan chain CSVs -> device tensor.
 * Replaces parse_cmdstan_csv (src/mcmc_ref/cmdstan_generate.py:13-29): the csv.DictReader row loop and
 * its float() per field.  Lines starting with '#' are dropped wherever they stand, the first remaining
 * line is the header, whitespace-only lines are no rows.  The text is uploaded once; one kernel indexes
 * the data rows, one parses them: every field is converted on the device by the Eisel-Lemire algorithm
 * (Lemire 2021; Mushtak & Lemire 2023), which is float()'s correctly rounded value or "hard".  Hard
 * fields -- more than 19 significant digits that sit on a rounding boundary, inf / nan, anything outside
 * [ws][+-]digits[.digits][eE[+-]digits][ws] -- are finished on the host with strtod after a check of
 * float()'s grammar (no underscores) and patched in; text float() would refuse ends the call with
 * MCR_EINVAL naming file, data row, column and text.  So does a row whose field count differs from the
 * header's and a '"' in a data row ("quoted fields are not supported").
 * Limits: the files of one call hold less than 4 GiB of text (offsets are 32-bit); at most 65535 files.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mcr_csv mcr_csv;
#define MCR_CSV_CHUNK 16384 /* bytes of text one workgroup of the line index scans */

/* Host only (ctx may be NULL, like mcr_parquet_open): finds the header line (cmdstan_generate.py:16-20), the body
 * offset and the column names of a file image, which the caller keeps alive and unchanged until mcr_csv_close. */
int mcr_csv_open(mcr_ctx* ctx, const void* bytes, size_t len, mcr_csv** out);
/* The same for files: replaces Path(path).open() + the line filter (cmdstan_generate.py:16-19) with the reader of
 * mcr_summarize_files -- MCR_IO_THREADS threads pread the images into the context's pinned buffer, the uploads are
 * issued behind them -- and fills out[0 .. n_paths).  The handles stay stageable until the context reads other files
 * (the next mcr_csv_open_paths, mcr_csv_stage of caller images, mcr_summarize_files or mcr_parquet_decode). */
int mcr_csv_open_paths(mcr_ctx* ctx, const char* const* paths, int n_paths, mcr_csv** out);
void mcr_csv_close(mcr_csv* f);
int mcr_csv_num_columns(const mcr_csv* f);                   /* 0: the file has no header line */
const char* mcr_csv_column_name(const mcr_csv* f, int column); /* raw header field, whitespace stripped; NULL if out of range */
int64_t mcr_csv_body_offset(const mcr_csv* f);               /* first byte after the header line */

/* Uploads the images (unless mcr_csv_open_paths already has), runs the line index and returns the data rows of
 * every file: the `for row in reader` count of cmdstan_generate.py:23.  All files share the launches. */
int mcr_csv_stage(mcr_ctx* ctx, const mcr_csv* const* files, int n_files, int64_t* rows);

/* Parses header columns columns[f * n_cols + k], k < n_cols, of the first max_rows data rows of every staged file f
 * into out_dev[f * stride_file + r * stride_row + k * stride_col] (float(value), cmdstan_generate.py:28; the caller
 * picks the columns, e.g. those not ending in "__", cmdstan_generate.py:25).  *hard = fields finished on the host. */
int mcr_csv_decode(mcr_ctx* ctx, const int* columns, int n_cols, int64_t max_rows, double* out_dev,
                   int64_t stride_file, int64_t stride_row, int64_t stride_col, int64_t* hard);

/* The device's field parser on the host (float(), cmdstan_generate.py:28).  Returns 0 = decided, 1 = hard (*out is
 * then the host finisher's strtod value), MCR_EINVAL = float() would raise ValueError. */
int mcr_parse_double(const char* text, size_t len, double* out);

/* ------------------------------------------------------------------------------------------------
 * Table CSVs -> device matrix: the table mode of the mcr_csv family.
 * Replaces pyarrow.csv.read_csv of the reference's convert_file (src/mcmc_ref/convert.py:70-75) for the
 * subset of its inputs that is certified against it: a header line (the first non-empty line, names raw)
 * and rows of numbers.  Every line is a data row unless it is empty ("\n\n", "\r\n\r\n"); "\r\n" is a
 * line end and the last line needs no newline; nothing is dropped for starting with '#'.  Every field
 * has to match -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)? with nothing around it and is converted
 * like mcr_parse_double; hard fields are finished on the host and patched in.  A column whose literals
 * all lack fraction and exponent is one pyarrow types int64 (all_int); -0 is stored as -0.0 and stays
 * so in a column that ends up double, as with pyarrow; a column that ends up all_int has its -0.0
 * rewritten to +0.0 before the call returns (int64 has no negative zero).
 * What leaves the subset ends the call with MCR_EFALLBACK -- the message names the first reason, the
 * file and the byte offset -- and the caller's host reader decides (it is the source of every
 * exception): a '"' anywhere, a field outside the grammar (empty, whitespace, '+', leading zeros, .5,
 * 5., inf, nan, text), an integer literal above 2^53, a row whose field count differs from the header's,
 * a "\r" without "\n", a non-empty whitespace-only line, a byte-order mark, a duplicated or empty header
 * name, a non-integer literal in an id column, no header or no data rows.  Limits as for the chain files
 * (4 GiB of text: MCR_EINVAL).
 * ---------------------------------------------------------------------------------------------- */
#define MCR_CSV_T_BOM 1        /* mcr_csv_table_flags: the header conditions that leave the subset */
#define MCR_CSV_T_DUP_NAME 2
#define MCR_CSV_T_EMPTY_NAME 4
#define MCR_CSV_T_QUOTE 8
#define MCR_CSV_T_CR 16
#define MCR_CSV_T_NO_HEADER 32
/* mcr_csv_open / mcr_csv_open_paths in table mode.  The handles work with mcr_csv_close, mcr_csv_num_columns,
 * mcr_csv_column_name (raw bytes, not stripped), mcr_csv_body_offset and mcr_csv_stage, which counts the rows by the
 * table rules and answers MCR_EFALLBACK for a flagged header or a file without data rows.  Table files and chain files
 * do not share a stage call. */
int mcr_csv_open_table(mcr_ctx* ctx, const void* bytes, size_t len, mcr_csv** out);
int mcr_csv_open_table_paths(mcr_ctx* ctx, const char* const* paths, int n_paths, mcr_csv** out);
int mcr_csv_table_flags(const mcr_csv* f); /* MCR_CSV_T_* bits; -1 for NULL or a chain-file handle */

/* Parses the staged table files whole.  columns[f * n_cols + k] = header column of file f stored as output column k
 * (-1: the file has fewer), id_columns[2 * f] / [2 * f + 1] = its `chain` / `draw` column (-1: absent); every header
 * column has to be one or the other.  Values go to out_dev[f * stride_file + r * stride_row + k * stride_col];
 * stride_file = stride_col = 0 asks for the packed layout: file after file, each [its columns][its rows] ([P][M] with
 * stride_row = 1).  Id fields go as int64 to ids_dev, laid out [file][chain | draw][row] (2 * rows entries per file,
 * packed).  all_int[f * n_cols + k] (host) = 1 when every literal of the column is an integer.  Rows past max_rows are
 * not read.  *hard = fields finished on the host. */
int mcr_csv_decode_table(mcr_ctx* ctx, const int* columns, int n_cols, const int* id_columns, int64_t max_rows,
                         double* out_dev, int64_t stride_file, int64_t stride_row, int64_t stride_col,
                         int64_t* ids_dev, uint8_t* all_int, int64_t* hard);

/* The table parser's field routine on the host.  Returns 0 = decided, 1 = hard (*value is then the host finisher's),
 * MCR_EFALLBACK = text outside the subset or an integer literal above 2^53.
 * *is_int = the literal has neither fraction nor exponent ("-0": -0.0 with *is_int = 1). */
int mcr_parse_csv_number(const char* text, size_t len, double* value, int* is_int);

/* ------------------------------------------------------------------------------------------------
 * Chain-list JSON -> device tensor.
 * Replaces json.loads + np.asarray of the JSON-zip reader (src/mcmc_ref/convert.py:78-102) for the
 * inflated text of a `<name>.json.zip` member: [ {"param": [draws...], ...}, ... ], one object per chain.
 * The text is uploaded once.  A structural index finds every [ ] { } : , outside a string; the host
 * walks the few tokens that are not commas against the text (chains, keys, arrays and their lengths);
 * one kernel checks every array element against the strict JSON number grammar
 * -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)? and converts the selected ones like mcr_parse_double.
 * Hard elements (rounding decided by digits past the 19th; exactly NaN, Infinity, -Infinity) are
 * finished on the host and patched in.  An integer literal has no negative zero (-0 is +0.0).
 * The certified subset: no backslash anywhere; a non-empty top-level array of objects; every member a
 * key without control characters and a flat array of numbers; no key twice in one object; no integer
 * literal above 2^53 among the stored elements.  Everything else -- valid JSON or not -- ends the call
 * with MCR_EFALLBACK and the caller's host reader decides (it is the source of every exception).
 * Limit: a document holds less than 4 GiB (offsets are 32-bit), checked before a byte is read.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mcr_json mcr_json;
#define MCR_JSON_CHUNK 16384      /* bytes of text one workgroup of the structural index scans */
#define MCR_JSON_PARSE_BLOCK 256  /* array elements one workgroup of the element parser converts */

/* Uploads the document, runs the structural index and the skeleton walk.  The caller keeps `bytes` alive and unchanged
 * until mcr_json_close, and closes the handle before the context is freed.  It invalidates files staged by mcr_csv_stage
 * and handles of mcr_csv_open_paths (the index borrows the staged row table): open and stage them again before a decode. */
int mcr_json_open(mcr_ctx* ctx, const void* bytes, size_t len, mcr_json** out);
void mcr_json_close(mcr_json* f);
int mcr_json_num_chains(const mcr_json* f);
int mcr_json_num_keys(const mcr_json* f, int chain);
const char* mcr_json_key(const mcr_json* f, int chain, int k); /* raw UTF-8 between the quotes, document order */
int64_t mcr_json_length(const mcr_json* f, int chain, int k);  /* elements of the key's array */

/* arrays[c * n_params + p] = the key, within chain c, of parameter slot p.  The first n_draws elements of each selected
 * array (none may be shorter) go to out_dev[c * stride_c + v * stride_n + p * stride_p]; every other element of the
 * document is checked against the grammar only.  all_int[c * n_params + p] = 1 when all stored elements of that array
 * were integer literals (no fraction, no exponent).  *hard = elements finished on the host. */
int mcr_json_decode(mcr_ctx* ctx, const mcr_json* f, const int* arrays, int n_params, int64_t n_draws, double* out_dev,
                    int64_t stride_c, int64_t stride_n, int64_t stride_p, uint8_t* all_int, int64_t* hard);

/* The device's element routine on the host (float(json.loads(text))).  Returns 0 = decided, 1 = hard (*value is then the
 * host finisher's), MCR_EINVAL = not a number json.loads accepts, MCR_EFALLBACK = an integer literal above 2^53.
 * *is_int = the literal has neither fraction nor exponent. */
int mcr_parse_json_number(const char* text, size_t len, double* value, int* is_int);

#ifdef __cplusplus
}
#endif
#pragma GCC visibility pop
#endif /* MCMCREF_HIP_H */
