/*
 * mcmcref_bm.h -- the C ABI of libmcmcref_bm.so, the second companion library of libmcmcref_hip.so: batch means of the
 * draws, the long-run covariance Sigma of the Markov-chain central limit theorem, sqrt(M) (xbar - mu) -> N(0, Sigma),
 * and what follows from it: a calibrated joint test of two samples' means and the multivariate effective sample size.
 * Entries are prefixed mcb_, constants MCB_.  No structures: plain pointers and sizes.  This header takes from
 * mcmcref_hip.h the return codes (MCR_OK, MCR_EINVAL, MCR_EHIP, MCR_ENOMEM, MCR_ENODEVICE) and the dtype constants
 * (MCR_F64, MCR_F32) and nothing else; the library links against neither of the other two and uses none of their
 * internals.  Device addresses come from the caller (for instance mcr_dev_alloc of a ctx on the same device): the libraries
 * run in one process on one HIP runtime, so an address is valid in all of them.  The caller orders its own work first
 * (mcr_sync) -- an mcb call runs on a stream its handle owns, and every mcb_*_dev entry is synchronous.  Calls on one
 * handle are serialised by the caller.
 *
 * WHAT IT IS.  The replicated multivariate batch-means estimator, centred at the overall mean of the batch means (Vats,
 * Flegal and Jones 2019, Multivariate output analysis for Markov chain Monte Carlo), optionally in its lugsail form with
 * r = 3 (Vats and Flegal 2022), which takes out most of the estimator's downward bias.  The chi-square of the mean test
 * is ASYMPTOTIC: it holds as the batches grow long beside the autocorrelation time and many beside P.  The numbers differ
 * from R's mcmcse (mcse.multi, multiESS), which is not installed here and was not compared against, in which draws are
 * dropped (here the FIRST N - a b of every chain) and in the batch-size rule (mcb_batch_size).
 *
 * THE DEFINITION.
 * Tensor and batches.  Element (c, n, p) is at c stride_c + n stride_n + p stride_p (elements, strides >= 0), dtype
 * MCR_F64 or MCR_F32; an f32 draw is widened exactly.  C, N, P >= 1; batch size 1 <= b <= N; a = floor(N / b) batches
 * per chain, A = C a in all.  Batches cover the LAST a b draws of each chain: with n0 = N - a b, batch k of chain c covers
 * the draws n0 + k b ... n0 + (k + 1) b - 1.
 * Batch sums and means.  Pivot K_p = x[0][n0][p]; leaves t_i = x_i - K_p, rounded once.  A batch sum s is taken in the
 * project's one association: blocks of MCB_BLOCK = 1024 consecutive leaves, counted from the batch's first draw; within a
 * block the balanced binary tree over adjacent leaves, +0 past the end; the blocks' roots added in ascending order from
 * +0; no fused multiply-add anywhere.  Then
 *     bm[p][c a + k] = K_p + s / b                      bm is f64 [P][ld], ld >= A: with ld = A what mcr_covariance_dev reads
 *     mu[p]          = K_p + S / (A b)                  S = the sum of the A batch sums in index order, in the same tree
 * (b and A b are converted to double; A b is formed as an integer).  A constant parameter has every leaf +0: bm and mu
 * are exactly its value and every variance below is exactly zero.  NaN / Inf draws are not looked for: they propagate.
 * Default batch size (mcb_batch_size).  r = 1: b = floor(sqrt(N)).  r = 3: b = 3 max(1, floor(sqrt(N) / 3)), which needs
 * N >= 3.  r is 1 or 3.
 * Finish (element-wise).  Cb [P][P] is the population covariance of the rows of bm (mcr_covariance_dev with M = A); for
 * r = 3 Cb3 is the same of the batch means at batch size b / 3, of which there are A3 = C floor(N / (b / 3)).
 *     Sigma_b = Cb f,   f = ((double) b * (double) A) / (double) (A - 1)        (operations left to right)
 *     Sigma   = Sigma_b                             for r = 1
 *     Sigma   = 2 Sigma_b - Sigma_{b/3}             for r = 3 (lugsail), Sigma_{b/3} = Cb3 f3 with b / 3 and A3 in f
 * A < 2: every entry NaN.
 * Pool (element-wise).  scale s [P] finite and >= 0, NULL = all ones, 0 drops the parameter; the live parameters are
 * compacted in their order, P_live of them, as in mcrx_gaussian_check.  With M = A b of each sample (the draws its batches
 * cover) and i, j live:
 *     V_ij = (s_i * s_j) * (Sr_ij / M_r + Sa_ij / M_a) + [i == j] jitter     d_i = s_i * (mu_act_i - mu_ref_i)
 *     z_i  = d_i / sqrt(V_ii)                                                the shift in Monte Carlo standard errors
 * With the actual sample's pair of pointers NULL the second term and mu_act drop out (V_ij = (s_i * s_j) * (Sr_ij / M_r) +
 * [i == j] jitter, d_i = s_i * mu_ref_i): with M_r = 1 that is the scaled live matrix itself.
 * Test.  L = mcrx_cholesky_dev(V) gives info and logdet; y = mcrx_solve_lower_dev(L, d); T = sum y_i^2 in the tree
 * (mcb_tree_sum_host); p_value = mcr_chi2_sf(T, P_live).  Under equal means T ~ chi^2 with P_live degrees of freedom.  A
 * singular V is a finding, not an error, and a V that lugsail has made indefinite counts as singular too: info != 0 and
 * T, p_value and y NaN.  For r = 1 V is certainly singular when (A_ref - 1) + (A_act - 1) < P_live: a covariance of A
 * batch means has rank A - 1 at most.
 * Multivariate ESS (Vats, Flegal and Jones 2019).  Lambda = mcr_covariance_dev of the pooled C N draws [P][C N];
 *     mESS = C N exp((logdet Lambda_s - logdet Sigma_s) / P_live)
 * on the scaled live matrices (pool with a NULL actual pair and M_r = 1); per parameter mcse_mean = sqrt(Sigma_pp / (A b))
 * and ess_bm = C N Lambda_pp / Sigma_pp.
 *
 * THE CALL SEQUENCE for a C caller, all buffers from mcr_dev_alloc, per sample:
 *     mcr_sync; mcb_batch_means_dev (b) -> bm, mu; mcr_covariance_dev(bm, A, P) -> Cb;
 *     for r = 3 the same at b / 3 -> Cb3;  mcb_lrv_finish_dev -> Sigma;
 * then mcb_pool_dev -> V, d, z; mcrx_cholesky_dev(V); mcrx_solve_lower_dev(V, d, K = 1); d to the host;
 * mcb_tree_sum_host; mcr_chi2_sf.  For mESS: mcb_pooled_dev -> [P][C N]; mcr_covariance_dev -> Lambda; mcb_pool_dev of
 * each of Lambda and Sigma alone; mcrx_cholesky_dev of both.
 */
#ifndef MCMCREF_BM_H
#define MCMCREF_BM_H

#include "mcmcref_hip.h"

#pragma GCC visibility push(default)
#ifdef __cplusplus
extern "C" {
#endif

#define MCB_VERSION 100
#define MCB_BLOCK 1024         /* consecutive leaves of one tree; part of the summation order */
#define MCB_KERNEL_TIME 0      /* mcb_kernel_ms: index of k_bm_time's time */
#define MCB_KERNEL_TILE 1      /* ... of k_bm_tile's */
#define MCB_KERNEL_MEAN 2      /* ... of k_bm_mean's */
#define MCB_KERNEL_FINISH 3    /* ... of k_bm_finish's */
#define MCB_KERNEL_POOL 4      /* ... of k_bm_pool's */
#define MCB_KERNEL_POOLED 5    /* ... of k_bm_pooled's */
#define MCB_KERNELS 6

/* The library's version, MCB_VERSION. */
int mcb_version(void);
/* A handle on HIP device `device`: a stream and device workspace that only grows.  MCR_ENODEVICE when the device cannot
 * be used; then mcb_last_error(NULL) holds the message. */
int mcb_init(int device, void** handle);
void mcb_free(void* handle);
/* The message of the last failed call on the handle (NULL: of this thread's last failed call that takes no handle). */
const char* mcb_last_error(void* handle);
/* Upper bound in bytes of the device workspace of one chunk of parameters of mcb_batch_means(_dev) (the batch sums, 8 A
 * bytes per parameter; default 1 GiB).  A call cuts its parameters into chunks under it; MCR_ENOMEM from a later call when
 * one parameter alone does not fit. */
int mcb_set_workspace_limit(void* handle, size_t bytes);
/* The default batch size b of chains of N draws and the batches a = floor(N / b) per chain, for r = 1 or 3 (above).
 * MCR_EINVAL: a NULL pointer, N < 1, r not 1 or 3, r = 3 with N < 3. */
int mcb_batch_size(int64_t N, int r, int64_t* b, int64_t* a);

/* Batch means bm_dev [P][ld] and the overall means mu_dev [P] (either may be NULL) of a draw tensor, all in device memory.
 * One streaming pass over the tensor on one of two routes that give the same bits as each other and as
 * mcb_batch_means_host.  k_bm_time (stride_n == 1): a wave takes batches of one (p, c) -- eight batches at a time, one per
 * register row, when b <= 128, else a block of 1024 leaves at a time -- with two consecutive leaves per lane (one 16-byte
 * load where the address allows it) and builds the tree from its lanes.  k_bm_tile (any other strides): a wave takes 64
 * parameters, lane = parameter, so that the 64 loads of a step are 64 rows of 64 consecutive parameters (coalesced when
 * stride_p == 1, the sampler's [C][N][P]; they go straight to registers: a lane reads only its own column, so there is
 * nothing to exchange through LDS), sums its 64 leaves in the fixed tree of 64 and pairs the 64-leaf nodes up with a
 * binary counter (pairwise summation, four pending nodes).  Vector stores
 * only, no atomics, a fixed order.  Then k_bm_mean, a wave per parameter.  A parameter's outputs have the same bits alone,
 * anywhere in a batch, under any chunking, on either route, at any alignment, with or without profiling.
 * MCR_EINVAL (the message names the cause): a NULL handle or tensor, both outputs NULL; a dtype other than the two; C, N
 * or P < 1; b outside [1, N]; a negative stride; ld < A.  After an error the handle stays usable. */
int mcb_batch_means_dev(void* handle, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                        int64_t stride_n, int64_t stride_p, int64_t b, double* bm_dev, int64_t ld, double* mu_dev);
/* The same on a tensor in host memory, which it uploads (the span the strides reach); bm [P][ld] and mu [P] on the host. */
int mcb_batch_means(void* handle, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                    int64_t stride_n, int64_t stride_p, int64_t b, double* bm, int64_t ld, double* mu);
/* The definition on the host: no handle, no device, the same refusals.  Same bits as the device. */
int mcb_batch_means_host(const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c, int64_t stride_n,
                         int64_t stride_p, int64_t b, double* bm, int64_t ld, double* mu);
/* The exact f64 copy pooled_dev [P][ld] of the tensor, pooled_dev[p][c N + n] = x[c][n][p] (ld >= C N): what
 * mcr_covariance_dev reads for Lambda.  k_bm_pooled.  Refusals as above. */
int mcb_pooled_dev(void* handle, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                   int64_t stride_n, int64_t stride_p, double* pooled_dev, int64_t ld);

/* Finish: sigma [P][P] from cb [P][P] and, for r = 3, cb3 [P][P] (ignored for r = 1, may be NULL); sigma may be cb.
 * k_bm_finish.  MCR_EINVAL: a NULL pointer; P < 1; b < 1; A < 1; r not 1 or 3; r = 3 with b not divisible by 3 or A3 < 1. */
int mcb_lrv_finish_dev(void* handle, const double* cb_dev, const double* cb3_dev, int64_t P, int64_t b, int64_t A,
                       int64_t A3, int r, double* sigma_dev);
int mcb_lrv_finish_host(const double* cb, const double* cb3, int64_t P, int64_t b, int64_t A, int64_t A3, int r,
                        double* sigma);

/* Pool: v [P_live][P_live] (row stride P_live), d [P_live] and z [P_live] from the two samples' sigma [P][P] and mu [P];
 * sig_act and mu_act may both be NULL (above).  scale [P] (may be NULL) and *p_live are on the host.  k_bm_pool.
 * MCR_EINVAL: a NULL pointer other than those; P < 1; M_ref or M_act < 1; a non-finite or negative scale or jitter.
 * P_live == 0 succeeds and writes nothing but *p_live. */
int mcb_pool_dev(void* handle, const double* sig_ref_dev, const double* mu_ref_dev, int64_t M_ref, const double* sig_act_dev,
                 const double* mu_act_dev, int64_t M_act, int64_t P, const double* scale, double jitter, double* v_dev,
                 double* d_dev, double* z_dev, int64_t* p_live);
int mcb_pool_host(const double* sig_ref, const double* mu_ref, int64_t M_ref, const double* sig_act, const double* mu_act,
                  int64_t M_act, int64_t P, const double* scale, double jitter, double* v, double* d, double* z,
                  int64_t* p_live);

/* *sum = the sum of y_i * y_i (squares != 0; each product rounded) or of y_i over i < n, in the tree.  n == 0 gives +0.
 * MCR_EINVAL: a NULL pointer, n < 0. */
int mcb_tree_sum_host(const double* y, int64_t n, int squares, double* sum);

/* Per-kernel times: when enabled (on != 0) every later mcb_*_dev call brackets its kernels with HIP events;
 * mcb_kernel_ms writes the LAST call's totals over its chunks in milliseconds by the MCB_KERNEL_* indices (cap >=
 * MCB_KERNELS, else MCR_EINVAL); a kernel that did not run in that call, or an untimed call, reads 0. */
int mcb_profile_enable(void* handle, int on);
int mcb_kernel_ms(void* handle, double* ms, int cap);

#ifdef __cplusplus
}
#endif
#pragma GCC visibility pop

#endif
