/*
 * mcmcref_hip_ext.h -- the extension ABI of libmcmcref_hip.so: entries added after the surface of mcmcref_hip.h was
 * frozen.  Entries are prefixed mcrx_, constants MCRX_.  No structures: plain pointers and sizes.  The conventions of
 * mcmcref_hip.h hold (return codes, mcr_last_error, one ctx per GPU, calls on a ctx serialised by the caller).
 *
 * Dense symmetric positive definite linear algebra in IEEE double (true division, correctly rounded sqrt), and the
 * joint Gaussian check built on it: do the first two moments of two samples' joint distributions agree?
 */
#ifndef MCMCREF_HIP_EXT_H
#define MCMCREF_HIP_EXT_H

#include "mcmcref_hip.h"

#pragma GCC visibility push(default)
#ifdef __cplusplus
extern "C" {
#endif

#define MCRX_LINALG_MAX_P 8192 /* the largest matrix order, as mcr_covariance */
#define MCRX_CHOL_NB 64        /* block size of the factorisation and the solve; part of the summation order */

/* out8 of mcrx_gaussian_check, and info3 */
#define MCRX_G_D2_REF 0
#define MCRX_G_D2_ACT 1
#define MCRX_G_TRACE_REF 2
#define MCRX_G_TRACE_ACT 3
#define MCRX_G_LOGDET_REF 4
#define MCRX_G_LOGDET_ACT 5
#define MCRX_G_KL_ACT_REF 6
#define MCRX_G_KL_REF_ACT 7
#define MCRX_G_OUT 8
#define MCRX_G_P_LIVE 0
#define MCRX_G_INFO_REF 1
#define MCRX_G_INFO_ACT 2
#define MCRX_G_INFO 3

/* Cholesky factor of A [P][P], row-major with row stride lda >= P (elements): L lower triangular, L L^T = A, positive
 * diagonal.  Only the lower triangle (i >= j) of A is read: a NaN in the strict upper triangle changes nothing.
 *     l_jj = sqrt(a_jj - sum_{k<j} l_jk^2)        l_ij = (a_ij - sum_{k<j} l_ik l_jk) / l_jj
 * The strict upper triangle of the result is +0.0 (numpy.linalg.cholesky).
 * *info = 0, or c + 1 for the first column c whose pivot p fails p > 0 (zero, negative, NaN): LAPACK dpotrf's convention.
 * Then the leading c x c block of the result is the factor of that leading minor, the rest is unspecified and *logdet is
 * NaN; the call still returns MCR_OK.  *logdet = 2 sum_i log l_ii, the terms summed in the balanced tree of blocks of 1024
 * that the weighted summaries use (mcmcref_hip.h, MCR_WEIGHTED_BLOCK).  info and logdet may be NULL.
 *
 * The sum of an entry runs over the block columns of MCRX_CHOL_NB columns in ascending order: a block column's 64
 * products are accumulated on the matrix cores (v_mfma_f64_16x16x4f64, four columns per step, ascending) and the total is
 * subtracted from the entry; the entry's own block column is subtracted product by product, ascending, with fma.  Tiles
 * are anchored at row / column 0, so the bits of l_ij depend on the entries a_uv with u <= i and v <= j alone -- not on
 * P, lda or alignment: chol(A)[:n, :n] equals chol(A[:n, :n]) in bits for every n.
 * Right-looking: per block column k_chol_panel (one wave, a row of the diagonal block per lane), k_chol_below (the blocks under
 * it, a lane per row) and k_chol_update (the trailing lower-triangle tiles, MFMA), then k_chol_finish: 3 ceil(P / NB) - 1
 * launches, no host synchronisation between them; a failed pivot sets a device word that every later kernel reads first.
 * Cost P^3 / 3 multiply-adds.  a_dev in this ctx's device memory, factored IN PLACE; info and logdet on the host.
 * MCR_EINVAL (the message names the cause): a NULL pointer, P < 0, lda < P, P > MCRX_LINALG_MAX_P, summaries in flight.
 * P == 0 succeeds (*info = 0, *logdet = 0).  Synchronous, on the current lane's workspace, like mcr_covariance_dev. */
int mcrx_cholesky_dev(mcr_ctx* ctx, double* a_dev, int64_t P, int64_t lda, int64_t* info, double* logdet);
/* The same on host memory: a [P][P] with row stride lda is read, l [P][P] (row stride P) written.  Same bits. */
int mcrx_cholesky(mcr_ctx* ctx, const double* a, int64_t P, int64_t lda, double* l, int64_t* info, double* logdet);
/* The definition on the host (no ctx, no device): the unblocked loops above in ascending k, log from libm.  Its factor
 * meets the same error bound as the device's but is not equal to it in bits (the MFMA's order is not a host order).
 * The leading-minor property holds here too.  MCR_EINVAL as above (codes only, no message). */
int mcrx_cholesky_host(const double* a, int64_t P, int64_t lda, double* l, int64_t* info, double* logdet);

/* Solve L X = B: L [P][P] lower triangular with row stride ldl >= P (only i >= j is read, the diagonal is not checked),
 * B [P][K] row-major with row stride ldb >= K; X overwrites B.
 *     x_i = (b_i - sum_{j<i} l_ij x_j) / l_ii
 * with j in the blocked ascending order of the factorisation (earlier block rows on the matrix cores, the own block with
 * fma).  A column of X has the same bits alone or anywhere in a batch, for any K and ldb.  k_solve_lower: a workgroup
 * owns 64 columns of B and walks the block rows top to bottom; one launch for any K.  l_dev and b_dev in this ctx's
 * device memory.  MCR_EINVAL: a NULL pointer, P or K < 0, ldl < P, ldb < K, P > MCRX_LINALG_MAX_P, summaries in flight.
 * P == 0 or K == 0 succeeds and writes nothing.  Synchronous. */
int mcrx_solve_lower_dev(mcr_ctx* ctx, const double* l_dev, int64_t P, int64_t ldl, double* b_dev, int64_t K, int64_t ldb);
/* The same on host memory; x [P][K] (row stride K) receives the solution, b is only read.  Same bits. */
int mcrx_solve_lower(mcr_ctx* ctx, const double* l, int64_t P, int64_t ldl, const double* b, int64_t K, int64_t ldb, double* x);
/* The definition on the host: the unblocked loop in ascending j.  MCR_EINVAL as above (codes only). */
int mcrx_solve_lower_host(const double* l, int64_t P, int64_t ldl, const double* b, int64_t K, int64_t ldb, double* x);

/* Joint Gaussian check of two samples, ref [P][Mr] and act [P][Ma], row-major f64 as for mcr_two_sample.
 * scale [P]: finite and >= 0, NULL = all ones.  The LIVE parameters are those with scale > 0, P_live of them, kept in
 * their order; jitter is finite and >= 0.  With s the live scales, mu the means -- mu_p = K + (sum_m (x_pm - K)) / M around
 * the pivot K = x_p0, so that a constant parameter has exactly its value as mean and an exactly zero variance (k_row_mean;
 * not the streaming moments of mcr_covariance, whose summation order follows the rows' alignment) -- and Sigma the
 * population covariances around them (k_cov_mfma and k_cov_final, as mcr_covariance):
 *     C_r = diag(s) Sigma_ref diag(s) + jitter I     C_a = diag(s) Sigma_act diag(s) + jitter I     d = s (mu_act - mu_ref)
 *     L_r = chol(C_r)   L_a = chol(C_a)              info_ref, info_act (columns counted among the live parameters)
 *     y_r = L_r^-1 d    d2_ref = y_r^T y_r           squared Mahalanobis distance of the mean shift in the reference's metric
 *     y_a = L_a^-1 d    d2_act = y_a^T y_a
 *     trace_ref = |L_r^-1 L_a|_F^2 = tr(C_r^-1 C_a)  trace_act = |L_a^-1 L_r|_F^2                   (no inverse is formed)
 *     kl_act_ref = (trace_ref + d2_ref - P_live + logdet_ref - logdet_act) / 2                      KL(N_act || N_ref)
 *     kl_ref_act = (trace_act + d2_act - P_live + logdet_act - logdet_ref) / 2
 * (the entry s_i s_j Sigma_ij is (s_i * s_j) * Sigma_ij; the KL sums run left to right as written).
 * out8[MCRX_G_OUT], by the MCRX_G_* indices: d2_ref, d2_act, trace_ref, trace_act, logdet_ref, logdet_act, kl_act_ref,
 * kl_ref_act.  info3 = {P_live, info_ref, info_act}.  shift (P_live doubles, may be NULL) receives y_r: entry i is the
 * shift of live parameter i given the ones before it, in conditional standard deviations.
 * A singular covariance (a constant or exactly dependent parameter) is a FINDING, not an error: MCR_OK with the info set
 * and every output that needs the failed factor NaN (d2_act and logdet_act survive a failed reference factor, and vice
 * versa).  Non-finite draws are not looked for: a NaN reaches a pivot and is reported through info.  P_live == 0: NaN
 * outputs, zero infos.  NO p-value, for the reason given at mcr_energy_distance.  In exact arithmetic with jitter = 0 every
 * output but the two logdets is invariant to scale: the scale is there for conditioning and gives jitter a meaning on the
 * correlation scale.
 * Every sum (d2, the Frobenius norms row by row and then over the rows, logdet) is taken in the tree of blocks of 1024, in
 * an order that depends on P_live only: a call gives the same bits from the host and the device entry, at any 8-byte
 * alignment of the inputs, on repeated calls, with or without profiling.
 * Cost O((Mr + Ma) P^2 + P^3).  The call carves its whole workspace once (mcrx_gaussian_workspace: both matrices, the
 * solve result, the covariance partials, the means); there is no chunking: MCR_ENOMEM, naming the need, when the
 * workspace limit is smaller.  MCR_EINVAL (naming the cause): a NULL pointer (ref, act, out8, info3), P < 0, Mr or Ma < 1,
 * P > MCRX_LINALG_MAX_P, a negative or non-finite scale or jitter, summaries in flight.  P == 0 succeeds and writes
 * nothing.  The context stays usable after every error.  Synchronous. */
int mcrx_gaussian_check(mcr_ctx* ctx, const double* ref, int64_t Mr, const double* act, int64_t Ma, int64_t P,
                        const double* scale, double jitter, double* out8, int64_t* info3, double* shift);
/* The same with ref_dev / act_dev in this ctx's device memory; everything else on the host. */
int mcrx_gaussian_check_dev(mcr_ctx* ctx, const double* ref_dev, int64_t Mr, const double* act_dev, int64_t Ma, int64_t P,
                            const double* scale, double jitter, double* out8, int64_t* info3, double* shift);
/* The definition on the host, without a context: plain unblocked loops in double (means and centred products in
 * ascending draw order, the same pivot, mcrx_cholesky_host, mcrx_solve_lower_host, the same tree sums).  Codes only, no message. */
int mcrx_gaussian_check_host(const double* ref, int64_t Mr, const double* act, int64_t Ma, int64_t P, const double* scale,
                             double jitter, double* out8, int64_t* info3, double* shift);
/* Bytes of workspace a mcrx_gaussian_check(_dev) call of this shape carves (sized for P_live = P). */
int mcrx_gaussian_workspace(mcr_ctx* ctx, int64_t Mr, int64_t Ma, int64_t P, size_t* bytes);

#ifdef __cplusplus
}
#endif
#pragma GCC visibility pop
#endif /* MCMCREF_HIP_EXT_H */
