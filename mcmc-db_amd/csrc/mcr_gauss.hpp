// mcr_gauss.hpp -- dense symmetric positive definite linear algebra in fp64 and the joint Gaussian check on top of it
// (include/mcmcref_hip_ext.h has the definitions): a blocked right-looking Cholesky factorisation, the forward solve
// L X = B, the scaled gather of a covariance matrix and the tree sums of the check's statistics, each with the host
// routine behind its mcrx_*_host entry.
//
// The block size kCholNB = 64 is part of the summation order.  An entry (i, j) of the factor, in block (bi, bj), takes
//   1. for every block column k < bj, in ascending order: a 64-term product sum from the matrix cores
//      (v_mfma_f64_16x16x4f64: four columns per instruction, ascending), subtracted from the entry (k_chol_update);
//   2. its own block column: product by product, ascending, with fma, then the division or the square root
//      (k_chol_panel on the diagonal block, k_chol_below under it).
// Tiles are anchored at row / column 0 and a lane's result depends on its own operand row and column only, so the bits
// of l_ij are a function of the entries a_uv, u <= i, v <= j: not of P, lda, alignment or what else is in the matrix.
// The solve follows the same rule with one accumulator over all earlier block rows (k_solve_lower).
// 64 against 128: a 64 x 64 fp64 block is 32 KB, so the diagonal block and a 64-row strip (or both MFMA operands) sit in
// LDS together with room for a second workgroup per CU, and the shapes validate() sees (P of a few hundred) are a handful
// of launches either way.  128 would halve the trailing update's memory traffic at P in the thousands; that was not
// measured here.
#pragma once
#include <cmath>
#include <limits>
#include <vector>

#include "mcr_device.hpp"
#include "mcr_tree.hpp"

namespace mcr {

constexpr int kCholNB = 64;                   // MCRX_CHOL_NB
constexpr int kCholLdV = kCholNB + 1;         // LDS row stride where a lane walks its own row (VALU kernels): lane + column banks
constexpr int kCholLdM = kCholNB + 2;         // ... where the MFMA operands are fetched (lane 16 k + i reads row i, column k)
constexpr i64 kLinalgMaxP = 8192;             // MCRX_LINALG_MAX_P
constexpr int kGaussOut = 8;                  // MCRX_G_OUT

// ---- the host definitions -------------------------------------------------------------------------------------------

// A sum in the one association of mcr_tree.hpp.
template <class Term> inline double gauss_sum_host(i64 n, Term&& term)
{
    WgtHostTree tr;
    return wgt_host_sum(tr, n, term);
}

// 0, or 1 for a bad argument.  l [P][P] with row stride P; *info and *logdet as mcrx_cholesky states.
inline int chol_host(const double* a, i64 P, i64 lda, double* l, i64* info, double* logdet)
{
    if (P < 0 || P > kLinalgMaxP || lda < P || (P > 0 && (!a || !l))) return 1;
    i64 bad = 0;
    for (i64 e = 0; e < P * P; ++e) l[e] = 0.0;
    for (i64 i = 0; i < P && !bad; ++i)
        for (i64 j = 0; j <= i; ++j) {
            double s = a[i * lda + j];
            for (i64 k = 0; k < j; ++k) s = std::fma(-l[i * P + k], l[j * P + k], s);
            if (i == j) {
                if (!(s > 0.0)) { bad = j + 1; break; }
                l[i * P + j] = std::sqrt(s);
            } else {
                l[i * P + j] = s / l[j * P + j];
            }
        }
    if (info) *info = bad;
    if (logdet)
        *logdet = bad ? std::numeric_limits<double>::quiet_NaN()
                      : 2.0 * gauss_sum_host(P, [&](i64 i) { return std::log(l[i * P + i]); });
    return 0;
}

// 0, or 1 for a bad argument.  x [P][K] with row stride K.
inline int solve_lower_host(const double* l, i64 P, i64 ldl, const double* b, i64 K, i64 ldb, double* x)
{
    if (P < 0 || K < 0 || P > kLinalgMaxP || ldl < P || ldb < K || (P > 0 && K > 0 && (!l || !b || !x))) return 1;
    for (i64 i = 0; i < P; ++i)
        for (i64 c = 0; c < K; ++c) {
            double s = b[i * ldb + c];
            for (i64 j = 0; j < i; ++j) s = std::fma(-l[i * ldl + j], x[j * K + c], s);
            x[i * K + c] = s / l[i * ldl + i];
        }
    return 0;
}

// The live parameters of a call: 0, or 1 for a negative or non-finite scale.
inline int gauss_live(const double* scale, i64 P, std::vector<int>& idx, std::vector<double>& s)
{
    for (i64 p = 0; p < P; ++p) {
        const double v = scale ? scale[p] : 1.0;
        if (!(v >= 0.0) || std::isinf(v)) return 1;
        if (v > 0.0) { idx.push_back((int)p); s.push_back(v); }
    }
    return 0;
}

// The two divergences from the six sums, and NaN for whatever needs a factor that failed.
inline void gauss_outputs(double* out, i64 PL, i64 info_ref, i64 info_act)
{
#pragma clang fp contract(off)
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (PL == 0) { for (int k = 0; k < kGaussOut; ++k) out[k] = nan; return; }
    if (info_ref) out[0] = out[4] = nan;
    if (info_act) out[1] = out[5] = nan;
    if (info_ref || info_act) out[2] = out[3] = nan;
    out[6] = 0.5 * (out[2] + out[0] - (double)PL + out[4] - out[5]);
    out[7] = 0.5 * (out[3] + out[1] - (double)PL + out[5] - out[4]);
}

// 0, or 1 for a bad argument.
inline int gauss_host(const double* ref, i64 Mr, const double* act, i64 Ma, i64 P, const double* scale, double jitter,
                      double* out, i64* info3, double* shift)
{
#pragma clang fp contract(off)
    if (P < 0 || P > kLinalgMaxP || Mr < 1 || Ma < 1 || !(jitter >= 0.0) || std::isinf(jitter)) return 1;
    if (P == 0) return 0;
    if (!ref || !act || !out || !info3) return 1;
    std::vector<int> idx;
    std::vector<double> s;
    if (gauss_live(scale, P, idx, s)) return 1;
    const i64 PL = (i64)idx.size();
    info3[0] = PL; info3[1] = info3[2] = 0;
    if (PL == 0) { gauss_outputs(out, 0, 0, 0); return 0; }
    std::vector<double> mu[2], C[2], L[2], y[2], X((size_t)(PL * PL)), d((size_t)PL);
    const double* src[2] = {ref, act};
    const i64 M[2] = {Mr, Ma};
    for (int g = 0; g < 2; ++g) {
        mu[g].resize((size_t)PL); C[g].assign((size_t)(PL * PL), 0.0); L[g].resize((size_t)(PL * PL)); y[g].resize((size_t)PL);
        for (i64 i = 0; i < PL; ++i) {
            const double* x = src[g] + idx[(size_t)i] * M[g];
            const double K = std::isfinite(x[0]) ? x[0] : 0.0;     // the pivot: a constant parameter has the mean K exactly
            double t = 0.0;
            for (i64 m = 0; m < M[g]; ++m) t += x[m] - K;
            mu[g][(size_t)i] = K + t / (double)M[g];
        }
        for (i64 i = 0; i < PL; ++i)
            for (i64 j = 0; j <= i; ++j) {
                const double *xi = src[g] + idx[(size_t)i] * M[g], *xj = src[g] + idx[(size_t)j] * M[g];
                const double mi = mu[g][(size_t)i], mj = mu[g][(size_t)j];
                double t = 0.0;
                for (i64 m = 0; m < M[g]; ++m) t += (xi[m] - mi) * (xj[m] - mj);
                double v = (s[(size_t)i] * s[(size_t)j]) * (t / (double)M[g]);
                if (i == j) v = v + jitter;
                C[g][(size_t)(i * PL + j)] = v;
            }
    }
    for (i64 i = 0; i < PL; ++i) d[(size_t)i] = s[(size_t)i] * (mu[1][(size_t)i] - mu[0][(size_t)i]);
    i64 info[2];
    for (int g = 0; g < 2; ++g) {
        chol_host(C[g].data(), PL, PL, L[g].data(), &info[g], &out[4 + g]);
        if (info[g]) continue;
        solve_lower_host(L[g].data(), PL, PL, d.data(), 1, 1, y[g].data());
        out[g] = gauss_sum_host(PL, [&](i64 i) { return y[g][(size_t)i] * y[g][(size_t)i]; });
    }
    for (int g = 0; g < 2 && !info[0] && !info[1]; ++g) {             // |L_g^-1 L_other|_F^2: the rows' sums, then their sum
        solve_lower_host(L[g].data(), PL, PL, L[1 - g].data(), PL, PL, X.data());
        std::vector<double> rows((size_t)PL);
        for (i64 i = 0; i < PL; ++i)
            rows[(size_t)i] = gauss_sum_host(PL, [&](i64 j) { return X[(size_t)(i * PL + j)] * X[(size_t)(i * PL + j)]; });
        out[2 + g] = gauss_sum_host(PL, [&](i64 i) { return rows[(size_t)i]; });
    }
    info3[1] = info[0]; info3[2] = info[1];
    if (shift && !info[0]) for (i64 i = 0; i < PL; ++i) shift[i] = y[0][(size_t)i];
    if (shift && info[0]) for (i64 i = 0; i < PL; ++i) shift[i] = std::numeric_limits<double>::quiet_NaN();
    gauss_outputs(out, PL, info[0], info[1]);
    return 0;
}

// ---- the kernels ----------------------------------------------------------------------------------------------------

// A sum of n terms by a 256-thread workgroup in the association of mcr_tree.hpp: blocks of 1024 consecutive terms, a
// block's terms the leaves of the balanced tree over adjacent indices (a thread adds its four leaves, levels 1 and 2; the
// other eight levels go through red[256]), the blocks' roots added in ascending order from +0.  Every thread returns the sum.
template <class Term> __device__ __forceinline__ double gauss_tree_sum(i64 n, Term&& term, double* red)
{
#pragma clang fp contract(off)
    static_assert(kWgtBlock == 1024, "four leaves per thread of a 256-thread workgroup");
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (i64 b0 = 0; b0 < n; b0 += kWgtBlock) {
        const i64 i = b0 + 4 * tid;
        const double l0 = i < n ? term(i) : 0.0, l1 = i + 1 < n ? term(i + 1) : 0.0;
        const double l2 = i + 2 < n ? term(i + 2) : 0.0, l3 = i + 3 < n ? term(i + 3) : 0.0;
        red[tid] = (l0 + l1) + (l2 + l3);
        for (int w = 1; w < 256; w <<= 1) {
            __syncthreads();
            if ((tid & (2 * w - 1)) == 0) red[tid] = red[tid] + red[tid + w];
        }
        __syncthreads();
        acc = acc + red[0];
        __syncthreads();
    }
    return acc;
}

// The diagonal block at (k0, k0), n = min(NB, P - k0) rows, factored column by column by ONE wave, lane i holding row i
// in registers (the block is serial anyway; LDS only transposes the block on the way in and out and broadcasts the
// finished column): the pivot, the column under it, then the rank-1 update of the block's remaining lower triangle --
// entry (i, j) takes the products of the columns c < j in ascending order, each with fma(-l_ic, l_jc, a_ij).  Fully
// unrolled, so that the row stays in registers; one barrier per column (the broadcast column is double buffered).  A
// pivot that fails p > 0 writes its column + 1 to *info with an ordinary store and ends the factorisation; the block
// goes back as far as it got (the columns in front are final).
__global__ __launch_bounds__(kCholNB) void k_chol_panel(double* A, i64 P, i64 lda, i64 k0, i64* info)
{
    __shared__ double s[kCholNB * kCholLdV];
    __shared__ double col[2][kCholNB];
    if (*info != 0) return;
    const int t = threadIdx.x;
    const int n = P - k0 < kCholNB ? (int)(P - k0) : kCholNB;
    for (int r = 0; r < kCholNB; ++r) s[r * kCholLdV + t] = (r < n && t <= r) ? A[(k0 + r) * lda + k0 + t] : 0.0;
    __syncthreads();
    double row[kCholNB];
#pragma unroll
    for (int j = 0; j < kCholNB; ++j) row[j] = s[t * kCholLdV + j];
    bool live = true;                                            // uniform: no pivot has failed
#pragma unroll
    for (int c = 0; c < kCholNB; ++c) {
        const double p = __shfl(row[c], c, kWave);               // the same value in every lane
        if (live && c < n && !(p > 0.0)) {
            if (t == 0) *info = k0 + c + 1;
            live = false;
        }
        if (live && c < n) {
            const double d = sqrt(p);
            if (t == c) row[c] = d;
            else if (t > c) row[c] = row[c] / d;                 // (rows past n hold zeros and are not stored)
            col[c & 1][t] = row[c];
            __syncthreads();
#pragma unroll
            for (int j = c + 1; j < kCholNB; ++j) {
                const double lj = col[c & 1][j];
                if (t >= j) row[j] = fma(-row[c], lj, row[j]);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kCholNB; ++j) s[t * kCholLdV + j] = row[j];
    __syncthreads();
    for (int r = 0; r < kCholNB; ++r)
        if (r < n && t <= r) A[(k0 + r) * lda + k0 + t] = s[r * kCholLdV + t];
}

// The blocks under the diagonal block of block column k0 (which is full: there are rows under it): X L_kk^T = A, a lane
// per row, x_j = (a_j - sum_{c<j} x_c l_jc) / l_jj in ascending c with fma.  One wave per 64 rows; L_kk and the rows sit in
// LDS (the factor's reads are broadcasts, a lane's own row is one bank per lane).
__global__ __launch_bounds__(kCholNB) void k_chol_below(double* A, i64 P, i64 lda, i64 k0, const i64* info)
{
    __shared__ double sL[kCholNB * kCholLdV];
    __shared__ double sR[kCholNB * kCholLdV];
    if (*info != 0) return;
    const int t = threadIdx.x;
    const i64 r0 = k0 + kCholNB + (i64)blockIdx.x * kCholNB;
    for (int r = 0; r < kCholNB; ++r) {
        sL[r * kCholLdV + t] = t <= r ? A[(k0 + r) * lda + k0 + t] : 0.0;
        sR[r * kCholLdV + t] = r0 + r < P ? A[(r0 + r) * lda + k0 + t] : 0.0;
    }
    __syncthreads();
    double* row = sR + t * kCholLdV;
    for (int j = 0; j < kCholNB; ++j) {
        double acc = row[j];
#pragma unroll 8
        for (int c = 0; c < j; ++c) acc = fma(-row[c], sL[j * kCholLdV + c], acc);
        row[j] = acc / sL[j * kCholLdV + j];
    }
    __syncthreads();
    for (int r = 0; r < kCholNB; ++r)
        if (r0 + r < P) A[(r0 + r) * lda + k0 + t] = sR[r * kCholLdV + t];
}

// 64 x 64 x 64 on the matrix cores by a 256-thread workgroup: acc += sA sB^T (TRANS_B: sB holds [n][k]) or sA sB (sB holds
// [k][n]).  Wave w owns the 32 x 32 quadrant (w / 2, w % 2) as 2 x 2 MFMA tiles; the k axis goes four columns at a time in
// ascending order.  Operand and result layout as in k_cov_mfma (measured by tools/ubench/mfma64_layout.hip): lane 16 k + i
// supplies A[i][k] and B[k][i], and acc[a][b][v] is the entry (16 a + lane / 16 + 4 v, 16 b + lane % 16) of the quadrant.
typedef double gauss_v4d __attribute__((ext_vector_type(4)));
template <bool TRANS_B>
__device__ __forceinline__ void gauss_mfma_tile(const double* sA, const double* sB, gauss_v4d (&acc)[2][2])
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int wr = (w >> 1) * 32, wc = (w & 1) * 32, oi = lane & 15, ok = lane >> 4;
#pragma unroll
    for (int kk = 0; kk < kCholNB / 4; ++kk) {
        const int c = kk * 4 + ok;
        double av[2], bv[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            av[a] = sA[(wr + 16 * a + oi) * kCholLdM + c];
            bv[a] = TRANS_B ? sB[(wc + 16 * a + oi) * kCholLdM + c] : sB[c * kCholLdM + wc + 16 * a + oi];
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
    }
}

// The trailing update of block column k0: every tile (ti, tj), tj <= ti, of the lower triangle behind it takes
// A_ij -= L_ik L_jk^T.  No workgroup sits above the diagonal; a diagonal tile stores its lower half only.  Rows past P are
// staged as zeros and not stored.
__global__ __launch_bounds__(256) void k_chol_update(double* A, i64 P, i64 lda, i64 k0, const i64* info)
{
    __shared__ double sA[kCholNB * kCholLdM];
    __shared__ double sB[kCholNB * kCholLdM];
    if (*info != 0) return;
    int ti = 0, rest = (int)blockIdx.x;                          // lower-triangle tile index -> (ti, tj): row ti holds ti + 1 tiles
    while (rest > ti) { rest -= ti + 1; ++ti; }
    const int tj = rest, tid = threadIdx.x;
    const i64 ra = k0 + (i64)kCholNB * (1 + ti), rb = k0 + (i64)kCholNB * (1 + tj);
    for (int e = tid; e < kCholNB * kCholNB; e += 256) {
        const int r = e / kCholNB, c = e % kCholNB;
        sA[r * kCholLdM + c] = ra + r < P ? A[(ra + r) * lda + k0 + c] : 0.0;
        sB[r * kCholLdM + c] = rb + r < P ? A[(rb + r) * lda + k0 + c] : 0.0;
    }
    __syncthreads();
    gauss_v4d acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = gauss_v4d{0, 0, 0, 0};
    gauss_mfma_tile<true>(sA, sB, acc);
    const int lane = tid & 63, w = tid >> 6;
    const int wr = (w >> 1) * 32, wc = (w & 1) * 32, oi = lane & 15, ok = lane >> 4;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const i64 gi = ra + wr + 16 * a + ok + 4 * v, gj = rb + wc + 16 * b + oi;
                if (gi < P && gj <= gi) A[gi * lda + gj] = A[gi * lda + gj] - acc[a][b][v];
            }
}

// The finisher: +0.0 into the strict upper triangle, and from workgroup 0 the log-determinant 2 sum log l_ii in the tree
// (NaN when a pivot failed).
__global__ __launch_bounds__(256) void k_chol_finish(double* A, i64 P, i64 lda, const i64* info, double* logdet)
{
    __shared__ double red[256];
    const i64 e = (i64)blockIdx.x * 256 + threadIdx.x;
    if (e < P * P) {
        const i64 i = e / P, j = e % P;
        if (j > i) A[i * lda + j] = 0.0;
    }
    if (blockIdx.x != 0) return;
    const bool bad = *info != 0;
    const double t = gauss_tree_sum(bad ? 0 : P, [&](i64 i) { return log(A[i * lda + i]); }, red);
    if (threadIdx.x == 0) *logdet = bad ? __builtin_nan("") : 2.0 * t;
}

// L X = B for a strip of 64 columns of B per workgroup, which walks the block rows top to bottom on its own: block row bi
// takes sum_{bj < bi} L[bi][bj] X[bj] on the matrix cores (one accumulator, bj ascending) from the X blocks this workgroup
// wrote earlier, subtracts it from B[bi], and runs the 64 x 64 forward substitution in LDS (a lane per column, ascending
// with fma).  No workgroup depends on another.  info0 / info1 (either may be null): the call's factors; set means no solve.
__global__ __launch_bounds__(256) void k_solve_lower(const double* L, i64 P, i64 ldl, double* B, i64 K, i64 ldb,
                                                     const i64* info0, const i64* info1)
{
    __shared__ double sL[kCholNB * kCholLdM];
    __shared__ double sX[kCholNB * kCholLdM];
    if ((info0 && *info0 != 0) || (info1 && *info1 != 0)) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wr = (w >> 1) * 32, wc = (w & 1) * 32, oi = lane & 15, ok = lane >> 4;
    const i64 n0 = (i64)blockIdx.x * kCholNB;
    const i64 nblk = (P + kCholNB - 1) / kCholNB;
    for (i64 bi = 0; bi < nblk; ++bi) {
        const i64 r0 = bi * kCholNB;
        const int n = P - r0 < kCholNB ? (int)(P - r0) : kCholNB;
        gauss_v4d acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[a][b] = gauss_v4d{0, 0, 0, 0};
        for (i64 bj = 0; bj < bi; ++bj) {
            __syncthreads();                                     // the tile before is consumed; X[bj] is written and visible
            for (int e = tid; e < kCholNB * kCholNB; e += 256) {
                const int r = e / kCholNB, c = e % kCholNB;
                sL[r * kCholLdM + c] = r < n ? L[(r0 + r) * ldl + bj * kCholNB + c] : 0.0;
                sX[r * kCholLdM + c] = n0 + c < K ? B[(bj * kCholNB + r) * ldb + n0 + c] : 0.0;
            }
            __syncthreads();
            gauss_mfma_tile<false>(sL, sX, acc);
        }
        __syncthreads();
        for (int e = tid; e < kCholNB * kCholNB; e += 256) {
            const int r = e / kCholNB, c = e % kCholNB;
            sL[r * kCholLdM + c] = (r < n && c <= r) ? L[(r0 + r) * ldl + r0 + c] : 0.0;
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int r = wr + 16 * a + ok + 4 * v, c = wc + 16 * b + oi;
                    const double g = (r < n && n0 + c < K) ? B[(r0 + r) * ldb + n0 + c] : 0.0;
                    sX[r * kCholLdM + c] = g - acc[a][b][v];
                }
        __syncthreads();
        if (tid < kCholNB) {
            for (int i = 0; i < n; ++i) {
                double v = sX[i * kCholLdM + tid];
#pragma unroll 8
                for (int c = 0; c < i; ++c) v = fma(-sL[i * kCholLdM + c], sX[c * kCholLdM + tid], v);
                sX[i * kCholLdM + tid] = v / sL[i * kCholLdM + i];
            }
        }
        __syncthreads();
        for (int e = tid; e < kCholNB * kCholNB; e += 256) {
            const int r = e / kCholNB, c = e % kCholNB;
            if (r < n && n0 + c < K) B[(r0 + r) * ldb + n0 + c] = sX[r * kCholLdM + c];
        }
    }
}

// The live gather of a covariance matrix: C[i][j] = (s_i s_j) cov[idx_i][idx_j], + jitter on the diagonal, C [PL][PL].
// With mean_ref (the second sample's launch) also the scaled mean shift d_i = s_i (mean_act - mean_ref)[idx_i], twice:
// the two right-hand sides the solves overwrite.
__global__ __launch_bounds__(256) void k_sym_scale(const double* __restrict__ cov, i64 P, const double* __restrict__ s,
                                                   const int* __restrict__ idx, i64 PL, double jitter, double* __restrict__ C,
                                                   const double* __restrict__ mean_ref, const double* __restrict__ mean_act,
                                                   double* __restrict__ y_ref, double* __restrict__ y_act)
{
#pragma clang fp contract(off)
    const i64 e = (i64)blockIdx.x * 256 + threadIdx.x;
    if (e < PL * PL) {
        const i64 i = e / PL, j = e % PL;
        double v = (s[i] * s[j]) * cov[(i64)idx[i] * P + idx[j]];
        if (i == j) v = v + jitter;
        C[e] = v;
    }
    if (mean_ref && e < PL) {
        const double d = s[e] * (mean_act[idx[e]] - mean_ref[idx[e]]);
        y_ref[e] = d;
        y_act[e] = d;
    }
}

// mean[r] = K + (sum_m (X[r][m] - K)) / M with the pivot K = X[r][0] (0 when that is not finite), the sum in the tree: a
// workgroup per row, 8-byte loads -- the same bits at any alignment of X, and a constant row has the mean K exactly, so
// that its centred draws and its pivot in the factorisation are exactly zero.
__global__ __launch_bounds__(256) void k_row_mean(const double* __restrict__ X, i64 M, double* __restrict__ mean)
{
#pragma clang fp contract(off)
    __shared__ double red[256];
    const double* x = X + (i64)blockIdx.x * M;
    const double K = isfinite(x[0]) ? x[0] : 0.0;
    const double t = gauss_tree_sum(M, [&](i64 m) { return x[m] - K; }, red);
    if (threadIdx.x == 0) mean[blockIdx.x] = K + t / (double)M;
}

// out[r] = sum_c X[r][c]^2 in the tree, a workgroup per row.
__global__ __launch_bounds__(256) void k_row_sumsq(const double* __restrict__ X, i64 cols, i64 ld, double* __restrict__ out,
                                                   const i64* info0, const i64* info1)
{
#pragma clang fp contract(off)
    __shared__ double red[256];
    if (*info0 != 0 || *info1 != 0) return;
    const double* x = X + (i64)blockIdx.x * ld;
    const double t = gauss_tree_sum(cols, [&](i64 c) { const double v = x[c]; return v * v; }, red);
    if (threadIdx.x == 0) out[blockIdx.x] = t;
}

// res[0 .. 3] = |y_ref|^2, |y_act|^2, sum rows_ref, sum rows_act: four tree sums over n terms by one workgroup.  Whatever
// belongs to a failed factor is read as it lies and discarded by the host (gauss_outputs).
__global__ __launch_bounds__(256) void k_gauss_sums(const double* __restrict__ y_ref, const double* __restrict__ y_act,
                                                    const double* __restrict__ rows_ref, const double* __restrict__ rows_act,
                                                    i64 n, double* __restrict__ res)
{
#pragma clang fp contract(off)
    __shared__ double red[256];
    const double a = gauss_tree_sum(n, [&](i64 i) { const double v = y_ref[i]; return v * v; }, red);
    const double b = gauss_tree_sum(n, [&](i64 i) { const double v = y_act[i]; return v * v; }, red);
    const double c = gauss_tree_sum(n, [&](i64 i) { return rows_ref[i]; }, red);
    const double d = gauss_tree_sum(n, [&](i64 i) { return rows_act[i]; }, red);
    if (threadIdx.x == 0) { res[0] = a; res[1] = b; res[2] = c; res[3] = d; }
}

}  // namespace mcr
