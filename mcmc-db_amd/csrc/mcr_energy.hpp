// mcr_energy.hpp -- the energy distance of Szekely and Rizzo between two samples of joint draws,
//     E(X, Y) = 2 E|X - Y| - E|X - X'| - E|Y - Y'|      (V-statistic: the zero diagonals are counted),
// a direction-free, rotation-invariant two-sample statistic without a tuning parameter.  The definition is in
// mcmcref_hip.h; this file has the ONE text of the per-pair arithmetic and of the six outputs, the host routine behind
// mcr_energy_distance_host (plain C++: this part compiles without HIP), and the two kernels.
//
//   u_p(x) = x_p * scale_p (rounded once)       acc = +0.0;  p = 0 .. P-1 in order:  t = u_p(x) - u_p(y),  acc = fma(t, t, acc)
//   d(x, y) = sqrt(acc), correctly rounded
//
// d does not depend on where the pair sits in a tile, a launch or a chunk of parameters; d(x, y) = d(y, x) and
// d(x, x) = +0.0 exactly.  A padded parameter contributes fma(0, 0, acc) = acc: acc is never -0.0.
#pragma once
#include <cmath>
#include <cstdint>
#include <thread>
#include <vector>

namespace mcr {

constexpr int kEnNT = 256;                    // threads of a k_energy_pairs workgroup, a 16 x 16 grid of register blocks
constexpr int kEnTI = 128, kEnTJ = 128;       // draws x draws of a workgroup's tile (MCR_ENERGY_TILE_I / _J)
constexpr int kEnPC = 8;                      // parameters staged in LDS at a time (MCR_ENERGY_CHUNK_P)
constexpr int kEnRB = 8;                      // a thread's block: kEnRB x kEnRB pairs, 64 fp64 accumulators = 128 VGPRs
constexpr long long kEnMaxWork = 1ll << 44;   // pair-parameters of a call (MCR_ENERGY_MAX_WORK)
constexpr long long kEnLaunchWork = 1ll << 38;   // pair-parameters of a launch (MCR_ENERGY_LAUNCH_WORK)
static_assert(kEnTI == 16 * kEnRB && kEnTJ == 16 * kEnRB && kEnNT == 256, "a 16 x 16 grid of kEnRB x kEnRB blocks");

#if defined(__HIPCC__)
#define MCR_EN_HD __host__ __device__
#else
#define MCR_EN_HD
#endif

// Pairs of a call times its parameters, (Mr Ma + Mr (Mr + 1) / 2 + Ma (Ma + 1) / 2) P: what the cost limit is about.
// false: over kEnMaxWork (nothing overflows on the way: the pairs alone are compared first).
inline bool energy_work_ok(long long Mr, long long Ma, long long P)
{
    typedef unsigned __int128 u128;
    const u128 pairs = (u128)Mr * (u128)Ma + (u128)Mr * ((u128)Mr + 1) / 2 + (u128)Ma * ((u128)Ma + 1) / 2;
    return pairs <= (u128)kEnMaxWork && pairs * (u128)P <= (u128)kEnMaxWork;
}

// The tile jobs of a call, in the one order of the partials: the cross tiles (ti over ref, tj over act, tj fastest), then
// the tiles of ref x ref with tj >= ti, then those of act x act.  Row ti of a triangle starts at tri_row(nt, ti).
struct EnergyJobs {
    long long ntr, nta;               // tiles along ref (kEnTI draws) and act
    long long xy, xx, yy;             // jobs of each sum
    MCR_EN_HD long long total() const { return xy + xx + yy; }
};
MCR_EN_HD inline EnergyJobs energy_jobs(long long Mr, long long Ma)
{
    EnergyJobs j;
    j.ntr = (Mr + kEnTI - 1) / kEnTI; j.nta = (Ma + kEnTI - 1) / kEnTI;
    j.xy = j.ntr * j.nta; j.xx = j.ntr * (j.ntr + 1) / 2; j.yy = j.nta * (j.nta + 1) / 2;
    return j;
}
MCR_EN_HD inline long long tri_row(long long nt, long long ti) { return ti * nt - ti * (ti - 1) / 2; }

// Launches of a call and jobs of each but the last: no launch carries more than `budget` pair-parameters, a tile counting
// as kEnTI kEnTJ P whatever part of it lies inside the samples (one tile when the budget is below that); the jobs are
// spread evenly over the fewest launches that respect it.
inline void energy_launches(const EnergyJobs& j, long long P, long long budget, long long& launches, long long& per)
{
    const long long tile = (long long)kEnTI * kEnTJ * P;
    long long cap = budget / tile;
    if (cap < 1) cap = 1;
    if (cap > 0x7FFFFFF8ll) cap = 0x7FFFFFF8ll;          // a one-dimensional grid, padded to a multiple of 8
    launches = (j.total() + cap - 1) / cap;
    per = (j.total() + launches - 1) / launches;
}

// The six outputs from the three pair sums: A, B, C one division each.
MCR_EN_HD inline void energy_outputs(double Sxy, double Sxx, double Syy, long long Mr, long long Ma, double* out)
{
    const double mr = (double)Mr, ma = (double)Ma;
    const double A = Sxy / (mr * ma), B = Sxx / (mr * mr), C = Syy / (ma * ma);
    const double E = (A - B) + (A - C);
    out[0] = A; out[1] = B; out[2] = C; out[3] = E;
    out[4] = A == 0.0 ? 0.0 : E / (2.0 * A);
    out[5] = mr * ma / (mr + ma) * E;
}

// ---- the host routine -------------------------------------------------------------------------------------------------
// u[m][p] = x[p][m] * scale[p] (scale == nullptr: x itself, which is x * 1.0), draw-major so that a pair reads two rows.
inline void energy_scale_host(const double* x, long long M, long long P, const double* scale, std::vector<double>& u)
{
    u.resize((size_t)M * (size_t)P);
    for (long long p = 0; p < P; ++p) {
        const double s = scale ? scale[p] : 1.0;
        for (long long m = 0; m < M; ++m) u[(size_t)m * P + p] = x[(size_t)p * M + m] * s;
    }
}

inline double energy_pair_host(const double* ux, const double* uy, long long P)
{
    double acc = 0.0;
    for (long long p = 0; p < P; ++p) {
        const double t = ux[p] - uy[p];
        acc = std::fma(t, t, acc);
    }
    return std::sqrt(acc);
}

// sum_{i < Mx} sum_{j in J(i)} d(x_i, y_j) in long double, J(i) = [0, My) or, for a within-sample sum (upper), (i, My)
// doubled (the diagonal is +0.0).  Row i is summed for j ascending into four interleaved long double accumulators (j mod
// 4 of the row's own count), joined (0 + 1) + (2 + 3); the rows are added in order.  The threads only share out the
// rows: the result does not depend on their number.
inline long double energy_sum_host(const std::vector<double>& ux, long long Mx, const std::vector<double>& uy, long long My,
                                   long long P, bool upper)
{
    std::vector<long double> row((size_t)Mx);
    unsigned hw = std::thread::hardware_concurrency();
    const int nt = (int)(hw < 1 ? 1 : (hw > 16 ? 16 : hw));
    auto work = [&](int t) {
        double d[256];
        for (long long i = t; i < Mx; i += nt) {
            long double a[4] = {0.0L, 0.0L, 0.0L, 0.0L};
            const double* xi = ux.data() + (size_t)i * P;
            long long k = 0;
            for (long long j0 = upper ? i + 1 : 0; j0 < My; j0 += 256) {
                const int n = (int)(My - j0 < 256 ? My - j0 : 256);
                for (int e = 0; e < n; ++e) d[e] = energy_pair_host(xi, uy.data() + (size_t)(j0 + e) * P, P);
                for (int e = 0; e < n; ++e, ++k) a[k & 3] += (long double)d[e];
            }
            row[(size_t)i] = (a[0] + a[1]) + (a[2] + a[3]);
        }
    };
    if (nt == 1 || Mx * (upper ? My / 2 + 1 : My) * P < (1ll << 16)) {
        for (int t = 0; t < nt; ++t) work(t);
    } else {
        std::vector<std::thread> th;
        for (int t = 0; t < nt; ++t) th.emplace_back(work, t);
        for (std::thread& x : th) x.join();
    }
    long double s = 0.0L;
    for (long long i = 0; i < Mx; ++i) s += row[(size_t)i];
    return upper ? 2.0L * s : s;
}

// 0: out[0..5] written; 1: a bad argument; 2: non-finite draws, or a squared distance (or a sum) that overflows
inline int energy_host(const double* ref, long long Mr, const double* act, long long Ma, long long P, const double* scale,
                       double* out)
{
    if (!ref || !act || !out || Mr < 1 || Ma < 1 || P < 1) return 1;
    for (long long p = 0; scale && p < P; ++p)
        if (!(scale[p] >= 0.0) || std::isinf(scale[p])) return 1;
    if (!energy_work_ok(Mr, Ma, P)) return 1;
    std::vector<double> ur, ua;
    energy_scale_host(ref, Mr, P, scale, ur);
    energy_scale_host(act, Ma, P, scale, ua);
    const double Sxy = (double)energy_sum_host(ur, Mr, ua, Ma, P, false);
    const double Sxx = (double)energy_sum_host(ur, Mr, ur, Mr, P, true);
    const double Syy = (double)energy_sum_host(ua, Ma, ua, Ma, P, true);
    if (!std::isfinite(Sxy) || !std::isfinite(Sxx) || !std::isfinite(Syy)) return 2;
    energy_outputs(Sxy, Sxx, Syy, Mr, Ma, out);
    return 0;
}

}  // namespace mcr

#if defined(__HIPCC__)
#include "mcr_device.hpp"

namespace mcr {

// ------------------------------------------------------------------------------------------------
// k_energy_pairs: one workgroup per tile job (energy_jobs), kEnTI x kEnTJ pairs of draws; all three sums go through the
// one job list.  Thread (ty, tx) = (tid / 16, tid % 16) owns the pairs of rows {32 k + 2 ty, 32 k + 2 ty + 1 : k < 4} with the
// same set of columns from tx: 64 squared-distance accumulators in registers.  The parameters stream through LDS in chunks
// of kEnPC rows [p][draw] per side, scaled ONCE when staged, zero past P.  Per pair-parameter: one subtract, one fma; per
// parameter a thread reads 8 + 8 doubles from LDS for 64 pairs, as eight 16-byte reads -- the kernel is bound by the fp64
// VALU.  The rows' reads are 4 addresses per wave (64 contiguous bytes, broadcast to the 16 lanes of a ty), the columns'
// 16 contiguous 16-byte addresses = all 64 banks once (broadcast to the 4 ty): both conflict-free in every lane group of
// ds_read_b128.  Staging: thread t loads row t / 32 of the chunk, draws 2 (t % 32) and 64 + 2 (t % 32) (+1) of each side:
// 512 contiguous bytes per 32 lanes.  The loads of chunk c + 1 are issued before the arithmetic of chunk c and written to
// the other LDS buffer after it: one barrier per chunk.
// ALIGNED: both samples 16-byte aligned with an even number of draws, so every staged pair is one 16-byte load.  Loads
// are unconditional on addresses clamped into the sample; a lane past the end holds some draw of the sample and its
// pairs are left out of the sum.  After the last chunk every accumulator takes one correctly rounded sqrt, the thread
// adds its 64 in a fixed order (+0.0 for a pair outside), the workgroup adds the threads by a fixed tree:
// partial[job] = the tile's sum, doubled (exactly) for a within-sample tile off the diagonal.  A diagonal tile is
// computed in full and counted once: its own diagonal is +0.0 by the definition.
// grid: jobs of the launch rounded up to a multiple of 8, one-dimensional.  The remap gives every XCD a contiguous range
// of jobs, so that the tiles sharing a band of `ti` draws follow each other on one XCD's L2 (speed only).
// ------------------------------------------------------------------------------------------------
template <bool ALIGNED>
__global__ __launch_bounds__(kEnNT, 2) void k_energy_pairs(const double* __restrict__ ref, i64 Mr,
                                                           const double* __restrict__ act, i64 Ma, i64 P,
                                                           const double* __restrict__ scale, i64 job0, i64 njobs,
                                                           double* __restrict__ partial)
{
    __shared__ __attribute__((aligned(16))) double sA[2][kEnPC][kEnTI];
    __shared__ __attribute__((aligned(16))) double sB[2][kEnPC][kEnTJ];
    __shared__ double red[kEnNT];
    const int tid = threadIdx.x;
    const i64 swz = (i64)(blockIdx.x % 8) * (gridDim.x / 8) + blockIdx.x / 8;      // gridDim.x is a multiple of 8
    if (swz >= njobs) return;
    const i64 g = job0 + swz;
    const EnergyJobs jb = energy_jobs(Mr, Ma);
    // job -> (the two samples, ti, tj)
    const double *A, *B;
    i64 MA, MB, ti, tj;
    bool twice = false;
    if (g < jb.xy) {
        A = ref; MA = Mr; B = act; MB = Ma;
        ti = g / jb.nta; tj = g % jb.nta;
    } else {
        const bool second = g >= jb.xy + jb.xx;
        const i64 k = g - jb.xy - (second ? jb.xx : 0), nt = second ? jb.nta : jb.ntr;
        A = B = second ? act : ref; MA = MB = second ? Ma : Mr;
        const double b = (double)(2 * nt + 1);
        ti = (i64)((b - sqrt(b * b - 8.0 * (double)k)) * 0.5);       // the row of the triangle, then made exact
        if (ti < 0) ti = 0;
        if (ti > nt - 1) ti = nt - 1;
        while (ti + 1 < nt && tri_row(nt, ti + 1) <= k) ++ti;
        while (ti > 0 && tri_row(nt, ti) > k) --ti;
        tj = ti + (k - tri_row(nt, ti));
        twice = tj != ti;
    }
    const i64 i0 = ti * kEnTI, j0 = tj * kEnTJ;

    // staging role: row sr of the chunk, draws sc, sc + 1, 64 + sc, 64 + sc + 1 of each side
    const int sr = tid >> 5, sc = 2 * (tid & 31);
    double2 fa[2], fb[2];
    double fs = 0.0;
    bool fv = false;
    auto fetch = [&](i64 p0) {
        const i64 p = p0 + sr;
        fv = p < P;
        const i64 pr = fv ? p : P - 1;
        fs = scale[pr];
        const double* ra = A + pr * MA;
        const double* rb = B + pr * MB;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const i64 ca = i0 + 64 * h + sc, cb = j0 + 64 * h + sc;
            if constexpr (ALIGNED) {       // M even, ca even: ca < M implies ca + 1 < M; a lane past the end re-reads the last pair
                fa[h] = *reinterpret_cast<const double2*>(ra + (ca < MA ? ca : MA - 2));
                fb[h] = *reinterpret_cast<const double2*>(rb + (cb < MB ? cb : MB - 2));
            } else {
                fa[h].x = ra[ca < MA ? ca : MA - 1]; fa[h].y = ra[ca + 1 < MA ? ca + 1 : MA - 1];
                fb[h].x = rb[cb < MB ? cb : MB - 1]; fb[h].y = rb[cb + 1 < MB ? cb + 1 : MB - 1];
            }
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            double2 a, b;
            a.x = fv ? fa[h].x * fs : 0.0; a.y = fv ? fa[h].y * fs : 0.0;
            b.x = fv ? fb[h].x * fs : 0.0; b.y = fv ? fb[h].y * fs : 0.0;
            *reinterpret_cast<double2*>(&sA[buf][sr][64 * h + sc]) = a;
            *reinterpret_cast<double2*>(&sB[buf][sr][64 * h + sc]) = b;
        }
    };

    const int ty = tid >> 4, tx = tid & 15;
    double acc[kEnRB][kEnRB];
#pragma unroll
    for (int r = 0; r < kEnRB; ++r)
#pragma unroll
        for (int c = 0; c < kEnRB; ++c) acc[r][c] = 0.0;

    const i64 nchunks = (P + kEnPC - 1) / kEnPC;
    fetch(0);
    for (i64 ch = 0; ch < nchunks; ++ch) {
        const int buf = (int)(ch & 1);
        stash(buf);                           // (the readers of this buffer, two chunks back, passed the last barrier)
        __syncthreads();
        if (ch + 1 < nchunks) fetch((ch + 1) * kEnPC);
        const int np = (int)(P - ch * kEnPC < kEnPC ? P - ch * kEnPC : kEnPC);
#pragma unroll 2
        for (int pp = 0; pp < np; ++pp) {
            double a[kEnRB], b[kEnRB];
#pragma unroll
            for (int k = 0; k < kEnRB / 2; ++k) {
                const double2 va = *reinterpret_cast<const double2*>(&sA[buf][pp][32 * k + 2 * ty]);
                const double2 vb = *reinterpret_cast<const double2*>(&sB[buf][pp][32 * k + 2 * tx]);
                a[2 * k] = va.x; a[2 * k + 1] = va.y;
                b[2 * k] = vb.x; b[2 * k + 1] = vb.y;
            }
#pragma unroll
            for (int r = 0; r < kEnRB; ++r)
#pragma unroll
                for (int c = 0; c < kEnRB; ++c) {
                    const double t = a[r] - b[c];
                    acc[r][c] = fma(t, t, acc[r][c]);
                }
        }
    }

    double s = 0.0;
#pragma unroll
    for (int r = 0; r < kEnRB; ++r) {
        const bool vi = i0 + 32 * (r >> 1) + 2 * ty + (r & 1) < MA;
#pragma unroll
        for (int c = 0; c < kEnRB; ++c) {
            const bool vj = j0 + 32 * (c >> 1) + 2 * tx + (c & 1) < MB;
            const double d = __dsqrt_rn(acc[r][c]);
            s += (vi && vj) ? d : 0.0;
        }
    }
    red[tid] = s;
    __syncthreads();
#pragma unroll
    for (int st = kEnNT / 2; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    if (tid == 0) partial[g] = twice ? 2.0 * red[0] : red[0];
}

// ------------------------------------------------------------------------------------------------
// k_energy_reduce: one workgroup.  Each of the three ranges of partials (jobs.xy, .xx, .yy, in this order) is summed by
// thread t over partial[t], partial[t + 256], .. in order, the threads by the same fixed tree:
// res[0..5] = the six outputs, res[6..8] = S_xy, S_xx, S_yy (the host looks at these for a non-finite value).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kEnNT) void k_energy_reduce(const double* __restrict__ partial, i64 Mr, i64 Ma,
                                                         double* __restrict__ res)
{
    __shared__ double red[kEnNT];
    __shared__ double S[3];
    const int tid = threadIdx.x;
    const EnergyJobs jb = energy_jobs(Mr, Ma);
    const i64 lo[3] = {0, jb.xy, jb.xy + jb.xx}, hi[3] = {jb.xy, jb.xy + jb.xx, jb.total()};
    for (int q = 0; q < 3; ++q) {
        double s = 0.0;
        for (i64 e = lo[q] + tid; e < hi[q]; e += kEnNT) s += partial[e];
        red[tid] = s;
        __syncthreads();
        for (int st = kEnNT / 2; st > 0; st >>= 1) {
            if (tid < st) red[tid] += red[tid + st];
            __syncthreads();
        }
        if (tid == 0) S[q] = red[0];
        __syncthreads();
    }
    if (tid == 0) {
        energy_outputs(S[0], S[1], S[2], Mr, Ma, res);
        res[6] = S[0]; res[7] = S[1]; res[8] = S[2];
    }
}

}  // namespace mcr
#endif  // __HIPCC__
