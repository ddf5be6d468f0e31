// mcr_stats.hip -- the statistics unit of libmcmcref_hip.so's C ABI (see include/mcmcref_hip.h) beside the summary:
// two-sample and sliced KS / W1, the energy distance, and the calls on one draw tensor -- nested R-hat, Pareto k-hat, PSIS,
// HDI, weighted summaries, SBC, autocorrelation -- and covariance, each with its plan, device, host-upload and *_host
// entries; and the extension entries of include/mcmcref_hip_ext.h (mcrx_*: Cholesky, lower solve, Gaussian check).  What they use of the summary pipeline of mcr_api.hip is mcr_pipe.hpp; no kernel of that unit is launched here.
#include "mcr_pipe.hpp"

#include <cmath>
#include <cstring>
#include <exception>
#include <unordered_map>

#include "mcr_ext.hpp"
#include "mcr_energy.hpp"
#include "mcr_nested.hpp"
#include "mcr_acf.hpp"
#include "mcr_pareto.hpp"
#include "mcr_psis.hpp"
#include "mcr_hdi.hpp"
#include "mcr_weighted.hpp"
#include "mcr_sbc.hpp"
#include "mcr_gauss.hpp"
#include "../../include/mcmcref_hip_ext.h"

using namespace mcr;
using namespace mcr::host;

extern "C" {

// The workspace of a two-sample pass over P rows: the two samples, the parked sorted reference, the merge partials, the
// results, the non-finite counts, then the two sorts one after the other in the same space.
struct TwoSampleWs {
    double *Xr, *Xa, *Sr, *part, *d_ks, *d_w, *bad;
    PipeIn ar{}, aa{};
    int nblk;
};

static void carve_two_sample(Carve& cv, TwoSampleWs& t, i64 P, i64 Mr, i64 Ma)
{
    t.nblk = (int)((Mr + Ma + kTile - 1) / kTile);
    t.ar.M = Mr; t.aa.M = Ma;
    t.ar.pc = t.aa.pc = P; t.ar.C = t.aa.C = 1; t.ar.do_diag = t.aa.do_diag = false;
    t.Xr = cv.take<double>((size_t)P * Mr);
    t.Xa = cv.take<double>((size_t)P * Ma);
    t.Sr = cv.take<double>((size_t)P * Mr);
    t.part = cv.take<double>((size_t)P * t.nblk * 2);
    t.d_ks = cv.take<double>((size_t)P);
    t.d_w = cv.take<double>((size_t)P);
    t.bad = cv.take<double>((size_t)P * 2);
    const size_t base = cv.off;
    carve_pipe(cv, t.ar, false, FftPlan{}, false);
    const size_t end_r = cv.off;
    cv.off = base;
    carve_pipe(cv, t.aa, false, FftPlan{}, false);
    if (end_r > cv.off) cv.off = end_r;
}

// From the rows t.Xr [P][Mr], t.Xa [P][Ma] on the device to ks[P], w1[P] on the host: the two sorts, the non-finite
// counts, one merge-path pass, the finisher and the non-finite check (`what` names the rows in its message).  Synchronous.
static int two_sample_tail(mcr_ctx* ctx, TwoSampleWs& t, i64 P, double* ks, double* w1, const char* what)
{
    const i64 Mr = t.ar.M, Ma = t.aa.M;
    const int nblk = t.nblk;
    Sorted so;
    t.ar.X = t.Xr;                // ascending order of the reference sample, parked in Sr
    int rc = sort_stage(ctx, t.ar, so);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(t.Sr, so.keys, sizeof(double) * (size_t)P * Mr, hipMemcpyDeviceToDevice, ctx->stream));
    hipLaunchKernelGGL(k_bad_count, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)t.ar.part,
                       (int)t.ar.ntiles, (i64)P, t.bad);
    t.aa.X = t.Xa;                // ascending order of the actual sample, then one merge-path pass over both
    rc = sort_stage(ctx, t.aa, so);
    if (rc) return rc;
    hipLaunchKernelGGL(k_bad_count, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)t.aa.part,
                       (int)t.aa.ntiles, (i64)P, t.bad + P);
    LAUNCH(ctx, K_TWO_SAMPLE, (k_two_sample<256, 16>), dim3((unsigned)nblk, (unsigned)P), dim3(256), 0,
           (const double*)t.Sr, (i64)Mr, (const double*)so.keys, (i64)Ma, t.part, nblk);
    LAUNCH(ctx, K_TWO_SAMPLE, k_two_sample_final, dim3((unsigned)((P + 255) / 256)), dim3(256), 0,
           (const double*)t.part, nblk, (i64)P, (double)Mr * (double)Ma, t.d_ks, t.d_w);
    HIP_TRY(ctx, hipMemcpyAsync(ks, t.d_ks, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(w1, t.d_w, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<double> h_bad((size_t)2 * (size_t)P);
    HIP_TRY(ctx, hipMemcpyAsync(h_bad.data(), t.bad, sizeof(double) * h_bad.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    for (i64 p = 0; p < P; ++p)
        if (h_bad[(size_t)p] != 0.0 || h_bad[(size_t)(P + p)] != 0.0 || !(ks[p] == ks[p]) || !(w1[p] == w1[p]) || std::isinf(w1[p]))
            return fail(ctx, MCR_ENONFINITE, "%s contain non-finite values", what);
    return MCR_OK;
}

// The length limits of a two-sample pass (positions are 32-bit; the KS numerator must stay exact in f64).
static bool two_sample_too_long(i64 Mr, i64 Ma)
{
    return Mr >= (i64)0xFFFFFFFFll || Ma >= (i64)0xFFFFFFFFll || (double)Mr * (double)Ma >= 9007199254740992.0;
}

int mcr_two_sample(mcr_ctx* ctx, const double* ref, int64_t Mr, const double* act, int64_t Ma, int64_t P,
                   double* ks, double* w1)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (P < 0 || Mr < 1 || Ma < 1 || (P > 0 && (!ref || !act || !ks || !w1)))
        return fail(ctx, MCR_EINVAL, "bad argument (both samples need at least one draw)");
    if (P == 0) return MCR_OK;
    if (P > kMaxGridY) return fail(ctx, MCR_EINVAL, "P > %d", kMaxGridY);
    if (two_sample_too_long(Mr, Ma)) return fail(ctx, MCR_EINVAL, "samples too long (Mr * Ma must stay below 2^53)");
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "mcr_two_sample with summaries in flight");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    TwoSampleWs t;
    const int rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) { carve_two_sample(cv, t, P, Mr, Ma); });
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(t.Xr, ref, sizeof(double) * (size_t)P * Mr, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(t.Xa, act, sizeof(double) * (size_t)P * Ma, hipMemcpyHostToDevice, ctx->stream));
    return two_sample_tail(ctx, t, P, ks, w1, "draws");
}

// One k_project launch: Z[K][M] = W[K][P] (X[P][M] - c[P]).  The 16-byte instance when every row of X and Z starts
// 16-byte aligned; both instances give the same bits.
static int launch_project(mcr_ctx* ctx, const double* X, const double* W, const double* c, i64 M, i64 P, i64 K, double* Z)
{
    const i64 mtiles = ((M + kProjTileM - 1) / kProjTileM + 7) / 8 * 8, ktiles = (K + kProjTileK - 1) / kProjTileK;
    if (mtiles * ktiles > 0x7FFFFFFFll) return fail(ctx, MCR_EINVAL, "too many draws x directions for one projection launch");
    const dim3 grid((unsigned)(mtiles * ktiles));
    if ((M & 1) == 0 && ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Z)) & 15) == 0)
        LAUNCH(ctx, K_PROJECT, (k_project<true>), grid, dim3(kProjNT), 0, X, W, c, M, P, K, Z);
    else
        LAUNCH(ctx, K_PROJECT, (k_project<false>), grid, dim3(kProjNT), 0, X, W, c, M, P, K, Z);
    return MCR_OK;
}

// The workspace of kc directions of a sliced call: the two-sample workspace over kc rows (its Xr / Xa are the
// projections), the chunk's directions and the center.
struct SlicedWs { TwoSampleWs t; double *W, *c; };

static void carve_sliced(Carve& cv, SlicedWs& s, i64 kc, i64 Mr, i64 Ma, i64 P)
{
    carve_two_sample(cv, s.t, kc, Mr, Ma);
    s.W = cv.take<double>((size_t)kc * P);
    s.c = cv.take<double>((size_t)P);
}

// Directions per workspace chunk: the most whose workspace fits the limit (all K when they fit at once).
static int plan_sliced(mcr_ctx* ctx, i64 Mr, i64 Ma, i64 P, i64 K, i64& kc)
{
    auto measure = [&](i64 k) { Carve m{nullptr}; SlicedWs s; carve_sliced(m, s, k, Mr, Ma, P); return m.off; };
    const i64 Mmax = Mr > Ma ? Mr : Ma;                // k_project's one-dimensional grid: draw tiles x direction tiles < 2^31
    const i64 grid_cap = 0x7FFFFFFFll / (((Mmax + kProjTileM - 1) / kProjTileM + 7) / 8 * 8) * kProjTileK;
    if (K > grid_cap) K = grid_cap;
    kc = most_that_fit(K, [&](i64 k) { return measure(k) <= ctx->ws_limit; });
    if (!kc)
        return fail(ctx, MCR_ENOMEM, "workspace limit too small: one direction needs %zu bytes, the limit is %zu", measure(1),
                    ctx->ws_limit);
    return MCR_OK;
}

static int sliced_check(mcr_ctx* ctx, const void* ref, i64 Mr, const void* act, i64 Ma, i64 P, const double* dirs,
                 const double* center, i64 K, const double* ks, const double* w1)
{
    if (K < 0 || Mr < 1 || Ma < 1 || (K > 0 && (P < 1 || !ref || !act || !dirs || !ks || !w1)))
        return fail(ctx, MCR_EINVAL, "bad argument (both samples need at least one draw and one parameter)");
    if (K == 0) return MCR_OK;
    if (K > kMaxGridY) return fail(ctx, MCR_EINVAL, "K > %d", kMaxGridY);
    if (two_sample_too_long(Mr, Ma)) return fail(ctx, MCR_EINVAL, "samples too long (Mr * Ma must stay below 2^53)");
    for (i64 i = 0; i < K * P; ++i)
        if (!std::isfinite(dirs[i])) return fail(ctx, MCR_EINVAL, "direction %lld has a non-finite weight", (long long)(i / P));
    for (i64 p = 0; center && p < P; ++p)
        if (!std::isfinite(center[p])) return fail(ctx, MCR_EINVAL, "center[%lld] is not finite", (long long)p);
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "mcr_sliced_two_sample with summaries in flight");
    return MCR_OK;
}

static_assert(kProjTileM == MCR_PROJ_TILE_M && kProjTileK == MCR_PROJ_TILE_K && kProjChunkP == MCR_PROJ_CHUNK_P,
              "mcmcref_hip.h states k_project's geometry");

int mcr_sliced_plan(mcr_ctx* ctx, int64_t Mr, int64_t Ma, int64_t P, int64_t K, int64_t* dirs_per_chunk)
{
    if (!ctx || !dirs_per_chunk) return fail(ctx, MCR_EINVAL, "mcr_sliced_plan: NULL argument");
    if (Mr < 1 || Ma < 1 || P < 1 || K < 1 || K > kMaxGridY) { *dirs_per_chunk = 0; return MCR_OK; }
    i64 kc = 0;
    const int rc = plan_sliced(ctx, Mr, Ma, P, K, kc);
    if (rc) return rc;
    *dirs_per_chunk = kc;
    return MCR_OK;
}

int mcr_sliced_two_sample_dev(mcr_ctx* ctx, const double* ref_dev, int64_t Mr, const double* act_dev, int64_t Ma, int64_t P,
                              const double* dirs, const double* center, int64_t K, double* ks, double* w1,
                              double* proj_ref, double* proj_act)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    int rc = sliced_check(ctx, ref_dev, Mr, act_dev, Ma, P, dirs, center, K, ks, w1);
    if (rc || K == 0) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    i64 kcmax = 0;
    rc = plan_sliced(ctx, Mr, Ma, P, K, kcmax);
    if (rc) return rc;
    const std::vector<double> zeros(center ? 0 : (size_t)P, 0.0);
    for (i64 k0 = 0; k0 < K; k0 += kcmax) {            // the directions are independent: chunking changes no bit
        const i64 kc = K - k0 < kcmax ? K - k0 : kcmax;
        SlicedWs s;
        rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) { carve_sliced(cv, s, kc, Mr, Ma, P); });
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(s.W, dirs + k0 * P, sizeof(double) * (size_t)kc * P, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(s.c, center ? center : zeros.data(), sizeof(double) * (size_t)P, hipMemcpyHostToDevice,
                                    ctx->stream));
        rc = launch_project(ctx, ref_dev, s.W, s.c, Mr, P, kc, s.t.Xr);
        if (!rc) rc = launch_project(ctx, act_dev, s.W, s.c, Ma, P, kc, s.t.Xa);
        if (rc) return rc;
        if (proj_ref)
            HIP_TRY(ctx, hipMemcpyAsync(proj_ref + k0 * Mr, s.t.Xr, sizeof(double) * (size_t)kc * Mr, hipMemcpyDeviceToHost, ctx->stream));
        if (proj_act)
            HIP_TRY(ctx, hipMemcpyAsync(proj_act + k0 * Ma, s.t.Xa, sizeof(double) * (size_t)kc * Ma, hipMemcpyDeviceToHost, ctx->stream));
        rc = two_sample_tail(ctx, s.t, kc, ks + k0, w1 + k0, "draws or their projections");
        if (rc) return rc;
    }
    return MCR_OK;
}

int mcr_sliced_two_sample(mcr_ctx* ctx, const double* ref, int64_t Mr, const double* act, int64_t Ma, int64_t P,
                          const double* dirs, const double* center, int64_t K, double* ks, double* w1,
                          double* proj_ref, double* proj_act)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    int rc = sliced_check(ctx, ref, Mr, act, Ma, P, dirs, center, K, ks, w1);
    if (rc || K == 0) return rc;
    const double *Xr, *Xa;
    rc = stage_two_samples(ctx, ref, Mr, act, Ma, P, &Xr, &Xa);
    if (rc) return rc;
    return mcr_sliced_two_sample_dev(ctx, Xr, Mr, Xa, Ma, P, dirs, center, K, ks, w1, proj_ref, proj_act);
}

// ---- energy distance (mcr_energy.hpp) ---------------------------------------------------------------------------------
static_assert(kEnTI == MCR_ENERGY_TILE_I && kEnTJ == MCR_ENERGY_TILE_J && kEnPC == MCR_ENERGY_CHUNK_P &&
              kEnMaxWork == MCR_ENERGY_MAX_WORK && kEnLaunchWork == MCR_ENERGY_LAUNCH_WORK,
              "mcmcref_hip.h states k_energy_pairs' geometry and the work limits");

// The workspace of a call: one partial per tile job, the scales, the results (six outputs + the three sums).
struct EnergyWs { double *part, *scale, *res; };

static void carve_energy(Carve& cv, EnergyWs& w, const EnergyJobs& jb, i64 P)
{
    w.part = cv.take<double>((size_t)jb.total());
    w.scale = cv.take<double>((size_t)P);
    w.res = cv.take<double>(9);
}

// The shape of a call: MCR_EINVAL with the cause, else MCR_OK.
static int energy_shape_check(mcr_ctx* ctx, i64 Mr, i64 Ma, i64 P)
{
    if (Mr < 1 || Ma < 1) return fail(ctx, MCR_EINVAL, "mcr_energy_distance: both samples need at least one draw (Mr = %lld, Ma = %lld)", Mr, Ma);
    if (P < 1) return fail(ctx, MCR_EINVAL, "mcr_energy_distance: P = %lld, at least one parameter is needed", P);
    if (!energy_work_ok(Mr, Ma, P))
        return fail(ctx, MCR_EINVAL, "mcr_energy_distance: (Mr Ma + Mr (Mr + 1) / 2 + Ma (Ma + 1) / 2) P is over the work limit "
                    "MCR_ENERGY_MAX_WORK = %lld pair-parameters (Mr = %lld, Ma = %lld, P = %lld): thin the samples", kEnMaxWork, Mr, Ma, P);
    return MCR_OK;
}

static int energy_check(mcr_ctx* ctx, const void* ref, i64 Mr, const void* act, i64 Ma, i64 P, const double* scale, const double* out)
{
    if (!ref || !act || !out) return fail(ctx, MCR_EINVAL, "mcr_energy_distance: NULL argument (%s)", !ref ? "ref" : !act ? "act" : "out");
    const int rc = energy_shape_check(ctx, Mr, Ma, P);
    if (rc) return rc;
    for (i64 p = 0; scale && p < P; ++p)
        if (!(scale[p] >= 0.0) || std::isinf(scale[p]))
            return fail(ctx, MCR_EINVAL, "mcr_energy_distance: scale[%lld] is negative or not finite", (long long)p);
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "mcr_energy_distance with summaries in flight");
    return MCR_OK;
}

int mcr_energy_workspace(mcr_ctx* ctx, int64_t Mr, int64_t Ma, int64_t P, size_t* bytes)
{
    if (!ctx || !bytes) return fail(ctx, MCR_EINVAL, "mcr_energy_workspace: NULL argument");
    const int rc = energy_shape_check(ctx, Mr, Ma, P);
    if (rc) return rc;
    Carve m{nullptr};
    EnergyWs w;
    carve_energy(m, w, energy_jobs(Mr, Ma), P);
    *bytes = m.off;
    return MCR_OK;
}

int mcr_energy_distance_dev(mcr_ctx* ctx, const double* ref_dev, int64_t Mr, const double* act_dev, int64_t Ma, int64_t P,
                            const double* scale, double* out)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    int rc = energy_check(ctx, ref_dev, Mr, act_dev, Ma, P, scale, out);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const EnergyJobs jb = energy_jobs(Mr, Ma);
    EnergyWs w;
    { Carve m{nullptr}; carve_energy(m, w, jb, P);
      if (m.off > ctx->ws_limit)
          return fail(ctx, MCR_ENOMEM, "workspace limit too small: the energy distance of this shape needs %zu bytes, the limit is %zu",
                      m.off, ctx->ws_limit); }
    rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) { carve_energy(cv, w, jb, P); });
    if (rc) return rc;
    const std::vector<double> ones(scale ? 0 : (size_t)P, 1.0);            // x * 1.0 is x: one kernel text for both
    HIP_TRY(ctx, hipMemcpyAsync(w.scale, scale ? scale : ones.data(), sizeof(double) * (size_t)P, hipMemcpyHostToDevice, ctx->stream));
    const bool aligned = ((Mr | Ma) & 1) == 0 &&
                         ((reinterpret_cast<uintptr_t>(ref_dev) | reinterpret_cast<uintptr_t>(act_dev)) & 15) == 0;
    i64 launches = 0, per = 0;
    energy_launches(jb, P, ctx->energy_launch_work, launches, per);
    for (i64 l = 0; l < launches; ++l) {                 // a partial per job: how the jobs are cut into launches changes no bit
        const i64 job0 = l * per, n = jb.total() - job0 < per ? jb.total() - job0 : per;
        const dim3 grid((unsigned)((n + 7) / 8 * 8));
        if (aligned)
            LAUNCH(ctx, K_ENERGY_PAIRS, (k_energy_pairs<true>), grid, dim3(kEnNT), 0, ref_dev, (i64)Mr, act_dev, (i64)Ma, (i64)P,
                   (const double*)w.scale, job0, n, w.part);
        else
            LAUNCH(ctx, K_ENERGY_PAIRS, (k_energy_pairs<false>), grid, dim3(kEnNT), 0, ref_dev, (i64)Mr, act_dev, (i64)Ma, (i64)P,
                   (const double*)w.scale, job0, n, w.part);
    }
    LAUNCH(ctx, K_ENERGY_REDUCE, k_energy_reduce, dim3(1), dim3(kEnNT), 0, (const double*)w.part, (i64)Mr, (i64)Ma, w.res);
    double res[9];
    HIP_TRY(ctx, hipMemcpyAsync(res, w.res, sizeof(res), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    if (!std::isfinite(res[6]) || !std::isfinite(res[7]) || !std::isfinite(res[8]))
        return fail(ctx, MCR_ENONFINITE, "draws contain non-finite values, or a squared distance overflows");
    memcpy(out, res, 6 * sizeof(double));
    return MCR_OK;
}

int mcr_energy_distance(mcr_ctx* ctx, const double* ref, int64_t Mr, const double* act, int64_t Ma, int64_t P,
                        const double* scale, double* out)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    int rc = energy_check(ctx, ref, Mr, act, Ma, P, scale, out);
    if (rc) return rc;
    const double *Xr, *Xa;
    rc = stage_two_samples(ctx, ref, Mr, act, Ma, P, &Xr, &Xa);
    if (rc) return rc;
    return mcr_energy_distance_dev(ctx, Xr, Mr, Xa, Ma, P, scale, out);
}

int mcr_energy_distance_host(const double* ref, int64_t Mr, const double* act, int64_t Ma, int64_t P, const double* scale,
                             double* out)
{
    try {
        const int rc = energy_host(ref, Mr, act, Ma, P, scale, out);
        return rc == 0 ? MCR_OK : rc == 1 ? MCR_EINVAL : MCR_ENONFINITE;
    } catch (const std::exception&) {
        return MCR_ENOMEM;
    }
}

}  // extern "C"

// ---- Calls on the pooled ascending order, and the other calls on one draw tensor ------------------------------------------
// Nested R-hat, Pareto k-hat, PSIS, HDI and autocorrelation each take one (C, N, P) tensor, run synchronously and cut its
// parameters into chunks under the workspace limit.  What that takes is here, once: the tensor and its acceptance
// (Tensor, pooled_check), the entry and the plan entry (tensor_entry, plan_entry), the chunk size and the chunk loop
// (plan_params, tensor_chunks) and the context's two call buffers (call_table, pooled_results).  Pareto k-hat, PSIS and HDI
// run the summary pipeline without diagnostics and quantiles -- tile sort, merges / bucket partition, k_order_stats,
// k_finalize for the non-finite count -- and then their own kernels on the keys the sort stage left (pooled_chunks); the
// two with tails share tail_check and tail_lds.  A family below supplies its own arguments' check, its chunk's layout,
// its launches and the scatter of its results, and nothing else.  Simulation-based calibration takes S such tensors (the
// Tensor's fourth axis) through the same entry and cuts its SIMULATIONS into chunks, where it needs the ingest copy at all.
namespace {

struct Tensor {
    const void* draws; int dtype; i64 C, N, P, sc, sn, sp;
    i64 S = 1, ss = 0;   // the fourth axis (mcr_sbc_ranks): S such tensors, each ss elements behind the one before
    i64 M() const { return C * N; }
    i64 extent() const
    {
        const i64 e = tensor_extent(C, N, P, sc, sn, sp);
        if (S < 1 || e <= 0) return S < 1 ? 0 : e;
        return ss < 0 ? -1 : (S - 1) * ss + e;
    }
    // f32 draws are widened by the ingest pass: the answer is the f64 call's on the widened tensor
    bool ingest() const { return dtype == MCR_F32 || needs_ingest(C, N, P, sc, sn, sp) || (S > 1 && ss != P * M()); }
};

// Acceptance of the tensor of such a call (`what` names the entry in the message).
int pooled_check(mcr_ctx* ctx, const char* what, const Tensor& t, const void* out)
{
    if (!out) return fail(ctx, MCR_EINVAL, "out is NULL");
    if (t.dtype != MCR_F64 && t.dtype != MCR_F32) return fail(ctx, MCR_EINVAL, "unsupported dtype %d", t.dtype);
    if (t.C < 0 || t.N < 0 || t.P < 0) return fail(ctx, MCR_EINVAL, "negative dimension (C=%lld N=%lld P=%lld)", (long long)t.C, (long long)t.N, (long long)t.P);
    if (t.N > 0 && (t.C > (i64)0x7FFFFFFFll / t.N || t.M() >= (i64)0x7FFFFFFFll)) return fail(ctx, MCR_EINVAL, "C*N must be < 2^31 - 1");
    if (!t.draws && t.S != 0 && t.M() * t.P > 0) return fail(ctx, MCR_EINVAL, "draws is NULL");   // (S == 0: nothing to read)
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "%s with summaries in flight", what);
    return MCR_OK;
}

// A host entry's upload: the tensor's extent (> 0) into ctx->stage; t.draws becomes the device copy.
int pooled_upload(mcr_ctx* ctx, Tensor& t)
{
    const size_t bytes = (size_t)t.extent() * (t.dtype == MCR_F64 ? 8 : 4);
    void* X = nullptr;
    const int rc = stage_buffers(ctx, {bytes}, &X);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(X, t.draws, bytes, hipMemcpyHostToDevice, ctx->stream));
    t.draws = X;
    return MCR_OK;
}

// An entry of such a call, the host's (the draws are uploaded) or the device's.  check(): the call's own arguments,
// once, behind the tensor's acceptance: every refusal comes before anything is uploaded or written.  empty(): the
// results of a tensor without draws (it has no extent: nothing is uploaded, and its strides are not looked at).
// run(t): the call on the tensor in device memory.
template <class Check, class Empty, class Run>
int tensor_entry(mcr_ctx* ctx, const char* what, Tensor t, const void* out, bool host, Check&& check, Empty&& empty, Run&& run)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    int rc = pooled_check(ctx, what, t, out);
    if (!rc) rc = check();
    if (rc || t.P == 0 || t.S == 0) return rc;
    if (t.M() == 0) { empty(); return MCR_OK; }
    if (t.extent() < 0) return fail(ctx, MCR_EINVAL, "negative strides are not supported");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (host && (rc = pooled_upload(ctx, t))) return rc;
    rc = run(t);
    return rc ? drain(ctx, rc, true) : rc;
}

// Parameters per workspace chunk: the most, up to P and to cap (what the launches' grids hold), whose layout fits the
// workspace limit.  layout(cv, pc) carves a chunk of pc parameters.
template <class Layout>
int plan_params(mcr_ctx* ctx, i64 P, i64 cap, Layout&& layout, i64& pcmax)
{
    auto measure = [&](i64 pc) { Carve m{nullptr}; layout(m, pc); return m.off; };
    pcmax = most_that_fit(P < cap ? P : cap, [&](i64 pc) { return measure(pc) <= ctx->ws_limit; });
    if (!pcmax) return fail(ctx, MCR_ENOMEM, "one parameter needs %zu bytes of workspace; limit is %zu", measure(1), ctx->ws_limit);
    return MCR_OK;
}

// An mcr_*_plan entry: 0 for a shape no call runs on (empty, or one pooled_check refuses), else what plan(pcmax) --
// the call's own argument check where it has one, then its plan_params -- answers (0 when it leaves pcmax alone).
template <class Plan>
int plan_entry(mcr_ctx* ctx, const char* what, const Tensor& t, int64_t* params_per_chunk, Plan&& plan)
{
    if (!ctx || !params_per_chunk) return fail(ctx, MCR_EINVAL, "%s: NULL argument", what);
    i64 pcmax = 0;
    if (t.C >= 1 && t.N >= 1 && t.P >= 1 && t.C <= (i64)0x7FFFFFFFll / t.N && t.M() < (i64)0x7FFFFFFFll) {
        const int rc = plan(pcmax);
        if (rc) return rc;
    }
    *params_per_chunk = pcmax;
    return MCR_OK;
}

// The chunks of a call: per chunk of at most pcmax parameters its workspace -- layout(cv, pc), as in plan_params,
// returns the chunk's ingest copy -- the ingest pass where the tensor needs one, then body(pc, p0, X): the call's launches
// on the chunk's f64 draws X[pc][M], the copy or the user's tensor at parameter p0.
template <class Layout, class Body>
int tensor_chunks(mcr_ctx* ctx, const Tensor& t, i64 pcmax, Layout&& layout, Body&& body)
{
    const bool ingest = t.ingest();
    for (i64 p0 = 0; p0 < t.P; p0 += pcmax) {
        const i64 pc = (t.P - p0 < pcmax) ? t.P - p0 : pcmax;
        double* copy = nullptr;
        int rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) { copy = layout(cv, pc); });
        if (!rc && ingest) rc = launch_ingest(ctx, t.draws, t.dtype, copy, t.C, t.N, pc, t.sc, t.sn, t.sp, p0);   // (one tensor: z = 1)
        if (!rc) rc = body(pc, p0, ingest ? copy : reinterpret_cast<const double*>(t.draws) + p0 * t.M());
        if (rc) return rc;
    }
    return MCR_OK;
}

// The call-level device table (the context's, shared by these calls): `head` -- a call's tail lengths, its chain
// permutation -- uploaded, and behind it the result rows.
template <typename T>
int call_table(mcr_ctx* ctx, const std::vector<T>& head, size_t res_doubles, T*& d_head, double*& d_res)
{
    const int rc = carve(ctx, ctx->call_dev, [&](Carve& cv) { d_head = cv.take<T>(head.size()); d_res = cv.take<double>(res_doubles); });
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_head, head.data(), sizeof(T) * head.size(), hipMemcpyHostToDevice, ctx->stream));
    return MCR_OK;
}

// The one D2H of the result table at the end of a call whose chunks ran the pipeline; each(r, pc, p0, p): the rows r of
// the chunk at p0, parameter p of its pc.  MCR_ENONFINITE when the pipeline counted a NaN or Inf draw (the outputs are
// written all the same).
template <class Each>
int pooled_results(mcr_ctx* ctx, const double* d_res, int fields, i64 P, i64 pcmax, Each&& each)
{
    const size_t bytes = sizeof(double) * (size_t)fields * (size_t)P;
    const int rc = ctx->call_host.reserve(ctx, bytes);
    if (rc) return rc;
    const double* h = ctx->call_host.as<double>();
    HIP_TRY(ctx, hipMemcpyAsync(ctx->call_host.p, d_res, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    double nbad = 0.0;
    for (i64 at = 0; at < P; ++at) {
        const i64 p = at % pcmax, p0 = at - p, pc = (P - p0 < pcmax) ? P - p0 : pcmax;
        const double* r = h + (size_t)fields * (size_t)p0;
        nbad += r[(size_t)R_BAD * pc + p];
        each(r, pc, p0, p);
    }
    if (nbad > 0.0) return fail(ctx, MCR_ENONFINITE, "draws contain %.0f non-finite value(s)", nbad);
    return MCR_OK;
}

constexpr int kPoolField0 = R_Q0;                          // the pipeline runs without quantiles: its rows end here

// The pipeline on pc parameters of one chain of M pooled draws, without quantiles; do_diag: with the rank codes.
PipeIn one_chain_pipe(i64 M, i64 pc, bool do_diag)
{
    PipeIn a{};
    a.M = M; a.pc = pc; a.C = 1; a.n = 1; a.nh = 0; a.nstage = 1; a.q.nq = 0; a.do_diag = do_diag;
    return a;
}

// The layout of a stats-only chunk, into a: the sort alone and the split points k_order_stats writes, then extra(cv, a):
// what the caller needs behind the pipeline's buffers.
template <class Extra>
auto pooled_layout(const Tensor& t, PipeIn& a, Extra& extra)
{
    return [&](Carve& cv, i64 pc) {
        a = one_chain_pipe(t.M(), pc, false);
        double* X = carve_pipe(cv, a, false, FftPlan{}, t.ingest());
        a.split = cv.take<i64>((size_t)pc);
        extra(cv, a);
        return X;
    };
}

// Parameters per workspace chunk of a call on the pooled order; grid_hi: what its own kernels' grids hold.
template <class Extra>
int plan_pooled(mcr_ctx* ctx, const Tensor& t, Extra&& extra, i64& pcmax, i64 grid_hi = kMaxGridY / 2)
{
    PipeIn a{};
    return plan_params(ctx, t.P, grid_hi < kMaxGridY / 2 ? grid_hi : kMaxGridY / 2, pooled_layout(t, a, extra), pcmax);
}

// The chunks of such a call: the stats-only pipeline into the chunk's rows d_res + fields * p0, then after(a, so, p0):
// the caller's kernels on the chunk's keys.
template <class Extra, class After>
int pooled_chunks(mcr_ctx* ctx, const Tensor& t, i64 pcmax, int fields, double* d_res, Extra&& extra, After&& after)
{
    PipeIn a{};
    return tensor_chunks(ctx, t, pcmax, pooled_layout(t, a, extra), [&](i64, i64 p0, const double* X) {
        a.X = X;
        a.d_res = d_res + (size_t)fields * (size_t)p0;
        Sorted so;
        const int rc = run_pipeline(ctx, a, &so);          // sort, order statistics, finalize (the bad count)
        return rc ? rc : after(a, so, p0);
    });
}

// A caller's tail length of parameter p, where it gives any.
int tail_check(mcr_ctx* ctx, const int64_t* ndraws_tail, i64 p)
{
    if (ndraws_tail && ndraws_tail[p] < 1)
        return fail(ctx, MCR_EINVAL, "ndraws_tail[%lld] = %lld: a tail length must be >= 1", (long long)p, (long long)ndraws_tail[p]);
    return MCR_OK;
}

// The dynamic LDS of a tail kernel on the chunk [p0, p0 + pc): `base` doubles and the chunk's longest tail that is staged
// there.  Above 60 KB the kernel is told.
int tail_lds(mcr_ctx* ctx, const std::vector<i64>& teff, i64 p0, i64 pc, size_t base, const void* kernel, size_t& lds)
{
    i64 tmax = 0;
    for (i64 p = p0; p < p0 + pc; ++p)
        if (teff[(size_t)p] <= kParetoLdsTail && teff[(size_t)p] > tmax) tmax = teff[(size_t)p];
    lds = sizeof(double) * (base + (size_t)tmax);
    if (lds > 60 * 1024) HIP_TRY(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return MCR_OK;
}

}  // namespace

extern "C" {

// ---- nested R-hat (mcr_nested.hpp) ------------------------------------------------------------------------------------
constexpr i64 kMaxNestedChains = (i64)1 << 20;
constexpr int kNestKinds = 3;                              // raw, bulk, tail
constexpr int kNestField0 = kPoolField0;
constexpr int kNestFields = kNestField0 + 3 * kNestKinds;  // + (nrhat, B, W) per kind

static_assert(kMaxNestedChains == MCR_NESTED_MAX_CHAINS && kNestBlock == MCR_NESTED_BLOCK, "mcmcref_hip.h states the nested limits");

// The workspace of a chunk of pc parameters: the summary pipeline's layout for ONE chain of M draws (no buffer grows
// with chains x segments), then the chain moments and the superchain records.  Returns the ingest copy.
struct NestedChunk {
    const Tensor& t; i64 K;
    PipeIn a{}; double *mom = nullptr, *sup = nullptr;
    double* operator()(Carve& cv, i64 pc)
    {
        a = one_chain_pipe(t.M(), pc, true);
        double* X = carve_pipe(cv, a, true, FftPlan{}, t.ingest());
        mom = cv.take<double>((size_t)pc * kNestKinds * (size_t)t.C * 2);
        sup = cv.take<double>((size_t)pc * kNestKinds * (size_t)(K > 0 ? K : 1) * 2);
        return X;
    }
};

// Parameters per workspace chunk of a nested call (the most whose layout fits the limit and whose grids fit a launch).
static int plan_nested(mcr_ctx* ctx, NestedChunk& ch, i64& pcmax)
{
    const i64 nb = (ch.t.C + kNestChains - 1) / kNestChains;
    const i64 grid_cap = ((i64)0x7FFFFFFF / nb) / 8 * 8;   // k_chain_moments: ceil(pc / 8) * 8 * nb workgroups
    return plan_params(ctx, ch.t.P, grid_cap < kMaxGridY / 2 ? grid_cap : kMaxGridY / 2, ch, pcmax);
}

// What a nested call asks beyond pooled_check, and the chains ordered by superchain (stable): K runs of L chains in perm.
static int nested_check(mcr_ctx* ctx, i64 C, const int32_t* superchain, std::vector<int32_t>& perm, i64& K, i64& L)
{
    if (C > kMaxNestedChains)
        return fail(ctx, MCR_EINVAL, "nested R-hat supports at most %lld chains; got %lld", (long long)kMaxNestedChains, (long long)C);
    if (C > 0 && !superchain) return fail(ctx, MCR_EINVAL, "superchain is NULL");
    // superchains in the order of their first chain, chains in index order inside: the labels are names only
    std::unordered_map<int32_t, int32_t> dense;
    std::vector<int32_t> sid((size_t)C), count, first_label;
    for (i64 c = 0; c < C; ++c) {
        const auto it = dense.emplace(superchain[c], (int32_t)count.size());
        if (it.second) { count.push_back(0); first_label.push_back(superchain[c]); }
        sid[(size_t)c] = it.first->second;
        ++count[(size_t)it.first->second];
    }
    K = (i64)count.size();
    L = K > 0 ? count[0] : 0;
    for (i64 k = 1; k < K; ++k)
        if (count[(size_t)k] != L)
            return fail(ctx, MCR_EINVAL, "superchains must have the same number of chains: superchain %d has %lld, superchain %d has %lld",
                        (int)first_label[0], (long long)L, (int)first_label[(size_t)k], (long long)count[(size_t)k]);
    perm.resize((size_t)C);
    std::vector<i64> fill((size_t)K, 0);
    for (i64 c = 0; c < C; ++c) { const i64 k = sid[(size_t)c]; perm[(size_t)(k * L + fill[(size_t)k]++)] = (int32_t)c; }
    return MCR_OK;
}

static int nested_run(mcr_ctx* ctx, const Tensor& t, const std::vector<int32_t>& perm, i64 K, i64 L, const mcr_nested* out)
{
    const i64 M = t.M(), C = t.C, N = t.N, P = t.P;        // (the raw kind reads f64 rows: those of the ingest copy for f32 draws)
    NestedChunk ch{t, K};
    i64 pcmax = 0;
    int rc = plan_nested(ctx, ch, pcmax);
    if (rc) return rc;
    int32_t* d_perm = nullptr;
    double *d_res = nullptr, *ztab = nullptr;
    rc = get_ztab(ctx, M, &ztab);
    if (!rc) rc = call_table(ctx, perm, (size_t)kNestFields * (size_t)P, d_perm, d_res);
    if (rc) return rc;
    rc = tensor_chunks(ctx, t, pcmax, ch, [&](i64 pc, i64 p0, const double* X) -> int {
        PipeIn& a = ch.a;
        a.ztab = ztab;
        a.X = X;
        a.d_res = d_res + (size_t)kNestFields * (size_t)p0;
        const int rc = run_pipeline(ctx, a);   // one chain: sort, order statistics, bulk codes, fold, finalize (the bad count)
        if (rc) return rc;
        const i64 nb = (C + kNestChains - 1) / kNestChains;
        LAUNCH(ctx, K_CHAIN_MOMENTS, k_chain_moments, dim3((unsigned)((pc + 7) / 8 * 8 * nb)), dim3(kNestNT), 0,
               X, (const u32*)a.zb, (const u32*)a.zt, (const double*)ztab, M, C, N, pc, ch.mom);
        LAUNCH(ctx, K_NESTED_COMBINE, k_nested_combine, dim3((unsigned)pc, kNestKinds), dim3(kNestCombNT), 0,
               (const double*)ch.mom, (const int*)d_perm, C, K, L, N, ch.sup, a.d_res, pc, kNestField0);
        return MCR_OK;
    });
    if (rc) return rc;
    double* const dst[kNestKinds][3] = {{out->nrhat_raw, out->between_raw, out->within_raw},
                                        {out->nrhat_bulk, out->between_bulk, out->within_bulk},
                                        {out->nrhat_tail, out->between_tail, out->within_tail}};
    return pooled_results(ctx, d_res, kNestFields, P, pcmax, [&](const double* r, i64 pc, i64 p0, i64 p) {
        for (int k = 0; k < kNestKinds; ++k)
            for (int f = 0; f < 3; ++f)
                if (dst[k][f]) dst[k][f][p0 + p] = r[(size_t)(kNestField0 + 3 * k + f) * pc + p];
        if (out->nrhat) {                      // Python's max(bulk, tail)
            const double rb = r[(size_t)(kNestField0 + 3) * pc + p], rt = r[(size_t)(kNestField0 + 6) * pc + p];
            out->nrhat[p0 + p] = (rt > rb) ? rt : rb;
        }
    });
}

static void nested_fill_nan(const mcr_nested* o, i64 P)
{
    double* arrs[] = {o->nrhat, o->nrhat_bulk, o->nrhat_tail, o->nrhat_raw, o->between_bulk, o->within_bulk,
                      o->between_tail, o->within_tail, o->between_raw, o->within_raw};
    for (double* a : arrs)
        if (a) for (i64 p = 0; p < P; ++p) a[p] = NAN;
}

int mcr_nested_plan(mcr_ctx* ctx, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp,
                    int64_t K, int64_t* params_per_chunk)
{
    const Tensor t{nullptr, dtype, C, N, P, sc, sn, sp};
    return plan_entry(ctx, "mcr_nested_plan", t, params_per_chunk, [&](i64& pcmax) -> int {
        if (K < 1 || C > kMaxNestedChains) return MCR_OK;
        NestedChunk ch{t, K};
        return plan_nested(ctx, ch, pcmax);
    });
}

static int nested_entry(mcr_ctx* ctx, const Tensor& t, const int32_t* superchain, mcr_nested* out, bool host)
{
    std::vector<int32_t> perm;
    i64 K = 0, L = 0;
    return tensor_entry(ctx, "mcr_nested_rhat", t, out, host, [&] { return nested_check(ctx, t.C, superchain, perm, K, L); },
                        [&] { nested_fill_nan(out, t.P); },
                        [&](const Tensor& dev) { return nested_run(ctx, dev, perm, K, L, out); });
}

int mcr_nested_rhat_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc,
                        int64_t sn, int64_t sp, const int32_t* superchain, mcr_nested* out)
{
    return nested_entry(ctx, {draws_dev, dtype, C, N, P, sc, sn, sp}, superchain, out, false);
}

int mcr_nested_rhat(mcr_ctx* ctx, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn,
                    int64_t sp, const int32_t* superchain, mcr_nested* out)
{
    return nested_entry(ctx, {draws, dtype, C, N, P, sc, sn, sp}, superchain, out, true);
}

// ---- Pareto k-hat (mcr_pareto.hpp) --------------------------------------------------------------------------------------
constexpr int kParField0 = kPoolField0;
constexpr int kParFields = kParField0 + 2;                 // + khat_left, khat_right

static_assert(kParetoLdsTail == MCR_PARETO_LDS_TAIL, "mcmcref_hip.h states the LDS tail");

// Behind the pipeline's buffers: the grid values l_j of every tail.
static double* carve_pareto(Carve& cv, const PipeIn& a)
{
    return cv.take<double>((size_t)a.pc * 2 * (size_t)pareto_grid(a.M / 2));
}

// Parameters per workspace chunk of a Pareto call.
static int plan_pareto(mcr_ctx* ctx, const Tensor& t, i64& pcmax)
{
    return plan_pooled(ctx, t, [](Carve& cv, PipeIn& a) { carve_pareto(cv, a); }, pcmax);
}

// The default tail length: the smallest t with t^2 r_eff >= 9 M (that is ceil(3 sqrt(M / r_eff))) for M > 225, else
// floor(M / 5).  A bisection over integers: t^2 is exact, its product with r_eff rounds once and is monotone in t, no
// sqrt takes part.  Capped at 2^31, beyond the floor(M / 2) of any call.  (pareto_tail_bisect: the bisection alone, for
// every M -- mcr_psis takes its minimum with ceil(M / 5).)
static i64 pareto_tail_bisect(i64 M, double r_eff)
{
    const double need = 9.0 * (double)M;
    i64 lo = 0, hi = (i64)1 << 31;                         // lo fails, hi holds (or is the cap)
    while (hi - lo > 1) {
        const i64 mid = lo + (hi - lo) / 2;
        if ((double)(mid * mid) * r_eff >= need) hi = mid; else lo = mid;
    }
    return hi;
}
static i64 pareto_default_tail(i64 M, double r_eff) { return M <= 225 ? M / 5 : pareto_tail_bisect(M, r_eff); }

// The tail lengths a Pareto call is given, and the effective tail length of every parameter.
static int pareto_check(mcr_ctx* ctx, i64 M, i64 P, const int64_t* ndraws_tail, std::vector<i64>& teff)
{
    teff.resize((size_t)P);
    for (i64 p = 0; p < P; ++p) {
        const int rc = tail_check(ctx, ndraws_tail, p);
        if (rc) return rc;
        teff[(size_t)p] = pareto_tail_eff(M, ndraws_tail ? ndraws_tail[p] : pareto_default_tail(M, 1.0));
    }
    return MCR_OK;
}

static int pareto_run(mcr_ctx* ctx, const Tensor& t, const std::vector<i64>& teff, const mcr_pareto* out)
{
    const i64 M = t.M(), P = t.P;
    i64 pcmax = 0;
    int rc = plan_pareto(ctx, t, pcmax);
    i64* d_tail = nullptr;
    double* d_res = nullptr;
    if (!rc) rc = call_table(ctx, teff, (size_t)kParFields * (size_t)P, d_tail, d_res);
    if (rc) return rc;
    const i64 gmax = pareto_grid(M / 2);
    double* lg = nullptr;
    rc = pooled_chunks(ctx, t, pcmax, kParFields, d_res, [&](Carve& cv, PipeIn& a) { lg = carve_pareto(cv, a); },
                       [&](const PipeIn& a, const Sorted& so, i64 p0) -> int {
        size_t lds = 0;
        const int rc = tail_lds(ctx, teff, p0, a.pc, 0, reinterpret_cast<const void*>(&k_pareto_fit), lds);
        if (rc) return rc;
        LAUNCH(ctx, K_PARETO_FIT, k_pareto_fit, dim3((unsigned)((a.pc + 7) / 8 * 8 * 2)), dim3(kParetoNT), lds,
               (const double*)so.keys, M, a.pc, (const i64*)(d_tail + p0), so.keys_free, lg, gmax, a.d_res, kParField0);
        return MCR_OK;
    });
    if (rc) return rc;
    return pooled_results(ctx, d_res, kParFields, P, pcmax, [&](const double* r, i64 pc, i64 p0, i64 p) {
        const double kl = r[(size_t)kParField0 * pc + p], kr = r[(size_t)(kParField0 + 1) * pc + p];
        if (out->khat_left) out->khat_left[p0 + p] = kl;
        if (out->khat_right) out->khat_right[p0 + p] = kr;
        if (out->khat) out->khat[p0 + p] = (kr > kl) ? kr : kl;     // Python's max(left, right)
        if (out->ndraws_tail) out->ndraws_tail[p0 + p] = teff[(size_t)(p0 + p)];
    });
}

static void pareto_fill_nan(const mcr_pareto* o, i64 P)
{
    for (double* a : {o->khat, o->khat_left, o->khat_right})
        if (a) for (i64 p = 0; p < P; ++p) a[p] = NAN;
    if (o->ndraws_tail) for (i64 p = 0; p < P; ++p) o->ndraws_tail[p] = 0;
}

int mcr_pareto_plan(mcr_ctx* ctx, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp,
                    int64_t* params_per_chunk)
{
    const Tensor t{nullptr, dtype, C, N, P, sc, sn, sp};
    return plan_entry(ctx, "mcr_pareto_plan", t, params_per_chunk, [&](i64& pcmax) { return plan_pareto(ctx, t, pcmax); });
}

static int pareto_entry(mcr_ctx* ctx, const Tensor& t, const int64_t* ndraws_tail, mcr_pareto* out, bool host)
{
    std::vector<i64> teff;
    return tensor_entry(ctx, "mcr_pareto_khat", t, out, host, [&] { return pareto_check(ctx, t.M(), t.P, ndraws_tail, teff); },
                        [&] { pareto_fill_nan(out, t.P); }, [&](const Tensor& dev) { return pareto_run(ctx, dev, teff, out); });
}

int mcr_pareto_khat_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc,
                        int64_t sn, int64_t sp, const int64_t* ndraws_tail, mcr_pareto* out)
{
    return pareto_entry(ctx, {draws_dev, dtype, C, N, P, sc, sn, sp}, ndraws_tail, out, false);
}

int mcr_pareto_khat(mcr_ctx* ctx, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn,
                    int64_t sp, const int64_t* ndraws_tail, mcr_pareto* out)
{
    return pareto_entry(ctx, {draws, dtype, C, N, P, sc, sn, sp}, ndraws_tail, out, true);
}

int64_t mcr_pareto_tail_length(int64_t M, double r_eff)
{
    if (!(r_eff > 0.0) || std::isinf(r_eff)) return MCR_EINVAL;
    return M < 1 ? 0 : pareto_default_tail(M, r_eff);
}

int mcr_pareto_fit_host(const double* sorted, int64_t M, int64_t ndraws_tail, double* khat_left, double* khat_right,
                        int64_t* t_eff)
{
    if (M < 0 || ndraws_tail < 0 || (M > 0 && !sorted)) return MCR_EINVAL;
    const i64 t = pareto_tail_eff(M, ndraws_tail > 0 ? ndraws_tail : pareto_default_tail(M, 1.0));
    if (t_eff) *t_eff = t;
    double kl = NAN, kr = NAN;
    if (t >= kParetoMinTail && t < (i64)0x7FFFFFFFll) {
        std::vector<double> e((size_t)t), lg((size_t)pareto_grid(t));
        const ParetoHostWave w;
        for (i64 i = 0; i < t; ++i) e[(size_t)i] = sorted[t] - sorted[t - 1 - i];
        kl = pareto_fit(w, e.data(), (int)t, lg.data());
        for (i64 i = 0; i < t; ++i) e[(size_t)i] = sorted[M - t + i] - sorted[M - t - 1];
        kr = pareto_fit(w, e.data(), (int)t, lg.data());
    }
    if (khat_left) *khat_left = kl;
    if (khat_right) *khat_right = kr;
    return MCR_OK;
}

// ---- Pareto-smoothed importance sampling and PSIS-LOO (mcr_psis.hpp) ------------------------------------------------------
constexpr int kPsisField0 = kPoolField0;
constexpr int kPsisFields = kPsisField0 + kPsisRows;       // + khat, ndraws_tail, lppd, elpd, p_loo

struct PsisWs { double *lg, *cols, *w; };

// The fit's grid values of a column: carve_pareto's scratch as it is, 2 pareto_grid(M / 2) >= pareto_grid(M - 1) doubles.
static i64 psis_gmax(i64 M) { return 2 * (i64)pareto_grid(M / 2); }

// Behind the pipeline's buffers: that scratch, the columns' scalars for k_psis_weights and, for the host entry's weights,
// the chunk's [pc][M] log weights.
static void carve_psis(Carve& cv, const PipeIn& a, bool host_weights, PsisWs& w)
{
    w.lg = carve_pareto(cv, a);
    w.cols = cv.take<double>((size_t)a.pc * kPsisCols);
    w.w = host_weights ? cv.take<double>((size_t)a.pc * (size_t)a.M) : nullptr;
}

// Columns per workspace chunk of a PSIS call: what fits, and no more than k_psis_weights' one-dimensional grid holds.
static int plan_psis(mcr_ctx* ctx, const Tensor& t, bool host_weights, i64& pcmax)
{
    const i64 grid_hi = ((i64)0x7FFFFFFFll / ((t.M() + kPsisBlock - 1) / kPsisBlock)) / 8 * 8;     // >= 1016: M < 2^31
    return plan_pooled(ctx, t, [&](Carve& cv, PipeIn& a) { PsisWs w; carve_psis(cv, a, host_weights, w); }, pcmax, grid_hi);
}

static bool psis_r_eff_ok(double r) { return r > 0.0 && !std::isinf(r); }

// The default tail length of M >= 1 values: min(ceil(M / 5), the smallest t with t^2 r_eff >= 9 M).
static i64 psis_default_tail(i64 M, double r_eff)
{
    const i64 fifth = (M + 4) / 5, root = pareto_tail_bisect(M, r_eff);
    return fifth < root ? fifth : root;
}

// The effective tail length: min(t_req, M - 1), t_req the caller's (>= 1) or the default.
static i64 psis_tail_eff(i64 M, i64 t_req, double r_eff)
{
    if (t_req < 1) t_req = psis_default_tail(M, r_eff);
    return t_req < M - 1 ? t_req : M - 1;
}

// The arguments of a PSIS call, and the effective tail length of every column.
static int psis_check(mcr_ctx* ctx, i64 M, i64 P, int negate, const double* r_eff, const int64_t* ndraws_tail, std::vector<i64>& teff)
{
    if (negate != 0 && negate != 1) return fail(ctx, MCR_EINVAL, "negate must be 0 or 1; got %d", negate);
    teff.resize((size_t)P);
    for (i64 p = 0; p < P; ++p) {
        const int rc = tail_check(ctx, ndraws_tail, p);
        if (rc) return rc;
        if (r_eff && !psis_r_eff_ok(r_eff[p]))
            return fail(ctx, MCR_EINVAL, "r_eff[%lld] = %g: a relative efficiency must be finite and > 0", (long long)p, r_eff[p]);
        teff[(size_t)p] = M < 1 ? 0 : psis_tail_eff(M, ndraws_tail ? ndraws_tail[p] : 0, r_eff ? r_eff[p] : 1.0);
    }
    return MCR_OK;
}

static int psis_run(mcr_ctx* ctx, const Tensor& t, int negate, const std::vector<i64>& teff, const mcr_psis_out* out, bool host_weights)
{
    const i64 M = t.M(), P = t.P;
    const bool hw = host_weights && out->log_weights;
    i64 pcmax = 0;
    int rc = plan_psis(ctx, t, hw, pcmax);
    i64* d_tail = nullptr;
    double* d_res = nullptr;
    if (!rc) rc = call_table(ctx, teff, (size_t)kPsisFields * (size_t)P, d_tail, d_res);
    if (rc) return rc;
    const i64 gmax = psis_gmax(M);
    const unsigned nb = (unsigned)((M + kPsisBlock - 1) / kPsisBlock);
    PsisWs w{};
    rc = pooled_chunks(ctx, t, pcmax, kPsisFields, d_res, [&](Carve& cv, PipeIn& a) { carve_psis(cv, a, hw, w); },
                       [&](const PipeIn& a, const Sorted& so, i64 p0) -> int {
        size_t lds = 0;
        const int rc = tail_lds(ctx, teff, p0, a.pc, kPsisScratch, reinterpret_cast<const void*>(&k_psis_column), lds);
        if (rc) return rc;
        const unsigned pgrp = (unsigned)((a.pc + 7) / 8 * 8);
        LAUNCH(ctx, K_PSIS_COLUMN, k_psis_column, dim3(pgrp), dim3(kPsisNT), lds, (const double*)so.keys, M, a.pc, negate,
               (const i64*)(d_tail + p0), so.keys_free, w.lg, gmax, a.d_res, kPsisField0, w.cols);
        if (!out->log_weights) return MCR_OK;
        double* dst = hw ? w.w : out->log_weights + p0 * M;
        if (a.idx16)
            LAUNCH(ctx, K_PSIS_WEIGHTS, k_psis_weights<unsigned short>, dim3(pgrp * nb), dim3(256), 0, (const double*)so.keys,
                   (const unsigned short*)so.pos, M, a.pc, negate, (const double*)w.cols, dst);
        else
            LAUNCH(ctx, K_PSIS_WEIGHTS, k_psis_weights<u32>, dim3(pgrp * nb), dim3(256), 0, (const double*)so.keys,
                   (const u32*)so.pos, M, a.pc, negate, (const double*)w.cols, dst);
        if (hw)
            HIP_TRY(ctx, hipMemcpyAsync(out->log_weights + p0 * M, w.w, sizeof(double) * (size_t)a.pc * (size_t)M,
                                        hipMemcpyDeviceToHost, ctx->stream));
        return MCR_OK;
    });
    if (rc) return rc;
    return pooled_results(ctx, d_res, kPsisFields, P, pcmax, [&](const double* r, i64 pc, i64 p0, i64 p) {
        const double* f = r + (size_t)kPsisField0 * pc + p;
        if (out->khat) out->khat[p0 + p] = f[PR_KHAT * pc];
        if (out->ndraws_tail) out->ndraws_tail[p0 + p] = (i64)f[PR_NTAIL * pc];
        if (out->lppd) out->lppd[p0 + p] = f[PR_LPPD * pc];
        if (out->elpd) out->elpd[p0 + p] = f[PR_ELPD * pc];
        if (out->p_loo) out->p_loo[p0 + p] = f[PR_PLOO * pc];
    });
}

static void psis_fill_nan(const mcr_psis_out* o, i64 P)
{
    for (double* a : {o->khat, o->lppd, o->elpd, o->p_loo})
        if (a) for (i64 p = 0; p < P; ++p) a[p] = NAN;
    if (o->ndraws_tail) for (i64 p = 0; p < P; ++p) o->ndraws_tail[p] = 0;
}

// host: the host entry, whose log weights (like its draws) are the caller's host memory.
static int psis_entry(mcr_ctx* ctx, const Tensor& t, int negate, const double* r_eff, const int64_t* ndraws_tail, mcr_psis_out* out,
                      bool host)
{
    std::vector<i64> teff;
    return tensor_entry(ctx, "mcr_psis", t, out, host, [&] { return psis_check(ctx, t.M(), t.P, negate, r_eff, ndraws_tail, teff); },
                        [&] { psis_fill_nan(out, t.P); },
                        [&](const Tensor& dev) { return psis_run(ctx, dev, negate, teff, out, host); });
}

int mcr_psis_plan(mcr_ctx* ctx, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp,
                  int host_weights, int64_t* params_per_chunk)
{
    const Tensor t{nullptr, dtype, C, N, P, sc, sn, sp};
    return plan_entry(ctx, "mcr_psis_plan", t, params_per_chunk, [&](i64& pcmax) { return plan_psis(ctx, t, host_weights != 0, pcmax); });
}

int mcr_psis_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn,
                 int64_t sp, int negate, const double* r_eff, const int64_t* ndraws_tail, mcr_psis_out* out)
{
    return psis_entry(ctx, {draws_dev, dtype, C, N, P, sc, sn, sp}, negate, r_eff, ndraws_tail, out, false);
}

int mcr_psis(mcr_ctx* ctx, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp,
             int negate, const double* r_eff, const int64_t* ndraws_tail, mcr_psis_out* out)
{
    return psis_entry(ctx, {draws, dtype, C, N, P, sc, sn, sp}, negate, r_eff, ndraws_tail, out, true);
}

int64_t mcr_psis_tail_length(int64_t M, double r_eff)
{
    if (!psis_r_eff_ok(r_eff)) return MCR_EINVAL;
    return M < 1 ? 0 : psis_default_tail(M, r_eff);
}

int mcr_psis_host(const double* values, int64_t M, int negate, double r_eff, int64_t ndraws_tail, double* khat,
                  int64_t* n_tail, double* lppd, double* elpd, double* p_loo, double* log_weights)
{
    if (M < 0 || M >= (i64)0x7FFFFFFFll || (M > 0 && !values) || (negate != 0 && negate != 1) || ndraws_tail < 0 ||
        !psis_r_eff_ok(r_eff))
        return MCR_EINVAL;
    PsisResult c{};
    c.khat = c.lppd = c.elpd = c.ploo = NAN;
    if (M > 0) {
        for (i64 i = 0; i < M; ++i)
            if (!std::isfinite(values[i])) return MCR_ENONFINITE;
        std::vector<i64> at((size_t)M);
        for (i64 i = 0; i < M; ++i) at[(size_t)i] = i;
        std::sort(at.begin(), at.end(), [&](i64 a, i64 b) { return values[a] < values[b]; });
        std::vector<double> keys((size_t)M);
        for (i64 j = 0; j < M; ++j) keys[(size_t)j] = values[at[(size_t)j]];
        const i64 t = psis_tail_eff(M, ndraws_tail, r_eff);
        std::vector<double> e((size_t)(t > 0 ? t : 1)), lg((size_t)pareto_grid(t));
        const PsisKeys s{keys.data(), M, negate};
        c = psis_column(PsisHostGroup{}, s, t, e.data(), lg.data());
        if (log_weights)
            for (i64 j = 0; j < M; ++j) log_weights[at[(size_t)j]] = psis_log_weight(s, c, negate ? M - 1 - j : j);
    }
    if (khat) *khat = c.khat;
    if (n_tail) *n_tail = c.n;
    if (lppd) *lppd = c.lppd;
    if (elpd) *elpd = c.elpd;
    if (p_loo) *p_loo = c.ploo;
    return MCR_OK;
}

// ---- Highest-density intervals (mcr_hdi.hpp) ----------------------------------------------------------------------------
constexpr int kHdiField0 = kPoolField0;
constexpr int hdi_fields(int nprob) { return kHdiField0 + 3 * nprob; }     // + lo, hi, index of every probability

static_assert(kHdiSlice == MCR_HDI_SLICE && kHdiMaxProbs == MCR_HDI_MAX_PROBS, "mcmcref_hip.h states the slice and the cap");
static_assert((kHdiSlice & (kHdiSlice - 1)) == 0, "a slice is a power of two");

// Behind the pipeline's buffers: one candidate per (parameter, probability, slice), for the most slices a probability can
// need (inc = 0: W = M) -- the plan knows the number of probabilities, not their values.
static HdiCand* carve_hdi(Carve& cv, const PipeIn& a, int nprob)
{
    return cv.take<HdiCand>((size_t)a.pc * (size_t)nprob * (size_t)hdi_slices(a.M));
}

// Parameters per workspace chunk of an HDI call: what fits, and no more than k_hdi_window's one-dimensional grid holds.
static int plan_hdi(mcr_ctx* ctx, const Tensor& t, int nprob, i64& pcmax)
{
    const i64 grid_hi = ((i64)0x7FFFFFFFll / ((i64)nprob * hdi_slices(t.M()))) / 8 * 8;  // >= 4096: M < 2^31, nprob <= 16
    return plan_pooled(ctx, t, [&](Carve& cv, PipeIn& a) { carve_hdi(cv, a, nprob); }, pcmax, grid_hi);
}

// The probabilities of a call, and inc = floor(prob * M) of every one: one rounded product.
static int hdi_check(mcr_ctx* ctx, const double* probs, int nprob, i64 M, HdiArgs& h)
{
    if (nprob < 1 || nprob > kHdiMaxProbs) return fail(ctx, MCR_EINVAL, "nprob must be in [1, %d]; got %d", kHdiMaxProbs, nprob);
    if (!probs) return fail(ctx, MCR_EINVAL, "probs is NULL");
    h.nprob = nprob;
    for (int j = 0; j < nprob; ++j) {
        if (!(probs[j] > 0.0 && probs[j] < 1.0)) return fail(ctx, MCR_EINVAL, "probs[%d] = %g: a probability must lie in (0, 1)", j, probs[j]);
        h.inc[j] = (i64)std::floor(probs[j] * (double)M);
    }
    return MCR_OK;
}

static void hdi_store(const mcr_hdi_out* o, i64 at, double lo, double hi, i64 index)
{
    if (o->lo) o->lo[at] = lo;
    if (o->hi) o->hi[at] = hi;
    if (o->index) o->index[at] = index;
}

static int hdi_run(mcr_ctx* ctx, const Tensor& t, const HdiArgs& h, const mcr_hdi_out* out)
{
    const i64 M = t.M(), P = t.P;
    const int nprob = h.nprob, fields = hdi_fields(nprob), nsl = (int)hdi_slices(M);
    i64 pcmax = 0;
    int rc = plan_hdi(ctx, t, nprob, pcmax);
    double* d_res = nullptr;
    if (!rc) rc = carve(ctx, ctx->call_dev, [&](Carve& cv) { d_res = cv.take<double>((size_t)fields * (size_t)P); });
    if (rc) return rc;
    HdiCand* part = nullptr;
    rc = pooled_chunks(ctx, t, pcmax, fields, d_res, [&](Carve& cv, PipeIn& a) { part = carve_hdi(cv, a, nprob); },
                       [&](const PipeIn& a, const Sorted& so, i64) -> int {
        LAUNCH(ctx, K_HDI_WINDOW, k_hdi_window, dim3((unsigned)((a.pc + 7) / 8 * 8 * nprob * nsl)), dim3(kHdiNT), 0,
               (const double*)so.keys, M, a.pc, h, nsl, part);
        LAUNCH(ctx, K_HDI_PICK, k_hdi_pick, dim3((unsigned)((a.pc * nprob + 63) / 64)), dim3(64), 0,
               (const double*)so.keys, M, a.pc, h, nsl, (const HdiCand*)part, a.d_res, kHdiField0);
        return MCR_OK;
    });
    if (rc) return rc;
    return pooled_results(ctx, d_res, fields, P, pcmax, [&](const double* r, i64 pc, i64 p0, i64 p) {
        for (int j = 0; j < nprob; ++j) {
            const double* f = r + (size_t)(kHdiField0 + 3 * j) * pc + p;
            hdi_store(out, (p0 + p) * nprob + j, f[0], f[pc], (i64)f[2 * pc]);
        }
    });
}

int mcr_hdi_plan(mcr_ctx* ctx, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp, int nprob,
                 int64_t* params_per_chunk)
{
    const Tensor t{nullptr, dtype, C, N, P, sc, sn, sp};
    return plan_entry(ctx, "mcr_hdi_plan", t, params_per_chunk, [&](i64& pcmax) {
        if (nprob < 1 || nprob > kHdiMaxProbs) return fail(ctx, MCR_EINVAL, "nprob must be in [1, %d]; got %d", kHdiMaxProbs, nprob);
        return plan_hdi(ctx, t, nprob, pcmax);
    });
}

static int hdi_entry(mcr_ctx* ctx, const Tensor& t, const double* probs, int nprob, mcr_hdi_out* out, bool host)
{
    HdiArgs h{};
    return tensor_entry(ctx, "mcr_hdi", t, out, host, [&] { return hdi_check(ctx, probs, nprob, t.M(), h); },
                        [&] { for (i64 at = 0; at < t.P * nprob; ++at) hdi_store(out, at, NAN, NAN, -1); },
                        [&](const Tensor& dev) { return hdi_run(ctx, dev, h, out); });
}

int mcr_hdi_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn,
                int64_t sp, const double* probs, int nprob, mcr_hdi_out* out)
{
    return hdi_entry(ctx, {draws_dev, dtype, C, N, P, sc, sn, sp}, probs, nprob, out, false);
}

int mcr_hdi(mcr_ctx* ctx, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp,
            const double* probs, int nprob, mcr_hdi_out* out)
{
    return hdi_entry(ctx, {draws, dtype, C, N, P, sc, sn, sp}, probs, nprob, out, true);
}

int mcr_hdi_sorted_host(const double* sorted, int64_t M, const double* probs, int nprob, double* lo, double* hi, int64_t* index)
{
    if (M < 0 || (M > 0 && !sorted) || !probs || nprob < 1 || nprob > kHdiMaxProbs) return MCR_EINVAL;
    for (int j = 0; j < nprob; ++j)
        if (!(probs[j] > 0.0 && probs[j] < 1.0)) return MCR_EINVAL;
    for (int j = 0; j < nprob; ++j) {
        const i64 inc = (i64)std::floor(probs[j] * (double)M), W = M - inc;
        HdiCand best = HdiCand::none();
        for (i64 i = 0; i < W; ++i) hdi_take(best, sorted[i + inc] - sorted[i], i);
        const bool ok = best.i >= 0 && best.i < W;
        if (lo) lo[j] = ok ? sorted[best.i] : NAN;
        if (hi) hi[j] = ok ? sorted[best.i + inc] : NAN;
        if (index) index[j] = ok ? best.i : -1;
    }
    return MCR_OK;
}

// ---- Importance-weighted summaries (mcr_weighted.hpp) -------------------------------------------------------------------
constexpr int kWgtField0 = kPoolField0;
constexpr int wgt_fields(int nq) { return kWgtField0 + WR_Q0 + nq; }       // + mean, sd, mean_se and every quantile

static_assert(kWgtBlock == MCR_WEIGHTED_BLOCK && kWgtMaxQ == MCR_WEIGHTED_MAX_Q, "mcmcref_hip.h states the block and the cap");

struct WgtWs { double *part, *mean, *qb; };

// Behind the pipeline's buffers: the moment passes' block sums (two per block in the second pass), the means between the
// passes and, with quantiles, the sorted order's block sums.
static void carve_weighted(Carve& cv, const PipeIn& a, int nq, WgtWs& w)
{
    const size_t nb = (size_t)wgt_blocks(a.M);
    w.part = cv.take<double>((size_t)a.pc * nb * 2);
    w.mean = cv.take<double>((size_t)a.pc);
    w.qb = nq > 0 ? cv.take<double>((size_t)a.pc * nb) : nullptr;
}

// Parameters per workspace chunk of a weighted call: what fits, and no more than the one-dimensional grids hold.
static int plan_weighted(mcr_ctx* ctx, const Tensor& t, int nq, i64& pcmax)
{
    const i64 grid_hi = ((i64)0x7FFFFFFFll / wgt_blocks(t.M())) / 8 * 8;          // >= 1016: M < 2^31
    return plan_pooled(ctx, t, [&](Carve& cv, PipeIn& a) { WgtWs w; carve_weighted(cv, a, nq, w); }, pcmax, grid_hi);
}

// The call's own arguments: the flags, the weight vector's presence, the probabilities.
static int weighted_check(mcr_ctx* ctx, const double* v, i64 M, int flags, const double* probs, int nq, WgtArgs& g)
{
    if (flags & ~MCR_W_LOG) return fail(ctx, MCR_EINVAL, "unknown flag bits 0x%x", flags & ~MCR_W_LOG);
    if (nq < 0 || nq > kWgtMaxQ) return fail(ctx, MCR_EINVAL, "nq must be in [0, %d]; got %d", kWgtMaxQ, nq);
    if (nq > 0 && !probs) return fail(ctx, MCR_EINVAL, "probs is NULL");
    if (M > 0 && !v) return fail(ctx, MCR_EINVAL, "weights is NULL");
    g.nq = nq;
    for (int j = 0; j < nq; ++j) {
        if (!(probs[j] >= 0.0 && probs[j] <= 1.0)) return fail(ctx, MCR_EINVAL, "probs[%d] = %g: a probability must lie in [0, 1]", j, probs[j]);
        g.q[j] = probs[j];
    }
    return MCR_OK;
}

// What the prepared totals say about the weight vector, in one text for the device and the host routine.
static const char* weighted_refusal(const double* tot, char* text, size_t len)
{
    if (tot[WT_BAD] > 0.0) snprintf(text, len, "weights: %.0f entries are not weights (linear: finite and >= 0; log: finite or -inf)", tot[WT_BAD]);
    else if (!(tot[WT_S1] > 0.0)) snprintf(text, len, "weights: no entry is positive");
    else if (std::isinf(tot[WT_S1]) || std::isinf(tot[WT_S2])) snprintf(text, len, "weights: their sum or sum of squares overflows");
    else return nullptr;
    return text;
}

static void weighted_fill_nan(const mcr_weighted_out* o, i64 P, int nq)
{
    for (double* a : {o->mean, o->sd, o->mean_se})
        if (a) for (i64 p = 0; p < P; ++p) a[p] = NAN;
    if (o->quantiles) for (i64 at = 0; at < P * nq; ++at) o->quantiles[at] = NAN;
    if (o->ess) *o->ess = NAN;
    if (o->weight_sum) *o->weight_sum = NAN;
}

// host: the host entry, whose weight vector and weights output (like its draws) are the caller's host memory.
static int weighted_run(mcr_ctx* ctx, const Tensor& t, const double* v, int flags, const WgtArgs& g, const mcr_weighted_out* out, bool host)
{
    const i64 M = t.M(), P = t.P, nb = wgt_blocks(M);
    const int nq = g.nq, fields = wgt_fields(nq), log = (flags & MCR_W_LOG) ? 1 : 0;
    i64 pcmax = 0;
    int rc = plan_weighted(ctx, t, nq, pcmax);
    double *d_v = nullptr, *d_w = nullptr, *d_bs = nullptr, *d_tot = nullptr, *d_res = nullptr;
    if (!rc) rc = carve(ctx, ctx->call_dev, [&](Carve& cv) {
        d_v = host ? cv.take<double>((size_t)M) : nullptr;
        d_w = cv.take<double>((size_t)M);
        d_bs = cv.take<double>((size_t)nb * 2);
        d_tot = cv.take<double>(kWgtTotals);
        d_res = cv.take<double>((size_t)fields * (size_t)P);
    });
    if (rc) return rc;
    if (host) HIP_TRY(ctx, hipMemcpyAsync(d_v, v, sizeof(double) * (size_t)M, hipMemcpyHostToDevice, ctx->stream));
    LAUNCH(ctx, K_WEIGHT_PREPARE, k_weight_prepare, dim3(1), dim3(kWgtPrepNT), 0, host ? (const double*)d_v : v, M, log, d_w, d_bs, d_tot);
    double tot[kWgtTotals];
    HIP_TRY(ctx, hipMemcpyAsync(tot, d_tot, sizeof tot, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    char text[160];
    if (weighted_refusal(tot, text, sizeof text)) return fail(ctx, MCR_EINVAL, "%s", text);
    WgtWs w{};
    const unsigned nsl = (unsigned)((nb + kWgtSlice - 1) / kWgtSlice);
    rc = pooled_chunks(ctx, t, pcmax, fields, d_res, [&](Carve& cv, PipeIn& a) { carve_weighted(cv, a, nq, w); },
                       [&](const PipeIn& a, const Sorted& so, i64) -> int {
        const unsigned pgrp = (unsigned)((a.pc + 7) / 8 * 8);
        LAUNCH(ctx, K_WEIGHTED_MOMENTS, k_weighted_moments<1>, dim3(pgrp * nsl), dim3(kWgtNT), 0, (const double*)a.X, (const double*)d_w, M, a.pc,
               (const double*)w.mean, w.part);
        LAUNCH(ctx, K_WEIGHTED_COMBINE, k_weighted_combine<1>, dim3((unsigned)a.pc), dim3(kWave), 0, (const double*)w.part, nb, a.pc,
               (const double*)d_tot, w.mean, a.d_res, kWgtField0);
        LAUNCH(ctx, K_WEIGHTED_MOMENTS, k_weighted_moments<2>, dim3(pgrp * nsl), dim3(kWgtNT), 0, (const double*)a.X, (const double*)d_w, M, a.pc,
               (const double*)w.mean, w.part);
        LAUNCH(ctx, K_WEIGHTED_COMBINE, k_weighted_combine<2>, dim3((unsigned)a.pc), dim3(kWave), 0, (const double*)w.part, nb, a.pc,
               (const double*)d_tot, w.mean, a.d_res, kWgtField0);
        if (!nq) return MCR_OK;
        if (a.idx16) {
            LAUNCH(ctx, K_WQ_BLOCKS, k_wq_blocks<unsigned short>, dim3(pgrp * (unsigned)nb), dim3(kWave), 0,
                   (const unsigned short*)so.pos, (const double*)d_w, M, a.pc, w.qb);
            LAUNCH(ctx, K_WQ_PICK, k_wq_pick<unsigned short>, dim3(pgrp), dim3(kWgtNT), 0, (const double*)so.keys,
                   (const unsigned short*)so.pos, (const double*)d_w, M, a.pc, g, (const double*)w.qb, a.d_res, kWgtField0 + WR_Q0);
        } else {
            LAUNCH(ctx, K_WQ_BLOCKS, k_wq_blocks<u32>, dim3(pgrp * (unsigned)nb), dim3(kWave), 0, (const u32*)so.pos,
                   (const double*)d_w, M, a.pc, w.qb);
            LAUNCH(ctx, K_WQ_PICK, k_wq_pick<u32>, dim3(pgrp), dim3(kWgtNT), 0, (const double*)so.keys, (const u32*)so.pos,
                   (const double*)d_w, M, a.pc, g, (const double*)w.qb, a.d_res, kWgtField0 + WR_Q0);
        }
        return MCR_OK;
    });
    if (rc) return rc;
    if (out->weights)
        HIP_TRY(ctx, hipMemcpyAsync(out->weights, d_w, sizeof(double) * (size_t)M, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                                    ctx->stream));
    if (out->ess) *out->ess = wgt_sq(tot[WT_S1]) / tot[WT_S2];
    if (out->weight_sum) *out->weight_sum = tot[WT_S1];
    return pooled_results(ctx, d_res, fields, P, pcmax, [&](const double* r, i64 pc, i64 p0, i64 p) {
        const double* f = r + (size_t)kWgtField0 * pc + p;
        if (out->mean) out->mean[p0 + p] = f[WR_MEAN * pc];
        if (out->sd) out->sd[p0 + p] = f[WR_SD * pc];
        if (out->mean_se) out->mean_se[p0 + p] = f[WR_SE * pc];
        if (out->quantiles) for (int j = 0; j < nq; ++j) out->quantiles[(p0 + p) * nq + j] = f[(WR_Q0 + j) * pc];
    });
}

int mcr_weighted_plan(mcr_ctx* ctx, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp, int nq,
                      int64_t* params_per_chunk)
{
    const Tensor t{nullptr, dtype, C, N, P, sc, sn, sp};
    return plan_entry(ctx, "mcr_weighted_plan", t, params_per_chunk, [&](i64& pcmax) {
        if (nq < 0 || nq > kWgtMaxQ) return fail(ctx, MCR_EINVAL, "nq must be in [0, %d]; got %d", kWgtMaxQ, nq);
        return plan_weighted(ctx, t, nq, pcmax);
    });
}

static int weighted_entry(mcr_ctx* ctx, const Tensor& t, const double* v, int flags, const double* probs, int nq,
                          mcr_weighted_out* out, bool host)
{
    WgtArgs g{};
    return tensor_entry(ctx, "mcr_weighted_summary", t, out, host, [&] { return weighted_check(ctx, v, t.M(), flags, probs, nq, g); },
                        [&] { weighted_fill_nan(out, t.P, nq); },
                        [&](const Tensor& dev) { return weighted_run(ctx, dev, v, flags, g, out, host); });
}

int mcr_weighted_summary_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc,
                             int64_t sn, int64_t sp, const double* weights_dev, int flags, const double* probs, int nq,
                             mcr_weighted_out* out)
{
    return weighted_entry(ctx, {draws_dev, dtype, C, N, P, sc, sn, sp}, weights_dev, flags, probs, nq, out, false);
}

int mcr_weighted_summary(mcr_ctx* ctx, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn,
                         int64_t sp, const double* weights, int flags, const double* probs, int nq, mcr_weighted_out* out)
{
    return weighted_entry(ctx, {draws, dtype, C, N, P, sc, sn, sp}, weights, flags, probs, nq, out, true);
}

int mcr_weighted_host(const double* x, const double* v, int64_t M, int flags, const double* probs, int nq, double* mean,
                      double* sd, double* mean_se, double* quantiles, double* ess, double* weight_sum, double* weights)
{
    if (M < 0 || M >= (i64)0x7FFFFFFFll || (M > 0 && (!x || !v)) || (flags & ~MCR_W_LOG) || nq < 0 || nq > kWgtMaxQ || (nq > 0 && !probs))
        return MCR_EINVAL;
    for (int j = 0; j < nq; ++j)
        if (!(probs[j] >= 0.0 && probs[j] <= 1.0)) return MCR_EINVAL;
    double r_mean = NAN, r_sd = NAN, r_se = NAN, r_ess = NAN, r_s1 = NAN;
    std::vector<double> q((size_t)nq, NAN);
    if (M > 0) {
        const int log = (flags & MCR_W_LOG) ? 1 : 0;
        double tot[kWgtTotals] = {0.0, -INFINITY, 0.0, 0.0};
        for (i64 m = 0; m < M; ++m) {
            if (wgt_bad(v[m], log)) tot[WT_BAD] += 1.0;
            else if (v[m] > tot[WT_MAX]) tot[WT_MAX] = v[m];
        }
        std::vector<double> w((size_t)M, 0.0);
        WgtHostTree tr;
        if (!(tot[WT_BAD] > 0.0) && !(log && !(tot[WT_MAX] > -INFINITY))) {
            for (i64 m = 0; m < M; ++m) w[(size_t)m] = wgt_weight(v[m], log, tot[WT_MAX]);
            tot[WT_S1] = wgt_host_sum(tr, M, [&](i64 m) { return w[(size_t)m]; });
            tot[WT_S2] = wgt_host_sum(tr, M, [&](i64 m) { return wgt_sq(w[(size_t)m]); });
        }
        char text[160];
        if (weighted_refusal(tot, text, sizeof text)) return MCR_EINVAL;
        for (i64 m = 0; m < M; ++m)
            if (!std::isfinite(x[m])) return MCR_ENONFINITE;
        const double S1 = tot[WT_S1];
        r_s1 = S1;
        r_ess = wgt_sq(S1) / tot[WT_S2];
        r_mean = wgt_host_sum(tr, M, [&](i64 m) { return wgt_wx(w[(size_t)m], x[m]); }) / S1;
        double t1, t2;
        const double q1 = wgt_host_sum(tr, M, [&](i64 m) { wgt_dev2(w[(size_t)m], x[m], r_mean, t1, t2); return t1; });
        const double q2 = wgt_host_sum(tr, M, [&](i64 m) { wgt_dev2(w[(size_t)m], x[m], r_mean, t1, t2); return t2; });
        r_sd = std::sqrt(q1 / S1);
        r_se = std::sqrt(q2) / S1;
        if (nq > 0) {
            std::vector<i64> at((size_t)M);
            for (i64 i = 0; i < M; ++i) at[(size_t)i] = i;
            std::sort(at.begin(), at.end(), [&](i64 a, i64 b) { return x[a] < x[b] || (x[a] == x[b] && a < b); });
            const auto u = [&](i64 j) { return w[(size_t)at[(size_t)j]]; };
            std::vector<double> roots;
            wgt_host_sum(tr, M, u, &roots);
            for (int j = 0; j < nq; ++j) {
                double t = 0.0, prev = 0.0;
                const i64 b = wgt_find_block([&](i64 k) { return roots[(size_t)k]; }, (i64)roots.size(), probs[j], t, prev);
                if (b < 0) continue;
                tr.build([&](int i) { const i64 k = b * kWgtBlock + i; return k < M ? u(k) : 0.0; });
                for (int i = 0; i < kWgtBlock && b * kWgtBlock + i < M; ++i)
                    if (wgt_reached(wgt_add(prev, wgt_prefix(tr, i + 1)), t)) { q[(size_t)j] = x[at[(size_t)(b * kWgtBlock + i)]]; break; }
            }
        }
        if (weights) for (i64 m = 0; m < M; ++m) weights[m] = w[(size_t)m];
    }
    if (mean) *mean = r_mean;
    if (sd) *sd = r_sd;
    if (mean_se) *mean_se = r_se;
    if (ess) *ess = r_ess;
    if (weight_sum) *weight_sum = r_s1;
    if (quantiles) for (int j = 0; j < nq; ++j) quantiles[j] = q[(size_t)j];
    return MCR_OK;
}

// ---- Simulation-based calibration (mcr_sbc.hpp) ------------------------------------------------------------------------------
// The tensor's fourth axis: the call is cut into chunks of SIMULATIONS, not of parameters, and only where it needs the
// ingest copy; the result table [kSbcFields][S P] lies behind the uploaded truth in the call's device table.

// What a call asks of its shape beyond pooled_check (`ctx` NULL: the host routine's, no message kept): the plan entry's too.
static int sbc_shape_check(mcr_ctx* ctx, i64 S, i64 P)
{
    if (S < 0) return fail(ctx, MCR_EINVAL, "negative dimension (S=%lld)", (long long)S);
    if (P > 0 && S > (i64)0x7FFFFFFFll / P) return fail(ctx, MCR_EINVAL, "S*P must be < 2^31");
    return MCR_OK;
}

// ... and of its true values.
static int sbc_check(mcr_ctx* ctx, i64 S, i64 P, const double* truth)
{
    const int rc = sbc_shape_check(ctx, S, P);
    if (rc) return rc;
    if (!truth && S * P > 0) return fail(ctx, MCR_EINVAL, "truth is NULL");
    for (i64 k = 0; k < S * P; ++k)
        if (!std::isfinite(truth[k]))
            return fail(ctx, MCR_EINVAL, "truth[%lld][%lld] = %g: the true values must be finite", (long long)(k / P), (long long)(k % P), truth[k]);
    return MCR_OK;
}

// Simulations without draws: the counts 0, NaN mean and sd.
static void sbc_fill_empty(const mcr_sbc_out* o, i64 rows)
{
    for (int64_t* a : {o->n_less, o->n_equal})
        if (a) for (i64 k = 0; k < rows; ++k) a[k] = 0;
    for (double* a : {o->mean, o->sd})
        if (a) for (i64 k = 0; k < rows; ++k) a[k] = NAN;
}

// Simulations per workspace chunk: all of them where the kernel reads the caller's rows, else as many ingest copies as fit.
static int plan_sbc(mcr_ctx* ctx, const Tensor& t, i64& scmax)
{
    scmax = t.S;
    if (!t.ingest()) return MCR_OK;
    // k P < 2^31 rows (sbc_shape_check) of M < 2^31 - 1 draws: the count of doubles stays below 2^62; its bytes may not fit
    auto measure = [&](i64 k) {
        const size_t n = (size_t)k * (size_t)t.P * (size_t)t.M();
        if (n > SIZE_MAX / (2 * sizeof(double))) return (size_t)SIZE_MAX;
        Carve m{nullptr};
        m.take<double>(n);
        return m.off;
    };
    scmax = most_that_fit(t.S, [&](i64 k) { return measure(k) <= ctx->ws_limit; });
    if (!scmax) return fail(ctx, MCR_ENOMEM, "one simulation needs %zu bytes of workspace; limit is %zu", measure(1), ctx->ws_limit);
    return MCR_OK;
}

// Rows of up to kSbcRegBlocks blocks stay in registers between the passes; one block needs a quarter of them.
static int launch_sbc(mcr_ctx* ctx, const double* X, i64 L, i64 rows, const double* d_truth, double* d_res, i64 stride)
{
    const dim3 grid((unsigned)((rows + kSbcRows - 1) / kSbcRows));
    if (L > kWgtBlock && L <= (i64)kSbcRegBlocks * kWgtBlock)
        LAUNCH(ctx, K_SBC_RANKS, (k_sbc_ranks<kSbcRegBlocks>), grid, dim3(kSbcNT), 0, X, L, rows, d_truth, d_res, stride);
    else
        LAUNCH(ctx, K_SBC_RANKS, (k_sbc_ranks<1>), grid, dim3(kSbcNT), 0, X, L, rows, d_truth, d_res, stride);
    return MCR_OK;
}

static int sbc_run(mcr_ctx* ctx, const Tensor& t, const double* truth, const mcr_sbc_out* out)
{
    const i64 L = t.M(), P = t.P, rows = t.S * P;
    i64 scmax = 0;
    int rc = plan_sbc(ctx, t, scmax);
    if (rc) return rc;
    const std::vector<double> head(truth, truth + rows);
    double *d_truth = nullptr, *d_res = nullptr;
    rc = call_table(ctx, head, (size_t)kSbcFields * (size_t)rows, d_truth, d_res);
    if (!rc) rc = ctx->call_host.reserve(ctx, sizeof(double) * (size_t)kSbcFields * (size_t)rows);
    if (rc) return rc;
    const bool ingest = t.ingest();
    const size_t es = t.dtype == MCR_F64 ? 8 : 4;
    for (i64 s0 = 0; s0 < t.S; s0 += scmax) {
        const i64 sc = t.S - s0 < scmax ? t.S - s0 : scmax, r0 = s0 * P;
        const double* X = reinterpret_cast<const double*>(t.draws) + r0 * L;
        if (ingest) {
            double* copy = nullptr;
            rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) { copy = cv.take<double>((size_t)sc * (size_t)P * (size_t)L); });
            for (i64 s = 0; s < sc && !rc; s += kMaxGridY)                         // (k_ingest's simulations lie along z,
                for (i64 p0 = 0; p0 < P && !rc; p0 += kMaxGridY / 2) {             //  its parameters along y)
                    const i64 ns = sc - s < kMaxGridY ? sc - s : kMaxGridY, pc = P - p0 < kMaxGridY / 2 ? P - p0 : kMaxGridY / 2;
                    rc = launch_ingest(ctx, static_cast<const char*>(t.draws) + (size_t)(s0 + s) * (size_t)t.ss * es, t.dtype,
                                       copy + (s * P + p0) * L, t.C, t.N, pc, t.sc, t.sn, t.sp, p0, ns, t.ss, P * L);
                }
            if (rc) return rc;
            X = copy;
        }
        rc = launch_sbc(ctx, X, L, sc * P, d_truth + r0, d_res + r0, rows);
        if (rc) return rc;
    }
    const double* h = ctx->call_host.as<double>();
    HIP_TRY(ctx, hipMemcpyAsync(ctx->call_host.p, d_res, sizeof(double) * (size_t)kSbcFields * (size_t)rows, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    double nbad = 0.0;
    for (i64 k = 0; k < rows; ++k) {
        if (out->n_less) out->n_less[k] = (int64_t)h[(size_t)SB_LESS * (size_t)rows + (size_t)k];
        if (out->n_equal) out->n_equal[k] = (int64_t)h[(size_t)SB_EQUAL * (size_t)rows + (size_t)k];
        nbad += h[(size_t)SB_BAD * (size_t)rows + (size_t)k];
    }
    if (out->mean) memcpy(out->mean, h + (size_t)SB_MEAN * (size_t)rows, sizeof(double) * (size_t)rows);
    if (out->sd) memcpy(out->sd, h + (size_t)SB_SD * (size_t)rows, sizeof(double) * (size_t)rows);
    if (nbad > 0.0) return fail(ctx, MCR_ENONFINITE, "draws contain %.0f non-finite value(s)", nbad);
    return MCR_OK;
}

static Tensor sbc_tensor(const void* draws, int dtype, i64 S, i64 C, i64 N, i64 P, i64 ss, i64 sc, i64 sn, i64 sp)
{
    Tensor t{draws, dtype, C, N, P, sc, sn, sp};
    t.S = S; t.ss = ss;
    return t;
}

static int sbc_entry(mcr_ctx* ctx, const Tensor& t, const double* truth, mcr_sbc_out* out, bool host)
{
    return tensor_entry(ctx, "mcr_sbc_ranks", t, out, host, [&] { return sbc_check(ctx, t.S, t.P, truth); },
                        [&] { sbc_fill_empty(out, t.S * t.P); }, [&](const Tensor& dev) { return sbc_run(ctx, dev, truth, out); });
}

int mcr_sbc_ranks_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t S, int64_t C, int64_t N, int64_t P, int64_t ss,
                      int64_t sc, int64_t sn, int64_t sp, const double* truth, mcr_sbc_out* out)
{
    return sbc_entry(ctx, sbc_tensor(draws_dev, dtype, S, C, N, P, ss, sc, sn, sp), truth, out, false);
}

int mcr_sbc_ranks(mcr_ctx* ctx, const void* draws, int dtype, int64_t S, int64_t C, int64_t N, int64_t P, int64_t ss, int64_t sc,
                  int64_t sn, int64_t sp, const double* truth, mcr_sbc_out* out)
{
    return sbc_entry(ctx, sbc_tensor(draws, dtype, S, C, N, P, ss, sc, sn, sp), truth, out, true);
}

int mcr_sbc_plan(mcr_ctx* ctx, int dtype, int64_t S, int64_t C, int64_t N, int64_t P, int64_t ss, int64_t sc, int64_t sn,
                 int64_t sp, int64_t* sims_per_chunk)
{
    const Tensor t = sbc_tensor(nullptr, dtype, S, C, N, P, ss, sc, sn, sp);
    return plan_entry(ctx, "mcr_sbc_plan", t, sims_per_chunk, [&](i64& scmax) {
        const int rc = sbc_shape_check(ctx, S, P);                         // (what the call would refuse, the plan refuses)
        return rc || S < 1 ? rc : plan_sbc(ctx, t, scmax);
    });
}

int mcr_sbc_ranks_host(const double* x, int64_t S, int64_t P, int64_t L, const double* truth, mcr_sbc_out* out)
{
    if (!out || P < 0 || L < 0 || L >= (i64)0x7FFFFFFFll) return MCR_EINVAL;
    const int rc = sbc_check(nullptr, S, P, truth);
    if (rc) return rc;
    const i64 rows = S * P;
    if (rows == 0) return MCR_OK;
    if (L == 0) { sbc_fill_empty(out, rows); return MCR_OK; }
    if (!x) return MCR_EINVAL;
    WgtHostTree tr;
    i64 nbad = 0;
    for (i64 k = 0; k < rows; ++k) {
        i64 less, equal, bad;
        double mean, sd;
        sbc_row_host(tr, x + k * L, L, truth[k], less, equal, bad, mean, sd);
        if (out->n_less) out->n_less[k] = less;
        if (out->n_equal) out->n_equal[k] = equal;
        if (out->mean) out->mean[k] = mean;
        if (out->sd) out->sd[k] = sd;
        nbad += bad;
    }
    return nbad > 0 ? MCR_ENONFINITE : MCR_OK;
}

double mcr_chi2_sf(double x, double dof)
{
    if (!(dof > 0.0) || !(x >= 0.0)) return NAN;
    return sbc_gamma_q(0.5 * dof, 0.5 * x);
}

int mcr_sbc_uniformity(const int64_t* ranks, int64_t S, int64_t P, int64_t L, int64_t B, int64_t* counts, double* expected,
                       double* chi2, double* pvalue, double* ecdf_dev)
{
    if (!ranks || S < 1 || P < 0 || L < 0 || L >= (i64)0x7FFFFFFFll || B < 2 || B > L + 1) return MCR_EINVAL;
    std::vector<double> ex((size_t)B);
    for (i64 b = 0; b < B; ++b)
        ex[(size_t)b] = (double)S * (double)(sbc_bin_start(b + 1, B, L) - sbc_bin_start(b, B, L)) / (double)(L + 1);
    if (expected) memcpy(expected, ex.data(), sizeof(double) * (size_t)B);
    std::vector<i64> sorted((size_t)S);
    for (i64 p = 0; p < P; ++p) {
        double c2, ec;
        if (!sbc_uniform_column(reinterpret_cast<const i64*>(ranks) + p, S, P, L, B, ex.data(), sorted, counts ? reinterpret_cast<i64*>(counts) + p * B : nullptr, c2, ec))
            return MCR_EINVAL;
        if (chi2) chi2[p] = c2;
        if (pvalue) pvalue[p] = mcr_chi2_sf(c2, (double)(B - 1));
        if (ecdf_dev) ecdf_dev[p] = ec;
    }
    return MCR_OK;
}

// ---- Autocorrelation functions and times (mcr_acf.hpp) ---------------------------------------------------------------------
static_assert(kAcfMaxLag == MCR_ACF_MAX_LAG && kAcfBlock == MCR_ACF_BLOCK, "mcmcref_hip.h states the lag limit and the block");

// The workspace of a chunk of pc parameters: the ingest copy (returned), the chains' means, the blocks' lag products, the
// chains' gamma.
struct AcfChunk {
    const Tensor& t; AcfGeom g;
    double *mean = nullptr, *part = nullptr, *gam = nullptr;
    double* operator()(Carve& cv, i64 pc)
    {
        const size_t chains = (size_t)pc * (size_t)t.C;
        double* X = t.ingest() ? cv.take<double>(chains * (size_t)t.N) : nullptr;
        mean = cv.take<double>(chains);
        part = cv.take<double>(chains * (size_t)g.nblk * (size_t)g.lp);
        gam = cv.take<double>(chains * (size_t)g.lp);
        return X;
    }
};

// Parameters per workspace chunk of an autocorrelation call: what fits, and no more than k_acf_products' grid holds.
static int plan_acf(mcr_ctx* ctx, AcfChunk& ch, i64& pcmax)
{
    return plan_params(ctx, ch.t.P, ((i64)0x7FFFFFFFll / (ch.g.nbg * ch.g.nlb)) / 8 * 8, ch, pcmax);
}

// The lag, flag and window arguments of a call on chains of N draws (`ctx` NULL: the host routine's, no message kept).
static int acf_check_args(mcr_ctx* ctx, i64 N, i64 L, int flags, double wc)
{
    if (L < 0) return fail(ctx, MCR_EINVAL, "max_lag = %lld: a maximum lag must be >= 0", (long long)L);
    if (L > kAcfMaxLag) return fail(ctx, MCR_EINVAL, "max_lag = %lld exceeds MCR_ACF_MAX_LAG = %lld", (long long)L, (long long)kAcfMaxLag);
    if (N >= 1 && L > N - 1) return fail(ctx, MCR_EINVAL, "max_lag = %lld exceeds N - 1 = %lld", (long long)L, (long long)(N - 1));
    if (flags & ~MCR_ACF_UNBIASED) return fail(ctx, MCR_EINVAL, "unknown flag bits 0x%x", (unsigned)(flags & ~MCR_ACF_UNBIASED));
    if (!std::isfinite(wc) || !(wc > 0.0)) return fail(ctx, MCR_EINVAL, "window_c = %g: the window constant must be finite and > 0", wc);
    return MCR_OK;
}

// An empty chain (or none): NaN and -1 everywhere.
static void acf_fill_nan(const mcr_acf_out* o, i64 C, i64 P, i64 L)
{
    const i64 pcn = P * C;
    if (o->acf) for (i64 k = 0; k < pcn * (L + 1); ++k) o->acf[k] = NAN;
    for (double* a : {o->var, o->tau})
        if (a) for (i64 k = 0; k < pcn; ++k) a[k] = NAN;
    if (o->window) for (i64 k = 0; k < pcn; ++k) o->window[k] = -1;
    if (o->acf_pooled) for (i64 k = 0; k < P * (L + 1); ++k) o->acf_pooled[k] = NAN;
    if (o->tau_pooled) for (i64 p = 0; p < P; ++p) o->tau_pooled[p] = NAN;
    if (o->window_pooled) for (i64 p = 0; p < P; ++p) o->window_pooled[p] = -1;
}

static int acf_run(mcr_ctx* ctx, const Tensor& t, i64 L, int flags, double wc, const mcr_acf_out* out)
{
    const i64 C = t.C, N = t.N, P = t.P;
    AcfChunk ch{t, acf_geom(N, L)};
    const AcfGeom& g = ch.g;
    i64 pcmax = 0;
    int rc = plan_acf(ctx, ch, pcmax);
    if (rc) return rc;
    const size_t pcn = (size_t)P * (size_t)C, nl = (size_t)(L + 1);
    double *d_acf = nullptr, *d_var, *d_tau, *d_bad, *d_acfp, *d_taup;
    i64 *d_win, *d_winp;
    rc = carve(ctx, ctx->call_dev, [&](Carve& cv) {
        d_acf = out->acf ? cv.take<double>(pcn * nl) : nullptr;
        d_var = cv.take<double>(pcn); d_tau = cv.take<double>(pcn); d_win = cv.take<i64>(pcn); d_bad = cv.take<double>(pcn);
        d_acfp = cv.take<double>((size_t)P * nl); d_taup = cv.take<double>((size_t)P); d_winp = cv.take<i64>((size_t)P);
    });
    if (!rc) rc = ctx->call_host.reserve(ctx, sizeof(double) * pcn);
    if (rc) return rc;
    // the chains of a launch lie along y and z (any C), four per workgroup in k_acf_mean
    auto chain_grid = [](i64 n, unsigned gx) { const i64 gy = n < kMaxGridY ? n : kMaxGridY; return dim3(gx, (unsigned)gy, (unsigned)((n + gy - 1) / gy)); };
    const size_t lds = sizeof(double) * acf_lds_doubles(g), lds_fin = sizeof(double) * nl;
    rc = tensor_chunks(ctx, t, pcmax, ch, [&](i64 pc, i64 p0, const double* X) -> int {
        const unsigned gx = (unsigned)((pc + 7) / 8 * 8);
        const size_t at = (size_t)p0 * (size_t)C;
        LAUNCH(ctx, K_ACF_MEAN, k_acf_mean, chain_grid((C + 3) / 4, gx), dim3(256), 0, X, C, N, pc, ch.mean, d_bad + at);
        LAUNCH(ctx, K_ACF_PRODUCTS, k_acf_products, chain_grid(C, (unsigned)(gx * g.nbg * g.nlb)), dim3((unsigned)acf_threads(g)), lds,
               X, (const double*)ch.mean, C, N, pc, g, ch.part);
        LAUNCH(ctx, K_ACF_FINISH, k_acf_finish, chain_grid(C, gx), dim3(kAcfFinNT), lds_fin, (const double*)ch.part, C, N, pc, L, g,
               flags & MCR_ACF_UNBIASED, wc, ch.gam, d_acf ? d_acf + at * nl : nullptr, d_var + at, d_tau + at, d_win + at);
        LAUNCH(ctx, K_ACF_POOL, k_acf_pool, dim3(gx), dim3(kAcfFinNT), lds_fin, (const double*)ch.gam, C, pc, L, g.lp, wc,
               d_acfp + (size_t)p0 * nl, d_taup + p0, d_winp + p0);
        return MCR_OK;
    });
    if (rc) return rc;
    double* h_bad = ctx->call_host.as<double>();
    auto fetch = [&](void* dst, const void* src, size_t bytes) {
        return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
    };
    HIP_TRY(ctx, fetch(h_bad, d_bad, sizeof(double) * pcn));
    HIP_TRY(ctx, fetch(out->acf, d_acf, sizeof(double) * pcn * nl));
    HIP_TRY(ctx, fetch(out->var, d_var, sizeof(double) * pcn));
    HIP_TRY(ctx, fetch(out->tau, d_tau, sizeof(double) * pcn));
    HIP_TRY(ctx, fetch(out->window, d_win, sizeof(i64) * pcn));
    HIP_TRY(ctx, fetch(out->acf_pooled, d_acfp, sizeof(double) * (size_t)P * nl));
    HIP_TRY(ctx, fetch(out->tau_pooled, d_taup, sizeof(double) * (size_t)P));
    HIP_TRY(ctx, fetch(out->window_pooled, d_winp, sizeof(i64) * (size_t)P));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    double nbad = 0.0;
    for (size_t k = 0; k < pcn; ++k) nbad += h_bad[k];
    if (nbad > 0.0) return fail(ctx, MCR_ENONFINITE, "draws contain %.0f non-finite value(s)", nbad);
    return MCR_OK;
}

int mcr_autocorr_plan(mcr_ctx* ctx, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp,
                      int64_t max_lag, int64_t* params_per_chunk)
{
    const Tensor t{nullptr, dtype, C, N, P, sc, sn, sp};
    return plan_entry(ctx, "mcr_autocorr_plan", t, params_per_chunk, [&](i64& pcmax) {
        const int rc = acf_check_args(ctx, N, max_lag, 0, 1.0);
        if (rc) return rc;
        AcfChunk ch{t, acf_geom(N, max_lag)};
        return plan_acf(ctx, ch, pcmax);
    });
}

static int acf_entry(mcr_ctx* ctx, const Tensor& t, i64 L, int flags, double wc, mcr_acf_out* out, bool host)
{
    return tensor_entry(ctx, "mcr_autocorr", t, out, host, [&] { return acf_check_args(ctx, t.N, L, flags, wc); },
                        [&] { acf_fill_nan(out, t.C, t.P, L); }, [&](const Tensor& dev) { return acf_run(ctx, dev, L, flags, wc, out); });
}

int mcr_autocorr_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn,
                     int64_t sp, int64_t max_lag, int flags, double window_c, mcr_acf_out* out)
{
    return acf_entry(ctx, {draws_dev, dtype, C, N, P, sc, sn, sp}, max_lag, flags, window_c, out, false);
}

int mcr_autocorr(mcr_ctx* ctx, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp,
                 int64_t max_lag, int flags, double window_c, mcr_acf_out* out)
{
    return acf_entry(ctx, {draws, dtype, C, N, P, sc, sn, sp}, max_lag, flags, window_c, out, true);
}

int mcr_autocorr_host(const double* chains, int64_t C, int64_t N, int64_t max_lag, int flags, double window_c, mcr_acf_out* out)
{
    if (!out || C < 0 || N < 0 || (N > 0 && (C > (i64)0x7FFFFFFFll / N || C * N >= (i64)0x7FFFFFFFll)) || (C * N > 0 && !chains)) return MCR_EINVAL;
    const i64 L = max_lag;
    const int rc = acf_check_args(nullptr, N, L, flags, window_c);
    if (rc) return rc;
    if (C * N == 0) { acf_fill_nan(out, C, 1, L); return MCR_OK; }
    const bool unbiased = (flags & MCR_ACF_UNBIASED) != 0;
    const i64 nblk = (N + kAcfBlock - 1) / kAcfBlock;
    std::vector<double> d((size_t)N), gam((size_t)(L + 1)), rho((size_t)(L + 1)), pool((size_t)(L + 1), 0.0);
    i64 nbad = 0;
    for (i64 c = 0; c < C; ++c) {
        const double* x = chains + c * N;
        double v[kWave];
        for (int j = 0; j < kWave; ++j) v[j] = acf_lane_sum(x, N, j, &nbad);
        for (int o = kWave >> 1; o > 0; o >>= 1)                       // the xor tree, as lane 0 sees it
            for (int j = 0; j < o; ++j) v[j] = v[j] + v[j + o];
        const double m = v[0] / (double)N;
        for (i64 i = 0; i < N; ++i) d[(size_t)i] = x[i] - m;
        for (i64 l = 0; l <= L; ++l) {
            double S = 0.0;
            for (i64 b = 0; b < nblk; ++b) {
                const i64 i0 = b * kAcfBlock, i1 = i0 + kAcfBlock < N - l ? i0 + kAcfBlock : N - l;
                double acc = 0.0;
                for (i64 i = i0; i < i1; ++i) acc = fma(d[(size_t)i], d[(size_t)(i + l)], acc);
                S += acc;
            }
            gam[(size_t)l] = acf_gamma(S, N, l, unbiased);
            pool[(size_t)l] += gam[(size_t)l];
        }
        for (i64 l = 0; l <= L; ++l) rho[(size_t)l] = acf_rho(gam[(size_t)l], gam[0]);
        double t;
        i64 w;
        acf_tau_scan(rho.data(), L, window_c, t, w);
        if (out->acf) memcpy(out->acf + c * (L + 1), rho.data(), sizeof(double) * (size_t)(L + 1));
        if (out->var) out->var[c] = gam[0];
        if (out->tau) out->tau[c] = t;
        if (out->window) out->window[c] = w;
    }
    for (i64 l = 0; l <= L; ++l) pool[(size_t)l] = pool[(size_t)l] / (double)C;
    for (i64 l = 0; l <= L; ++l) rho[(size_t)l] = acf_rho(pool[(size_t)l], pool[0]);
    double t;
    i64 w;
    acf_tau_scan(rho.data(), L, window_c, t, w);
    if (out->acf_pooled) memcpy(out->acf_pooled, rho.data(), sizeof(double) * (size_t)(L + 1));
    if (out->tau_pooled) *out->tau_pooled = t;
    if (out->window_pooled) *out->window_pooled = w;
    return nbad > 0 ? MCR_ENONFINITE : MCR_OK;
}

// The covariance of one sample as a plan, a layout and its launches, so that mcr_covariance_dev and the Gaussian check
// (which carves once for everything it does) run the same kernels on the same geometry.
struct CovPlan { int nb, ksplit; i64 P64, tiles, kchunk; };
struct CovWs { double *partial, *mpart, *mean, *std; };
constexpr int kCovMomS = 8;

static CovPlan cov_plan(i64 M, i64 P)
{
    CovPlan c;
    c.nb = (int)((P + kCovBM - 1) / kCovBM);
    c.P64 = (i64)c.nb * kCovBM;
    c.tiles = (i64)c.nb * (c.nb + 1) / 2;                            // workgroups per draw slice (none below the diagonal)
    int ksplit = (int)((512 + c.tiles - 1) / c.tiles);               // >= ~512 workgroups: two per CU
    const i64 maxsplit = (M + 16 * kCovBK - 1) / (16 * kCovBK);      // a slice is at least 16 panels long
    if (ksplit > maxsplit) ksplit = (int)maxsplit;
    {   // the slices' partial tiles are summed by k_cov_final: at most 128 MB of them
        const i64 cap = ((i64)128 << 20) / (c.P64 * c.P64 * 8);
        if (ksplit > cap) ksplit = (int)(cap < 1 ? 1 : cap);
    }
    if (ksplit < 1) ksplit = 1;
    i64 kchunk = (M + ksplit - 1) / ksplit;
    c.kchunk = (kchunk + kCovBK - 1) / kCovBK * kCovBK;
    c.ksplit = (int)((M + c.kchunk - 1) / c.kchunk);
    return c;
}

static void carve_cov(Carve& cv, CovWs& w, const CovPlan& c, i64 P)
{
    w.partial = cv.take<double>((size_t)c.ksplit * c.P64 * c.P64);
    w.mpart = cv.take<double>((size_t)P * kCovMomS * kMomRec);
    w.mean = cv.take<double>((size_t)P);
    w.std = cv.take<double>((size_t)P);
}

// k_cov_mfma and k_cov_final around the given means on the current stream; no synchronisation.  partial may be larger than
// the plan needs.
static int cov_tiles_launch(mcr_ctx* ctx, const double* draws_dev, i64 M, i64 P, const CovPlan& c, const double* mean,
                            double* partial, double* cov_dev)
{
    if ((M & 1) == 0 && (reinterpret_cast<uintptr_t>(draws_dev) & 15) == 0) {
        LAUNCH(ctx, K_COV, (k_cov_mfma<true>), dim3((unsigned)c.tiles, (unsigned)c.ksplit), dim3(256), 0, draws_dev,
               mean, (i64)M, (i64)P, c.nb, c.kchunk, partial);
    } else {
        LAUNCH(ctx, K_COV, (k_cov_mfma<false>), dim3((unsigned)c.tiles, (unsigned)c.ksplit), dim3(256), 0, draws_dev,
               mean, (i64)M, (i64)P, c.nb, c.kchunk, partial);
    }
    LAUNCH(ctx, K_COV_FINAL, k_cov_final, dim3((unsigned)((P * P + 255) / 256)), dim3(256), 0, (const double*)partial,
           c.ksplit, c.nb, (i64)M, (i64)P, cov_dev);
    return MCR_OK;
}

// The streaming moments, then the tiles around their means: mcr_covariance.
static int cov_launch(mcr_ctx* ctx, const double* draws_dev, i64 M, i64 P, const CovPlan& c, const CovWs& w, double* cov_dev)
{
    const int rc = moments_rows(ctx, draws_dev, M, P, w.mean, w.std, w.mpart, (M >= 8 * 2048) ? kCovMomS : 1);
    return rc ? rc : cov_tiles_launch(ctx, draws_dev, M, P, c, w.mean, w.partial, cov_dev);
}

// Device-resident form (draws_dev [P][M] f64, cov_dev [P][P] f64, both in this context's device memory): what
// tools/cov_bench.py times.  Synchronous.
int mcr_covariance_dev(mcr_ctx* ctx, const double* draws_dev, int64_t M, int64_t P, double* cov_dev)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (P < 0 || M < 1 || (P > 0 && (!draws_dev || !cov_dev))) return fail(ctx, MCR_EINVAL, "bad argument");
    if (P == 0) return MCR_OK;
    if (P > 8192) return fail(ctx, MCR_EINVAL, "P > 8192 not supported by mcr_covariance");
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "mcr_covariance with summaries in flight");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const CovPlan c = cov_plan(M, P);
    CovWs w;
    int rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) { carve_cov(cv, w, c, P); });
    if (rc) return rc;
    rc = cov_launch(ctx, draws_dev, M, P, c, w, cov_dev);
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    return MCR_OK;
}

int mcr_covariance(mcr_ctx* ctx, const double* draws, int64_t M, int64_t P, double* cov)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (P < 0 || M < 1 || (P > 0 && (!draws || !cov))) return fail(ctx, MCR_EINVAL, "bad argument");
    if (P == 0) return MCR_OK;
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "mcr_covariance with summaries in flight");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    void* buf[2];
    int rc = stage_buffers(ctx, {sizeof(double) * (size_t)P * M, sizeof(double) * (size_t)P * P}, buf);
    if (rc) return rc;
    double *X = (double*)buf[0], *d_cov = (double*)buf[1];
    HIP_TRY(ctx, hipMemcpyAsync(X, draws, sizeof(double) * (size_t)P * M, hipMemcpyHostToDevice, ctx->stream));
    rc = mcr_covariance_dev(ctx, X, M, P, d_cov);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(cov, d_cov, sizeof(double) * (size_t)P * P, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MCR_OK;
}

// ---- the extension entries (include/mcmcref_hip_ext.h, mcr_gauss.hpp): Cholesky, lower solve, Gaussian check ----------
static_assert(kCholNB == MCRX_CHOL_NB && kLinalgMaxP == MCRX_LINALG_MAX_P && kGaussOut == MCRX_G_OUT,
              "mcmcref_hip_ext.h states the block size, the order limit and the number of outputs");

// The order and a row stride of a matrix argument: MCR_EINVAL with the cause, else MCR_OK.
static int linalg_check(mcr_ctx* ctx, const char* who, i64 P, const char* ld_name, i64 ld, i64 ld_min)
{
    if (P < 0) return fail(ctx, MCR_EINVAL, "%s: P = %lld is negative", who, P);
    if (P > kLinalgMaxP) return fail(ctx, MCR_EINVAL, "%s: P = %lld is over MCRX_LINALG_MAX_P = %lld", who, P, kLinalgMaxP);
    if (ld < ld_min) return fail(ctx, MCR_EINVAL, "%s: %s = %lld is smaller than the row length %lld", who, ld_name, ld, ld_min);
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "%s with summaries in flight", who);
    return MCR_OK;
}

// The factorisation's launches on the current stream, in place on A: 3 ceil(P / NB) - 1 of them, no synchronisation.
// *info_dev is 0 on entry (a set word makes every kernel but the finisher return at once).
static int chol_launch(mcr_ctx* ctx, double* A, i64 P, i64 lda, i64* info_dev, double* logdet_dev)
{
    const i64 nblk = (P + kCholNB - 1) / kCholNB;
    for (i64 b = 0; b < nblk; ++b) {
        const i64 k0 = b * kCholNB, m = nblk - b - 1;             // m block rows under the diagonal block
        LAUNCH(ctx, K_CHOL_PANEL, k_chol_panel, dim3(1), dim3(kCholNB), 0, A, P, lda, k0, info_dev);
        if (m == 0) break;
        LAUNCH(ctx, K_CHOL_BELOW, k_chol_below, dim3((unsigned)m), dim3(kCholNB), 0, A, P, lda, k0, (const i64*)info_dev);
        LAUNCH(ctx, K_CHOL_UPDATE, k_chol_update, dim3((unsigned)(m * (m + 1) / 2)), dim3(256), 0, A, P, lda, k0, (const i64*)info_dev);
    }
    LAUNCH(ctx, K_CHOL_FINISH, k_chol_finish, dim3((unsigned)((P * P + 255) / 256)), dim3(256), 0, A, P, lda,
           (const i64*)info_dev, logdet_dev);
    return MCR_OK;
}

static int solve_launch(mcr_ctx* ctx, const double* L, i64 P, i64 ldl, double* B, i64 K, i64 ldb, const i64* info0, const i64* info1)
{
    LAUNCH(ctx, K_SOLVE_LOWER, k_solve_lower, dim3((unsigned)((K + kCholNB - 1) / kCholNB)), dim3(256), 0, L, P, ldl, B, K, ldb,
           info0, info1);
    return MCR_OK;
}

// mcrx_cholesky_dev behind its argument check, P > 0: the status words from the lane's workspace, the launches, the results.
static int chol_run(mcr_ctx* ctx, double* a_dev, i64 P, i64 lda, int64_t* info, double* logdet)
{
    i64* d_info; double* d_logdet;
    int rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) { d_info = cv.take<i64>(1); d_logdet = cv.take<double>(1); });
    if (rc) return rc;
    HIP_TRY(ctx, hipMemsetAsync(d_info, 0, sizeof(i64), ctx->stream));
    rc = chol_launch(ctx, a_dev, P, lda, d_info, d_logdet);
    if (rc) return rc;
    i64 h_info = 0; double h_logdet = 0.0;
    HIP_TRY(ctx, hipMemcpyAsync(&h_info, d_info, sizeof(i64), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&h_logdet, d_logdet, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    if (info) *info = h_info;
    if (logdet) *logdet = h_logdet;
    return MCR_OK;
}

int mcrx_cholesky_dev(mcr_ctx* ctx, double* a_dev, int64_t P, int64_t lda, int64_t* info, double* logdet)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    const int rc = linalg_check(ctx, "mcrx_cholesky", P, "lda", lda, P);
    if (rc) return rc;
    if (P == 0) { if (info) *info = 0; if (logdet) *logdet = 0.0; return MCR_OK; }
    if (!a_dev) return fail(ctx, MCR_EINVAL, "mcrx_cholesky: NULL argument (a)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return chol_run(ctx, a_dev, P, lda, info, logdet);
}

int mcrx_cholesky(mcr_ctx* ctx, const double* a, int64_t P, int64_t lda, double* l, int64_t* info, double* logdet)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    int rc = linalg_check(ctx, "mcrx_cholesky", P, "lda", lda, P);
    if (rc) return rc;
    if (P == 0) { if (info) *info = 0; if (logdet) *logdet = 0.0; return MCR_OK; }
    if (!a || !l) return fail(ctx, MCR_EINVAL, "mcrx_cholesky: NULL argument (%s)", !a ? "a" : "l");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    void* buf[1];
    rc = stage_buffers(ctx, {sizeof(double) * (size_t)P * P}, buf);
    if (rc) return rc;
    double* A = (double*)buf[0];
    const size_t row = sizeof(double) * (size_t)P;
    HIP_TRY(ctx, hipMemcpy2DAsync(A, row, a, sizeof(double) * (size_t)lda, row, (size_t)P, hipMemcpyHostToDevice, ctx->stream));
    rc = chol_run(ctx, A, P, P, info, logdet);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(l, A, row * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MCR_OK;
}

int mcrx_cholesky_host(const double* a, int64_t P, int64_t lda, double* l, int64_t* info, double* logdet)
{
    i64 bad = 0;
    if (chol_host(a, P, lda, l, &bad, logdet)) return MCR_EINVAL;
    if (info) *info = bad;
    return MCR_OK;
}

static int solve_check(mcr_ctx* ctx, i64 P, i64 ldl, i64 K, i64 ldb)
{
    if (K < 0) return fail(ctx, MCR_EINVAL, "mcrx_solve_lower: K = %lld is negative", K);
    if (P >= 0 && ldb < K) return fail(ctx, MCR_EINVAL, "mcrx_solve_lower: ldb = %lld is smaller than the row length %lld", ldb, K);
    return linalg_check(ctx, "mcrx_solve_lower", P, "ldl", ldl, P);
}

int mcrx_solve_lower_dev(mcr_ctx* ctx, const double* l_dev, int64_t P, int64_t ldl, double* b_dev, int64_t K, int64_t ldb)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    int rc = solve_check(ctx, P, ldl, K, ldb);
    if (rc) return rc;
    if (P == 0 || K == 0) return MCR_OK;
    if (!l_dev || !b_dev) return fail(ctx, MCR_EINVAL, "mcrx_solve_lower: NULL argument (%s)", !l_dev ? "l" : "b");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = solve_launch(ctx, l_dev, P, ldl, b_dev, K, ldb, nullptr, nullptr);
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    return MCR_OK;
}

int mcrx_solve_lower(mcr_ctx* ctx, const double* l, int64_t P, int64_t ldl, const double* b, int64_t K, int64_t ldb, double* x)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    int rc = solve_check(ctx, P, ldl, K, ldb);
    if (rc) return rc;
    if (P == 0 || K == 0) return MCR_OK;
    if (!l || !b || !x) return fail(ctx, MCR_EINVAL, "mcrx_solve_lower: NULL argument (%s)", !l ? "l" : !b ? "b" : "x");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    void* buf[2];
    rc = stage_buffers(ctx, {sizeof(double) * (size_t)P * P, sizeof(double) * (size_t)P * K}, buf);
    if (rc) return rc;
    double *L = (double*)buf[0], *B = (double*)buf[1];
    const size_t lrow = sizeof(double) * (size_t)P, brow = sizeof(double) * (size_t)K;
    HIP_TRY(ctx, hipMemcpy2DAsync(L, lrow, l, sizeof(double) * (size_t)ldl, lrow, (size_t)P, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpy2DAsync(B, brow, b, sizeof(double) * (size_t)ldb, brow, (size_t)P, hipMemcpyHostToDevice, ctx->stream));
    rc = solve_launch(ctx, L, P, P, B, K, K, nullptr, nullptr);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(x, B, brow * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    return MCR_OK;
}

int mcrx_solve_lower_host(const double* l, int64_t P, int64_t ldl, const double* b, int64_t K, int64_t ldb, double* x)
{
    return solve_lower_host(l, P, ldl, b, K, ldb, x) ? MCR_EINVAL : MCR_OK;
}

// The workspace of a Gaussian check, carved once: the covariance's partials (the larger of the two samples' plans), both
// samples' means, both matrices (factored in place), W -- each
// covariance before its scaled gather, then each solve result --, the right-hand sides, the rows' sums, the live
// parameters' scales and indices, the six sums and the two status words.
struct GaussWs {
    double *partial, *mean_ref, *mean_act, *Cr, *Ca, *W, *yr, *ya, *rows_r, *rows_a, *s, *res; int* idx; i64* info;
};

static void carve_gauss(Carve& cv, GaussWs& w, const CovPlan& cr, const CovPlan& ca, i64 P)
{
    w.partial = cv.take<double>((size_t)(cr.ksplit >= ca.ksplit ? cr.ksplit : ca.ksplit) * cr.P64 * cr.P64);      // (P64 is the same)
    w.mean_ref = cv.take<double>((size_t)P);
    w.mean_act = cv.take<double>((size_t)P);
    w.Cr = cv.take<double>((size_t)P * P);
    w.Ca = cv.take<double>((size_t)P * P);
    w.W = cv.take<double>((size_t)P * P);
    w.yr = cv.take<double>((size_t)P);
    w.ya = cv.take<double>((size_t)P);
    w.rows_r = cv.take<double>((size_t)P);
    w.rows_a = cv.take<double>((size_t)P);
    w.s = cv.take<double>((size_t)P);
    w.idx = cv.take<int>((size_t)P);
    w.res = cv.take<double>(6);
    w.info = cv.take<i64>(2);
}

static int gauss_shape_check(mcr_ctx* ctx, i64 Mr, i64 Ma, i64 P)
{
    if (P < 0) return fail(ctx, MCR_EINVAL, "mcrx_gaussian_check: P = %lld is negative", P);
    if (P > kLinalgMaxP) return fail(ctx, MCR_EINVAL, "mcrx_gaussian_check: P = %lld is over MCRX_LINALG_MAX_P = %lld", P, kLinalgMaxP);
    if (Mr < 1 || Ma < 1) return fail(ctx, MCR_EINVAL, "mcrx_gaussian_check: both samples need at least one draw (Mr = %lld, Ma = %lld)", Mr, Ma);
    return MCR_OK;
}

// Everything but the shape, for P > 0.
static int gauss_check(mcr_ctx* ctx, const void* ref, const void* act, i64 P, const double* scale, double jitter,
                       const double* out, const int64_t* info3)
{
    if (!ref || !act || !out || !info3)
        return fail(ctx, MCR_EINVAL, "mcrx_gaussian_check: NULL argument (%s)", !ref ? "ref" : !act ? "act" : !out ? "out8" : "info3");
    if (!(jitter >= 0.0) || std::isinf(jitter)) return fail(ctx, MCR_EINVAL, "mcrx_gaussian_check: jitter is negative or not finite");
    for (i64 p = 0; scale && p < P; ++p)
        if (!(scale[p] >= 0.0) || std::isinf(scale[p]))
            return fail(ctx, MCR_EINVAL, "mcrx_gaussian_check: scale[%lld] is negative or not finite", (long long)p);
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "mcrx_gaussian_check with summaries in flight");
    return MCR_OK;
}

int mcrx_gaussian_workspace(mcr_ctx* ctx, int64_t Mr, int64_t Ma, int64_t P, size_t* bytes)
{
    if (!ctx || !bytes) return fail(ctx, MCR_EINVAL, "mcrx_gaussian_workspace: NULL argument");
    const int rc = gauss_shape_check(ctx, Mr, Ma, P);
    if (rc) return rc;
    *bytes = 0;
    if (P == 0) return MCR_OK;
    Carve m{nullptr};
    GaussWs w;
    carve_gauss(m, w, cov_plan(Mr, P), cov_plan(Ma, P), P);
    *bytes = m.off;
    return MCR_OK;
}

int mcrx_gaussian_check_dev(mcr_ctx* ctx, const double* ref_dev, int64_t Mr, const double* act_dev, int64_t Ma, int64_t P,
                            const double* scale, double jitter, double* out8, int64_t* info3, double* shift)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    int rc = gauss_shape_check(ctx, Mr, Ma, P);
    if (rc) return rc;
    if (P == 0) return MCR_OK;
    rc = gauss_check(ctx, ref_dev, act_dev, P, scale, jitter, out8, info3);
    if (rc) return rc;
    std::vector<int> idx;
    std::vector<double> s;
    gauss_live(scale, P, idx, s);
    const i64 PL = (i64)idx.size();
    info3[MCRX_G_P_LIVE] = PL; info3[MCRX_G_INFO_REF] = info3[MCRX_G_INFO_ACT] = 0;
    if (PL == 0) { gauss_outputs(out8, 0, 0, 0); return MCR_OK; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const CovPlan cr = cov_plan(Mr, P), ca = cov_plan(Ma, P);
    GaussWs w;
    { Carve m{nullptr}; carve_gauss(m, w, cr, ca, P);
      if (m.off > ctx->ws_limit)
          return fail(ctx, MCR_ENOMEM, "workspace limit too small: the Gaussian check of this shape needs %zu bytes, the limit is %zu",
                      m.off, ctx->ws_limit); }
    rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) { carve_gauss(cv, w, cr, ca, P); });
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(w.s, s.data(), sizeof(double) * (size_t)PL, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(w.idx, idx.data(), sizeof(int) * (size_t)PL, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(w.info, 0, 2 * sizeof(i64), ctx->stream));
    const i64 *info_r = w.info, *info_a = w.info + 1;
    const dim3 gather((unsigned)((PL * PL + 255) / 256));
    const double* none = nullptr;
    // both covariances through W into their scaled, gathered matrices; the second gather also makes the mean shift.  The
    // means are k_row_mean's, not the streaming moments' (whose summation order follows the rows' alignment).
    LAUNCH(ctx, K_ROW_MEAN, k_row_mean, dim3((unsigned)P), dim3(256), 0, ref_dev, (i64)Mr, w.mean_ref);
    rc = cov_tiles_launch(ctx, ref_dev, Mr, P, cr, w.mean_ref, w.partial, w.W);
    if (rc) return rc;
    LAUNCH(ctx, K_SYM_SCALE, k_sym_scale, gather, dim3(256), 0, (const double*)w.W, (i64)P, (const double*)w.s, (const int*)w.idx, PL,
           jitter, w.Cr, none, none, (double*)nullptr, (double*)nullptr);
    LAUNCH(ctx, K_ROW_MEAN, k_row_mean, dim3((unsigned)P), dim3(256), 0, act_dev, (i64)Ma, w.mean_act);
    rc = cov_tiles_launch(ctx, act_dev, Ma, P, ca, w.mean_act, w.partial, w.W);
    if (rc) return rc;
    LAUNCH(ctx, K_SYM_SCALE, k_sym_scale, gather, dim3(256), 0, (const double*)w.W, (i64)P, (const double*)w.s, (const int*)w.idx, PL,
           jitter, w.Ca, (const double*)w.mean_ref, (const double*)w.mean_act, w.yr, w.ya);
    // the factors (their log-determinants land in res[4], res[5]) and the whitened mean shifts
    rc = chol_launch(ctx, w.Cr, PL, PL, w.info, w.res + 4);
    if (!rc) rc = chol_launch(ctx, w.Ca, PL, PL, w.info + 1, w.res + 5);
    if (!rc) rc = solve_launch(ctx, w.Cr, PL, PL, w.yr, 1, 1, info_r, nullptr);
    if (!rc) rc = solve_launch(ctx, w.Ca, PL, PL, w.ya, 1, 1, info_a, nullptr);
    if (rc) return rc;
    // |L_r^-1 L_a|_F^2 and |L_a^-1 L_r|_F^2: a copy of the other factor is the right-hand side
    const size_t mat = sizeof(double) * (size_t)PL * PL;
    HIP_TRY(ctx, hipMemcpyAsync(w.W, w.Ca, mat, hipMemcpyDeviceToDevice, ctx->stream));
    rc = solve_launch(ctx, w.Cr, PL, PL, w.W, PL, PL, info_r, info_a);
    if (rc) return rc;
    LAUNCH(ctx, K_ROW_SUMSQ, k_row_sumsq, dim3((unsigned)PL), dim3(256), 0, (const double*)w.W, PL, PL, w.rows_r, info_r, info_a);
    HIP_TRY(ctx, hipMemcpyAsync(w.W, w.Cr, mat, hipMemcpyDeviceToDevice, ctx->stream));
    rc = solve_launch(ctx, w.Ca, PL, PL, w.W, PL, PL, info_r, info_a);
    if (rc) return rc;
    LAUNCH(ctx, K_ROW_SUMSQ, k_row_sumsq, dim3((unsigned)PL), dim3(256), 0, (const double*)w.W, PL, PL, w.rows_a, info_r, info_a);
    LAUNCH(ctx, K_GAUSS_SUMS, k_gauss_sums, dim3(1), dim3(256), 0, (const double*)w.yr, (const double*)w.ya, (const double*)w.rows_r,
           (const double*)w.rows_a, PL, w.res);
    double res[6];
    i64 info[2];
    HIP_TRY(ctx, hipMemcpyAsync(res, w.res, sizeof(res), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(info, w.info, sizeof(info), hipMemcpyDeviceToHost, ctx->stream));
    if (shift) HIP_TRY(ctx, hipMemcpyAsync(shift, w.yr, sizeof(double) * (size_t)PL, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    memcpy(out8, res, sizeof(res));
    gauss_outputs(out8, PL, info[0], info[1]);
    info3[MCRX_G_INFO_REF] = info[0];
    info3[MCRX_G_INFO_ACT] = info[1];
    if (shift && info[0]) for (i64 i = 0; i < PL; ++i) shift[i] = std::numeric_limits<double>::quiet_NaN();
    return MCR_OK;
}

int mcrx_gaussian_check(mcr_ctx* ctx, const double* ref, int64_t Mr, const double* act, int64_t Ma, int64_t P,
                        const double* scale, double jitter, double* out8, int64_t* info3, double* shift)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    int rc = gauss_shape_check(ctx, Mr, Ma, P);
    if (rc) return rc;
    if (P == 0) return MCR_OK;
    rc = gauss_check(ctx, ref, act, P, scale, jitter, out8, info3);
    if (rc) return rc;
    const double *Xr, *Xa;
    rc = stage_two_samples(ctx, ref, Mr, act, Ma, P, &Xr, &Xa);
    if (rc) return rc;
    return mcrx_gaussian_check_dev(ctx, Xr, Mr, Xa, Ma, P, scale, jitter, out8, info3, shift);
}

int mcrx_gaussian_check_host(const double* ref, int64_t Mr, const double* act, int64_t Ma, int64_t P, const double* scale,
                             double jitter, double* out8, int64_t* info3, double* shift)
{
    try {
        i64 info[3] = {0, 0, 0};
        if (gauss_host(ref, Mr, act, Ma, P, scale, jitter, out8, info3 ? info : nullptr, shift)) return MCR_EINVAL;
        if (info3 && P > 0) for (int k = 0; k < 3; ++k) info3[k] = info[k];
        return MCR_OK;
    } catch (const std::exception&) {
        return MCR_ENOMEM;
    }
}

}  // extern "C"
