// mcr_pipe.hpp -- how another unit runs the summary pipeline of mcr_api.hip: the result table and the moment records its
// kernels write, a pipeline's arguments and carved buffers, and the functions that carve, sort and run it.  mcr_api.hip
// defines all of it and mcr_stats.hip is the other user; the kernel headers of the pipeline (mcr_kernels.hpp, and mcr_ext.hpp
// for the moment records) take the table and record formats from here.  Internal: not installed, no kernel in it.
#pragma once
#include "mcr_host.hpp"

namespace mcr {

// result table: SoA, res[field * P + p]
enum ResField {
    R_MEAN = 0, R_STD, R_MEDIAN, R_RHAT, R_RHAT_BULK, R_RHAT_TAIL, R_ESS_BULK, R_ESS_TAIL,
    R_LAG_BULK, R_LAG_TAIL, R_BAD, R_Q0  // R_Q0 .. R_Q0 + nq - 1
};

struct QArgs {
    int nq;
    i64 lo[32];
    double g[32];
    // the draws in time order, [pc][M] (f64, or f32 with xf32): only a median of exactly zero looks at them (wave_order_stats)
    const void* xt = nullptr;
    int xf32 = 0;
};

constexpr int kMomRec = 5;           // doubles of a slice's moment record (mcr_kernels.hpp: the moments kernels)

namespace host {

constexpr int kTile = 4096;          // pooled draws per sorted tile / bucket capacity

// The FFT tier of a call (plan_fft of mcr_api.hip); FftPlan{}: none.
struct FftPlan { bool on = false; int logN = 0, log1 = 0, log2 = 0, slots = 0, cb = 0; };

// (mcr_host.hpp names the type, for SummaryCall::last)
struct PipeIn {
    const void* X;       // [pc][M] contiguous: f64 (user tensor or ingest buffer) or, x_f32, the user's f32 tensor itself
    bool x_f32 = false;
    // f32 tensors take the packed records (k_tile_sort32, RecSlots<u64>) whenever the bucket partition applies (pooled arrays up to
    // 512 K draws) and MCR_F32_RECORDS is not 0; otherwise the tile sort widens the f32 draws and the f64 kernels run
    bool records = false;
    bool idx16 = false;  // M <= kIdx16Max: 16-bit positions through the sort (else 32-bit)
    i64 M, pc;
    int C;
    const i64* d_off;
    i64 n, nh;
    QArgs q;
    double* d_res;       // chunk's result table, stride pc
    // carved buffers
    double *kA, *kB, *part;
    u32 *zb, *zt;        // rank codes n2 of every draw in time order (z = ztab[n2], rank = (n2 + 1) / 2)
    void *iA, *iB;       // pooled-position payload of the sort: u16 when idx16, else u32
    i64* split;
    double* rec;         // [pc][2][C][nseg][kSegRec] first-pass segment records
    unsigned* more;      // [pc][2] continuation flags
    double* state;       // [pc][2][4] rho scan state
    double* chstate;     // [pc][2][C][kChState]
    double* rec2;        // [pc][2][C][nseg][64*kMoreBlocks] lag products of tier 2 (lags 64..255)
    double* acov;        // [pc][2][n] deviation products of tier 3 (lags >= 256), listed pairs only
    unsigned* long_count; // [1] number of pairs in the tier-3 list of this call
    unsigned* long_list;  // [2 pc]
    unsigned* t3c;        // [kT3Stages + 1][2 pc] k_tier3: per pair and stage the finished lag groups (+ kT3Prev), then "decided"
    FftPlan fft;          // FFT tier for long chains (mcr_fft.hpp): buffers shared by the chunks of a call
    double2 *fft_A = nullptr, *fft_B = nullptr; double* fft_S = nullptr;
    double2 *tw1 = nullptr, *tw2 = nullptr;
    i64 nstage;          // longest chain prefix the segment grid has to cover
    double* ztab;        // [2M] z of every possible tie run (shared by all parameters of the call)
    double* samp;        // [pc][ntiles][64] regular samples of the sorted tiles
    u32* cut;            // [pc][B+1][ntiles]
    u32* boff;           // [pc][B+1]
    int bk_B = 0, bk_D = 0, bk_k = 0;
    i64 bk_R = 0;
    i64 ntiles;
    bool do_diag = true;  // false: Backend.stats only (sort + order statistics + moments)
    bool fork = false;    // lone call: the bulk half of the diagnostics on the lane's second stream (run_pipeline)
};

// What the sort stage leaves: the ascending (key, position) order of every parameter in one of the two ping-pong buffer
// pairs, the other pair free, and whether the bulk rank codes z_bulk are written already (bucket path with do_diag).
// On the f32 records path the keys are packed (key, position) records and the positions are unused: pos / pos_free are then
// the two position buffers in no particular order (which is which depends on the number of merge passes), nothing may read them.
struct Sorted {
    double* keys; void* pos;
    double* keys_free; void* pos_free;
    bool ranked;
};

// Extent (in elements) touched by a strided tensor, or -1 if strides are negative.
inline i64 tensor_extent(i64 C, i64 N, i64 P, i64 sc, i64 sn, i64 sp)
{
    if (C == 0 || N == 0 || P == 0) return 0;
    if (sc < 0 || sn < 0 || sp < 0) return -1;
    return (C - 1) * sc + (N - 1) * sn + (P - 1) * sp + 1;
}

// Tensors in the Arrow column layout [P][C][N] are consumed in place, f64 and f32 alike (the tile sort widens f32 as it
// loads); anything else goes through one ingest pass into X[P][M] f64.
inline bool needs_ingest(i64 C, i64 N, i64 P, i64 sc, i64 sn, i64 sp)
{
    return !((N <= 1 || sn == 1) && (C <= 1 || sc == N) && (P <= 1 || sp == C * N));
}

// Defined once, in mcr_api.hip, where their comments are.
int get_ztab(mcr_ctx* ctx, i64 M, double** out);
double* carve_pipe(Carve& cv, PipeIn& a, bool records, const FftPlan& fp, bool ingest);
int sort_stage(mcr_ctx* ctx, PipeIn& a, Sorted& out);
int run_pipeline(mcr_ctx* ctx, PipeIn& a, Sorted* sorted_out = nullptr);
int launch_ingest(mcr_ctx* ctx, const void* src, int dtype, double* X, i64 C, i64 N, i64 pc, i64 sc, i64 sn, i64 sp, i64 p0, i64 nt = 1,
                  i64 ss = 0, i64 xs = 0);
int moments_rows(mcr_ctx* ctx, const double* src, i64 M, i64 P, double* d_mean, double* d_std, double* part, int S);
int stage_two_samples(mcr_ctx* ctx, const double* ref, i64 Mr, const double* act, i64 Ma, i64 P, const double** ref_dev,
                      const double** act_dev);

}  // namespace host
}  // namespace mcr
