// bm_host_check.cpp -- the host definitions of include/mcmcref_bm.h (mcb_batch_means_host, mcb_lrv_finish_host,
// mcb_pool_host, mcb_tree_sum_host, mcb_batch_size) as a stand-alone program, for sanitizer runs.  They live in
// mcb_api.hip, whose header holds the kernels, so the program is built from that unit with hipcc and the sanitizers are
// given to the host side alone; no device is opened:
//
//     hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -Iinclude -Wno-unused-value \
//         -x hip mcmc-db_amd/csrc/mcb_api.hip tools/bm_host_check.cpp -o bm_host_check && ./bm_host_check
//
// It walks the routines through their edges -- batch sizes around the lane, row and block edges of the tree, b = 1 and
// b = N, a dropped head, 1 and 3 chains, f32 and f64, every layout of the strides, a repeated chain, NULL outputs, every
// refusal -- with each tensor in a heap block of exactly its span, so that a read past either end is caught, and checks
// what is exact: a constant parameter, the batch-size rule, NaN for fewer than two batches, the compaction of the pool.
// Exit status 0: all held.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mcmcref_bm.h"

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static unsigned long long rng_state = 88172645463325252ull;
static double uniform()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}

template <class T>
static void means_case(int dtype, int64_t C, int64_t N, int64_t P, int64_t b, int layout)
{
    // layout 0: [P][C][N]; 1: [C][N][P]; 2: [P][C][2 N] thinned; 3: one chain repeated (stride_c = 0)
    int64_t sc, sn, sp;
    if (layout == 0) { sn = 1; sc = N; sp = C * N; }
    else if (layout == 1) { sp = 1; sn = P; sc = N * P; }
    else if (layout == 2) { sn = 2; sc = 2 * N; sp = 2 * C * N; }
    else { sn = 1; sc = 0; sp = N; }
    const size_t span = (size_t)((C - 1) * sc + (N - 1) * sn + (P - 1) * sp + 1);
    std::vector<T> x(span);
    for (T& v : x) v = (T)(uniform() * 10.0 - 3.0);
    for (int64_t c = 0; c < C; ++c)                                  // the last parameter is constant
        for (int64_t n = 0; n < N; ++n) x[(size_t)(c * sc + n * sn + (P - 1) * sp)] = (T)2.5;
    const int64_t a = N / b, A = C * a;
    std::vector<double> bm((size_t)(P * A)), mu((size_t)P), mu2((size_t)P);
    CHECK(mcb_batch_means_host(x.data(), dtype, C, N, P, sc, sn, sp, b, bm.data(), A, mu.data()) == MCR_OK);
    CHECK(mcb_batch_means_host(x.data(), dtype, C, N, P, sc, sn, sp, b, nullptr, 0, mu2.data()) == MCR_OK);
    CHECK(std::memcmp(mu.data(), mu2.data(), (size_t)P * 8) == 0);
    CHECK(mcb_batch_means_host(x.data(), dtype, C, N, P, sc, sn, sp, b, bm.data(), A, nullptr) == MCR_OK);
    CHECK(mu[(size_t)(P - 1)] == 2.5);
    for (int64_t k = 0; k < A; ++k) CHECK(bm[(size_t)((P - 1) * A + k)] == 2.5);
    double plain = 0.0;                                              // parameter 0 against a plain mean
    for (int64_t c = 0; c < C; ++c)
        for (int64_t n = N - a * b; n < N; ++n) plain += (double)x[(size_t)(c * sc + n * sn)];
    CHECK(std::fabs(mu[0] - plain / (double)(A * b)) <= 1e-12 * 10.0);
}

int main()
{
    const int64_t sizes[] = {1, 2, 3, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2049};
    for (int64_t b : sizes)
        for (int64_t r0 : {(int64_t)0, (int64_t)1, b - 1})
            for (int layout = 0; layout < 4; ++layout) {
                means_case<double>(MCR_F64, layout == 3 ? 3 : 1 + (b % 2) * 2, 3 * b + r0, 3, b, layout);
                means_case<float>(MCR_F32, layout == 3 ? 3 : 1 + (b % 2) * 2, 3 * b + r0, 2, b, layout);
            }
    means_case<double>(MCR_F64, 2, 50, 1, 50, 0);                    // b = N
    means_case<double>(MCR_F64, 1, 1, 1, 1, 1);

    int64_t b = 0, a = 0;
    CHECK(mcb_batch_size(1000, 3, &b, &a) == MCR_OK && b == 30 && a == 33);
    CHECK(mcb_batch_size(2000, 1, &b, &a) == MCR_OK && b == 44 && a == 45);
    CHECK(mcb_batch_size(3, 3, &b, &a) == MCR_OK && b == 3 && a == 1);
    CHECK(mcb_batch_size(2, 3, &b, &a) == MCR_EINVAL && mcb_batch_size(0, 1, &b, &a) == MCR_EINVAL);
    CHECK(mcb_batch_size(9, 2, &b, &a) == MCR_EINVAL && mcb_batch_size(9, 1, nullptr, &a) == MCR_EINVAL);

    const int64_t P = 5;
    std::vector<double> cb((size_t)(P * P)), cb3((size_t)(P * P)), sig((size_t)(P * P)), sig2((size_t)(P * P)), mu((size_t)P), mu2((size_t)P);
    for (size_t i = 0; i < cb.size(); ++i) { cb[i] = uniform(); cb3[i] = uniform(); }
    for (double& v : mu) v = uniform();
    for (double& v : mu2) v = uniform();
    CHECK(mcb_lrv_finish_host(cb.data(), nullptr, P, 7, 40, 0, 1, sig.data()) == MCR_OK && sig[3] == cb[3] * ((7.0 * 40.0) / 39.0));
    CHECK(mcb_lrv_finish_host(cb.data(), cb3.data(), P, 6, 40, 121, 3, sig2.data()) == MCR_OK);
    CHECK(sig2[7] == 2.0 * (cb[7] * ((6.0 * 40.0) / 39.0)) - cb3[7] * ((2.0 * 121.0) / 120.0));
    CHECK(mcb_lrv_finish_host(cb.data(), nullptr, P, 7, 1, 0, 1, sig2.data()) == MCR_OK && std::isnan(sig2[0]) && std::isnan(sig2[24]));
    CHECK(mcb_lrv_finish_host(cb.data(), cb3.data(), P, 7, 40, 121, 3, sig2.data()) == MCR_EINVAL);
    CHECK(mcb_lrv_finish_host(cb.data(), nullptr, P, 6, 40, 121, 3, sig2.data()) == MCR_EINVAL);
    CHECK(mcb_lrv_finish_host(nullptr, nullptr, P, 6, 40, 0, 1, sig2.data()) == MCR_EINVAL);

    const double scale[P] = {0.0, 2.0, 0.0, 0.5, 0.0};
    int64_t live = -1;
    std::vector<double> v(4), d(2), z(2);                            // exactly P_live^2 and P_live doubles
    CHECK(mcb_pool_host(sig.data(), mu.data(), 900, sig.data(), mu2.data(), 700, P, scale, 0.25, v.data(), d.data(), z.data(), &live) == MCR_OK);
    CHECK(live == 2 && d[1] == 0.5 * (mu2[3] - mu[3]));
    CHECK(v[1] == (2.0 * 0.5) * (sig[1 * P + 3] / 900.0 + sig[1 * P + 3] / 700.0));
    CHECK(v[3] == (0.5 * 0.5) * (sig[3 * P + 3] / 900.0 + sig[3 * P + 3] / 700.0) + 0.25 && z[1] == d[1] / std::sqrt(v[3]));
    CHECK(mcb_pool_host(sig.data(), mu.data(), 1, nullptr, nullptr, 1, P, scale, 0.0, v.data(), d.data(), z.data(), &live) == MCR_OK);
    CHECK(live == 2 && v[2] == (0.5 * 2.0) * sig[3 * P + 1] && d[0] == 2.0 * mu[1]);
    const double none[P] = {0, 0, 0, 0, 0};
    CHECK(mcb_pool_host(sig.data(), mu.data(), 1, nullptr, nullptr, 1, P, none, 0.0, v.data(), d.data(), z.data(), &live) == MCR_OK && live == 0);
    const double bad[P] = {1, 1, -1, 1, 1};
    CHECK(mcb_pool_host(sig.data(), mu.data(), 1, nullptr, nullptr, 1, P, bad, 0.0, v.data(), d.data(), z.data(), &live) == MCR_EINVAL);
    CHECK(mcb_pool_host(sig.data(), mu.data(), 1, nullptr, nullptr, 1, P, scale, -1.0, v.data(), d.data(), z.data(), &live) == MCR_EINVAL);
    CHECK(mcb_pool_host(sig.data(), mu.data(), 1, sig.data(), nullptr, 1, P, scale, 0.0, v.data(), d.data(), z.data(), &live) == MCR_EINVAL);

    std::vector<double> y(2049, 0.5);
    double s = -1.0;
    CHECK(mcb_tree_sum_host(y.data(), 2049, 1, &s) == MCR_OK && s == 2049 * 0.25);
    CHECK(mcb_tree_sum_host(y.data(), 1025, 0, &s) == MCR_OK && s == 1025 * 0.5);
    CHECK(mcb_tree_sum_host(nullptr, 0, 0, &s) == MCR_OK && s == 0.0);
    CHECK(mcb_tree_sum_host(y.data(), -1, 0, &s) == MCR_EINVAL && mcb_tree_sum_host(y.data(), 1, 0, nullptr) == MCR_EINVAL);

    double x[8] = {1, 2, 3, 4, 5, 6, 7, 8}, out[8];
    CHECK(mcb_batch_means_host(nullptr, MCR_F64, 1, 8, 1, 8, 1, 8, 2, out, 4, out) == MCR_EINVAL);
    CHECK(mcb_batch_means_host(x, 9, 1, 8, 1, 8, 1, 8, 2, out, 4, out) == MCR_EINVAL);
    CHECK(mcb_batch_means_host(x, MCR_F64, 1, 8, 1, 8, 1, 8, 0, out, 4, out) == MCR_EINVAL);
    CHECK(mcb_batch_means_host(x, MCR_F64, 1, 8, 1, 8, 1, 8, 9, out, 4, out) == MCR_EINVAL);
    CHECK(mcb_batch_means_host(x, MCR_F64, 1, 8, 1, 8, -1, 8, 2, out, 4, out) == MCR_EINVAL);
    CHECK(mcb_batch_means_host(x, MCR_F64, 1, 8, 1, 8, 1, 8, 2, out, 3, out) == MCR_EINVAL);
    CHECK(mcb_batch_means_host(x, MCR_F64, 1, 8, 1, 8, 1, 8, 2, nullptr, 4, nullptr) == MCR_EINVAL);
    CHECK(std::strstr(mcb_last_error(nullptr), "NULL") != nullptr);
    CHECK(mcb_batch_means_host(x, MCR_F64, 1, 8, 1, 8, 1, 8, 3, out, 2, out + 4) == MCR_OK && out[0] == 4.0 && out[1] == 7.0 && out[4] == 5.5);
    CHECK(mcb_set_workspace_limit(nullptr, 1) == MCR_EINVAL && mcb_version() == MCB_VERSION);

    std::printf(failures ? "%d check(s) FAILED\n" : "all checks held\n", failures);
    return failures ? 1 : 0;
}
