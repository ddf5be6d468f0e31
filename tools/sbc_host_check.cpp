// sbc_host_check.cpp -- the host routines of simulation-based calibration (mcr_sbc_ranks_host, mcr_sbc_uniformity,
// mcr_chi2_sf) as a stand-alone program, for sanitizer runs.  They live in mcr_stats.hip, whose headers hold kernels and
// which runs the pipeline of mcr_api.hip, so the program is built from both units with hipcc and the sanitizers are given
// to the host side alone; no device is opened:
//
//     hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -Iinclude -Wno-unused-value -Wno-pass-failed \
//         -x hip mcmc-db_amd/csrc/mcr_api.hip mcmc-db_amd/csrc/mcr_stats.hip tools/sbc_host_check.cpp \
//         -o sbc_host_check && ./sbc_host_check
//
// It walks the routines through their edges -- no draws, one draw, row lengths around the summation block of 1024, bins 2,
// 20 and L + 1, every refusal, non-finite draws -- and checks what is exact: the counts against a plain loop, uniform
// ranks (chi2 = 0, p = 1, no ECDF deviation), Q(1, x / 2) = exp(-x / 2).  Exit status 0: all held.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "mcmcref_hip.h"

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

int main()
{
    const int64_t S = 3, P = 4;
    for (int64_t L : {0, 1, 2, 63, 65, 1023, 1024, 1025, 2049, 5000}) {
        const size_t rows = (size_t)(S * P);
        std::vector<double> x(rows * (size_t)L), t(rows), mean(rows), sd(rows);
        for (double& v : x) v = std::floor(uniform() * 16.0) / 16.0 - 0.5;       // (a grid: ties with the truth)
        for (double& v : t) v = std::floor(uniform() * 16.0) / 16.0 - 0.5;
        std::vector<int64_t> less(rows), equal(rows);
        mcr_sbc_out out{less.data(), equal.data(), mean.data(), sd.data()};
        CHECK(mcr_sbc_ranks_host(L ? x.data() : nullptr, S, P, L, t.data(), &out) == MCR_OK);
        for (size_t k = 0; k < rows; ++k) {
            int64_t a = 0, b = 0;
            for (int64_t i = 0; i < L; ++i) { a += x[k * (size_t)L + (size_t)i] < t[k]; b += x[k * (size_t)L + (size_t)i] == t[k]; }
            CHECK(less[k] == a && equal[k] == b);
            CHECK(L ? (mean[k] >= -0.5 && mean[k] <= 0.5 && sd[k] >= 0.0) : (std::isnan(mean[k]) && std::isnan(sd[k])));
        }
        mcr_sbc_out some{nullptr, equal.data(), nullptr, nullptr};               // NULL members are skipped
        CHECK(mcr_sbc_ranks_host(L ? x.data() : nullptr, S, P, L, t.data(), &some) == MCR_OK);
        if (L >= 1) {
            for (int64_t B : {(int64_t)2, L + 1 < 20 ? L + 1 : (int64_t)20, L + 1}) {
                std::vector<int64_t> counts((size_t)(P * B));
                std::vector<double> ex((size_t)B), c2((size_t)P), pv((size_t)P), ed((size_t)P);
                CHECK(mcr_sbc_uniformity(less.data(), S, P, L, B, counts.data(), ex.data(), c2.data(), pv.data(), ed.data()) == MCR_OK);
                for (int64_t p = 0; p < P; ++p) {
                    int64_t n = 0;
                    for (int64_t b = 0; b < B; ++b) n += counts[(size_t)(p * B + b)];
                    CHECK(n == S && c2[(size_t)p] >= 0.0 && pv[(size_t)p] >= 0.0 && pv[(size_t)p] <= 1.0 && ed[(size_t)p] <= 1.0);
                }
                CHECK(mcr_sbc_uniformity(less.data(), S, P, L, B, nullptr, nullptr, nullptr, nullptr, nullptr) == MCR_OK);
            }
            x[(size_t)L - 1] = std::numeric_limits<double>::quiet_NaN();
            CHECK(mcr_sbc_ranks_host(x.data(), S, P, L, t.data(), &out) == MCR_ENONFINITE);
        }
    }
    {   // uniform ranks are exactly uniform
        const int64_t L = 99, B = 20, n = 3 * (L + 1);
        std::vector<int64_t> ranks((size_t)n), counts((size_t)B);
        for (int64_t s = 0; s < n; ++s) ranks[(size_t)s] = s % (L + 1);
        double ex[20], c2, pv, ed;
        CHECK(mcr_sbc_uniformity(ranks.data(), n, 1, L, B, counts.data(), ex, &c2, &pv, &ed) == MCR_OK);
        CHECK(c2 == 0.0 && pv == 1.0 && ed == 0.0 && counts[0] == 15 && ex[19] == 15.0);
    }
    {   // refusals
        double x[6] = {0, 1, 2, 3, 4, 5}, t[2] = {1.0, 2.0}, m[2], s[2];
        int64_t a[2], b[2], r[2] = {0, 3};
        mcr_sbc_out out{a, b, m, s};
        CHECK(mcr_sbc_ranks_host(x, 2, 1, 3, t, nullptr) == MCR_EINVAL && mcr_sbc_ranks_host(nullptr, 2, 1, 3, t, &out) == MCR_EINVAL);
        CHECK(mcr_sbc_ranks_host(x, 2, 1, 3, nullptr, &out) == MCR_EINVAL && mcr_sbc_ranks_host(x, -1, 1, 3, t, &out) == MCR_EINVAL);
        CHECK(mcr_sbc_ranks_host(x, 2, -1, 3, t, &out) == MCR_EINVAL && mcr_sbc_ranks_host(x, 2, 1, -3, t, &out) == MCR_EINVAL);
        CHECK(mcr_sbc_ranks_host(x, (int64_t)1 << 31, 1, 3, t, &out) == MCR_EINVAL);
        CHECK(mcr_sbc_ranks_host(x, 2, 1, ((int64_t)1 << 31) - 1, t, &out) == MCR_EINVAL);
        t[1] = std::numeric_limits<double>::infinity();
        CHECK(mcr_sbc_ranks_host(x, 2, 1, 3, t, &out) == MCR_EINVAL);
        CHECK(mcr_sbc_uniformity(r, 2, 1, 3, 1, nullptr, nullptr, m, nullptr, nullptr) == MCR_EINVAL);
        CHECK(mcr_sbc_uniformity(r, 2, 1, 3, 5, nullptr, nullptr, m, nullptr, nullptr) == MCR_EINVAL);
        CHECK(mcr_sbc_uniformity(r, 2, 1, 2, 2, nullptr, nullptr, m, nullptr, nullptr) == MCR_EINVAL);     // the rank 3 > L
        CHECK(mcr_sbc_uniformity(r, 0, 1, 3, 2, nullptr, nullptr, m, nullptr, nullptr) == MCR_EINVAL);
        CHECK(mcr_sbc_uniformity(nullptr, 2, 1, 3, 2, nullptr, nullptr, m, nullptr, nullptr) == MCR_EINVAL);
        CHECK(mcr_sbc_uniformity(r, 2, 1, 3, 2, nullptr, nullptr, m, nullptr, nullptr) == MCR_OK);
    }
    for (double x : {0.0, 1e-3, 0.5, 2.0, 6.0, 100.0, 1000.0}) CHECK(std::fabs(mcr_chi2_sf(x, 2.0) - std::exp(-x / 2)) <= 1e-9 * std::exp(-x / 2));
    for (double dof : {1.0, 3.0, 19.0, 999.0})
        for (double x : {0.0, 1e-3, 1.0, 50.0, 5000.0, 1e6, 1e300}) { const double q = mcr_chi2_sf(x, dof); CHECK(q >= 0.0 && q <= 1.0); }
    CHECK(std::isnan(mcr_chi2_sf(-1.0, 3.0)) && std::isnan(mcr_chi2_sf(1.0, 0.0)) && mcr_chi2_sf(INFINITY, 3.0) == 0.0);
    std::printf(failures ? "%d check(s) failed\n" : "sbc_host_check: all checks held\n", failures);
    return failures != 0;
}
