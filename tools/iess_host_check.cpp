// iess_host_check.cpp -- the host definition of the indicator ESS (mci_indicator_ess_host of include/mcmcref_iess.h) as a
// stand-alone program, for sanitizer runs.  It lives in mci_api.hip, whose header holds the kernels, so the program is
// built from that unit with hipcc and the sanitizers are given to the host side alone; no device is opened:
//
//     hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -Iinclude -Wno-unused-value \
//         -x hip mcmc-db_amd/csrc/mci_api.hip tools/iess_host_check.cpp -o iess_host_check && ./iess_host_check
//
// It walks the routine through its edges -- chains of 1 and 2 draws, chain lengths around the 64-draw word and the lag
// block, 1 to 5 chains, 1 and MCI_MAX_REQUESTS requests, constant and empty indicators, NaN draws, infinite thresholds,
// NULL outputs, every refusal -- and checks what is exact: the count against a plain loop, the hand case 1,1,1,0,0,0
// (truncation 3, ESS 30/11), the truncation lag against plain integer loops in 128-bit arithmetic.  Exit status 0: all held.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "mcmcref_iess.h"

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

// The first lag with A(lag) < 0 by the definition's plain loops (n when none; 0 for a constant indicator; -1 for n < 2).
static int64_t plain_trunc(const std::vector<double>& x, int64_t C, int64_t N, double lo, double hi, int64_t* ones)
{
    std::vector<int> b((size_t)(C * N));
    int64_t total = 0;
    for (size_t i = 0; i < b.size(); ++i) total += b[i] = lo < x[i] && x[i] <= hi;
    *ones = total;
    if (N < 2) return -1;
    bool constant = true;
    for (size_t i = 1; i < b.size(); ++i) constant = constant && b[i] == b[0];
    if (constant) return 0;
    for (int64_t lag = 1; lag < N; ++lag) {
        __int128 A = 0;
        for (int64_t c = 0; c < C; ++c) {
            const int* bc = b.data() + c * N;
            int64_t k = 0, S = 0, H = 0, T = 0;
            for (int64_t i = 0; i < N; ++i) k += bc[i];
            for (int64_t i = 0; i < N - lag; ++i) { S += bc[i] * bc[i + lag]; H += bc[i]; }
            for (int64_t i = lag; i < N; ++i) T += bc[i];
            A += (__int128)N * N * S - (__int128)N * k * (H + T) + (__int128)(N - lag) * k * k;
        }
        if (A < 0) return lag;
    }
    return N;
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(mci_version() == MCI_VERSION);
    for (int64_t N : {1, 2, 3, 63, 64, 65, 127, 128, 129, MCI_LAG_BLOCK - 1, MCI_LAG_BLOCK, MCI_LAG_BLOCK + 1, 2 * MCI_LAG_BLOCK + 1})
        for (int64_t C : {1, 2, 3, 5}) {
            std::vector<double> x((size_t)(C * N));
            double v = 0.0;
            for (double& e : x) { v = 0.95 * v + uniform() - 0.5; e = std::floor(v * 8.0) / 8.0; }     // sticky, with ties
            if (N > 5) x[3] = nan;
            const double lo[4] = {-inf, -inf, 0.0, 0.25}, hi[4] = {0.0, inf, inf, 0.25};
            double ess[4];
            int64_t trunc[4], ones[4];
            CHECK(mci_indicator_ess_host(x.data(), C, N, lo, hi, 4, ess, trunc, ones) == MCR_OK);
            for (int k = 0; k < 4; ++k) {
                int64_t n1 = 0;
                const int64_t t = plain_trunc(x, C, N, lo[k], hi[k], &n1);
                CHECK(ones[k] == n1);
                CHECK(trunc[k] == t);
                CHECK(N < 2 ? std::isnan(ess[k]) : (ess[k] > 0.0 && std::isfinite(ess[k])));
                if (trunc[k] == 0) CHECK(ess[k] == (double)(C * N));
            }
            CHECK(ones[3] == 0 && (N < 2 || trunc[3] == 0));                       // lower == upper: empty
            CHECK(mci_indicator_ess_host(x.data(), C, N, lo, hi, 4, nullptr, nullptr, nullptr) == MCR_OK);
        }
    {
        const double x[6] = {1, 1, 1, 0, 0, 0}, lo = 0.5, hi = inf;
        double ess = 0.0;
        int64_t trunc = 0, ones = 0;
        CHECK(mci_indicator_ess_host(x, 1, 6, &lo, &hi, 1, &ess, &trunc, &ones) == MCR_OK);
        CHECK(trunc == 3 && ones == 3 && std::fabs(ess - 30.0 / 11.0) < 1e-14);
    }
    {
        std::vector<double> x(64, 0.5), lo(MCI_MAX_REQUESTS + 1, 0.0), hi(MCI_MAX_REQUESTS + 1, 1.0), ess(MCI_MAX_REQUESTS + 1);
        CHECK(mci_indicator_ess_host(x.data(), 2, 32, lo.data(), hi.data(), MCI_MAX_REQUESTS, ess.data(), nullptr, nullptr) == MCR_OK);
        CHECK(ess[0] == 64.0 && ess[MCI_MAX_REQUESTS - 1] == 64.0);
        CHECK(mci_indicator_ess_host(x.data(), 2, 32, lo.data(), hi.data(), MCI_MAX_REQUESTS + 1, ess.data(), nullptr, nullptr) == MCR_EINVAL);
        CHECK(mci_indicator_ess_host(x.data(), 2, 32, lo.data(), hi.data(), 0, ess.data(), nullptr, nullptr) == MCR_EINVAL);
        CHECK(mci_indicator_ess_host(nullptr, 2, 32, lo.data(), hi.data(), 1, ess.data(), nullptr, nullptr) == MCR_EINVAL);
        CHECK(mci_indicator_ess_host(x.data(), 2, 32, nullptr, hi.data(), 1, ess.data(), nullptr, nullptr) == MCR_EINVAL);
        CHECK(mci_indicator_ess_host(x.data(), 0, 32, lo.data(), hi.data(), 1, ess.data(), nullptr, nullptr) == MCR_EINVAL);
        CHECK(mci_indicator_ess_host(x.data(), 2, 0, lo.data(), hi.data(), 1, ess.data(), nullptr, nullptr) == MCR_EINVAL);
        CHECK(mci_indicator_ess_host(x.data(), 1, MCI_MAX_DRAWS + 1, lo.data(), hi.data(), 1, ess.data(), nullptr, nullptr) == MCR_EINVAL);
        CHECK(mci_indicator_ess_host(x.data(), 1 << 21, 1 << 10, lo.data(), hi.data(), 1, ess.data(), nullptr, nullptr) == MCR_EINVAL);
        lo[1] = nan;
        CHECK(mci_indicator_ess_host(x.data(), 2, 32, lo.data(), hi.data(), 2, ess.data(), nullptr, nullptr) == MCR_EINVAL);
        CHECK(mci_last_error(nullptr)[0] != 0);
    }
    std::printf(failures ? "%d check(s) failed\n" : "iess_host_check: all held\n", failures);
    return failures ? 1 : 0;
}
