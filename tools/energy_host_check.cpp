// energy_host_check.cpp -- the host routine behind mcr_energy_distance_host as a stand-alone program, for sanitizer runs:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//         tools/energy_host_check.cpp -o energy_host_check && ./energy_host_check
//
// mcr_energy.hpp's host part is plain C++ (the kernels are behind __HIPCC__), so no HIP and no device is involved.  The
// program walks the routine through its edges -- one draw, one parameter, sizes around the block of 256 pairs and the
// four interleaved accumulators, the threaded and the serial path, every argument error, non-finite input -- and checks
// what is exact: integer lattices, d(x, y) = d(y, x), d(x, x) = +0.0, a dropped parameter.  Exit status 0: all held.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../mcmc-db_amd/csrc/mcr_energy.hpp"

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

// draws a_i (1, .., 1), integer a_i, P a perfect square: every distance is sqrt(P) |a_i - a_j|
static void lattice(long long Mr, long long Ma, long long P, long long root)
{
    std::vector<long long> a((size_t)Mr), b((size_t)Ma);
    for (auto& v : a) v = (long long)(uniform() * 101.0) - 50;
    for (auto& v : b) v = (long long)(uniform() * 101.0) - 50;
    std::vector<double> ref((size_t)(P * Mr)), act((size_t)(P * Ma));
    for (long long p = 0; p < P; ++p) {
        for (long long m = 0; m < Mr; ++m) ref[(size_t)(p * Mr + m)] = (double)a[(size_t)m];
        for (long long m = 0; m < Ma; ++m) act[(size_t)(p * Ma + m)] = (double)b[(size_t)m];
    }
    auto total = [&](const std::vector<long long>& x, const std::vector<long long>& y) {
        long long s = 0;
        for (long long u : x) for (long long v : y) s += u > v ? u - v : v - u;
        return root * s;
    };
    double out[6];
    CHECK(mcr::energy_host(ref.data(), Mr, act.data(), Ma, P, nullptr, out) == 0);
    CHECK(out[0] == (double)total(a, b) / (double)(Mr * Ma));
    CHECK(out[1] == (double)total(a, a) / (double)(Mr * Mr));
    CHECK(out[2] == (double)total(b, b) / (double)(Ma * Ma));
    CHECK(out[3] == (out[0] - out[1]) + (out[0] - out[2]));
}

static void general(long long Mr, long long Ma, long long P)
{
    std::vector<double> ref((size_t)(P * Mr)), act((size_t)(P * Ma)), scale((size_t)P);
    for (auto& v : ref) v = uniform() * 4.0 - 2.0;
    for (auto& v : act) v = uniform() * 5.0 - 2.0;
    for (auto& v : scale) v = 0.25 + uniform();
    double o1[6], o2[6], o3[6];
    CHECK(mcr::energy_host(ref.data(), Mr, act.data(), Ma, P, scale.data(), o1) == 0);
    CHECK(mcr::energy_host(act.data(), Ma, ref.data(), Mr, P, scale.data(), o2) == 0);
    CHECK(o1[0] == o2[0] && o1[1] == o2[2] && o1[2] == o2[1]);            // the samples exchanged
    CHECK(o1[3] >= -1e-12 * o1[0] && o1[4] <= 1.0 + 1e-12);
    CHECK(mcr::energy_host(ref.data(), Mr, ref.data(), Mr, P, scale.data(), o3) == 0);
    CHECK(o3[0] == o3[1] && o3[1] == o3[2] && o3[3] == 0.0 && o3[5] == 0.0);       // a sample against itself
    if (P > 1) {                                                          // a parameter with scale 0 drops out
        scale[(size_t)(P - 1)] = 0.0;
        CHECK(mcr::energy_host(ref.data(), Mr, act.data(), Ma, P, scale.data(), o1) == 0);
        CHECK(mcr::energy_host(ref.data(), Mr, act.data(), Ma, P - 1, scale.data(), o2) == 0);    // (rows are [p][M]: the first
        for (int k = 0; k < 6; ++k) CHECK(o1[k] == o2[k]);                                         // P - 1 rows are the same data)
    }
}

int main()
{
    const long long sizes[] = {1, 2, 3, 4, 5, 37, 255, 256, 257, 300, 513};
    for (long long Mr : sizes)
        for (long long Ma : sizes) {
            lattice(Mr, Ma, 4, 2);
            general(Mr, Ma, Mr % 3 + 1);
        }
    lattice(700, 900, 9, 3);        // the threaded path
    general(600, 600, 7);
    general(1, 1, 100);
    // argument errors and non-finite input
    double x[6] = {0, 1, 2, 3, 4, 5}, out[6], s[2] = {1.0, -1.0};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(mcr::energy_host(nullptr, 3, x, 3, 2, nullptr, out) == 1);
    CHECK(mcr::energy_host(x, 3, nullptr, 3, 2, nullptr, out) == 1);
    CHECK(mcr::energy_host(x, 3, x, 3, 2, nullptr, nullptr) == 1);
    CHECK(mcr::energy_host(x, 0, x, 3, 2, nullptr, out) == 1);
    CHECK(mcr::energy_host(x, 3, x, 0, 2, nullptr, out) == 1);
    CHECK(mcr::energy_host(x, 3, x, 3, 0, nullptr, out) == 1);
    CHECK(mcr::energy_host(x, 3, x, 3, 2, s, out) == 1);
    s[1] = nan; CHECK(mcr::energy_host(x, 3, x, 3, 2, s, out) == 1);
    s[1] = inf; CHECK(mcr::energy_host(x, 3, x, 3, 2, s, out) == 1);
    CHECK(mcr::energy_host(x, 1ll << 22, x, 1ll << 22, 1, nullptr, out) == 1);
    CHECK(mcr::energy_host(x, 1ll << 62, x, 1ll << 62, 1ll << 62, nullptr, out) == 1);
    x[4] = nan; CHECK(mcr::energy_host(x, 3, x, 3, 2, nullptr, out) == 2);
    x[4] = inf; CHECK(mcr::energy_host(x, 3, x, 3, 2, nullptr, out) == 2);
    x[4] = 1e200; x[5] = -1e200; CHECK(mcr::energy_host(x, 3, x, 3, 2, nullptr, out) == 2);
    std::printf(failures ? "%d check(s) failed\n" : "energy_host_check: all checks held\n", failures);
    return failures ? 1 : 0;
}
