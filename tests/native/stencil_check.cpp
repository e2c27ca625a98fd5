// rust-ida_amd/csrc/stencil_problems.hpp on the host: the banded device problems' descriptions -- the text every stencil kernel
// evaluates -- printed value by value for tests/test_stencil_problems.py, which compares the bits with the numpy restatements
// (tests/dq_ref.py, tests/bruss_ref.py). For each case: the seeded state it was evaluated at, every row of F, every Jacobian entry the
// kernels' band predicate lets through, and the predicate itself for every (r, c) up to two places outside the band.
// Doubles are printed as their 64-bit patterns. Build: g++ -O1 -std=c++17 -ffp-contract=off -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "stencil_problems.hpp"

using namespace idahip;

static uint64_t bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

// uniform in [lo, hi) from a 64-bit LCG (the top 53 bits)
struct Rng {
    uint64_t s;
    double next(double lo, double hi) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return lo + (hi - lo) * ((double)(s >> 11) * 0x1p-53);
    }
};

static void put_vec(const char* tag, const std::vector<double>& v) {
    std::printf("%s", tag);
    for (double x : v) std::printf(" %016llx", (unsigned long long)bits(x));
    std::printf("\n");
}

template <class P>
static void run_case(const char* name, int n, uint64_t seed) {
    Rng g{seed};
    // exact-size vectors: a read outside [0, n) or [0, NPARAM) is an AddressSanitizer error
    std::vector<double> y(n), yp(n), prm(P::NPARAM);
    for (double& v : y) v = g.next(0.25, 3.0);
    for (double& v : yp) v = g.next(-2.0, 2.0);
    for (double& v : prm) v = g.next(0.5, 4.0);
    const double cj = g.next(1.0, 50.0);
    std::printf("case %s %d %d %d\n", name, n, P::NPARAM, P::HALF_BW);
    put_vec("y", y);
    put_vec("yp", yp);
    put_vec("prm", prm);
    put_vec("cj", {cj});
    const double* yd = y.data();
    for (int r = 0; r < n; ++r) {
        const double f = P::row(n, r, yp[r], prm.data(), [&](int k) { return yd[k]; });
        std::printf("row %d %016llx\n", r, (unsigned long long)bits(f));
    }
    for (int c = 0; c < n; ++c) {
        for (int r = c - P::HALF_BW - 2; r <= c + P::HALF_BW + 2; ++r) {
            if (r < 0 || r >= n) continue;
            const bool in = stencil_in_band<P>(r, c);
            std::printf("band %d %d %d\n", r, c, in ? 1 : 0);
            if (in) std::printf("jac %d %d %016llx\n", r, c, (unsigned long long)bits(P::jac_entry(yd, n, r, c, cj, prm.data())));
        }
    }
}

int main() {
    static_assert(Heat1D::KIND == IDAHIP_HEAT1D && Heat1D::NPARAM == 1 && Heat1D::HALF_BW == 1, "heat");
    static_assert(Bruss1D::KIND == IDAHIP_BRUSS1D && Bruss1D::NPARAM == 5 && Bruss1D::HALF_BW == 2, "Brusselator");
    run_case<Heat1D>("heat", 9, 11);
    run_case<Heat1D>("heat", 10, 12);
    run_case<Heat1D>("heat", 23, 13);
    run_case<Bruss1D>("bruss", 10, 14);
    run_case<Bruss1D>("bruss", 12, 15);
    std::printf("all ok\n");
    return 0;
}
