// Stand-alone host check of the Newton flow in rust-ida_amd/host/ida_controller.hpp (tests/test_newton_shared.py): newton_begin and
// newton_after_ctest, which every stepper instantiates, against the oracle's restatement of the reference's Newton::solve
// (oracle/newton.hpp) on a scripted problem. A script fixes the solver's initial jcur, the caller's call_lsetup, the result of each
// linear setup and the outcome of each convergence test (go on / converged / ConvergenceRecover); EVERY script is run through
// oracle::Newton::solve and through a driver loop over the shared functions -- the loop each stepper writes in its own mechanics --
// and the return code, niters, nconvfails, jcur, curiter and the exact sequence of sys / setup / solve calls must agree. Both
// flavours of the setup's bookkeeping are driven: after_lsetup, and after_lsetup_nojac with a psetup's failure on top. Also here:
// conv_test_core's compile-time iterations against a restatement with std::pow, and the identity they rest on, pow(b, 1.0) == b bit
// for bit. Every group prints a line "ok <name>"; the first failed check prints "FAIL line <n>: <expression>" and ends the program
// with status 1. Also the program to run under -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>

#include "ida_controller.hpp"
#include "newton.hpp"

using namespace idactl;

#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            std::printf("FAIL line %d: %s\n", __LINE__, #x);      \
            std::exit(1);                                         \
        }                                                         \
    } while (0)

namespace {

enum Outcome { GO_ON = 0, CONVERGED = 1, RECOVER = 2 };
constexpr int PASSES = 2;                    // a solve restarts at most once: the setup of the second pass makes the Jacobian current
constexpr int TESTS = PASSES * MAXNLSIT;     // convergence tests a solve can make

struct Script {
    bool jcur, call_lsetup;
    bool setup_fails[PASSES];   // by setup call
    int outcome[TESTS];         // by convergence test
};

// the scripted problem under the oracle's solver; log: 'y' sys, 'S' setup, 'l' solve
struct Scripted : oracle::NLProblem {
    const Script& sc;
    std::string log;
    int nsetup = 0, ntest = 0;
    explicit Scripted(const Script& s) : sc(s) {}
    int sys(const double*, double* f) override {
        log += 'y';
        f[0] = 1.0;
        return oracle::NLS_SUCCESS;
    }
    int setup(const double*, const double*, bool, bool* jcur) override {
        log += 'S';
        CHECK(nsetup < PASSES);
        *jcur = true;
        return sc.setup_fails[nsetup++] ? oracle::NLS_LSETUP_RECVR : oracle::NLS_SUCCESS;
    }
    int solve(const double*, double*) override {
        log += 'l';
        return oracle::NLS_SUCCESS;
    }
    int ctest(const oracle::Newton&, const double*, const double*, double, const double*, bool* converged) override {
        CHECK(ntest < TESTS);
        const int o = sc.outcome[ntest++];
        *converged = o == CONVERGED;
        return o == RECOVER ? oracle::NLS_CONV_RECVR : oracle::NLS_SUCCESS;
    }
};

// the driver loop of a stepper over the shared flow; nojac: the setup's bookkeeping of a Krylov ctx with a psetup that can fail
int drive(SysCore& s, const Script& sc, bool nojac, std::string& log) {
    int nsetup = 0, ntest = 0;
    for (;;) {
        log += 'y';  // sys(y0)
        s.nre += 1;
        if (s.call_lsetup) {
            log += 'S';
            CHECK(nsetup < PASSES);
            const int info = sc.setup_fails[nsetup++] ? 1 : 0;
            if (nojac) {
                after_lsetup_nojac(s);
                if (info) s.nls_ret = NLS_LSETUP_RECVR;
            } else {
                after_lsetup(s, info);
            }
        }
        if (!newton_begin(s, s.call_lsetup)) break;
        NewtonNext next;
        do {
            log += 'l';
            s.niters += 1;
            CHECK(ntest < TESTS);
            const int o = sc.outcome[ntest++];
            next = newton_after_ctest(s, o == RECOVER ? NLS_CONV_RECVR : NLS_SUCCESS, o == CONVERGED);
            if (next == NEWTON_ITERATE) {  // sys(y)
                log += 'y';
                s.nre += 1;
            }
        } while (next == NEWTON_ITERATE);
        if (next == NEWTON_DONE) break;
    }
    return s.nls_ret;
}

long every_script(bool nojac) {
    long scripts = 0, restarts = 0, q3 = 0, setup_failures = 0, maxit = 0;
    int total = 1;
    for (int i = 0; i < TESTS; ++i) total *= 3;
    for (int head = 0; head < 16; ++head) {
        for (int code = 0; code < total; ++code) {
            Script sc;
            sc.jcur = head & 1;
            sc.call_lsetup = head & 2;
            sc.setup_fails[0] = head & 4;
            sc.setup_fails[1] = head & 8;
            for (int i = 0, c = code; i < TESTS; ++i, c /= 3) sc.outcome[i] = c % 3;

            Scripted prob(sc);
            oracle::Newton nw(1, MAXNLSIT);
            nw.jcur = sc.jcur;
            const double y0[1] = {0.0}, w[1] = {1.0};
            double y[1] = {0.0};
            const int ret_o = nw.solve(prob, y0, y, w, 1.0, sc.call_lsetup);

            SysCore s;
            s.jcur = sc.jcur;
            s.call_lsetup = sc.call_lsetup;
            s.nls_ret = NLS_SUCCESS;  // begin_attempt
            s.cj = 2.0;
            std::string log;
            const int ret = drive(s, sc, nojac, log);

            CHECK(ret == ret_o);
            CHECK(s.niters == nw.niters);
            CHECK(s.nconvfails == nw.nconvfails);
            CHECK(s.jcur == nw.jcur);
            CHECK(s.curiter == nw.curiter);
            CHECK(log == prob.log);
            long nsys = 0, nset = 0;
            for (char ch : log) { nsys += ch == 'y'; nset += ch == 'S'; }
            CHECK(s.nre == nsys);  // (the caller's rule: nre where it runs a residual, niters where it runs a linear solve)
            CHECK(s.nsetups == nset && s.nje == (nojac ? 0 : nset));
            scripts += 1;
            restarts += nset == 2 || (nset == 1 && !sc.call_lsetup);
            q3 += ret == NLS_CONV_RECVR;
            setup_failures += ret == NLS_LSETUP_RECVR;
            maxit += s.curiter == MAXNLSIT;
        }
    }
    // the enumeration reaches every exit: restart with a setup, Q3's return, a failed setup in either pass, the MAXNLSIT exit
    CHECK(restarts > 0 && q3 > 0 && setup_failures > 0 && maxit > 0);
    return scripts;
}

// idaNlsConvTest restated with std::pow for every m (ida_nls.rs:218-266)
int conv_test_pow(int m, double delnrm, double toldel, double eps_newt, double& oldnrm, double& ss, bool* converged) {
    *converged = false;
    if (m == 0) {
        oldnrm = delnrm;
        if (delnrm <= 0.0001 * toldel) { *converged = true; return NLS_SUCCESS; }
    } else {
        const double rate = std::pow(delnrm / oldnrm, 1.0 / (double)m);
        if (rate > RATEMAX) return NLS_CONV_RECVR;
        ss = rate / (1.0 - rate);
    }
    if (ss * delnrm <= eps_newt) *converged = true;
    return NLS_SUCCESS;
}

uint64_t bits(double x) {
    uint64_t u;
    std::memcpy(&u, &x, 8);
    return u;
}
double from_bits(uint64_t u) {
    double x;
    std::memcpy(&x, &u, 8);
    return x;
}

// a deterministic sweep of positive doubles: every exponent many times over, mantissas from a multiplicative sequence
template <class F>
void sweep(F&& f) {
    const uint64_t top = 0x7ff0000000000000ull;  // +infinity
    uint64_t mant = 0x9e3779b97f4a7c15ull;
    for (uint64_t u = 1; u < top; u += 0x00003ffffffff123ull) {
        f(from_bits(u));
        mant = mant * 6364136223846793005ull + 1442695040888963407ull;
        f(from_bits((u & top) | (mant >> 12)));
    }
    f(from_bits(1));                  // the smallest subnormal
    f(from_bits(top - 1));            // the largest finite double
    f(1.0);
    f(RATEMAX);
}

void pow_identity() {
    long n = 0;
    sweep([&](double b) {
        CHECK(bits(std::pow(b, 1.0)) == bits(b));
        n += 1;
    });
    CHECK(n > 100000);
    CHECK(bits(std::pow(0.0, 1.0)) == bits(0.0));
    const double inf = std::numeric_limits<double>::infinity();
    CHECK(bits(std::pow(inf, 1.0)) == bits(inf));
    const double nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(bits(std::pow(nan, 1.0)) == bits(nan));
}

void conv_test_core_against_pow() {
    const double olds[] = {1.0e-3, 0.37, 5.0e8}, tols[] = {1.0, 1.0e-9}, sss[] = {20.0, 100.0, 0.3};
    long n = 0;
    sweep([&](double d) {
        n += 1;
        if (n % 7 != 0) return;
        for (double old : olds)
            for (double tol : tols)
                for (double ss0 : sss)
                    for (int m = 0; m < MAXNLSIT; ++m) {
                        const double eps = 0.33 * tol;
                        double o1 = old, s1 = ss0, o2 = old, s2 = ss0, o3 = old, s3 = ss0;
                        bool c1 = false, c2 = false, c3 = false;
                        const int r1 = conv_test_pow(m, d, tol, eps, o1, s1, &c1);
                        const int r2 = conv_test_core(m, d, tol, eps, o2, s2, &c2);
                        CHECK(r1 == r2 && c1 == c2 && bits(o1) == bits(o2) && bits(s1) == bits(s2));
                        if (m > 1) continue;
                        const int r3 = m == 0 ? conv_test_core<0>(9, d, tol, eps, o3, s3, &c3) : conv_test_core<1>(9, d, tol, eps, o3, s3, &c3);
                        CHECK(r1 == r3 && c1 == c3 && bits(o1) == bits(o3) && bits(s1) == bits(s3));
                        // and through the record, as the steppers call it
                        SysCore s;
                        s.curiter = m; s.toldel = tol; s.eps_newt = eps; s.oldnrm = old; s.ss = ss0;
                        bool c4 = false;
                        CHECK(conv_test(s, d, &c4) == r1 && c4 == c1 && bits(s.oldnrm) == bits(o1) && bits(s.ss) == bits(s1));
                    }
    });
}

}  // namespace

int main() {
    const long expect = 16L * 6561L;
    CHECK(every_script(false) == expect);
    std::printf("ok direct_setup\n");
    CHECK(every_script(true) == expect);
    std::printf("ok nojac_setup\n");
    pow_identity();
    std::printf("ok pow_identity\n");
    conv_test_core_against_pow();
    std::printf("ok conv_test_core\n");
    std::printf("all ok\n");
    return 0;
}
