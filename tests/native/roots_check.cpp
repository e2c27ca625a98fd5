// Stand-alone host check of rust-ida_amd/host/ida_solve_flow.hpp (tests/test_roots_shared.py): the root finding, the stop tests and
// the loop-top checks that the host stepper and the device steppers share, instantiated with a closed-form backend -- every
// component of y is a fixed cubic in t, g_i = y[comp_i] - thr_i, interp(t) evaluates the cubics, eval counts its calls -- on
// controller records with hand-set tn, hh, toutc. Every case prints a line "ok <name>"; the first failed check prints
// "FAIL <file line>: <expression>" and ends the program with status 1. Also the program to run under -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ida_solve_flow.hpp"

using namespace idactl;

#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            std::printf("FAIL line %d: %s\n", __LINE__, #x);      \
            std::exit(1);                                         \
        }                                                         \
    } while (0)

namespace {

constexpr int NC = 4;  // components of y

struct Roots {  // the host stepper's kind of root state: vectors
    std::vector<double> glo, ghi, grout, iroots;
    std::vector<int32_t> gactive;
    explicit Roots(int nr, int active = 1) : glo(nr, 0.0), ghi(nr, 0.0), grout(nr, 0.0), iroots(nr, 0.0), gactive(nr, active) {}
};

struct Poly {  // y_c(t) = ((c3 t + c2) t + c1) t + c0
    double c[NC][4] = {{0}};
    double at(int k, double t) const { return ((c[k][3] * t + c[k][2]) * t + c[k][1]) * t + c[k][0]; }
    double slope(int k, double t) const { return (3.0 * c[k][3] * t + 2.0 * c[k][2]) * t + c[k][1]; }
};

struct Backend {
    const Poly& p;
    std::vector<int> comp;
    std::vector<double> thr;
    double t0 = 0.0;               // where phi[0], phi[1] = y(t0), y'(t0) belong
    double phi1[NC] = {0, 0, 0, 0};   // phi[1] of yy_add_phi1
    double y[NC] = {0, 0, 0, 0};   // the current yy
    double tcur = 0.0;             // the t of the last interp
    long calls = 0, fail_at = 0;   // evaluations of g so far; the call that fails (0: none)
    int nsol = 0, sol_rc = 0;      // solution_at: calls, what it returns
    double sol_t = 0.0;
    // where the evaluations after an interp fell relative to `root`: counts and the longest run on each side
    double root = 0.0;
    bool track = false;
    int nlo = 0, nhi = 0, run = 0, last = 0, maxrun_lo = 0, maxrun_hi = 0;
    std::vector<double> ts = {};  // every t that interp was asked for

    int interp(double t) {
        tcur = t;
        ts.push_back(t);
        for (int k = 0; k < NC; ++k) y[k] = p.at(k, t);
        return 0;
    }
    int solution_at(double t) {
        nsol += 1;
        sol_t = t;
        return sol_rc;
    }
    int g_now(double* g) {
        calls += 1;
        if (calls == fail_at) return IDAENS_RTFUNC_FAIL;
        for (size_t i = 0; i < comp.size(); ++i) g[i] = y[comp[i]] - thr[i];
        return 0;
    }
    int eval(double, double* g) {
        if (track) {
            const int side = tcur < root ? 1 : 2;
            run = side == last ? run + 1 : 1;
            last = side;
            if (side == 1) { nlo += 1; if (run > maxrun_lo) maxrun_lo = run; }
            else { nhi += 1; if (run > maxrun_hi) maxrun_hi = run; }
        }
        return g_now(g);
    }
    int eval_start(double* g) {
        for (int k = 0; k < NC; ++k) y[k] = p.at(k, t0);
        return g_now(g);
    }
    int yy_from_phi01(double f) {
        for (int k = 0; k < NC; ++k) y[k] = p.at(k, t0) + f * p.slope(k, t0);
        return 0;
    }
    int yy_add_phi1(double f) {
        for (int k = 0; k < NC; ++k) y[k] = y[k] + f * phi1[k];
        return 0;
    }
};

SysCore record(double tn, double hh, double toutc, double tlo) {
    SysCore s;
    s.tn = tn;
    s.hh = hh;
    s.hused = hh;
    s.toutc = toutc;
    s.taskc = IDAENS_NORMAL;
    s.tlo = tlo;
    s.nst = 1;
    return s;
}
double ttol_of(const SysCore& s) { return (std::fabs(s.tn) + std::fabs(s.hh)) * F64_EPS * 100.0; }

// (a), (b): a step from 0.5 to 1.0 over the root of t^2 - 0.5 (rising: rootsfound -1) and of 0.75 - t (falling: +1); a third
// function that does not change sign reports 0
void bracket_a_root() {
    Poly p;
    p.c[0][2] = 1.0; p.c[0][0] = -0.5;   // t^2 - 0.5
    p.c[1][1] = -1.0; p.c[1][0] = 0.75;  // 0.75 - t
    p.c[2][1] = 1.0;                     // t
    for (int which = 0; which < 2; ++which) {
        Backend be{p, {which, 2}, {0.0, 5.0}};
        Roots rs(2);
        SysCore s = record(1.0, 0.5, 2.0, 0.5);
        rs.glo[0] = p.at(which, 0.5);
        rs.glo[1] = p.at(2, 0.5) - 5.0;
        const double glo0 = rs.glo[0];
        CHECK(r_check3(s, rs, 2, be) == IDAENS_ROOT_RETURN);
        const double ttol = ttol_of(s);
        CHECK(s.ttol == ttol && s.trout == s.thi && s.tlo == s.trout);
        // g(trout) is on the far side of the root or on it, g(trout - ttol) on the near side or on it
        const double gt = p.at(which, s.trout), gb = p.at(which, s.trout - ttol);
        CHECK(gt * glo0 <= 0.0 && gb * glo0 >= 0.0);
        const double exact = which == 0 ? std::sqrt(0.5) : 0.75;
        CHECK(std::fabs(s.trout - exact) <= ttol + 2.0 * F64_EPS);
        CHECK(rs.iroots[0] == signum(glo0) && rs.iroots[0] == (which == 0 ? -1.0 : 1.0) && rs.iroots[1] == 0.0);
        CHECK(be.tcur == s.trout);  // yy, yp are left at the root
        CHECK(s.nge == be.calls && be.calls >= 2);
    }
    // toutc inside the step: the search ends at toutc (IDA_NORMAL), before the root -> no root
    {
        Backend be{p, {0}, {0.0}};
        Roots rs(1);
        SysCore s = record(1.0, 0.5, 0.625, 0.5);
        rs.glo[0] = p.at(0, 0.5);
        CHECK(r_check3(s, rs, 1, be) == IDAENS_UNFINISHED);
        CHECK(s.thi == 0.625 && s.trout == 0.625 && s.tlo == 0.625 && rs.glo[0] == p.at(0, 0.625) && s.nge == be.calls && be.calls == 1);
        // IDA_ONE_STEP looks as far as tn
        s = record(1.0, 0.5, 0.625, 0.5);
        s.taskc = IDAENS_ONE_STEP;
        rs.glo[0] = p.at(0, 0.5);
        CHECK(r_check3(s, rs, 1, be) == IDAENS_ROOT_RETURN && s.thi <= 1.0 && s.trout > 0.625);
    }
    std::puts("ok bracket_a_root");
}

// (c): g exactly 0 at t0. r_check1 switches the function off, nudges y along y', switches it on again with the nudged value; the
// step that follows reports no root at t0. A function that stays 0 after the nudge stays off.
void zero_at_t0() {
    Poly p;
    p.c[0][1] = 1.0;   // t: zero at t0 = 0, slope 1
    p.c[1][0] = 0.0;   // identically 0
    p.c[2][0] = 3.0;   // 3: never 0
    p.c[3][2] = 1.0;   // t^2: zero at t0 with slope 0 -> still 0 after the nudge, non-zero after the first step
    Backend be{p, {0, 1, 2, 3}, {0.0, 0.0, 1.0, 0.0}};
    Roots rs(4, 0);  // Ida::new: all inactive... r_check1 leaves the non-zero ones as they are
    rs.gactive[2] = 1;
    SysCore s;
    s.tn = 0.0;
    s.hh = 0.001;
    CHECK(r_check1(s, rs, 4, be) == 0);
    const double ttol = ttol_of(s);
    const double smallh = std::fmax(ttol / 0.001, 0.1) * 0.001;
    CHECK(s.tlo == 0.0 && s.ttol == ttol);
    CHECK(rs.gactive[0] == 1 && rs.glo[0] == smallh);  // y0 + smallh * y'0 = smallh
    CHECK(rs.gactive[1] == 0 && rs.glo[1] == 0.0);
    CHECK(rs.gactive[2] == 1 && rs.glo[2] == 2.0);
    CHECK(rs.gactive[3] == 0 && rs.glo[3] == 0.0);
    CHECK(rs.iroots[0] == 0.0 && rs.iroots[1] == 0.0 && rs.iroots[2] == 0.0 && rs.iroots[3] == 0.0);
    CHECK(s.nge == 2 && be.calls == 2);
    // a step so small that ttol / |hh| exceeds 0.1: the nudge is then ttol long, not 0.1 |hh|
    {
        Poly q;
        q.c[0][1] = 1.0;  // t, threshold 1: zero at t0 = 1
        Backend b3{q, {0}, {1.0}};
        b3.t0 = 1.0;
        Roots r3(1, 0);
        SysCore s3;
        s3.tn = 1.0;
        s3.hh = 1e-14;
        CHECK(r_check1(s3, r3, 1, b3) == 0);
        const double tt = (1.0 + 1e-14) * F64_EPS * 100.0, ratio = tt / 1e-14;
        CHECK(ratio > 2.0 && s3.ttol == tt && r3.gactive[0] == 1 && r3.glo[0] == (1.0 + (ratio * 1e-14) * 1.0) - 1.0 && r3.glo[0] > 1e-14);
    }
    // no zero at t0: one evaluation, no nudge
    {
        Backend b2{p, {2}, {1.0}};
        Roots r2(1);
        SysCore s2;
        s2.hh = 0.001;
        CHECK(r_check1(s2, r2, 1, b2) == 0 && s2.nge == 1 && b2.calls == 1 && r2.gactive[0] == 1);
    }
    // the first step, to tn = 0.001: g0 = tn > 0 like glo -> no root; the function that is identically 0 stays off
    s.nst = 1;
    s.tn = 0.001;
    s.hused = 0.001;
    s.toutc = 1.0;
    CHECK(r_check3(s, rs, 4, be) == IDAENS_UNFINISHED);
    CHECK(rs.iroots[0] == 0.0 && rs.iroots[1] == 0.0 && rs.iroots[2] == 0.0 && rs.iroots[3] == 0.0 && rs.gactive[1] == 0);
    CHECK(rs.gactive[3] == 1 && rs.glo[3] == 0.001 * 0.001);  // t^2 has left 0: switched on again, without a root
    CHECK(s.tlo == 0.001 && rs.glo[0] == 0.001 && s.nge == 3 && be.calls == 3);
    std::puts("ok zero_at_t0");
}

// (d): r_check2 on re-entry after a root return at tlo, with g exactly 0 at tlo
void reentry_after_a_root() {
    Poly p;
    p.c[0][0] = 0.0;   // identically 0: still 0 at tlo + smallh -> CLOSE_ROOTS
    p.c[1][1] = 1.0;   // t
    p.c[2][0] = 3.0;
    for (int arm = 0; arm < 2; ++arm) {  // 0: tlo + smallh is inside the last step (interp), 1: at or past tn (yy += hratio * phi[1])
        Backend be{p, {0}, {0.0}};
        Roots rs(1);
        SysCore s = record(1.0, 0.5, 2.0, arm == 0 ? 0.75 : 1.0);
        s.irfnd = true;
        s.nge = 7;
        CHECK(r_check2(s, rs, 1, be) == IDAENS_CLOSE_ROOTS);
        CHECK(s.nge == 9 && be.calls == 2);
        if (arm == 0) CHECK(be.tcur == 0.75 + ttol_of(s));
        else CHECK(be.tcur == 1.0);
    }
    // g = t - 1 is 0 at tlo = 1 and not at tlo + smallh: the call goes on, glo takes the value after the root
    {
        Backend be{p, {1, 2}, {1.0, 0.0}};
        be.phi1[1] = 0.5;  // hh * y'
        Roots rs(2);
        SysCore s = record(1.0, 0.5, 2.0, 1.0);
        s.irfnd = true;
        CHECK(r_check2(s, rs, 2, be) == IDAENS_UNFINISHED);
        const double ttol = ttol_of(s);
        CHECK(rs.glo[0] == (1.0 + (ttol / 0.5) * 0.5) - 1.0 && rs.glo[0] > 0.0 && rs.iroots[0] == 1.0 && rs.iroots[1] == 0.0);
        CHECK(s.nge == 2 && be.calls == 2);
    }
    // a second function exactly 0 at tlo + smallh: that is a root return of its own
    {
        SysCore s = record(1.0, 0.5, 2.0, 0.75);
        const double tplus = 0.75 + ttol_of(s);
        Backend be{p, {1, 1}, {0.75, tplus}};
        Roots rs(2);
        s.irfnd = true;
        CHECK(r_check2(s, rs, 2, be) == IDAENS_ROOT_RETURN);
        CHECK(rs.iroots[0] == 1.0 && rs.iroots[1] == 1.0 && rs.glo[0] == tplus - 0.75 && s.nge == 2 && be.calls == 2);
    }
    // not after a root return: nothing is evaluated
    {
        Backend be{p, {1}, {1.0}};
        Roots rs(1);
        SysCore s = record(1.0, 0.5, 2.0, 1.0);
        CHECK(r_check2(s, rs, 1, be) == IDAENS_UNFINISHED && be.calls == 0 && s.nge == 0);
    }
    std::puts("ok reentry_after_a_root");
}

// (e): g exactly 0 at thi and no sign change inside the step: a root return from the first scan, without a single bisection
void zero_at_thi() {
    Poly p;
    p.c[0][1] = 1.0; p.c[0][0] = -1.0;  // t - 1
    Backend be{p, {0}, {0.0}};
    Roots rs(1);
    SysCore s = record(1.0, 0.5, 2.0, 0.5);
    rs.glo[0] = -0.5;
    CHECK(r_check3(s, rs, 1, be) == IDAENS_ROOT_RETURN);
    CHECK(s.trout == 1.0 && s.tlo == 1.0 && rs.grout[0] == 0.0 && rs.glo[0] == 0.0 && rs.iroots[0] == -1.0);
    CHECK(s.nge == 1 && be.calls == 1);
    std::puts("ok zero_at_thi");
}

// (f): the modified secant against a restatement for ONE function, written from the method's description: the secant point
// tmid = thi - (thi - tlo) ghi / (ghi - alph glo); alph is 1 unless the last two points fell on the same side of the root, then it
// is doubled (both on tlo's side) or halved (both on thi's side) each time; a point closer than ttol / 2 to an end of the bracket
// is moved to a tenth of the bracket from that end (to 0.5 ttol when the bracket is shorter than 5 ttol).
struct Secant {
    std::vector<double> tmid, alph;
    double tlo, thi;
    int clamped = 0;
};
Secant secant_by_the_book(const Poly& p, int k, double tlo, double thi, double ttol) {
    Secant r;
    double glo = p.at(k, tlo), ghi = p.at(k, thi), alph = 1.0;
    int last = 0, same = 0;  // side of the last point (1: thi's, 2: tlo's) and how many in a row fell there
    while (std::fabs(thi - tlo) > ttol) {
        alph = same >= 2 ? (last == 2 ? alph * 2.0 : alph * 0.5) : 1.0;
        double tm = thi - (thi - tlo) * ghi / (ghi - alph * glo);
        const double frac = std::fabs(thi - tlo) / ttol > 5.0 ? 0.1 : 0.5 / (std::fabs(thi - tlo) / ttol);
        if (std::fabs(tm - tlo) < 0.5 * ttol) { tm = tlo + frac * (thi - tlo); r.clamped += 1; }
        if (std::fabs(thi - tm) < 0.5 * ttol) { tm = thi - frac * (thi - tlo); r.clamped += 1; }
        r.tmid.push_back(tm);
        r.alph.push_back(alph);
        const double gm = p.at(k, tm);
        int side;
        if (gm == 0.0 || glo * gm < 0.0) { thi = tm; ghi = gm; side = 1; }
        else { tlo = tm; glo = gm; side = 2; }
        if (gm == 0.0) break;
        same = side == last ? same + 1 : 1;
        last = side;
    }
    r.tlo = tlo;
    r.thi = thi;
    return r;
}
bool has(const std::vector<double>& v, double x) {
    for (double e : v) if (e == x) return true;
    return false;
}

void illinois_arms() {
    for (int arm = 0; arm < 2; ++arm) {
        Poly p;
        double exact;
        if (arm == 0) {  // t^3 - 0.001 on [0, 1]: convex, the secant's points fall short of the root 0.1 -> alph * 2
            p.c[0][3] = 1.0; p.c[0][0] = -0.001;
            exact = 0.1;
        } else {  // (t - 1)^3 + 0.001: concave, the points overshoot the root 0.9 -> alph * 0.5
            p.c[0][3] = 1.0; p.c[0][2] = -3.0; p.c[0][1] = 3.0; p.c[0][0] = -1.0 + 0.001;
            exact = 0.9;
        }
        Backend be{p, {0}, {0.0}};
        Roots rs(1);
        SysCore s = record(1.0, 1.0, 2.0, 0.0);
        rs.glo[0] = p.at(0, 0.0);
        s.thi = 1.0;
        rs.ghi[0] = p.at(0, 1.0);
        s.ttol = ttol_of(s);
        be.root = exact;
        be.track = true;
        const Secant ref = secant_by_the_book(p, 0, 0.0, 1.0, s.ttol);
        CHECK(root_find(s, rs, 1, be) == IDAENS_ROOT_RETURN);
        // the book's run takes both arms of the weight more than once and comes back to 1 in between
        if (arm == 0) CHECK(has(ref.alph, 2.0) && has(ref.alph, 4.0));
        else CHECK(has(ref.alph, 0.5) && has(ref.alph, 0.25));
        CHECK(ref.alph.size() > 4 && ref.alph.back() >= 0.0 && has(std::vector<double>(ref.alph.begin() + 3, ref.alph.end()), 1.0));
        // point for point the same run: every tmid, hence the number of evaluations, and the final bracket
        CHECK(be.ts == ref.tmid);
        CHECK(be.calls == (long)ref.tmid.size() && s.nge == be.calls);
        CHECK(s.trout == ref.thi && s.thi == ref.thi && s.tlo == ref.tlo);
        CHECK(be.nlo > 0 && be.nhi > 0 && be.calls == be.nlo + be.nhi);
        CHECK((arm == 0 ? be.maxrun_lo : be.maxrun_hi) >= 3);
        CHECK(std::fabs(s.trout - exact) <= s.ttol + 1e-13);  // 1e-13: the cubic's own rounding near its root, |g'| >= 0.03
        CHECK(rs.iroots[0] == -1.0);
    }
    // a point that lands closer than ttol / 2 to an end is moved into the bracket; by hand, with t^2 - 0.0001 on [0, 1]:
    // tmid = 1 - 0.9999 / (0.9999 + 0.0001) = 0.0001, inside ttol / 2 of tlo = 0
    for (int c = 0; c < 2; ++c) {
        Poly p;
        p.c[0][2] = 1.0; p.c[0][0] = -0.0001;
        Backend be{p, {0}, {0.0}};
        Roots rs(1);
        SysCore s = record(1.0, 1.0, 2.0, 0.0);
        rs.glo[0] = p.at(0, 0.0);
        s.thi = 1.0;
        rs.ghi[0] = p.at(0, 1.0);
        s.ttol = c == 0 ? 0.1 : 0.4;  // bracket / ttol = 10 > 5: a tenth of the bracket; = 2.5: the fraction 0.5 / 2.5
        CHECK(root_find(s, rs, 1, be) == IDAENS_ROOT_RETURN);
        CHECK(be.calls == 1 && be.ts.size() == 1 && be.ts[0] == (c == 0 ? 0.1 : 0.5 / (1.0 / 0.4)) && s.trout == be.ts[0] && s.tlo == 0.0);
    }
    {  // the same at thi's end: 0.0001 - (1 - t)^2, tmid = 1 - 0.0001 -> moved to 1 - 0.1 = 0.9, on tlo's side
        Poly p;
        p.c[0][2] = -1.0; p.c[0][1] = 2.0; p.c[0][0] = -1.0 + 0.0001;
        Backend be{p, {0}, {0.0}};
        Roots rs(1);
        SysCore s = record(1.0, 1.0, 2.0, 0.0);
        rs.glo[0] = p.at(0, 0.0);
        s.thi = 1.0;
        rs.ghi[0] = p.at(0, 1.0);
        s.ttol = 0.1;
        CHECK(rs.glo[0] < 0.0 && rs.ghi[0] > 0.0 && p.at(0, 0.9) < 0.0);
        CHECK(root_find(s, rs, 1, be) == IDAENS_ROOT_RETURN);
        CHECK(be.calls == 1 && be.ts[0] == 1.0 - 0.1 * 1.0 && s.tlo == be.ts[0] && s.trout == 1.0);
    }
    // two functions change sign in one step: the search follows the one whose root comes first (the larger |ghi / (ghi - glo)|).
    // t - 0.25 and t - 0.75 on [0, 1]: the secant of t - 0.25 hits its root exactly, one evaluation, and only that root is reported
    for (int order = 0; order < 2; ++order) {
        Poly p;
        p.c[0][1] = 1.0;
        const std::vector<double> thr = order == 0 ? std::vector<double>{0.75, 0.25} : std::vector<double>{0.25, 0.75};
        Backend be{p, {0, 0}, thr};
        Roots rs(2);
        SysCore s = record(1.0, 1.0, 2.0, 0.0);
        rs.glo[0] = -thr[0];
        rs.glo[1] = -thr[1];
        CHECK(r_check3(s, rs, 2, be) == IDAENS_ROOT_RETURN);
        CHECK(s.trout == 0.25 && be.calls == 2 && s.nge == 2);  // g(thi), g(0.25)
        CHECK(rs.iroots[order == 0 ? 1 : 0] == -1.0 && rs.iroots[order == 0 ? 0 : 1] == 0.0);
    }
    std::puts("ok illinois_arms");
}

// (g): the k-th evaluation fails: its code comes back from r_check1/2/3 and nge counts the k - 1 evaluations that succeeded (as the
// host stepper counted before the root finding became shared text: it added to nge after each successful call)
void failing_root_function() {
    Poly p;
    p.c[0][1] = 1.0;                     // t: zero at t0 = 0
    p.c[1][2] = 1.0; p.c[1][0] = -0.5;   // t^2 - 0.5
    for (long k = 1; k <= 2; ++k) {
        Backend be{p, {0}, {0.0}};
        be.fail_at = k;
        Roots rs(1);
        SysCore s;
        s.hh = 0.001;
        CHECK(r_check1(s, rs, 1, be) == IDAENS_RTFUNC_FAIL && s.nge == k - 1 && be.calls == k);
    }
    for (long k = 1; k <= 2; ++k) {
        Backend be{p, {0}, {1.0}};  // t - 1, zero at tlo = 1
        be.phi1[0] = 0.5;
        be.fail_at = k;
        Roots rs(1);
        SysCore s = record(1.0, 0.5, 2.0, 1.0);
        s.irfnd = true;
        s.nge = 10;
        CHECK(r_check2(s, rs, 1, be) == IDAENS_RTFUNC_FAIL && s.nge == 10 + k - 1 && be.calls == k);
    }
    for (long k = 1; k <= 3; ++k) {
        Backend be{p, {1}, {0.0}};
        be.fail_at = k;
        Roots rs(1);
        SysCore s = record(1.0, 0.5, 2.0, 0.5);
        rs.glo[0] = p.at(1, 0.5);
        s.nge = 10;
        CHECK(r_check3(s, rs, 1, be) == IDAENS_RTFUNC_FAIL && s.nge == 10 + k - 1 && be.calls == k);
    }
    std::puts("ok failing_root_function");
}

// (h): the stop tests in both task modes and the three exits of the loop-top checks
void stop_tests_and_loop_top() {
    Poly p;
    Backend be{p, {}, {}};
    // stop_test1, IDA_NORMAL
    SysCore s = record(1.0, 0.5, 0.0, 0.0);
    s.tretlast = 0.75;
    CHECK(stop_test1(s, 0.75, IDAENS_NORMAL, be) == IDAENS_SUCCESS && s.tret == 0.75 && be.nsol == 0);  // tout == tretlast
    CHECK(stop_test1(s, 0.875, IDAENS_NORMAL, be) == IDAENS_SUCCESS && s.tret == 0.875 && s.tretlast == 0.875 && be.nsol == 1 && be.sol_t == 0.875);
    CHECK(stop_test1(s, 1.0, IDAENS_NORMAL, be) == IDAENS_SUCCESS && s.tret == 1.0 && be.nsol == 2);  // tn == tout
    CHECK(stop_test1(s, 1.5, IDAENS_NORMAL, be) == IDAENS_UNFINISHED && s.tret == 1.0 && s.tretlast == 1.0 && be.nsol == 2);
    be.sol_rc = IDAENS_BAD_T;
    CHECK(stop_test1(s, 0.25, IDAENS_NORMAL, be) == IDAENS_BAD_T && s.tret == 1.0 && s.tretlast == 1.0 && be.nsol == 3);
    be.sol_rc = 0;
    s.hh = -0.5;  // backwards in time
    s.tn = -1.0;
    CHECK(stop_test1(s, -0.5, IDAENS_NORMAL, be) == IDAENS_SUCCESS && s.tret == -0.5);
    CHECK(stop_test1(s, -1.5, IDAENS_NORMAL, be) == IDAENS_UNFINISHED);
    // stop_test1, IDA_ONE_STEP: returns tn when tn has moved past the last return
    s = record(1.0, 0.5, 0.0, 0.0);
    s.tretlast = 0.75;
    be.nsol = 0;
    CHECK(stop_test1(s, 9.0, IDAENS_ONE_STEP, be) == IDAENS_SUCCESS && s.tret == 1.0 && s.tretlast == 1.0 && be.nsol == 1 && be.sol_t == 1.0);
    CHECK(stop_test1(s, 9.0, IDAENS_ONE_STEP, be) == IDAENS_UNFINISHED && be.nsol == 1);
    // stop_test2
    s = record(1.0, 0.5, 0.0, 0.0);
    be.nsol = 0;
    CHECK(stop_test2(s, 1.5, IDAENS_NORMAL, be) == IDAENS_UNFINISHED && be.nsol == 0 && s.tret == 0.0);
    CHECK(stop_test2(s, 0.875, IDAENS_NORMAL, be) == IDAENS_SUCCESS && s.tret == 0.875 && s.tretlast == 0.875 && be.nsol == 1 && be.sol_t == 0.875);
    CHECK(stop_test2(s, 9.0, IDAENS_ONE_STEP, be) == IDAENS_SUCCESS && s.tret == 1.0 && s.tretlast == 1.0 && be.nsol == 1);
    // loop_top: too many steps in this call (the system is not dead: the next call goes on)
    s = record(1.0, 0.5, 0.0, 0.0);
    s.ph = PH_LOOP_TOP;
    s.nstloc = 500;
    s.phi0nrm = 1.0;
    be.nsol = 0;
    CHECK(!loop_top(s, 500, be) && s.status == IDAENS_TOO_MUCH_WORK && s.ph == PH_IDLE && !s.dead && s.tret == 1.0 && s.tretlast == 1.0 && be.nsol == 0);
    s.ph = PH_LOOP_TOP;
    CHECK(loop_top(s, 0, be) && loop_top(s, 501, be) && s.ph == PH_LOOP_TOP && s.tolsf == F64_EPS);  // 0: no limit
    // bad error weights after a step
    s.ewt_bad = true;
    CHECK(!loop_top(s, 501, be) && s.status == IDAENS_ILL_INPUT && s.ph == PH_IDLE && s.dead && s.tret == 1.0 && be.nsol == 1 && be.sol_t == 1.0);
    s = SysCore();  // before the first step the weights of y0 are the caller's matter
    s.ph = PH_LOOP_TOP;
    s.ewt_bad = true;
    s.phi0nrm = 1.0;
    CHECK(loop_top(s, 500, be));
    // too much accuracy requested: at the first step (no interpolation) and later
    s.phi0nrm = 3.0 / F64_EPS;
    CHECK(!loop_top(s, 500, be) && s.status == IDAENS_TOO_MUCH_ACC && s.tolsf == F64_EPS * (3.0 / F64_EPS) * 10.0 && s.dead && s.ph == PH_IDLE && be.nsol == 1);
    s = record(1.0, 0.5, 0.0, 0.0);
    s.ph = PH_LOOP_TOP;
    s.phi0nrm = 3.0 / F64_EPS;
    CHECK(!loop_top(s, 500, be) && s.status == IDAENS_TOO_MUCH_ACC && s.tret == 1.0 && be.nsol == 2);
    std::puts("ok stop_tests_and_loop_top");
}

// the entry of a call: without root functions (NoRoots: no root code is instantiated), and IDA_ONE_STEP's return after a root
void call_entry() {
    Poly p;
    p.c[0][1] = 1.0;
    {
        Backend be{p, {}, {}};
        NoRoots none;
        SysCore s = record(1.0, 0.5, 0.0, 0.0);
        s.tout_cur = 2.0;
        s.nstloc = 9;
        CHECK(enter_call(s, none, 0, IDAENS_NORMAL, be) == IDAENS_UNFINISHED && s.nstloc == 0 && s.toutc == 2.0 && s.taskc == IDAENS_NORMAL);
        s.tout_cur = 0.75;
        CHECK(enter_call(s, none, 0, IDAENS_NORMAL, be) == IDAENS_SUCCESS && s.tret == 0.75 && be.nsol == 1);
        s.nst = 0;  // the first call never returns from the entry
        CHECK(enter_call(s, none, 0, IDAENS_NORMAL, be) == IDAENS_UNFINISHED);
    }
    {  // the last return was a root at tlo = 0.75 (g = t - 0.75); tn = 1: no further root up to tn -> ONE_STEP returns tn
        Backend be{p, {0}, {0.75}};
        be.phi1[0] = 0.5;
        Roots rs(1);
        SysCore s = record(1.0, 0.5, 2.0, 0.75);
        s.irfnd = true;
        s.tretlast = 0.75;
        s.tout_cur = 2.0;
        CHECK(enter_call(s, rs, 1, IDAENS_ONE_STEP, be) == IDAENS_SUCCESS && s.tret == 1.0 && !s.irfnd && s.toutc == 2.0 && be.nsol == 1);
        CHECK(s.nge == be.calls && be.calls == 3);  // r_check2: tlo and tlo + smallh; r_check3: thi
        // the same entry in IDA_NORMAL goes on stepping towards tout = 2
        Backend b2{p, {0}, {0.75}};
        Roots r2(1);
        s = record(1.0, 0.5, 2.0, 0.75);
        s.irfnd = true;
        s.tretlast = 0.75;
        s.tout_cur = 2.0;
        CHECK(enter_call(s, r2, 1, IDAENS_NORMAL, b2) == IDAENS_UNFINISHED && !s.irfnd && b2.nsol == 0 && s.nge == 3);
    }
    {  // the last return was a root exactly at tn = tretlast: nothing new to search, r_check3 is not run (irfnd stays as it is)
        Backend be{p, {0}, {1.0}};
        be.phi1[0] = 0.5;
        Roots rs(1);
        SysCore s = record(1.0, 0.5, 2.0, 1.0);
        s.irfnd = true;
        s.tretlast = 1.0;
        s.tout_cur = 2.0;
        CHECK(enter_call(s, rs, 1, IDAENS_NORMAL, be) == IDAENS_UNFINISHED && s.irfnd && s.nge == 2 && be.calls == 2 && be.ts.size() == 1);
    }
    std::puts("ok call_entry");
}

}  // namespace

int main() {
    bracket_a_root();
    zero_at_t0();
    reentry_after_a_root();
    zero_at_thi();
    illinois_arms();
    failing_root_function();
    stop_tests_and_loop_top();
    call_entry();
    std::puts("all ok");
    return 0;
}
