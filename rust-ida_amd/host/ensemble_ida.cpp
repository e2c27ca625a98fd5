// libidaens.so -- host-side BDF stepper for an ensemble of independent IVPs (implementation of
// include/ida_ensemble.h). Mirrors, per system and with the same names, the scalar logic of the reference:
//   Ida::solve            /root/reference/src/impl_solve.rs:69-376
//   Ida::step             /root/reference/src/lib.rs:613-711
//   set_coeffs            /root/reference/src/lib.rs:722-782
//   nonlinear_solve       /root/reference/src/lib.rs:787-890      (lsetup decision, ss resets)
//   Newton::solve         /root/reference/crates/nonlinear/src/newton.rs:51-167   (as a batched state machine)
//   idaNlsConvTest        /root/reference/src/ida_nls.rs:218-266   (host libm pow)
//   test_error            /root/reference/src/lib.rs:967-1039      (decisions; the norms come from the device)
//   restore               /root/reference/src/lib.rs:1044-1083
//   handle_n_flag         /root/reference/src/lib.rs:1120-1244
//   complete_step         /root/reference/src/impl_complete_step.rs:22-177
//   get_solution          /root/reference/src/lib.rs:1274-1343      (coefficients; the sums run on the device)
//   get_dky               /root/reference/src/lib.rs:424-529        (coefficients; quirk Q9: C IDA's loop bound)
//   stop_test1/2, r_check1/2/3, root_finding and the per-system pieces of Ida::solve: ida_solve_flow.hpp, shared with the device
//                         steppers like the controller (here: the backend HostFlow, y(t) interpolated on the device)
//   calc_ic               C IDA's IDACalcIC as DESIGN.md section 4f states it (the reference has none, src/lib.rs:328-335)
// Vectors live on the device; this file talks to it only through include/ida_hip.h. The oracle is NOT used here.
//
// Lock-step execution: one "round" is one step attempt (set_coeffs -> predict -> Newton -> error test -> accept or
// restore) for every system that still has to reach tout; systems diverge freely in h, order, Newton count and
// lsetup timing, the device calls act on compacted index lists.
//
// Deviations from the reference text, identical to the oracle's: Q1 (jac at tn), Q2 (LU failure is a
// recoverable lsetup failure), Q3 (Newton breaks out on ConvergenceRecover with a current Jacobian), Q4 (Newton
// ConvergenceRecover is recoverable at step level), Q5 (reset() rescales phi[1] only), Q15 (ONE_STEP's TSTOP return consumes the stop
// time). The stop time is per system (idaens_set_stop_time) and lives in SysCore, so it travels to the device steppers.
//
// A system whose solve call ended in a fatal IdaError (too much work, error-test or convergence failures, ...) is `dead`:
// the reference's Ida::solve could be called again after such an error and would try to continue; here the status is
// sticky -- later calls skip the system and report the same status (include/ida_ensemble.h says so).
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <chrono>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ida_ensemble.h"

#include "ida_solve_flow.hpp"

namespace {

using namespace idactl;  // constants, SysCore, the scalar controller and Ida::solve's per-system flow, shared with the device steppers

// root finding (src/lib.rs:225-244, src/impl_r_check.rs): the root state of ida_solve_flow.hpp; nrtfn entries when roots are enabled
struct RootVecs {
    std::vector<double> glo, ghi, grout, iroots;
    std::vector<int32_t> gactive;
};
template <class D, class S>
void copy_roots(D& d, const S& s, int nr) {  // between RootVecs and the device steppers' idahip_root_state
    for (int i = 0; i < nr; ++i) {
        d.glo[i] = s.glo[i]; d.ghi[i] = s.ghi[i]; d.grout[i] = s.grout[i];
        d.iroots[i] = s.iroots[i]; d.gactive[i] = s.gactive[i];
    }
}

struct Sys : SysCore {
    RootVecs rt;
    long nbacktr = 0;  // idaens_calc_ic: line-search backtracks (host-only: SysCore's size is part of the device steppers' ABI)
    long npe = 0, nps = 0;  // band preconditioner of a Krylov ctx: setups and solves (C IDA's npe, nps; host-only as well)
    double t_start = 0.0;   // the t0 this system was created or last reinitialised at (idaens_reinit); idaens_stream restarts at e->t0
    bool returned = false;  // a solve call has returned for this system since then: yy / yp on the device hold what it reported
};

}  // namespace

struct idaens {
    idahip_ctx* ctx = nullptr;
    int n = 0, batch = 0;
    std::vector<Sys> sys;
    std::string err;
    long mxstep = MXSTEP_DEFAULT;
    int maxord = MAXORD_DEFAULT;
    long maxncf = MXNCF, maxnef = MXNEF;
    double epcon = EPCON, hmax_inv = 0.0;
    int64_t total_rounds = 0;
    int trace_sys = -1;
    std::vector<double> trace;
    bool sched_unfinished = false;  // the last idaens_solve_schedule call stopped at its round limit
    double t0 = 0.0;                // every system starts at tn = t0 (Sys default)
    int64_t retired_iters = 0, passes = 0;  // idaens_stream: Newton iterations / integrations of systems already restarted
    bool have_ic = false, streaming = false;
    bool started = false;  // a solve / solve_schedule / stream call has been made: idaens_calc_ic is refused from then on
    bool constr = false;   // the ctx has constraints (idahip_set_constraints): read at the start of every solve / solve_schedule / stream call
    bool pow_mismatch = false; // glibc_pow.hpp != this host's std::pow (checked at create): the device steppers stay off
    bool device_ctl = true;    // small device problems: the whole of Ida::solve in one launch (idahip_tiny_solve), no lock-step rounds
    bool fused_newton = true;  // first two Newton iterations and their convergence tests in one device call (idahip_newton_iter2)
    std::vector<int64_t> start_round;  // idaens_stream with a stagger: the round at which each system first enters
    // root functions g_i(t, y, y') = y[rt_comp[i]] - rt_thr[i] (the form of the reference's Roberts example,
    // src/sample_problems/roberts.rs: g0 = y0 - 1e-4, g1 = y2 - 0.01); nrtfn == 0: no root finding
    int nrtfn = 0;
    std::vector<int32_t> rt_comp;
    std::vector<double> rt_thr;
    idaens_root_fn rt_fn = nullptr;  // or any host function (idaens_set_root_fn)
    void* rt_user = nullptr;
    std::vector<double> hy, hyp;  // host copies of one system's y, y' for the root functions
    // scratch for list calls
    std::vector<int32_t> idx, ia, ib;
    std::vector<double> da, db, dc, dd;
};

namespace {

int efail(idaens* e, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    e->err = buf;
    return code;
}

// IDAENS_PROFILE=1 in the environment: wall time inside device-library calls vs in this file's own host logic, printed
// by idaens_destroy (development aid for the host/device balance of a round)
static double g_prof_dev = 0.0, g_prof_t0 = -1.0;
static const bool g_prof = std::getenv("IDAENS_PROFILE") != nullptr;
static double prof_now() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
}
#define ENS_CALL(e, call)                                                                                   \
    do {                                                                                                    \
        const double t0__ = g_prof ? prof_now() : 0.0;                                                      \
        int rc__ = (call);                                                                                  \
        if (g_prof) g_prof_dev += prof_now() - t0__;                                                        \
        if (rc__ < 0) return efail((e), rc__, "%s failed (%d): %s", #call, rc__, idahip_last_error((e)->ctx)); \
    } while (0)

struct SolList {  // systems whose yy/yp must be interpolated by the device
    std::vector<int32_t> idx, kord;
    std::vector<double> cvals, dvals;
    void add(int b, const Sys& s, int kord_) {
        idx.push_back(b);
        kord.push_back(kord_);
        cvals.insert(cvals.end(), s.cvals, s.cvals + MXORDP1);
        dvals.insert(dvals.end(), s.dvals, s.dvals + MAXORD_DEFAULT);
    }
};

// get_solution(t) for system b: coefficients now, device sums deferred to the list. Returns 0 or IDAENS_BAD_T.
int queue_solution(Sys& s, int b, double t, SolList& sl) {
    int kord = 1;
    const int rc = get_solution_coeffs(s, t, &kord);
    if (rc) return rc;
    sl.add(b, s, kord);
    return 0;
}

int flush_solutions(idaens* e, SolList& sl) {
    if (sl.idx.empty()) return 0;
    ENS_CALL(e, idahip_get_solution(e->ctx, sl.kord.data(), sl.cvals.data(), sl.dvals.data(), sl.idx.data(), (int)sl.idx.size()));
    sl = SolList();
    return 0;
}

// ---------------------------------------------------------------- the backend of ida_solve_flow.hpp for system b
// Roots are rare events of single systems: the bracketing (ida_solve_flow.hpp) runs system by system on the host, with the device
// interpolating y(t), y'(t) (idahip_get_solution) and the two vectors coming back to e->hy, e->hyp for the root functions.
struct HostFlow {
    idaens* e;
    int b;
    SolList& sl;
    int solution_at(double t) { return queue_solution(e->sys[b], b, t, sl); }
    // get_solution(t) of system b on the device now (yy, yp of that system become y(t), y'(t), lib.rs:1274)
    int interp(double t) {
        Sys& s = e->sys[b];
        int kord = 1;
        const int rc = get_solution_coeffs(s, t, &kord);
        if (rc) return rc;
        const int32_t ib = b, ko = kord;
        ENS_CALL(e, idahip_get_solution(e->ctx, &ko, s.cvals, s.dvals, &ib, 1));
        ENS_CALL(e, idahip_download(e->ctx, IDAHIP_F_YY, b, 1, e->hy.data()));
        ENS_CALL(e, idahip_download(e->ctx, IDAHIP_F_YP, b, 1, e->hyp.data()));
        return 0;
    }
    int eval(double t, double* g) {
        if (e->rt_fn) return e->rt_fn(e->rt_user, b, t, e->hy.data(), e->hyp.data(), e->nrtfn, g) == 0 ? 0 : IDAENS_RTFUNC_FAIL;
        for (int i = 0; i < e->nrtfn; ++i) g[i] = e->hy[e->rt_comp[i]] - e->rt_thr[i];
        return 0;
    }
    int eval_start(double* g) {
        ENS_CALL(e, idahip_download(e->ctx, IDAHIP_F_PHI0, b, 1, e->hy.data()));
        ENS_CALL(e, idahip_download(e->ctx, (idahip_field)(IDAHIP_F_PHI0 + 1), b, 1, e->hyp.data()));
        return eval(e->sys[b].tn, g);
    }
    int yy_from_phi01(double f) {  // r_check1 only, after eval_start: hy, hyp hold phi[0], phi[1] (the callback keeps seeing phi[1] as y')
        for (int i = 0; i < e->n; ++i) e->hy[i] = e->hy[i] + f * e->hyp[i];
        ENS_CALL(e, idahip_upload(e->ctx, IDAHIP_F_YY, b, 1, e->hy.data()));
        return 0;
    }
    int yy_add_phi1(double f) {  // after interp: hy holds yy
        std::vector<double> p1(e->n);
        ENS_CALL(e, idahip_download(e->ctx, (idahip_field)(IDAHIP_F_PHI0 + 1), b, 1, p1.data()));
        for (int i = 0; i < e->n; ++i) e->hy[i] = e->hy[i] + f * p1[i];
        ENS_CALL(e, idahip_upload(e->ctx, IDAHIP_F_YY, b, 1, e->hy.data()));
        return 0;
    }
};

// residual evaluations of one band DQ Jacobian (idaLsBandDQJac): min(ml + mu + 1, n)
long dq_band_evals(idaens* e) {
    int ml = 0, mu = 0;
    idahip_band(e->ctx, &ml, &mu);
    return std::min<long>((long)ml + mu + 1, (long)e->n);
}

// ---------------------------------------------------------------- the batched Newton solve (newton.rs:51-167)
// `act`: systems taking a step attempt this round, with s.call_lsetup decided. Sets s.nls_ret.
int newton_solve_batched(idaens* e, const std::vector<int32_t>& act) {
    std::vector<Sys>& S = e->sys;
    std::vector<int32_t> R(act), I, C, L, P;
    std::vector<double> tn, cj, hh, sc, nrm;
    std::vector<int32_t> info;
    // the arguments of a listed device call: tn / cj / hh of the list's systems
    auto gather = [&](const std::vector<int32_t>& list) {
        tn.clear(); cj.clear(); hh.clear();
        for (int b : list) { tn.push_back(S[b].tn); cj.push_back(S[b].cj); hh.push_back(S[b].hh); }
    };
    while (!R.empty() || !I.empty()) {
        if (!R.empty()) {
            // sys(y0), y <- y0 = 0 (newton.rs:73); the systems whose Newton solve then calls setup (call_lsetup) get both
            // in one device call, the others sys alone
            L.clear(); P.clear();
            // a DQ ctx (idahip_set_jacobian_dq): sys for all of them, then the setups with their step sizes
            const bool dq = idahip_jacobian_dq(e->ctx) > 0;
            // a Krylov ctx (idahip_create_krylov): sys for all of them; without a preconditioner its linear setup forms and factors
            // nothing and cannot fail
            const bool kry = idahip_krylov(e->ctx, nullptr) == 1;
            for (int b : R) (S[b].call_lsetup && !dq && !kry ? L : P).push_back(b);
            if (!P.empty()) {
                gather(P);
                ENS_CALL(e, idahip_nls_sys(e->ctx, tn.data(), cj.data(), 1, P.data(), (int)P.size()));
            }
            for (int b : R) S[b].nre += 1;
            int pml = 0, pmu = 0;
            const bool prec = kry && idahip_krylov_band_prec(e->ctx, &pml, &pmu) == 1;
            if (kry)
                for (int b : R)
                    if (S[b].call_lsetup) after_lsetup_nojac(S[b]);  // idaNlsLSetup's bookkeeping; no Jacobian: nje stays
            if (prec) {
                // the band preconditioner: P is formed at the residual that sys has just left and factored; a zero
                // pivot is the recoverable setup failure of a direct solver
                for (int b : R)
                    if (S[b].call_lsetup) L.push_back(b);
                if (!L.empty()) {
                    gather(L);
                    info.assign(L.size(), 0);
                    ENS_CALL(e, idahip_krylov_psetup(e->ctx, tn.data(), cj.data(), hh.data(), info.data(), L.data(), (int)L.size()));
                    const long evals = std::min<long>((long)pml + pmu + 1, (long)e->n);
                    for (size_t q = 0; q < L.size(); ++q) {
                        Sys& s = S[L[q]];
                        s.nls_ret = info[q] ? NLS_LSETUP_RECVR : NLS_SUCCESS;
                        s.npe += 1;
                        s.nre_dq += evals;
                    }
                    L.clear();
                }
            }
            if (dq)
                for (int b : R)
                    if (S[b].call_lsetup) L.push_back(b);
            if (!L.empty() && dq) {
                gather(L);
                info.assign(L.size(), 0);
                ENS_CALL(e, idahip_nls_lsetup_dq(e->ctx, tn.data(), cj.data(), hh.data(), info.data(), L.data(), (int)L.size()));
                const long evals = idahip_band(e->ctx, nullptr, nullptr) > 0 ? dq_band_evals(e) : (long)e->n;
                for (size_t q = 0; q < L.size(); ++q) {
                    Sys& s = S[L[q]];
                    s.nre_dq += evals;
                    after_lsetup(s, info[q]);
                }
            } else if (!L.empty()) {
                gather(L);
                info.assign(L.size(), 0);
                ENS_CALL(e, idahip_nls_sys_setup(e->ctx, tn.data(), cj.data(), 1, info.data(), L.data(), (int)L.size()));
                for (size_t q = 0; q < L.size(); ++q) {
                    Sys& s = S[L[q]];
                    after_lsetup(s, info[q]);  // idaNlsLSetup / idaLsSetup bookkeeping (ida_nls.rs:168-179, ida_ls.rs:250)
                }
            }
            for (int b : R)
                if (newton_begin(S[b], S[b].call_lsetup)) I.push_back(b);
            R.clear();
        }
        if (I.empty()) break;
        sc.clear();
        const int lst = idahip_ls_type(e->ctx);
        if (lst == IDAHIP_LS_DIRECT) {   // idaLsSolve's bookkeeping around LSolver::solve (ida_ls.rs:316-418): the solver's type decides the tolerance it is
            // given (0 for a direct solver: idahip_ls_solve ignores it), the nli / ncfl counters and whether the correction is
            // scaled by 2 / (1 + cjratio) (:405-410). The dense and band solvers are Direct with no iterations and no failures.
            const long nli_inc = idahip_ls_num_iters(e->ctx);
            // tol = sqrt(N) * eplifac for an iterative solver, 0 for a direct one (:323-329; eplifac = 0.05, :211). The fused
            // iteration kernel is LSolver::solve of the DIRECT solver and takes no tolerance: anything else has no kernel here.
            const double tol = lsolve_tol(lst, std::sqrt((double)e->n), EPLIFAC);
            if (tol != 0.0) return efail(e, -3, "LSolverType %d (tol %g): a direct solver takes no tolerance", lst, tol);
            for (int b : I) sc.push_back(after_lsolve(S[b], lst, nli_inc, false) ? 2.0 / (1.0 + S[b].cjratio) : 1.0);
        } else if (lst != IDAHIP_LS_ITERATIVE) {
            return efail(e, -3, "LSolverType %d: only the direct solvers and the matrix-free SPGMR of a Krylov ctx are implemented", lst);
        }
        C.clear();
        // what follows a convergence test is newton_after_ctest's (ida_controller.hpp); here: iterate = list C (sys(y), then the next
        // pass), restart = list R, done = on no list
        auto after_ctest = [&](int b, int ret, bool converged) {
            const NewtonNext next = newton_after_ctest(S[b], ret, converged);
            if (next == NEWTON_ITERATE) C.push_back(b);
            else if (next == NEWTON_RESTART) R.push_back(b);
        };
        bool all_fresh = e->fused_newton && lst == IDAHIP_LS_DIRECT;
        for (int b : I) all_fresh = all_fresh && S[b].curiter == 0;
        if (lst == IDAHIP_LS_ITERATIVE) {
            // the Newton body of a Krylov ctx: the solver's tolerance is (sqrt(N) * eplifac) * eps_newt, formed by the
            // library from eps_newt; the correction is not scaled (ida_ls.rs:405-410); nli / ncfl through after_lsolve; the residual
            // evaluations of the difference quotients (one per linear iteration) go to nre_dq; every flag other than SUCCESS is
            // recoverable and takes Newton's ConvergenceRecover exit (newton.rs:146-153), ee left alone
            gather(I);
            std::vector<double> epsv;
            for (int b : I) epsv.push_back(S[b].eps_newt);
            nrm.assign(I.size(), 0.0);
            std::vector<int32_t> nli(I.size(), 0), lflag(I.size(), 0);
            const bool prec_on = idahip_krylov_band_prec(e->ctx, nullptr, nullptr) == 1;
            ENS_CALL(e, idahip_newton_iter_krylov(e->ctx, tn.data(), cj.data(), epsv.data(), nrm.data(), nli.data(), lflag.data(), I.data(), (int)I.size()));
            for (size_t q = 0; q < I.size(); ++q) {
                const int b = I[q];
                Sys& s = S[b];
                s.niters += 1;
                (void)after_lsolve(s, lst, nli[q], lflag[q] != 0);
                s.nre_dq += nli[q];
                if (prec_on) s.nps += 1 + nli[q];
                if (lflag[q] != 0) {
                    after_ctest(b, NLS_CONV_RECVR, false);
                    continue;
                }
                bool converged = false;
                const int ret = conv_test(s, nrm[q], &converged);
                after_ctest(b, ret, converged);
            }
        } else if (all_fresh) {
            // the first two iterations in one device call: both convergence tests are decided there (ctest_kernel<0>, <1>: the same
            // conv_test_core, no pow for m <= 1); the scalar state is brought up to date here by replaying the two tests, and what
            // follows them, over the two norms it returns. The device's flags say whether the second iteration ran.
            gather(I);
            std::vector<double> told, ssv, epsv;
            for (int b : I) { told.push_back(S[b].toldel); ssv.push_back(S[b].ss); epsv.push_back(S[b].eps_newt); }
            nrm.assign(2 * I.size(), 0.0);
            std::vector<int32_t> conv(I.size(), 0);
            ENS_CALL(e, idahip_newton_iter2(e->ctx, sc.data(), tn.data(), cj.data(), told.data(), ssv.data(), epsv.data(), nrm.data(),
                                            conv.data(), I.data(), (int)I.size()));
            for (size_t q = 0; q < I.size(); ++q) {
                const int b = I[q];
                Sys& s = S[b];
                bool converged = false;
                s.niters += 1;
                int ret = conv_test(s, nrm[2 * q], &converged);  // m = 0: never a failure
                // the device's flag decides whether the second iteration ran (newton_after_ctest itself, not the lambda: the device
                // has run this sys(y) already, the system joins no list yet)
                if (newton_after_ctest(s, ret, conv[q] == 1) != NEWTON_ITERATE) continue;
                s.nre += 1;
                s.niters += 1;
                ret = conv_test(s, nrm[2 * q + 1], &converged);  // m = 1
                after_ctest(b, ret, converged);
            }
        } else {
        nrm.assign(I.size(), 0.0);
        ENS_CALL(e, idahip_newton_iter(e->ctx, sc.data(), nrm.data(), I.data(), (int)I.size()));
        for (size_t q = 0; q < I.size(); ++q) {
            const int b = I[q];
            Sys& s = S[b];
            s.niters += 1;
            bool converged = false;
            const int ret = conv_test(s, nrm[q], &converged);  // idaNlsConvTest (ida_nls.rs:218-266)
            after_ctest(b, ret, converged);
        }
        }
        if (!C.empty()) {
            gather(C);
            ENS_CALL(e, idahip_nls_sys(e->ctx, tn.data(), cj.data(), 0, C.data(), (int)C.size()));
            for (int b : C) S[b].nre += 1;
        }
        I.swap(C);
    }
    return 0;
}

// ---------------------------------------------------------------- one idaens_solve / idaens_solve_schedule call
// A schedule touts[0..ntout) means: for every system, Ida::solve(touts[0]), then Ida::solve(touts[1]), ... -- but a
// system that returns from one call enters the next at once instead of waiting for the slowest system of the batch, so
// the lock-step rounds stay full. Each return is processed exactly as the reference does (stop tests, interpolation
// to tout).
struct SolveCall {
    const double* touts = nullptr;
    int ntout = 1;
    int itask = IDAENS_NORMAL;
    SolList sl;                                 // interpolations queued for the device
    std::vector<std::pair<int, int>> reached;   // (system, schedule index) whose output is in sl
    double *hYout = nullptr, *hYPout = nullptr; // optional [ntout][batch][n]
    int32_t* hReached = nullptr;                // optional [batch]: returns with IDAENS_SUCCESS so far
    bool recycle = false;                       // idaens_stream: a system that finished the schedule starts over at once
};

// run the queued interpolations, hand the outputs of the touts reached since the last call to the caller
int emit_outputs(idaens* e, SolveCall& C) {
    int rc = flush_solutions(e, C.sl);
    if (rc) return rc;
    if (C.hYout || C.hYPout) {
        const size_t n = e->n, bn = (size_t)e->batch * n;
        for (const auto& r : C.reached) {
            if (C.hYout) ENS_CALL(e, idahip_download(e->ctx, IDAHIP_F_YY, r.first, 1, C.hYout + r.second * bn + r.first * n));
            if (C.hYPout) ENS_CALL(e, idahip_download(e->ctx, IDAHIP_F_YP, r.first, 1, C.hYPout + r.second * bn + r.first * n));
        }
    }
    C.reached.clear();
    return 0;
}

// ---------------------------------------------------------------- one lock-step round over `act`
int continue_schedule(idaens* e, SolveCall& C, int b);

int attempt_round(idaens* e, std::vector<int32_t>& act, SolveCall& C) {
    SolList& sl = C.sl;
    const int itask = C.itask;
    std::vector<Sys>& S = e->sys;
    const int na = (int)act.size();
    // --- step() prologue + set_coeffs + tn += hh (lib.rs:619-653)
    // A system the device lock-step stepper left inside an attempt whose Newton solve must start over with a linear setup
    // (newton_retry: round_ida.hpp's round_newton_ctl_kernel, "in the next round") has had its begin_attempt and its prediction:
    // here it only joins the Newton solve, with call_lsetup set (a round-limited device call followed by a host-stepper call).
    std::vector<int32_t> pred, kkns;
    std::vector<double> beta, gamma;
    for (int q = 0; q < na; ++q) {
        Sys& s = S[act[q]];
        if (s.newton_retry) {
            s.newton_retry = false;
            s.call_lsetup = true;
            continue;
        }
        begin_attempt(s);  // step() prologue, set_coeffs, tn += hh, lsetup decision (ida_controller.hpp)
        pred.push_back(act[q]);
        kkns.push_back(s.kk);
        kkns.push_back(s.ns);
        beta.insert(beta.end(), s.beta, s.beta + MXORDP1);
        gamma.insert(gamma.end(), s.gamma, s.gamma + MXORDP1);
    }
    if (!pred.empty()) ENS_CALL(e, idahip_predict(e->ctx, kkns.data(), beta.data(), gamma.data(), pred.data(), (int)pred.size()));

    // --- Newton
    int rc = newton_solve_batched(e, act);
    if (rc) return rc;

    // --- final yy/yp + error-test norms (lib.rs:845-849, 983-1004; impl_complete_step.rs:74-77)
    std::vector<double> cj(na), norms(4 * (size_t)na);
    std::vector<int32_t> kk(na);
    for (int q = 0; q < na; ++q) {
        cj[q] = S[act[q]].cj;
        kk[q] = S[act[q]].kk;
    }
    // with constraints: the same launch also checks the new yy of the systems whose Newton solve succeeded
    // and either corrects ee before the norms are formed (flag 1) or asks for a shorter step (flag 2, with rr)
    std::vector<int32_t> cflag;
    std::vector<double> crr;
    if (e->constr) {
        std::vector<double> epsn(na);
        std::vector<int32_t> check(na);
        cflag.resize(na);
        crr.resize(na);
        for (int q = 0; q < na; ++q) {
            epsn[q] = S[act[q]].eps_newt;
            check[q] = S[act[q]].nls_ret == NLS_SUCCESS ? 1 : 0;
        }
        ENS_CALL(e, idahip_post_newton_constr(e->ctx, cj.data(), kk.data(), epsn.data(), check.data(), norms.data(), cflag.data(), crr.data(),
                                              act.data(), na));
    } else {
        ENS_CALL(e, idahip_post_newton(e->ctx, cj.data(), kk.data(), norms.data(), act.data(), na));
    }

    // --- decisions
    std::vector<int32_t> rest_idx, rest_kkns, done_idx, done_kused, reset_idx;
    std::vector<double> rest_cvals, done_ck, reset_fac;
    std::vector<int32_t> next;
    for (int q = 0; q < na; ++q) {
        const int b = act[q];
        Sys& s = S[b];
        HostFlow be{e, b, sl};
        double err_k, err_km1;
        const int nflag = attempt_nflag(s, e->constr ? cflag[q] : 0, e->constr ? crr[q] : 0.0, &norms[4 * q], &err_k, &err_km1);
        if (nflag != NFLAG_NONE) {
            // restore (with the kk/ns/beta of this attempt), then handle_n_flag
            const int kk_att = s.kk, ns_att = s.ns;
            restore_scalars(s);
            if (ns_att <= kk_att) {
                rest_idx.push_back(b);
                rest_kkns.push_back(kk_att);
                rest_kkns.push_back(ns_att);
                rest_cvals.insert(rest_cvals.end(), s.cvals, s.cvals + MXORDP1);
            }
            const int kflag = handle_n_flag(s, nflag, err_k, err_km1, e->maxnef, e->maxncf);
            if (kflag != 0) {
                step_failed(s, kflag, be);
                continue;
            }
            if (s.nst == 0) {  // reset(): psi[0] = hh; phi[1] *= rr  (Q5)
                first_step_reset(s);
                reset_idx.push_back(b);
                reset_fac.push_back(s.rr);
            }
            next.push_back(b);  // predict again
            continue;
        }
        // accepted: complete_step (scalars now, vectors below), ee *= ck
        complete_step_scalars(s, err_k, err_km1, norms[4 * q + 3], e->maxord, e->hmax_inv);
        done_idx.push_back(b);
        done_kused.push_back(s.kused);
        done_ck.push_back(s.ck);
        if (b == e->trace_sys) {
            e->trace.push_back(s.tn);
            e->trace.push_back(s.hused);
            e->trace.push_back((double)s.kused);
        }
    }
    if (!rest_idx.empty())
        ENS_CALL(e, idahip_restore(e->ctx, rest_kkns.data(), rest_cvals.data(), rest_idx.data(), (int)rest_idx.size()));
    if (!reset_idx.empty()) ENS_CALL(e, idahip_scale_phi1(e->ctx, reset_fac.data(), reset_idx.data(), (int)reset_idx.size()));
    if (!done_idx.empty()) {
        std::vector<double> p0(done_idx.size());
        std::vector<int32_t> bad(done_idx.size());
        ENS_CALL(e, idahip_complete_step(e->ctx, done_kused.data(), done_ck.data(), e->maxord, p0.data(), bad.data(), done_idx.data(),
                                         (int)done_idx.size()));
        for (size_t q = 0; q < done_idx.size(); ++q) {
            const int b = done_idx[q];
            Sys& s = S[b];
            s.phi0nrm = p0[q];
            s.ewt_bad = bad[q] != 0;
            s.nstloc += 1;
            s.ph = PH_LOOP_TOP;
            HostFlow be{e, b, sl};
            if (root_return_after_step(s, s.rt, e->nrtfn, be)) continue;
            const int istate = stop_test2(s, s.tout_cur, itask, be);
            if (istate != IDAENS_UNFINISHED) {
                s.status = istate;
                s.ph = PH_IDLE;
                const int cs = continue_schedule(e, C, b);  // the next tout of the schedule, if there is one
                if (cs < 0) return cs;
                if (cs == 1) next.push_back(b);
            } else {
                next.push_back(b);
            }
        }
    }
    act.swap(next);
    return 0;
}

}  // namespace

extern "C" {

int idaens_create(idaens** out, idahip_ctx* ctx, const double* hYY0, const double* hYP0) {
    if (!out || !ctx || !hYY0 || !hYP0) return -1;
    // a mass-action ctx without its network has no problem to step (the text is in idahip_last_error)
    if (idahip_kind(ctx) == IDAHIP_MASS_ACTION && idahip_mass_action_pattern(ctx, nullptr, nullptr, nullptr) != 0) return -2;
    idaens* e = new idaens();
    if (g_prof && g_prof_t0 < 0.0) g_prof_t0 = prof_now();
    e->ctx = ctx;
    e->n = idahip_n(ctx);
    e->batch = idahip_batch(ctx);
    // a host residual cannot run between two device iterations; a Krylov ctx has its own Newton body
    e->fused_newton = idahip_kind(ctx) != IDAHIP_HOST_CALLBACK && idahip_krylov(ctx, nullptr) != 1;
    e->sys.resize(e->batch);
    // Ida::new (lib.rs:291-293): phi[0] = yy0, phi[1] = yp0; yy/yp start as yy0/yp0 (ida_nls.rs:83-84)
    int rc = idahip_upload(ctx, IDAHIP_F_PHI0, 0, e->batch, hYY0);
    if (!rc) rc = idahip_upload(ctx, (idahip_field)(IDAHIP_F_PHI0 + 1), 0, e->batch, hYP0);
    if (!rc) rc = idahip_upload(ctx, IDAHIP_F_YY, 0, e->batch, hYY0);
    if (!rc) rc = idahip_upload(ctx, IDAHIP_F_YP, 0, e->batch, hYP0);
    if (rc) {
        delete e;
        return rc;
    }
    e->have_ic = idahip_snapshot_initial(ctx) == 0;  // for idaens_stream's restarts; costs two batch-sized vectors
    // The device steppers decide step sizes and orders with glibc_pow.hpp, a restatement of ONE libm's pow; the host stepper
    // (and the reference's f64::powf) use this host's std::pow. The two agree bit for bit on the hosts this was built for
    // (tests/test_glibc_pow.py); on another libm they need not, and the two steppers would then take different step
    // sequences without a sign. Checked once per process on the controller's argument ranges: on a mismatch the ensemble
    // stays on the host stepper and says so in its error text.
    // (the verdict is process-wide and guarded: ensembles may be created from several host threads. A self-check that could not
    // RUN -- idahip_pow_batch failed -- is not a verdict: this ensemble stays on the host stepper, says why, and the next
    // idaens_create tries again.)
    static std::mutex g_pow_mu;
    static int g_pow_ok = -1;  // -1: not known yet, 0: bits differ, 1: bit-identical
    bool could_not_run = false;
    int pow_ok;
    {
        std::lock_guard<std::mutex> lk(g_pow_mu);
        if (g_pow_ok < 0) {
            std::vector<double> x, y, r;
            unsigned long long z = 0x9E3779B97F4A7C15ull;
            auto u01 = [&]() { z ^= z << 13; z ^= z >> 7; z ^= z << 17; return (double)(z >> 11) / 9007199254740992.0; };
            for (int i = 0; i < 384; ++i) {
                const int k = 1 + i % 6;
                x.push_back(1.0e-4 + 3.0 * u01());                      // 2 err + 0.0001 (handle_n_flag, complete_step), delnrm / oldnrm (ctest)
                y.push_back((i & 1) ? -1.0 / (double)(k + 1) : 1.0 / (double)k);
            }
            r.resize(x.size());
            if (idahip_pow_batch(ctx, x.data(), y.data(), r.data(), x.size()) != 0) {
                could_not_run = true;
            } else {
                g_pow_ok = 1;
                for (size_t i = 0; i < x.size(); ++i) {
                    const double h = std::pow(x[i], y[i]);
                    if (std::memcmp(&h, &r[i], sizeof h) != 0) g_pow_ok = 0;
                }
            }
        }
        pow_ok = g_pow_ok;
    }
    if (could_not_run) {
        e->device_ctl = false;
        e->pow_mismatch = true;
        e->err = std::string("the device pow self-check could not run (idahip_pow_batch failed: ") + idahip_last_error(ctx) +
                 "): the device steppers are off for this ensemble (host stepper in use)";
    } else if (pow_ok == 0) {
        e->device_ctl = false;
        e->pow_mismatch = true;
        e->err = "the device pow does not reproduce this host's std::pow bit for bit: the device steppers are off (host stepper in use)";
    }
    *out = e;
    return 0;
}

int idaens_destroy(idaens* e) {
    if (g_prof && e) {
        const double tot = prof_now() - g_prof_t0;
        std::fprintf(stderr, "[idaens profile] rounds %lld: in device-library calls %.3f s, host logic + idle %.3f s (since the first create)\n",
                     (long long)e->total_rounds, g_prof_dev, tot - g_prof_dev);
    }
    delete e;
    return 0;
}

const char* idaens_last_error(const idaens* e) { return e ? e->err.c_str() : "null"; }

int idaens_set_max_num_steps(idaens* e, long mxstep) {
    if (!e || mxstep < 0) return -1;
    e->mxstep = mxstep;
    return 0;
}
int idaens_set_device_controller(idaens* e, int on) {
    if (!e) return -1;
    e->device_ctl = on != 0 && !e->pow_mismatch;
    return (on != 0 && e->pow_mismatch) ? 1 : 0;  // 1: refused (see idaens_last_error)
}
int idaens_set_fused_newton(idaens* e, int on) {
    if (!e) return -1;
    e->fused_newton = on != 0 && idahip_kind(e->ctx) != IDAHIP_HOST_CALLBACK && idahip_krylov(e->ctx, nullptr) != 1;
    return 0;
}

int idaens_set_stop_time(idaens* e, const double* hTstop, int ntstop) {
    if (!e) return -1;
    if (hTstop && ntstop != 1 && ntstop != e->batch) return efail(e, -2, "idaens_set_stop_time: ntstop is 1 or batch (%d), not %d", e->batch, ntstop);
    for (int b = 0; b < e->batch; ++b)
        if (e->sys[b].ph != PH_IDLE)
            return efail(e, -2, "idaens_set_stop_time: system %d is inside a round-limited call (IDAENS_UNFINISHED): finish that call first", b);
    for (int b = 0; b < e->batch && hTstop; ++b) {
        const double t = hTstop[ntstop == 1 ? 0 : b];
        const Sys& s = e->sys[b];
        if (t != t) continue;
        if (std::isinf(t)) return efail(e, -2, "idaens_set_stop_time: the stop time of system %d is infinite", b);
        if (s.nst > 0 && (t - s.tn) * s.hh < 0.0)  // IDASetStopTime's check
            return efail(e, -2, "idaens_set_stop_time: the stop time %.17g of system %d is behind its current t = %.17g in the direction of integration",
                         t, b, s.tn);
    }
    for (int b = 0; b < e->batch; ++b) {
        const double t = hTstop ? hTstop[ntstop == 1 ? 0 : b] : std::nan("");
        Sys& s = e->sys[b];
        s.tstopset = t == t;
        s.tstop = s.tstopset ? t : 0.0;
    }
    return 0;
}
int idaens_get_stop_time(const idaens* e, double* hTstop) {
    if (!e || !hTstop) return -1;
    for (int b = 0; b < e->batch; ++b) hTstop[b] = e->sys[b].tstopset ? e->sys[b].tstop : std::nan("");
    return 0;
}

int idaens_set_max_ord(idaens* e, int maxord) {
    if (!e || maxord < 1 || maxord > MAXORD_DEFAULT) return -1;
    e->maxord = maxord;
    return 0;
}

}  // extern "C"

namespace {

// A system's call has just returned (s.status set, phase idle). With IDAENS_SUCCESS and touts left in the schedule it
// enters the next call at once. Returns 1 when the system is stepping again, 0 when it is done for this call, < 0 on a
// device failure.
int continue_schedule(idaens* e, SolveCall& C, int b) {
    Sys& s = e->sys[b];
    for (;;) {
        if (s.status == IDAENS_SUCCESS) C.reached.push_back({b, s.sched_i});
        if (s.status != IDAENS_SUCCESS || s.sched_i + 1 >= C.ntout) return 0;
        s.sched_i += 1;
        s.tout_cur = C.touts[s.sched_i];
        // the next call may interpolate again for this system (tn already past the next tout), or bracket a root through
        // yy/yp: the output of the call that just returned has to be out of the way first
        if (e->nrtfn > 0 || (s.tn - s.tout_cur) * s.hh >= 0.0) {
            const int rc = emit_outputs(e, C);
            if (rc) return rc;
        }
        HostFlow be{e, b, C.sl};
        const int ist = enter_call(s, s.rt, e->nrtfn, C.itask, be);
        if (ist == IDAENS_UNFINISHED) {
            s.ph = PH_LOOP_TOP;
            return 1;
        }
        s.status = ist;
    }
}

// Small systems with a device residual: the whole call runs on the device, one thread per IVP with its own time loop and the
// controller of ida_controller.hpp compiled for the device (idahip_tiny_solve). The host only moves the controller states.
// 1 = one thread per system (idahip_tiny_solve), 2 = lock-step rounds driven from the device (idahip_round_solve), 0 = host stepper
int device_ctl_applies(const idaens* e, const SolveCall& C) {
    const int k = idahip_kind(e->ctx);
    if (!e->device_ctl || C.itask != IDAENS_NORMAL || e->trace_sys >= 0) return 0;
    // a Krylov ctx steps on the host unless idahip_set_krylov_rounds is on (read anew by every solve call)
    const bool kry = idahip_krylov(e->ctx, nullptr) == 1;
    if (kry && idahip_krylov_rounds(e->ctx) != 1) return 0;
    // root finding on the device: the function family of idaens_set_roots (not a user callback), not in idaens_stream
    if (e->nrtfn != 0 && (e->rt_fn != nullptr || e->nrtfn > IDAHIP_MAX_ROOTS || C.recycle)) return 0;
    if (kry)  // (constraints are refused on a Krylov ctx; no LU: the variant does not matter)
        return (e->n > 8 && e->n <= 4096 && (k == IDAHIP_LINEAR_DENSE || k == IDAHIP_HEAT1D || k == IDAHIP_BRUSS1D)) ? 2 : 0;
    if (e->n <= 8 && (k == IDAHIP_ROBERTS || k == IDAHIP_LORENZ63)) return 1;
    // a reaction network of that size runs there when its ctx opted in (idahip_set_mass_action_tiny, read anew by every solve call)
    if (e->n <= 8 && k == IDAHIP_MASS_ACTION && idahip_mass_action_tiny(e->ctx) == 1) return 1;
    if (idahip_constraints(e->ctx, nullptr) == 1) return 0;  // the lock-step device rounds have no constraint check
    if (e->n > 8 && e->n <= 4096 && (k == IDAHIP_LINEAR_DENSE || k == IDAHIP_HEAT1D || k == IDAHIP_BRUSS1D || k == IDAHIP_MASS_ACTION) && idahip_lu_variant(e->ctx) >= 4) return 2;
    return 0;
}

int solve_core_device(idaens* e, SolveCall& C, double* hTret, int32_t* hStatus, long max_rounds, int mode) {
    std::vector<Sys>& S = e->sys;
    const int batch = e->batch;
    const size_t n = e->n;
    const bool resume = C.ntout > 1 && e->sched_unfinished;
    auto reached_of = [&](const Sys& s) { return s.sched_i + ((s.ph == PH_IDLE && s.status == IDAENS_SUCCESS) ? 1 : 0); };
    std::vector<SysCore> st(batch);
    std::vector<int> prev(batch, 0);
    for (int b = 0; b < batch; ++b) {
        st[b] = S[b];
        if (resume) prev[b] = reached_of(S[b]);
    }
    idahip_tiny_call call;
    call.touts = C.touts;
    call.ntout = C.ntout;
    call.recycle = C.recycle ? 1 : 0;
    call.resume = resume ? 1 : 0;
    call.max_rounds = max_rounds;
    call.mxstep = e->mxstep;
    call.maxord = e->maxord;
    call.maxnef = e->maxnef;
    call.maxncf = e->maxncf;
    call.epcon = e->epcon;
    call.hmax_inv = e->hmax_inv;
    call.t0 = e->t0;
    call.start_round = (C.recycle && !e->start_round.empty()) ? e->start_round.data() : nullptr;
    call.round_base = e->total_rounds;
    // the systems' root state (Ida's ida_glo / ghi / grout / iroots / gactive) goes with the controller records
    std::vector<idahip_root_state> rstate;
    std::vector<int32_t> rcomp(e->rt_comp.begin(), e->rt_comp.end());
    call.nroots = e->nrtfn;
    call.root_comps = rcomp.data();
    call.root_thresholds = e->rt_thr.data();
    call.root_states = nullptr;
    if (e->nrtfn > 0) {
        rstate.resize(batch);
        for (int b = 0; b < batch; ++b) copy_roots(rstate[b], S[b].rt, e->nrtfn);
        call.root_states = rstate.data();
    }
    std::vector<int64_t> rounds(batch, 0);
    uint64_t acc[2] = {0, 0};
    std::vector<double> yo, ypo;
    if (C.hYout) yo.resize((size_t)C.ntout * batch * n);
    if (C.hYPout) ypo.resize((size_t)C.ntout * batch * n);
    int64_t rounds_run = -1;
    // a Krylov ctx's npe / nps are not in the record (Sys above): they go to the ctx and come back from it around the call
    const bool kry = mode == 2 && idahip_krylov(e->ctx, nullptr) == 1;
    std::vector<int64_t> npe, nps;
    if (kry) {
        npe.resize(batch);
        nps.resize(batch);
        for (int b = 0; b < batch; ++b) { npe[b] = S[b].npe; nps[b] = S[b].nps; }
        ENS_CALL(e, idahip_krylov_rounds_put_counters(e->ctx, npe.data(), nps.data()));
    }
    if (mode == 1)
        ENS_CALL(e, idahip_tiny_solve(e->ctx, st.data(), sizeof(SysCore), &call, rounds.data(), acc, C.hYout ? yo.data() : nullptr,
                                      C.hYPout ? ypo.data() : nullptr));
    else
        ENS_CALL(e, idahip_round_solve(e->ctx, st.data(), sizeof(SysCore), &call, rounds.data(), acc, C.hYout ? yo.data() : nullptr,
                                       C.hYPout ? ypo.data() : nullptr, &rounds_run));
    if (kry) {
        ENS_CALL(e, idahip_krylov_rounds_get_counters(e->ctx, npe.data(), nps.data()));
        for (int b = 0; b < batch; ++b) { S[b].npe = (long)npe[b]; S[b].nps = (long)nps[b]; }
    }
    int64_t rmax = 0;
    bool unfinished = false;
    for (int b = 0; b < batch; ++b) {
        static_cast<SysCore&>(S[b]) = st[b];
        if (e->nrtfn > 0) copy_roots(S[b].rt, rstate[b], e->nrtfn);
        rmax = std::max(rmax, rounds[b]);
        Sys& s = S[b];
        const int now = reached_of(s);
        for (int i = prev[b]; i < now; ++i) {  // the outputs of the touts reached in this call
            const size_t off = ((size_t)i * batch + b) * n;
            if (C.hYout) std::memcpy(C.hYout + off, yo.data() + off, sizeof(double) * n);
            if (C.hYPout) std::memcpy(C.hYPout + off, ypo.data() + off, sizeof(double) * n);
        }
        if (C.hReached) C.hReached[b] = now;
        if (s.ph != PH_IDLE) {
            hStatus[b] = IDAENS_UNFINISHED;
            hTret[b] = s.tn;
            unfinished = true;
        } else {
            hStatus[b] = s.status;
            hTret[b] = s.tret;
            s.returned = true;
        }
    }
    e->total_rounds += rounds_run >= 0 ? rounds_run : rmax;
    e->retired_iters += (int64_t)acc[0];
    e->passes += (int64_t)acc[1];
    e->sched_unfinished = C.ntout > 1 && unfinished;
    return 0;
}

// Whether the ctx has constraints, read anew by every solve / solve_schedule / stream call (C IDA lets a user change them between
// calls). With difference-quotient Jacobians they are refused: C IDA flips the increments' signs there.
int read_constraints(idaens* e) {
    e->constr = idahip_constraints(e->ctx, nullptr) == 1;
    if (e->constr && idahip_jacobian_dq(e->ctx) > 0)
        return efail(e, -2, "constraints on a ctx with difference-quotient Jacobians are not supported");
    return 0;
}

// The masked error norms (idahip_set_suppress_alg) need the id vector: C IDA's IDA_MISSING_ID. Read by every solve call, as the
// constraints are.
int check_suppress_alg(idaens* e) {
    if (idahip_suppress_alg(e->ctx) == 1 && idahip_id(e->ctx, nullptr) != 1)
        return efail(e, -2, "suppress_alg is on and the ctx has no id vector (idahip_set_id)");
    return 0;
}

int solve_core(idaens* e, SolveCall& C, double* hTret, int32_t* hStatus, long max_rounds) {
    if (const int rcc = read_constraints(e)) return rcc;
    if (const int rcm = check_suppress_alg(e)) return rcm;
    e->started = true;
    if (const int mode = device_ctl_applies(e, C)) return solve_core_device(e, C, hTret, hStatus, max_rounds, mode);
    std::vector<Sys>& S = e->sys;
    SolList& sl = C.sl;
    const double tout = C.touts[0];  // the first call's tout sizes the initial step (impl_solve.rs:104-131)
    std::vector<int32_t> act;
    const bool resume = C.ntout > 1 && e->sched_unfinished;  // continuing a round-limited schedule call

    // (re)enter the schedule with the idle systems `cand`: first-call block for those that have not started, then the
    // entry of their first Ida::solve call; whoever has to step is appended to `act`
    auto start_systems = [&](const std::vector<int32_t>& cand) -> int {
    // ---- first-call block for systems that have not started (impl_solve.rs:84-173)
        {
            std::vector<int32_t> fresh;
            for (int b : cand)
                if (S[b].ph == PH_IDLE && S[b].nst == 0 && !S[b].setup_done && !S[b].dead) fresh.push_back(b);
            if (!fresh.empty()) {
                // initial_setup's ewt_set(phi[0]) (lib.rs:537-545), ||phi[1]|| for the h0 heuristic (impl_solve.rs:122-126)
                // and ||phi[0]|| for the first tolsf test (impl_solve.rs:289-295)
                std::vector<double> ypnorm(fresh.size()), p0nrm(fresh.size());
                ENS_CALL(e, idahip_init_first(e->ctx, ypnorm.data(), p0nrm.data(), fresh.data(), (int)fresh.size()));
                std::vector<int32_t> viol;
                if (e->constr) {  // y0 must satisfy the constraints
                    viol.resize(fresh.size());
                    ENS_CALL(e, idahip_constr_check(e->ctx, IDAHIP_F_PHI0, viol.data(), fresh.data(), (int)fresh.size()));
                }
                std::vector<int32_t> ok;
                std::vector<double> fac;
                for (size_t q = 0; q < fresh.size(); ++q) {
                    Sys& s = S[fresh[q]];
                    if (!first_call_scalars(s, tout, ypnorm[q], p0nrm[q], e->epcon, e->hmax_inv, e->constr && viol[q])) continue;  // ILL_INPUT
                    ok.push_back(fresh[q]);
                    fac.push_back(s.hh);
                }
                if (e->nrtfn > 0)
                    for (size_t q = 0; q < ok.size();) {  // impl_solve.rs:157-159
                        HostFlow be{e, ok[q], sl};
                        const int rc1 = r_check1(S[ok[q]], S[ok[q]].rt, e->nrtfn, be);
                        if (rc1 == IDAENS_RTFUNC_FAIL) {  // the user's root function failed for this system: it never starts
                            S[ok[q]].status = rc1;
                            S[ok[q]].tret = S[ok[q]].tn;
                            S[ok[q]].dead = true;
                            ok.erase(ok.begin() + q);
                            fac.erase(fac.begin() + q);
                            continue;
                        }
                        if (rc1) return rc1;
                        ++q;
                    }
                if (!ok.empty()) ENS_CALL(e, idahip_scale_phi1(e->ctx, fac.data(), ok.data(), (int)ok.size()));  // phi[1] = hh*y'
            }
        }

        // ---- per-system entry: stop tests for started systems, then collect who steps (impl_solve.rs:179-241)
        for (int b : cand) {
            Sys& s = S[b];
            if (s.dead || !s.setup_done) continue;  // earlier fatal error / ILL_INPUT at the first call: status is sticky
            s.sched_i = 0;
            s.tout_cur = C.touts[0];
            HostFlow be{e, b, C.sl};
            const int ist = enter_call(s, s.rt, e->nrtfn, C.itask, be);
            if (ist == IDAENS_UNFINISHED) {
                s.ph = PH_LOOP_TOP;
                act.push_back(b);
                continue;
            }
            s.status = ist;
            const int cs = continue_schedule(e, C, b);
            if (cs < 0) return cs;
            if (cs == 1) act.push_back(b);
        }
        return 0;
    };
    {
        std::vector<int32_t> cand;
        for (int b = 0; b < e->batch; ++b) {
            if (S[b].ph != PH_IDLE) act.push_back(b);  // left mid-flight by a round limit: resume
            else if (C.recycle && !e->start_round.empty() && e->start_round[b] > e->total_rounds) continue;  // staggered start
            else if (!resume) cand.push_back(b);       // (resume: idle systems finished in an earlier slice of the call)
        }
        const int rc0 = start_systems(cand);
        if (rc0) return rc0;
    }

    // ---- main loop
    long rounds = 0;
    while (!act.empty()) {
        if (max_rounds > 0 && rounds >= max_rounds) break;
        // loop-top checks for systems starting a new step (impl_solve.rs:246-297)
        std::vector<int32_t> go;
        for (int b : act) {
            Sys& s = S[b];
            if (s.ph == PH_LOOP_TOP) {
                HostFlow be{e, b, sl};
                if (!loop_top(s, e->mxstep, be)) continue;
            }
            go.push_back(b);
        }
        act.swap(go);
        if (act.empty()) break;
        int rc = attempt_round(e, act, C);
        if (rc) return rc;
        rounds += 1;
        e->total_rounds += 1;
        if (C.ntout > 1 || C.recycle) {  // outputs of the touts reached in this round, before the next round steps on
            rc = emit_outputs(e, C);
            if (rc) return rc;
        }
        if (C.recycle) {  // Ida::new again for the systems that finished their schedule in this round
            std::vector<int32_t> again;
            for (int b = 0; b < e->batch; ++b) {
                Sys& s = S[b];
                if (stream_restart_due(s, C.ntout)) {
                    e->retired_iters += s.niters;
                    e->passes += 1;
                    s = Sys();
                    s.tn = e->t0;
                    again.push_back(b);
                }
            }
            if (!again.empty()) {
                ENS_CALL(e, idahip_restore_initial(e->ctx, again.data(), (int)again.size()));
                rc = start_systems(again);
                if (rc) return rc;
            }
            if (!e->start_round.empty()) {  // staggered start: the systems whose turn it is now
                std::vector<int32_t> late;
                for (int b = 0; b < e->batch; ++b)
                    if (e->start_round[b] == e->total_rounds && S[b].ph == PH_IDLE && S[b].nst == 0 && !S[b].setup_done) late.push_back(b);
                if (!late.empty()) {
                    rc = start_systems(late);
                    if (rc) return rc;
                }
            }
        }
    }
    int rc = emit_outputs(e, C);
    if (rc) return rc;
    bool unfinished = false;
    for (int b = 0; b < e->batch; ++b) {
        Sys& s = S[b];
        if (C.hReached) C.hReached[b] = s.sched_i + ((s.ph == PH_IDLE && s.status == IDAENS_SUCCESS) ? 1 : 0);
        if (s.ph != PH_IDLE) {
            hStatus[b] = IDAENS_UNFINISHED;
            hTret[b] = s.tn;
            unfinished = true;
        } else {
            hStatus[b] = s.status;
            hTret[b] = s.tret;
            s.returned = true;
        }
    }
    e->sched_unfinished = C.ntout > 1 && unfinished;
    return 0;
}

}  // namespace

extern "C" {

int idaens_device_controller_active(const idaens* e) {
    if (!e) return -1;
    SolveCall C;
    C.itask = IDAENS_NORMAL;
    return device_ctl_applies(e, C);
}

int idaens_solve(idaens* e, double tout, int itask, double* hTret, int32_t* hStatus, long max_rounds) {
    if (!e || !hTret || !hStatus) return -1;
    SolveCall C;
    C.touts = &tout;
    C.ntout = 1;
    C.itask = itask;
    return solve_core(e, C, hTret, hStatus, max_rounds);
}

int idaens_stream(idaens* e, const double* touts, int ntout, long max_rounds, long stagger_rounds, int64_t* passes_done) {
    if (!e || !touts || ntout < 1 || max_rounds < 1 || stagger_rounds < 0) return -1;
    if (const int rcc = read_constraints(e)) return rcc;
    if (!e->streaming && stagger_rounds > 0) {  // first call: system b enters at round b * stagger / batch
        e->start_round.resize(e->batch);
        for (int b = 0; b < e->batch; ++b) e->start_round[b] = e->total_rounds + (int64_t)b * stagger_rounds / e->batch;
    }
    if (e->nrtfn > 0) return efail(e, -2, "idaens_stream does not combine with root finding");
    for (int b = 0; b < e->batch; ++b)
        if (e->sys[b].tstopset)
            return efail(e, -2, "idaens_stream does not combine with a stop time (system %d has one): a restarted system is Ida::new, which has none", b);
    for (int b = 0; b < e->batch; ++b)
        if (std::memcmp(&e->sys[b].t_start, &e->t0, sizeof(double)) != 0)
            return efail(e, -2, "idaens_stream does not combine with a start time of a system's own (system %d was reinitialised at t0 = %.17g): a restarted system starts at %.17g",
                         b, e->sys[b].t_start, e->t0);
    if (!e->have_ic) return efail(e, -2, "no snapshot of the initial conditions (idaens_create failed to take it)");
    SolveCall C;
    C.touts = touts;
    C.ntout = ntout;
    C.itask = IDAENS_NORMAL;
    C.recycle = true;
    std::vector<double> tret(e->batch);
    std::vector<int32_t> status(e->batch);
    e->sched_unfinished = e->total_rounds > 0 && e->streaming;  // later slices continue the systems in flight
    e->streaming = true;
    const int rc = solve_core(e, C, tret.data(), status.data(), max_rounds);
    if (passes_done) *passes_done = e->passes;
    for (int b = 0; b < e->batch; ++b)
        if (status[b] < 0) return efail(e, -5, "system %d failed with status %d while streaming", b, status[b]);
    return rc;
}

int idaens_solve_schedule(idaens* e, const double* touts, int ntout, double* hTret, int32_t* hStatus, int32_t* hReached,
                          double* hYout, double* hYPout, long max_rounds) {
    if (!e || !touts || ntout < 1 || !hTret || !hStatus) return -1;
    SolveCall C;
    C.touts = touts;
    C.ntout = ntout;
    C.itask = IDAENS_NORMAL;
    C.hReached = hReached;
    C.hYout = hYout;
    C.hYPout = hYPout;
    return solve_core(e, C, hTret, hStatus, max_rounds);
}

}  // extern "C"

// ---------------------------------------------------------------- consistent initial conditions (IDACalcIC)
namespace {

namespace ic {
constexpr double EPS_NEWT = 0.01 * 0.33;
constexpr int MAXNH = 5, MAXNJ = 4, MAXNIT = 10, MAXBACKS = 100;
constexpr double ALPHALS = 1e-4, ICRATEMAX = 0.9;
enum Ret { OK = 0, FAIL_RECOV, LINESRCH, CONV, SLOW };
enum Stage { ST_RES = 0, ST_SETUP, ST_SOLVE, ST_TRIAL, ST_DONE };

// the scalar state of one system's IDACalcIC: idaNlsIC / idaNewtonIC / idaLineSrch as a resumable machine
struct State {
    int stage = ST_DONE, status = 0;
    double hic = 0.0, cj = 0.0;
    int nwt = 1, nh = 1, nj = 1, mxnh = 1;
    double fnorm = 0.0, fnorm0 = 0.0, oldfnrm = 0.0, rate = 0.0;
    int m = 0;
    double f1norm = 0.0, slpi = 0.0, minlam = 0.0, lambda = 1.0;
    int nbacks = 0;
};
}  // namespace ic

// cand: the systems to correct, none of which has taken a step; hTout1 / hStatus go by position in cand. whole: cand is the whole
// batch (idaens_calc_ic), and the call ends with the batch-wide snapshot and zero upload; otherwise both act on cand's systems only.
int calc_ic(idaens* e, int icopt, const std::vector<int32_t>& cand, const double* hTout1, int32_t* hStatus, bool whole) {
    using namespace ic;
    std::vector<Sys>& S = e->sys;
    const int batch = e->batch;
    const double eps = F64_EPS;
    const double steptol = std::pow(eps, 2.0 / 3.0);
    const bool dq = idahip_jacobian_dq(e->ctx) > 0;
    const long dq_evals = dq ? (idahip_band(e->ctx, nullptr, nullptr) > 0 ? dq_band_evals(e) : (long)e->n) : 0;
    std::vector<State> T(batch);
    std::vector<int32_t> L, acc, com, rst;
    std::vector<double> tn, cj, hh, lam, nrm;
    std::vector<int32_t> info;

    // ---- setup (steps 1-8). The distance test is made first, on the host: a call that can do nothing launches nothing
    std::vector<double> tout1_of(batch, 0.0);
    for (size_t q = 0; q < cand.size(); ++q) tout1_of[cand[q]] = hTout1[q];
    for (int b : cand) {
        const double t0 = S[b].tn;
        const double tout1 = tout1_of[b];
        const double tdist = std::fabs(tout1 - t0);
        // tdist == 0.0 is named on its own, as in the stepper's first call: with t0 == tout1 == 0 the bound is 0 too, and 0 < 0 is false
        if (tdist == 0.0 || tdist < 2.0 * eps * (std::fabs(t0) + std::fabs(tout1))) T[b].status = IDAENS_ILL_INPUT;
        else L.push_back(b);
    }
    if (!L.empty()) {
        nrm.assign(L.size(), 0.0);
        info.assign(L.size(), 0);
        ENS_CALL(e, idahip_ic_begin(e->ctx, nrm.data(), info.data(), L.data(), (int)L.size()));
        for (size_t q = 0; q < L.size(); ++q) {
            const int b = L[q];
            State& t = T[b];
            if (info[q] != 0) {
                t.status = IDAENS_BAD_EWT;
                continue;
            }
            const double t0 = S[b].tn;
            const double tout1 = tout1_of[b];
            t.hic = 0.001 * std::fabs(tout1 - t0);
            if (nrm[q] > 0.5 / t.hic) t.hic = 0.5 / nrm[q];
            if (tout1 < t0) t.hic = -t.hic;
            if (icopt == IDAENS_YA_YDP_INIT) {
                t.cj = 1.0 / t.hic;
                t.mxnh = MAXNH;
            } else {
                t.cj = 0.0;
                t.mxnh = 1;
            }
            t.stage = ST_RES;
        }
    }

    auto gather = [&](int stage) {
        L.clear(); tn.clear(); cj.clear();
        for (int b = 0; b < batch; ++b)
            if (T[b].stage == stage) {
                L.push_back(b);
                tn.push_back(S[b].tn);
                cj.push_back(T[b].cj);
            }
        return !L.empty();
    };
    // idaLineSrch's first lines, at the start of every Newton iteration
    auto begin_linesearch = [&](int b) {
        State& t = T[b];
        S[b].niters += 1;
        t.f1norm = t.fnorm * t.fnorm * 0.5;
        t.slpi = -2.0 * t.f1norm;
        t.minlam = steptol / t.fnorm;
        t.lambda = 1.0;
        t.nbacks = 0;
        t.stage = ST_TRIAL;
    };
    // idaNlsIC returned `ret` for this step size: the outer loops of IDACalcIC
    auto nls_returned = [&](int b, int ret) {
        State& t = T[b];
        if (ret == OK) {
            com.push_back(b);  // ewt, phi; the pass counter moves on once the weights are known to be good
            t.stage = ST_DONE;
            return;
        }
        S[b].ncfn += 1;
        if (t.nh == t.mxnh) {
            t.status = ret == FAIL_RECOV ? IDAENS_NO_RECOVERY : ret == LINESRCH ? IDAENS_LINESEARCH_FAIL : IDAENS_CONV_FAIL;
            t.stage = ST_DONE;
            return;
        }
        if (ret != SLOW) rst.push_back(b);
        t.hic *= 0.1;
        t.cj = 1.0 / t.hic;
        t.nh += 1;
        t.stage = ST_RES;
    };
    // idaNewtonIC returned `ret`: idaNlsIC's loop over Jacobian evaluations
    auto newton_returned = [&](int b, int ret) {
        State& t = T[b];
        if (ret == SLOW && t.nj < MAXNJ) {
            t.nj += 1;
            t.stage = ST_SETUP;  // (delta = savres: idahip_ic_setup)
            return;
        }
        nls_returned(b, ret);
    };
    // the Newton loop was left with `ret` (a failed line search, or maxnit iterations)
    auto newton_left = [&](int b, int ret) {
        State& t = T[b];
        if (t.rate <= ICRATEMAX) return newton_returned(b, ret);
        if (t.fnorm < 0.1 * t.fnorm0) return newton_returned(b, SLOW);
        return newton_returned(b, ret);
    };

    // ---- lock-step rounds: every system sits in one stage; a round issues one batched call per non-empty stage
    for (;;) {
        bool any = false;
        for (int b = 0; b < batch; ++b) any = any || T[b].stage != ST_DONE;
        if (!any) break;
        acc.clear(); com.clear(); rst.clear();
        if (gather(ST_RES)) {  // delta = savres = F(t0, yy0, yp0)
            ENS_CALL(e, idahip_ic_res(e->ctx, tn.data(), cj.data(), L.data(), (int)L.size()));
            for (int b : L) {
                S[b].nre += 1;
                T[b].nj = 1;
                T[b].stage = ST_SETUP;
            }
        }
        if (gather(ST_SETUP)) {  // J = dF/dy + cj dF/dy' at the iterate, factored
            info.assign(L.size(), 0);
            if (dq) {
                hh.clear();
                for (int b : L) hh.push_back(T[b].hic);
                ENS_CALL(e, idahip_ic_setup_dq(e->ctx, tn.data(), cj.data(), hh.data(), info.data(), L.data(), (int)L.size()));
            } else {
                ENS_CALL(e, idahip_ic_setup(e->ctx, tn.data(), cj.data(), info.data(), L.data(), (int)L.size()));
            }
            for (size_t q = 0; q < L.size(); ++q) {
                const int b = L[q];
                S[b].nsetups += 1;
                S[b].nje += 1;
                S[b].nre_dq += dq_evals;
                if (info[q] != 0) nls_returned(b, FAIL_RECOV);
                else T[b].stage = ST_SOLVE;
            }
        }
        if (gather(ST_SOLVE)) {  // delta = J^-1 delta; fnorm
            nrm.assign(L.size(), 0.0);
            ENS_CALL(e, idahip_ic_solve(e->ctx, nrm.data(), L.data(), (int)L.size()));
            for (size_t q = 0; q < L.size(); ++q) {
                const int b = L[q];
                State& t = T[b];
                t.fnorm = nrm[q];
                if (t.fnorm <= EPS_NEWT) {
                    newton_returned(b, OK);
                    continue;
                }
                t.fnorm0 = t.oldfnrm = t.fnorm;
                t.rate = 0.0;
                t.m = 0;
                begin_linesearch(b);
            }
        }
        if (gather(ST_TRIAL)) {  // savres = F(trial point); delnew = J^-1 savres; fnormp
            lam.clear();
            for (int b : L) lam.push_back(T[b].lambda);
            nrm.assign(L.size(), 0.0);
            ENS_CALL(e, idahip_ic_trial(e->ctx, icopt, tn.data(), cj.data(), lam.data(), nrm.data(), L.data(), (int)L.size()));
            for (size_t q = 0; q < L.size(); ++q) {
                const int b = L[q];
                State& t = T[b];
                const double fnormp = nrm[q];
                S[b].nre += 1;
                if (fnormp * fnormp * 0.5 <= t.f1norm + ALPHALS * t.slpi * t.lambda) {
                    acc.push_back(b);  // yy0 (yp0) = the trial point; delta = delnew
                    t.fnorm = fnormp;
                    t.rate = t.fnorm / t.oldfnrm;
                    if (t.fnorm <= EPS_NEWT) {
                        newton_returned(b, OK);
                        continue;
                    }
                    t.m += 1;
                    if (t.m >= MAXNIT) {
                        newton_left(b, CONV);
                        continue;
                    }
                    t.oldfnrm = t.fnorm;
                    begin_linesearch(b);
                    continue;
                }
                if (t.lambda < t.minlam) {
                    newton_left(b, LINESRCH);
                    continue;
                }
                t.lambda /= 2.0;
                S[b].nbacktr += 1;
                t.nbacks += 1;
                if (t.nbacks == MAXBACKS) newton_left(b, LINESRCH);
            }
        }
        if (!acc.empty()) ENS_CALL(e, idahip_ic_accept(e->ctx, icopt, acc.data(), (int)acc.size()));
        if (!rst.empty()) ENS_CALL(e, idahip_ic_reset(e->ctx, rst.data(), (int)rst.size()));
        if (!com.empty()) {  // a pass has converged: ewt = ewt_set(yy0); phi[0] = yy0; phi[1] = yp0; then the second pass
            info.assign(com.size(), 0);
            ENS_CALL(e, idahip_ic_commit(e->ctx, info.data(), com.data(), (int)com.size()));
            for (size_t q = 0; q < com.size(); ++q) {
                State& t = T[com[q]];
                if (info[q] != 0) {
                    t.status = IDAENS_BAD_EWT;
                } else if (t.nwt < 2) {
                    t.nwt += 1;
                    t.nh = 1;
                    t.stage = ST_RES;
                }
            }
        }
    }

    // ---- a failed system keeps what it was created with; the restarts of idaens_stream begin from the corrected values
    L.clear();
    std::vector<int32_t> ran;
    for (size_t q = 0; q < cand.size(); ++q) {
        const int b = cand[q];
        hStatus[q] = T[b].status;
        if (T[b].status != 0 && T[b].status != IDAENS_ILL_INPUT) L.push_back(b);
        if (T[b].status != IDAENS_ILL_INPUT) ran.push_back(b);
    }
    if (!L.empty()) ENS_CALL(e, idahip_restore_initial(e->ctx, L.data(), (int)L.size()));
    if (!ran.empty() && whole) {
        ENS_CALL(e, idahip_snapshot_initial(e->ctx));
        const std::vector<double> zero((size_t)batch * e->n, 0.0);  // phi[2..4] held the iterate and delnew
        for (int j = 2; j <= 4; ++j) ENS_CALL(e, idahip_upload(e->ctx, (idahip_field)(IDAHIP_F_PHI0 + j), 0, batch, zero.data()));
    } else if (!ran.empty()) {
        // the same two actions for these systems alone: their yy / yp equal phi[0] / phi[1] here (idahip_ic_commit and
        // idahip_restore_initial write both), so a reinit "at the current values" renews their snapshot rows and zeroes phi[2..5]
        ENS_CALL(e, idahip_reinit(e->ctx, ran.data(), (int)ran.size(), nullptr, nullptr, 1));
    }
    return 0;
}

// the refusals idaens_calc_ic and idaens_calc_ic_systems share, after the argument checks of each
int calc_ic_refusals(idaens* e, const char* who) {
    if (idahip_constraints(e->ctx, nullptr) == 1) return efail(e, -2, "%s: a ctx with constraints is not supported (idahip_set_constraints)", who);
    if (idahip_krylov(e->ctx, nullptr) == 1) return efail(e, -2, "%s: a Krylov ctx is not supported (idahip_create_krylov)", who);
    if (idahip_suppress_alg(e->ctx) == 1)
        return efail(e, -2, "%s: not with suppress_alg on (set_id, calc_ic, idahip_set_suppress_alg(1), solve is the supported order)", who);
    if (!e->have_ic) return efail(e, -2, "no snapshot of the initial conditions (idaens_create failed to take it)");
    return 0;
}

// IDAReInit for the listed systems: hT0 by list position; hYY0 / hYP0 / add as idahip_reinit takes them
int reinit_systems(idaens* e, const char* who, const int32_t* hIdx, int nsys, const double* hT0, const double* hYY0, const double* hYP0,
                   int add) {
    for (int q = 0; q < nsys; ++q) {
        const int b = hIdx[q];
        if (b < 0 || b >= e->batch) return efail(e, -2, "%s: system id %d out of range at list position %d", who, b, q);
        if (e->sys[b].ph != PH_IDLE)
            return efail(e, -2, "%s: system %d is inside a round-limited call (IDAENS_UNFINISHED): finish that call first", who, b);
        if (!std::isfinite(hT0[q])) return efail(e, -2, "%s: the t0 of system %d is not finite", who, b);
    }
    ENS_CALL(e, idahip_reinit(e->ctx, hIdx, nsys, hYY0, hYP0, add));  // (a list with one id twice is refused here: nothing has changed yet)
    for (int q = 0; q < nsys; ++q) {
        Sys& s = e->sys[hIdx[q]];
        e->retired_iters += s.niters;  // idaens_total_newton_iters is a total since creation
        s = Sys();
        s.tn = s.t_start = hT0[q];
        s.rt.glo.assign(e->nrtfn, 0.0);  // the root state as install_roots leaves it
        s.rt.ghi.assign(e->nrtfn, 0.0);
        s.rt.grout.assign(e->nrtfn, 0.0);
        s.rt.iroots.assign(e->nrtfn, 0.0);
        s.rt.gactive.assign(e->nrtfn, 0);
    }
    return 0;
}

}  // namespace

extern "C" int idaens_calc_ic(idaens* e, int icopt, double tout1, int32_t* hStatus) {
    if (!e || !hStatus) return -1;
    if (icopt != IDAENS_YA_YDP_INIT && icopt != IDAENS_Y_INIT) return efail(e, -2, "idaens_calc_ic: unknown icopt %d", icopt);
    if (icopt == IDAENS_YA_YDP_INIT && idahip_id(e->ctx, nullptr) != 1)
        return efail(e, -2, "idaens_calc_ic: IDAENS_YA_YDP_INIT needs the id vector (idahip_set_id)");
    if (e->started) return efail(e, -2, "idaens_calc_ic: only before the first solve, solve_schedule or stream call");
    if (const int rc = calc_ic_refusals(e, "idaens_calc_ic")) return rc;
    std::vector<int32_t> all(e->batch);
    for (int b = 0; b < e->batch; ++b) all[b] = b;
    const std::vector<double> touts((size_t)e->batch, tout1);
    return calc_ic(e, icopt, all, touts.data(), hStatus, true);
}

extern "C" int idaens_calc_ic_systems(idaens* e, int icopt, const int32_t* hIdx, int nsys, const double* hTout1, int32_t* hStatus) {
    if (!e || nsys < 0 || (nsys > 0 && (!hIdx || !hTout1 || !hStatus))) return -1;
    if (icopt != IDAENS_YA_YDP_INIT && icopt != IDAENS_Y_INIT) return efail(e, -2, "idaens_calc_ic_systems: unknown icopt %d", icopt);
    if (icopt == IDAENS_YA_YDP_INIT && idahip_id(e->ctx, nullptr) != 1)
        return efail(e, -2, "idaens_calc_ic_systems: IDAENS_YA_YDP_INIT needs the id vector (idahip_set_id)");
    if (const int rc = calc_ic_refusals(e, "idaens_calc_ic_systems")) return rc;
    std::vector<uint8_t> seen((size_t)e->batch, 0);
    for (int q = 0; q < nsys; ++q) {
        const int b = hIdx[q];
        if (b < 0 || b >= e->batch) return efail(e, -2, "idaens_calc_ic_systems: system id %d out of range at list position %d", b, q);
        if (seen[b]) return efail(e, -2, "idaens_calc_ic_systems: system id %d listed twice (again at list position %d)", b, q);
        seen[b] = 1;
        const Sys& s = e->sys[b];
        if (s.ph != PH_IDLE || s.nst > 0 || s.setup_done || s.dead)
            return efail(e, -2, "idaens_calc_ic_systems: system %d has started: only systems that have not taken a step since idaens_create or idaens_reinit", b);
    }
    if (nsys == 0) return 0;
    return calc_ic(e, icopt, std::vector<int32_t>(hIdx, hIdx + nsys), hTout1, hStatus, false);
}

extern "C" int idaens_reinit(idaens* e, const int32_t* hIdx, int nsys, const double* hT0, const double* hYY0, const double* hYP0) {
    if (!e || nsys < 0 || (nsys > 0 && (!hIdx || !hT0 || !hYY0 || !hYP0))) return -1;
    return reinit_systems(e, "idaens_reinit", hIdx, nsys, hT0, hYY0, hYP0, 0);
}

extern "C" int idaens_reinit_at_return(idaens* e, const int32_t* hIdx, int nsys, const double* hDY, const double* hDYP) {
    if (!e || nsys < 0 || (nsys > 0 && !hIdx)) return -1;
    std::vector<double> t0((size_t)nsys, 0.0);
    for (int q = 0; q < nsys; ++q) {
        const int b = hIdx[q];
        if (b < 0 || b >= e->batch) return efail(e, -2, "idaens_reinit_at_return: system id %d out of range at list position %d", b, q);
        const Sys& s = e->sys[b];
        if (s.ph == PH_IDLE && !s.returned)
            return efail(e, -2, "idaens_reinit_at_return: system %d has not returned from a solve call since it was created or reinitialised", b);
        t0[q] = s.tret;
    }
    return reinit_systems(e, "idaens_reinit_at_return", hIdx, nsys, t0.data(), hDY, hDYP, 1);
}

extern "C" {

// ---- several ensembles side by side on one device (include/ida_ensemble.h): one host thread per ensemble, each on its own
// context and HIP stream. The ensembles share nothing; what they gain is the device's own scheduling -- while one group's
// round is in a part that leaves most of the chip idle (the serial chain of the panel kernels, the later Newton passes and
// their residuals for a few hundred systems, round begin / end), the other groups' launches fill it.
namespace {
int check_group(idaens* const* ens, int ngroups) {
    if (!ens || ngroups < 1) return -1;
    for (int g = 0; g < ngroups; ++g)
        if (!ens[g]) return -1;
    for (int g = 0; g < ngroups; ++g)
        for (int h = g + 1; h < ngroups; ++h)
            if (ens[g] == ens[h] || ens[g]->ctx == ens[h]->ctx)
                return efail(ens[0], -2, "the ensembles of a group need a context (and HIP stream) each: groups %d and %d share one", g, h);
    return 0;
}
int run_group(int ngroups, long offset_us, const std::function<int(int)>& one) {
    std::vector<int> rc(ngroups, 0);
    std::vector<std::thread> th;
    th.reserve(ngroups > 0 ? ngroups - 1 : 0);
    for (int g = 1; g < ngroups; ++g)
        th.emplace_back([&, g]() {
            if (offset_us > 0) std::this_thread::sleep_for(std::chrono::microseconds((long long)g * offset_us));
            rc[g] = one(g);
        });
    rc[0] = one(0);  // group 0 on the calling thread
    for (auto& t : th) t.join();
    int worst = 0;
    for (int g = 0; g < ngroups; ++g)
        if (rc[g] < worst || (worst == 0 && rc[g] != 0)) worst = rc[g];
    return worst;
}
}  // namespace

int idaens_stream_group(idaens* const* ens, int ngroups, const double* touts, int ntout, long max_rounds, long stagger_rounds, long offset_us,
                        int64_t* passes_done) {
    const int rc = check_group(ens, ngroups);
    if (rc) return rc;
    return run_group(ngroups, offset_us, [&](int g) {
        return idaens_stream(ens[g], touts, ntout, max_rounds, stagger_rounds, passes_done ? passes_done + g : nullptr);
    });
}

int idaens_solve_schedule_group(idaens* const* ens, int ngroups, const double* touts, int ntout, double* const* hTret, int32_t* const* hStatus,
                                int32_t* const* hReached, long max_rounds) {
    const int rc = check_group(ens, ngroups);
    if (rc) return rc;
    if (!hTret || !hStatus) return -1;
    for (int g = 0; g < ngroups; ++g)
        if (!hTret[g] || !hStatus[g]) return -1;
    return run_group(ngroups, 0, [&](int g) {
        return idaens_solve_schedule(ens[g], touts, ntout, hTret[g], hStatus[g], hReached ? hReached[g] : nullptr, nullptr, nullptr, max_rounds);
    });
}

namespace {
int install_roots(idaens* e, int nroots) {
    for (const Sys& s : e->sys)
        if (s.nst > 0 || s.setup_done) return efail(e, -2, "root functions must be set before the first solve call");
    e->nrtfn = nroots;
    e->hy.assign(e->n, 0.0);
    e->hyp.assign(e->n, 0.0);
    for (Sys& s : e->sys) {
        s.rt.glo.assign(nroots, 0.0);
        s.rt.ghi.assign(nroots, 0.0);
        s.rt.grout.assign(nroots, 0.0);
        s.rt.iroots.assign(nroots, 0.0);
        s.rt.gactive.assign(nroots, 0);  // sic: false (lib.rs:373); r_check1/3 switch them on
    }
    return 0;
}
}  // namespace

int idaens_set_roots(idaens* e, int nroots, const int32_t* comps, const double* thresholds) {
    if (!e || nroots < 0 || (nroots > 0 && (!comps || !thresholds))) return -1;
    for (int i = 0; i < nroots; ++i)
        if (comps[i] < 0 || comps[i] >= e->n) return efail(e, -2, "root function %d: component %d outside 0..%d", i, comps[i], e->n - 1);
    const int rc = install_roots(e, nroots);
    if (rc) return rc;
    e->rt_fn = nullptr;
    e->rt_comp.assign(comps, comps + nroots);
    e->rt_thr.assign(thresholds, thresholds + nroots);
    return 0;
}

int idaens_set_root_fn(idaens* e, int nroots, idaens_root_fn fn, void* user) {
    if (!e || nroots < 0 || (nroots > 0 && !fn)) return -1;
    const int rc = install_roots(e, nroots);
    if (rc) return rc;
    e->rt_fn = nroots > 0 ? fn : nullptr;
    e->rt_user = user;
    e->rt_comp.clear();
    e->rt_thr.clear();
    return 0;
}

int idaens_get_roots(const idaens* e, int32_t* out) {
    if (!e || !out) return -1;
    for (int b = 0; b < e->batch; ++b)
        for (int i = 0; i < e->nrtfn; ++i) out[(size_t)b * e->nrtfn + i] = (int32_t)e->sys[b].rt.iroots[i];
    return 0;
}

int idaens_get_counter(const idaens* e, int which, int64_t* out) {
    if (!e || !out) return -1;
    for (int b = 0; b < e->batch; ++b) {
        const Sys& s = e->sys[b];
        int64_t v = 0;
        switch (which) {
            case IDAENS_C_NST: v = s.nst; break;
            case IDAENS_C_NRE: v = s.nre; break;
            case IDAENS_C_NJE: v = s.nje; break;
            case IDAENS_C_NSETUPS: v = s.nsetups; break;
            case IDAENS_C_NNI: v = s.niters; break;  // Q11: nni is the Newton counter (ida_io.rs:84-88)
            case IDAENS_C_NETF: v = s.netf; break;
            case IDAENS_C_NCFN: v = s.ncfn; break;
            case IDAENS_C_NATTEMPTS: v = s.n_attempts; break;
            case IDAENS_C_NLS_NCONVFAILS: v = s.nconvfails; break;
            case IDAENS_C_KUSED: v = s.kused; break;
            case IDAENS_C_KK: v = s.kk; break;
            case IDAENS_C_NGE: v = s.nge; break;
            case IDAENS_C_NLUFAIL: v = s.nlufail; break;
            case IDAENS_C_NCONV_JCUR: v = s.nconv_jcur; break;
            case IDAENS_C_NFAIL_FIRST: v = s.nfail_first; break;
            case IDAENS_C_NLI: v = s.nli; break;
            case IDAENS_C_NCFL: v = s.ncfl; break;
            case IDAENS_C_NRE_DQ: v = s.nre_dq; break;
            case IDAENS_C_NBACKTR: v = s.nbacktr; break;
            case IDAENS_C_NPE: v = s.npe; break;
            case IDAENS_C_NPS: v = s.nps; break;
            default: return -2;
        }
        out[b] = v;
    }
    return 0;
}

int idaens_get_real(const idaens* e, int which, double* out) {
    if (!e || !out) return -1;
    for (int b = 0; b < e->batch; ++b) {
        const Sys& s = e->sys[b];
        switch (which) {
            case IDAENS_R_TN: out[b] = s.tn; break;
            case IDAENS_R_HUSED: out[b] = s.hused; break;
            case IDAENS_R_HH: out[b] = s.hh; break;
            case IDAENS_R_H0U: out[b] = s.h0u; break;
            case IDAENS_R_TOLSF: out[b] = s.tolsf; break;
            default: return -2;
        }
    }
    return 0;
}

int idaens_get_yy(idaens* e, double* hYY) {
    if (!e) return -1;
    ENS_CALL(e, idahip_download(e->ctx, IDAHIP_F_YY, 0, e->batch, hYY));
    return 0;
}
int idaens_get_yp(idaens* e, double* hYP) {
    if (!e) return -1;
    ENS_CALL(e, idahip_download(e->ctx, IDAHIP_F_YP, 0, e->batch, hYP));
    return 0;
}

// IDAGetDky coefficients c_j^(k)(t) (lib.rs:464-508, recurrence; C IDA's loop bound, see ida_ensemble.h)
static int get_dky_coeffs(const Sys& s, double t, int k, double* cjk) {
    if (k < 0 || k > s.kused) return IDAENS_BAD_K;
    const double eps = F64_EPS;
    const double tfuzz = 100.0 * eps * (std::fabs(s.tn) + std::fabs(s.hh)) * signum(s.hh);
    const double tp = s.tn - s.hused - tfuzz;
    if ((t - tp) * s.hh < 0.0) return IDAENS_BAD_T;
    double cjk_1[MXORDP1] = {0.0};
    for (int j = 0; j < MXORDP1; ++j) cjk[j] = 0.0;
    const double delt = t - s.tn;
    double psij_1 = 0.0;
    for (int i = 0; i <= k; ++i) {
        const double scalar_i = (double)i;
        if (i == 0) {
            cjk[i] = 1.0;
        } else {
            cjk[i] = cjk[i - 1] * scalar_i / s.psi[i - 1];
            psij_1 = s.psi[i - 1];
        }
        for (int j = i + 1; j <= s.kused - k + i; ++j) {
            cjk[j] = (scalar_i * cjk_1[j - 1] + cjk[j - 1] * (delt + psij_1)) / s.psi[j - 1];
            psij_1 = s.psi[j - 1];
        }
        for (int j = i + 1; j <= s.kused - k + i; ++j) cjk_1[j] = cjk[j];
    }
    return 0;
}

int idaens_get_dky(idaens* e, double t, int k, double* hDky, int32_t* hStatus) {
    if (!e || !hDky || !hStatus) return -1;
    std::vector<int32_t> idx, k0, k1;
    std::vector<double> coef;
    for (int b = 0; b < e->batch; ++b) {
        double cjk[MXORDP1];
        hStatus[b] = get_dky_coeffs(e->sys[b], t, k, cjk);
        if (hStatus[b] != 0) continue;
        idx.push_back(b);
        k0.push_back(k);
        k1.push_back(e->sys[b].kused);
        coef.insert(coef.end(), cjk, cjk + MXORDP1);
    }
    if (idx.empty()) return 0;
    std::vector<double> out(idx.size() * (size_t)e->n);
    ENS_CALL(e, idahip_get_dky(e->ctx, k0.data(), k1.data(), coef.data(), out.data(), idx.data(), (int)idx.size()));
    for (size_t s = 0; s < idx.size(); ++s)
        std::memcpy(hDky + (size_t)idx[s] * e->n, out.data() + s * e->n, sizeof(double) * e->n);
    return 0;
}

int64_t idaens_total_newton_iters(const idaens* e) {
    int64_t t = 0;
    if (e) {
        t = e->retired_iters;
        for (const Sys& s : e->sys) t += s.niters;
    }
    return t;
}
int64_t idaens_total_rounds(const idaens* e) { return e ? e->total_rounds : 0; }

int idaens_trace_system(idaens* e, int sys) {
    if (!e || sys < -1 || sys >= e->batch) return -1;
    e->trace_sys = sys;
    e->trace.clear();
    return 0;
}
long idaens_trace_len(const idaens* e) { return e ? (long)(e->trace.size() / 3) : 0; }
int idaens_trace_get(const idaens* e, double* out) {
    if (!e || !out) return -1;
    for (size_t i = 0; i < e->trace.size(); ++i) out[i] = e->trace[i];
    return 0;
}

}  // extern "C"
