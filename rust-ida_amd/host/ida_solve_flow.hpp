// Ida::solve's flow for ONE system, above the scalar controller (ida_controller.hpp): root finding, stop tests, the entry of a
// call, the first-call scalars, the loop-top checks and what follows the Newton solve of a step attempt. One source for both
// places that run it, compiled exactly as ida_controller.hpp is:
//   * the host stepper (ensemble_ida.cpp, g++): per system between its batched device calls, and
//   * the device steppers (csrc/ida_flow.hpp, hipcc): per thread (tiny_ida.hpp) or per workgroup (round_ida.hpp).
// Mirrors, with the reference's names:
//   Ida::solve            src/impl_solve.rs:69-376  (first-call scalars, call entry, loop-top checks, failed step)
//   stop_test1/2          src/impl_stop_test.rs:36-211 (tstop: idaens_set_stop_time; the reference has the tests but no setter)
//   r_check1/2/3, root_finding  src/impl_r_check.rs:32-576
// Whatever touches vectors goes through a backend B, a small adapter each side writes. Every member returns 0 or a negative
// IDAENS_* code, which the functions here pass up unchanged (a backend that always returns 0 costs nothing: the checks fold):
//   interp(t)           y(t), y'(t) become the current yy, yp (get_solution, lib.rs:1274)
//   solution_at(t)      get_solution(t) for the caller's output (the host defers the sums to a list)
//   eval(t, g)          g at the current yy, yp
//   eval_start(g)       g at phi[0], phi[1], for r_check1
//   yy_from_phi01(f)    yy = phi[0] + f * phi[1]
//   yy_add_phi1(f)      yy += f * phi[1]
// The root state RS is used only as rs.glo[i], rs.ghi[i], rs.grout[i], rs.iroots[i], rs.gactive[i] for i < nr: the device's
// idahip_root_state, a struct of vectors on the host. RS = NoRoots compiles the root finding out of enter_call and
// root_return_after_step (the device steppers' no-roots kernels pay registers and scratch for it otherwise).
#pragma once
#include <type_traits>

#include "ida_controller.hpp"
#include "../../include/ida_ensemble.h"

namespace idactl {

struct NoRoots {};

IDA_HD inline double root_ttol(const SysCore& s) { return (IDA_FABS(s.tn) + IDA_FABS(s.hh)) * F64_EPS * 100.0; }

// ---------------------------------------------------------------- root finding (impl_r_check.rs:32-576)
// impl_r_check.rs:32-115 -- at the first call, before phi[1] is scaled by hh. 0 or < 0.
template <class RS, class B>
IDA_HD inline int r_check1(SysCore& s, RS& rs, int nr, B& be) {
    for (int i = 0; i < nr; ++i) rs.iroots[i] = 0.0;
    s.tlo = s.tn;
    s.ttol = root_ttol(s);
    int rc = be.eval_start(&rs.glo[0]);  // g(tlo, phi[0], phi[1])
    if (rc) return rc;
    s.nge = 1;
    bool zroot = false;
    for (int i = 0; i < nr; ++i)
        if (IDA_FABS(rs.glo[i]) == 0.0) {
            rs.gactive[i] = 0;
            zroot = true;
        }
    if (zroot) {
        const double hratio = IDA_FMAX(s.ttol / IDA_FABS(s.hh), 0.1);
        const double smallh = hratio * s.hh;
        rc = be.yy_from_phi01(smallh);
        if (rc) return rc;
        rc = be.eval(s.tlo + smallh, &rs.ghi[0]);
        if (rc) return rc;
        s.nge += 1;
        for (int i = 0; i < nr; ++i)
            if (!rs.gactive[i] && IDA_FABS(rs.ghi[i]) != 0.0) {
                rs.gactive[i] = 1;
                rs.glo[i] = rs.ghi[i];
            }
    }
    return 0;
}

// impl_r_check.rs:117-219 -- on re-entry after a root return. IDAENS_UNFINISHED (continue), ROOT_RETURN or < 0.
template <class RS, class B>
IDA_HD inline int r_check2(SysCore& s, RS& rs, int nr, B& be) {
    if (!s.irfnd) return IDAENS_UNFINISHED;
    int rc = be.interp(s.tlo);
    if (rc) return rc;
    rc = be.eval(s.tlo, &rs.glo[0]);
    if (rc) return rc;
    s.nge += 1;
    for (int i = 0; i < nr; ++i) rs.iroots[i] = 0.0;
    bool zroot = false;
    for (int i = 0; i < nr; ++i)
        if (rs.gactive[i] && IDA_FABS(rs.glo[i]) == 0.0) {
            zroot = true;
            rs.iroots[i] = 1.0;
        }
    if (zroot) {
        s.ttol = root_ttol(s);
        const double smallh = s.ttol * signum(s.hh);
        const double tplus = s.tlo + smallh;
        if ((tplus - s.tn) * s.hh >= 0.0) {
            const double hratio = smallh / s.hh;
            rc = be.yy_add_phi1(hratio);
        } else {
            rc = be.interp(tplus);
        }
        if (rc) return rc;
        rc = be.eval(tplus, &rs.ghi[0]);
        if (rc) return rc;
        s.nge += 1;
        bool zroot2 = false;
        for (int i = 0; i < nr; ++i) {
            if (!rs.gactive[i]) continue;
            if (IDA_FABS(rs.ghi[i]) == 0.0) {
                if (rs.iroots[i] > 0.0) return IDAENS_CLOSE_ROOTS;
                zroot2 = true;
                rs.iroots[i] = 1.0;
            } else if (rs.iroots[i] > 0.0) {
                rs.glo[i] = rs.ghi[i];
            }
        }
        if (zroot2) return IDAENS_ROOT_RETURN;
    }
    return IDAENS_UNFINISHED;
}

template <class RS>
IDA_HD inline void scan_roots(const RS& rs, int nr, const double* gval, bool first, bool* zroot, bool* sgnchg, int* imax) {
    double maxfrac = 0.0;
    *zroot = false;
    *sgnchg = false;
    for (int i = 0; i < nr; ++i) {
        if (!rs.gactive[i]) continue;
        const bool rootdir_glo_neg = 0.0 * rs.glo[i] <= 0.0;  // rootdir is 0 (no setter in the reference, lib.rs:372)
        if (first) {  // impl_r_check.rs:361-383
            if (IDA_FABS(gval[i]) == 0.0) {
                if (rootdir_glo_neg) *zroot = true;
                continue;
            }
        } else if (IDA_FABS(gval[i]) == 0.0 && rootdir_glo_neg) {  // impl_r_check.rs:486-504
            *zroot = true;
            continue;
        }
        if (rs.glo[i] * gval[i] < 0.0 && rootdir_glo_neg) {
            const double gfrac = IDA_FABS(gval[i] / (gval[i] - rs.glo[i]));
            if (gfrac > maxfrac) {
                *sgnchg = true;
                maxfrac = gfrac;
                *imax = i;
            }
        }
    }
}

// impl_r_check.rs:343-576 (modified secant / Illinois). IDAENS_UNFINISHED (no root), ROOT_RETURN or < 0.
template <class RS, class B>
IDA_HD inline int root_find(SysCore& s, RS& rs, int nr, B& be) {
    int imax = 0;
    bool zroot, sgnchg;
    scan_roots(rs, nr, &rs.ghi[0], true, &zroot, &sgnchg, &imax);
    if (!sgnchg) {
        s.trout = s.thi;
        for (int i = 0; i < nr; ++i) rs.grout[i] = rs.ghi[i];
        if (!zroot) return IDAENS_UNFINISHED;
        for (int i = 0; i < nr; ++i) {
            rs.iroots[i] = 0.0;
            if (rs.gactive[i] && IDA_FABS(rs.ghi[i]) == 0.0 && 0.0 * rs.glo[i] <= 0.0) rs.iroots[i] = signum(rs.glo[i]);
        }
        return IDAENS_ROOT_RETURN;
    }
    double alph = 1.0;
    int side = 0, sideprev = -1;
    for (;;) {
        if (IDA_FABS(s.thi - s.tlo) <= s.ttol) break;
        if (sideprev == side) alph = (side == 2) ? alph * 2.0 : alph * 0.5;
        else alph = 1.0;
        double tmid = s.thi - (s.thi - s.tlo) * rs.ghi[imax] / (rs.ghi[imax] - alph * rs.glo[imax]);
        if (IDA_FABS(tmid - s.tlo) < 0.5 * s.ttol) {
            const double fracint = IDA_FABS(s.thi - s.tlo) / s.ttol;
            const double fracsub = (fracint > 5.0) ? 0.1 : 0.5 / fracint;
            tmid = s.tlo + fracsub * (s.thi - s.tlo);
        }
        if (IDA_FABS(s.thi - tmid) < 0.5 * s.ttol) {
            const double fracint = IDA_FABS(s.thi - s.tlo) / s.ttol;
            const double fracsub = (fracint > 5.0) ? 0.1 : 0.5 / fracint;
            tmid = s.thi - fracsub * (s.thi - s.tlo);
        }
        int rc = be.interp(tmid);
        if (rc) return rc;
        rc = be.eval(tmid, &rs.grout[0]);
        if (rc) return rc;
        s.nge += 1;
        sideprev = side;
        scan_roots(rs, nr, &rs.grout[0], false, &zroot, &sgnchg, &imax);
        if (sgnchg) {
            s.thi = tmid;
            for (int i = 0; i < nr; ++i) rs.ghi[i] = rs.grout[i];
            side = 1;
            if (IDA_FABS(s.thi - s.tlo) <= s.ttol) break;
            continue;
        }
        if (zroot) {
            s.thi = tmid;
            for (int i = 0; i < nr; ++i) rs.ghi[i] = rs.grout[i];
            break;
        }
        s.tlo = tmid;
        for (int i = 0; i < nr; ++i) rs.glo[i] = rs.grout[i];
        side = 2;
        if (IDA_FABS(s.thi - s.tlo) <= s.ttol) break;
    }
    s.trout = s.thi;
    for (int i = 0; i < nr; ++i) rs.grout[i] = rs.ghi[i];
    for (int i = 0; i < nr; ++i) {
        rs.iroots[i] = 0.0;
        if (rs.gactive[i] && 0.0 * rs.glo[i] <= 0.0 && (IDA_FABS(rs.ghi[i]) == 0.0 || rs.glo[i] * rs.ghi[i] < 0.0))
            rs.iroots[i] = signum(rs.glo[i]);
    }
    return IDAENS_ROOT_RETURN;
}

// impl_r_check.rs:221-280 -- after a successful step. IDAENS_UNFINISHED (no root), ROOT_RETURN or < 0.
template <class RS, class B>
IDA_HD inline int r_check3(SysCore& s, RS& rs, int nr, B& be) {
    if (s.taskc == IDAENS_ONE_STEP) s.thi = s.tn;
    else s.thi = ((s.toutc - s.tn) * s.hh >= 0.0) ? s.tn : s.toutc;
    int rc = be.interp(s.thi);
    if (rc) return rc;
    rc = be.eval(s.thi, &rs.ghi[0]);
    if (rc) return rc;
    s.nge += 1;
    s.ttol = root_ttol(s);
    const int ier = root_find(s, rs, nr, be);
    if (ier < 0) return ier;
    for (int i = 0; i < nr; ++i)
        if (!rs.gactive[i] && rs.grout[i] != 0.0) rs.gactive[i] = 1;
    s.tlo = s.trout;
    for (int i = 0; i < nr; ++i) rs.glo[i] = rs.grout[i];
    if (ier == IDAENS_ROOT_RETURN) {
        rc = be.interp(s.trout);
        if (rc) return rc;
    }
    return ier;
}

// ---------------------------------------------------------------- stop tests (impl_stop_test.rs:36-211)
// With a stop time (s.tstopset, idaens_set_stop_time) a test may return IDAENS_TSTOP_RETURN -- y(tstop) interpolated, tret = tretlast =
// tstop, the stop time consumed (ida_tstop = None) -- or IDAENS_BAD_TSTOP, or clip hh so that the next step ends at tstop.
// One deviation from the reference's text: the ONE_STEP branch of stop_test1 returns TSTOP without clearing the
// stop time there (impl_stop_test.rs:109-113), so every later ONE_STEP call would return TSTOP again; C IDA clears it, and so does this.
IDA_HD inline double tstop_roundoff(const SysCore& s) { return 100.0 * F64_EPS * (IDA_FABS(s.tn) + IDA_FABS(s.hh)); }
// the step after this one would pass tstop: it ends there instead
IDA_HD inline void tstop_clip_hh(SysCore& s) {
    if ((s.tn + s.hh - s.tstop) * s.hh > 0.0) s.hh = (s.tstop - s.tn) * (1.0 - 4.0 * F64_EPS);
}

// whether tn has reached the stop time (within the round-off of the step)
template <bool TS>
IDA_HD inline bool tstop_reached(const SysCore& s) {
    if constexpr (TS) return s.tstopset && IDA_FABS(s.tn - s.tstop) <= tstop_roundoff(s);
    else return false;
}
template <bool TS>
IDA_HD inline bool tstop_is_set(const SysCore& s) {
    if constexpr (TS) return s.tstopset;
    else return false;
}
// TS = false compiles the stop time out of the functions below, for a caller that knows no system of its call has one: with it
// compiled in, stop_test1 alone costs the no-roots round_begin_kernel of the device lock-step rounds 58 -> 75 vector registers and a
// wave of occupancy, so those kernels are instantiated both ways, as they are for ROOTS.

// (each test interpolates at ONE place, for tout or for tstop: the device steppers inline get_solution at every call site)
template <bool TS = true, class B>
IDA_HD inline int stop_test1(SysCore& s, double tout, int itask, B& be) {
    if (tstop_is_set<TS>(s)) {
        if ((s.tn - s.tstop) * s.hh > 0.0) return IDAENS_BAD_TSTOP;  // the stop time is behind tn
    }
    double t;
    bool at_tstop = false;
    if (itask == IDAENS_NORMAL) {
        if (tout == s.tretlast) {
            s.tretlast = tout;
            s.tret = tout;
            return IDAENS_SUCCESS;
        }
        if ((s.tn - tout) * s.hh >= 0.0) t = tout;
        else if (tstop_reached<TS>(s)) at_tstop = true;
        else {
            if (tstop_is_set<TS>(s)) tstop_clip_hh(s);
            return IDAENS_UNFINISHED;  // ContinueSteps
        }
    } else {
        if ((s.tn - s.tretlast) * s.hh > 0.0) t = s.tn;
        else if (tstop_reached<TS>(s)) at_tstop = true;
        else {
            if (tstop_is_set<TS>(s)) tstop_clip_hh(s);
            return IDAENS_UNFINISHED;
        }
    }
    if (at_tstop) t = s.tstop;
    const int ier = be.solution_at(t);
    // a failed interpolation: returned as it is for tout (and for ONE_STEP's tstop, :109), BAD_TSTOP for NORMAL's tstop (:71-75);
    // ONE_STEP's interpolation at tn itself cannot fail and the reference ignores its result (:97)
    if (ier && (at_tstop || itask == IDAENS_NORMAL)) return (at_tstop && itask == IDAENS_NORMAL) ? IDAENS_BAD_TSTOP : ier;
    s.tretlast = t;
    s.tret = t;
    if (!at_tstop) return IDAENS_SUCCESS;
    s.tstopset = false;  // consumed. Q15: the reference leaves it set in the ONE_STEP branch (:109-113)
    return IDAENS_TSTOP_RETURN;
}

template <bool TS = true, class B>
IDA_HD inline int stop_test2(SysCore& s, double tout, int itask, B& be) {
    if (itask == IDAENS_NORMAL) {
        double t;
        bool at_tstop = false;
        if ((s.tn - tout) * s.hh >= 0.0) t = tout;
        else if (tstop_reached<TS>(s)) {
            at_tstop = true;
            t = s.tstop;
        } else {
            if (tstop_is_set<TS>(s)) tstop_clip_hh(s);
            return IDAENS_UNFINISHED;
        }
        s.tret = t;
        s.tretlast = t;
        (void)be.solution_at(t);
        if (!at_tstop) return IDAENS_SUCCESS;
        s.tstopset = false;
        return IDAENS_TSTOP_RETURN;
    }
    if (tstop_is_set<TS>(s)) {  // OneStep
        if (tstop_reached<TS>(s)) {
            (void)be.solution_at(s.tstop);
            s.tret = s.tstop;
            s.tretlast = s.tstop;
            s.tstopset = false;
            return IDAENS_TSTOP_RETURN;
        }
        tstop_clip_hh(s);
    }
    s.tret = s.tn;  // yy/yp already hold y(tn)
    s.tretlast = s.tn;
    return IDAENS_SUCCESS;
}

// ---------------------------------------------------------------- entry of one Ida::solve(s.tout_cur) call for a system that is
// between calls (impl_solve.rs:179-241): root checks and stop tests. IDAENS_UNFINISHED when the system has to step, else the
// status this call returns with (tret set).
template <bool TS = true, class RS, class B>
IDA_HD inline int enter_call(SysCore& s, RS& rs, int nr, int itask, B& be) {
    const double tout = s.tout_cur;
    s.nstloc = 0;
    if (itask == IDAENS_NORMAL) s.toutc = tout;
    s.taskc = itask;
    if constexpr (!std::is_same<RS, NoRoots>::value) {
        if (s.nst > 0 && nr > 0) {  // impl_solve.rs:187-229
            const bool irfndp = s.irfnd;
            int ier = r_check2(s, rs, nr, be);
            if (ier < 0) {
                s.dead = true;
                return ier;
            }
            if (ier == IDAENS_ROOT_RETURN) {
                s.tretlast = s.tlo;
                s.tret = s.tlo;
                return IDAENS_ROOT_RETURN;
            }
            const double troundoff = root_ttol(s);
            if (IDA_FABS(s.tn - s.tretlast) > troundoff) {
                ier = r_check3(s, rs, nr, be);
                if (ier < 0) {
                    s.dead = true;
                    return ier;
                }
                if (ier == IDAENS_UNFINISHED) {
                    s.irfnd = false;
                    if (itask == IDAENS_ONE_STEP && irfndp) {
                        s.tretlast = s.tn;
                        s.tret = s.tn;
                        (void)be.solution_at(s.tn);
                        return IDAENS_SUCCESS;
                    }
                } else {  // root found
                    s.irfnd = true;
                    s.tretlast = s.tlo;
                    s.tret = s.tlo;
                    return IDAENS_ROOT_RETURN;
                }
            }
        }
    }
    if (s.nst > 0) {
        const int istate = stop_test1<TS>(s, tout, itask, be);
        if (istate != IDAENS_UNFINISHED) {
            if (istate < 0) s.dead = true;
            return istate;
        }
    }
    return IDAENS_UNFINISHED;
}

// ---------------------------------------------------------------- the scalars of the first-call block (impl_solve.rs:84-173)
// ypnorm = ||phi[1]|| for the h0 heuristic, p0nrm = ||phi[0]|| for the first tolsf test. false: the call returns IDAENS_ILL_INPUT
// for this system; true: it has started (the caller runs r_check1, then scales phi[1] by hh).
template <bool TS = true>
IDA_HD inline bool first_call_scalars(SysCore& s, double tout, double ypnorm, double p0nrm, double epcon, double hmax_inv, bool y0_violates) {
    const double tdist = IDA_FABS(tout - s.tn);
    const double troundoff = 2.0 * F64_EPS * (IDA_FABS(s.tn) + IDA_FABS(tout));
    if (tdist == 0.0 || tdist < troundoff) {
        s.status = IDAENS_ILL_INPUT;  // "tout too close to t0 to start integration"
        s.tret = s.tn;
        return false;
    }
    if (y0_violates) {
        s.status = IDAENS_ILL_INPUT;  // y0 does not satisfy the constraints
        s.tret = s.tn;
        return false;
    }
    double hh = s.hin;
    if (hh == 0.0) {
        hh = 0.001 * tdist;
        if (ypnorm > 2.0 / hh) hh = 0.5 / ypnorm;  // Q7 kept (impl_solve.rs:127)
        if (tout < s.tn) hh = -hh;
    }
    const double rh = IDA_FABS(hh) * hmax_inv;
    if (rh > 1.0) hh /= rh;
    if (tstop_is_set<TS>(s)) {  // impl_solve.rs:137-150
        if ((s.tstop - s.tn) * hh <= 0.0) {
            s.status = IDAENS_ILL_INPUT;  // the stop time is behind t0 in the direction of integration: nothing of the record has changed
            s.tret = s.tn;
            return false;
        }
        if ((s.tn + hh - s.tstop) * hh > 0.0) hh = (s.tstop - s.tn) * (1.0 - 4.0 * F64_EPS);
    }
    s.setup_done = true;
    s.hh = hh;
    s.h0u = s.hh;
    s.kk = 0;
    s.kused = 0;
    s.eps_newt = epcon;
    s.toldel = 0.0001 * s.eps_newt;
    s.phi0nrm = p0nrm;
    return true;
}

// ---------------------------------------------------------------- loop-top checks of a new step (impl_solve.rs:246-297);
// false = the call returns
template <class B>
IDA_HD inline bool loop_top(SysCore& s, long mxstep, B& be) {
    if (mxstep > 0 && s.nstloc >= mxstep) {
        s.tret = s.tn;
        s.tretlast = s.tn;
        s.status = IDAENS_TOO_MUCH_WORK;  // recoverable for the caller: the next solve call continues
        s.ph = PH_IDLE;
        return false;
    }
    if (s.nst > 0 && s.ewt_bad) {
        (void)be.solution_at(s.tn);
        s.tret = s.tn;
        s.tretlast = s.tn;
        s.status = IDAENS_ILL_INPUT;
        s.dead = true;
        s.ph = PH_IDLE;
        return false;
    }
    s.tolsf = F64_EPS * s.phi0nrm;
    if (s.tolsf > 1.0) {
        s.tolsf *= 10.0;
        s.tret = s.tn;
        s.tretlast = s.tn;
        if (s.nst > 0) (void)be.solution_at(s.tn);
        s.status = IDAENS_TOO_MUCH_ACC;
        s.dead = true;
        s.ph = PH_IDLE;
        return false;
    }
    return true;
}

// ---------------------------------------------------------------- after the Newton solve of a step attempt (s.nls_ret set)
// What step() makes of it (lib.rs:655-690): NFLAG_NONE when the attempt passed the error test. cflag: the constraint check's
// verdict (0 passed or none | 1 corrected | 2 recover with the step-size factor crr).
IDA_HD inline int attempt_nflag(SysCore& s, int cflag, double crr, const double* norms, double* err_k, double* err_km1) {
    int nflag = NFLAG_NONE;
    *err_k = 0.0;
    *err_km1 = 0.0;
    if (cflag == 2) {
        nflag = NFLAG_CONSTR_RECVR;
        s.rr = crr;  // kept by handle_n_flag
    } else if (s.nls_ret == NLS_SUCCESS) {
        if (!test_error(s, s.ck, norms, err_k, err_km1)) nflag = NFLAG_TEST_FAIL;
    } else if (s.nls_ret == NLS_CONV_RECVR) {
        nflag = NFLAG_CONV_RECVR;
    } else {
        nflag = NFLAG_LSETUP_RECVR;
    }
    return nflag;
}
// the step failed for good (handle_n_flag returned kflag != 0): Ida::solve's failed-step path (impl_solve.rs:300-313)
template <class B>
IDA_HD inline void step_failed(SysCore& s, int kflag, B& be) {
    if (be.solution_at(s.tn) == 0) {
        s.tret = s.tn;
        s.tretlast = s.tn;
    }
    s.status = kflag;
    s.dead = true;
    s.ph = PH_IDLE;
}
// a failed attempt while nst == 0: reset() (Q5). The caller scales phi[1] by s.rr.
IDA_HD inline void first_step_reset(SysCore& s) { s.psi[0] = s.hh; }

// after an accepted step (impl_solve.rs:343-356): true = the call returns, with a root or with r_check3's error
template <class RS, class B>
IDA_HD inline bool root_return_after_step(SysCore& s, RS& rs, int nr, B& be) {
    if constexpr (!std::is_same<RS, NoRoots>::value) {
        if (nr > 0) {
            const int ier = r_check3(s, rs, nr, be);
            if (ier < 0) {
                s.status = ier;
                s.dead = true;
                s.ph = PH_IDLE;
                return true;
            }
            if (ier == IDAENS_ROOT_RETURN) {
                s.irfnd = true;
                s.tretlast = s.tlo;
                s.tret = s.tlo;
                s.status = IDAENS_ROOT_RETURN;
                s.ph = PH_IDLE;
                return true;
            }
        }
    }
    return false;
}

// idaens_stream: the system has finished its schedule and is to be created anew (Ida::new) and started over
IDA_HD inline bool stream_restart_due(const SysCore& s, int ntout) {
    return s.ph == PH_IDLE && !s.dead && s.setup_done && s.status == IDAENS_SUCCESS && s.sched_i == ntout - 1 && s.nst > 0;
}

}  // namespace idactl
