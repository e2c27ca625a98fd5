// Ida::solve for ONE system as device code: what is per thread around the text shared with the host stepper -- the scalar
// controller (host/ida_controller.hpp) and Ida::solve's per-system flow (host/ida_solve_flow.hpp: root finding, stop tests, call
// entry, first-call scalars, loop-top checks, what follows the Newton solve). Here: FlowArgs, the order of the vector primitives,
// the schedule's continuation, the stream's restarts, how a system enters a call. The vector work is behind a backend V:
//   * TinyVec (tiny_ida.hpp):  one thread owns the system, vectors are loops of that thread (n <= 8);
//   * WgVec   (round_ida.hpp): one workgroup owns the system, every thread runs the scalar logic on its own copy of the state
//                              (uniform control flow) and the vector primitives are cooperative, their sums sequential.
// Mirrors   Ida::solve  src/impl_solve.rs:69-376 (the order of the first-call block and of a call, IDA_NORMAL),
//           Ida::step   src/lib.rs:613-711 (attempt loop), complete_step src/impl_complete_step.rs:22-177,
//           get_solution src/lib.rs:1274-1343.
// The Newton solve between attempt_begin() and attempt_end() is the caller's (in-thread for TinyVec, batched kernels for WgVec).
#pragma once
#include "glibc_pow.hpp"
#include "../host/ida_solve_flow.hpp"
#include "common.hpp"

namespace idahip {

struct FlowArgs {
    const double* touts;  // [ntout] (device)
    int ntout;
    int recycle;          // idaens_stream: a system that finished its schedule starts over at once
    int resume;           // continuing a round-limited schedule call: idle systems have finished
    long mxstep;
    int maxord;
    long maxnef, maxncf;
    double epcon, hmax_inv, t0;
    const long long* start_round;  // [batch] or null: idaens_stream's staggered start (absolute round numbers)
    unsigned long long* acc;       // [2] retired Newton iterations, completed passes (idaens_stream)
    int batch;
    // root functions g_i = y[rt_comp[i]] - rt_thr[i] (nrt == 0: no root finding); their per-system state travels with the caller
    int nrt = 0;
    int rt_comp[IDAHIP_MAX_ROOTS] = {0};
    double rt_thr[IDAHIP_MAX_ROOTS] = {0};
};

// V provides: init_first(&ypnorm, &p0nrm), scale_phi1(f), predict(s), post_newton(s, norms[4]), restore_vec(s, kk_att, ns_att),
// complete_step_vec(s, kused, ck, maxord), get_solution_vec(s, kord), emit_output(slot), restore_initial(), and for the root
// functions: sync() (the vector primitives' results are visible to every thread of the system), yy_at(i), phi_at(j, i),
// yy_from_phi01(f) (yy = phi[0] + f * phi[1]), yy_add_phi1(f) (yy += f * phi[1])
// ROOTS = false compiles the root finding out (the steppers' kernels are instantiated both ways: the bracketing code costs
// the no-roots kernels registers and scratch otherwise -- config 2: 57 -> 46 M iters/s with it compiled in).
// CONSTR = true compiles the inequality-constraint check in: V then also provides
// post_newton_constr(s, checked, norms[4], &rr) -> 0 passed | 1 corrected | 2 recover, and constr_phi0_violated().
// TSTOP = false compiles the stop time (idaens_set_stop_time) out: for a call in which no system has one. The lock-step rounds'
// kernels are instantiated both ways (host/ida_solve_flow.hpp says what it costs them otherwise); the one-thread stepper, whose
// occupancy does not change with it, always has it in.
template <class V, bool ROOTS = false, bool CONSTR = false, bool TSTOP = true>
struct IdaFlow {
    const FlowArgs& a;
    idactl::SysCore& s;
    V& v;
    idahip_root_state* rt = nullptr;  // this system's root state (a.nrt > 0)

    // the backend of host/ida_solve_flow.hpp on V: the interpolation of y(t) is V's get_solution_vec, the function family is
    // evaluated in place (nothing crosses PCIe per evaluation); nothing here can fail but a t outside the last step
    struct Backend {
        const IdaFlow& f;
        __device__ int interp(double t) const { return f.get_solution(t); }
        __device__ int solution_at(double t) const { return f.get_solution(t); }
        __device__ int eval(double, double* g) const {  // g_i = y[comp_i] - thr_i at the current yy (examples/roberts.rs:53-56)
            f.v.sync();
            for (int i = 0; i < f.a.nrt; ++i) g[i] = f.v.yy_at(f.a.rt_comp[i]) - f.a.rt_thr[i];
            return 0;
        }
        __device__ int eval_start(double* g) const {
            for (int i = 0; i < f.a.nrt; ++i) g[i] = f.v.phi_at(0, f.a.rt_comp[i]) - f.a.rt_thr[i];
            return 0;
        }
        __device__ int yy_from_phi01(double h) const {
            f.v.yy_from_phi01(h);
            return 0;
        }
        __device__ int yy_add_phi1(double h) const {
            f.v.sync();
            f.v.yy_add_phi1(h);
            return 0;
        }
    };

    // get_solution(t) into yy/yp; returns 0 or IDAENS_BAD_T
    __device__ int get_solution(double t) const {
        int kord = 1;
        const int rc = idactl::get_solution_coeffs(s, t, &kord);
        if (rc) return rc;
        v.get_solution_vec(s, kord);
        return 0;
    }
    // entry of one Ida::solve(s.tout_cur) call: IDA_NORMAL, the only task of the device steppers
    // (enter_call, continue_schedule and start_system are inlined into their callers by force: left to itself the compiler
    // puts one of them out of line in the ROOTS kernels, and the call costs those kernels registers and scratch)
    __device__ __attribute__((always_inline)) int enter_call() const {
        const Backend be{*this};
        if constexpr (ROOTS) {
            return idactl::enter_call<TSTOP>(s, *rt, a.nrt, IDAENS_NORMAL, be);
        } else {
            idactl::NoRoots none;
            return idactl::enter_call<TSTOP>(s, none, 0, IDAENS_NORMAL, be);
        }
    }
    // the call has returned (s.status set, phase idle): with IDAENS_SUCCESS and touts left it enters the next call at once;
    // true = stepping again
    __device__ __attribute__((always_inline)) bool continue_schedule() const {
        for (;;) {
            if (s.status == IDAENS_SUCCESS) v.emit_output(s.sched_i);
            if (s.status != IDAENS_SUCCESS || s.sched_i + 1 >= a.ntout) return false;
            s.sched_i += 1;
            s.tout_cur = a.touts[s.sched_i];
            const int ist = enter_call();
            if (ist == IDAENS_UNFINISHED) {
                s.ph = idactl::PH_LOOP_TOP;
                return true;
            }
            s.status = ist;
        }
    }
    __device__ bool start_violates() const {
        if constexpr (CONSTR) return v.constr_phi0_violated();
        else return false;
    }
    // (re)enter the schedule: the first-call block for a system that has not started (impl_solve.rs:84-173), then the entry
    // of its first Ida::solve call; true = the system steps
    __device__ __attribute__((always_inline)) bool start_system() const {
        const double tout = a.touts[0];
        if (s.ph == idactl::PH_IDLE && s.nst == 0 && !s.setup_done && !s.dead) {
            double ypnorm, p0nrm;
            v.init_first(&ypnorm, &p0nrm);
            if (idactl::first_call_scalars<TSTOP>(s, tout, ypnorm, p0nrm, a.epcon, a.hmax_inv, start_violates())) {
                if constexpr (ROOTS) {
                    if (a.nrt > 0) {  // impl_solve.rs:157-159
                        const Backend be{*this};
                        (void)idactl::r_check1(s, *rt, a.nrt, be);
                        v.sync();
                    }
                }
                v.scale_phi1(s.hh);  // phi[1] = hh * y'
            }
        }
        if (s.dead || !s.setup_done) return false;  // earlier fatal error / ILL_INPUT at the first call: status is sticky
        s.sched_i = 0;
        s.tout_cur = tout;
        const int ist = enter_call();
        if (ist == IDAENS_UNFINISHED) {
            s.ph = idactl::PH_LOOP_TOP;
            return true;
        }
        s.status = ist;
        return continue_schedule();
    }
    // loop-top checks of a new step (impl_solve.rs:246-297); false = the call returns
    __device__ bool loop_top() const {
        const Backend be{*this};
        return idactl::loop_top(s, a.mxstep, be);
    }
    // a step attempt up to the Newton solve: step() prologue, set_coeffs, tn += hh, lsetup decision, prediction
    __device__ void attempt_begin() const {
        idactl::begin_attempt<TSTOP>(s);
        v.predict(s);
    }
    // the rest of the attempt once the Newton solve has set s.nls_ret; true = the system steps on
    __device__ bool attempt_end() const {
        const Backend be{*this};
        double norms[4], crr = 0.0;
        int cflag = 0;
        if constexpr (CONSTR) cflag = v.post_newton_constr(s, s.nls_ret == idactl::NLS_SUCCESS, norms, &crr);
        else v.post_newton(s, norms);
        double err_k, err_km1;
        const int nflag = idactl::attempt_nflag(s, cflag, crr, norms, &err_k, &err_km1);
        if (nflag != idactl::NFLAG_NONE) {
            const int kk_att = s.kk, ns_att = s.ns;
            idactl::restore_scalars(s);
            v.restore_vec(s, kk_att, ns_att);
            const int kflag = idactl::handle_n_flag(s, nflag, err_k, err_km1, a.maxnef, a.maxncf);
            if (kflag != 0) {
                idactl::step_failed(s, kflag, be);
                return false;
            }
            if (s.nst == 0) {  // reset(): psi[0] = hh; phi[1] *= rr  (Q5)
                idactl::first_step_reset(s);
                v.scale_phi1(s.rr);
            }
            return true;  // predict again
        }
        idactl::complete_step_scalars(s, err_k, err_km1, norms[3], a.maxord, a.hmax_inv);
        v.complete_step_vec(s, s.kused, s.ck, a.maxord);
        s.nstloc += 1;
        s.ph = idactl::PH_LOOP_TOP;
        if constexpr (ROOTS) {
            if (idactl::root_return_after_step(s, *rt, a.nrt, be)) return false;
        }
        const int istate = idactl::stop_test2<TSTOP>(s, s.tout_cur, IDAENS_NORMAL, be);
        if (istate != IDAENS_UNFINISHED) {
            s.status = istate;
            s.ph = idactl::PH_IDLE;
            return continue_schedule();
        }
        return true;
    }
    // what follows a round in idaens_stream (as the `recycle` block of ensemble_ida.cpp's solve_core): a system that finished its
    // schedule is created anew (Ida::new) and starts over; a staggered system starts when its round has come. `ground` = the
    // number of rounds completed. `count`: exactly one thread per system adds to the totals. Returns the new stepping state.
    __device__ bool after_round_stream(bool stepping, long long ground, int b, bool count) const {
        if (!stepping && idactl::stream_restart_due(s, a.ntout)) {
            if (count) {
                atomicAdd(&a.acc[0], (unsigned long long)s.niters);
                atomicAdd(&a.acc[1], 1ull);
            }
            s = idactl::SysCore();
            s.tn = a.t0;
            v.restore_initial();
            return start_system();
        }
        if (!stepping && a.start_round && a.start_round[b] == ground && s.ph == idactl::PH_IDLE && s.nst == 0 && !s.setup_done)
            return start_system();  // staggered start: this system's turn
        return stepping;
    }
    // how a system enters a call (ensemble_ida.cpp: the first block of solve_core)
    __device__ bool enter(long long ground, int b) const {
        if (s.ph != idactl::PH_IDLE) return true;  // left mid-flight by a round limit: resume
        if (a.recycle && a.start_round && a.start_round[b] > ground) return false;  // staggered start: not yet
        if (!a.resume) return start_system();
        return false;
    }
};

}  // namespace idahip
