/* ida_ensemble.h -- C entry points of libidaens.so: the host-side BDF stepper for an ensemble of independent IVPs.
 *
 * This is the caller side of the drop-in boundary: it plays the role of the reference's `Ida` object
 * (src/lib.rs:89-244) -- `Ida::new`, `Ida::solve`, the getters of src/ida_io.rs -- for `batch` systems at once, and
 * reaches the device only through include/ida_hip.h. In the reference this layer is Rust and stays Rust; no Rust
 * toolchain exists in the build image, so the stand-in is C++ with the reference's structure (IdaNLProblem /
 * IdaLProblem / Newton state per system, same names, same error behaviour). All scalar control logic (set_coeffs,
 * lsetup decision, idaNlsConvTest incl. powf, test_error decisions, handle_n_flag, complete_step order/step selection,
 * stop tests, get_solution coefficients) is one source (rust-ida_amd/host/ida_controller.hpp) that runs on the host with the
 * platform libm, per system, exactly as src/lib.rs / src/impl_*.rs do -- or, for small systems, on the device with a pow
 * that reproduces that libm's bits (idaens_set_device_controller); vectors never leave the device.
 */
#ifndef IDA_ENSEMBLE_H
#define IDA_ENSEMBLE_H

#include <stdint.h>

#include "ida_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct idaens idaens;

/* IdaTask (src/lib.rs:50-54) */
enum { IDAENS_NORMAL = 0, IDAENS_ONE_STEP = 1 };
/* per-system return of solve: IdaSolveStatus (src/lib.rs:56-62) >= 0, IdaError (src/error.rs) < 0 */
enum {
    IDAENS_SUCCESS = 0,
    IDAENS_TSTOP_RETURN = 1,
    IDAENS_ROOT_RETURN = 2,
    IDAENS_UNFINISHED = 99, /* round limit hit before the system reached tout (bench mode only) */
    IDAENS_TOO_MUCH_WORK = -1,
    IDAENS_TOO_MUCH_ACC = -2,
    IDAENS_ERR_FAIL = -3,
    IDAENS_CONV_FAIL = -4,
    IDAENS_LSETUP_FAIL = -6,
    IDAENS_CLOSE_ROOTS = -10, /* IdaError::CloseRoots (impl_r_check.rs:199) */
    IDAENS_CONSTR_FAIL = -11, /* the constraints (idahip_set_constraints) could not be met: maxncf failed attempts of one step, the
                                 last of them a constraint failure (C IDA's IDA_CONSTR_FAIL; the reference has no constraints) */
    IDAENS_RTFUNC_FAIL = -12, /* a host root function returned non-zero (C IDA's IDA_RTFUNC_FAIL; the reference has the check
                                 commented out, impl_r_check.rs:83) */
    IDAENS_LINESEARCH_FAIL = -13, /* idaens_calc_ic: the line search failed (C IDA's IDA_LINESEARCH_FAIL) */
    IDAENS_NO_RECOVERY = -14,     /* idaens_calc_ic: a singular Jacobian at the smallest step size tried (IDA_NO_RECOVERY) */
    IDAENS_ILL_INPUT = -22,
    IDAENS_BAD_EWT = -24, /* idaens_calc_ic: a component of the error weights is <= 0 (IDA_BAD_EWT) */
    IDAENS_BAD_K = -25,
    IDAENS_BAD_T = -26,
    IDAENS_BAD_TSTOP = -27 /* IdaError::BadStopTime: the stop time is behind the current t in the direction of integration
                              (impl_stop_test.rs:44-52; C IDA's IDA_ILL_INPUT "tstop is behind current t") */
};

/* Ida::new(problem, yy0, yp0, tol_control) for every system of ctx (src/lib.rs:278-405); ctx must already hold the
 * tolerances and problem data. hYY0, hYP0: [batch][n]. */
int idaens_create(idaens** e, idahip_ctx* ctx, const double* hYY0, const double* hYP0);
int idaens_destroy(idaens* e);
const char* idaens_last_error(const idaens* e);

/* optional inputs (the reference has defaults only, src/lib.rs:309-321; setters follow C IDA's names) */
int idaens_set_max_num_steps(idaens* e, long mxstep); /* 0 = unlimited; default 500 (MXSTEP_DEFAULT) */
int idaens_set_max_ord(idaens* e, int maxord);          /* 1..5, default 5 */
/* on (default; always off for IDAHIP_HOST_CALLBACK problems): a Newton solve runs its first two iterations and their
 * convergence tests in one device call (idahip_newton_iter2) instead of one host round trip per iteration. Results are
 * identical either way; the switch exists for measurements. */
int idaens_set_fused_newton(idaens* e, int on);
/* on (default): the step-size and order controller runs on the device where a device stepper exists
 * (IDA_NORMAL, no trace, not a Krylov ctx unless idahip_set_krylov_rounds is on; root functions only of idaens_set_roots' family and at most IDAHIP_MAX_ROOTS = 4 of
 * them, and not in idaens_stream -- with more functions, or with a user callback (idaens_set_root_fn), the host stepper runs and
 * idaens_device_controller_active reports 0; the results are the same):
 *   - small systems (n <= 8: Roberts, Lorenz63, and reaction networks that opted in with idahip_set_mass_action_tiny, which every
 *     solve call reads anew): a solve / solve_schedule / stream call is ONE launch in which every system
 *     runs its own time loop (idahip_tiny_solve);
 *   - linear dense, heat, Brusselator and mass-action problems with 8 < n <= 4096: lock-step rounds as below, but enqueued without a host round trip
 *     inside a round -- one synchronisation per round, none in idaens_stream (idahip_round_solve); for n > 1024 one more,
 *     hidden behind the residual kernels: the length of the round's LU list comes back to size the factorisation's launches.
 *     A Newton solve that has to start over with a fresh Jacobian does so in the next round, so a system may need one round
 *     more than with the host stepper; its steps, orders, counters and results are the same.
 * off: the lock-step host stepper for every problem. Same results either way (one controller source, pow with glibc's
 * bits); the switch is the A/B. idaens_create compares the device pow with this host's std::pow on the controller's argument
 * ranges once per process: if they differ (another libm than the one glibc_pow.hpp restates) the device steppers stay off,
 * idaens_last_error says so and this call returns 1 for on != 0. */
int idaens_set_device_controller(idaens* e, int on);
/* Which stepper an idaens_solve / _solve_schedule call (IDAENS_NORMAL) of this ensemble would run on as things stand:
 * 0 = the host stepper, 1 = the device stepper with one thread per system (n <= 8), 2 = the device lock-step rounds. A test
 * or a benchmark that means to measure a device stepper asserts this instead of trusting the setter. */
int idaens_device_controller_active(const idaens* e);
/* Root finding (the Root trait, src/traits.rs:72-94; src/impl_r_check.rs): nroots functions g_i(t, y, y') = y[comps[i]] -
 * thresholds[i] for every system -- the form of the reference's Roberts example (g0 = y0 - 1e-4, g1 = y2 - 0.01). Call
 * before the first solve; idaens_solve then reports IDAENS_ROOT_RETURN with tret = the root, yy/yp = the solution there,
 * and idaens_get_roots gives rootsfound (ida_iroots: -1/0/+1 per function). Root closures cannot cross the C ABI, so the
 * functions are this parametrised family. */
int idaens_set_roots(idaens* e, int nroots, const int32_t* comps, const double* thresholds);
int idaens_get_roots(const idaens* e, int32_t* out /* [batch][nroots] */);
/* Root::root (src/traits.rs:72-90) for any user function: gout[0..nroots) = g(t, yy, yp) of system `sys`, evaluated on the
 * host with y(t), y'(t) interpolated on the device and copied back (yy, yp: n doubles, valid during the call). Return 0, or
 * non-zero to fail that system with IDAENS_RTFUNC_FAIL. Replaces idaens_set_roots' family; same calling rules. The bracketing
 * (impl_r_check.rs) is per-system scalar work on the host either way: roots are rare events of single systems. */
typedef int (*idaens_root_fn)(void* user, int32_t sys, double t, const double* yy, const double* yp, int32_t nroots, double* gout);
int idaens_set_root_fn(idaens* e, int nroots, idaens_root_fn fn, void* user);

/* Inequality constraints on the solution: C IDA's IDASetConstraints (the reference has none), as DESIGN.md section 4g defines them.
 * They belong to the ctx -- idahip_set_constraints(ctx, c) with c_i = 0 (none), 1 (y_i >= 0), -1 (y_i <= 0), 2 (y_i > 0), -2 (y_i < 0),
 * shared by the ensemble -- and every idaens_solve / _solve_schedule / _stream call reads at its start whether the ctx has them, so
 * they may be set, changed or cleared between calls. With constraints set:
 *   - a system whose y0 violates them does not start: IDAENS_ILL_INPUT with tret = t0, exactly as for a tout too close to t0;
 *   - after every successful Newton solve the new y is checked; a small violation (weighted norm of the correction <= eps_newt) is
 *     taken out of the step's correction before the error test, a larger one fails the attempt like a convergence failure, with
 *     the step size reduced by rr = max(0.9 min_i phi[0]_i / (phi[0]_i - y_i), 0.1) instead of 0.25. Such failures count in ncfn
 *     and towards maxncf together with convergence and setup failures; when the last allowed one is a constraint failure the system
 *     ends with IDAENS_CONSTR_FAIL, which is fatal and sticky like IDAENS_CONV_FAIL;
 *   - every problem kind (host callbacks included), dense and band contexts, both tasks, root finding, schedules and streams work;
 *     Roberts, Lorenz63 and reaction networks that opted in keep their one-thread-per-system device stepper; for n > 8 the host stepper runs
 *     (idaens_device_controller_active reports 0): the device lock-step rounds have no constraint check.
 * Refused (negative return with a text, nothing launched): any solve call on a ctx with constraints AND difference-quotient
 * Jacobians (C IDA flips the increments' signs there), and idaens_calc_ic on a ctx with constraints (C IDA's line search has a
 * constraint branch of its own). */

/* A Krylov ctx (idahip_create_krylov: matrix-free SPGMR) under the stepper. The iterative branch of idaLsSolve
 * (src/ida_ls.rs:316-418) runs:
 *   - a system whose Newton solve asks for a linear setup gets its residual (idahip_nls_sys) and the setup's bookkeeping only --
 *     nsetups += 1, cjold = cj, cjratio = 1, ss = 20, jcur = true; nothing is formed or factored, nothing can fail, nje stays 0;
 *   - the Newton iteration is idahip_newton_iter_krylov, with the solver's tolerance (sqrt(N) * 0.05) * eps_newt; the correction is not
 *     scaled by 2 / (1 + cjratio); IDAENS_C_NLI grows by the solve's iterations and IDAENS_C_NRE_DQ by as many residual evaluations;
 *     any flag other than SUCCESS adds 1 to IDAENS_C_NCFL and is recoverable: the attempt takes Newton's ConvergenceRecover exit
 *     (a retry with a setup when the setup's data were stale, else a convergence failure of the step, counted in ncfn);
 *   - the fused first two Newton iterations are off (idaens_set_fused_newton changes nothing), idaens_device_controller_active reports 0:
 *     the host stepper runs unless idahip_set_krylov_rounds is on (below); idaens_calc_ic is refused (negative return with a text);
 *   - solve, schedules, streams, groups, both tasks and root finding never touch the linear solver and work unchanged.
 * With the band preconditioner on (idahip_set_krylov_band_prec) the linear setup is real again: the systems that
 * ask for one get, after their residual, one idahip_krylov_psetup call with their tn, cj and hh. Per such system: the bookkeeping
 * above (nje stays), IDAENS_C_NPE += 1, IDAENS_C_NRE_DQ += min(ml+mu+1, n), and a zero pivot in P is a recoverable setup failure
 * exactly as on a dense ctx (IDAENS_C_NLUFAIL counts it there). Every Newton iteration adds 1 + nli to IDAENS_C_NPS.
 * With idahip_set_krylov_rounds(ctx, 1) (off by default; read at the start of every solve call, so it may be changed between
 * round-limited calls) a Krylov ctx of a device kind with 8 < n <= 4096 steps on the device lock-step rounds wherever a dense ctx would
 * (idaens_device_controller_active reports 2; idaens_set_device_controller(e, 0) still forces the host stepper): one synchronisation
 * per round, none in idaens_stream. Every system performs the operations above in the same order with the same arithmetic, so its
 * results and all counters (IDAENS_C_NPE / _NPS / _NLI / _NCFL / _NRE_DQ included) are the host stepper's; a Newton solve that starts
 * over with a setup does so in the next round, so a call may take more rounds. idaens_calc_ic and constraints stay refused. */

/* Stop time: C IDA's IDASetStopTime. The reference's Ida::solve has every stop test (ida_tstop: Option<f64>, src/impl_solve.rs:137-150,
 * src/impl_stop_test.rs:36-211, src/lib.rs:640-644) and no setter; this is the setter. Every system is its own `Ida` object, so every
 * system has its own stop time. hTstop: ntstop = 1 (one value for all systems) or batch values; a NaN entry means "no stop time for
 * this system" and clears one that is set; hTstop == NULL clears all. May be called before the first solve and between solve calls.
 * With a stop time tstop set for a system:
 *   - first call: if (tstop - t0) * h0 <= 0 the system does not start: IDAENS_ILL_INPUT with tret = t0, exactly as for a tout too
 *     close to t0 -- nothing of its state has changed, the caller sets another stop time (or none) and calls again; if the first
 *     step would pass tstop, h0 = (tstop - t0)(1 - 4 eps);
 *   - no step passes tstop: before every step that would, hh = (tstop - tn)(1 - 4 eps);
 *   - a solve call whose tout lies beyond tstop returns IDAENS_TSTOP_RETURN with tret = tstop exactly and yy, yp = y(tstop), y'(tstop)
 *     once tn is within 100 eps (|tn| + |hh|) of tstop; a tout at or before tstop is reached first (IDAENS_SUCCESS). Both tasks;
 *   - the return consumes the stop time (ida_tstop = None): idaens_get_stop_time reports NaN from then on and the caller sets the
 *     next one. (For IDAENS_ONE_STEP the reference's text forgets this at the entry of a call, src/impl_stop_test.rs:109-113, and
 *     would report TSTOP for ever; this library clears it as C IDA does -- SURVEY.md quirk Q15.)
 *   - a solve call that finds tstop behind tn returns IDAENS_BAD_TSTOP, which is sticky like every negative status;
 *   - in idaens_solve_schedule / _group an IDAENS_TSTOP_RETURN ends that system's schedule exactly as a root return does;
 *   - root finding, constraints, every ctx kind (dense, band, Krylov, DQ Jacobians, host callbacks) and all three steppers work;
 *     idaens_device_controller_active reports what it reports without one.
 * Refused (negative return with a text, nothing changed): ntstop other than 1 or batch; an infinite value; any system still inside
 * a round-limited call (it last returned IDAENS_UNFINISHED); for a system that has taken a step (nst > 0), (tstop - tn) * hh < 0 --
 * C IDA's check in IDASetStopTime; the text names the first such system. idaens_stream and idaens_stream_group are refused (negative
 * return with a text, nothing launched) while any system has a stop time: a restarted system is Ida::new, which has none. */
int idaens_set_stop_time(idaens* e, const double* hTstop, int ntstop);
int idaens_get_stop_time(const idaens* e, double* hTstop /* [batch], NaN where none */);

/* Masked error norms: C IDA's IDASetSuppressAlg, the reference's ida_suppressalg (src/lib.rs:138). The switch belongs to the ctx
 * (idahip_set_suppress_alg, ida_hip.h), as the id vector and the constraints do, and is read at the start of every solve call. With
 * it on, every local error norm of the stepper leaves out the algebraic components (id_i = 0). Refused (negative return with a
 * text, nothing launched): any solve call with the switch on and no id vector (C IDA's IDA_MISSING_ID), and idaens_calc_ic with the
 * switch on -- the supported order is idahip_set_id, idaens_calc_ic, idahip_set_suppress_alg(ctx, 1), idaens_solve. */

/* Consistent initial conditions for every system: C IDA's IDACalcIC (the reference has none, src/lib.rs:328-335), as DESIGN.md
 * section 4f defines it -- no constraints, sysindex = 1, line search always on.
 *   IDAENS_YA_YDP_INIT: given the differential components of y0 (idahip_set_id: id_i = 1), compute the algebraic components of y0
 *                       and the differential components of y0' such that F(t0, y0, y0') = 0;
 *   IDAENS_Y_INIT:      given y0', compute y0.
 * tout1: the first output time; only its distance from t0 matters (it scales the step size hic of the Jacobian's cj = 1/hic).
 * To be called before the first solve / solve_schedule / stream call of the ensemble. Refused (negative return, error text, nothing
 * launched or changed) for an unknown icopt, for IDAENS_YA_YDP_INIT on a ctx without an id, and after the first solve call; a
 * host callback that returns non-zero aborts the call with -7. Otherwise returns 0 and hStatus[batch] holds IDAENS_SUCCESS,
 * IDAENS_CONV_FAIL, IDAENS_LINESEARCH_FAIL, IDAENS_NO_RECOVERY, IDAENS_BAD_EWT or IDAENS_ILL_INPUT (tout1 too close to t0) per
 * system. A negative status here is NOT sticky: a system that failed keeps the yy0, yp0 it was created with and may be integrated,
 * or the caller uploads other guesses with a new idaens_create. For a system with status 0 the device's phi[0], phi[1], yy, yp
 * and ewt hold the corrected values (idaens_get_yy / _yp return them) and the snapshot that idaens_stream's restarts begin from
 * is renewed. The work counts in nre, nsetups, nje, nni, ncfn (nre_dq on a DQ ctx) and IDAENS_C_NBACKTR; nothing else of the
 * controller state changes -- the first solve computes its own initial step size. */
enum { IDAENS_YA_YDP_INIT = 1, IDAENS_Y_INIT = 2 };
int idaens_calc_ic(idaens* e, int icopt, double tout1, int32_t* hStatus /* [batch] */);
/* The same for listed systems at any point of a run: systems that have not taken a step since idaens_create or idaens_reinit -- after
 * an event a DAE needs consistent algebraic components and derivatives before it steps on. hTout1 / hStatus: [nsys] by list position;
 * each system's own t0 is its current t. The per-system machine, its statuses and counters are idaens_calc_ic's; the snapshot rows
 * and phi[2..5] are renewed for the listed systems only, and no field of another system changes. Refused (-2 with a text naming the
 * system, nothing changed) when a listed system has started (a step taken, the first-call block run, mid-flight, or a fatal status), for
 * an id out of range or listed twice, and for what idaens_calc_ic refuses: constraints, a Krylov ctx, suppress_alg. */
int idaens_calc_ic_systems(idaens* e, int icopt, const int32_t* hIdx, int nsys, const double* hTout1 /* [nsys] */,
                           int32_t* hStatus /* [nsys] */);

/* C IDA's IDAReInit for the listed systems of a running ensemble: each becomes a created system (Ida::new) at
 * t0 = hT0[q] with y0 = hYY0[q], y0' = hYP0[q] (host arrays by list position, [nsys] and [nsys][n]). Everything per-system starts over:
 * the controller record, all counters (IDAENS_C_NBACKTR, _NPE, _NPS included), the root state (as idaens_set_roots leaves it), no stop
 * time (a restarted system is Ida::new, which has none), and a sticky negative status is gone. The next idaens_solve /
 * idaens_solve_schedule call runs the first-call block for exactly these systems -- the initial step size from that call's tout, the
 * constraints check of y0, the root functions at t0 -- on whichever stepper the call runs on; every other system continues as if
 * the call had not been made. idaens_total_newton_iters keeps the iterations of the discarded integration.
 * idaens_reinit_at_return is the event path: t0 = the tret the system last returned with, and the new values are what it reported
 * there (the device's yy / yp, idaens_get_yy) plus the jump hDY / hDYP ([nsys][n]; NULL: that side as it is), one addition per
 * component on the device -- nothing but the jump crosses to the device.
 * Refused (-2 with a text naming the first offending system, nothing changed): a listed system inside a round-limited call
 * (IDAENS_UNFINISHED); a t0 that is not finite; an id out of range or listed twice; for idaens_reinit_at_return a system that has
 * not returned from a solve call since it was created or reinitialised.
 * idaens_stream / idaens_stream_group restart systems at the ensemble's t0 = 0: while any system's start time differs from it bit
 * for bit they are refused (-2 with a text). After a reinit at t0 = 0 they work, and restart from the new values. */
int idaens_reinit(idaens* e, const int32_t* hIdx, int nsys, const double* hT0 /* [nsys] */, const double* hYY0,
                  const double* hYP0 /* [nsys][n] */);
int idaens_reinit_at_return(idaens* e, const int32_t* hIdx, int nsys, const double* hDY, const double* hDYP /* [nsys][n] or NULL */);

/* Ida::solve(tout, &mut tret, itask) for every system (src/impl_solve.rs:69-376). hTret/hStatus: [batch].
 * max_rounds > 0 bounds the number of lock-step attempt rounds (systems still stepping report IDAENS_UNFINISHED and
 * resume on the next call with the same tout). Returns 0, or < 0 on a device/ABI failure.
 * A negative per-system status (an IdaError) is sticky: later solve calls leave that system alone and report the same status
 * again (the reference's Ida::solve can be called again after an error and would try to continue), until idaens_reinit gives the
 * system new values: a reinitialised system is a created one, with no status.
 * Both time directions are supported: the first tout of a system fixes its direction (tout < t0: hh < 0), and every test of the
 * flow is written with the sign of hh. A tout behind the last step -- tout on the far side of tn - hused, in either direction;
 * a tout inside the last step interpolates -- returns IDAENS_BAD_T, sticky as above, with tret left as the previous return set
 * it. With root functions that refusal comes from the root check of the call's entry, r_check3, whose interpolation at tout it
 * is: r_check3 does NOT evaluate the root functions at a refused tout, and nge does not count such an evaluation. What comes before
 * it is as in the reference: directly after a IDAENS_ROOT_RETURN, r_check2 evaluates g at the root (and once more next to it where
 * a function is zero there) and counts that in nge before r_check3 refuses. (The reference's r_check3 ignores the failed
 * interpolation, evaluates g on the values of the previous return, counts that evaluation and searches a bracket made of them
 * before its stop test refuses the same tout, src/impl_r_check.rs:236-252: since the system is left alone from then on, the
 * library spends nothing on values that are not y(tout).) */
int idaens_solve(idaens* e, double tout, int itask, double* hTret, int32_t* hStatus, long max_rounds);

/* The same for a whole output schedule: for every system Ida::solve(touts[0]), Ida::solve(touts[1]), ... in IDA_NORMAL
 * mode -- each return processed exactly as the reference does (stop tests, interpolation to tout) -- but a system that
 * returns from one call enters the next at once instead of waiting for the slowest system of the batch, so the lock-step
 * rounds stay full. A system's schedule ends early with its first status other than IDAENS_SUCCESS (root return, error).
 * hReached[batch] (optional): number of touts returned with IDAENS_SUCCESS; hYout / hYPout (optional, [ntout][batch][n]):
 * y, y' at every tout reached. With max_rounds > 0 the call may stop early (IDAENS_UNFINISHED); calling again with the same
 * schedule continues it. */
int idaens_solve_schedule(idaens* e, const double* touts, int ntout, double* hTret, int32_t* hStatus, int32_t* hReached,
                          double* hYout, double* hYPout, long max_rounds);

/* Throughput mode: the schedule as above, and a system that has returned from its last tout is created anew from its
 * initial conditions (Ida::new) and starts the schedule again at once -- the batch never drains, every lock-step round
 * works on every system, each somewhere else in its integration. Runs max_rounds rounds; call again to continue.
 * stagger_rounds > 0 (first call only): system b enters at round b * stagger_rounds / batch, which spreads the systems
 * evenly over the phases of an integration from the start. passes_done (optional): integrations completed since the
 * ensemble was created. Per-system counters restart with the system; idaens_total_newton_iters keeps the total. */
int idaens_stream(idaens* e, const double* touts, int ntout, long max_rounds, long stagger_rounds, int64_t* passes_done);

/* Several ensembles side by side on ONE device. The reference integrates one IVP per `Ida` object and
 * nothing couples two objects (src/lib.rs:89-244); how many of them a host puts into one lock-step batch is a scheduling
 * choice. A lock-step round of one large batch is a serial chain of launches, and in some of them most of the chip idles
 * (the panel kernels' pivot chains, the later Newton passes that serve a few hundred systems, round begin / end). Split
 * into `ngroups` ensembles -- each created on its OWN idahip_ctx, hence its own HIP stream -- and driven by one host
 * thread each, one group's idle stretches are filled by the other groups' launches by the device's own scheduler: same
 * systems, same per-system results (every system is integrated exactly as alone), more of them per second.
 * idaens_stream_group = idaens_stream for every ens[g], concurrently; group g starts g * offset_us microseconds after
 * group 0 (0 = together). passes_done: [ngroups] or null. idaens_solve_schedule_group = idaens_solve_schedule for every
 * ens[g], concurrently (arrays of per-group result pointers: hTret[g], hStatus[g] of length batch(ens[g]); hReached may be
 * null). Returns 0, or the first failing group's (negative) code -- that group's idaens_last_error has the text.
 * Host threads: the calling thread drives group 0, ngroups - 1 std::threads the others; a ctx is used by one thread only.
 * Create the contexts on streams from idahip_concurrent_streams (ida_hip.h): the HIP runtime is free to put two ordinary
 * streams on one hardware queue, and those two groups then take turns instead of running side by side. */
int idaens_stream_group(idaens* const* ens, int ngroups, const double* touts, int ntout, long max_rounds, long stagger_rounds, long offset_us,
                        int64_t* passes_done);
int idaens_solve_schedule_group(idaens* const* ens, int ngroups, const double* touts, int ntout, double* const* hTret, int32_t* const* hStatus,
                                int32_t* const* hReached, long max_rounds);

/* getters (src/ida_io.rs:11-117), arrays of length batch */
enum {
    IDAENS_C_NST = 0, IDAENS_C_NRE = 1, IDAENS_C_NJE = 2, IDAENS_C_NSETUPS = 3, IDAENS_C_NNI = 4, IDAENS_C_NETF = 5,
    IDAENS_C_NCFN = 6, IDAENS_C_NATTEMPTS = 7, IDAENS_C_NLS_NCONVFAILS = 8, IDAENS_C_KUSED = 9, IDAENS_C_KK = 10,
    IDAENS_C_NGE = 11 /* root-function evaluations (ida_nge) */,
    /* times the system took a path on which this library follows C IDA and not the reference's text:      */
    IDAENS_C_NLUFAIL = 12 /* Q2: zero pivot reported by the factorisation, treated as recoverable                          */,
    IDAENS_C_NCONV_JCUR = 13 /* Q3/Q4: Newton's ConvergenceRecover with a current Jacobian, treated as recoverable          */,
    IDAENS_C_NFAIL_FIRST = 14 /* Q5: failed attempts before the first step (reset() rescales phi[1] only)                   */,
    IDAENS_C_NLI = 15 /* idaLsSolve: linear iterations (0 with a direct LSolver, src/ida_ls.rs:389-400) */,
    IDAENS_C_NCFL = 16 /* idaLsSolve: linear convergence failures (src/ida_ls.rs:413-415) */,
    IDAENS_C_NRE_DQ = 17 /* residual evaluations of difference-quotient Jacobians (C IDA's nreDQ; idahip_set_jacobian_dq) */,
    IDAENS_C_NBACKTR = 18 /* line-search backtracks of idaens_calc_ic (C IDA's nbacktr) */,
    IDAENS_C_NPE = 19 /* preconditioner setups of a Krylov ctx (C IDA's npe; idahip_set_krylov_band_prec) */,
    IDAENS_C_NPS = 20 /* preconditioner solves of a Krylov ctx (C IDA's nps): 1 + nli per linear solve */
};
int idaens_get_counter(const idaens* e, int which, int64_t* out);
enum { IDAENS_R_TN = 0, IDAENS_R_HUSED = 1, IDAENS_R_HH = 2, IDAENS_R_H0U = 3, IDAENS_R_TOLSF = 4 };
int idaens_get_real(const idaens* e, int which, double* out);
/* get_yy / get_yp: [batch][n] */
int idaens_get_yy(idaens* e, double* hYY);
int idaens_get_yp(idaens* e, double* hYP);
/* Ida::get_dky(t, k, dky) for every system (src/lib.rs:424-529, IDAGetDky): the k-th derivative of the interpolating
 * polynomial of the last step at t. hDky: [batch][n]; hStatus[batch]: IDAENS_SUCCESS, IDAENS_BAD_K (k > kused of that system)
 * or IDAENS_BAD_T (t outside the last step), rows of hDky with a bad status are left untouched. The coefficient recurrence
 * runs here (C IDA's inner-loop bound kused - k + i; the reference's kused - k + 1 agrees for k <= 1, drops terms for
 * k >= 2 and indexes out of bounds for k = 0, kused = 5 -- SURVEY.md quirk Q9), the sums on the device (idahip_get_dky). */
int idaens_get_dky(idaens* e, double t, int k, double* hDky, int32_t* hStatus);
/* totals over the ensemble since creation */
int64_t idaens_total_newton_iters(const idaens* e);
int64_t idaens_total_rounds(const idaens* e);
/* per-accepted-step trace of one system (tn, hused, kused), for parity tests; enable before solving */
int idaens_trace_system(idaens* e, int sys);
long idaens_trace_len(const idaens* e);
int idaens_trace_get(const idaens* e, double* out /* [len][3] */);

#ifdef __cplusplus
}
#endif
#endif
