/* ida_hip.h -- C ABI of libidahip.so: the MI355X (gfx950) implementation of rust-ida's BDF/Newton hot path for an
 * ensemble (batch) of independent IVPs.
 *
 * Every entry point is the batched generalisation of one trait method / function of the reference
 * (jondo2010/rust-ida, paths relative to the reference root); with batch = 1 and nsys = 1 a call reproduces the
 * reference call exactly. A Rust `impl LSolver / NLSolver / NLProblem / IdaProblem` forwards to these symbols
 * (binding sketch: INTEGRATION.md).
 *
 * Conventions
 *   - all floating point is fp64; no FMA contraction anywhere (the reference is plain Rust arithmetic);
 *   - matrices are column-major per system, A(i,j) = a[j*n + i] (nalgebra layout of crates/linear/src/dense.rs);
 *   - "h" pointers are host memory, borrowed for the duration of the call; "d" pointers are device memory;
 *   - hIdx[0..nsys) lists the systems a call acts on (the reference acts on one `Ida` at a time), each at most once: a list
 *     that names a system twice, or an id outside [0, batch), is refused (-2) before anything is uploaded or launched;
 *     per-call scalar arguments (hTn, hCj, ...) are indexed by list position, not by system id;
 *   - return value: 0 ok; > 0 recoverable (some listed system flagged, see the per-system output); < 0 fatal
 *     (bad argument, HIP error) -- the taxonomy documented at crates/nonlinear/src/traits.rs:17-22;
 *   - nothing panics, throws or aborts across this boundary; idahip_last_error() describes the last failure;
 *   - a ctx is not thread-safe (all reference methods take &mut self); different ctxs may be driven concurrently.
 */
#ifndef IDA_HIP_H
#define IDA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct idahip_ctx idahip_ctx; /* opaque; owns all device state of one ensemble on one device */

/* User problems on the device (src/traits.rs:12-70 `Residual`/`Jacobian`; H5 in SURVEY.md: a generic Rust closure cannot cross an
 * FFI into device code). The kinds compiled into the library are selected by enum; a problem of the user's own runs on the device
 * when it is DATA -- IDAHIP_MASS_ACTION, a polynomial reaction network interpreted by table-driven kernels -- and through host
 * functions otherwise (IDAHIP_HOST_CALLBACK). */
typedef enum {
    IDAHIP_ROBERTS = 0,      /* src/sample_problems/roberts.rs:47-91                                  (n = 3) */
    IDAHIP_LORENZ63 = 1,     /* tests/lorenz63.rs:17-25,47-53; params [p, r, b] per system            (n = 3) */
    IDAHIP_LINEAR_DENSE = 2, /* F = A y' + B y - c, A/B dense column-major per system */
    IDAHIP_HEAT1D = 3,       /* 1-D heat, method of lines; params [kappa/dx^2] per system (config 4)           */
    IDAHIP_HOST_CALLBACK = 4, /* any IdaProblem: res / jac are host functions (idahip_set_host_problem); slow path  */
    IDAHIP_BRUSS1D = 5,      /* 1-D Brusselator (reaction-diffusion), method of lines; params [a, b, d, ub, vb] per system: below */
    IDAHIP_MASS_ACTION = 6   /* a mass-action reaction network given as tables (idahip_set_mass_action); params k[R] per system: below */
} idahip_problem;

/* IDAHIP_MASS_ACTION: polynomial kinetics as data. The network is shared by the ensemble: n unknowns (2 <= n <= 4096); R >= 1
 * reactions, reaction r of order o_r in {0,1,2,3} with reactant slots s_r[0..o_r), a slot holding a species index (repeats allowed:
 * y1^2 is the slots (1, 1)), passed as int32 [R][3] with -1 in the unused trailing slots; E >= 0 stoichiometry entries
 * (row i, reaction r, nu) with nu a finite double, which keep, within a row, the order in which the caller listed them; and d[n],
 * finite, the coefficient of y'_i (1.0: a differential row, 0.0: an algebraic one). Per system the rate constants k[R]
 * (idahip_set_problem_params, nparam = R). The operation order is the definition; every line is one IEEE operation, nothing is
 * contracted.
 *   rate:      q_r = k_r, then q_r = q_r * y[s_r[p]] for p = 0, 1, 2 in slot order
 *   residual:  acc = nu_e * q_{r(e)} of the row's first entry, then acc = acc + nu_e * q_{r(e)} for the following entries in order
 *              (acc = +0.0 for a row without entries);   F_i = d_i * y'_i - acc
 *   derivative factor of slot p of reaction r:  g = k_r, then g = g * y[s_r[t]] for every slot t != p, in slot order
 *   J = dF/dy + cj dF/dy':  for a position (i, j), acc = the sum of nu_e * g over the row's entries in row order and, within an
 *              entry, over the slots p in slot order with s_r[p] == j, the first term starting the sum;
 *              base = cj * d_i if i == j, else +0.0;   J(i, j) = base - acc;   a position without a term holds base.
 * The Jacobian's PATTERN is the set of positions with a term, and every diagonal position; idahip_mass_action_pattern reports its
 * size and half-bandwidths. With d = (1, 1, 0), three first-order entries (nu = -1, k = 1) and one zero-order entry (nu = +1, k = 1)
 * in the last row, the form states IDAHIP_ROBERTS by value.
 * The difference-quotient Jacobian is idaLsDenseDQJac below with this residual as the row function, every entry by the definition
 * (a row that does not depend on y_j holds (1/inc)*(+0.0), with the sign of the increment).
 * It runs wherever a dense ctx runs: the host stepper at every n, the fused first two Newton iterations, idahip_ic_*, constraints,
 * and the device lock-step rounds for 8 < n <= 4096; idahip_create_band and idahip_create_krylov refuse the kind (-2), and the
 * one-thread device stepper (n <= 8) does not take it. Until idahip_set_mass_action has been called, every call that would evaluate
 * the problem -- idahip_nls_sys*, idahip_nls_lsetup*, idahip_jac_dq, idahip_newton_iter2, idahip_ic_res / _setup* / _trial,
 * idahip_round_solve, idahip_set_problem_params, idaens_create -- returns -2 with a text, and nothing is launched.
 *
 * RATE LAWS (idahip_set_rate_network instead of idahip_set_mass_action): a reaction may carry FACTORS, at most 4, in the caller's
 * order. A factor is (op, species s, constant c, exponent h) with op IDAHIP_RATE_SAT (y^h / (K^h + y^h): Michaelis-Menten at h = 1,
 * an activating Hill term above) or IDAHIP_RATE_INH (K^h / (K^h + y^h)), 0 <= s < n, 0 <= c < nconst, 1 <= h <= 4. The constants
 * are per system and follow the rate constants in the parameter vector: [k_0 .. k_{R-1}, K_0 .. K_{nconst-1}], nparam = R + nconst.
 *   pw(x, h):   p = x;  (h - 1 times) p = p * x
 *   f(factor):  yh = pw(y_s, h);  Kh = pw(K_c, h);  den = Kh + yh;   SAT: f = yh / den;   INH: f = Kh / den
 *   df(factor): num = Kh if h == 1, else num = ((double)h * Kh) * pw(y_s, h - 1);   q = num / (den * den);   SAT: df = q;   INH: df = -q
 *   rate:       q_r as above, then q_r = q_r * f(factor) for the reaction's factors, in order; the residual is unchanged otherwise
 *   J:          position (i, j) takes the row's entries in order; within an entry first one term per slot p with s_r[p] == j, in
 *               slot order: g as above (k_r times the other slots), then g = g * f(factor) for every factor in order; then one
 *               term per factor whose species is j, in factor order: g = k_r times ALL slots in order, then times the factors in
 *               order with df in place of f for that one factor. Each term is nu_e * g; sum, base and sign as above.
 * The pattern gains the positions reached through a factor. den == 0 is not trapped: the result is what IEEE gives (NaN, +-inf),
 * and a NaN acc is F_i as it is, sign included (the subtraction does not touch it).
 * A network without factors is the polynomial network above, by the same tables and the same kernels. */
#define IDAHIP_RATE_SAT 1
#define IDAHIP_RATE_INH 2
#define IDAHIP_RATE_MAX_FACTORS 4

/* IDAHIP_BRUSS1D: the nonlinear, stiff, banded device problem. m grid points, two species interleaved: n = 2m (even, n >= 10),
 * y[2i] = u_i, y[2i+1] = v_i; parameters [a, b, d, ub, vb] per system (idahip_set_problem_params, nparam = 5), d = the diffusion
 * coefficient divided by dx^2. The operation order is the definition; every line is one IEEE operation, nothing is contracted.
 *   end points i = 0 and i = m-1 (algebraic):   r[2i] = u_i - ub;   r[2i+1] = v_i - vb
 *   interior:  w  = (u_i*u_i)*v_i
 *              lu = (u_{i-1} - 2.0*u_i) + u_{i+1};   lv = (v_{i-1} - 2.0*v_i) + v_{i+1}
 *              r[2i]   = u'_i - (((a - (b + 1.0)*u_i) + w) + d*lu)
 *              r[2i+1] = v'_i - ((b*u_i - w) + d*lv)
 * J = dF/dy + cj dF/dy': identity rows at the end points; interior rows, with t2 = (2.0*u_i)*v_i and uu = u_i*u_i:
 *   J(2i,  2i-2) = -d     J(2i,  2i)   = cj - ((t2 - (b + 1.0)) - 2.0*d)     J(2i,  2i+1) = -uu      J(2i,  2i+2) = -d
 *   J(2i+1,2i-1) = -d     J(2i+1,2i)   = -(b - t2)     J(2i+1,2i+1) = cj + (uu + 2.0*d)              J(2i+1,2i+3) = -d
 * and +0.0 everywhere else, the in-band entries such as J(2i, 2i-1) included: ml = mu = 2. Every ctx constructor refuses the kind
 * for odd n or n < 10 (-2). It runs wherever IDAHIP_HEAT1D runs: dense, band (ml, mu >= 2) and Krylov ctx, band preconditioner of any
 * width, difference-quotient Jacobians, idahip_ic_*, and the device lock-step rounds. */

/* The user problem of kind IDAHIP_HOST_CALLBACK: Residual::res and Jacobian::jac of src/traits.rs:12-70 as C callbacks, called on
 * the host for one listed system at a time (`sys` = its index in the batch, `user` = the pointer given at registration).
 *   res: resval[0..n) = F(tt, yy, yp)                                                       (traits.rs:28-37)
 *   jac: J = dF/dy + cj dF/dy', written column-major (J[j * n + i] = row i, column j) into a matrix the library has zeroed,
 *        as idaLsSetup does (src/ida_ls.rs:255); resvec is the residual at (yy, yp)        (traits.rs:58-69)
 * A nonzero return aborts the call that triggered it (it returns -7). Everything else -- batched LU, triangular solves,
 * norms, the stepper's vectors -- runs on the device as for the built-in problems; y, y' and the residual cross PCIe once
 * per evaluation, the Jacobian once per linear setup. */
typedef int (*idahip_res_fn)(int sys, double tt, const double* yy, const double* yp, double* resval, void* user);
typedef int (*idahip_jac_fn)(int sys, double tt, double cj, const double* yy, const double* yp, const double* resvec, double* J,
                             void* user);

/* The band form of idahip_jac_fn (a ctx made by idahip_create_band): J written into LAPACK band storage that the library has
 * zeroed, element (i, j) at AB[j * ldab + ml + mu + i - j] for j - mu <= i <= j + ml, ldab = 2 ml + mu + 1 (the top ml rows of a
 * column are fill space: leave them zero). */
typedef int (*idahip_band_jac_fn)(int sys, double tt, double cj, const double* yy, const double* yp, const double* resvec, double* AB,
                                  int ldab, void* user);

/* ctx-resident vectors of the reference's IdaNLProblem / Ida structs (src/ida_nls.rs:27-59, src/lib.rs:104-126) */
typedef enum {
    IDAHIP_F_YY = 0,
    IDAHIP_F_YP = 1,
    IDAHIP_F_YYPREDICT = 2,
    IDAHIP_F_YPPREDICT = 3,
    IDAHIP_F_EWT = 4,
    IDAHIP_F_EE = 5,
    IDAHIP_F_DELTA = 6, /* Newton::delta (crates/nonlinear/src/newton.rs:21): residual in, update out */
    IDAHIP_F_SAVRES = 7,
    IDAHIP_F_PHI0 = 8, /* phi[j] = IDAHIP_F_PHI0 + j, j = 0..5 (MXORDP1 = 6, src/constants.rs:6) */
    IDAHIP_F_PHI5 = 13
} idahip_field;

/* ---- lifetime: LS::new(n) + NLS::new(n, maxiters) + IdaNLProblem::new (src/lib.rs:399-400, src/ida_ls.rs:192) ---- */
int idahip_create(idahip_ctx** ctx, int device, int n, int batch, idahip_problem kind, void* hip_stream /* or NULL */);
int idahip_destroy(idahip_ctx* ctx);
/* A BAND ctx (the SUNLinSol_Band of C IDA; the reference ships only `Dense`, crates/linear/src/traits.rs is where it plugs in):
 * the same ensemble, but the Jacobian of every system has lower bandwidth ml and upper bandwidth mu and is stored, factored and
 * solved in LAPACK band storage ([batch][ldab * n], ldab = 2 ml + mu + 1, rust-ida_amd/csrc/band_kernels.hpp) instead of n x n.
 * Kinds IDAHIP_HEAT1D (ml, mu >= 1), IDAHIP_BRUSS1D (ml, mu >= 2) and IDAHIP_HOST_CALLBACK (idahip_set_host_band_problem), 8 < n <= 4096, 0 <= ml, mu < n;
 * anything else is refused (-2). Exactness: pivots are those of dense_get_rf on the same matrix; factors, solutions and
 * integrations equal the dense ones by value (-0.0 == +0.0; steps, orders, counters, hused and tn bit-identical) for finite
 * inputs -- the contract in band_kernels.hpp. Dense-only calls (idahip_download_lu, idahip_set_linear_dense,
 * idahip_set_host_problem, idahip_ls_setup) return -2 on a band ctx. */
int idahip_create_band(idahip_ctx** ctx, int device, int n, int batch, idahip_problem kind, void* hip_stream, int ml, int mu);
/* 1 for a band ctx (*ml, *mu set when non-null), 0 for a dense one, -1 for a null ctx */
int idahip_band(const idahip_ctx* ctx, int* ml, int* mu);
/* IDAHIP_HOST_CALLBACK on a band ctx: the residual and the band Jacobian callbacks (both required) */
int idahip_set_host_band_problem(idahip_ctx* ctx, idahip_res_fn res, idahip_band_jac_fn bjac, void* user);
/* band factors of one system (hAB [ldab * n]), its pivots (hPiv [n]); a band ctx only */
int idahip_download_lu_band(idahip_ctx* ctx, int sys, double* hAB, int64_t* hPiv);
/* LSolver setup / solve in band storage on caller-owned device buffers dAB [batch][ldab * n], dPiv [batch][n], dX / dB [batch][n],
 * on any ctx (n is the ctx's, no upper limit; 0 <= ml, mu < n). Same list rules, hInfo and return values as idahip_ls_setup /
 * idahip_ls_solve; the factorisation is in place (the fill rows need nothing on entry), the solve may have dX == dB and ignores tol. */
int idahip_ls_setup_band(idahip_ctx* ctx, int ml, int mu, double* dAB, int64_t* dPiv, int32_t* hInfo, const int32_t* hIdx, int nsys);
int idahip_ls_solve_band(idahip_ctx* ctx, int ml, int mu, const double* dAB, const int64_t* dPiv, double* dX, const double* dB, double tol,
                         const int32_t* hIdx, int nsys);
/* ---- A KRYLOV ctx: matrix-free SPGMR behind the iterative branch of idaLsSolve (the reference has no iterative solver; this text and
 * DESIGN.md section 4h are the definition). C IDA's default iterative setup: SPGMR, no preconditioner, scaling by ewt on both sides,
 * modified Gram-Schmidt, maxl = 5, no restarts, J v by a difference quotient of the residual (idaLsDQJtimes). The ctx holds no work
 * matrix, no factors and no pivots: memory per system is O(maxl n) instead of O(n^2). Kinds IDAHIP_HEAT1D, IDAHIP_BRUSS1D, IDAHIP_LINEAR_DENSE (the
 * problem's own A and B remain) and IDAHIP_HOST_CALLBACK (idahip_set_host_residual: there is no Jacobian to ask for); 8 < n <= 4096;
 * maxl = 0 means 5; maxl > 16 or maxl > n is refused (-2).
 *
 * Inner product kdot(x, y): p_i = x_i*y_i; partial q (q = 0..63) is the left-to-right sum of p_q, p_{q+64}, p_{q+128}, ... from +0.0;
 * the result is the left-to-right sum of the 64 partials from +0.0 (partials without an element are +0.0).
 *
 * The solve of one system. In: b, w = ewt, the current yy, yp, rr = savres (the residual there, as idahip_nls_sys leaves it), tn, cj,
 * tol = (sqrt(n) * 0.05) * eps_newt (C IDA's eplin). No FMA; 1/x is a true division; |.| is fabs.
 *   1. V0_i = w_i*b_i; beta = sqrt(kdot(V0, V0)). beta <= tol: nli = 0, flag SUCCESS, res_norm = beta, x = b unchanged.
 *   2. V0_i = V0_i*(1/beta); rot = 1.0; H (17 x 16) all zero.
 *   3. l = 0 .. maxl-1, nli += 1 at the top:
 *        z_i = V_l,i / w_i;  sig = sqrt(n)*1.0;  y'_i = sig*z_i + yy_i;  yp'_i = (cj*sig)*z_i + yp_i;
 *        F' = F(tn, y', yp'), a full residual evaluation in the residual kernel's own operation order;
 *        Jv_i = (1/sig)*(F'_i - rr_i);  V_{l+1},i = w_i*Jv_i;
 *        modified Gram-Schmidt: i = 0..l: H[i][l] = kdot(V_i, V_{l+1}), then V_{l+1} = V_{l+1} - H[i][l]*V_i;
 *        hn = H[l+1][l] = sqrt(kdot(V_{l+1}, V_{l+1}))   (SUNDIALS' rare re-orthogonalisation pass is left out);
 *        earlier rotations, k = 0..l-1, c = q[2k], s = q[2k+1], t1 = H[k][l], t2 = H[k+1][l]:
 *          H[k][l] = c*t1 - s*t2;  H[k+1][l] = s*t1 + c*t2;
 *        new rotation from t1 = H[l][l], t2 = H[l+1][l]:  t2 == 0: c = 1, s = 0;
 *          |t2| >= |t1|: t3 = t1/t2, s = -1/sqrt(1 + t3*t3), c = -s*t3;  otherwise: t3 = t2/t1, c = 1/sqrt(1 + t3*t3), s = -c*t3;
 *        q[2l] = c; q[2l+1] = s; H[l][l] = c*t1 - s*t2 (H[l+1][l] keeps hn);
 *        rot = rot*s; rho = |rot*beta|; res_norm = rho; rho <= tol: converged, krydim = l+1, leave the loop;
 *        otherwise V_{l+1},i = V_{l+1},i*(1/hn).
 *   4. no convergence: krydim = maxl; !(rho < beta): flag CONV_FAIL, no solution is formed; otherwise RES_REDUCED.
 *   5. SUCCESS and RES_REDUCED: g = [beta, 0, ...]; the rotations k = 0..krydim-1 applied to g (same two-line form); back-substitution
 *      k = krydim-1 .. 0: H[k][k] == 0: flag QRSOL_FAIL, stop; g[k] = g[k]/H[k][k]; i < k: g[i] = g[i] - g[k]*H[i][k];
 *      xc = g[0]*V0, then xc = xc + g[k]*V_k for ascending k; x_i = xc_i/w_i.
 * Flags: 0 SUCCESS, 1 RES_REDUCED, 2 CONV_FAIL, 3 QRSOL_FAIL. The loop is bounded by maxl whatever the data.
 *
 * Built-in kinds run the whole solve of a listed system in ONE launch (one workgroup per system; the basis [batch][maxl+1][n] stays in
 * L2); idahip_set_krylov_fused(ctx, 0) runs the same device functions one launch per step with the host looping over l -- how a
 * host-callback residual runs (always; the switch is 0 there and cannot be set), and the cross-check of the fused kernel.
 * On a Krylov ctx idahip_ls_type is IDAHIP_LS_ITERATIVE, idahip_ls_num_iters the sum and idahip_ls_res_norm the maximum over the
 * listed systems of the last solve call. Refused with -2: idahip_ls_setup (no dense work matrices), idahip_nls_lsetup*, idahip_nls_sys_setup, idahip_newton_iter,
 * idahip_newton_iter2, idahip_download_lu*, idahip_set_jacobian_dq(1), idahip_set_constraints, idahip_set_host_problem,
 * idahip_ic_*, idahip_round_solve (unless idahip_set_krylov_rounds is on, below). */
int idahip_create_krylov(idahip_ctx** ctx, int device, int n, int batch, idahip_problem kind, void* hip_stream, int maxl);
/* 1 for a Krylov ctx (*maxl set when non-null), 0 otherwise, -1 for a null ctx */
int idahip_krylov(const idahip_ctx* ctx, int* maxl);
int idahip_set_krylov_fused(idahip_ctx* ctx, int on);
int idahip_krylov_fused(const idahip_ctx* ctx); /* 1 fused (the default for built-in kinds), 0 split */
/* The solve of the definition for the listed systems at the ctx-resident yy, yp, savres, ewt: hB, hX host arrays [nsys][n] by list
 * position; hTol, hNli, hFlag, hResNorm [nsys]. The stand-alone LSolver::solve. Returns 1 if some flag is not SUCCESS. */
int idahip_krylov_solve(idahip_ctx* ctx, const double* hTn, const double* hCj, const double* hTol, const double* hB, double* hX,
                        int32_t* hNli, int32_t* hFlag, double* hResNorm, const int32_t* hIdx, int nsys);
/* The Newton loop body on a Krylov ctx: delta = -delta; the solve with b = delta and tol = (sqrt(n)*0.05)*hEpsNewt[s]; flag SUCCESS:
 * delta = x, ee += delta, hDelnrm[s] = ||delta||_wrms(ewt) summed left to right as everywhere else; any other flag: ee is untouched,
 * delta keeps the negated residual, hDelnrm[s] = 0. The correction is not scaled by 2/(1+cjratio) (src/ida_ls.rs:405-410).
 * Returns 1 if some flag is not SUCCESS (recoverable: Newton's ConvergenceRecover exit). */
int idahip_newton_iter_krylov(idahip_ctx* ctx, const double* hTn, const double* hCj, const double* hEpsNewt, double* hDelnrm,
                              int32_t* hNli, int32_t* hFlag, const int32_t* hIdx, int nsys);
/* The device LOCK-STEP ROUNDS on a Krylov ctx (idahip_round_solve below; DESIGN.md section 4h/4i, addendum). Off by default: with the
 * switch off idahip_round_solve refuses a Krylov ctx (-2) and libidaens steps it on the host stepper. With it on, idahip_round_solve
 * takes IDAHIP_HEAT1D and IDAHIP_BRUSS1D (with or without the band preconditioner) and IDAHIP_LINEAR_DENSE (without), 8 < n <= 4096,
 * whatever the LU variant: a round is the sequence of the dense and band contexts with the linear algebra replaced -- the residual for
 * every system whose Newton solve starts, the preconditioner's band DQ Jacobian and factorisation for the listed systems that ask
 * for a setup, and four passes of the one-launch solve (idahip_set_krylov_fused is ignored) with the tolerance
 * (sqrt(n)*0.05)*eps_newt formed on the device from the system's record. Per system the operations, their order and the counters are
 * the host stepper's; idahip_set_lu_period is treated as 1. idahip_ls_num_iters / idahip_ls_res_norm are left as they were.
 * idahip_set_krylov_rounds returns -2 (and changes nothing) on a ctx that is not a Krylov ctx, on IDAHIP_HOST_CALLBACK (a host residual
 * cannot run inside a round) and for on != 0 with n <= 8. May be changed between solve calls.
 * idahip_krylov_rounds: 1 on, 0 off, -1 for a null ctx. */
int idahip_set_krylov_rounds(idahip_ctx* ctx, int on);
int idahip_krylov_rounds(const idahip_ctx* ctx);
/* npe / nps (preconditioner setups and solves per system, C IDA's counters) are not part of the controller record that
 * idahip_round_solve moves: the caller hands the systems' current values to the ctx before the call and reads them back after it,
 * host arrays [batch]. A system that idaens_stream's restarts create anew inside the call starts again from 0. */
int idahip_krylov_rounds_put_counters(idahip_ctx* ctx, const int64_t* hNpe, const int64_t* hNps);
int idahip_krylov_rounds_get_counters(const idahip_ctx* ctx, int64_t* hNpe, int64_t* hNps);
/* ---- The BAND PRECONDITIONER of a Krylov ctx: left-preconditioned SPGMR (C IDA's IDABBDPRE with one block and left preconditioning
 * in SPGMR; neither the reference nor a SUNDIALS copy is at hand: this text and DESIGN.md section 4i are the definition). Off by
 * default; with it off nothing of the ctx changes.
 *
 * A Krylov ctx may carry a band preconditioner with half-bandwidths (ml, mu), 0 <= ml, mu < n. Storage: per system P is held in LAPACK
 * band storage exactly as a band ctx holds its Jacobian -- ldab = 2 ml + mu + 1, [batch][ldab*n] doubles and [batch][n] int64 pivots;
 * O((ml + mu) n) per system.
 *   Setup (psetup): P = the band difference-quotient Jacobian of the "band:" paragraph above (same increments, same groups
 *     g < min(ml+mu+1, n)) at the ctx-resident yy, yp, ewt, rr = savres and the caller's tn, cj, hh; then factored by the band getrf
 *     (the register kernel for (1,1), the generic one otherwise). info = 0, or the 1-based column of a zero pivot. It costs
 *     min(ml+mu+1, n) residual evaluations.
 *   Solve (psolve(r) -> z): the band getrs on those factors: the interleaved forward solve, then back substitution with true division.
 *   Left-preconditioned SPGMR: the solve of the definition above with exactly two changes.
 *     Step 1: r = psolve(b) first, then V0_i = w_i*r_i. On the zero-iteration return (beta <= tol) x = r (C IDA copies the solver's
 *       residual vector, which is P^-1 b). On any failure flag nothing is formed: x / delta keep what they keep without the mode.
 *     Step 3: after Jv_i = (1/sig)*(F'_i - rr_i): u = psolve(Jv), then V_{l+1},i = w_i*u_i.
 *   kdot, Gram-Schmidt, Givens, rho, the flags, steps 4 and 5, x_i = xc_i/w_i, the tolerance, the missing 2/(1+cjratio) scaling and
 *   the missing re-orthogonalisation are unchanged. rho is now the norm of the preconditioned scaled residual. A solve performs
 *   1 + nli preconditioner solves.
 * The band kernels equal the dense LU by value (-0.0 == +0.0) and nothing in SPGMR reads the sign of a zero.
 *
 * idahip_set_krylov_band_prec: turns the mode on and allocates the storage; ml = mu = -1 turns it off and frees it. Kinds
 * IDAHIP_HEAT1D, IDAHIP_BRUSS1D and IDAHIP_HOST_CALLBACK (idahip_set_host_residual), the kinds with a band difference quotient; IDAHIP_LINEAR_DENSE is
 * refused (-2: a random dense Jacobian has no band approximation worth factoring), and so are a ctx that is not a Krylov ctx and
 * widths out of range. With the mode on, idahip_krylov_solve and idahip_newton_iter_krylov run the preconditioned definition; for a
 * listed system without factors yet (no psetup, no upload) they are refused (-2, nothing launched). The four stand-alone calls below
 * are refused the same way on a ctx with the mode off. */
int idahip_set_krylov_band_prec(idahip_ctx* ctx, int ml, int mu);
/* 1 with the mode on (*ml, *mu set when non-null), 0 otherwise, -1 for a null ctx */
int idahip_krylov_band_prec(const idahip_ctx* ctx, int* ml, int* mu);
/* psetup for the listed systems: hTn, hCj, hHh, hInfo [nsys]. Heat and Brusselator: one device pass; host callbacks: the pack / host residual /
 * scatter round trip of a band ctx, once per group. Returns 1 if some info != 0. */
int idahip_krylov_psetup(idahip_ctx* ctx, const double* hTn, const double* hCj, const double* hHh, int32_t* hInfo, const int32_t* hIdx,
                         int nsys);
/* psolve alone (C IDA's IDABBDPrecSolve): hR, hZ host arrays [nsys][n] by list position; the device function the solve kernels call */
int idahip_krylov_psolve(idahip_ctx* ctx, const double* hR, double* hZ, const int32_t* hIdx, int nsys);
/* The factors of one system in idahip_download_lu_band's format (hAB: ldab*n doubles, hPiv: n pivots, 0-based rows). Upload is the
 * user-supplied preconditioner: any non-singular factored band matrix of the ctx's widths is a valid P; pivots outside
 * j <= piv[j] <= min(n-1, j+ml) are refused. */
int idahip_krylov_download_prec(idahip_ctx* ctx, int sys, double* hAB, int64_t* hPiv);
int idahip_krylov_upload_prec(idahip_ctx* ctx, int sys, const double* hAB, const int64_t* hPiv);
/* `count` HIP streams on `device` for contexts that are to work SIDE BY SIDE (idaens_stream_group, ida_ensemble.h). The HIP
 * runtime maps its streams onto a few hardware queues as it sees fit, and two streams on one queue take turns; this call
 * creates streams and keeps those a probe kernel shows to run concurrently with every stream kept before. streams_out[count]
 * receives hipStream_t handles for idahip_create's hip_stream argument (the caller keeps ownership: idahip_release_streams
 * after the contexts are destroyed); *nconcurrent (optional) = how many of them, from the front, are mutually concurrent --
 * less than count when the runtime offers fewer hardware queues (GPU_MAX_HW_QUEUES, 4 by default). */
int idahip_concurrent_streams(int device, int count, void** streams_out, int* nconcurrent);
int idahip_release_streams(int device, int count, void** streams);
/* Diagnostic: how evenly the device shares itself between two streams whose kernels each want the whole chip -- *frac = the part
 * of two probe grids' joint span in which both had workgroups running (about 1: the dispatcher interleaves them; about 0.5: the
 * second grid's workgroups only start when the first's are all out). */
int idahip_stream_pair_share(int device, void* streamA, void* streamB, double* frac);
const char* idahip_last_error(const idahip_ctx* ctx);
int idahip_sync(idahip_ctx* ctx);
int idahip_n(const idahip_ctx* ctx);
int idahip_batch(const idahip_ctx* ctx);
int idahip_kind(const idahip_ctx* ctx); /* the idahip_problem the ctx was created with */

/* TolControlSS (natol == 1) / TolControlSV (natol == n), src/tol_control.rs:6-82; shared by the ensemble */
int idahip_set_tolerances(idahip_ctx* ctx, double rtol, const double* hAtol, int natol);
/* C IDA's IDASetId: hId[i] = 1.0 marks component i as differential, 0.0 as algebraic (any other value: -2); shared by the
 * ensemble, as the tolerances are; NULL clears it. Read by idahip_ic_trial / idaens_calc_ic with IDAHIP_IC_YA_YDP, and by the masked
 * error norms (idahip_set_suppress_alg, idahip_wrms_masked). */
int idahip_set_id(idahip_ctx* ctx, const double* hId /* [n] or NULL */);
/* 1 if an id is set (hId, when non-null, receives it), 0 if not, -1 for a null ctx */
int idahip_id(const idahip_ctx* ctx, double* hId);
/* C IDA's IDASetSuppressAlg, the reference's ida_suppressalg (src/lib.rs:138, no setter there): on != 0 masks the LOCAL ERROR norms
 * of the stepper with the id vector -- per element p = (x_i w_i) m_i with m_i = 1.0 where id_i != 0 and 0.0 elsewhere, the p p added
 * left to right from 0.0 by one lane, divided by the FULL n, then the square root (src/norm_rms.rs:49-57; a non-finite masked element
 * still makes the norm NaN). Default off. The switch belongs to the ctx, as id and the constraints do, is shared by the ensemble and
 * is read at the start of every call, so it may change between solve calls. Masked when on -- every norm the reference passes
 * ida_suppressalg to: ypnorm and ||phi[0]|| of idahip_init_first, the four sums of idahip_post_newton / _post_newton_constr,
 * ||phi[0]|| of idahip_complete_step, and the same sums inside idahip_tiny_solve / idahip_round_solve. Never masked: Newton's delnrm
 * (idahip_newton_iter, _iter2, _iter_krylov), the constraint correction's norm, SPGMR's norms, DQ increments, idahip_wrms and
 * everything of the idahip_ic_* calls. With the switch off every kernel does exactly what it did without it.
 * Refused (-2 with a text, nothing launched): the calls above with the switch on and no id set (C IDA's IDA_MISSING_ID), and
 * idaens_calc_ic with the switch on: the supported order is idahip_set_id, idaens_calc_ic, idahip_set_suppress_alg(ctx, 1), solve. */
int idahip_set_suppress_alg(idahip_ctx* ctx, int on);
/* 1 on, 0 off, -1 for a null ctx */
int idahip_suppress_alg(const idahip_ctx* ctx);
/* C IDA's IDASetConstraints (the reference has none; DESIGN.md section 4g is the definition): hC[i] = 0.0 no constraint on component
 * i, 1.0: y_i >= 0, -1.0: y_i <= 0, 2.0: y_i > 0, -2.0: y_i < 0; any other value: -2. Shared by the ensemble, as the tolerances are;
 * NULL clears it; an all-zero vector counts as set (the check runs and always passes). Read by idahip_post_newton_constr,
 * idahip_constr_check, the one-thread-per-system device stepper and libidaens' host stepper. Component i of a vector y is VIOLATED iff
 * (|c_i| > 1.5 and y_i*c_i <= 0) or (|c_i| > 0.5 and y_i*c_i < 0); a NaN violates nothing. Not supported together with
 * difference-quotient Jacobians (idahip_tiny_solve returns -2, libidaens refuses every solve call), by idahip_round_solve (-2) and by
 * idaens_calc_ic (refused). */
int idahip_set_constraints(idahip_ctx* ctx, const double* hC /* [n] or NULL = clear */);
/* 1 if constraints are set (hC, when non-null, receives them), 0 if not, -1 for a null ctx */
int idahip_constraints(const idahip_ctx* ctx, double* hC);
/* per-system problem parameters, systems [first, first+count): LORENZ63 [count][3], HEAT1D [count][1], BRUSS1D [count][5],
 * MASS_ACTION [count][nreac] (idahip_set_rate_network: [count][nreac + nconst]) */
int idahip_set_problem_params(idahip_ctx* ctx, int first, int count, const double* hParams, int nparam);
/* IDAHIP_MASS_ACTION: the network, once per ctx, after idahip_create and before anything evaluates the problem. reactants
 * [nreac][3], rows / reacs / nu [nentries], d [n] as defined above. Everything is validated -- index ranges, -1 only in trailing
 * slots, finite nu and d, nreac >= 1 --: a bad input is refused with -2 and a text that names the first offending item, and
 * nothing is changed; so is a ctx of another kind, and a second call. Builds and uploads the row-CSR of the residual and the CSR
 * of the Jacobian's pattern, and allocates the rate constants [batch][nreac] (all 0.0 until idahip_set_problem_params). */
int idahip_set_mass_action(idahip_ctx* ctx, int nreac, const int32_t* reactants /*[nreac][3]*/, int nentries, const int32_t* rows,
                           const int32_t* reacs, const double* nu, const double* d /*[n]*/);
/* The same with rate laws (defined above), instead of idahip_set_mass_action: once per ctx across the two setters. factors [nfac][5] =
 * (reaction, op, species, constant, exponent), in any order of reactions; the factors of one reaction keep the caller's order.
 * nconst >= 0 constants per system follow the rate constants (nparam = nreac + nconst); a constant no factor uses is allowed.
 * Validated as above, and: every factor's reaction, op, species, constant and exponent range, at most 4 factors per reaction.
 * With nfac = 0 and nconst = 0 it is idahip_set_mass_action. */
int idahip_set_rate_network(idahip_ctx* ctx, int nreac, const int32_t* reactants /*[nreac][3]*/, int nfac, const int32_t* factors /*[nfac][5]*/,
                            int nconst, int nentries, const int32_t* rows, const int32_t* reacs, const double* nu, const double* d /*[n]*/);
/* the pattern of the network's Jacobian: its positions (*nnz) and half-bandwidths (*ml = max i - j, *mu = max j - i); any pointer
 * may be null. -2 on a ctx of another kind and before idahip_set_mass_action. */
int idahip_mass_action_pattern(idahip_ctx* ctx, int* nnz, int* ml, int* mu);
/* The analytic Jacobian of one system at the ctx-resident yy, to host memory -- for tests/inspection, as idahip_download_lu: hJ [n*n]
 * column-major, every position outside the pattern +0.0. The kernel of idahip_nls_lsetup launched for one system into a buffer of its
 * own: the ctx's work matrices and factors are left alone. */
int idahip_mass_action_jac(idahip_ctx* ctx, int sys, double cj, double* hJ);
/* A network of n <= 8 species on the ONE-THREAD STEPPER (idahip_tiny_solve below). Off by default: with the switch off nothing
 * changes -- idahip_tiny_solve refuses the ctx and libidaens steps it on the host stepper. With it on, idahip_tiny_solve takes the ctx
 * (polynomial or with rate laws; analytic or difference-quotient Jacobians; roots, constraints, idaens_stream as for the built-in
 * kinds) and libidaens' device controller runs it there: a whole solve call in one launch, one thread per system interpreting the
 * network's tables. Per system the operations, their order and every counter are the host stepper's.
 * idahip_set_mass_action_tiny returns -2 with a text (and changes nothing) on a ctx of another kind, for n > 8 and on a band or
 * Krylov ctx. It may be called before or after the network is set, and between solve calls.
 * idahip_mass_action_tiny: 1 on, 0 off, -1 for a null ctx. */
int idahip_set_mass_action_tiny(idahip_ctx* ctx, int on);
int idahip_mass_action_tiny(const idahip_ctx* ctx);
/* LINEAR_DENSE data, systems [first, first+count): hA, hB [count][n*n] column-major, hC [count][n] */
int idahip_set_linear_dense(idahip_ctx* ctx, int first, int count, const double* hA, const double* hB, const double* hC);
/* IDAHIP_HOST_CALLBACK: the problem's callbacks (both required) and the pointer handed back to them */
int idahip_set_host_problem(idahip_ctx* ctx, idahip_res_fn res, idahip_jac_fn jac, void* user);
/* state movement: field of systems [first, first+count) <-> host [count][n] */
int idahip_upload(idahip_ctx* ctx, idahip_field f, int first, int count, const double* h);
int idahip_download(idahip_ctx* ctx, idahip_field f, int first, int count, double* h);
/* factored Jacobian of one system (column-major n*n), its pivots and the zero-pivot flag -- for tests/inspection */
int idahip_download_lu(idahip_ctx* ctx, int sys, double* hLU, int64_t* hPiv);

/* raw device memory for the stand-alone solver calls below (so callers need no HIP runtime of their own) */
void* idahip_dev_alloc(idahip_ctx* ctx, size_t bytes);
int idahip_dev_free(idahip_ctx* ctx, void* d);
int idahip_memcpy_h2d(idahip_ctx* ctx, void* d, const void* h, size_t bytes);
int idahip_memcpy_d2h(idahip_ctx* ctx, void* h, const void* d, size_t bytes);

/* ---- LSolver trait (crates/linear/src/traits.rs:27-91) on caller-owned device buffers [batch][n*n], [batch][n] ----
 * setup  = Dense::setup  -> dense_get_rf (crates/linear/src/dense.rs:38-44, 86-158): in-place PA = LU, pivots out;
 *          hInfo[s] = 0 | 1-based zero-pivot column (linear::Error::LUFactFail{col}, crates/linear/src/lib.rs:11-12).
 * solve  = Dense::solve  -> x <- b; dense_get_rs (dense.rs:46-63, 165-206). `tol` is ignored by a direct solver.   */
int idahip_ls_setup(idahip_ctx* ctx, double* dA, int64_t* dPiv, int32_t* hInfo, const int32_t* hIdx, int nsys);
int idahip_ls_solve(idahip_ctx* ctx, const double* dLU, const int64_t* dPiv, double* dX, const double* dB, double tol,
                    const int32_t* hIdx, int nsys);
/* LSolver::get_type (crates/linear/src/traits.rs:36-38, LSolverType: crates/linear/src/lib.rs:15-20): what idaLsSolve branches on
 * (src/ida_ls.rs:316-329, 387-410: the tolerance handed to the solver, which vector is copied to b, whether the 2/(1+cjratio)
 * scaling applies, the nli / ncfl counters). This library's solver is the dense direct one: IDAHIP_LS_DIRECT, no iterations,
 * no residual norm (Dense::num_iters / res_norm, traits.rs:82-90); the host stepper's bookkeeping takes the type from here. */
typedef enum { IDAHIP_LS_DIRECT = 0, IDAHIP_LS_ITERATIVE = 1, IDAHIP_LS_MATRIX_ITERATIVE = 2 } idahip_ls_kind;
int idahip_ls_type(const idahip_ctx* ctx);
int idahip_ls_num_iters(const idahip_ctx* ctx);
double idahip_ls_res_norm(const idahip_ctx* ctx);
/* NormRms::norm_wrms (src/norm_rms.rs:31-38): hOut[s] = sqrt(sum_i (x_i w_i)^2 / n), summed left to right */
int idahip_wrms(idahip_ctx* ctx, const double* dX, const double* dW, double* hOut, const int32_t* hIdx, int nsys);
/* the masked variant (src/norm_rms.rs:49-57) with the ctx's id as the mask: hOut[s] = sqrt(sum_i ((x_i w_i) m_i)^2 / n), m_i = 1.0 where
 * id_i != 0, 0.0 elsewhere. It does not look at idahip_set_suppress_alg; without an id it is refused (-2). */
int idahip_wrms_masked(idahip_ctx* ctx, const double* dX, const double* dW, double* hOut, const int32_t* hIdx, int nsys);

/* IdaNLProblem::sys immediately followed by IdaNLProblem::setup for the same systems -- the order Newton::solve runs them
 * in when call_lsetup is set (crates/nonlinear/src/newton.rs:73-96; src/ida_nls.rs:118-188). Same results as
 * idahip_nls_sys + idahip_nls_lsetup; for the linear dense problem the residual pass also forms J = B + cj*A, so A and B are
 * read once instead of twice. hInfo / return value as idahip_nls_lsetup. */
int idahip_nls_sys_setup(idahip_ctx* ctx, const double* hTn, const double* hCj, int reset_ee, int32_t* hInfo,
                         const int32_t* hIdx, int nsys);

/* ---- NLProblem trait as implemented by IdaNLProblem (src/ida_nls.rs:118-266), on the ctx-resident state ----
 * sys    = idaNlsResidual (:118-153): yy = yypredict + ycor; yp = yppredict + cj*ycor; delta = savres = F(tn,yy,yp).
 *          ycor is the accumulated correction `ee` (Newton's y); reset_ee != 0 first sets ee = 0 (Newton's y <- y0 = 0,
 *          crates/nonlinear/src/newton.rs:75,93).
 * lsetup = idaNlsLSetup (:156-187) + idaLsSetup (src/ida_ls.rs:232-290): J <- 0; jac(tn, cj, yy, yp, res); LU(J).
 *          hInfo[s] = 0 | 1-based zero-pivot column (recoverable). The caller resets cjold/cjratio/ss as :177-179.
 * newton_iter = one pass of the Newton loop body (newton.rs:98-110): delta = -delta; idaNlsLSolve (src/ida_nls.rs:190,
 *          src/ida_ls.rs:298-455: getrs, then delta *= hScale[s] with hScale = 2/(1+cjratio), or 1.0 when cjratio == 1);
 *          ee += delta; hDelnrm[s] = ||delta||_wrms(ewt) for idaNlsConvTest (:218-266), which the host evaluates
 *          (its `powf` must be the platform libm's).                                                   */
int idahip_nls_sys(idahip_ctx* ctx, const double* hTn, const double* hCj, int reset_ee, const int32_t* hIdx, int nsys);
int idahip_nls_lsetup(idahip_ctx* ctx, const double* hTn, const double* hCj, int32_t* hInfo, const int32_t* hIdx, int nsys);

/* ---- Difference-quotient Jacobians: C IDA's idaLsDenseDQJac (dense ctx) and idaLsBandDQJac (band ctx) ----
 * With the mode on, every Jacobian the ctx forms -- idahip_nls_lsetup_dq, the device steppers, libidaens -- is a DQ one, for every
 * problem kind; with it off (the default) nothing changes. The definition (SUNDIALS ida_ls.c), at the ctx's yy, yp, ewt and
 * rr = savres (the residual at tn that idahip_nls_sys left), with srur = sqrt(DBL_EPSILON), MAX(a, b) = a > b ? a : b:
 *   inc_j = MAX(srur * MAX(|yy_j|, |hh*yp_j|), 1/ewt_j);  if (hh*yp_j < 0) inc_j = -inc_j;  inc_j = (yy_j + inc_j) - yy_j;
 *   column j perturbed: yy_j + inc_j, yp_j + cj*inc_j.
 *   dense: one residual rtemp per column; J(:,j) = N_VLinearSum(1/inc_j, rtemp, -1/inc_j, rr) (the serial vector's case order:
 *          rtemp - rr for 1/inc = 1, rr - rtemp for -1, (1/inc)*(rtemp + rr) for +-0, (1/inc)*(rtemp - rr) otherwise).
 *   band:  width = ml + mu + 1; group g < min(width, n) perturbs every column j = g (mod width) at once and takes one residual;
 *          J(i,j) = (1/inc_j)*(rtemp_i - rr_i) for max(0, j-mu) <= i <= min(n-1, j+ml); every other band entry +0.0.
 * A dense DQ Jacobian costs n residual evaluations, a band one min(width, n); libidaens counts them in IDAENS_C_NRE_DQ (C IDA's
 * nreDQ), not in nre. The heat kernel writes, on a dense ctx, only rows j-1..j+1 of column j, as its analytic kernel does:
 * entries that the definition gives as -0.0 there are +0.0. The Brusselator kernel does the same with rows j-2..j+2. Constraints flip inc's sign in C IDA; here a ctx with both constraints
 * (idahip_set_constraints) and DQ Jacobians is refused by the steppers instead.
 * A DQ ctx refuses idahip_nls_lsetup and idahip_nls_sys_setup (-2: they carry no step sizes); idahip_nls_lsetup_dq is
 * idahip_nls_lsetup with them, and returns -2 on a ctx without DQ. */
int idahip_set_jacobian_dq(idahip_ctx* ctx, int on);
int idahip_jacobian_dq(const idahip_ctx* ctx);  /* 1 on, 0 off */
/* IDAHIP_HOST_CALLBACK, dense or band ctx: a residual and no Jacobian. Turns DQ on: idahip_set_jacobian_dq(ctx, 0) then returns
 * -2, until idahip_set_host_problem / idahip_set_host_band_problem registers a Jacobian again (which leaves the mode as it is). */
int idahip_set_host_residual(idahip_ctx* ctx, idahip_res_fn res, void* user);
int idahip_nls_lsetup_dq(idahip_ctx* ctx, const double* hTn, const double* hCj, const double* hHh, int32_t* hInfo, const int32_t* hIdx,
                         int nsys);
/* The DQ Jacobian of the listed systems at the ctx-resident state, to host memory: hJ [nsys][n*n] column-major, or on a band ctx
 * [nsys][ldab*n] in the band storage of idahip_download_lu_band. Works whatever the mode (a check of an analytic Jacobian);
 * leaves the ctx's work matrices and factors alone. */
int idahip_jac_dq(idahip_ctx* ctx, const double* hTn, const double* hCj, const double* hHh, double* hJ, const int32_t* hIdx, int nsys);
int idahip_newton_iter(idahip_ctx* ctx, const double* hScale, double* hDelnrm, const int32_t* hIdx, int nsys);
/* The first two iterations of Newton::solve in one call, without the host in between (first slice):
 *   newton body (m = 0) -> idaNlsConvTest -> NLProblem::sys -> newton body (m = 1) -> idaNlsConvTest
 * for the listed systems, each of which must be at curiter = 0 with its residual in `delta` (i.e. right after idahip_nls_sys
 * or idahip_nls_sys_setup). The two tests need no powf (m = 0: two comparisons; m = 1: rate = delnrm / oldnrm exactly,
 * src/ida_nls.rs:243-262), so they are decided on the device with the caller's per-system hToldel, hSs, hEpsNewt; a system
 * that has ended is skipped by the kernels that follow. Out: hDelnrm[s][0..2) = the norms of the two corrections (the second
 * is 0 if not run), hConv[s] = 0 go on with m = 2 (NLProblem::sys first) | 1 converged at m = 0 | 2 converged at m = 1 |
 * 3 ConvergenceRecover at m = 1. The caller updates oldnrm = hDelnrm[s][0] and, if the second iteration ran and did not end
 * in 3, ss = rate / (1 - rate) with rate = hDelnrm[s][1] / hDelnrm[s][0]. Not for IDAHIP_HOST_CALLBACK. */
int idahip_newton_iter2(idahip_ctx* ctx, const double* hScale, const double* hTn, const double* hCj, const double* hToldel,
                        const double* hSs, const double* hEpsNewt, double* hDelnrm, int32_t* hConv, const int32_t* hIdx, int nsys);

/* ---- vector parts of the stepper that touch the same device-resident state ----
 * init_first : initial_setup + first-call block of Ida::solve (src/lib.rs:537-545, src/impl_solve.rs:120-126):
 *              ewt = ewt_set(phi[0]); hYpnorm[s] = ||phi[1]||_wrms(ewt); hPhi0Nrm[s] = ||phi[0]||_wrms(ewt) (the first
 *              tolsf test, impl_solve.rs:289-295).
 * scale_phi1 : phi[1] *= hFac[s]   (phi[1] = hh*y', impl_solve.rs:167-168; reset() after a failed first step)
 * predict    : set_coeffs' phi-star scaling phi[j] *= beta[j], j = ns..kk (lib.rs:768-779) followed by IDAPredict
 *              (lib.rs:894-959). hKkNs [nsys][2], hBeta/hGamma [nsys][6].
 * post_newton: yy = yypredict + ee; yp = yppredict + cj*ee (lib.rs:845-849) and the four norms the error test /
 *              order selection may need (lib.rs:983-1004, impl_complete_step.rs:74-77):
 *              hNorms[s] = { ||ee||, ||ee+phi[kk]||, ||ee+phi[kk]+phi[kk-1]||, ||ee-phi[kk+1]|| } (0 where undefined).
 * restore    : IDARestore's phi part, phi[j] *= cvals[j-ns], j = ns..kk (lib.rs:1057-1082). hCvals [nsys][6].
 * complete_step: phi[kused+1] = ee (if kused < maxord), the phi recurrence (impl_complete_step.rs:152-176), ee *= ck
 *              (lib.rs:708), then the next step's ewt_set(phi[0]) and tolsf norm (impl_solve.rs:266-295):
 *              hPhi0Nrm[s] = ||phi[0]||_wrms(ewt), hEwtBad[s] != 0 if some ewt component <= 0 (a NaN is not).
 * get_solution: IDAGetSolution's linear combinations (lib.rs:1319-1340). hCvals [nsys][6], hDvals [nsys][5].       */
int idahip_init_first(idahip_ctx* ctx, double* hYpnorm, double* hPhi0Nrm, const int32_t* hIdx, int nsys);
int idahip_scale_phi1(idahip_ctx* ctx, const double* hFac, const int32_t* hIdx, int nsys);
int idahip_predict(idahip_ctx* ctx, const int32_t* hKkNs, const double* hBeta, const double* hGamma, const int32_t* hIdx, int nsys);
int idahip_post_newton(idahip_ctx* ctx, const double* hCj, const int32_t* hKk, double* hNorms, const int32_t* hIdx, int nsys);
int idahip_restore(idahip_ctx* ctx, const int32_t* hKkNs, const double* hCvals, const int32_t* hIdx, int nsys);
/* idahip_post_newton with the constraint check of an attempt between the final yy / yp and the norms, in one
 * launch; a ctx with constraints only (-2 otherwise). For a listed system s with hCheck[s] != 0 (its Newton solve succeeded):
 *   - no component of yy violated: hFlag[s] = 0, everything as idahip_post_newton;
 *   - otherwise v_i = yy_i - 0.1*((a_i*c_i)/ewt_i) for the violated i (a_i = 1 for |c_i| = 2, else 0), v_i = +0.0 elsewhere, and
 *     vnorm = ||v||_wrms(ewt), summed left to right, sqrt and comparison on the device:
 *       vnorm <= hEpsNewt[s]: hFlag[s] = 1; ee_i -= v_i for the violated i only; the four norms are those of the corrected ee;
 *                             yy and yp keep their uncorrected values;
 *       otherwise:            hFlag[s] = 2; hRr[s] = fmax(0.9*q, 0.1) with q the minimum of phi[0]_i / (phi[0]_i - yy_i) over the
 *                             violated i with phi[0]_i != yy_i (DBL_MAX when there is none); ee is left alone, hNorms[s] = 0.
 * hRr[s] = 0 unless hFlag[s] = 2. hCheck[s] == 0 skips the check: that system's results are idahip_post_newton's, bit for bit,
 * with hFlag[s] = 0. A NaN in phi[0] or ewt is outside the definition. */
int idahip_post_newton_constr(idahip_ctx* ctx, const double* hCj, const int32_t* hKk, const double* hEpsNewt, const int32_t* hCheck,
                              double* hNorms, int32_t* hFlag, double* hRr, const int32_t* hIdx, int nsys);
/* The constraint mask of one field: hViolated[s] = 1 if a component of `field` of listed system s is violated, else 0 (the start of
 * an integration checks IDAHIP_F_PHI0). A ctx with constraints only (-2 otherwise). */
int idahip_constr_check(idahip_ctx* ctx, idahip_field field, int32_t* hViolated, const int32_t* hIdx, int nsys);
int idahip_complete_step(idahip_ctx* ctx, const int32_t* hKused, const double* hCk, int maxord, double* hPhi0Nrm,
                         int32_t* hEwtBad, const int32_t* hIdx, int nsys);
int idahip_get_solution(idahip_ctx* ctx, const int32_t* hKord, const double* hCvals, const double* hDvals,
                        const int32_t* hIdx, int nsys);
/* IDAGetDky (src/lib.rs:424-529), the vector part: hOut[s][0..n) = sum_{j = hKfirst[s] .. hKlast[s]} hCjk[s][j] * phi[j] of
 * listed system s, accumulated from zero in ascending j (lib.rs:517-526). The coefficients c_j^(k)(t) (lib.rs:464-508) are
 * the host's (libidaens: idaens_get_dky); 0 <= kfirst <= klast <= 5. hOut is a host array [nsys][n]. */
int idahip_get_dky(idahip_ctx* ctx, const int32_t* hKfirst, const int32_t* hKlast, const double* hCjk /*[nsys][6]*/, double* hOut,
                   const int32_t* hIdx, int nsys);

/* Ida::new again for some systems of a running ensemble (src/lib.rs:278-405: phi[0] = yy = y0, phi[1] = yp = y0'):
 * idahip_snapshot_initial keeps a device copy of the current phi[0], phi[1] of every system (call it right after the
 * initial conditions were uploaded); idahip_restore_initial puts the listed systems back to it. */
int idahip_snapshot_initial(idahip_ctx* ctx);
int idahip_restore_initial(idahip_ctx* ctx, const int32_t* hIdx, int nsys);
/* Ida::new with new values for the listed systems, in the middle of a run (C IDA's IDAReInit, the vector part; libidaens:
 * idaens_reinit). add == 0: hYY0 / hYP0 are host arrays [nsys][n] by list position, both required, the new y0 / y0'. add != 0: the
 * new values are the system's current device yy / yp (what a returned system reported) plus the packed increment, one IEEE
 * addition per component; either pointer may be NULL and that side is then taken as it is (no + 0.0, a -0.0 stays). For every
 * listed system phi[0] = yy = y0, phi[1] = yp = y0', phi[2..5] = +0.0, and where idahip_snapshot_initial has been taken the
 * snapshot's rows follow, so that a later idahip_restore_initial starts from the new values. The ctx's own per-system marks (a
 * Krylov ctx's npe / nps of the lock-step rounds, the band preconditioner's "has factors") return to a created system's. Systems
 * not listed are not touched. Every ctx form; no matrix is read or written. The list rules are those of every listed entry point. */
int idahip_reinit(idahip_ctx* ctx, const int32_t* hIdx, int nsys, const double* hYY0, const double* hYP0, int add);

/* ---- Consistent initial conditions: the device side of C IDA's IDACalcIC (the reference has none) ----
 * The Newton / line-search state machine of DESIGN.md section 4f runs per system on the host (libidaens: idaens_calc_ic); these are
 * its batched vector steps, for any problem kind, on a dense or a band ctx, with analytic or DQ Jacobians. They run before the first
 * step of the listed systems and keep the iterate (y0, y0') in phi[2], phi[3], delnew in phi[4] and the direction in `delta`;
 * phi[0], phi[1] hold the guess until idahip_ic_commit. Norms come back as sqrt(sum / n) with the sum taken left to right.
 *   begin : ewt = ewt_set(phi[0]), hEwtBad[s] != 0 if a component is <= 0; hYpnorm[s] = ||phi[1]||_wrms(ewt); iterate = (phi[0], phi[1])
 *   reset : iterate = (phi[0], phi[1])
 *   res   : yy, yp = the iterate; delta = savres = F(tn, yy, yp)
 *   setup : yy, yp = the iterate; delta = savres; J = dF/dy + cj dF/dy' there, factored with the ctx's LU (hInfo / return value as
 *           idahip_nls_lsetup); _dq: the DQ Jacobian of a DQ ctx with hh = hHh[s] and rr = savres (-2 on the wrong kind of ctx, as
 *           idahip_nls_lsetup / idahip_nls_lsetup_dq)
 *   solve : delta = J^-1 delta (getrs, no scaling); hFnorm[s] = ||delta||_wrms(ewt)
 *   trial : the line search's trial point into yy, yp -- with IDAHIP_IC_YA_YDP, id_i == 1: y_i = y0_i, y'_i = y0'_i - (cj*lambda)*delta_i;
 *           every other component, and every component with IDAHIP_IC_Y: y_i = y0_i - lambda*delta_i, y'_i = y0'_i --; savres = F
 *           there; delnew = J^-1 savres; hFnormp[s] = ||delnew||_wrms(ewt). One launch for the built-in problems on a dense ctx, two on
 *           a band ctx; a host-callback residual is called on the host as in idahip_nls_sys. IDAHIP_IC_YA_YDP needs idahip_set_id.
 *   accept: iterate y = yy, with IDAHIP_IC_YA_YDP also iterate y' = yp; delta = delnew
 *   commit: ewt = ewt_set(iterate y), hEwtBad as in begin; phi[0] = yy = iterate y, phi[1] = yp = iterate y' */
typedef enum { IDAHIP_IC_YA_YDP = 1, IDAHIP_IC_Y = 2 } idahip_icopt;
int idahip_ic_begin(idahip_ctx* ctx, double* hYpnorm, int32_t* hEwtBad, const int32_t* hIdx, int nsys);
int idahip_ic_reset(idahip_ctx* ctx, const int32_t* hIdx, int nsys);
int idahip_ic_res(idahip_ctx* ctx, const double* hTn, const double* hCj, const int32_t* hIdx, int nsys);
int idahip_ic_setup(idahip_ctx* ctx, const double* hTn, const double* hCj, int32_t* hInfo, const int32_t* hIdx, int nsys);
int idahip_ic_setup_dq(idahip_ctx* ctx, const double* hTn, const double* hCj, const double* hHh, int32_t* hInfo, const int32_t* hIdx,
                       int nsys);
int idahip_ic_solve(idahip_ctx* ctx, double* hFnorm, const int32_t* hIdx, int nsys);
int idahip_ic_trial(idahip_ctx* ctx, int icopt, const double* hTn, const double* hCj, const double* hLambda, double* hFnormp,
                    const int32_t* hIdx, int nsys);
int idahip_ic_accept(idahip_ctx* ctx, int icopt, const int32_t* hIdx, int nsys);
int idahip_ic_commit(idahip_ctx* ctx, int32_t* hEwtBad, const int32_t* hIdx, int nsys);

/* ---- device-resident stepper for small systems (n <= 8: IDAHIP_ROBERTS / IDAHIP_LORENZ63, and an IDAHIP_MASS_ACTION ctx with
 * idahip_set_mass_action_tiny on) ----
 * The whole of Ida::solve (src/impl_solve.rs:69-376: first-call block, loop-top checks, Ida::step with its attempt loop,
 * Newton::solve, error test, complete_step, stop tests and the interpolation to tout), for every system of the ctx, in ONE
 * launch: one thread per IVP runs its own time loop, the step-size and order controller included. The
 * controller is the same source as libidaens' host stepper (rust-ida_amd/host/ida_controller.hpp) compiled for the device
 * with a pow that reproduces glibc's bits (rust-ida_amd/csrc/glibc_pow.hpp).
 *   hSys       [batch] controller states (idactl::SysCore of ida_controller.hpp, sys_bytes = sizeof of it), in and out
 *   call       the schedule and the limits of this call (what idaens_solve / _solve_schedule / _stream take)
 *   hRoundsDone[batch] out: step-attempt rounds each system took part in
 *   hAcc       [2] out: Newton iterations of the integrations retired by `recycle`, number of those integrations
 *   hYout/hYPout optional raw dumps [ntout][batch][n] of the device-side output slots (a slot is written when its tout is
 *              reached; the caller knows from the states which slots are new)
 * idahip_pow_batch: the controller's pow for n argument pairs, computed on the device (test hook for glibc_pow.hpp). */
/* Root finding on the device (src/impl_r_check.rs:32-576) for the function family of the reference's own example,
 * g_i(t, y, y') = y[comp[i]] - threshold[i] (examples/roberts.rs:53-56): per-system state of `Ida`'s root fields
 * (ida_glo, ida_ghi, ida_grout, ida_iroots, ida_gactive: src/lib.rs:225-244), moved with the controller record. */
#define IDAHIP_MAX_ROOTS 4
typedef struct idahip_root_state {
    double glo[IDAHIP_MAX_ROOTS], ghi[IDAHIP_MAX_ROOTS], grout[IDAHIP_MAX_ROOTS], iroots[IDAHIP_MAX_ROOTS];
    int32_t gactive[IDAHIP_MAX_ROOTS];
} idahip_root_state;
typedef struct idahip_tiny_call {
    const double* touts; /* [ntout] host */
    int ntout;
    int recycle;         /* idaens_stream: a system that finished its schedule is created anew and starts over */
    int resume;          /* continuing a round-limited schedule call: idle systems have finished */
    long max_rounds;     /* step attempts per system in this launch; 0 = until every system has returned */
    long mxstep;
    int maxord;
    long maxnef, maxncf;
    double epcon, hmax_inv, t0;
    const int64_t* start_round; /* [batch] host or NULL: idaens_stream's staggered start (absolute round numbers) */
    int64_t round_base;         /* rounds executed before this call */
    int nroots;                 /* 0, or the number of root functions (<= IDAHIP_MAX_ROOTS) */
    const int32_t* root_comps;  /* [nroots] host */
    const double* root_thresholds; /* [nroots] host */
    idahip_root_state* root_states; /* [batch] host, in and out (NULL iff nroots == 0) */
} idahip_tiny_call;
int idahip_tiny_solve(idahip_ctx* ctx, void* hSys, size_t sys_bytes, const idahip_tiny_call* call, int64_t* hRoundsDone, uint64_t* hAcc,
                      double* hYout, double* hYPout);
int idahip_pow_batch(idahip_ctx* ctx, const double* hX, const double* hY, double* hOut, size_t count);
/* The same call for larger systems (8 < n <= 4096, IDAHIP_LINEAR_DENSE, IDAHIP_HEAT1D, IDAHIP_BRUSS1D or IDAHIP_MASS_ACTION, LU variant 4) as LOCK-STEP ROUNDS driven from the
 * device side: a round = one step attempt of every stepping system (Ida::step's attempt loop body, src/lib.rs:613-711, with
 * Newton::solve, crates/nonlinear/src/newton.rs:51-167, and the batched kernels of this library inside), the controller
 * state of every system and the index lists live on the device, the host only enqueues each round's fixed launch sequence:
 * one synchronisation per round (to learn whether any system still steps), none at all when `recycle` is set (throughput
 * mode runs exactly max_rounds rounds). Arguments as idahip_tiny_solve; rounds_run: rounds executed by this call.
 * A Krylov ctx is refused (-2) unless idahip_set_krylov_rounds is on (above). */
int idahip_round_solve(idahip_ctx* ctx, void* hSys, size_t sys_bytes, const idahip_tiny_call* call, int64_t* hRoundsDone, uint64_t* hAcc,
                       double* hYout, double* hYPout, int64_t* rounds_run);

/* LU implementation choice. Both variants are bit-identical to dense_get_rf; they factor in 64-column
 * super-panels with a rank-64 trailing update in wave-private 16-row strips and differ in how a super-panel is factored:
 *   4 = default: one wavefront per matrix factors the whole super-panel (<= 512 live rows);
 *   3 = two 32-column panels with two rows per lane and a narrow update between them (the cross-check in the tests, and what
 *       the leading super-panels of matrices with more than 512 rows use; more than 1024 rows: 8-column panels).
 * Any other value is refused. (Round 2's variant 5, the same kernels with FMA-contracted updates, is gone: DESIGN.md.) */
int idahip_set_lu_variant(idahip_ctx* ctx, int variant);
int idahip_lu_variant(const idahip_ctx* ctx); /* the variant in force */
/* IDAHIP_LINEAR_DENSE with analytic Jacobians, 8 < n <= 512, LU variant 4, the ctx's own work matrix and factors: where the Newton
 * matrix J = B + cj*A is formed. Inside the factorisation: the first super-panel's launches and the first trailing launch read A
 * and B and combine them as they load, the residual of the systems that set up is the plain sweep (kernel class IDAHIP_K_SYS;
 * IDAHIP_K_SYS_JAC and IDAHIP_K_JAC then count nothing) and J never passes through memory. Or outside it: by the fused residual +
 * Jacobian sweep (idahip_nls_sys_setup, idahip_round_solve) or the Jacobian kernel (idahip_nls_lsetup) into the work matrix.
 * Same expression, multiply then add: factors, pivots and every result are bit-identical either way.
 *   never set (the default): inside in idahip_round_solve (the device lock-step stepper) where 448 < n <= 512 -- the first panel is
 *                            then the eight-slot instantiation, the size the path was measured at; smaller matrices take a
 *                            first-panel kernel that reads its slot count at run time, unmeasured, and stay outside --;
 *                            idahip_nls_lsetup and idahip_nls_sys_setup -- and with the latter the host stepper -- launch the
 *                            kernels they always launched;
 *   1: inside, in all three, for every eligible n;   0: outside, in all three.
 * Turning it on is refused (-2) on a ctx that is not eligible (another kind, a band or Krylov ctx, n outside the range); a DQ ctx
 * or LU variant 3 keep the setting and use the other path while they last. The calls on caller-supplied matrices
 * (idahip_ls_setup) and the initial-condition calls are not affected. */
int idahip_set_jac_in_lu(idahip_ctx* ctx, int on);
/* What is in effect now: 0 = outside everywhere; 1 = inside in idahip_round_solve alone (never set, n > 448); 2 = inside in
 * idahip_round_solve, idahip_nls_lsetup and idahip_nls_sys_setup (set to 1). */
int idahip_jac_in_lu(const idahip_ctx* ctx);
/* Dense direct ctx, 8 < n <= 512, LU variant 4: the layout of the ctx's OWN factors (what idahip_nls_lsetup, idahip_nls_sys_setup,
 * idahip_round_solve and the initial-condition setups write and idahip_newton_iter and the initial-condition solves read).
 *   staged (1): below the diagonal block of every 64-column block column the rows of L stand in the order the factorisation's
 *               list of not-yet-pivoted rows had when the block column's super-panel was done, not in final pivot order; a map per
 *               system and super-panel says where each row went, and a solve permutes its right-hand side in LDS block by block
 *               with it. The factorisation then ends without its pass that scatters rows to their pivot positions.
 *   reference (0): every row at its pivot position (dgetrf's layout), written by that pass.
 * Pivots, Newton iterations, norms and every result are bit-identical either way: each entry of a right-hand side receives the
 * same updates in the same order. Never set: staged where 448 < n <= 512 (the size it was measured at), the reference layout
 * below; 1: staged at every eligible n; 0: the reference layout.
 * The setting describes the factors the ctx holds: after changing it (or the LU variant) every system is set up again before its
 * next solve. Turning it on is refused (-2) on a ctx that is not eligible (band, Krylov, n outside the range); with LU variant 3
 * the setting is kept and the reference layout used while that lasts.
 * idahip_download_lu returns the REFERENCE layout under either setting (the maps are composed on the host). Caller-supplied
 * matrices (idahip_ls_setup / idahip_ls_solve) are always in the reference layout; the ctx's own factors cannot reach
 * idahip_ls_solve, since no call hands out their address.
 * A system whose setup fails (info != 0): in the reference layout its previous factors stay whole (the scatter skips it); staged,
 * the launches that ran before the zero pivot was found have already overwritten part of its factors, maps and permutation, and
 * idahip_download_lu returns a mixture. Either way the system has no valid factors until a setup of it succeeds, and the steppers
 * set it up again before they solve with it. */
int idahip_set_lu_staged(idahip_ctx* ctx, int on);
/* 1 = the ctx's own factors are written and read staged now, 0 = in the reference layout. */
int idahip_lu_staged(const idahip_ctx* ctx);
/* Matrices with more than 1024 rows: how a 64-column super-panel is factored. 1 = in one launch of the left-looking
 * workgroup-per-matrix kernel (lu_superpanel_kernel): the faster pipeline for BANDED matrices in dense storage (config 4's heat
 * Jacobians: 238 against 322 us per 4096 x 4096 matrix) and the default for IDAHIP_HEAT1D and IDAHIP_BRUSS1D; 0 = eight 8-column panel launches with a
 * narrow update after each, faster on DENSE matrices (they spread the update over several workgroups per matrix) and the default for
 * every other problem kind. A hint about structure, never about results: the factors are bit-identical either way. */
int idahip_set_lu_superpanel(idahip_ctx* ctx, int on);
int idahip_lu_superpanel(const idahip_ctx* ctx); /* the setting in force */
/* Device lock-step stepper (idahip_round_solve): linear setups -- Jacobian + dense_get_rf, ida_ls.rs:232-290 -- batched over rounds.
 * With rounds = k > 1 a lock-step round sets nothing up unless at least (k - 1) / k of the systems that are stepping ask for a setup
 * (lib.rs:806-817) or k - 1 rounds in a row have waited already; a system that asks waits, its attempt begun, while the others go
 * on stepping, and a round without setups launches no factorisation at all. 1 = every round serves its setups (the default); at
 * most 64. A scheduling choice: every system performs the same attempts with the same arithmetic, so its results and counters do not
 * change (tests/test_gpu_device_controller.py). It pays where a batched factorisation costs about the same for 50 matrices as for
 * 250 -- matrices of thousands of rows, a workgroup per matrix and a long chain of launches (config 4) -- and costs throughput where
 * the factorisation's time is proportional to the batch (config 3). */
int idahip_set_lu_period(idahip_ctx* ctx, int rounds);
int idahip_lu_period(const idahip_ctx* ctx); /* the setting in force */
/* Device lock-step stepper (idahip_round_solve) on a dense direct ctx, 8 < n <= 1024: where the length of a round's list of systems
 * to factor is known when the factorisation's kernels are launched.
 *   1: on the host. The kernel that builds the list posts its length to pinned host memory, the host polls for it behind the round's
 *      first residual sweep, every LU launch of the round has exactly the workgroups it needs, and a round without setups launches
 *      neither the setups' residual sweep nor a factorisation. One host wait per round.
 *   0: on the device only. Every LU launch is sized for the whole batch and its surplus workgroups leave on reading the count; the
 *      host never waits inside a round.
 *  -1: the library's choice (the default; IDAHIP_LU_COUNT_ON_HOST=-1|0|1, read at idahip_create, sets it too).
 * Matrices with more than 1024 rows always take the host count; band and Krylov contexts never do. A scheduling choice: the
 * same kernels run on the same matrices, results and counters are bit-identical (tests/test_gpu_lu_launch_sizes.py).
 * Any other value is refused (-1). */
int idahip_set_lu_count_on_host(idahip_ctx* ctx, int on);
int idahip_lu_count_on_host(const idahip_ctx* ctx); /* what idahip_round_solve does on this ctx now: 0 or 1 */
/* The number of workgroups of the wave-per-matrix panels' second (SLOW) launches (LU variant 4, <= 512 live rows), in every call that
 * factors. They walk the list of matrices their first launch handed over -- matrices with exact zeros, NaNs or infinities;
 * normally none -- in a grid-stride loop, so that any number is correct. 0 = automatic (the default): one per listed system, and in
 * idahip_round_solve with the count on the host (n <= 1024) clamp(2 * the largest list of the last round's factorisation + 32, 32,
 * count). Tests set 1 or 2 to make every workgroup walk several entries. Negative values are refused (-1). */
int idahip_set_lu_slow_grid(idahip_ctx* ctx, int workgroups);
/* 0 for the product library. 1 for a TIMING BUILD (-DIDAHIP_TIMING_BUILD, rust-ida_amd/csrc/exp_switches.hpp): a library in
 * which parts of kernels were removed or replaced to measure what they cost -- its results are garbage by design; a caller
 * that cares (tests, bench.py) refuses to run on one. No ctx, no device needed. */
int idahip_timing_build(void);

/* ---- measurement hooks (bench.py / profiles): device time of the launches of the last call, by HIP events on the
 * ctx stream, and launch counters per kernel class ---- */
typedef enum {
    IDAHIP_K_NEWTON_ITER = 0, IDAHIP_K_SYS = 1, IDAHIP_K_JAC = 2, IDAHIP_K_LU = 3, IDAHIP_K_VECTOR = 4, IDAHIP_K_SOLVE = 5,
    IDAHIP_K_SYS_JAC = 6, /* fused residual + Jacobian pass of idahip_nls_sys_setup */
    /* single kernels of the batched LU (timing level 2 only): every launch of the kernel is bracketed by its own pair of
     * events; `systems` counts matrices x launches */
    IDAHIP_K_LU_PANEL = 7,    /* lu_wavepanel_kernel (variant 3, or more than 512 live rows: lu_panel2_kernel / lu_panelr_kernel + narrow lu_trail_kernel) */
    IDAHIP_K_LU_TRAIL = 8,    /* lu_trail64w_kernel */
    IDAHIP_K_LU_FINALIZE = 9, /* lu_finalize_kernel */
    IDAHIP_K_COUNT = 10
} idahip_kclass;
/* on = 0: no events, no synchronisation (launch counters still run); 1: device time per kernel class (one event pair and
 * one hipEventSynchronize per class call); 2: additionally per kernel of the LU (which perturbs the class figure of the
 * LU: use separate passes). */
int idahip_timing_enable(idahip_ctx* ctx, int on);
/* accumulated device milliseconds and launch count of a kernel class since the last reset */
int idahip_timing_get(idahip_ctx* ctx, idahip_kclass k, double* ms, int64_t* launches, int64_t* systems);
int idahip_timing_reset(idahip_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* IDA_HIP_H */
