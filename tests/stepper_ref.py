"""Plain float64 restatement of the stepper's vector entry points and of the Newton iteration body (include/ida_hip.h),
one system at a time, in the reference's operation order.

TEST INFRASTRUCTURE ONLY (tests/test_stepper_ref.py pins it on the oracle; tests/test_gpu_stepper_entry_points.py
compares the device with it). Elementwise numpy float64 operations are single IEEE operations (no contraction), so
each line below carries the reference's bits; every sum that feeds a norm goes through the oracle's sequential
`norm_wrms` (O.wrms) and every triangular solve through the oracle's `dense_get_rs` (O.getrs), so nothing is re-summed
in numpy's pairwise order. Arrays are never modified in place: every function returns new arrays.

  phi          [6][n]  (MXORDP1 = 6, src/constants.rs:6)
  atol         a scalar (TolControlSS) or an [n] vector (TolControlSV), src/tol_control.rs:6-82
"""
import numpy as np

import oracle_lib as O

MXORDP1 = 6
RATEMAX = 0.9  # src/ida_nls.rs:15


def _f(a):
    return np.array(a, dtype=np.float64, copy=True)


def ewt_set(y, rtol, atol):
    """TolControl::ewt_set (src/tol_control.rs:36-44, 71-82): ewt_i = 1 / (rtol |y_i| + atol_i)."""
    y = np.asarray(y, dtype=np.float64)
    at = np.broadcast_to(np.asarray(atol, dtype=np.float64), y.shape)
    return 1.0 / (rtol * np.abs(y) + at)


def init_first(phi, rtol, atol):
    """initial_setup + first-call block (src/lib.rs:537-545, src/impl_solve.rs:120-126, 289-295):
    ewt = ewt_set(phi[0]); returns (ewt, ||phi[1]||_wrms(ewt), ||phi[0]||_wrms(ewt))."""
    ewt = ewt_set(phi[0], rtol, atol)
    return ewt, O.wrms(phi[1], ewt), O.wrms(phi[0], ewt)


def scale_phi1(phi, fac):
    """phi[1] *= fac (src/impl_solve.rs:167-168; Ida::reset, src/lib.rs:1249-1252)."""
    phi = _f(phi)
    phi[1] = phi[1] * fac
    return phi


def predict(phi, kk, ns, beta, gamma):
    """set_coeffs' phi-star scaling (src/lib.rs:768-779: phi[j] *= beta[j] for j = ns..kk when ns <= kk), then IDAPredict
    (src/lib.rs:894-959): yypredict = sum_{j=0..kk} phi[j] and yppredict = sum_{j=1..kk} gamma[j] phi[j], each accumulated
    from zero in ascending j, product first. Returns (phi, yypredict, yppredict)."""
    phi = _f(phi)
    if ns <= kk:
        for j in range(ns, kk + 1):
            phi[j] = phi[j] * beta[j]
    yyp = np.zeros(phi.shape[1])
    for j in range(0, kk + 1):
        yyp = yyp + phi[j]
    ypp = np.zeros(phi.shape[1])
    for j in range(1, kk + 1):
        ypp = ypp + gamma[j] * phi[j]
    return phi, yyp, ypp


def post_newton(yypredict, yppredict, ee, ewt, phi, cj, kk):
    """The final yy / yp of nonlinear_solve (src/lib.rs:845-849) and the four norms the error test and the order selection may
    need (src/lib.rs:983-1004, src/impl_complete_step.rs:74-77), 0 where the reference computes none:
      ||ee||;  kk > 1: ||phi[kk] + ee||;  kk > 2: ||(phi[kk] + ee) + phi[kk-1]||;  kk + 1 < 6: ||ee - phi[kk+1]||.
    Returns (yy, yp, norms[4])."""
    yy = yypredict + ee
    yp = yppredict + cj * ee
    norms = np.zeros(4)
    norms[0] = O.wrms(ee, ewt)
    if kk > 1:
        d = phi[kk] + ee                 # lib.rs:992
        norms[1] = O.wrms(d, ewt)
        if kk > 2:
            d = d + phi[kk - 1]          # lib.rs:1002
            norms[2] = O.wrms(d, ewt)
    if kk + 1 < MXORDP1:
        norms[3] = O.wrms(ee - phi[kk + 1], ewt)  # impl_complete_step.rs:75
    return yy, yp, norms


def restore(phi, kk, ns, cvals):
    """IDARestore's phi part (src/lib.rs:1057-1082): phi[j] *= cvals[j - ns] for j = ns..kk, nothing when ns > kk."""
    phi = _f(phi)
    if ns <= kk:
        for j in range(ns, kk + 1):
            phi[j] = phi[j] * cvals[j - ns]
    return phi


def complete_step(phi, ee, kused, ck, maxord, rtol, atol):
    """The vector part of a successful step: phi[kused+1] = ee if kused < maxord, then tmp = ee; for j = kused..0:
    tmp += phi[j]; phi[j] = tmp (src/impl_complete_step.rs:152-176); then ee *= ck (src/lib.rs:708); then the next
    solve-loop pass's ewt = ewt_set(phi[0]), its ewt check `x <= 0` (src/impl_solve.rs:266-272: NaN is not bad) and
    ||phi[0]||_wrms(ewt) (:289-295). Returns (phi, ee, ewt, phi0nrm, ewt_bad)."""
    phi = _f(phi)
    if kused < maxord:
        phi[kused + 1] = ee
    tmp = _f(ee)
    for j in range(kused, -1, -1):
        tmp = tmp + phi[j]
        phi[j] = tmp
    ee = ee * ck
    ewt = ewt_set(phi[0], rtol, atol)
    bad = bool((ewt <= 0.0).any())
    return phi, ee, ewt, O.wrms(phi[0], ewt), bad


def get_solution(phi, kord, cvals, dvals):
    """IDAGetSolution's linear combinations (src/lib.rs:1319-1340), scaled_add from zero in ascending j:
    yy = sum_{j=0..kord} cvals[j] phi[j]; yp = sum_{j=1..kord} dvals[j-1] phi[j]. Returns (yy, yp)."""
    yy = np.zeros(phi.shape[1])
    for j in range(0, kord + 1):
        yy = yy + cvals[j] * phi[j]
    yp = np.zeros(phi.shape[1])
    for j in range(1, kord + 1):
        yp = yp + dvals[j - 1] * phi[j]
    return yy, yp


def get_dky(phi, kfirst, klast, cjk):
    """IDAGetDky's vector part (src/lib.rs:517-526): dky = sum_{j=kfirst..klast} phi[j] cjk[j], from zero in ascending j."""
    d = np.zeros(phi.shape[1])
    for j in range(kfirst, klast + 1):
        d = d + phi[j] * cjk[j]
    return d


def newton_iter(lu, piv, delta, ee, ewt, scale):
    """One pass of the Newton loop body (crates/nonlinear/src/newton.rs:98-110): delta = -delta; getrs (src/ida_ls.rs:298-455,
    crates/linear/src/dense.rs:165-206); delta *= scale (ida_ls.rs:406-410: 2 / (1 + cjratio), 1.0 when cjratio == 1);
    ee += delta; ||delta||_wrms(ewt). lu / piv: the logical factors and pivots of download_lu. Returns (delta, ee, delnrm)."""
    x = O.getrs(lu, piv, -np.asarray(delta, dtype=np.float64))
    x = x * scale
    ee = ee + x
    return x, ee, O.wrms(x, ewt)


def newton_ctest(d0, d1, toldel, ss, eps_newt):
    """The two convergence tests idahip_newton_iter2 decides on the device (src/ida_nls.rs:243-262, m <= 1), as its hConv code:
      m = 0: d0 <= 0.0001 toldel, or ss d0 <= eps_newt (ss of the previous solve)  -> 1
      m = 1: rate = (d1 / d0)^(1/1) = d1 / d0 exactly; rate > RATEMAX               -> 3 (ConvergenceRecover)
             ss = rate / (1 - rate); ss d1 <= eps_newt                               -> 2
      otherwise                                                                      -> 0 (go on with m = 2)
    d1 is only read when the m = 0 test fails (the second iteration runs only then)."""
    if d0 <= 0.0001 * toldel:
        return 1
    if ss * d0 <= eps_newt:
        return 1
    rate = d1 / d0
    if rate > RATEMAX:
        return 3
    if (rate / (1.0 - rate)) * d1 <= eps_newt:
        return 2
    return 0


def nasty(rng, shape, special=True):
    """Random doubles for state vectors: magnitudes spread over 10^-300 .. 10^300, both signs, with +0.0, -0.0 and subnormals
    mixed in (special=False: ordinary magnitudes, 10^-3 .. 10^3)."""
    lo, hi = (-300, 300) if special else (-3, 3)
    x = rng.standard_normal(shape) * 10.0 ** rng.uniform(lo, hi, size=shape)
    if special:
        u = rng.random(shape)
        x = np.where(u < 0.03, 0.0, x)
        x = np.where((u >= 0.03) & (u < 0.06), -0.0, x)
        x = np.where((u >= 0.06) & (u < 0.09), rng.choice([-1.0, 1.0], size=shape) * 5e-324 * rng.integers(1, 1 << 40, size=shape), x)
    return x


def same_bits(got, want):
    """Bit-identical where `want` is a number (so the sign of a zero counts), any NaN where `want` is NaN (sign and payload of a
    NaN are not part of the contract: test_nan_and_infinity_follow_the_reference_scan)."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64)))
