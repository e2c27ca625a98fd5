"""IDACalcIC for ONE system restated in float64 numpy: the algorithm of DESIGN.md section 4f (C IDA's ida_ic.c without constraints,
sysindex = 1, line search always on), built only from primitives that are pinned on the oracle elsewhere -- oracle_lib.problem_res /
problem_jac, getrf / getrs, wrms, and dq_ref's difference-quotient Jacobians -- or from a Python callable that the product is given
too (host-callback problems). numpy's elementwise float64 arithmetic is IEEE without fused multiply-add, so every value here is
what libidaens + libidahip must produce: bit for bit on a dense ctx, by value on a band ctx.

The steps the device runs as entry points of their own -- begin, trial_point, solve_norm, accept, commit -- are module-level
functions, and calc_ic is made of them: tests/test_gpu_ic_entry_points.py compares each idahip_ic_* call with the same statement of
its formula that the whole runs are compared with.

TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np

import dq_ref as R
import oracle_lib as O

YA_YDP_INIT, Y_INIT = 1, 2
SUCCESS, CONV_FAIL, LINESEARCH_FAIL, NO_RECOVERY, ILL_INPUT, BAD_EWT = 0, -4, -13, -14, -22, -24

EPS = float(np.finfo(np.float64).eps)
EPS_NEWT = 0.01 * 0.33
MAXNH, MAXNJ, MAXNIT, MAXBACKS = 5, 4, 10, 100
ALPHALS, ICRATEMAX = 1e-4, 0.9
STEPTOL = math.pow(EPS, 2.0 / 3.0)

OK, FAIL_RECOV, LINESRCH, CONV, SLOW = range(5)
COUNTERS = ("nre", "nsetups", "nje", "nni", "ncfn", "nbacktr", "nre_dq")


def ewt_set(y, rtol, atol):
    with np.errstate(all="ignore"):
        return 1.0 / (rtol * np.abs(y) + atol)


def begin(phi0, phi1, rtol, atol):
    """idahip_ic_begin / IDACalcIC's first lines -> (ewt = ewt_set(phi0), bad: some weight <= 0 (a NaN is not), ||phi1||_wrms(ewt))"""
    ewt = ewt_set(phi0, rtol, atol)
    return ewt, bool((ewt <= 0.0).any()), O.wrms(phi1, ewt)


def commit(y0, rtol, atol):
    """the weights of a converged pass -> (ewt = ewt_set(y0), bad)"""
    ewt = ewt_set(y0, rtol, atol)
    return ewt, bool((ewt <= 0.0).any())


def trial_point(y0, yp0, delta, lam, cj, diff):
    """The line search's point: a differential component (diff[i]; none with Y_INIT) keeps y and moves y' by (cj*lam)*delta, every
    other one moves y by lam*delta and keeps y'."""
    with np.errstate(all="ignore"):
        return np.where(diff, y0, y0 - lam * delta), np.where(diff, yp0 - (cj * lam) * delta, yp0)


def solve_norm(lu, piv, rhs, ewt):
    """-> (x = LU^-1 rhs, ||x||_wrms(ewt)): getrs without scaling, the sum taken left to right"""
    x = O.getrs(lu, piv, rhs)
    return x, O.wrms(x, ewt)


def accept(y0, yp0, ynew, ypnew, delnew, icopt):
    """an accepted trial -> (iterate y, iterate y', direction): y' moves only with YA_YDP_INIT; delta <- delnew"""
    return ynew, (ypnew if icopt == YA_YDP_INIT else yp0), delnew


class Problem:
    """res(y, yp) -> F [n]; jac(cj, y, yp, rr, hic, ewt) -> J [n][n] column-major (J[j, i] = J(i, j)); dq_evals: residual
    evaluations one Jacobian adds to nre_dq (0: analytic)."""

    def __init__(self, n, res, jac, dq_evals=0):
        self.n, self.res, self.jac, self.dq_evals = n, res, jac, dq_evals


def device_problem(kind, n, sysdata, t0=0.0, dq=False, band=None):
    """One system of a built-in problem kind. sysdata: params (lorenz63) / coef (heat1d) / A, B, c (linear_dense, column-major).
    dq: the ctx's difference-quotient Jacobian (dense ctx, or band=(ml, mu) for heat1d on a band ctx)."""
    if kind == "bruss1d":  # sysdata: params [a, b, d, ub, vb] (bruss_ref)
        import bruss_ref as BR
        assert not dq
        p = sysdata["params"]
        return Problem(n, lambda y, yp: BR.res(p, y, yp), lambda cj, y, yp, rr, hic, ewt: BR.jac(p, cj, y))
    if kind == "mass_action":  # sysdata: net (massaction_ref.Net or ratelaw_ref.Net), ref (that module), k (the system's constants)
        assert not dq
        M, net, k = sysdata["ref"], sysdata["net"], sysdata["k"]
        return Problem(n, lambda y, yp: M.res(net, k, y, yp), lambda cj, y, yp, rr, hic, ewt: M.jac(net, k, cj, y))
    kw = {}
    if kind == "lorenz63":
        kw["params"] = sysdata["params"]
    elif kind == "heat1d":
        kw["params"] = np.array([float(sysdata["coef"])])
    elif kind == "linear_dense":
        kw.update(A=sysdata["A"], B=sysdata["B"], c=sysdata["c"])

    def res(y, yp):
        return O.problem_res(kind, n, y, yp, tt=t0, **kw)

    if not dq:
        return Problem(n, res, lambda cj, y, yp, rr, hic, ewt: O.problem_jac(kind, n, cj, y, yp, rr=rr, tt=t0, **kw))
    if band is not None:
        assert kind == "heat1d"
        from idahip import band_unpack
        ml, mu = band

        def jac(cj, y, yp, rr, hic, ewt):
            ab = R.band_dq(R.residual_fn(kind, sysdata), y, yp, ewt, rr, cj, hic, ml, mu)
            return np.ascontiguousarray(band_unpack(ab, n, ml, mu).T)  # logical (i, j) -> column-major [j][i]

        return Problem(n, res, jac, R.dq_evals(n, band))
    if kind == "linear_dense":
        jac = lambda cj, y, yp, rr, hic, ewt: R.linear_dense_dq(sysdata["A"], sysdata["B"], sysdata["c"], y, yp, ewt, rr, cj, hic)
    elif kind == "heat1d":
        jac = lambda cj, y, yp, rr, hic, ewt: R.heat_dense_dq_banded(float(sysdata["coef"]), y, yp, ewt, rr, cj, hic)
    else:
        jac = lambda cj, y, yp, rr, hic, ewt: R.dense_dq(R.residual_fn(kind, sysdata), y, yp, ewt, rr, cj, hic)
    return Problem(n, res, jac, R.dq_evals(n))


def calc_ic(prob, yy0, yp0, rtol, atol, icopt, tout1, id=None, t0=0.0):
    """-> dict(status, yy, yp, ewt, hic, counters). On failure yy, yp are the values given (what a failed system keeps)."""
    n = prob.n
    given = (np.array(yy0, dtype=np.float64), np.array(yp0, dtype=np.float64))
    phi0, phi1 = given[0].copy(), given[1].copy()
    atol = np.asarray(atol, dtype=np.float64)
    atol = atol if atol.size == n else np.full(n, float(atol.ravel()[0]))
    cnt = dict.fromkeys(COUNTERS, 0)
    diff = np.zeros(n, dtype=bool) if icopt == Y_INIT else (np.asarray(id, dtype=np.float64) == 1.0)

    def done(status, hic=0.0, ewt=None):
        ok = status == SUCCESS
        return {"status": status, "yy": phi0 if ok else given[0], "yp": phi1 if ok else given[1], "ewt": ewt, "hic": hic,
                "counters": cnt}

    ewt, bad, ypnorm = begin(phi0, phi1, rtol, atol)
    if bad:
        return done(BAD_EWT)
    tdist = abs(tout1 - t0)
    if tdist == 0.0 or tdist < 2.0 * EPS * (abs(t0) + abs(tout1)):  # t0 == tout1 == 0: the bound is 0 too, and 0 < 0 is false
        return done(ILL_INPUT)
    hic = 0.001 * tdist
    if ypnorm > 0.5 / hic:
        hic = 0.5 / ypnorm
    if tout1 < t0:
        hic = -hic
    cj, mxnh = (1.0 / hic, MAXNH) if icopt == YA_YDP_INIT else (0.0, 1)
    st = {"yy0": phi0.copy(), "yp0": phi1.copy(), "savres": None, "delta": None, "delnew": None, "fnorm": 0.0}

    def linesearch(lu, piv):
        fnorm = st["fnorm"]
        f1norm = fnorm * fnorm * 0.5
        slpi = -2.0 * f1norm
        with np.errstate(all="ignore"):
            minlam = np.float64(STEPTOL) / np.float64(fnorm)
        lam, nbacks = 1.0, 0
        while True:
            if nbacks == MAXBACKS:
                return LINESRCH
            ynew, ypnew = trial_point(st["yy0"], st["yp0"], st["delta"], lam, cj, diff)
            st["savres"] = prob.res(ynew, ypnew)
            cnt["nre"] += 1
            st["delnew"], fnormp = solve_norm(lu, piv, st["savres"], ewt)
            if fnormp * fnormp * 0.5 <= f1norm + ALPHALS * slpi * lam:
                break
            if lam < minlam:
                return LINESRCH
            lam /= 2.0
            cnt["nbacktr"] += 1
            nbacks += 1
        st["yy0"], st["yp0"], st["accepted"] = accept(st["yy0"], st["yp0"], ynew, ypnew, st["delnew"], icopt)
        st["fnorm"] = fnormp
        return OK

    def newton(lu, piv):
        st["delta"], st["fnorm"] = solve_norm(lu, piv, st["delta"], ewt)
        if st["fnorm"] <= EPS_NEWT:
            return OK
        fnorm0 = oldfnrm = st["fnorm"]
        rate, m = 0.0, 0
        while True:
            cnt["nni"] += 1
            ret = linesearch(lu, piv)
            if ret != OK:
                break
            with np.errstate(all="ignore"):
                rate = float(np.float64(st["fnorm"]) / np.float64(oldfnrm))
            if st["fnorm"] <= EPS_NEWT:
                return OK
            m += 1
            if m >= MAXNIT:
                ret = CONV
                break
            st["delta"] = st["accepted"]
            oldfnrm = st["fnorm"]
        if rate <= ICRATEMAX:
            return ret
        if st["fnorm"] < 0.1 * fnorm0:
            return SLOW
        return ret

    def nls():
        st["savres"] = prob.res(st["yy0"], st["yp0"])
        st["delta"] = st["savres"].copy()
        cnt["nre"] += 1
        for nj in range(1, MAXNJ + 1):
            cnt["nsetups"] += 1
            cnt["nje"] += 1
            cnt["nre_dq"] += prob.dq_evals
            J = prob.jac(cj, st["yy0"], st["yp0"], st["savres"], hic, ewt)
            info, lu, piv = O.getrf(np.ascontiguousarray(J.T))
            if info != 0:
                return FAIL_RECOV
            ret = newton(lu, piv)
            if ret == SLOW and nj < MAXNJ:
                st["delta"] = st["savres"].copy()
                continue
            return ret

    ret = OK
    for nwt in (1, 2):
        for nh in range(1, mxnh + 1):
            ret = nls()
            if ret == OK:
                break
            cnt["ncfn"] += 1
            if nh == mxnh:
                break
            if ret != SLOW:
                st["yy0"], st["yp0"] = phi0.copy(), phi1.copy()
            hic *= 0.1
            cj = 1.0 / hic
        if ret != OK:
            break
        ewt, bad = commit(st["yy0"], rtol, atol)
        if bad:
            return done(BAD_EWT, hic)
        phi0, phi1 = st["yy0"].copy(), st["yp0"].copy()
    if ret == OK:
        return done(SUCCESS, hic, ewt)
    return done({FAIL_RECOV: NO_RECOVERY, LINESRCH: LINESEARCH_FAIL, CONV: CONV_FAIL, SLOW: CONV_FAIL}[ret], hic)


def calc_ic_batch(probs, yy0, yp0, rtol, atol, icopt, tout1, id=None, t0=0.0):
    """calc_ic for every system -> dict(status [B], yy [B][n], yp [B][n], ewt (list; None where failed), hic [B], counters {name: [B]})."""
    rs = [calc_ic(p, yy0[b], yp0[b], rtol, atol, icopt, tout1, id=id, t0=t0) for b, p in enumerate(probs)]
    return {"status": np.array([r["status"] for r in rs], dtype=np.int32), "yy": np.stack([r["yy"] for r in rs]),
            "yp": np.stack([r["yp"] for r in rs]), "ewt": [r["ewt"] for r in rs], "hic": np.array([r["hic"] for r in rs]),
            "counters": {k: np.array([r["counters"][k] for r in rs], dtype=np.int64) for k in COUNTERS}}
