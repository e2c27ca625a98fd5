"""Reference for the inequality constraints of DESIGN.md section 4g (C IDA's IDASetConstraints; the reference project has none).

TEST INFRASTRUCTURE ONLY (tests/test_constr_ref.py pins it on the oracle and takes the census of its branches;
tests/test_gpu_constraints.py compares the device with it). Two parts:

  * RefIda / run(): Ida::solve, Ida::step, handle_n_flag and reset as oracle/ida.hpp has them (solve :287-417, step :420-467,
    handle_n_flag :602-638, reset :641-644), restated in Python around one OracleIda, with the definition of section 4g inserted:
    the start check in the first-call block, the check between the Newton solve and the error test, the NFLAG_CONSTR_RECVR branch of
    handle_n_flag. Everything else is the oracle's own code through its seams (set_coeffs, predict, nonlinear_solve, test_error,
    restore, complete_step, get_solution); the one pow is math.pow (the platform libm's, as std::pow), every norm O.wrms. The
    return conventions are the product's (include/ida_ensemble.h): a negative status is sticky, except ILL_INPUT from the first-call
    block, which leaves the system unstarted. No root finding, no tstop.
  * post_newton_constr(): idahip_post_newton_constr for one system, on tests/stepper_ref.py's post_newton.

With c = None or all zeros the loop is Ida::solve itself (test_constr_ref.py: bit for bit)."""
import math

import numpy as np

import oracle_lib as O
import stepper_ref as R

EPS = 2.220446049250313e-16
DBL_MAX = 1.7976931348623157e308
EPCON = 0.33
MXNCF = MXNEF = 10
SUCCESS, CONTINUE = 0, 99
TOO_MUCH_WORK, TOO_MUCH_ACC, ERR_FAIL, CONV_FAIL, LSETUP_FAIL, CONSTR_FAIL, ILL_INPUT = -1, -2, -3, -4, -6, -11, -22
NFLAG_NONE, NFLAG_TEST_FAIL, NFLAG_CONV_RECVR, NFLAG_LSETUP_RECVR, NFLAG_CONSTR_RECVR = 0, 1, 2, 3, 4
CNT = ("nst", "nre", "nje", "nsetups", "nni", "netf", "ncfn", "n_attempts")
CENSUS = ("passed", "corrected", "recovered", "constr_fail", "start_ill")


def violated(c, y):
    """The mask: (|c_i| > 1.5 and y_i c_i <= 0) or (|c_i| > 0.5 and y_i c_i < 0); a NaN makes every comparison false."""
    c, y = np.asarray(c, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        yc = y * c
        return ((np.abs(c) > 1.5) & (yc <= 0.0)) | ((np.abs(c) > 0.5) & (yc < 0.0))


def correction(c, yy, ewt, m):
    """v_i = yy_i - 0.1 ((a_i c_i) / ewt_i) for the violated i (a_i = 1 for |c_i| >= 1.5, else 0), +0.0 elsewhere."""
    v = np.zeros(yy.shape)
    a = np.where(np.abs(c) >= 1.5, 1.0, 0.0)
    v[m] = yy[m] - 0.1 * ((a[m] * c[m]) / ewt[m])
    return v


def recover_rr(phi0, yy, m):
    """rr = fmax(0.9 q, 0.1), q = min over the violated i with phi0_i != yy_i of phi0_i / (phi0_i - yy_i) (DBL_MAX when none)."""
    q = DBL_MAX
    for i in np.flatnonzero(m):
        t = phi0[i] - yy[i]
        if t != 0.0:
            quot = phi0[i] / t
            if quot < q:
                q = quot
    return float(np.fmax(0.9 * q, 0.1))


def post_newton_constr(yypredict, yppredict, ee, ewt, phi, cj, kk, c, eps_newt, check):
    """idahip_post_newton_constr for one system -> (yy, yp, ee, norms[4], flag, rr). ee is returned new (corrected for flag 1)."""
    yy, yp, norms = R.post_newton(yypredict, yppredict, ee, ewt, phi, cj, kk)
    ee = np.array(ee, dtype=np.float64, copy=True)
    if not check:
        return yy, yp, ee, norms, 0, 0.0
    m = violated(c, yy)
    if not m.any():
        return yy, yp, ee, norms, 0, 0.0
    v = correction(c, yy, ewt, m)
    if O.wrms(v, ewt) <= eps_newt:
        ee[m] = ee[m] - v[m]
        _, _, norms = R.post_newton(yypredict, yppredict, ee, ewt, phi, cj, kk)
        return yy, yp, ee, norms, 1, 0.0
    return yy, yp, ee, np.zeros(4), 2, recover_rr(phi[0], yy, m)


class RefIda:
    """One system: the restated Ida::solve around an OracleIda, with the constraint vector constr ([n], or None: no check at all)."""

    def __init__(self, kind, n, yy0, yp0, rtol, atol, constr=None, mxstep=500, **data):
        self.o = O.OracleIda(kind, n, yy0, yp0, rtol, atol, **data)
        self.n, self.rtol, self.atol = n, rtol, np.asarray(atol, dtype=np.float64)
        self.c = None if constr is None else np.array(constr, dtype=np.float64)
        self.mxstep = mxstep
        self.setup_done = self.dead = False
        self.status, self.tret = 0, 0.0
        self.nfail_first = 0
        self.steps = []  # (tn, hused, kused, nni, nsetups) per accepted step, as the oracle records them
        self.census = dict.fromkeys(CENSUS, 0)

    # -------- seams
    def _phi(self):
        return self.o.getv("phi").reshape(6, self.n)

    def _get_solution(self, t):
        return self.o.L.oracle_ida_get_solution(self.o.h, float(t))

    # -------- stop tests (oracle/ida.hpp:820-908 without tstop)
    def _stop_test1(self, tout, itask):
        o = self.o
        tn, hh = o.get("tn"), o.get("hh")
        if itask == 0:
            if tout == o.get("tretlast"):
                o.set("tretlast", tout)
                return SUCCESS, tout
            if (tn - tout) * hh >= 0.0:
                ier = self._get_solution(tout)
                if ier != SUCCESS:
                    return ier, self.tret
                o.set("tretlast", tout)
                return SUCCESS, tout
            return CONTINUE, None
        if (tn - o.get("tretlast")) * hh > 0.0:
            self._get_solution(tn)
            o.set("tretlast", tn)
            return SUCCESS, tn
        return CONTINUE, None

    def _stop_test2(self, tout, itask):
        o = self.o
        tn, hh = o.get("tn"), o.get("hh")
        if itask == 0:
            if (tn - tout) * hh >= 0.0:
                o.set("tretlast", tout)
                self._get_solution(tout)
                return SUCCESS, tout
            return CONTINUE, None
        o.set("tretlast", tn)
        return SUCCESS, tn

    # -------- handle_n_flag (oracle/ida.hpp:602-638) with the NFLAG_CONSTR_RECVR branch
    def _handle_n_flag(self, nflag, err_k, err_km1, cnt):
        o = self.o
        o.set("phase", 1)
        if nflag == NFLAG_TEST_FAIL:
            cnt["nef"] += 1
            o.set("netf", o.get("netf") + 1)
            kk, knew = int(o.get("kk")), int(o.get("knew"))
            if cnt["nef"] == 1:
                err_knew = err_k if kk == knew else err_km1
                kk = knew
                base = 2.0 * err_knew + 0.0001
                arg = 1.0 / float(kk + 1)
                rr = 0.9 * math.pow(base, -arg)
                rr = float(np.fmax(0.25, np.fmin(0.9, rr)))
            elif cnt["nef"] == 2:
                kk, rr = knew, 0.25
            elif cnt["nef"] < MXNEF:
                kk, rr = 1, 0.25
            else:
                return ERR_FAIL
            o.set("kk", kk)
            o.set("rr", rr)
            o.set("hh", o.get("hh") * rr)
            return SUCCESS
        cnt["ncf"] += 1
        o.set("ncfn", o.get("ncfn") + 1)
        if nflag != NFLAG_CONSTR_RECVR:
            o.set("rr", 0.25)
        o.set("hh", o.get("hh") * o.get("rr"))
        if cnt["ncf"] < MXNCF:
            return SUCCESS
        return CONSTR_FAIL if nflag == NFLAG_CONSTR_RECVR else CONV_FAIL

    # -------- the check of an attempt (section 4g); returns the nflag
    def _constraint_check(self):
        o = self.o
        yy, ewt = o.getv("yy"), o.getv("ewt")
        m = violated(self.c, yy)
        if not m.any():
            self.census["passed"] += 1
            return NFLAG_NONE
        v = correction(self.c, yy, ewt, m)
        if O.wrms(v, ewt) <= o.get("eps_newt"):
            ee = o.getv("ee")
            ee[m] = ee[m] - v[m]
            o.setv("ee", ee)
            self.census["corrected"] += 1
            return NFLAG_NONE
        o.set("rr", recover_rr(self._phi()[0], yy, m))
        self.census["recovered"] += 1
        return NFLAG_CONSTR_RECVR

    # -------- step (oracle/ida.hpp:420-467)
    def _step(self):
        o, L, h = self.o, self.o.L, self.o.h
        saved_t = o.get("tn")
        if o.get("nst") == 0:
            o.set("kk", 1)
            o.set("kused", 0)
            o.set("hused", 0.0)
            psi = o.getv("psi")
            psi[0] = o.get("hh")
            o.setv("psi", psi)
            o.set("cj", 1.0 / o.get("hh"))
            o.set("phase", 0)
            o.set("ns", 0)
        cnt = {"ncf": 0, "nef": 0}
        while True:
            o.set("n_attempts", o.get("n_attempts") + 1)
            ck = L.oracle_ida_set_coeffs(h)
            o.set("tn", o.get("tn") + o.get("hh"))
            L.oracle_ida_predict(h)
            nflag, err_k, err_km1 = NFLAG_NONE, 0.0, 0.0
            nls_ret = L.oracle_ida_nonlinear_solve(h)
            if nls_ret == 0:
                if self.c is not None:
                    nflag = self._constraint_check()
                if nflag == NFLAG_NONE:
                    ek, ekm1 = O.C.c_double(0.0), O.C.c_double(0.0)
                    if not L.oracle_ida_test_error(h, ck, O.C.byref(ek), O.C.byref(ekm1)):
                        nflag = NFLAG_TEST_FAIL
                    err_k, err_km1 = ek.value, ekm1.value
            elif nls_ret == 1:
                nflag = NFLAG_CONV_RECVR
            elif nls_ret == 2:
                nflag = NFLAG_LSETUP_RECVR
            else:
                L.oracle_ida_restore(h, saved_t)
                return LSETUP_FAIL
            if nflag == NFLAG_NONE:
                break
            if o.get("nst") == 0:
                self.nfail_first += 1
            L.oracle_ida_restore(h, saved_t)
            kflag = self._handle_n_flag(nflag, err_k, err_km1, cnt)
            if kflag != SUCCESS:
                if kflag == CONSTR_FAIL:
                    self.census["constr_fail"] += 1
                return kflag
            if o.get("nst") == 0:  # reset()
                psi = o.getv("psi")
                psi[0] = o.get("hh")
                o.setv("psi", psi)
                phi = self._phi()
                phi[1] = phi[1] * o.get("rr")
                o.setv("phi", phi)
        L.oracle_ida_complete_step(h, err_k, err_km1)
        o.setv("ee", o.getv("ee") * ck)
        self.steps.append((o.get("tn"), o.get("hused"), o.get("kused"), o.get("nni"), o.get("nsetups")))
        return SUCCESS

    # -------- solve (oracle/ida.hpp:287-417)
    def solve(self, tout, itask=0):
        self.status, self.tret = self._solve(float(tout), itask)
        return self.status, self.tret

    def _solve(self, tout, itask):
        o = self.o
        if self.dead:
            return self.status, self.tret
        if not self.setup_done:
            phi = self._phi()
            ewt = R.ewt_set(phi[0], self.rtol, self.atol)
            o.setv("ewt", ewt)
            tn = o.get("tn")
            tdist = abs(tout - tn)
            if tdist == 0.0 or tdist < 2.0 * EPS * (abs(tn) + abs(tout)):
                return ILL_INPUT, tn
            if self.c is not None and violated(self.c, phi[0]).any():
                self.census["start_ill"] += 1
                return ILL_INPUT, tn
            self.setup_done = True
            hh = o.get("hin")
            if hh == 0.0:
                hh = 0.001 * tdist
                ypnorm = O.wrms(phi[1], ewt)
                if ypnorm > 2.0 / hh:
                    hh = 0.5 / ypnorm
                if tout < tn:
                    hh = -hh
            rh = abs(hh) * o.get("hmax_inv")
            if rh > 1.0:
                hh /= rh
            o.set("hh", hh)
            o.set("h0u", hh)
            o.set("kk", 0)
            o.set("kused", 0)
            phi[1] = phi[1] * hh
            o.setv("phi", phi)
            o.set("eps_newt", EPCON)
            o.set("toldel", 0.0001 * EPCON)
        nstloc = 0
        if o.get("nst") > 0:
            ist, tret = self._stop_test1(tout, itask)
            if ist != CONTINUE:
                if ist < 0:
                    self.dead = True
                return ist, tret
        while True:
            tn = o.get("tn")
            if self.mxstep > 0 and nstloc >= self.mxstep:
                o.set("tretlast", tn)
                return TOO_MUCH_WORK, tn
            phi0 = self._phi()[0]
            if o.get("nst") > 0:
                ewt = R.ewt_set(phi0, self.rtol, self.atol)
                o.setv("ewt", ewt)
                if (ewt <= 0.0).any():
                    self._get_solution(tn)
                    o.set("tretlast", tn)
                    self.dead = True
                    return ILL_INPUT, tn
            tolsf = EPS * O.wrms(phi0, o.getv("ewt"))
            if tolsf > 1.0:
                o.set("tolsf", tolsf * 10.0)
                o.set("tretlast", tn)
                if o.get("nst") > 0:
                    self._get_solution(tn)
                self.dead = True
                return TOO_MUCH_ACC, tn
            o.set("tolsf", tolsf)
            sflag = self._step()
            if sflag != SUCCESS:
                tn = o.get("tn")
                tret = self.tret
                if self._get_solution(tn) == SUCCESS:
                    tret = tn
                    o.set("tretlast", tn)
                self.dead = True
                return sflag, tret
            nstloc += 1
            ist, tret = self._stop_test2(tout, itask)
            if ist != CONTINUE:
                return ist, tret


def systems(prob, c=None, mxstep=500, ids=None):
    """One RefIda per system of a generated problem (idahip.problems); c [n] is shared, as the ABI's vector is."""
    B = prob["yy0"].shape[0]
    out = []
    for s in (range(B) if ids is None else ids):
        data = {}
        if prob.get("params") is not None:
            data["params"] = prob["params"][s]
        for k in ("A", "B", "c"):
            if prob.get(k) is not None:
                data[k] = prob[k][s]
        out.append(RefIda(prob["kind"], prob["n"], prob["yy0"][s], prob["yp0"][s], prob["rtol"], prob["atol"], constr=c, mxstep=mxstep, **data))
    return out


def run(prob, c, touts, mxstep=500, itask=0, ids=None):
    """Ida::solve(tout) for every tout and every system, each call's return recorded as the product reports it.
    -> dict(status [ntout][B], tret, yy / yp [ntout][B][n] (the system's yy / yp after the call), counters, kused, hused, hh, tn,
    nfail_first, steps [B] arrays [nsteps][5], census [B] dicts)."""
    sy = systems(prob, c, mxstep, ids)
    B, n, T = len(sy), prob["n"], len(touts)
    st, tr = np.zeros((T, B), dtype=np.int32), np.zeros((T, B))
    yy, yp = np.zeros((T, B, n)), np.zeros((T, B, n))
    for i, t in enumerate(touts):
        for b, s in enumerate(sy):
            st[i, b], tr[i, b] = s.solve(t, itask)
            yy[i, b], yp[i, b] = s.o.getv("yy"), s.o.getv("yp")
    cnts = [s.o.counters() for s in sy]
    return {"status": st, "tret": tr, "yy": yy, "yp": yp,
            "counters": {k: np.array([c_[k] for c_ in cnts], dtype=np.int64) for k in CNT},
            "kused": np.array([int(s.o.get("kused")) for s in sy], dtype=np.int64),
            "hused": np.array([s.o.get("hused") for s in sy]), "hh": np.array([s.o.get("hh") for s in sy]),
            "tn": np.array([s.o.get("tn") for s in sy]), "nfail_first": np.array([s.nfail_first for s in sy], dtype=np.int64),
            "steps": [np.array(s.steps, dtype=np.float64).reshape(-1, 5) for s in sy], "census": [dict(s.census) for s in sy]}


def census_total(ref):
    return {k: sum(c[k] for c in ref["census"]) for k in CENSUS}
