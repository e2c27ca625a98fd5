"""Reference for the matrix-free SPGMR solver of a Krylov ctx (C IDA's default iterative linear solver -- the
reference project has none, so the definition in section 4h is the definition and this file is its restatement in numpy).

TEST INFRASTRUCTURE ONLY (tests/test_krylov_ref.py pins it on something independent and takes the census of its branches;
tests/test_gpu_krylov.py compares the device with it, bit for bit). Two parts:

  * kdot / spgmr_solve / newton_iter_krylov: every line one IEEE operation (numpy does not contract a*b + c), residuals through
    oracle_lib.problem_res, which is the operation order of the device's residual kernels.
  * RefIda / run(): tests/constr_ref.py's restated Ida::solve around one OracleIda, with Ida::nonlinear_solve and Newton::solve
    (oracle/ida.hpp:514-536, oracle/newton.hpp:55-101) restated in Python and the Krylov solve inside. direct=True puts the oracle's
    own dense direct solve back (Jacobian, dense_get_rf / dense_get_rs, the 2/(1+cjratio) scaling): that loop is Ida::solve itself.
"""
import math

import numpy as np

import constr_ref as CR
import oracle_lib as O

SUCCESS, RES_REDUCED, CONV_FAIL, QRSOL_FAIL = 0, 1, 2, 3
MAXL_MAX = 16
XRATE, RATEMAX, MAXNLSIT = 0.25, 0.9, 4
NLS_SUCCESS, NLS_CONV_RECVR, NLS_LSETUP_RECVR = 0, 1, 2
CENSUS = ("zero_iter", "conv_early", "conv_last", "res_reduced", "conv_fail", "qrsol_fail", "givens_t2_zero", "givens_t2_ge_t1",
          "givens_t1_gt_t2")
CNT = CR.CNT + ("nli", "ncfl", "nre_dq")


def new_census():
    return dict.fromkeys(CENSUS, 0)


def kdot(x, y):
    """p_i = x_i y_i; partial q = p_q + p_{q+64} + ... left to right from +0.0; the 64 partials summed left to right from +0.0."""
    p = np.asarray(x, dtype=np.float64) * np.asarray(y, dtype=np.float64)
    part = np.zeros(64)
    for k in range(0, p.size, 64):
        c = p[k:k + 64]
        part[:c.size] = part[:c.size] + c
    r = np.float64(0.0)
    for q in range(64):
        r = r + part[q]
    return float(r)


def eplin(n, eps_newt):
    """tol = (sqrt(n) * 0.05) * eps_newt."""
    return (math.sqrt(float(n)) * 0.05) * eps_newt


def make_res(prob, s):
    """The residual of system s of a generated problem (idahip.problems) as res(tn, y, yp)."""
    data = {}
    if prob.get("params") is not None:
        data["params"] = prob["params"][s]
    for k in ("A", "B", "c"):
        if prob.get(k) is not None:
            data[k] = prob[k][s]
    kind, n = prob["kind"], prob["n"]
    return lambda tn, y, yp: O.problem_res(kind, n, y, yp, tt=tn, **data)


def givens_column(H, q, l, census=None):
    """The Givens update of column l of H in place (earlier rotations, then the new one) -> (c, s)."""
    for k in range(l):
        c, s = q[2 * k], q[2 * k + 1]
        t1, t2 = H[k][l], H[k + 1][l]
        H[k][l] = c * t1 - s * t2
        H[k + 1][l] = s * t1 + c * t2
    t1, t2 = H[l][l], H[l + 1][l]
    if t2 == 0.0:
        c, s = 1.0, 0.0
        branch = "givens_t2_zero"
    elif abs(t2) >= abs(t1):
        t3 = t1 / t2
        s = -1.0 / math.sqrt(1.0 + t3 * t3)
        c = -s * t3
        branch = "givens_t2_ge_t1"
    else:
        t3 = t2 / t1
        c = 1.0 / math.sqrt(1.0 + t3 * t3)
        s = -c * t3
        branch = "givens_t1_gt_t2"
    if census is not None:
        census[branch] += 1
    q[2 * l], q[2 * l + 1] = c, s
    H[l][l] = c * t1 - s * t2
    return c, s


def qr_solve(H, q, beta, krydim):
    """g = Q [beta, 0, ...], then the back-substitution -> (g, ok); ok False on a zero diagonal entry."""
    g = [0.0] * (MAXL_MAX + 1)
    g[0] = beta
    for k in range(krydim):
        c, s = q[2 * k], q[2 * k + 1]
        t1, t2 = g[k], g[k + 1]
        g[k] = c * t1 - s * t2
        g[k + 1] = s * t1 + c * t2
    for k in range(krydim - 1, -1, -1):
        if H[k][k] == 0.0:
            return g, False
        g[k] = g[k] / H[k][k]
        for i in range(k):
            g[i] = g[i] - g[k] * H[i][k]
    return g, True


def spgmr_solve(res, b, w, yy, yp, rr, tn, cj, tol, maxl, census=None, dump=None):
    """The linear solve of one system -> dict(x, nli, flag, res_norm). census: branch counters (new_census()); dump: a list that
    receives (l, column of H before the Givens update [l + 2 entries]) per iteration and at the end ("end", beta, tol)."""
    b, w, yy, yp, rr = (np.asarray(v, dtype=np.float64) for v in (b, w, yy, yp, rr))
    n = b.size
    V = np.zeros((maxl + 1, n))
    V[0] = w * b
    beta = math.sqrt(kdot(V[0], V[0]))
    if dump is not None:
        dump.append(("begin", beta, tol))
    if beta <= tol:
        if census is not None:
            census["zero_iter"] += 1
        return {"x": b.copy(), "nli": 0, "flag": SUCCESS, "res_norm": beta}
    V[0] = V[0] * (1.0 / beta)
    rot = 1.0
    H = [[0.0] * MAXL_MAX for _ in range(MAXL_MAX + 1)]
    q = [0.0] * (2 * MAXL_MAX)
    nli, rho, krydim, converged = 0, beta, 0, False
    sig = math.sqrt(float(n)) * 1.0
    cjsig = cj * sig
    inv_sig = 1.0 / sig
    for l in range(maxl):
        nli += 1
        z = V[l] / w
        y1 = sig * z + yy
        yp1 = cjsig * z + yp
        f1 = res(tn, y1, yp1)
        jv = inv_sig * (f1 - rr)
        V[l + 1] = w * jv
        for i in range(l + 1):
            H[i][l] = kdot(V[i], V[l + 1])
            V[l + 1] = V[l + 1] - H[i][l] * V[i]
        hn = math.sqrt(kdot(V[l + 1], V[l + 1]))
        H[l + 1][l] = hn
        if dump is not None:
            dump.append((l, [H[i][l] for i in range(l + 2)]))
        c, s = givens_column(H, q, l, census)
        rot = rot * s
        rho = abs(rot * beta)
        if rho <= tol:
            converged, krydim = True, l + 1
            break
        V[l + 1] = V[l + 1] * (1.0 / hn)
    flag = SUCCESS
    if not converged:
        krydim = maxl
        if not (rho < beta):
            if census is not None:
                census["conv_fail"] += 1
            return {"x": b.copy(), "nli": nli, "flag": CONV_FAIL, "res_norm": rho}
        flag = RES_REDUCED
    g, ok = qr_solve(H, q, beta, krydim)
    if not ok:
        if census is not None:
            census["qrsol_fail"] += 1
        return {"x": b.copy(), "nli": nli, "flag": QRSOL_FAIL, "res_norm": rho}
    if census is not None:
        census["res_reduced" if flag == RES_REDUCED else ("conv_last" if krydim == maxl else "conv_early")] += 1
    xc = g[0] * V[0]
    for k in range(1, krydim):
        xc = xc + g[k] * V[k]
    return {"x": xc / w, "nli": nli, "flag": flag, "res_norm": rho, "g": g[:krydim], "H": H, "q": q, "krydim": krydim}


def newton_iter_krylov(res, delta, ee, ewt, yy, yp, savres, tn, cj, eps_newt, maxl, census=None):
    """idahip_newton_iter_krylov for one system -> (delta, ee, delnrm, nli, flag): delta = -delta; the solve; flag 0: delta = x,
    ee += delta, delnrm = the left-to-right WRMS norm; any other flag: ee untouched, delta the negated residual, delnrm 0."""
    d = -np.asarray(delta, dtype=np.float64)
    ee = np.array(ee, dtype=np.float64, copy=True)
    r = spgmr_solve(res, d, ewt, yy, yp, savres, tn, cj, eplin(d.size, eps_newt), maxl, census)
    if r["flag"] != SUCCESS:
        return d, ee, 0.0, r["nli"], r["flag"]
    d = r["x"]
    return d, ee + d, O.wrms(d, ewt), r["nli"], r["flag"]


class RefIda(CR.RefIda):
    """One system: constr_ref's restated Ida::solve with the Newton solve restated here and the Krylov solve of section 4h inside
    (direct=True: the oracle's dense direct solve instead). No constraints."""

    def __init__(self, kind, n, yy0, yp0, rtol, atol, maxl=5, direct=False, mxstep=500, **data):
        super().__init__(kind, n, yy0, yp0, rtol, atol, constr=None, mxstep=mxstep, **data)
        self.kind, self.data = kind, data
        self.maxl, self.direct = maxl, direct
        self.nli = self.ncfl = self.nre_dq = 0
        self.kcensus = new_census()
        self.lu = self.piv = None

    def _res(self, tn, y, yp):
        return O.problem_res(self.kind, self.n, y, yp, tt=tn, **self.data)

    # -------- NLProblem::sys / setup / solve (oracle/ida.hpp:161-183) on the oracle's state
    def _sys(self, ycor):
        o = self.o
        yy = o.getv("yypredict") + ycor
        yp = o.getv("yppredict") + o.get("cj") * ycor
        o.setv("yy", yy)
        o.setv("yp", yp)
        r = self._res(o.get("tn"), yy, yp)
        o.set("nre", o.get("nre") + 1)
        o.setv("savres", r)
        return r

    def _setup(self, r):
        o = self.o
        o.set("nsetups", o.get("nsetups") + 1)
        info = 0
        if self.direct:
            o.set("nje", o.get("nje") + 1)
            J = O.problem_jac(self.kind, self.n, o.get("cj"), o.getv("yy"), o.getv("yp"), rr=r, tt=o.get("tn"), **self.data)
            info, self.lu, self.piv = O.getrf(J.T)
        o.set("cjold", o.get("cj"))
        o.set("cjratio", 1.0)
        o.set("ss", 20.0)
        return NLS_SUCCESS if info == 0 else NLS_LSETUP_RECVR

    def _lsolve(self, delta, w):
        """-> (x, failed)"""
        o = self.o
        if self.direct:
            x = O.getrs(self.lu, self.piv, delta)
            cjratio = o.get("cjratio")
            if cjratio != 1.0:
                x = x * (2.0 / (1.0 + cjratio))
            return x, False
        r = spgmr_solve(self._res, delta, w, o.getv("yy"), o.getv("yp"), o.getv("savres"), o.get("tn"), o.get("cj"),
                        eplin(self.n, o.get("eps_newt")), self.maxl, self.kcensus)
        self.nli += r["nli"]
        self.nre_dq += r["nli"]
        if r["flag"] != SUCCESS:
            self.ncfl += 1
            return None, True
        return r["x"], False

    def _ctest(self, m, delta, w):
        o = self.o
        delnrm = O.wrms(delta, w)
        if m == 0:
            o.set("oldnrm", delnrm)
            if delnrm <= 0.0001 * o.get("toldel"):
                return NLS_SUCCESS, True
        else:
            rate = math.pow(delnrm / o.get("oldnrm"), 1.0 / float(m))
            if rate > RATEMAX:
                return NLS_CONV_RECVR, False
            o.set("ss", rate / (1.0 - rate))
        return NLS_SUCCESS, o.get("ss") * delnrm <= o.get("eps_newt")

    # -------- Newton::solve (oracle/newton.hpp:55-101)
    def _newton(self, call_lsetup, w):
        o = self.o
        y0 = np.zeros(self.n)
        ee = o.getv("ee")
        while True:
            delta = self._sys(y0)
            retval = NLS_SUCCESS
            if call_lsetup:
                retval = self._setup(delta)
                o.set("jcur", 1)
            if retval == NLS_SUCCESS:
                curiter = 0
                ee = y0.copy()
                while True:
                    o.set("nni", o.get("nni") + 1)
                    delta = -delta
                    x, failed = self._lsolve(delta, w)
                    if failed:
                        retval = NLS_CONV_RECVR
                        break
                    delta = x
                    ee = ee + delta
                    retval, converged = self._ctest(curiter, delta, w)
                    if retval != NLS_SUCCESS:
                        break
                    if converged:
                        o.set("jcur", 0)
                        o.setv("ee", ee)
                        return NLS_SUCCESS
                    curiter += 1
                    if curiter >= MAXNLSIT:
                        retval = NLS_CONV_RECVR
                        break
                    delta = self._sys(ee)
            if retval == NLS_CONV_RECVR and not o.get("jcur"):
                o.set("nls_nconvfails", o.get("nls_nconvfails") + 1)
                call_lsetup = True
                continue
            break
        o.set("nls_nconvfails", o.get("nls_nconvfails") + 1)
        o.setv("ee", ee)
        return retval

    # -------- Ida::nonlinear_solve (oracle/ida.hpp:514-536)
    def _nonlinear_solve(self):
        o = self.o
        call_lsetup = False
        if o.get("nst") == 0:
            o.set("cjold", o.get("cj"))
            o.set("ss", 20.0)
            call_lsetup = True
        cjratio = o.get("cj") / o.get("cjold")
        o.set("cjratio", cjratio)
        temp1 = (1.0 - XRATE) / (1.0 + XRATE)
        temp2 = 1.0 / temp1
        if cjratio < temp1 or cjratio > temp2:
            call_lsetup = True
        if o.get("cj") != o.get("cjlast"):
            o.set("ss", 100.0)
        o.setv("delta", np.zeros(self.n))  # Ida's delta is Newton's y0 (its own update vector is not part of the state)
        retval = self._newton(call_lsetup, o.getv("ewt"))
        ee = o.getv("ee")
        o.setv("yy", o.getv("yypredict") + ee)
        o.setv("yp", o.getv("yppredict") + o.get("cj") * ee)
        return retval

    # -------- step (oracle/ida.hpp:420-467): constr_ref's, with the Newton solve above
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
            nflag, err_k, err_km1 = CR.NFLAG_NONE, 0.0, 0.0
            nls_ret = self._nonlinear_solve()
            if nls_ret == NLS_SUCCESS:
                ek, ekm1 = O.C.c_double(0.0), O.C.c_double(0.0)
                if not L.oracle_ida_test_error(h, ck, O.C.byref(ek), O.C.byref(ekm1)):
                    nflag = CR.NFLAG_TEST_FAIL
                err_k, err_km1 = ek.value, ekm1.value
            elif nls_ret == NLS_CONV_RECVR:
                nflag = CR.NFLAG_CONV_RECVR
            else:
                nflag = CR.NFLAG_LSETUP_RECVR
            if nflag == CR.NFLAG_NONE:
                break
            if o.get("nst") == 0:
                self.nfail_first += 1
            L.oracle_ida_restore(h, saved_t)
            kflag = self._handle_n_flag(nflag, err_k, err_km1, cnt)
            if kflag != CR.SUCCESS:
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
        return CR.SUCCESS


def systems(prob, maxl=5, direct=False, mxstep=500, ids=None):
    B = prob["yy0"].shape[0]
    out = []
    for s in (range(B) if ids is None else ids):
        data = {}
        if prob.get("params") is not None:
            data["params"] = prob["params"][s]
        for k in ("A", "B", "c"):
            if prob.get(k) is not None:
                data[k] = prob[k][s]
        out.append(RefIda(prob["kind"], prob["n"], prob["yy0"][s], prob["yp0"][s], prob["rtol"], prob["atol"], maxl=maxl, direct=direct,
                          mxstep=mxstep, **data))
    return out


def run(prob, touts, maxl=5, direct=False, mxstep=500, itask=0, ids=None):
    """Ida::solve(tout) for every tout and every system -> dict(status, tret, yy, yp [ntout][B][..] after each call, counters
    [ntout][B] per name of CNT, kused, hused, tn [ntout][B], steps, census [B] (the Krylov solver's branches))."""
    sy = systems(prob, maxl, direct, mxstep, ids)
    B, n, T = len(sy), prob["n"], len(touts)
    st, tr = np.zeros((T, B), dtype=np.int32), np.zeros((T, B))
    yy, yp = np.zeros((T, B, n)), np.zeros((T, B, n))
    cn = {k: np.zeros((T, B), dtype=np.int64) for k in CNT}
    ku, hu, tn = np.zeros((T, B), dtype=np.int64), np.zeros((T, B)), np.zeros((T, B))
    for i, t in enumerate(touts):
        for b, s in enumerate(sy):
            st[i, b], tr[i, b] = s.solve(t, itask)
            yy[i, b], yp[i, b] = s.o.getv("yy"), s.o.getv("yp")
            c = s.o.counters()
            c.update(nli=s.nli, ncfl=s.ncfl, nre_dq=s.nre_dq)
            for k in CNT:
                cn[k][i, b] = c[k]
            ku[i, b], hu[i, b], tn[i, b] = int(s.o.get("kused")), s.o.get("hused"), s.o.get("tn")
    return {"status": st, "tret": tr, "yy": yy, "yp": yp, "counters": cn, "kused": ku, "hused": hu, "tn": tn,
            "steps": [np.array(s.steps, dtype=np.float64).reshape(-1, 5) for s in sy], "census": [dict(s.kcensus) for s in sy],
            "systems": sy}


def census_total(censuses):
    return {k: sum(c[k] for c in censuses) for k in CENSUS}
