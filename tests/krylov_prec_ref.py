"""Reference for the band preconditioner of a Krylov ctx and the left-preconditioned SPGMR solve (C IDA's
IDABBDPRE with one block and left preconditioning in SPGMR -- the reference project has neither, so the definition in section 4i is the
definition and this file is its restatement in numpy).

TEST INFRASTRUCTURE ONLY (tests/test_krylov_prec_ref.py pins it on something independent and takes the census of its branches;
tests/test_gpu_krylov_prec.py compares the device with it, by value). Three parts, every line one IEEE operation:

  * band_getrf / band_getrs: the arithmetic stated at the top of rust-ida_amd/csrc/band_kernels.hpp on LAPACK band storage, in the
    layout of tests/dq_ref.py: AB [n][ldab] with AB[j, ml + mu + i - j] = A(i, j), ldab = 2 ml + mu + 1.
  * spgmr_solve_prec: krylov_ref.spgmr_solve with the two changes of section 4i (r = P^-1 b in step 1, u = P^-1 Jv in step 3).
  * RefIda / run(): krylov_ref.RefIda whose linear setup is dq_ref.band_dq plus the factorisation, with the recoverable-failure exit
    and the counters npe, nps, nre_dq.
"""
import math

import numpy as np

import dq_ref as DQ
import krylov_ref as KR
from krylov_ref import SUCCESS, RES_REDUCED, CONV_FAIL, QRSOL_FAIL, NLS_SUCCESS, NLS_LSETUP_RECVR, kdot, givens_column, qr_solve

PREC_CENSUS = ("prec_zero_iter", "prec_iter")
CNT = KR.CNT + ("npe", "nps")


def new_census():
    c = KR.new_census()
    c.update(dict.fromkeys(PREC_CENSUS, 0))
    return c


# ------------------------------------------------------------------------------------------------ band LU
def band_getrf(ab, n, ml, mu):
    """dgbtf2 with band_kernels.hpp's arithmetic -> (info, factors [n][ldab], piv [n] int64, 0-based rows). Strict `>` pivot search
    (lowest row on ties), reciprocal then multiply, unfused a_ij -= a_kj * a_ik, a column skipped when a_kj == 0; stops at the first
    zero pivot (info = its 1-based column; what is stored from there on is unspecified)."""
    kv, ld = ml + mu, 2 * ml + mu + 1
    A = np.array(ab, dtype=np.float64).reshape(n, ld).copy()
    for j in range(n):  # the fill rows start as zeros
        for i in range(max(0, j - kv), j - mu):
            A[j, kv + i - j] = 0.0
    piv = np.zeros(n, dtype=np.int64)
    info, ju = 0, 0
    with np.errstate(all="ignore"):
        for j in range(n):
            km = min(ml, n - 1 - j)
            jp = 0
            for r in range(1, km + 1):
                if abs(A[j, kv + r]) > abs(A[j, kv + jp]):
                    jp = r
            piv[j] = j + jp
            if A[j, kv + jp] == 0.0:
                info = j + 1
                break
            ju = max(ju, min(j + mu + jp, n - 1))
            if jp != 0:
                for c in range(j, ju + 1):
                    t = A[c, kv + j - c]
                    A[c, kv + j - c] = A[c, kv + j + jp - c]
                    A[c, kv + j + jp - c] = t
            mult = 1.0 / A[j, kv]
            A[j, kv + 1:kv + km + 1] = A[j, kv + 1:kv + km + 1] * mult
            lcol = A[j, kv + 1:kv + km + 1].copy()
            for c in range(j + 1, ju + 1):
                akj = A[c, kv + j - c]
                if akj != 0.0:
                    A[c, kv + j + 1 - c:kv + j + km + 1 - c] = A[c, kv + j + 1 - c:kv + j + km + 1 - c] - akj * lcol
    return info, A, piv


def band_getrs(A, piv, n, ml, mu, b):
    """dgbtrs: the interleaved forward solve (swap b_j / b_piv[j], then eliminate with column j of L), then back substitution with
    true division."""
    kv = ml + mu
    x = np.array(b, dtype=np.float64).copy()
    with np.errstate(all="ignore"):
        for j in range(n):
            l = int(piv[j])
            if l != j:
                t = x[l]
                x[l] = x[j]
                x[j] = t
            bj = x[j]
            lm = min(ml, n - 1 - j)
            x[j + 1:j + lm + 1] = x[j + 1:j + lm + 1] - A[j, kv + 1:kv + lm + 1] * bj
        for k in range(n - 1, -1, -1):
            x[k] = x[k] / A[k, kv]
            xk = x[k]
            lo = max(0, k - kv)
            x[lo:k] = x[lo:k] - A[k, kv + lo - k:kv] * xk
    return x


def psetup(res, yy, yp, ewt, rr, cj, hh, ml, mu):
    """P = the band DQ Jacobian at (yy, yp) with rr = res(yy, yp), factored -> (info, factors, piv). res(y, yp)."""
    n = np.asarray(yy).size
    return band_getrf(DQ.band_dq(res, yy, yp, ewt, rr, cj, hh, ml, mu), n, ml, mu)


# ------------------------------------------------------------------------------------------------ the solve
def spgmr_solve_prec(res, psolve, b, w, yy, yp, rr, tn, cj, tol, maxl, census=None):
    """krylov_ref.spgmr_solve with r = psolve(b) in step 1 (the zero-iteration return gives x = r) and u = psolve(Jv) in step 3.
    A failure flag forms nothing: x = b, as without a preconditioner."""
    b, w, yy, yp, rr = (np.asarray(v, dtype=np.float64) for v in (b, w, yy, yp, rr))
    n = b.size
    V = np.zeros((maxl + 1, n))
    r0 = psolve(b)
    V[0] = w * r0
    beta = math.sqrt(kdot(V[0], V[0]))
    if beta <= tol:
        if census is not None:
            census["zero_iter"] += 1
            census["prec_zero_iter"] += 1
        return {"x": r0.copy(), "nli": 0, "flag": SUCCESS, "res_norm": beta}
    V[0] = V[0] * (1.0 / beta)
    rot = 1.0
    H = [[0.0] * KR.MAXL_MAX for _ in range(KR.MAXL_MAX + 1)]
    q = [0.0] * (2 * KR.MAXL_MAX)
    nli, rho, krydim, converged = 0, beta, 0, False
    sig = math.sqrt(float(n)) * 1.0
    cjsig = cj * sig
    inv_sig = 1.0 / sig
    for l in range(maxl):
        nli += 1
        if census is not None and l >= 1:
            census["prec_iter"] += 1
        z = V[l] / w
        y1 = sig * z + yy
        yp1 = cjsig * z + yp
        f1 = res(tn, y1, yp1)
        jv = inv_sig * (f1 - rr)
        u = psolve(jv)
        V[l + 1] = w * u
        for i in range(l + 1):
            H[i][l] = kdot(V[i], V[l + 1])
            V[l + 1] = V[l + 1] - H[i][l] * V[i]
        hn = math.sqrt(kdot(V[l + 1], V[l + 1]))
        H[l + 1][l] = hn
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
    return {"x": xc / w, "nli": nli, "flag": flag, "res_norm": rho}


def newton_iter_krylov_prec(res, psolve, delta, ee, ewt, yy, yp, savres, tn, cj, eps_newt, maxl, census=None):
    """idahip_newton_iter_krylov on a preconditioned ctx for one system -> (delta, ee, delnrm, nli, flag)."""
    import oracle_lib as O
    d = -np.asarray(delta, dtype=np.float64)
    ee = np.array(ee, dtype=np.float64, copy=True)
    r = spgmr_solve_prec(res, psolve, d, ewt, yy, yp, savres, tn, cj, KR.eplin(d.size, eps_newt), maxl, census)
    if r["flag"] != SUCCESS:
        return d, ee, 0.0, r["nli"], r["flag"]
    d = r["x"]
    return d, ee + d, O.wrms(d, ewt), r["nli"], r["flag"]


# ------------------------------------------------------------------------------------------------ the stepper
class RefIda(KR.RefIda):
    """krylov_ref.RefIda with the band preconditioner (ml, mu): the linear setup forms and factors P (a zero pivot is the recoverable
    setup failure of a direct solver), the linear solve is the left-preconditioned one."""

    def __init__(self, kind, n, yy0, yp0, rtol, atol, ml, mu, maxl=5, mxstep=500, **data):
        super().__init__(kind, n, yy0, yp0, rtol, atol, maxl=maxl, direct=False, mxstep=mxstep, **data)
        self.ml, self.mu = ml, mu
        self.npe = self.nps = 0
        self.kcensus = new_census()
        self.pab = self.ppiv = None

    def _setup(self, r):
        o = self.o
        o.set("nsetups", o.get("nsetups") + 1)
        tn = o.get("tn")
        info, self.pab, self.ppiv = psetup(lambda y, yp: self._res(tn, y, yp), o.getv("yy"), o.getv("yp"), o.getv("ewt"), r,
                                           o.get("cj"), o.get("hh"), self.ml, self.mu)
        self.npe += 1
        self.nre_dq += DQ.dq_evals(self.n, (self.ml, self.mu))
        o.set("cjold", o.get("cj"))
        o.set("cjratio", 1.0)
        o.set("ss", 20.0)
        return NLS_SUCCESS if info == 0 else NLS_LSETUP_RECVR

    def _psolve(self, v):
        return band_getrs(self.pab, self.ppiv, self.n, self.ml, self.mu, v)

    def _lsolve(self, delta, w):
        o = self.o
        r = spgmr_solve_prec(self._res, self._psolve, delta, w, o.getv("yy"), o.getv("yp"), o.getv("savres"), o.get("tn"), o.get("cj"),
                             KR.eplin(self.n, o.get("eps_newt")), self.maxl, self.kcensus)
        self.nli += r["nli"]
        self.nre_dq += r["nli"]
        self.nps += 1 + r["nli"]
        if r["flag"] != SUCCESS:
            self.ncfl += 1
            return None, True
        return r["x"], False


def systems(prob, ml, mu, maxl=5, mxstep=500):
    out = []
    for s in range(prob["yy0"].shape[0]):
        data = {}
        if prob.get("params") is not None:
            data["params"] = prob["params"][s]
        for k in ("A", "B", "c"):
            if prob.get(k) is not None:
                data[k] = prob[k][s]
        out.append(RefIda(prob["kind"], prob["n"], prob["yy0"][s], prob["yp0"][s], prob["rtol"], prob["atol"], ml, mu, maxl=maxl,
                          mxstep=mxstep, **data))
    return out


def run(prob, touts, ml, mu, maxl=5, mxstep=500, itask=0):
    """krylov_ref.run with the preconditioner -> the same dict, counters per name of CNT (npe, nps added)."""
    sy = systems(prob, ml, mu, maxl, mxstep)
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
            c.update(nli=s.nli, ncfl=s.ncfl, nre_dq=s.nre_dq, npe=s.npe, nps=s.nps)
            for k in CNT:
                cn[k][i, b] = c[k]
            ku[i, b], hu[i, b], tn[i, b] = int(s.o.get("kused")), s.o.get("hused"), s.o.get("tn")
    return {"status": st, "tret": tr, "yy": yy, "yp": yp, "counters": cn, "kused": ku, "hused": hu, "tn": tn,
            "census": [dict(s.kcensus) for s in sy], "systems": sy}


# ------------------------------------------------------------------------------------------------ the cases both test files share
STEP_N, STEP_MAXL, STEP_WIDTH = 65, 5, (1, 1)
# krylov_cases.step_problem's family (kappa_b = K (1 + b), B = 6) with K raised from 0.02 until the unpreconditioned reference
# records a linear convergence failure on every system (test_krylov_prec_ref.py asserts that it does)
STEP_KAPPA0 = 0.5


def step_problem():
    import krylov_cases as KC
    p = KC.step_problem("heat1d", STEP_N)
    n = STEP_N
    kappa = STEP_KAPPA0 * (1.0 + np.arange(KC.STEP_B))
    dx = 1.0 / (n - 1)
    coef = kappa / (dx * dx)
    y = p["yy0"][0]
    p["params"] = coef.reshape(KC.STEP_B, 1)
    p["yp0"][:] = 0.0
    p["yp0"][:, 1:-1] = coef[:, None] * ((y[None, :-2] - 2.0 * y[None, 1:-1]) + y[None, 2:])
    return p


_STEP = {}


def step_reference():
    """-> (problem, preconditioned reference run), computed once."""
    if "p" not in _STEP:
        p = step_problem()
        _STEP["p"] = (p, run(p, p["touts"], *STEP_WIDTH, maxl=STEP_MAXL))
    return _STEP["p"]


def step_reference_plain():
    if "u" not in _STEP:
        p = step_problem()
        _STEP["u"] = KR.run(p, p["touts"], maxl=STEP_MAXL)
    return _STEP["u"]


_SOLVE = {}


def solve_reference(n, maxl, ml, mu, hh=1.0e-3):
    """The preconditioned solve of every system of krylov_cases.solve_inputs("heat1d", n, maxl) with P from psetup at (ml, mu) and the
    case's own cj, computed once -> (inputs, [(info, ab, piv)], [result dict], census)."""
    import krylov_cases as KC
    key = (n, maxl, ml, mu)
    if key not in _SOLVE:
        c = KC.solve_inputs("heat1d", n, maxl)
        census = new_census()
        facs, out = [], []
        for s in range(KC.B):
            res = KR.make_res(c["prob"], s)
            tn = c["tn"][s]
            f = psetup(lambda y, yp: res(tn, y, yp), c["yy"][s], c["yp"][s], c["ewt"][s], c["savres"][s], c["cj"][s], hh, ml, mu)
            assert f[0] == 0
            facs.append(f)
            out.append(spgmr_solve_prec(res, lambda v: band_getrs(f[1], f[2], n, ml, mu, v), c["b"][s], c["ewt"][s], c["yy"][s],
                                        c["yp"][s], c["savres"][s], tn, c["cj"][s], c["tol"][s], maxl, census))
        _SOLVE[key] = (c, facs, out, census)
    return _SOLVE[key]
