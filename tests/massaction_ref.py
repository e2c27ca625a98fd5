"""IDAHIP_MASS_ACTION (include/ida_hip.h) restated in IEEE double arithmetic, in the header's operation order: Python floats are
IEEE doubles and nothing here is fused, so every value is what the device kernels (-ffp-contract=off) must produce, bit for bit.

TEST INFRASTRUCTURE ONLY (tests/test_massaction_ref.py pins it; tests/test_gpu_mass_action.py compares the device with it). Parts:

  * Net(prob): the network of a generated problem (idahip.problems: "reactions", "d") as per-row entry lists, built from the flat
    arrays the C ABI takes; res / jac / dense_dq: k [R] the system's rate constants; Jacobians [n][n] column-major
    (J[j, i] = J(i, j)), as tests/dq_ref.py lays them out.
  * twin(): the same network as the host callbacks of a host-callback ctx.
  * DirectIda: krylov_ref.RefIda(direct=True) with _res and _setup replaced, exactly as tests/bruss_ref.py does it, plus the
    constraint check of constr_ref after the Newton solve (constr=None: no check) and the dense DQ Jacobian (dq=True).
"""
import numpy as np

import constr_ref as CR
import dq_ref as DQ
import krylov_ref as KR
import oracle_lib as O


class Net:
    def __init__(self, prob):
        from idahip import mass_action
        self.n = int(prob["n"])
        slots, rows, reacs, nu, d = mass_action.flatten(self.n, prob["reactions"], prob["d"])
        self.slots = [tuple(int(x) for x in s if x >= 0) for s in slots]
        self.d = [float(x) for x in d]
        self.rows = [[] for _ in range(self.n)]
        for e in range(rows.size):  # ascending e: the caller's order within a row
            self.rows[int(rows[e])].append((float(nu[e]), int(reacs[e])))
        self.nreac = len(self.slots)


def _net(prob):
    if "_net" not in prob:
        prob["_net"] = Net(prob)
    return prob["_net"]


def res(net, k, y, yp):
    k, y, yp = ([float(v) for v in np.asarray(a, dtype=np.float64)] for a in (k, y, yp))
    out = np.empty(net.n)
    for i, row in enumerate(net.rows):
        acc = 0.0
        for e, (nu, r) in enumerate(row):
            q = k[r]
            for sp in net.slots[r]:
                q = q * y[sp]
            t = nu * q
            acc = t if e == 0 else acc + t
        out[i] = net.d[i] * yp[i] - acc
    return out


def jac(net, k, cj, y):
    """J = dF/dy + cj dF/dy' -> [n][n] column-major; +0.0 at every off-diagonal position without a term."""
    k, y = ([float(v) for v in np.asarray(a, dtype=np.float64)] for a in (k, y))
    cj = float(cj)
    n = net.n
    J = np.zeros((n, n))
    for i, row in enumerate(net.rows):
        acc = {}
        for nu, r in row:
            s = net.slots[r]
            for p, j in enumerate(s):
                g = k[r]
                for t, sp in enumerate(s):
                    if t != p:
                        g = g * y[sp]
                term = nu * g
                acc[j] = term if j not in acc else acc[j] + term
        for j, a in acc.items():
            J[j, i] = (cj * net.d[i] if i == j else 0.0) - a
        if i not in acc:
            J[i, i] = cj * net.d[i]
    return J


def dense_dq(net, k, yy, yp, ewt, rr, cj, hh):
    """idaLsDenseDQJac with res as the row function: every entry by the definition (dq_ref.dense_dq)."""
    return DQ.dense_dq(lambda y, ypv: res(net, k, y, ypv), yy, yp, ewt, rr, cj, hh)


def select(prob, ids):
    out = {k: v for k, v in prob.items() if k != "_net"}
    for k in ("yy0", "yp0", "params"):
        out[k] = np.ascontiguousarray(prob[k][list(ids)])
    return out


def prob_res(prob, s):
    net, k = _net(prob), prob["params"][s]
    return lambda y, yp: res(net, k, y, yp)


# ------------------------------------------------------------------------------------------------ the callback twin
def twin(prob):
    """The same systems as a host-callback problem (idahip.problems.make_ctx takes it): res and the dense jac."""
    net, P = _net(prob), prob["params"]
    out = {k: v for k, v in prob.items() if k not in ("_net", "params", "reactions", "d")}
    out["kind"] = "host_callback"
    out["res"] = lambda s, t, y, yp: res(net, P[s], y, yp)
    out["jac"] = lambda s, t, cj, y, yp, r: jac(net, P[s], cj, y).T  # (row, column)
    return out


# ------------------------------------------------------------------------------------------------ the reference stepper
class DirectIda(KR.RefIda):
    """The OracleIda underneath is created as a heat problem of the same size: on this path its own residual is never called."""

    def __init__(self, net, k, yy0, yp0, rtol, atol, constr=None, dq=False, mxstep=500):
        KR.RefIda.__init__(self, "heat1d", net.n, yy0, yp0, rtol, atol, direct=True, mxstep=mxstep, params=np.array([1.0]))
        self.net, self.k, self.dq = net, np.array(k, dtype=np.float64), dq
        self.c = None if constr is None else np.array(constr, dtype=np.float64)

    def _res(self, tn, y, yp):
        return res(self.net, self.k, y, yp)

    def _setup(self, r):
        o = self.o
        o.set("nsetups", o.get("nsetups") + 1)
        o.set("nje", o.get("nje") + 1)
        info, self.lu, self.piv = O.getrf(self._jacobian(r).T)
        o.set("cjold", o.get("cj"))
        o.set("cjratio", 1.0)
        o.set("ss", 20.0)
        return KR.NLS_SUCCESS if info == 0 else KR.NLS_LSETUP_RECVR

    def _jacobian(self, r):
        """J [n][n] column-major at the oracle's current state, r the residual there (a subclass with another problem overrides
        this and _res: tests/backward_cases.py)."""
        o = self.o
        if self.dq:
            self.nre_dq += self.net.n
            return dense_dq(self.net, self.k, o.getv("yy"), o.getv("yp"), o.getv("ewt"), r, o.get("cj"), o.get("hh"))
        return jac(self.net, self.k, o.get("cj"), o.getv("yy"))

    # -------- the constraint check of an attempt (constr_ref._constraint_check, inherited), between the Newton solve and the error
    # test. krylov_ref.RefIda._step has no place for it and is not copied here: a recoverable violation leaves the Newton solve as
    # a recoverable failure -- the step loop restores and calls _handle_n_flag exactly as for one --, and _handle_n_flag is told
    # which of the two it was. A passed or corrected check goes on to the error test as in constr_ref.RefIda._step.
    def _nonlinear_solve(self):
        ret = KR.RefIda._nonlinear_solve(self)
        self._constr_recvr = False
        if ret == KR.NLS_SUCCESS and self.c is not None and self._constraint_check() == CR.NFLAG_CONSTR_RECVR:
            self._constr_recvr = True
            return KR.NLS_CONV_RECVR
        return ret

    def _handle_n_flag(self, nflag, err_k, err_km1, cnt):
        if getattr(self, "_constr_recvr", False):
            nflag = CR.NFLAG_CONSTR_RECVR
        kflag = KR.RefIda._handle_n_flag(self, nflag, err_k, err_km1, cnt)
        if kflag == CR.CONSTR_FAIL:
            self.census["constr_fail"] += 1
        return kflag


RUN_CNT = ("nst", "nre", "nje", "nsetups", "nni", "netf", "ncfn", "n_attempts")


def systems(prob, ids=None, constr=None, dq=False, rtol=None):
    net = _net(prob)
    return [DirectIda(net, prob["params"][s], prob["yy0"][s], prob["yp0"][s], prob["rtol"] if rtol is None else rtol, prob["atol"],
                      constr=constr, dq=dq) for s in (range(prob["yy0"].shape[0]) if ids is None else ids)]


def run(prob, touts, ids=None, constr=None, dq=False, rtol=None):
    """Ida::solve(tout) for every tout and system -> dict(status, tret, yy, yp, counters (RUN_CNT and nre_dq), kused, hused, tn),
    arrays [ntout][B][..], ewt [B][n] after the last call, and census [B] (constr_ref's, of the constraint check)."""
    sy = systems(prob, ids, constr, dq, rtol)
    B, n, T = len(sy), prob["n"], len(touts)
    st, tr = np.zeros((T, B), dtype=np.int32), np.zeros((T, B))
    yy, yp = np.zeros((T, B, n)), np.zeros((T, B, n))
    cn = {k: np.zeros((T, B), dtype=np.int64) for k in RUN_CNT + ("nre_dq",)}
    ku, hu, tn = np.zeros((T, B), dtype=np.int64), np.zeros((T, B)), np.zeros((T, B))
    for i, t in enumerate(touts):
        for b, s in enumerate(sy):
            st[i, b], tr[i, b] = s.solve(float(t), 0)
            yy[i, b], yp[i, b] = s.o.getv("yy"), s.o.getv("yp")
            c = s.o.counters()
            c["nre_dq"] = s.nre_dq
            for k in cn:
                cn[k][i, b] = c[k]
            ku[i, b], hu[i, b], tn[i, b] = int(s.o.get("kused")), s.o.get("hused"), s.o.get("tn")
    return {"status": st, "tret": tr, "yy": yy, "yp": yp, "counters": cn, "kused": ku, "hused": hu, "tn": tn,
            "ewt": np.array([s.o.getv("ewt") for s in sy]), "census": [dict(s.census) for s in sy]}
