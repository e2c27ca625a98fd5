"""The 1-D Brusselator (IDAHIP_BRUSS1D, include/ida_hip.h) restated in float64 numpy, in the header's operation order: numpy's
elementwise arithmetic is IEEE with no fused multiply-add, so every value here is what the device kernels (-ffp-contract=off)
must produce, bit for bit.

TEST INFRASTRUCTURE ONLY (tests/test_bruss_ref.py pins it; tests/test_gpu_bruss.py compares the device with it). Parts:

  * res / jac / dense_dq_banded: p = [a, b, d, ub, vb]; y [2m] interleaved (y[2i] = u_i, y[2i+1] = v_i); Jacobians [n][n]
    column-major (J[j, i] = J(i, j)), as tests/dq_ref.py lays them out.
  * twin(): the host callbacks of a host-callback ctx that computes the same problem (dense jac, band bjac, res alone).
  * DirectIda / KrylovIda / PrecIda: krylov_ref.RefIda and krylov_prec_ref.RefIda with _res and the Jacobian of _setup replaced.
    The OracleIda underneath is created as a heat problem: on these paths its own residual is never called.
"""
import numpy as np

import dq_ref as DQ
import krylov_prec_ref as PR
import krylov_ref as KR
import oracle_lib as O

ML = MU = 2


def res(p, y, yp):
    a, b, d, ub, vb = (float(v) for v in p)
    y, yp = np.asarray(y, dtype=np.float64), np.asarray(yp, dtype=np.float64)
    n = y.size
    u, v = y[0::2], y[1::2]
    r = np.empty(n)
    with np.errstate(all="ignore"):
        r[0], r[1] = u[0] - ub, v[0] - vb
        r[n - 2], r[n - 1] = u[-1] - ub, v[-1] - vb
        ui, vi = u[1:-1], v[1:-1]
        w = (ui * ui) * vi
        lu = (u[:-2] - 2.0 * ui) + u[2:]
        lv = (v[:-2] - 2.0 * vi) + v[2:]
        r[2:-2:2] = yp[2:-2:2] - (((a - (b + 1.0) * ui) + w) + d * lu)
        r[3:-2:2] = yp[3:-2:2] - ((b * ui - w) + d * lv)
    return r


def jac(p, cj, y):
    """J = dF/dy + cj dF/dy' -> [n][n] column-major; +0.0 wherever the header names no entry."""
    a, b, d, ub, vb = (float(v) for v in p)
    y = np.asarray(y, dtype=np.float64)
    n = y.size
    m = n // 2
    J = np.zeros((n, n))
    for k in (0, 1, n - 2, n - 1):
        J[k, k] = 1.0
    with np.errstate(all="ignore"):
        for i in range(1, m - 1):
            u, v = y[2 * i], y[2 * i + 1]
            t2 = (2.0 * u) * v
            uu = u * u
            r = 2 * i
            J[r - 2, r] = -d
            J[r, r] = cj - ((t2 - (b + 1.0)) - 2.0 * d)
            J[r + 1, r] = -uu
            J[r + 2, r] = -d
            r = 2 * i + 1
            J[r - 2, r] = -d
            J[r - 1, r] = -(b - t2)
            J[r, r] = cj + (uu + 2.0 * d)
            J[r + 2, r] = -d
    return J


def dense_dq_banded(p, yy, yp, ewt, rr, cj, hh):
    """What the device writes on a dense ctx: dq_ref.dense_dq at rows j-2..j+2 of column j (where a perturbation of y_j can reach),
    +0.0 elsewhere -- equal by value to dense_dq wherever rr is the residual at (yy, yp) and finite."""
    n = np.asarray(yy).size
    full = DQ.dense_dq(lambda y, ypv: res(p, y, ypv), yy, yp, ewt, rr, cj, hh)
    J = np.zeros((n, n))
    for j in range(n):
        lo, hi = max(0, j - 2), min(n - 1, j + 2)
        J[j, lo:hi + 1] = full[j, lo:hi + 1]
    return J


def select(prob, ids):
    """The generated problem restricted to the systems `ids` (distinct parameters, in that order)."""
    out = dict(prob)
    for k in ("yy0", "yp0", "params"):
        out[k] = np.ascontiguousarray(prob[k][list(ids)])
    return out


def prob_res(prob, s):
    p = prob["params"][s]
    return lambda y, yp: res(p, y, yp)


# ------------------------------------------------------------------------------------------------ the callback twin
def twin(prob, band=None):
    """The same systems as a host-callback problem (idahip.problems.make_ctx takes it): res, the dense jac, and with band=(ml, mu)
    the band bjac."""
    P = prob["params"]
    out = dict(prob)
    out["kind"] = "host_callback"
    out.pop("params")
    out["res"] = lambda s, t, y, yp: res(P[s], y, yp)
    out["jac"] = lambda s, t, cj, y, yp, r: jac(P[s], cj, y).T  # (row, column)
    if band is not None:
        import idahip
        ml, mu = band
        out["band"] = (ml, mu)
        out["bjac"] = lambda s, t, cj, y, yp, r, ab: idahip.band_pack(jac(P[s], cj, y).T, ml, mu)
    return out


# ------------------------------------------------------------------------------------------------ the reference steppers
def _oracle_stub(n):
    """data for the OracleIda underneath: a heat problem of the same size (its residual is never called)"""
    return {"params": np.array([1.0])}


class _Bruss:
    def _res(self, tn, y, yp):
        return res(self.p, y, yp)


class KrylovIda(_Bruss, KR.RefIda):
    """direct=True: the dense direct solve with the analytic Jacobian above; direct=False: plain SPGMR."""

    def __init__(self, p, n, yy0, yp0, rtol, atol, maxl=5, direct=False, mxstep=500):
        KR.RefIda.__init__(self, "heat1d", n, yy0, yp0, rtol, atol, maxl=maxl, direct=direct, mxstep=mxstep, **_oracle_stub(n))
        self.p = np.array(p, dtype=np.float64)

    def _setup(self, r):
        o = self.o
        o.set("nsetups", o.get("nsetups") + 1)
        info = 0
        if self.direct:
            o.set("nje", o.get("nje") + 1)
            info, self.lu, self.piv = O.getrf(jac(self.p, o.get("cj"), o.getv("yy")).T)
        o.set("cjold", o.get("cj"))
        o.set("cjratio", 1.0)
        o.set("ss", 20.0)
        return KR.NLS_SUCCESS if info == 0 else KR.NLS_LSETUP_RECVR


class PrecIda(_Bruss, PR.RefIda):
    """SPGMR with the band preconditioner (ml, mu): krylov_prec_ref's setup already differences _res."""

    def __init__(self, p, n, yy0, yp0, rtol, atol, ml, mu, maxl=5, mxstep=500):
        PR.RefIda.__init__(self, "heat1d", n, yy0, yp0, rtol, atol, ml, mu, maxl=maxl, mxstep=mxstep, **_oracle_stub(n))
        self.p = np.array(p, dtype=np.float64)


def systems(prob, mode, ids=None, maxl=5, width=None):
    """mode: "direct", "krylov" or "prec" (width = (ml, mu))."""
    out = []
    for s in (range(prob["yy0"].shape[0]) if ids is None else ids):
        a = (prob["params"][s], prob["n"], prob["yy0"][s], prob["yp0"][s], prob["rtol"], prob["atol"])
        if mode == "prec":
            out.append(PrecIda(*a, width[0], width[1], maxl=maxl))
        else:
            out.append(KrylovIda(*a, maxl=maxl, direct=(mode == "direct")))
    return out


def run(prob, touts, mode="direct", ids=None, maxl=5, width=None):
    """Ida::solve(tout) for every tout and system -> dict(status, tret, yy, yp, counters (per name of krylov_prec_ref.CNT, zeros where
    the mode has none), kused, hused, tn), arrays [ntout][B][..]."""
    sy = systems(prob, mode, ids, maxl, width)
    B, n, T = len(sy), prob["n"], len(touts)
    st, tr = np.zeros((T, B), dtype=np.int32), np.zeros((T, B))
    yy, yp = np.zeros((T, B, n)), np.zeros((T, B, n))
    cn = {k: np.zeros((T, B), dtype=np.int64) for k in PR.CNT}
    ku, hu, tn = np.zeros((T, B), dtype=np.int64), np.zeros((T, B)), np.zeros((T, B))
    for i, t in enumerate(touts):
        for b, s in enumerate(sy):
            st[i, b], tr[i, b] = s.solve(float(t), 0)
            yy[i, b], yp[i, b] = s.o.getv("yy"), s.o.getv("yp")
            c = s.o.counters()
            c.update(nli=s.nli, ncfl=s.ncfl, nre_dq=s.nre_dq, npe=getattr(s, "npe", 0), nps=getattr(s, "nps", 0))
            for k in PR.CNT:
                cn[k][i, b] = c[k]
            ku[i, b], hu[i, b], tn[i, b] = int(s.o.get("kused")), s.o.get("hused"), s.o.get("tn")
    return {"status": st, "tret": tr, "yy": yy, "yp": yp, "counters": cn, "kused": ku, "hused": hu, "tn": tn}
