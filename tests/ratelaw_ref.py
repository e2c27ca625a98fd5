"""IDAHIP_MASS_ACTION with rate laws (idahip_set_rate_network, include/ida_hip.h) restated in IEEE double arithmetic, in the header's
operation order: every value is what the device kernels (-ffp-contract=off) must produce, bit for bit. Arithmetic is np.float64
under np.errstate(all="ignore"): a zero denominator gives what IEEE gives (NaN, +-inf), where a Python float would raise.

TEST INFRASTRUCTURE ONLY (tests/test_ratelaw_ref.py pins it; tests/test_gpu_rate_laws.py compares the device with it). It follows
tests/massaction_ref.py part by part, and reuses what does not depend on the rate: the reference stepper (DirectIda with _res and
_setup replaced), select and the counters.

  * Net(prob): the network of a generated problem (idahip.problems: "reactions" with factors, "d", "nconst") as per-row entry lists
    and per-reaction factor lists; res / jac / dense_dq: k [R + nconst] the system's parameters (rate constants, then constants);
    Jacobians [n][n] column-major (J[j, i] = J(i, j)).
  * twin(): the same network as the host callbacks of a host-callback ctx.
  * run(...): massaction_ref.run's outputs.
"""
import numpy as np

import dq_ref as DQ
import krylov_ref as KR
import massaction_ref as MA
import oracle_lib as O

SAT, INH = 1, 2
F64 = np.float64


class Net:
    def __init__(self, prob):
        from idahip import mass_action
        self.n = int(prob["n"])
        self.nconst = int(prob.get("nconst", 0))
        slots, fac, rows, reacs, nu, d = mass_action.flatten_laws(self.n, prob["reactions"], prob["d"], self.nconst)
        self.slots = [tuple(int(x) for x in s if x >= 0) for s in slots]
        self.d = [F64(x) for x in d]
        self.rows = [[] for _ in range(self.n)]
        for e in range(rows.size):  # ascending e: the caller's order within a row
            self.rows[int(rows[e])].append((F64(nu[e]), int(reacs[e])))
        self.nreac = len(self.slots)
        self.factors = [[] for _ in range(self.nreac)]
        for r, op, sp, c, h in fac:  # ascending: the caller's order within a reaction
            self.factors[int(r)].append((int(op), int(sp), int(c), int(h)))


def _net(prob):
    if "_lawnet" not in prob:
        prob["_lawnet"] = Net(prob)
    return prob["_lawnet"]


def pw(x, h):
    p = x
    for _ in range(h - 1):
        p = p * x
    return p


def f_val(fac, K, y):
    op, sp, c, h = fac
    yh, Kh = pw(y[sp], h), pw(K[c], h)
    den = Kh + yh
    return yh / den if op == SAT else Kh / den


def f_der(fac, K, y):
    op, sp, c, h = fac
    yh, Kh = pw(y[sp], h), pw(K[c], h)
    den = Kh + yh
    num = Kh if h == 1 else (F64(h) * Kh) * pw(y[sp], h - 1)
    q = num / (den * den)
    return q if op == SAT else -q


def _vec(a):
    return [F64(v) for v in np.asarray(a, dtype=np.float64)]


def res(net, k, y, yp):
    k, y, yp = _vec(k), _vec(y), _vec(yp)
    K = k[net.nreac:]
    out = np.empty(net.n)
    with np.errstate(all="ignore"):
        for i, row in enumerate(net.rows):
            acc = F64(0.0)
            for e, (nu, r) in enumerate(row):
                g = k[r]
                for sp in net.slots[r]:
                    g = g * y[sp]
                for fac in net.factors[r]:
                    g = g * f_val(fac, K, y)
                t = nu * g
                acc = t if e == 0 else acc + t
            out[i] = net.d[i] * yp[i] - acc
    return out


def jac(net, k, cj, y):
    """J = dF/dy + cj dF/dy' -> [n][n] column-major; +0.0 at every off-diagonal position without a term."""
    k, y = _vec(k), _vec(y)
    K = k[net.nreac:]
    cj = F64(cj)
    n = net.n
    J = np.zeros((n, n))
    with np.errstate(all="ignore"):
        for i, row in enumerate(net.rows):
            acc = {}

            def add(j, term):
                acc[j] = term if j not in acc else acc[j] + term

            for nu, r in row:
                s, fs = net.slots[r], net.factors[r]
                for p, j in enumerate(s):  # one term per slot, in slot order: k times the other slots, then every f
                    g = k[r]
                    for t, sp in enumerate(s):
                        if t != p:
                            g = g * y[sp]
                    for fac in fs:
                        g = g * f_val(fac, K, y)
                    add(j, nu * g)
                for q, fq in enumerate(fs):  # one term per factor, in factor order: k times all slots, then f with df for this one
                    g = k[r]
                    for sp in s:
                        g = g * y[sp]
                    for t, fac in enumerate(fs):
                        g = g * (f_der(fac, K, y) if t == q else f_val(fac, K, y))
                    add(fq[1], nu * g)
            for j, a in acc.items():
                J[j, i] = (cj * net.d[i] if i == j else F64(0.0)) - a
            if i not in acc:
                J[i, i] = cj * net.d[i]
    return J


def dense_dq(net, k, yy, yp, ewt, rr, cj, hh):
    """idaLsDenseDQJac with res as the row function: every entry by the definition (dq_ref.dense_dq)."""
    return DQ.dense_dq(lambda y, ypv: res(net, k, y, ypv), yy, yp, ewt, rr, cj, hh)


def select(prob, ids):
    out = {k: v for k, v in prob.items() if k not in ("_net", "_lawnet")}
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
    out = {k: v for k, v in prob.items() if k not in ("_net", "_lawnet", "params", "reactions", "d", "nconst")}
    out["kind"] = "host_callback"
    out["res"] = lambda s, t, y, yp: res(net, P[s], y, yp)
    out["jac"] = lambda s, t, cj, y, yp, r: jac(net, P[s], cj, y).T  # (row, column)
    return out


# ------------------------------------------------------------------------------------------------ the reference stepper
class DirectIda(MA.DirectIda):
    """massaction_ref.DirectIda (the constraint check and the DQ switch included) with the residual and the Jacobian of this file"""

    def _res(self, tn, y, yp):
        return res(self.net, self.k, y, yp)

    def _setup(self, r):
        o = self.o
        o.set("nsetups", o.get("nsetups") + 1)
        o.set("nje", o.get("nje") + 1)
        if self.dq:
            J = dense_dq(self.net, self.k, o.getv("yy"), o.getv("yp"), o.getv("ewt"), r, o.get("cj"), o.get("hh"))
            self.nre_dq += self.net.n
        else:
            J = jac(self.net, self.k, o.get("cj"), o.getv("yy"))
        info, self.lu, self.piv = O.getrf(J.T)
        o.set("cjold", o.get("cj"))
        o.set("cjratio", 1.0)
        o.set("ss", 20.0)
        return KR.NLS_SUCCESS if info == 0 else KR.NLS_LSETUP_RECVR


RUN_CNT = MA.RUN_CNT


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


# ------------------------------------------------------------------------------------------------ the integration cases
# (n, B, touts) of idahip.problems.enzyme_chain(n, B): shared by tests/test_ratelaw_ref.py (the reference runs end well) and
# tests/test_gpu_rate_laws.py (the device against them)
CASES = {"n5": (5, 5, (0.05, 0.5)), "n9": (9, 16, (0.01, 0.02, 0.03)), "n16": (16, 67, (0.05, 0.1)), "n65": (65, 3, (0.005, 0.01))}
_CACHE = {}


def case(name, **kw):
    """(problem, touts, the reference run): computed once per process, shared and left unchanged"""
    from idahip import problems
    key = (name,) + tuple(sorted((k, tuple(v) if hasattr(v, "__len__") else v) for k, v in kw.items()))
    if key not in _CACHE:
        n, B, touts = CASES[name]
        p = problems.enzyme_chain(n, B)
        _CACHE[key] = (p, touts, run(p, touts, **kw))
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ a hand-written network, and what is refused
# species 0 sits in a slot and in a factor of reaction 0; reaction 1 reaches (2, 3) through a factor alone; reaction 2 is polynomial
HAND = [((0,), {0: -1.0, 1: 1.0}, [("sat", 0, 0, 1)]), ((), {2: 1.0}, [("inh", 3, 1, 2)]), ((1, 2), {3: 1.0})]

# the texts of idahip_set_rate_network's refusals (tests/test_gpu_rate_laws.py matches the library's against the same list)
REFUSALS = [
    ("factor 0: species 4 outside [0, 4)", dict(fac=(0, 0, ("sat", 4, 0, 1)))),
    ("factor 0: species -1 outside [0, 4)", dict(fac=(0, 0, ("sat", -1, 0, 1)))),
    ("factor 1: constant 2 outside [0, 2)", dict(fac=(1, 0, ("inh", 3, 2, 2)))),
    ("factor 1: constant -1 outside [0, 2)", dict(fac=(1, 0, ("inh", 3, -1, 2)))),
    ("factor 0: exponent 5 outside [1, 4]", dict(fac=(0, 0, ("sat", 0, 0, 5)))),
    ("factor 1: exponent 0 outside [1, 4]", dict(fac=(1, 0, ("inh", 3, 1, 0)))),
    ("factor 0: op 3 is neither IDAHIP_RATE_SAT (1) nor IDAHIP_RATE_INH (2)", dict(fac=(0, 0, (3, 0, 0, 1)))),
    ("factor 6: reaction 2 has more than 4 factors", dict(many=2)),
    ("nconst = -1 is negative", dict(nconst=-1)),
    ("reaction 2, slot 1: species 7 outside [0, 4)", dict(slot=(2, 1, 7))),
    ("entry 1: row 4 outside [0, 4)", dict(row=(0, 4))),
    ("d[2] = inf is not finite", dict(d=(2, np.inf))),
]


def refused_network(kw):
    """HAND with one thing wrong -> (reactions, d, nconst)"""
    reactions = [(list(r[0]), dict(r[1]), list(r[2]) if len(r) > 2 else []) for r in HAND]
    d, nconst = [1.0, 1.0, 1.0, 0.0], kw.get("nconst", 2)
    if "fac" in kw:
        r, q, f = kw["fac"]
        reactions[r][2][q] = f
    if "many" in kw:
        reactions[kw["many"]][2].extend([("sat", 1, 0, 1)] * 5)
    if "slot" in kw:
        r, q, sp = kw["slot"]
        reactions[r][0][q] = sp
    if "row" in kw:
        r, row = kw["row"]
        reactions[r] = (reactions[r][0], [(0, -1.0), (row, 1.0)], reactions[r][2])
    if "d" in kw:
        d[kw["d"][0]] = kw["d"][1]
    return reactions, d, nconst


def raw_arrays(reactions, d):
    """the flat arrays of idahip_set_rate_network, UNCHECKED (what flatten_laws would refuse goes through to the library):
    -> (slots, factors, rows, reacs, nu, d)"""
    R = len(reactions)
    slots = np.full((R, 3), -1, dtype=np.int32)
    fac, rows, reacs, nu = [], [], [], []
    for r, reaction in enumerate(reactions):
        for q, sp in enumerate(reaction[0]):
            slots[r, q] = sp
        for row, v in (reaction[1].items() if hasattr(reaction[1], "items") else reaction[1]):
            rows.append(row)
            reacs.append(r)
            nu.append(v)
        for op, sp, c, h in (reaction[2] if len(reaction) > 2 else []):
            fac.append((r, {"sat": SAT, "inh": INH}.get(op, op), sp, c, h))
    return (slots, np.array(fac, dtype=np.int32).reshape(-1, 5), np.array(rows, dtype=np.int32), np.array(reacs, dtype=np.int32),
            np.array(nu, dtype=np.float64), np.array(d, dtype=np.float64))
