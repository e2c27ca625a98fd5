"""The cases of the root-finding tests, shared by the CPU census (tests/test_roots_oracle.py) and the GPU tests (tests/test_gpu_roots.py).
TEST INFRASTRUCTURE ONLY.

A case is a problem of idahip.problems, its touts and the components whose functions g_i = y[comp_i] - thr_i are watched; a variant
adds stop times, a function that is exactly zero at t0, masked norms or another number of functions. Thresholds are not constants here:
for system 0 the oracle runs once without roots to the last tout and thr_i = 0.5 * (y0[comp_i] + y_end[comp_i]), the same for every
system of the batch. Stop times come from each system's own root times in the oracle's roots-only run.

A run is driven as tests/tstop_cases.py drives its runs -- through stop(values) and solve(tout, itask) -> statuses, which the harness
(HarnessDriver) and the product (ProductDriver) both implement -- and leaves the list of ops for a replay on the other.
"""
import numpy as np

import roots_oracle as RO
import tstop_cases as K
import tstop_oracle as T

NAN = float("nan")
MAX_RETURNS = 12  # per tout: at most five roots, a stop time, the tout itself; then something is wrong

# name -> (components, device stepper of the problem: 1 = one thread per system, 2 = lock-step rounds)
CASES = {
    "roberts": ([0, 2], 1),
    "roberts012": ([0, 1, 2], 1),
    "lorenz": ([0, 1, 2], 1),
    "linear24": ([1, 13, 23], 2),
    # stride passes 0, 2, 4 of a 64-lane workgroup, lanes 1, 13, 43. (With system 0's thresholds for the whole batch, [1, 151, 299] leaves
    # system 1 without a root; component 141 crosses its threshold in all three systems.)
    "linear300": ([1, 141, 299], 2),
    "heat20": ([1, 10, 18], 2),
    "heat1100": ([1, 550, 1098], 2),  # the n > 1024 round path
}
LINEAR24_FIVE = [1, 13, 23, 5, 7]
VARIANTS = ("plain", "tstop", "zero_at_t0")
_CACHE = {}


def _problem(name):
    from idahip import problems
    if name in ("roberts", "roberts012"):
        return K.roberts_batch(70), [0.4, 0.8, 1.6]
    if name == "lorenz":
        return problems.lorenz63(batch=70), [0.1, 0.2, 0.4]
    if name == "linear24":
        return problems.linear_dense(n=24, batch=7, procs=1), [0.1, 0.2, 0.4]
    if name == "linear300":
        return problems.linear_dense(n=300, batch=3), [0.1, 0.2, 0.4]
    if name == "heat20":
        return problems.heat1d(n=20, batch=3), [0.1, 0.2, 0.4]
    if name == "heat1100":
        return problems.heat1d(n=1100, batch=2), [0.1, 0.2]
    raise KeyError(name)


def problem(name):
    if ("problem", name) not in _CACHE:
        _CACHE["problem", name] = _problem(name)
    return _CACHE["problem", name]


def thresholds(name, comps):
    """0.5 * (y0 + y(last tout)) of system 0 at comps, from the oracle without roots (one run per problem)."""
    prob, touts = problem(name)
    pname = "roberts" if name == "roberts012" else name
    if ("yend", pname) not in _CACHE:
        h = RO.Harness(prob, 0, roots=([], []))
        st, _ = h.solve(touts[-1])
        assert st == T.SUCCESS, st
        _CACHE["yend", pname] = h.getv("yy")
    return [0.5 * (float(prob["yy0"][0, c]) + float(_CACHE["yend", pname][c])) for c in comps]


def case(name, variant="plain", nroots=None):
    """-> {"name", "prob", "touts", "roots": (comps, thr), "how": the harness' switches, "id", "stops": [batch] or None, "stepper"}.
    variant: "plain" | "tstop" | "zero_at_t0" | "masked"; nroots (linear24 only): the first nroots of LINEAR24_FIVE."""
    key = ("case", name, variant, nroots)
    if key in _CACHE:
        return _CACHE[key]
    prob, touts = problem(name)
    comps, stepper = CASES[name]
    if nroots is not None:
        assert name == "linear24"
        comps = LINEAR24_FIVE[:nroots]
    thr = [1e-4, 0.01] if name == "roberts" else thresholds(name, comps)  # roberts: the reference example's two functions
    c = {"name": "%s/%s%s" % (name, variant, "" if nroots is None else "/%d" % nroots), "prob": prob, "touts": touts, "id": None,
         "stops": None, "stepper": stepper, "how": {}}
    if variant == "zero_at_t0":
        thr = [float(prob["yy0"][0, comps[0]])] + thr[1:]
    elif variant == "masked":
        c["id"] = K.third_algebraic(prob["n"])
        c["how"] = {"id": c["id"], "suppress": True}
    c["roots"] = (list(comps), thr)
    c["how"]["roots"] = c["roots"]
    if variant == "tstop":
        c["stops"] = stop_times(root_times(name))
    _CACHE[key] = c
    return c


def root_times(name):
    """Per system the tret of every ROOT return of the oracle's own roots-only run."""
    plain = case(name)
    rec = reference(plain, ops_on_harness(plain))
    B = plain["prob"]["yy0"].shape[0]
    return [[float(r["tret"][b]) for r in rec if r["status"][b] == T.ROOT_RETURN] for b in range(B)]


def stop_times(times):
    """By b % 4: none, 0.9 * t_root1, t_root1 exactly, midway between the first and the last root time."""
    out = np.full(len(times), NAN)
    for b, t in enumerate(times):
        assert len(t) >= 1, "system %d has no root return" % b
        out[b] = (NAN, 0.9 * t[0], t[0], 0.5 * (t[0] + t[-1]))[b % 4]
    return out


def all_cases():
    """Every (name, variant, nroots) the tests run."""
    out = [(n, v, None) for n in CASES for v in VARIANTS]
    out += [("linear24", "masked", None), ("roberts", "masked", None)]
    out += [("linear24", "plain", k) for k in (1, 4, 5)]
    return out


def drive(c, d, max_returns=MAX_RETURNS):
    """Every tout until no system reports a root or a stop time any more. -> the ops made, in order."""
    ops = []
    if c["stops"] is not None:
        ops.append(("stop", np.array(c["stops"], dtype=np.float64)))
        d.stop(c["stops"])
    for t in c["touts"]:
        for _ in range(max_returns):
            ops.append(("solve", float(t), T.NORMAL))
            st = d.solve(float(t), T.NORMAL)
            if ((st == T.SUCCESS) | (st < 0)).all():
                break
        else:
            raise AssertionError("%s: no end of returns at tout %g: %s" % (c["name"], t, st))
    return ops


class HarnessDriver(K.HarnessDriver):
    def __init__(self, c):
        prob = c["prob"]
        self.B = prob["yy0"].shape[0]
        self.ids = list(range(self.B))
        self.hs = [RO.Harness(prob, s, **c["how"]) for s in self.ids]


def ops_on_harness(c):
    """The case's ops as the harness itself drives them (the CPU census; the GPU tests replay the product's ops instead)."""
    return drive(c, HarnessDriver(c))


def ops_key(ops):
    return tuple((o[0], o[1] if o[0] != "stop" else None if o[1] is None else o[1].tobytes()) + tuple(map(str, o[2:])) for o in ops)


def reference(c, ops):
    """The oracle's records of the ops (tstop_oracle.run_ops' records plus iroots and nge), one run per (case, ops)."""
    key = ("ref", c["name"], ops_key(ops))
    if key not in _CACHE:
        _CACHE[key] = RO.run_ops(c["prob"], ops, **c["how"])[0]
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ the product behind the same interface
class ProductDriver(K.ProductDriver):
    """tstop_cases.ProductDriver whose records also hold roots_found() and the root-function evaluations."""

    def __init__(self, ens, max_rounds=0):
        K.ProductDriver.__init__(self, ens)
        self.max_rounds = max_rounds  # > 0: every solve is one round-limited call, status 99 for the systems still inside it

    def solve(self, tout, itask):
        e = self.ens
        before = e.stop_time()
        st, tret = e.solve(tout, itask=itask, max_rounds=self.max_rounds)
        r = {"status": st.copy(), "tret": tret.copy(), "yy": e.yy(), "yp": e.yp(), "tstop": e.stop_time(), "tstop_before": before,
             "iroots": e.roots_found().copy(), "nge": e.counter("nge")}
        for k in ("tn", "hh", "hused"):
            r[k] = e.real(k)
        for k in K.INT_FIELDS:
            r[k] = e.counter(k)
        self.rec.append(r)
        return st


def compare(got, want, by_value=False, what=""):
    """tstop_cases.compare, plus rootsfound and the root-function evaluations at every return. No tolerances."""
    K.compare(got, want, by_value=by_value, what=what)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g["iroots"], w["iroots"]), (what, i, "iroots", g["iroots"], w["iroots"])
        assert np.array_equal(g["nge"], w["nge"].astype(np.int64)), (what, i, "nge", g["nge"], w["nge"])
