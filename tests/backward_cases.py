"""The cases of the tests that integrate in the negative time direction (tout < t0, hh < 0), shared by the CPU census
(tests/test_backward_oracle.py) and the GPU tests (tests/test_gpu_backward.py). TEST INFRASTRUCTURE ONLY.

A case is a problem of idahip.problems, a list of descending touts (t0 = 0, every tout < 0) and, by variant, root functions, stop
times, an id vector, constraints, DQ Jacobians or a band / Krylov form. Runs are driven through the interface of tests/tstop_cases.py
and tests/roots_cases.py (stop / stop_rel / solve), recorded by `Product` (roots_cases.ProductDriver plus the remaining counters) and
compared with reinit_oracle.compare; there is no second harness here. Two references stand behind that one record format:

  * "oracle": oracle/ida.hpp through reinit_oracle.Harness (roots, stop times, masked norms) for Roberts, Lorenz63, linear dense, heat;
  * "python": the restated stepper of tests/krylov_ref.py (`PyIda`: any residual, the analytic, dense-DQ or band-DQ Jacobian, a
    constraint vector; `krylov_ref.RefIda` / `krylov_prec_ref.RefIda` themselves for a Krylov ctx) for the kinds the oracle does not
    have -- the Brusselator, reaction networks -- and for DQ, constraints and Krylov on every kind. It has no roots and no stop time.

Mirrored twins. Integrating most of these problems backwards is the unstable direction, so where the parameters allow it the case is
the MIRRORED problem, mirror(P): the problem whose backward solution is P's forward solution reflected in time, y_m(-t) = y(t),
y_m'(-t) = -y'(t). heat: coef -> -coef; linear dense: A -> -A; networks: every rate constant negated; y0' negated in all of them.
Lorenz63, Roberts and the Brusselator cannot be mirrored through their parameters: their horizons are short enough for the oracle.
Negation is exact in IEEE arithmetic, so a forward run of P to +T and a backward run of mirror(P) to -T agree bit for bit in yy and
every counter, with tn, hh, hused, tret and yp negated -- `MIRROR_EXACT` lists the kinds for which tests/test_backward_oracle.py
establishes this on the references, and `mirrored()` is the comparison.
"""
import numpy as np

import dq_ref as DQ
import krylov_ref as KR
import massaction_ref as MA
import oracle_lib as O
import reinit_oracle as RI
import roots_cases as RC
import stepper_ref as R
import tstop_cases as K
import tstop_oracle as T

NAN = float("nan")
_CACHE = {}
# name -> (reference, device stepper: 1 = one thread per system, 2 = lock-step rounds, band widths or None, touts)
CASES = {
    "lorenz": ("oracle", 1, None, [-0.05, -0.1, -0.2]),       # B = 70: more than one wavefront of the one-thread stepper
    "roberts": ("oracle", 1, None, [-0.02, -0.04, -0.08]),
    "linear24": ("oracle", 2, None, [-0.1, -0.2, -0.4]),      # mirrored
    "heat20": ("oracle", 2, (1, 1), [-0.1, -0.2, -0.4]),      # mirrored
    "heat20_twin": ("oracle", 0, None, [-0.1, -0.2, -0.4]),   # the mirrored heat problem written out as host callbacks
    "bruss6": ("python", 2, (2, 2), [-0.1, -0.2, -0.4]),
    "chain12": ("python", 2, None, [-0.01, -0.02, -0.03]),    # mirrored
}
# the kinds whose mirror property tests/test_backward_oracle.py finds exact on the references (all that can be mirrored)
MIRROR_EXACT = ("linear24", "heat20", "heat20_twin", "chain12")
ROOT_COMPS = {"lorenz": [0, 1, 2], "roberts": [2, 1], "linear24": [1, 13, 23], "heat20": [1, 10, 18], "heat20_twin": [1, 10, 18]}
# Roberts' systems start from different y0: fixed thresholds that every system's y2 and y1 cross on the way to t = -0.08. (Not y0:
# next to 1 a threshold is met to the bit over more than the root tolerance at these small |t|, which is CLOSE_ROOTS at the next call.)
ROOT_THR = {"roberts": [-4.0e-4, -3.0e-5]}
FLIP = ("tret", "tn", "hh", "hused", "yp")  # what a mirrored run negates; everything else is equal


# ------------------------------------------------------------------------------------------------ problems and their mirrors
def mirror(prob):
    """mirror(P) of a generated problem: see the module docstring. Involutive: mirror(mirror(P)) is P, bit for bit."""
    q = {k: v for k, v in prob.items() if k != "_net"}
    q["yp0"] = -prob["yp0"]
    if prob["kind"] == "heat1d":
        q["params"] = -prob["params"]
    elif prob["kind"] == "linear_dense":
        q["A"] = -prob["A"]
    elif prob["kind"] == "mass_action" and "nconst" not in prob:
        q["params"] = -prob["params"]
    else:
        raise ValueError("%s cannot be mirrored through its parameters" % prob["kind"])
    return q


def heat_callbacks(coef):
    """The heat problem's residual and dense Jacobian by hand, coef [B] of either sign (oracle/problems.hpp's operation order)."""
    def res(s, t, y, yp):
        return DQ.heat_res(float(coef[s]), y, yp)

    def jac(s, t, cj, y, yp, r):
        return DQ.analytic_jac("heat1d", {"coef": coef[s]}, cj, y).T  # (row, column)

    return res, jac


def forward_problem(name):
    """The problem a case is built from, as idahip.problems generates it (for the mirrorable kinds: the P of mirror(P))."""
    from idahip import problems
    if ("fwd", name) not in _CACHE:
        _CACHE["fwd", name] = {
            "lorenz": lambda: problems.lorenz63(batch=70),
            "roberts": lambda: K.roberts_batch(8),
            "linear24": lambda: problems.linear_dense(n=24, batch=7, procs=1),
            "heat20": lambda: problems.heat1d(n=20, batch=3),
            "heat20_twin": lambda: problems.heat1d(n=20, batch=3),
            "bruss6": lambda: problems.bruss1d(m=6, batch=4),
            "chain12": lambda: problems.reaction_chain(12, 6),
        }[name]()
    return _CACHE["fwd", name]


def problem(name):
    """The problem the backward run integrates (the oracle's description; product_problem is what make_ctx takes)."""
    if ("prob", name) not in _CACHE:
        p = forward_problem(name)
        _CACHE["prob", name] = mirror(p) if name in MIRROR_EXACT else p
    return _CACHE["prob", name]


def product_problem(name, prob=None):
    prob = problem(name) if prob is None else prob
    if name != "heat20_twin":
        return prob
    res, jac = heat_callbacks(prob["params"][:, 0])
    q = {k: v for k, v in prob.items() if k != "params"}
    q.update(kind="host_callback", res=res, jac=jac)
    return q


# ------------------------------------------------------------------------------------------------ the python reference
class _Size:
    def __init__(self, n):
        self.n = n


class PyIda(MA.DirectIda):
    """massaction_ref.DirectIda -- krylov_ref.RefIda(direct=True) with constr_ref's constraint check -- with its two hooks replaced:
    any residual res(y, yp), and as Jacobian jac(cj, y) -> [n][n] column-major, or dq = "dense" / (ml, mu) for dq_ref's difference
    quotients (a band one is unpacked and factored densely: equal by value to the band kernels). dq_signs collects
    sign(hh * yp_j) at every DQ Jacobian for the census."""

    def __init__(self, n, res, jac, yy0, yp0, rtol, atol, dq=None, constr=None, mxstep=500):
        MA.DirectIda.__init__(self, _Size(n), np.zeros(0), yy0, yp0, rtol, atol, constr=constr, dq=dq, mxstep=mxstep)
        self.res_fn, self.jac_fn = res, jac
        self.dq_signs = []

    def _res(self, tn, y, yp):
        return self.res_fn(y, yp)

    def _jacobian(self, r):
        import idahip
        o = self.o
        if self.dq is None:
            return self.jac_fn(o.get("cj"), o.getv("yy"))
        a = (self.res_fn, o.getv("yy"), o.getv("yp"), o.getv("ewt"), r, o.get("cj"), o.get("hh"))
        self.dq_signs.append(np.sign(o.get("hh") * o.getv("yp")))
        self.nre_dq += DQ.dq_evals(self.n, None if self.dq == "dense" else self.dq)
        if self.dq == "dense":
            return DQ.dense_dq(*a)
        return idahip.band_unpack(DQ.band_dq(*a, *self.dq), self.n, *self.dq).T


def res_jac_of(prob, s):
    """(res(y, yp), jac(cj, y)) of system s of a generated problem, every kind the cases use."""
    kind = prob["kind"]
    if kind == "bruss1d":
        import bruss_ref as BR
        p = prob["params"][s]
        return (lambda y, yp: BR.res(p, y, yp)), (lambda cj, y: BR.jac(p, cj, y))
    if kind == "mass_action":
        net, k = MA._net(prob), prob["params"][s]
        return (lambda y, yp: MA.res(net, k, y, yp)), (lambda cj, y: MA.jac(net, k, cj, y))
    data = {"params": prob["params"][s]} if "params" in prob else {}
    if kind == "heat1d":
        data = {"coef": prob["params"][s, 0]}
    for key in ("A", "B", "c"):
        if key in prob:
            data[key] = prob[key][s]
    return DQ.residual_fn(kind, data), (lambda cj, y: DQ.analytic_jac(kind, data, cj, y))


def py_systems(prob, how):
    """how: {"dq": None | "dense" | (ml, mu), "constr": c | None, "krylov": None | "plain" | (ml, mu), "mxstep"}."""
    import krylov_prec_ref as PR
    B = prob["yy0"].shape[0]
    a = lambda s: (prob["yy0"][s], prob["yp0"][s], prob["rtol"], prob["atol"])
    mx = how.get("mxstep", 500)
    if how.get("krylov") is not None:
        assert prob["kind"] == "heat1d"
        if how["krylov"] == "plain":
            return [KR.RefIda("heat1d", prob["n"], *a(s), maxl=5, mxstep=mx, params=prob["params"][s]) for s in range(B)]
        return [PR.RefIda("heat1d", prob["n"], *a(s), *how["krylov"], maxl=5, mxstep=mx, params=prob["params"][s]) for s in range(B)]
    return [PyIda(prob["n"], *res_jac_of(prob, s), *a(s), dq=how.get("dq"), constr=how.get("constr"), mxstep=mx) for s in range(B)]


KRYLOV_COUNTERS = ("nre_dq", "nli", "ncfl", "npe", "nps")


def py_state(s):
    o = s.o
    d = {k: o.get(k) for k in T.SCALARS + RI.EXTRA_COUNTERS}
    d["yy"], d["yp"] = o.getv("yy"), o.getv("yp")
    d["tstop"], d["iroots"], d["nge"] = NAN, np.zeros(0, dtype=np.int32), 0.0
    for k in KRYLOV_COUNTERS:
        d[k] = float(getattr(s, k, 0))
    return d


def py_reference(prob, ops, how):
    """The solve ops on the python reference -> (records shaped like tstop_oracle.run_ops', the systems)."""
    sy = py_systems(prob, how)
    rec = []
    for op in ops:
        assert op[0] == "solve", "the python reference has no stop time"
        out = [s.solve(op[1], op[2]) for s in sy]
        sts = [py_state(s) for s in sy]
        r = {"status": np.array([o[0] for o in out], dtype=np.int32), "tret": np.array([o[1] for o in out])}
        for k in sts[0]:
            r[k] = np.array([st[k] for st in sts])
        rec.append(r)
    return rec, sy


# ------------------------------------------------------------------------------------------------ cases
def end_values(name, tout):
    """yy [B][n] of the oracle's run without roots at tout (one call)."""
    key = ("end", name, tout)
    if key not in _CACHE:
        prob = problem(name)
        hs = [RI.Harness(prob, s, roots=([], [])) for s in range(prob["yy0"].shape[0])]
        for h in hs:
            st, _ = h.solve(tout)
            assert st == T.SUCCESS, (name, st)
        _CACHE[key] = np.array([h.getv("yy") for h in hs])
    return _CACHE[key]


def case(name, variant="plain"):
    """-> {"name", "prob", "touts", "roots", "how", "id", "stops", "stepper", "ref", "band", "script"}.
    variant: "plain" | "roots" (thr_i midway between system 0's y0 and y(last tout)) | "root_at_tout" (the first function's threshold
    is system 0's y(touts[0]) itself: its root lies exactly at that tout) | "roots_tstop" | "masked" | "tstop" | "entry"."""
    key = ("case", name, variant)
    if key in _CACHE:
        return _CACHE[key]
    ref, stepper, band, touts = CASES[name]
    prob = problem(name)
    c = {"name": "%s/%s" % (name, variant), "kind": name, "prob": prob, "touts": list(touts), "id": None, "stops": None, "stepper": stepper,
         "ref": ref, "band": band, "roots": ([], []), "how": {}, "script": None}
    if variant in ("roots", "root_at_tout", "roots_tstop", "masked"):
        assert ref == "oracle"
        comps = ROOT_COMPS[name]
        y0, yend = prob["yy0"][0], end_values(name, touts[-1])[0]
        thr = list(ROOT_THR.get(name, ())) or [0.5 * (float(y0[i]) + float(yend[i])) for i in comps]
        if variant == "root_at_tout":
            thr[0] = float(end_values(name, touts[0])[0][comps[0]])
        c["roots"] = (list(comps), thr)
        if variant == "masked":
            c["id"] = K.third_algebraic(prob["n"])
            c["how"] = {"id": c["id"], "suppress": True}
    elif variant in ("tstop", "entry"):
        c["script"] = "residues" if variant == "tstop" else "entry"
    elif variant != "plain":
        raise KeyError(variant)
    if ref == "oracle":
        c["how"]["roots"] = c["roots"]
    if variant == "roots_tstop":
        c["stops"] = RC.stop_times(root_times(name))
    _CACHE[key] = c
    return c


def root_times(name):
    """Per system the tret of every ROOT return of the oracle's own run of the "roots" case."""
    c = case(name, "roots")
    rec = reference(c, ops_on_harness(c))
    B = c["prob"]["yy0"].shape[0]
    return [[float(r["tret"][b]) for r in rec if r["status"][b] == T.ROOT_RETURN] for b in range(B)]


def drive(c, d):
    """The case's script on a driver -> the ops made: tstop_cases.drive for a stop-time script, roots_cases.drive otherwise."""
    if c["script"] is not None:
        return K.drive(c, d)
    if c["name"].endswith("/root_at_tout"):
        # A root exactly at tout is reported at every call with that tout, without end and in either direction: r_check2 finds g = 0 at
        # tlo = tout and g != 0 next to it, r_check3 then looks at thi = tout again (oracle/ida.hpp restates impl_r_check.rs here, and
        # so does the library). At most four calls per tout, as tstop_cases.drive makes them.
        ops = []
        for t in c["touts"]:
            for _ in range(4):
                ops.append(("solve", float(t), T.NORMAL))
                st = d.solve(float(t), T.NORMAL)
                if ((st == T.SUCCESS) | (st < 0)).all():
                    break
        return ops
    return RC.drive(c, d)


class HarnessDriver(K.HarnessDriver):
    def __init__(self, c):
        prob = c["prob"]
        self.B = prob["yy0"].shape[0]
        self.ids = list(range(self.B))
        self.hs = [RI.Harness(prob, s, **c["how"]) for s in self.ids]


def ops_on_harness(c):
    """The case's ops as the oracle harness itself drives them (the CPU census; the GPU tests replay the product's ops instead)."""
    return drive(c, HarnessDriver(c))


def plain_ops(c, itask=T.NORMAL):
    return [("solve", float(t), itask) for t in c["touts"]]


def reference(c, ops, how=None):
    """The reference's records of the ops, one run per (case, ops, how); how: the python reference's switches (py_systems)."""
    key = ("ref", c["name"], RC.ops_key(ops), repr(how))
    if key not in _CACHE:
        if c["ref"] == "oracle" and not how:
            _CACHE[key] = T.run_ops(c["prob"], ops, harness=RI.Harness, **c["how"])
        else:
            _CACHE[key] = py_reference(c["prob"], ops, how or {})
    return _CACHE[key][0]


def reference_systems(c, ops, how=None):
    reference(c, ops, how)
    return _CACHE["ref", c["name"], RC.ops_key(ops), repr(how)][1]


# ------------------------------------------------------------------------------------------------ the product behind the same interface
class Product(RC.ProductDriver):
    """roots_cases.ProductDriver whose records also hold reinit_oracle's extra counters and the Krylov / DQ ones."""

    def solve(self, tout, itask=T.NORMAL):
        st = RC.ProductDriver.solve(self, tout, itask)
        for k in RI.EXTRA_COUNTERS + KRYLOV_COUNTERS:
            self.rec[-1][k] = self.ens.counter(k)
        return st


def compare(got, want, by_value=False, what="", krylov=False):
    """reinit_oracle.compare: status, tret, yy, yp, tn, hh, hused, tstop, kused, nst, nre, nni, netf, ncfn, nsetups, iroots, nge, nje,
    n_attempts, nls_nconvfails at every call; krylov: nre_dq, nli, ncfl, npe, nps as well. No tolerances."""
    RI.compare(got, want, by_value=by_value, what=what)
    if krylov:
        for i, (g, w) in enumerate(zip(got, want)):
            for k in KRYLOV_COUNTERS:
                assert np.array_equal(g[k], w[k].astype(np.int64)), (what, i, k, g[k], w[k])


def mirrored(fwd, bwd, what=""):
    """Records of a forward run of P and of the backward run of mirror(P) with the touts negated: every field equal bit for bit,
    the FLIP fields negated -- those by value, since a zero that comes out of a sum (y' = 0 at the heat problem's ends, hused before
    the first step) is +0.0 on both sides."""
    assert len(fwd) == len(bwd)
    for i, (f, b) in enumerate(zip(fwd, bwd)):
        for k in f:
            if k in ("tstop", "tstop_before"):
                continue
            fv, bv = np.asarray(f[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)
            assert np.array_equal(-fv, bv) if k in FLIP else R.same_bits(fv, bv), (what, i, k, fv, bv)


def constraint_how():
    """heat20 with every temperature >= 0: the profile of the (mirrored) heat problem decays towards the ends, where the
    constraint becomes active and steps are corrected."""
    return {"constr": np.ones(20)}


def lorenz_constraint_case():
    """The first eight Lorenz systems with y1 >= 0 and mxstep = 80, two calls with tout = -0.05: going backwards y1 falls through zero
    near t = -0.03, the constraint becomes active, steps are corrected and recovered, and the calls end with TOO_MUCH_WORK (heat20's
    constrained run is the one that finishes). The case of the one-thread device stepper, which checks constraints itself."""
    if "lorenz8" not in _CACHE:
        c = dict(case("lorenz"))
        p = dict(c["prob"])
        for k in ("yy0", "yp0", "params"):
            p[k] = np.ascontiguousarray(p[k][:8])
        c.update(name="lorenz8/constr", prob=p, touts=[-0.05, -0.05])
        _CACHE["lorenz8"] = c
    return _CACHE["lorenz8"], {"constr": np.array([0.0, 1.0, 0.0]), "mxstep": 80}


def forward_case(name):
    """The forward twin of a mirrored case: P itself, the touts negated."""
    assert name in MIRROR_EXACT
    c = dict(case(name))
    c.update(name="%s/forward" % name, prob=forward_problem(name), touts=[-t for t in c["touts"]])
    return c


def harness_get_dky(h, t, k):
    """Ida::get_dky(t, k) of a harness' oracle object -> (status, dky [n])."""
    import ctypes as C
    out = np.zeros(h.n)
    h.L.oracle_ida_get_dky.argtypes = [C.c_void_p, C.c_double, C.c_int, O.dp, C.c_int]
    h.L.oracle_ida_get_dky.restype = C.c_int
    return h.L.oracle_ida_get_dky(h.h, float(t), int(k), O._ptr(out), 0), out


def calcic_reference(name):
    """tests/calcic_ref.py on a case of tests/calcic_cases.py with its tout1 negated (hic < 0, cj < 0); computed once."""
    import calcic_cases as CK
    import calcic_ref as IC
    if ("calcic", name) not in _CACHE:
        c = CK.case(name)
        B = c["yy0"].shape[0]
        _CACHE["calcic", name] = IC.calc_ic_batch([CK.ref_problem(c, b) for b in range(B)], c["yy0"], c["yp0"], c["rtol"], c["atol"], c["icopt"],
                                                  -c["tout1"], id=c["id"])
    return _CACHE["calcic", name]
