"""Inputs of the IDACalcIC tests (test_calcic_ref.py on the CPU, test_gpu_calc_ic.py on the GPU) and their reference results,
computed once per process with calcic_ref and shared. Every case is a dict
    kind, n, band (None or (ml, mu)), dq, icopt, id, rtol, atol, tout1, yy0 [B][n], yp0 [B][n], data (what make_ctx needs)
Shapes are the smallest that reach each code path: n <= 8 (one thread per system), 8 < n <= 64 (one wavefront's diagonal block),
65 and 257 (more than one 64-column block, more than one pass of a 256-thread workgroup), odd and even n (the solves' vector width).

TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import calcic_ref as IC


def _rng(*key):
    return np.random.Generator(np.random.PCG64(list(key)))


def roberts(vector_atol):
    B = 64
    u = _rng(1, 3).uniform(0.05, 1.0, size=B)
    yy0 = np.stack([1.0 - 1.0e-3 * u, 1.0e-5 * u, 0.5 * u], axis=1)
    atol = np.array([1.0e-8, 1.0e-14, 1.0e-6]) if vector_atol else np.array([1.0e-8])
    return {"kind": "roberts", "n": 3, "band": None, "dq": False, "icopt": IC.YA_YDP_INIT, "id": np.array([1.0, 1.0, 0.0]),
            "rtol": 1.0e-4, "atol": atol, "tout1": 0.4, "yy0": yy0, "yp0": np.zeros((B, 3)), "data": {}}


def lorenz():
    from idahip import problems
    p = problems.lorenz63(batch=16)
    return {"kind": "lorenz63", "n": 3, "band": None, "dq": False, "icopt": IC.YA_YDP_INIT, "id": np.ones(3), "rtol": p["rtol"],
            "atol": p["atol"], "tout1": 0.1, "yy0": p["yy0"], "yp0": np.zeros((16, 3)), "data": {"params": p["params"]}}


def linear(n, pattern, icopt=IC.YA_YDP_INIT, dq=False, B=None):
    """F = A y' + B y - c with A = diag(id) (I + small coupling) -- singular in the algebraic rows --, B diagonally dominant,
    random y0. pattern: "one_alg" (one algebraic component), "one_diff" (all but one), "mixed" (every third algebraic).
    Y_INIT: y0' is given (random) and y0 is solved for."""
    B = B or (4 if n >= 257 else 16)
    id_ = {"one_alg": np.ones(n), "one_diff": np.zeros(n), "mixed": np.where(np.arange(n) % 3 == 2, 0.0, 1.0)}[pattern].copy()
    if pattern == "one_alg":
        id_[n // 2] = 0.0
    if pattern == "one_diff":
        id_[n // 3] = 1.0
    A, Bm, c, yy0, yp0 = (np.empty(s) for s in ((B, n, n), (B, n, n), (B, n), (B, n), (B, n)))
    for b in range(B):
        g = _rng(2, n, b)
        M = np.eye(n) + (0.05 / np.sqrt(n)) * g.uniform(-1.0, 1.0, size=(n, n))
        Al = id_[:, None] * M                                   # logical (row, column)
        Bl = -((0.5 / np.sqrt(n)) * g.standard_normal(size=(n, n)))
        Bl[np.arange(n), np.arange(n)] -= 1.0 + g.uniform(0.0, 1.0)
        A[b], Bm[b] = Al.T, Bl.T                                # column-major per system
        c[b] = g.uniform(-1.0, 1.0, size=n)
        yy0[b] = g.uniform(-1.0, 1.0, size=n)
        yp0[b] = g.uniform(-1.0, 1.0, size=n) if icopt == IC.Y_INIT else 0.0
    return {"kind": "linear_dense", "n": n, "band": None, "dq": dq, "icopt": icopt, "id": id_, "rtol": 1.0e-6,
            "atol": np.array([1.0e-8]), "tout1": 0.1, "yy0": yy0, "yp0": yp0, "data": {"A": A, "B": Bm, "c": c}}


def heat(n, band=None, dq=False):
    from idahip import problems
    B = 4
    p = problems.heat1d(n=n, batch=B)
    x = np.arange(n) / (n - 1.0)
    id_ = np.ones(n)
    id_[0] = id_[-1] = 0.0
    return {"kind": "heat1d", "n": n, "band": band, "dq": dq, "icopt": IC.YA_YDP_INIT, "id": id_, "rtol": p["rtol"], "atol": p["atol"],
            "tout1": 0.1, "yy0": np.tile(np.sin(np.pi * x) + 0.1, (B, 1)), "yp0": np.zeros((B, n)), "data": {"params": p["params"]}}


# ---- the two-unknown host-callback DAE of the line-search and failure cases: F = (y1' + y1 - z, g(z)), id = (1, 0)
LS_NAMES = ("converges", "backtracks", "conv_fail", "linesearch_fail", "no_recovery")


def ls_res(sys, t, y, yp):
    if sys == 3:
        g = y[1] * y[1] + 1.0  # no root
    else:
        g = np.arctan(y[1]) - 0.3
    return np.array([yp[0] + y[0] - y[1], g])


def ls_jac(sys, t, cj, y, yp, rr):
    """[n][n] (row, column)"""
    if sys == 4:
        d = 0.0  # the algebraic row is zero: a singular Jacobian whatever the step size
        z = 0.0
    elif sys == 3:
        d, z = 2.0 * y[1], -1.0
    else:
        d, z = 1.0 / (1.0 + y[1] * y[1]), -1.0
    return np.array([[cj + 1.0, z], [0.0, d]])


def linesearch():
    z0 = np.array([0.5, 3.0, 1.0, 2.0, 0.5])
    return {"kind": "host_callback", "n": 2, "band": None, "dq": False, "icopt": IC.YA_YDP_INIT, "id": np.array([1.0, 0.0]),
            "rtol": 1.0e-6, "atol": np.array([1.0e-8]), "tout1": 1.0, "yy0": np.stack([np.ones(5), z0], axis=1),
            "yp0": np.zeros((5, 2)), "data": {"res": ls_res, "jac": ls_jac}}


CASES = {
    "roberts_satol": lambda: roberts(False),
    "roberts_vatol": lambda: roberts(True),
    "lorenz": lorenz,
    "heat9": lambda: heat(9), "heat16": lambda: heat(16), "heat65": lambda: heat(65),
    "heat9_band": lambda: heat(9, band=(1, 1)), "heat16_band": lambda: heat(16, band=(1, 1)), "heat65_band": lambda: heat(65, band=(1, 1)),
    "linear40_yinit": lambda: linear(40, "mixed", icopt=IC.Y_INIT),
    "linear40_mixed": lambda: linear(40, "mixed"),
    "linear9_dq": lambda: linear(9, "one_alg", dq=True),
    "heat16_band_dq": lambda: heat(16, band=(1, 1), dq=True),
    "linesearch": linesearch,
}
for _n in (9, 40, 65, 257):
    for _pat in ("one_alg", "one_diff"):
        CASES["linear%d_%s" % (_n, _pat)] = (lambda n=_n, pat=_pat: linear(n, pat))

DENSE_DEVICE = [k for k in CASES if k != "linesearch" and not k.endswith("_dq") and "band" not in k]
BAND = ["heat9_band", "heat16_band", "heat65_band"]
DQ = ["linear9_dq", "heat16_band_dq"]
# the systems that may fail in the reference: the three failure cases of the line-search batch, and nothing else
EXPECTED_FAILURES = {"linesearch": {2: IC.CONV_FAIL, 3: IC.LINESEARCH_FAIL, 4: IC.NO_RECOVERY}}


# ---- batches with mixed fates on the device kinds (their trials run in the fused kernels): systems that converge, backtrack, retry
# at a smaller step size and fail side by side, with a different step size hic -- so a different cj -- in every system
def bruss_mixed():
    """bruss1d(m = 16) with Y_INIT: y'(0) the problem's own (non-zero: hic differs per system), y(0) scaled componentwise by
    1 + 0.1 m_s U(-1, 1) with a magnitude m_s per system, from a nudge to a guess far outside the basin of attraction."""
    from idahip import problems
    mags = np.array([0.01, 0.1, 0.5, 2.5, 2.5, 4.0, 8.0, 2.5, 9.9])
    p = problems.bruss1d(m=16, batch=mags.size)
    u = _rng(5, 16, 19).uniform(-1.0, 1.0, size=p["yy0"].shape)
    return {"kind": "bruss1d", "n": 32, "band": None, "dq": False, "icopt": IC.Y_INIT, "id": None, "rtol": p["rtol"], "atol": p["atol"],
            "tout1": 0.25, "yy0": p["yy0"] * (1.0 + 0.1 * mags[:, None] * u), "yp0": p["yp0"].copy(), "data": {"params": p["params"]}}


def heat_mixed(n, B, hard):
    """heat1d with YA_YDP_INIT: the systems `hard` start as the heat cases above do (sin + 0.1 with y' = 0: their first step size
    fails and they retry at hic/10), every other one from the generator's own consistent values, with its non-zero y'(0)."""
    from idahip import problems
    c = heat(n)
    p = problems.heat1d(n=n, batch=B)
    yy0, yp0 = p["yy0"].copy(), p["yp0"].copy()
    for b in hard:
        yy0[b], yp0[b] = c["yy0"][0], 0.0
    return dict(c, yy0=yy0, yp0=yp0, data={"params": p["params"]})


def linear_singular(n, sys, row):
    """linear(n, "mixed") with a zero row in A and in B of one system: its Jacobian is singular at every step size."""
    c = linear(n, "mixed")
    d = {k: v.copy() for k, v in c["data"].items()}
    d["A"][sys, :, row] = 0.0  # column-major per system: [j][i]
    d["B"][sys, :, row] = 0.0
    return dict(c, data=d)


def linear_inf(n, sys, comp):
    """linear(n, "mixed") with y_comp(0) = +inf in one system: its weight there is +0.0."""
    c = linear(n, "mixed")
    yy0 = c["yy0"].copy()
    yy0[sys, comp] = np.inf
    return dict(c, yy0=yy0)


def linear_big(n, B):
    """linear(n, "mixed") at the benchmark's size, B systems, from a non-zero y'(0) in the differential components"""
    c = linear(n, "mixed")
    yp0 = np.stack([c["id"] * _rng(6, n, b).uniform(-50.0, 50.0, size=n) * (1.0 + 10.0 * b) for b in range(B)])
    return dict(c, yy0=c["yy0"][:B], yp0=yp0, data={k: v[:B] for k, v in c["data"].items()})


MIXED = {
    "bruss32_mixed": bruss_mixed,
    "heat65_mixed": lambda: heat_mixed(65, 5, (1, 3)),
    "linear40_singular": lambda: linear_singular(40, 5, 17),
    "linear40_inf": lambda: linear_inf(40, 3, 11),
    "linear512_mixed": lambda: linear_big(512, 4),
    "heat1030": lambda: heat_mixed(1030, 2, (1,)),
}


# every status of the reference on them (test_calcic_ref.py asserts these and the properties each case is there for)
MIXED_STATUS = {
    "bruss32_mixed": [0, 0, 0, IC.CONV_FAIL, IC.CONV_FAIL, IC.CONV_FAIL, IC.LINESEARCH_FAIL, 0, IC.CONV_FAIL],
    "heat65_mixed": [0] * 5,
    "linear40_singular": [0] * 5 + [IC.NO_RECOVERY] + [0] * 10,
    "linear40_inf": [0] * 3 + [IC.BAD_EWT] + [0] * 12,
    "linear512_mixed": [0] * 4,
    "heat1030": [0] * 2,
}


@functools.lru_cache(maxsize=None)
def case(name):
    return (CASES.get(name) or MIXED[name])()


def sysdata(c, b):
    d = c["data"]
    if c["kind"] == "linear_dense":
        return {"A": d["A"][b], "B": d["B"][b], "c": d["c"][b]}
    if c["kind"] == "lorenz63":
        return {"params": d["params"][b]}
    if c["kind"] == "heat1d":
        return {"coef": d["params"][b, 0]}
    if c["kind"] == "bruss1d":
        return {"params": d["params"][b]}
    if c["kind"] == "mass_action":  # a network with rate laws ("nconst") is ratelaw_ref's, a plain one massaction_ref's
        import massaction_ref
        import ratelaw_ref
        M = ratelaw_ref if "nconst" in d else massaction_ref
        if "_net" not in c:
            c["_net"] = M.Net(dict(d, n=c["n"]))
        return {"ref": M, "net": c["_net"], "k": d["params"][b]}
    return {}


def ref_problem(c, b):
    if c["kind"] == "host_callback":
        n = c["n"]
        res = lambda y, yp: np.asarray(c["data"]["res"](b, 0.0, y, yp), dtype=np.float64)
        # the library's matrix is column-major: J[j, i] = J(i, j)
        jac = lambda cj, y, yp, rr, hic, ewt: np.ascontiguousarray(np.asarray(c["data"]["jac"](b, 0.0, cj, y, yp, rr), dtype=np.float64).reshape(n, n).T)
        return IC.Problem(n, res, jac)
    return IC.device_problem(c["kind"], c["n"], sysdata(c, b), dq=c["dq"], band=c["band"] if c["dq"] else None)


@functools.lru_cache(maxsize=None)
def reference(name):
    """calcic_ref on every system of the case; computed once, never modified by the tests."""
    c = case(name)
    B = c["yy0"].shape[0]
    r = IC.calc_ic_batch([ref_problem(c, b) for b in range(B)], c["yy0"], c["yp0"], c["rtol"], c["atol"], c["icopt"], c["tout1"], id=c["id"])
    for v in (r["status"], r["yy"], r["yp"], r["hic"]) + tuple(r["counters"].values()):
        v.setflags(write=False)
    return r


def make_ctx(c):
    """The device context of a case (GPU tests)."""
    import idahip
    from idahip import problems
    B = c["yy0"].shape[0]
    prob = dict(c["data"], kind=c["kind"], n=c["n"], yy0=c["yy0"], rtol=c["rtol"], atol=c["atol"])
    ctx = problems.make_ctx(prob, band=c["band"] if c["band"] else False)
    assert ctx.batch == B
    if c["dq"]:
        ctx.set_jacobian_dq(True)
    if c["id"] is not None:
        ctx.set_id(c["id"])
    return ctx
