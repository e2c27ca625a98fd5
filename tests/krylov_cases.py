"""The cases of tests/test_krylov_ref.py (census) and tests/test_gpu_krylov.py: inputs of the SPGMR solve of DESIGN.md section 4h for an
ensemble of B = 5 systems, and the short integrations of the host stepper. Input generation only (numpy, idahip.problems); the
parameters were picked by running tests/krylov_ref.py until its census showed every branch (test_krylov_ref.py keeps checking that).

A solve case is (kind, n, maxl). System b of the five gets its own tn, cj and heat coefficient kappa/dx^2, and one recipe:
  0  a random right-hand side, tol = (sqrt(n) 0.05) 0.33: what the stepper asks for -- on the stiff heat Jacobian GMRES(maxl) does not
     get there (RES_REDUCED)
  1  the same right-hand side scaled by 1e-13: beta <= tol, the zero-iteration return
  2  a loose tol = 0.3 beta: convergence after a few columns
  3  heat: kappa = 0 and b = e_j, so that J v0 = cj v0 exactly, V1 vanishes and the Givens case t2 == 0 is taken (rho = 0: converged);
     linear dense: recipe 0 with tol = 1e-3 beta
  4  heat: b = e_j next to a component with a weight 1e10 times larger: t1/t2 ~ 1e-10, s = -1 exactly, rho == beta: with maxl = 1 the
     solve ends in CONV_FAIL; linear dense: recipe 0 with tol = 1e-9 beta
QRSOL_FAIL needs an exactly singular Hessenberg matrix after a reduction of the residual and is not met.
"""
import numpy as np

import krylov_ref as KR
import stepper_ref as R

B = 5


def idx_for(maxl):
    """The list of a solve test: it skips one system and reorders the others (two lists, so that every recipe reaches the device)."""
    return np.array([4, 0, 3, 1] if maxl != 5 else [2, 4, 1, 3], dtype=np.int32)


NS = (9, 63, 64, 65, 257, 300)
MAXLS = (1, 5, 16)
HEAT_COEF = np.array([4.0e2, 1.0, 3.0e4, 0.0, 2.0e6])  # kappa/dx^2 per system, growing stiffness (system 3: kappa = 0)


def solve_cases():
    """(kind, n, maxl) for every kind, n and maxl of the issue (maxl > n is refused: n = 9 takes 1 and 5 only)."""
    return [(kind, n, maxl) for kind in ("heat1d", "linear_dense") for n in NS for maxl in MAXLS if maxl <= n]


def problem(kind, n):
    from idahip import problems
    if kind == "heat1d":
        p = problems.heat1d(n=n, batch=B)
        p["params"] = HEAT_COEF.reshape(B, 1).copy()
        y = p["yy0"][0]
        p["yp0"][:] = 0.0
        p["yp0"][:, 1:-1] = HEAT_COEF[:, None] * ((y[None, :-2] - 2.0 * y[None, 1:-1]) + y[None, 2:])
        return p
    return problems.linear_dense(n=n, batch=B)


def solve_inputs(kind, n, maxl):
    """-> dict(prob, yy, yp, ewt, savres [B][n], tn, cj, tol [B], b [B][n]) by system id."""
    prob = problem(kind, n)
    rng = np.random.Generator(np.random.PCG64(1000 * n + maxl + (7 if kind == "heat1d" else 0)))
    yy = prob["yy0"] + 1.0e-3 * rng.uniform(-1.0, 1.0, size=(B, n))
    yp = prob["yp0"] + 1.0e-3 * rng.uniform(-1.0, 1.0, size=(B, n))
    ewt = np.stack([R.ewt_set(yy[s], prob["rtol"], prob["atol"]) for s in range(B)])
    tn = 0.01 * (1.0 + np.arange(B))
    cj = 50.0 * (1.0 + np.arange(B))
    rhs = rng.uniform(-1.0, 1.0, size=(B, n)) / ewt
    tol = np.full(B, KR.eplin(n, 0.33))
    j = n // 2
    if kind == "heat1d":
        rhs[3] = 0.0
        rhs[3, j] = 1.0 / ewt[3, j]
        rhs[4] = 0.0
        rhs[4, j] = 1.0 / ewt[4, j]
        ewt[4, j + 1] = 1.0e10 * ewt[4, j]
    rhs[1] = 1.0e-13 * rhs[0]
    savres = np.stack([KR.make_res(prob, s)(tn[s], yy[s], yp[s]) for s in range(B)])
    beta = np.array([np.sqrt(KR.kdot(ewt[s] * rhs[s], ewt[s] * rhs[s])) for s in range(B)])
    tol[2] = 0.3 * beta[2]
    if kind != "heat1d":
        tol[3] = 1.0e-3 * beta[3]
        tol[4] = 1.0e-9 * beta[4]
    return {"prob": prob, "yy": yy, "yp": yp, "ewt": ewt, "savres": savres, "tn": tn, "cj": cj, "tol": tol, "b": rhs}


_REF = {}


def solve_reference(kind, n, maxl):
    """The reference's solve of every system of the case, computed once -> (inputs, [result dict per system], census)."""
    key = (kind, n, maxl)
    if key not in _REF:
        c = solve_inputs(kind, n, maxl)
        census = KR.new_census()
        out = [KR.spgmr_solve(KR.make_res(c["prob"], s), c["b"][s], c["ewt"][s], c["yy"][s], c["yp"][s], c["savres"][s], c["tn"][s],
                              c["cj"][s], c["tol"][s], maxl, census) for s in range(B)]
        _REF[key] = (c, out, census)
    return _REF[key]


# ---- whole integrations on the host stepper: (kind, n, maxl), B = 6 with per-system parameters, three outputs. Unpreconditioned
# GMRES(5) does not get a linear dense index-1 DAE through (every system ends in CONV_FAIL after ten recoveries); n = 12 runs with
# maxl = n (all six finish, no linear failure), n = 70 with maxl = 16 (one finishes after four recoveries, five end in CONV_FAIL);
# heat n = 65 recovers from up to five linear failures per system and finishes.
STEP_B = 6
STEP_CASES = (("heat1d", 16, 5), ("heat1d", 65, 5), ("linear_dense", 12, 12), ("linear_dense", 70, 16))


def step_problem(kind, n):
    from idahip import problems
    if kind == "heat1d":
        p = problems.heat1d(n=n, batch=STEP_B)
        kappa = 0.02 * (1.0 + np.arange(STEP_B))  # mild enough for GMRES(5) to get through, stiff enough for linear failures
        dx = 1.0 / (n - 1)
        coef = kappa / (dx * dx)
        y = p["yy0"][0]
        p["params"] = coef.reshape(STEP_B, 1)
        p["yp0"][:] = 0.0
        p["yp0"][:, 1:-1] = coef[:, None] * ((y[None, :-2] - 2.0 * y[None, 1:-1]) + y[None, 2:])
        p["touts"] = np.array([0.002, 0.004, 0.006])
        return p
    p = problems.linear_dense(n=n, batch=STEP_B)
    p["touts"] = np.array([0.02, 0.04, 0.06])
    return p


_STEP_REF = {}


def step_reference(kind, n, maxl):
    key = (kind, n, maxl)
    if key not in _STEP_REF:
        p = step_problem(kind, n)
        _STEP_REF[key] = (p, KR.run(p, p["touts"], maxl=maxl))
    return _STEP_REF[key]
