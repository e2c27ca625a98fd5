"""Difference-quotient Jacobians restated in float64 numpy: C IDA's idaLsDenseDQJac and idaLsBandDQJac (SUNDIALS ida_ls.c),
with SUNDIALS' serial N_VLinearSum case order, and the four device problems' residuals in the operation order of
rust-ida_amd/csrc/problem_kernels.hpp and oracle/problems.hpp. numpy's elementwise float64 arithmetic is IEEE with no fused
multiply-add, so every value here is what the device kernels (-ffp-contract=off) must produce, bit for bit.

Layouts: a dense Jacobian is [n][n] with J[j, i] = J(i, j) (column-major, as the library stores it); a band one is [n][ldab]
with AB[j, ml + mu + i - j] = J(i, j) (LAPACK band storage, ldab = 2 ml + mu + 1)."""
import numpy as np

SRUR = 2.0 ** -26  # sqrt(DBL_EPSILON)


def increments(yy, yp, ewt, hh):
    """inc_j = MAX(srur * MAX(|yy_j|, |hh*yp_j|), 1/ewt_j), negated when hh*yp_j < 0, then (yy_j + inc_j) - yy_j.
    MAX(a, b) = a > b ? a : b (SUNMAX: a NaN in a picks b)."""
    yy, yp, ewt = (np.asarray(v, dtype=np.float64) for v in (yy, yp, ewt))
    hh = np.float64(hh)
    with np.errstate(all="ignore"):
        ay, ah = np.abs(yy), np.abs(hh * yp)
        m = np.where(ay > ah, ay, ah)
        t, w = SRUR * m, 1.0 / ewt
        inc = np.where(t > w, t, w)
        inc = np.where(hh * yp < 0.0, -inc, inc)
        return (yy + inc) - yy


def linsum(inv, rt, r):
    """N_VLinearSum(inv, rt, -inv, r) of SUNDIALS' serial vector: VDiff for inv = +-1, VScaleSum for inv == -inv (+-0),
    VScaleDiff for every other non-NaN inv, the general form for NaN."""
    inv = np.float64(inv)
    with np.errstate(all="ignore"):
        if inv == 1.0:
            return rt - r
        if inv == -1.0:
            return r - rt
        if inv == -inv:
            return inv * (rt + r)
        if inv == inv:
            return inv * (rt - r)
        return inv * rt + (-inv) * r


# ------------------------------------------------------------------------------------------------ residuals
def roberts_res(y, yp):
    with np.errstate(all="ignore"):
        r0 = -0.04 * y[0] + 1.0e4 * y[1] * y[2]
        r1 = -r0 - 3.0e7 * y[1] * y[1] - yp[1]
        r0 = r0 - yp[0]
        r2 = y[0] + y[1] + y[2] - 1.0
    return np.array([r0, r1, r2])


def lorenz_res(prm, y, yp):
    p, r, b = (float(v) for v in prm)
    with np.errstate(all="ignore"):
        return np.array([yp[0] - p * (y[1] - y[0]), yp[1] - (y[0] * (r - y[2]) - y[1]), yp[2] - (y[0] * y[1] - b * y[2])])


def linear_res(A, B, c, yy, yp):
    """F = A y' + B y - c; A, B [n][n] column-major (A[j, i] = A(i, j)): two chains over ascending column j."""
    n = c.size
    ra, rb = np.zeros(n), np.zeros(n)
    with np.errstate(all="ignore"):
        for j in range(n):
            ra = ra + A[j] * yp[j]
            rb = rb + B[j] * yy[j]
        return (ra + rb) - c


def heat_res(coef, y, yp):
    n = y.size
    r = np.empty(n)
    with np.errstate(all="ignore"):
        r[0], r[n - 1] = y[0], y[n - 1]
        r[1:n - 1] = yp[1:n - 1] - coef * ((y[0:n - 2] - 2.0 * y[1:n - 1]) + y[2:n])
    return r


def residual_fn(kind, sysdata):
    """res(yy, yp) of one system. sysdata: dict with params / A, B, c as the kind needs."""
    if kind == "roberts":
        return roberts_res
    if kind == "lorenz63":
        return lambda y, yp: lorenz_res(sysdata["params"], y, yp)
    if kind == "linear_dense":
        return lambda y, yp: linear_res(sysdata["A"], sysdata["B"], sysdata["c"], y, yp)
    if kind == "heat1d":
        return lambda y, yp: heat_res(float(sysdata["coef"]), y, yp)
    raise ValueError(kind)


def analytic_jac(kind, sysdata, cj, yy):
    """The oracle's analytic Jacobians (oracle/problems.hpp), [n][n] column-major."""
    n = yy.size
    J = np.zeros((n, n))
    if kind == "roberts":
        J.T[:] = [[-0.04 - cj, 1.0e4 * yy[2], 1.0e4 * yy[1]], [0.04, -1.0e4 * yy[2] - 6.0e7 * yy[1] - cj, -1.0e4 * yy[1]], [1.0, 1.0, 1.0]]
    elif kind == "lorenz63":
        p, r, b = sysdata["params"]
        J.T[:] = [[p + cj, -p, 0.0], [-(r - yy[2]), 1.0 + cj, yy[0]], [-yy[1], -yy[0], b + cj]]
    elif kind == "linear_dense":
        J[:] = sysdata["B"] + cj * sysdata["A"]
    elif kind == "heat1d":
        coef = float(sysdata["coef"])
        J[0, 0] = J[n - 1, n - 1] = 1.0
        for i in range(1, n - 1):
            J[i - 1, i], J[i, i], J[i + 1, i] = -coef, cj + 2.0 * coef, -coef
    return J


# ------------------------------------------------------------------------------------------------ DQ Jacobians
def dense_dq(res, yy, yp, ewt, rr, cj, hh):
    """idaLsDenseDQJac: one residual per column, only that column perturbed. Returns [n][n] column-major."""
    yy, yp, rr = (np.asarray(v, dtype=np.float64) for v in (yy, yp, rr))
    n = yy.size
    inc = increments(yy, yp, ewt, hh)
    J = np.empty((n, n))
    for j in range(n):
        y2, p2 = yy.copy(), yp.copy()
        with np.errstate(all="ignore"):
            y2[j] = yy[j] + inc[j]
            p2[j] = yp[j] + cj * inc[j]
            inv = 1.0 / inc[j]
        J[j] = linsum(inv, res(y2, p2), rr)
    return J


def linear_dense_dq(A, B, c, yy, yp, ewt, rr, cj, hh):
    """dense_dq for F = A y' + B y - c, every column at once: the chains run over k with the operand yp 1^T, its diagonal
    replaced by the perturbed entries (the same values and order as n calls of linear_res)."""
    yy, yp, rr = (np.asarray(v, dtype=np.float64) for v in (yy, yp, rr))
    n = yy.size
    inc = increments(yy, yp, ewt, hh)
    with np.errstate(all="ignore"):
        pyy, pyp = yy + inc, yp + cj * inc
        RA, RB = np.zeros((n, n)), np.zeros((n, n))  # [j][i]: column j's chains
        for k in range(n):
            opa = np.full(n, yp[k]); opa[k] = pyp[k]
            opb = np.full(n, yy[k]); opb[k] = pyy[k]
            RA = RA + opa[:, None] * A[k][None, :]
            RB = RB + opb[:, None] * B[k][None, :]
        RT = (RA + RB) - c[None, :]
        inv = 1.0 / inc
    return np.stack([linsum(inv[j], RT[j], rr) for j in range(n)])


def heat_dense_dq_banded(coef, yy, yp, ewt, rr, cj, hh):
    """What the heat kernel writes on a dense ctx: dense_dq at rows j-1..j+1 of column j (where the perturbation reaches),
    +0.0 elsewhere -- equal by value to dense_dq wherever rr is the residual at (yy, yp) and finite."""
    yy, yp, rr = (np.asarray(v, dtype=np.float64) for v in (yy, yp, rr))
    n = yy.size
    inc = increments(yy, yp, ewt, hh)
    J = np.zeros((n, n))
    with np.errstate(all="ignore"):
        for j in range(n):
            lo, hi = max(0, j - 1), min(n - 1, j + 1)
            y2, p2 = yy[max(0, lo - 1):hi + 2].copy(), yp[max(0, lo - 1):hi + 2].copy()
            off = max(0, lo - 1)
            y2[j - off] = yy[j] + inc[j]
            p2[j - off] = yp[j] + cj * inc[j]
            inv = 1.0 / inc[j]
            for i in range(lo, hi + 1):
                if i == 0 or i == n - 1:
                    rt = y2[i - off]
                else:
                    rt = p2[i - off] - coef * ((y2[i - 1 - off] - 2.0 * y2[i - off]) + y2[i + 1 - off])
                J[j, i] = linsum(inv, np.array([rt]), np.array([rr[i]]))[0]
    return J


def band_dq(res, yy, yp, ewt, rr, cj, hh, ml, mu):
    """idaLsBandDQJac: min(ml + mu + 1, n) groups, each one residual with all its columns perturbed. Returns [n][ldab]."""
    yy, yp, rr = (np.asarray(v, dtype=np.float64) for v in (yy, yp, rr))
    n = yy.size
    width, kv, ldab = ml + mu + 1, ml + mu, 2 * ml + mu + 1
    inc = increments(yy, yp, ewt, hh)
    AB = np.zeros((n, ldab))
    with np.errstate(all="ignore"):
        for g in range(min(width, n)):
            cols = np.arange(g, n, width)
            y2, p2 = yy.copy(), yp.copy()
            y2[cols] = yy[cols] + inc[cols]
            p2[cols] = yp[cols] + cj * inc[cols]
            rt = res(y2, p2)
            for j in cols:
                i1, i2 = max(0, j - mu), min(n - 1, j + ml)
                rows = np.arange(i1, i2 + 1)
                AB[j, kv + rows - j] = (1.0 / inc[j]) * (rt[rows] - rr[rows])
    return AB


def dq_evals(n, band=None):
    """Residual evaluations of one DQ Jacobian (C IDA's nreDQ increment)."""
    return n if band is None else min(band[0] + band[1] + 1, n)
