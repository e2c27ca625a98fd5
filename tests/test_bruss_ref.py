"""tests/bruss_ref.py (the numpy restatement of IDAHIP_BRUSS1D) pinned on things independent of it, the generator
idahip.problems.bruss1d, and the conditions that keep the GPU tests from passing on a problem that has become linear in effect."""
import os
import re

import numpy as np
import pytest

import bruss_ref as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = np.array([1.25, 3.5, 4.5, 1.25, 2.8])


def state(m, seed=0):
    rng = np.random.default_rng(seed)
    n = 2 * m
    return 1.0 + rng.uniform(0.0, 2.0, n), rng.uniform(-1.0, 1.0, n)


@pytest.mark.parametrize("m", [5, 16])
def test_jac_equals_a_central_difference_of_res(m):
    y, yp = state(m, m)
    n, cj = 2 * m, 7.5
    J = BR.jac(P, cj, y)
    for j in range(n):
        h = 1.0e-5 * max(1.0, abs(y[j]))
        col = np.zeros(n)
        for sgn in (1.0, -1.0):  # dF/dy_j + cj dF/dy'_j: perturb y_j by h and y'_j by cj h
            y2, p2 = y.copy(), yp.copy()
            y2[j] += sgn * h
            p2[j] += sgn * cj * h
            col += sgn * BR.res(P, y2, p2)
        col /= 2.0 * h
        scale = np.abs(J[j]).max()
        assert np.abs(col - J[j]).max() <= 1.0e-5 * scale, (j, np.abs(col - J[j]).max(), scale)


@pytest.mark.parametrize("m", [5, 16])
def test_jac_is_exactly_zero_outside_the_band(m):
    y, _ = state(m, 3)
    n = 2 * m
    J = BR.jac(P, 2.0, y)
    i, j = np.meshgrid(np.arange(n), np.arange(n))  # J[j, i] = J(i, j)
    out = np.abs(i - j) > 2
    assert np.array_equal(J[out].view(np.uint64), np.zeros(out.sum(), dtype=np.uint64))
    assert np.count_nonzero(J[~out]) > 0
    # the in-band entries the definition does not name are +0.0 too
    assert J[3, 4].view(np.uint64) == 0 and J[6, 5].view(np.uint64) == 0  # J(4, 3) and J(5, 6), interior rows of m >= 5


@pytest.mark.parametrize("m", [5, 16, 65])
def test_residual_is_exactly_zero_at_the_boundary_state(m):
    n = 2 * m
    for p in (P, np.array([1.0, 3.0, 0.02 * (m - 1) ** 2, 1.0, 3.0])):
        y = np.empty(n)
        y[0::2], y[1::2] = p[3], p[4]
        r = BR.res(p, y, np.zeros(n))
        if p[3] == p[0] and p[4] * p[0] == p[1]:  # the steady state (ub, vb) = (a, b/a), exactly representable
            assert not r.any(), r
        else:
            assert not r[[0, 1, n - 2, n - 1]].any()


@pytest.mark.parametrize("m,batch", [(5, 3), (16, 5), (65, 2)])
def test_generator(m, batch):
    from idahip import problems
    p = problems.bruss1d(m=m, batch=batch)
    n = 2 * m
    assert p["kind"] == "bruss1d" and p["n"] == n and p["params"].shape == (batch, 5)
    assert p["rtol"] == 1.0e-6 and p["atol"].tolist() == [1.0e-8] and np.array_equal(p["touts"], [0.25, 0.5, 0.75, 1.0])
    for s in range(batch):
        a, b, d, ub, vb = p["params"][s]
        assert (a, b, d, ub, vb) == (1.0 + s / 64.0, 3.0 + s / 32.0, 0.02 * (m - 1) ** 2, a, b / a)
        y = p["yy0"][s]
        assert (y[0], y[1], y[n - 2], y[n - 1]) == (ub, vb, ub, vb)
        x = np.arange(m) / (m - 1)
        assert np.array_equal(y[2:-2:2], (ub + 0.1 * np.sin(np.pi * x))[1:-1])
        assert np.array_equal(y[3:-2:2], (vb + 0.1 * np.sin(np.pi * x))[1:-1])
        assert not p["yp0"][s][[0, 1, n - 2, n - 1]].any() and p["yp0"][s].any()
        r = BR.res(p["params"][s], y, p["yp0"][s])
        assert not r.any(), (s, np.abs(r).max())  # y'(0) makes the residual exactly zero


def test_enum_value_and_python_name():
    import idahip
    text = open(os.path.join(ROOT, "include", "ida_hip.h")).read()
    assert re.search(r"\bIDAHIP_BRUSS1D\s*=\s*5\b", text)
    assert idahip.KIND["bruss1d"] == 5 and idahip.BRUSS1D == 5


def test_twin_callbacks_restate_the_problem():
    import idahip
    from idahip import problems
    p = problems.bruss1d(m=6, batch=2)
    t = BR.twin(p, band=(3, 4))
    y, yp = state(6, 1)
    for s in range(2):
        assert np.array_equal(t["res"](s, 0.0, y, yp), BR.res(p["params"][s], y, yp))
        J = BR.jac(p["params"][s], 3.0, y)
        assert np.array_equal(t["jac"](s, 0.0, 3.0, y, yp, None), J.T)
        ab = t["bjac"](s, 0.0, 3.0, y, yp, None, None)
        assert np.array_equal(idahip.band_unpack(ab, 12, 3, 4), J.T)


def test_dense_dq_banded_is_the_definition_by_value():
    import dq_ref as DQ
    from idahip import problems
    p = problems.bruss1d(m=8, batch=2)
    for s in range(2):
        y = p["yy0"][s] * (1.0 + 0.01 * np.cos(np.arange(16)))
        yp = p["yp0"][s]
        ewt = 1.0 / (1e-6 * np.abs(y) + 1e-8)
        rr = BR.res(p["params"][s], y, yp)
        J = BR.dense_dq_banded(p["params"][s], y, yp, ewt, rr, 40.0, 1e-3)
        full = DQ.dense_dq(BR.prob_res(p, s), y, yp, ewt, rr, 40.0, 1e-3)
        assert np.array_equal(J, full)
        A = BR.jac(p["params"][s], 40.0, y)
        assert np.abs(J - A).max() <= 1e-4 * np.abs(A).max()


def test_direct_reference_run_is_nonlinear_in_effect():
    """Systems 1..5 at m = 16 to t = 0.5 through the dense direct reference: status 0, second Newton iterations happen
    (nni > nst) and an error test fails (netf >= 1), for each. System 0 (a = 1, b = 3) passes every error test (netf = 0, 28 steps,
    32 iterations), so the set starts at system 1; system 3 gives 28 steps, 36 iterations, 14 setups, one failed error test."""
    from idahip import problems
    p = BR.select(problems.bruss1d(m=16, batch=6), [1, 2, 3, 4, 5])
    ref = BR.run(p, [0.5], mode="direct")
    assert [int(ref["counters"][k][0][2]) for k in ("nst", "nni", "nsetups", "netf", "ncfn")] == [28, 36, 14, 1, 0]
    c = ref["counters"]
    assert (ref["status"] == 0).all(), ref["status"]
    print("nst", c["nst"][0], "nni", c["nni"][0], "nsetups", c["nsetups"][0], "netf", c["netf"][0], "ncfn", c["ncfn"][0])
    assert (c["nni"][0] > c["nst"][0]).all(), (c["nni"][0], c["nst"][0])
    assert (c["netf"][0] >= 1).all(), c["netf"][0]
