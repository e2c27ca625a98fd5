"""CPU checks of tests/dq_ref.py, the restatement of C IDA's difference-quotient Jacobians that the GPU tests compare against:
hand-checked increments and N_VLinearSum cases, and DQ close to the oracle's analytic Jacobians for the four device problems."""
import numpy as np

import dq_ref as R


def test_increment_zero_state_is_inverse_weight():
    inc = R.increments([0.0, 0.0], [0.0, 0.0], [4.0, 0.5], 0.1)
    assert inc.tolist() == [0.25, 2.0]


def test_increment_sign_follows_hh_times_yp():
    # hh*yp < 0 flips the sign; the sign comes from the product, not from yp alone
    inc = R.increments([0.0, 0.0, 0.0, 0.0], [1.0, -1.0, 1.0, -1.0], [1.0] * 4, np.array(1.0))
    assert inc.tolist() == [1.0, -1.0, 1.0, -1.0]
    inc = R.increments([0.0, 0.0], [1.0, -1.0], [1.0, 1.0], -1.0)
    assert inc.tolist() == [-1.0, 1.0]
    inc = R.increments([0.0, 0.0], [1.0, -1.0], [1.0, 1.0], 0.0)  # hh*yp = +-0: not < 0
    assert inc.tolist() == [1.0, 1.0]


def test_increment_uses_srur_times_max():
    y, yp, hh = 3.0e9, 1.0, 1.0
    inc = R.increments([y], [yp], [1.0e30], hh)[0]
    assert inc == (y + R.SRUR * y) - y
    inc = R.increments([1.0], [1.0e12], [1.0e30], 2.0)[0]
    assert inc == (1.0 + R.SRUR * 2.0e12) - 1.0


def test_increment_is_representable_difference():
    # at large |yy_j| the increment is rounded through yy_j: (yy_j + inc) - yy_j != inc
    y = 1.0e17  # srur * y = 1.49e9 = 1/ewt's competitor; ulp(y) = 16, so the raw increment is rounded
    raw = R.SRUR * y
    inc = R.increments([y], [0.0], [1.0], 0.1)[0]
    assert inc != raw and inc == (y + raw) - y


def test_linsum_cases():
    rt, r = np.array([5.0, -2.0]), np.array([3.0, 7.0])
    assert R.linsum(1.0, rt, r).tolist() == [2.0, -9.0]
    assert R.linsum(-1.0, rt, r).tolist() == [-2.0, 9.0]
    assert R.linsum(0.5, rt, r).tolist() == [1.0, -4.5]
    z = R.linsum(0.0, rt, r)  # inv = +0: VScaleSum, 0 * (rt + r)
    assert z.tolist() == [0.0, 0.0] and not np.signbit(z).any()
    z = R.linsum(-0.0, rt, r)
    assert np.signbit(z).all()
    n = R.linsum(np.nan, rt, r)
    assert np.isnan(n).all()
    # VScaleSum (inv = +-0) multiplies the sum: an infinite sum gives NaN where the difference would give 0 * 0
    big = np.array([1.7e308])
    assert np.isnan(R.linsum(0.0, big, big)).all()


def test_inv_exactly_one_takes_the_difference():
    # ewt = 1, y = 0, yp = 0: inc = 1, inv = 1 -> rtemp - rr exactly, no multiplication
    res = lambda y, yp: np.array([y[0] * 3.0 + yp[0], y[0] - 2.0 * yp[0]])
    yy, yp, ewt = np.zeros(2), np.zeros(2), np.ones(2)
    rr = res(yy, yp)
    J = R.dense_dq(res, yy, yp, ewt, rr, 0.5, 0.1)
    assert J[0].tolist() == [3.5, 0.0]
    # hh*yp < 0 with |inc| = 1: inv = -1 -> rr - rtemp
    yp2 = np.array([-1.0, 0.0])
    J = R.dense_dq(res, yy, yp2, ewt, res(yy, yp2), 0.5, 0.1)
    assert R.increments(yy, yp2, ewt, 0.1)[0] == -1.0
    assert J[0].tolist() == [3.5, 0.0]


def test_nan_in_yp_propagates():
    res = R.roberts_res
    yy, yp = np.array([1.0, 1e-5, 0.0]), np.array([np.nan, 0.0, 0.0])
    J = R.dense_dq(res, yy, yp, np.ones(3) * 1e4, res(yy, yp), 10.0, 1e-3)
    assert np.isnan(J[0]).any()  # the NaN column (inc falls back to 1/ewt; the residual carries the NaN)
    assert np.isfinite(J[1][1:]).all()


def _rng_state(rng, n):
    yy = rng.standard_normal(n)
    yp = rng.standard_normal(n)
    ewt = 1.0 / (1e-6 * np.abs(yy) + 1e-8)
    return yy, yp, ewt


def _close(J, K, tol):
    scale = np.maximum(np.abs(K).max(), 1.0)
    return np.abs(J - K).max() <= tol * scale


def test_dq_close_to_analytic_roberts_lorenz():
    rng = np.random.default_rng(1)
    for kind, data in (("roberts", {}), ("lorenz63", {"params": np.array([10.0, 28.0, 8.0 / 3.0])})):
        res = R.residual_fn(kind, data)
        for _ in range(5):
            yy, yp, ewt = _rng_state(rng, 3)
            cj, hh = 200.0, 1e-3
            J = R.dense_dq(res, yy, yp, ewt, res(yy, yp), cj, hh)
            K = R.analytic_jac(kind, data, cj, yy)
            assert _close(J, K, 1e-6), (kind, J, K)


def test_dq_close_to_analytic_linear_dense():
    rng = np.random.default_rng(2)
    n = 24
    A, B, c = rng.standard_normal((n, n)), rng.standard_normal((n, n)), rng.standard_normal(n)
    data = {"A": A, "B": B, "c": c}
    yy, yp, ewt = _rng_state(rng, n)
    rr = R.linear_res(A, B, c, yy, yp)
    J = R.linear_dense_dq(A, B, c, yy, yp, ewt, rr, 50.0, 0.02)
    assert _close(J, R.analytic_jac("linear_dense", data, 50.0, yy), 1e-6)
    # the all-columns form is the per-column definition, bit for bit
    J2 = R.dense_dq(R.residual_fn("linear_dense", data), yy, yp, ewt, rr, 50.0, 0.02)
    assert np.array_equal(J.view(np.uint64), J2.view(np.uint64))


def test_dq_heat_dense_and_band():
    rng = np.random.default_rng(3)
    n, coef = 40, 1.7e3
    data = {"coef": coef}
    res = R.residual_fn("heat1d", data)
    yy, yp, ewt = _rng_state(rng, n)
    rr = res(yy, yp)
    J = R.dense_dq(res, yy, yp, ewt, rr, 1.0e3, -1e-3)
    K = R.analytic_jac("heat1d", data, 1.0e3, yy)
    assert _close(J, K, 1e-6)
    # what the device heat kernel writes: the same values (zeros by value off the band)
    Jb = R.heat_dense_dq_banded(coef, yy, yp, ewt, rr, 1.0e3, -1e-3)
    assert np.array_equal(J, Jb)
    on = np.abs(np.subtract.outer(np.arange(n), np.arange(n))) <= 1
    assert np.array_equal(J[on].view(np.uint64), Jb[on].view(np.uint64))
    for ml, mu in ((1, 1), (2, 3), (5, 1)):
        AB = R.band_dq(res, yy, yp, ewt, rr, 1.0e3, -1e-3, ml, mu)
        kv = ml + mu
        for j in range(n):
            for i in range(max(0, j - mu), min(n, j + ml + 1)):
                assert AB[j, kv + i - j] == J[j, i], (ml, mu, i, j)
        assert R.dq_evals(n, (ml, mu)) == ml + mu + 1


def test_band_dq_groups_share_one_residual():
    # a residual that couples column j to row j + width: the band DQ sees group neighbours' perturbations (C IDA's behaviour)
    n, ml, mu = 12, 1, 1
    calls = []

    def res(y, yp):
        calls.append(1)
        return y + np.roll(y, 3) + yp

    yy, yp, ewt = np.arange(n, dtype=float), np.ones(n), np.ones(n)
    AB = R.band_dq(res, yy, yp, ewt, res(yy, yp), 2.0, 0.1, ml, mu)
    assert len(calls) == 1 + 3
    inc = R.increments(yy, yp, ewt, 0.1)
    y2, p2 = yy.copy(), yp.copy()
    y2[0::3] = yy[0::3] + inc[0::3]  # group 0: columns 0, 3, 6, 9 (width 3)
    p2[0::3] = yp[0::3] + 2.0 * inc[0::3]
    rt = y2 + np.roll(y2, 3) + p2
    rr = yy + np.roll(yy, 3) + yp
    assert AB[0, ml + mu] == (1.0 / inc[0]) * (rt[0] - rr[0])


def test_roberts_dq_column_error_at_late_times():
    # late in the Roberts run y1 ~ 2e-8 lies far below the increment floor 1/ewt_1 ~ atol_1 = 1e-6, and the residual is quadratic in
    # y1: DQ's J(1,1) carries -3e7 * inc_1 (30 here), many times J(0,1) + J(1,1), on which the iteration matrix's conditioning rests
    y = np.array([4.938102e-03, 1.984924e-08, 9.950619e-01])
    yp = np.array([-1.1e-8, -4.0e-14, 1.1e-8])
    ewt = 1.0 / (1e-4 * np.abs(y) + np.array([1e-8, 1e-6, 1e-6]))
    cj, hh = 2.0e-4, 5.0e3
    J = R.dense_dq(R.roberts_res, y, yp, ewt, R.roberts_res(y, yp), cj, hh)
    K = R.analytic_jac("roberts", {}, cj, y)
    inc1 = R.increments(y, yp, ewt, hh)[1]
    err = J[1, 1] - K[1, 1]
    assert abs(err + 3.0e7 * inc1) < 1e-9 * abs(K[1, 1])
    assert abs(err) > 20 * abs(K[1, 0] + K[1, 1])
    assert abs(J[0] - K[0]).max() < 1e-6 * abs(K[0]).max()  # the other columns are accurate
