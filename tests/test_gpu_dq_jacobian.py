"""idahip_jac_dq and idahip_nls_lsetup_dq (difference-quotient Jacobians, dq_kernels.hpp) against tests/dq_ref.py: every problem
kind on dense and band ctxs, bit for bit (NaN against NaN); the factors of nls_lsetup_dq against the oracle's dense_get_rf of the
restated Jacobian; the counters of the host stepper; and every -2 refusal of the DQ entry points."""
import numpy as np
import pytest

import dq_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu
F_YY, F_YP, F_YYPREDICT, F_YPPREDICT, F_EWT, F_EE, F_DELTA, F_SAVRES = range(8)
LORENZ = np.array([10.0, 28.0, 8.0 / 3.0])


def same(a, b):
    """bit for bit, a NaN matching any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.where(nan, 0.0, a).view(np.uint64), np.where(nan, 0.0, b).view(np.uint64))


def state(rng, B, n, wild=True):
    """yy, yp, ewt [B][n] and hh [B]: signed values over many decades, exact zeros, tiny and huge entries; hh of both signs and 0"""
    mag = lambda: 10.0 ** rng.uniform(-3, 3, (B, n))
    yy, yp = rng.standard_normal((B, n)) * mag(), rng.standard_normal((B, n)) * mag()
    if wild:
        for a in (yy, yp):
            m = rng.random((B, n))
            a[m < 0.05] = 0.0
            a[(m >= 0.05) & (m < 0.08)] *= 1e-300
            a[(m >= 0.08) & (m < 0.10)] *= 1e12
    ewt = 1.0 / (1e-6 * np.abs(yy) + 1e-8)
    hh = np.array([(1e-3, -2e-3, 0.0, 0.37)[s % 4] for s in range(B)])
    return yy, yp, ewt, hh


class Case:
    """A ctx of one kind with its per-system data and a residual function per system (the dq_ref restatement)."""

    def __init__(self, kind, n, B, band=None, host=False, seed=0):
        import idahip
        self.kind, self.n, self.B, self.band = kind, n, B, band
        rng = np.random.default_rng(seed)
        self.rng = rng
        self.data = []
        for s in range(B):
            if kind == "lorenz63":
                self.data.append({"params": LORENZ * (1.0 + 0.01 * s)})
            elif kind == "heat1d":
                self.data.append({"coef": 1.0e3 * (1.0 + s / 7.0)})
            elif kind == "linear_dense":
                self.data.append({"A": rng.standard_normal((n, n)), "B": rng.standard_normal((n, n)), "c": rng.standard_normal(n)})
            else:
                self.data.append({})
        self.res = [R.residual_fn(kind, d) for d in self.data]
        self.ctx = idahip.Ctx("host_callback" if host else kind, n, B, band=band)
        self.ctx.set_tolerances(1e-6, [1e-8])
        if host:
            self.ctx.set_host_residual(lambda s, t, y, yp: self.res[s](y, yp))
        elif kind == "lorenz63":
            self.ctx.set_problem_params(np.stack([d["params"] for d in self.data]))
        elif kind == "heat1d":
            self.ctx.set_problem_params(np.array([[d["coef"]] for d in self.data]))
        elif kind == "linear_dense":
            self.ctx.set_linear_dense(np.stack([d["A"] for d in self.data]), np.stack([d["B"] for d in self.data]),
                                      np.stack([d["c"] for d in self.data]))

    def load(self, yy, yp, ewt, cj):
        """the state through nls_sys (yypredict = yy, ee = 0): savres is the device's residual there, pinned to dq_ref's"""
        c = self.ctx
        c.upload(F_YYPREDICT, yy); c.upload(F_YPPREDICT, yp); c.upload(F_EWT, ewt)
        c.nls_sys(0.0, cj, True)
        self.yy, self.yp = c.download(F_YY), c.download(F_YP)
        self.ewt, self.rr = ewt, c.download(F_SAVRES)
        for s in range(self.B):
            assert same(self.res[s](self.yy[s], self.yp[s]), self.rr[s]), ("residual restatement", s)

    def ref(self, s, cj, hh):
        y, yp, w, rr, d = self.yy[s], self.yp[s], self.ewt[s], self.rr[s], self.data[s]
        if self.band is not None:
            return R.band_dq(self.res[s], y, yp, w, rr, cj, hh, *self.band)
        if self.kind == "linear_dense":
            return R.linear_dense_dq(d["A"], d["B"], d["c"], y, yp, w, rr, cj, hh)
        if self.kind == "heat1d" and not self.host_kind():
            return R.heat_dense_dq_banded(d["coef"], y, yp, w, rr, cj, hh)
        return R.dense_dq(self.res[s], y, yp, w, rr, cj, hh)

    def host_kind(self):
        import idahip
        return self.ctx.kind == idahip.HOST_CALLBACK

    def close(self):
        self.ctx.close()


CASES = [
    ("roberts", 3, 64, None, False), ("lorenz63", 3, 64, None, False),
    ("linear_dense", 24, 9, None, False), ("linear_dense", 257, 3, None, False), ("linear_dense", 1100, 2, None, False),
    ("heat1d", 24, 8, None, False), ("heat1d", 257, 5, None, False), ("heat1d", 1100, 3, None, False), ("heat1d", 4096, 3, None, False),
    ("heat1d", 24, 8, (1, 1), False), ("heat1d", 257, 5, (2, 3), False), ("heat1d", 1100, 3, (1, 1), False), ("heat1d", 4096, 3, (1, 1), False),
    ("heat1d", 24, 4, None, True), ("heat1d", 257, 3, None, True), ("roberts", 3, 8, None, True),
    ("heat1d", 24, 4, (1, 1), True), ("heat1d", 257, 3, (3, 2), True), ("heat1d", 1100, 2, (1, 1), True),
]


@pytest.mark.parametrize("kind,n,B,band,host", CASES, ids=lambda v: str(v))
def test_jac_dq_matches_restatement(kind, n, B, band, host):
    cs = Case(kind, n, B, band, host, seed=n + B)
    yy, yp, ewt, hh = state(cs.rng, B, n, wild=(kind != "heat1d" or band is not None or host))
    cj = 10.0 ** cs.rng.uniform(-1, 4, B)
    cs.load(yy, yp, ewt, cj)
    rng = np.random.default_rng(7)
    for idx in (np.arange(B), rng.permutation(B), np.array([B - 1]), np.arange(0, B, 2)[::-1]):
        J = cs.ctx.jac_dq(0.0, cj[idx], hh[idx], idx)
        for q, s in enumerate(idx):
            assert same(J[q], cs.ref(s, cj[s], hh[s])), (s, q)
    cs.close()


def test_heat_dense_dq_is_the_full_definition_by_value():
    """the heat kernel writes rows j-1..j+1 only: with a consistent, finite state the rest of the definition is +-0"""
    cs = Case("heat1d", 40, 2)
    yy, yp, ewt, hh = state(cs.rng, 2, 40, wild=False)
    cs.load(yy, yp, ewt, np.array([5.0, 7.0]))
    J = cs.ctx.jac_dq(0.0, [5.0, 7.0], hh[:2])
    for s in range(2):
        full = R.dense_dq(cs.res[s], cs.yy[s], cs.yp[s], cs.ewt[s], cs.rr[s], [5.0, 7.0][s], hh[s])
        assert np.array_equal(J[s], full)
    cs.close()


@pytest.mark.parametrize("kind,n,B,band", [("roberts", 3, 16, None), ("lorenz63", 3, 16, None), ("linear_dense", 257, 4, None),
                                           ("heat1d", 1100, 4, None), ("heat1d", 2048, 3, None), ("heat1d", 1100, 4, (1, 1)),
                                           ("heat1d", 257, 4, (2, 3))])
def test_nls_lsetup_dq_factors_match_oracle(kind, n, B, band):
    import idahip
    cs = Case(kind, n, B, band, seed=3)
    yy, yp, ewt, hh = state(cs.rng, B, n, wild=False)
    cj = np.full(B, 50.0)
    cs.load(yy, yp, ewt, cj)
    cs.ctx.set_jacobian_dq(True)
    idx = np.array([B - 1] + list(range(0, B - 1, 2)), dtype=np.int32)
    off = [s for s in range(B) if s not in idx]
    before = {s: (cs.ctx.download_lu_band(s) if band else cs.ctx.download_lu(s)) for s in off}
    rc, info = cs.ctx.nls_lsetup_dq(0.0, cj[idx], hh[idx], idx)
    refs = np.stack([cs.ref(s, cj[s], hh[s]) for s in idx])
    dense = np.stack([idahip.band_unpack(r, n, *band).T for r in refs]) if band else refs
    cm = np.ascontiguousarray(dense)  # [s][j][i]: column-major storage already
    oinfo, opiv = O.getrf_batch(cm)
    assert np.array_equal(info, oinfo) and rc == (1 if oinfo.any() else 0)
    for q, s in enumerate(idx):
        if band:
            fac, piv = cs.ctx.download_lu_band(s)
            assert np.array_equal(piv, opiv[q])
            if oinfo[q] == 0:
                assert np.array_equal(idahip.band_expand_factors(fac, piv, n, *band), cm[q].T)
        else:
            lu, piv = cs.ctx.download_lu(s)
            assert np.array_equal(piv, opiv[q])
            assert np.array_equal(lu, cm[q].T)  # by value
    for s in off:  # off the list: untouched
        now = cs.ctx.download_lu_band(s) if band else cs.ctx.download_lu(s)
        assert all(np.array_equal(a, b) for a, b in zip(now, before[s]))
    cs.close()


def test_refusals():
    import idahip
    cs = Case("heat1d", 24, 2)
    c = cs.ctx
    one = np.zeros(2)
    assert not c.jacobian_dq()
    with pytest.raises(idahip.IdaHipError, match=r"\(-2\)"):
        c.nls_lsetup_dq(one, one, one)  # not a DQ ctx
    c.set_jacobian_dq(True)
    assert c.jacobian_dq()
    with pytest.raises(idahip.IdaHipError, match=r"\(-2\)"):
        c.nls_lsetup(one, one)
    with pytest.raises(idahip.IdaHipError, match=r"\(-2\)"):
        c.nls_sys_setup(one, one)
    c.set_jacobian_dq(False)
    c.nls_lsetup(one, one + 1.0)  # analytic again
    cs.close()
    h = idahip.Ctx("host_callback", 24, 2, band=(1, 1))
    with pytest.raises(idahip.IdaHipError, match=r"\(-2\)"):
        cs2 = idahip.Ctx("heat1d", 24, 2)
        try:
            cs2.set_host_residual(lambda s, t, y, yp: y)  # not a host-callback ctx
        finally:
            cs2.close()
    h.set_host_residual(lambda s, t, y, yp: y)
    assert h.jacobian_dq()
    with pytest.raises(idahip.IdaHipError, match=r"\(-2\)"):
        h.set_jacobian_dq(False)
    assert h.jacobian_dq()
    h.set_host_band_problem(lambda s, t, y, yp: y, lambda s, t, cj, y, yp, r, ab: None)  # a Jacobian again: DQ may go off
    assert h.jacobian_dq()
    h.set_jacobian_dq(False)
    assert not h.jacobian_dq()
    h.close()
    # existing registrations keep their behaviour: a NULL Jacobian is still refused
    H = idahip.load()[0]
    d = idahip.Ctx("host_callback", 24, 2)
    assert H.idahip_set_host_problem(d.h, idahip.RES_FN(lambda *a: 0), idahip.JAC_FN(), None) == -1
    d.close()


@pytest.mark.parametrize("band", [None, (1, 1), (2, 1)])
def test_host_stepper_counts_dq_evaluations(band):
    """nre_dq grows by n (dense) or min(ml + mu + 1, n) (band) per Jacobian and nre does not: with a residual-only host problem,
    every call of the user's residual is counted exactly once, in nre or in nre_dq"""
    import idahip
    from idahip import problems
    n, B = 64, 4
    p = problems.heat1d(n=n, batch=B)
    coef = p["params"][:, 0]
    calls = np.zeros(B, dtype=np.int64)

    def res(s, t, y, yp):
        calls[s] += 1
        return R.heat_res(float(coef[s]), y, yp)

    ctx = idahip.Ctx("host_callback", n, B, band=band)
    ctx.set_tolerances(p["rtol"], p["atol"])
    ctx.set_host_residual(res)
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    st, _ = ens.solve(0.02)
    assert (st == 0).all()
    c = ens.counters()
    assert (c["nje"] > 0).all()
    assert np.array_equal(c["nre_dq"], c["nje"] * R.dq_evals(n, band))
    assert np.array_equal(calls, c["nre"] + c["nre_dq"])
    assert (c["nre"] >= c["nni"]).all() and (c["nre"] < c["nre_dq"]).all()
    yy = ens.yy()
    ens.close()
    ctx.close()
    if band == (2, 1):  # the band DQ Jacobian of the heat problem equals the dense one by value (test_dq_ref.py): so does the run
        dense = idahip.Ctx("host_callback", n, B)
        dense.set_tolerances(p["rtol"], p["atol"])
        dense.set_host_residual(lambda s, t, y, yp: R.heat_res(float(coef[s]), y, yp))
        ens = idahip.Ensemble(dense, p["yy0"], p["yp0"])
        st, _ = ens.solve(0.02)
        assert (st == 0).all()
        assert np.array_equal(yy, ens.yy())  # by value
        for k in ("nst", "nje", "nsetups", "nni", "netf", "ncfn", "kused"):
            assert np.array_equal(c[k], ens.counter(k)), k
        ens.close()
        dense.close()


def test_heat_dq_setups_after_a_factorisation_that_left_the_work_matrix_zero():
    """n > 1024 with super-panels (the heat default): a factorisation leaves the work matrix all +0.0 (LuWs::jwzero), and the next
    DQ Jacobian writes only rows j-1..j+1 of each column. Three setups in a row, each against the oracle."""
    cs = Case("heat1d", 2048, 3, seed=11)
    assert cs.ctx.H.idahip_lu_superpanel(cs.ctx.h) == 1
    yy, yp, ewt, hh = state(cs.rng, 3, 2048, wild=False)
    cs.ctx.set_jacobian_dq(True)
    for cj in (50.0, 80.0, 3.0e4):
        cjs = np.full(3, cj)
        cs.load(yy, yp, ewt, cjs)
        rc, info = cs.ctx.nls_lsetup_dq(0.0, cjs, hh)
        cm = np.ascontiguousarray(np.stack([cs.ref(s, cj, hh[s]) for s in range(3)]))
        oinfo, opiv = O.getrf_batch(cm)
        assert np.array_equal(info, oinfo)
        for s in range(3):
            lu, piv = cs.ctx.download_lu(s)
            assert np.array_equal(piv, opiv[s]) and np.array_equal(lu, cm[s].T), (cj, s)
        yy = yy * 1.01
    cs.close()


def test_roberts_dq_column_error_at_late_times():
    """Why DQ Roberts stops short of 4e10 with the example's tolerances: late in the run y1 ~ 1e-8, far
    below the increment floor 1/ewt_1 ~ atol_1 = 1e-6; the residual is quadratic in y1, so the DQ column 1 carries -3e7 * inc_1
    on top of the analytic -6e7 y1 - 1e4 y2 - cj. That error is small against J(1,1) but many times larger than J(0,1) + J(1,1),
    the combination the nearly singular iteration matrix depends on (rows 0 and 1 cancel up to the y1 terms)."""
    cs = Case("roberts", 3, 1, seed=1)
    y = np.array([[4.938102e-03, 1.984924e-08, 9.950619e-01]])  # the DQ run at t = 4e5
    yp = np.array([[-1.1e-8, -4.0e-14, 1.1e-8]])
    ewt = 1.0 / (1e-4 * np.abs(y) + np.array([1e-8, 1e-6, 1e-6]))
    cj, hh = np.array([2.0e-4]), np.array([5.0e3])
    cs.load(y, yp, ewt, cj)
    J = cs.ctx.jac_dq(0.0, cj, hh)[0]
    assert same(J, cs.ref(0, cj[0], hh[0]))
    K = R.analytic_jac("roberts", {}, cj[0], cs.yy[0])
    inc1 = R.increments(cs.yy[0], cs.yp[0], ewt[0], hh[0])[1]
    assert abs(inc1) > 40 * cs.yy[0][1]  # (negative here: hh * yp_1 < 0)
    err = J[1, 1] - K[1, 1]
    assert abs(err - (-3.0e7 * inc1)) < 1e-6 * abs(K[1, 1])
    assert abs(err) > 10 * abs(K[1, 0] + K[1, 1])
