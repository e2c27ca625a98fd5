"""Band contexts (idahip_create_band) at bandwidths other than (1, 1), against the oracle: the ctx setups through band callbacks
and through the heat band Jacobian kernel, the Newton body (idahip_newton_iter, idahip_newton_iter2), the launch widths of the
band kernels, and whole integrations on the host stepper and on the device lock-step stepper.

(1, 1) takes the register kernels and runs beside the other widths as the control; every other width takes the generic kernels
(band_getrf_kernel, band_getrs_generic inside band_newton_iter_kernel<-1, -1>). The linear problems are band_problems.py's,
whose Jacobians make partial pivoting swap rows, so that U's fill above the mu-th super-diagonal -- the top ml rows of the ctx's
band storage -- is non-zero (tests/test_band_problems.py asserts that on the oracle; the tests here assert it again on the
oracle's pivots of the very matrices they factor).

Comparisons follow the contract at the top of csrc/band_kernels.hpp: pivots, info, counters, kused, hused, orders and every
weighted norm bit-identical; factors, solutions, delta, ee, y and y' equal by value (-0.0 == +0.0); a system off a list
unchanged bit for bit. No tolerance appears anywhere."""
import numpy as np
import pytest

import band_problems as BP
import dq_ref as DQ
import oracle_lib as O
import stepper_ref as SR
from test_gpu_band_stepper import integrate_and_compare
from test_gpu_stepper_entry_points import rhs_of

pytestmark = pytest.mark.gpu

VEC = ("yy", "yp", "yypredict", "yppredict", "ewt", "ee", "delta", "savres")
HEAT_WIDTHS = [c for c in BP.setup_cases() if c[1] >= 1 and c[2] >= 1 and c != (4096, 1, 1)]


def fid(name):
    import idahip
    return {"yy": idahip.F_YY, "yp": idahip.F_YP, "yypredict": idahip.F_YYPREDICT, "yppredict": idahip.F_YPPREDICT, "ewt": idahip.F_EWT,
            "ee": idahip.F_EE, "delta": idahip.F_DELTA, "savres": idahip.F_SAVRES}[name]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def signed_zeros(rng, x):
    """x with runs of +0.0 and -0.0 entries"""
    u = rng.random(x.shape)
    return np.where(u < 0.1, 0.0, np.where(u < 0.2, -0.0, x))


def lists_of(B):
    """Two permuted partial lists over B >= 3 systems: the first leaves system 1 off, the second is shorter and overlaps it."""
    first = [s for s in range(B - 1, -1, -1) if s != 1]
    first[1:] = first[:0:-1]          # B = 5: [4, 0, 2, 3]
    second = [1, B - 1] if B == 3 else [2, 1, B - 1]
    return np.array(first, dtype=np.int32), np.array(second, dtype=np.int32)


class Case:
    """A band ctx, a host mirror of its vectors and the oracle's factors of every system set up so far."""

    def __init__(self, ctx, n, band, B, seed):
        self.ctx, self.n, self.band, self.B = ctx, n, band, B
        self.rng = np.random.default_rng(seed)
        rng = self.rng
        self.v = {f: rng.standard_normal((B, n)) for f in VEC}
        self.v["ewt"] = rng.uniform(0.5, 2.0, (B, n))
        self.v["ee"] = signed_zeros(rng, 1.0e-3 * rng.standard_normal((B, n)))
        for f in VEC:
            ctx.upload(fid(f), self.v[f])
        self.fac = {}   # system -> (oracle's dense factors, logical [n][n]; pivots)
        self.raw = [self.storage(s) for s in range(B)]

    def close(self):
        self.ctx.close()

    def storage(self, s):
        return self.ctx.download_lu_band(int(s))

    def set_ee(self, ee):
        self.v["ee"] = ee
        self.ctx.upload(fid("ee"), ee)

    def residual(self, s, yy, yp):
        raise NotImplementedError

    def jac(self, s, cj):
        raise NotImplementedError

    def expect_sys(self, idx, cjs, reset):
        """idaNlsResidual of the listed systems on the mirror"""
        for q, s in enumerate(idx):
            if reset:
                self.v["ee"][s] = np.zeros(self.n)
            self.v["yy"][s] = self.v["yypredict"][s] + self.v["ee"][s]
            self.v["yp"][s] = self.v["yppredict"][s] + cjs[q] * self.v["ee"][s]
            r = self.residual(s, self.v["yy"][s], self.v["yp"][s])
            self.v["delta"][s], self.v["savres"][s] = r, r.copy()

    def check_vectors(self, what):
        for f in VEC:
            got = self.ctx.download(fid(f))
            for s in range(self.B):
                assert SR.same_bits(got[s], self.v[f][s]), (what, f, s)

    def check_factors(self, idx, cjs, info, what, want_info=None):
        """The listed systems' pivots, info and factors against the oracle's getrf of the dense Jacobians; every other system's
        storage and pivots as they were, bit for bit."""
        import idahip
        n, (ml, mu) = self.n, self.band
        cm = np.ascontiguousarray(np.stack([self.jac(s, cjs[q]) for q, s in enumerate(idx)]))
        oinfo, opiv = O.getrf_batch(cm)
        assert np.array_equal(info, oinfo), (what, info, oinfo)
        if want_info is not None:
            assert np.array_equal(oinfo, want_info), (what, oinfo)
        ii, jj = np.indices((n, n)) if n <= 1100 else (None, None)
        for q, s in enumerate(idx):
            ab, piv = self.storage(s)
            self.raw[s] = (ab, piv)
            if oinfo[q] != 0:
                self.fac.pop(int(s), None)
                continue
            assert np.array_equal(piv, opiv[q]), (what, s)
            assert np.array_equal(idahip.band_expand_factors(ab, piv, n, ml, mu), cm[q].T), (what, s)  # by value
            if ml >= 1 and mu >= 1 and self.pivoting:  # not vacuous: rows were swapped and U filled above its mu-th super-diagonal
                assert (opiv[q] != np.arange(n)).any(), (what, s)
                if ii is not None and mu < n - 1:
                    assert np.any(cm[q].T[(jj - ii) > mu]), (what, s)
            self.fac[int(s)] = (cm[q].T, opiv[q])
        self.check_others(idx, what)
        return oinfo

    def check_others(self, idx, what):
        for s in np.setdiff1d(np.arange(self.B), idx):
            ab, piv = self.storage(s)
            assert np.array_equal(bits(ab), bits(self.raw[s][0])) and np.array_equal(piv, self.raw[s][1]), (what, s)

    def cjs(self, m):
        return 10.0 ** self.rng.uniform(0.5, 3.5, m)

    def newton(self, ids, delta, ee, scale, what):
        """idahip_newton_iter of the listed (factored) systems against stepper_ref.newton_iter on the oracle's dense factors"""
        self.v["delta"] = delta.copy()
        self.ctx.upload(fid("delta"), delta)
        self.set_ee(ee.copy())
        dn = self.ctx.newton_iter(scale, ids)
        got_d, got_e = self.ctx.download(fid("delta")), self.ctx.download(fid("ee"))
        for q, s in enumerate(ids):
            lu, piv = self.fac[int(s)]
            d, e, nrm = SR.newton_iter(lu, piv, delta[s], ee[s], self.v["ewt"][s], scale[q])
            assert np.isfinite(d).all()
            assert np.array_equal(got_d[s], d) and np.array_equal(got_e[s], e), (what, s)  # by value
            assert SR.same_bits(np.float64(dn[q]), np.float64(nrm)), (what, s, dn[q], nrm)
            self.v["delta"][s], self.v["ee"][s] = got_d[s], got_e[s]
        for s in np.setdiff1d(np.arange(self.B), ids):
            assert SR.same_bits(got_d[s], delta[s]) and SR.same_bits(got_e[s], ee[s]), (what, s)
        for f in ("yy", "yp", "yypredict", "yppredict", "ewt", "savres"):
            got = self.ctx.download(fid(f))
            assert np.array_equal(bits(got), bits(self.v[f])), (what, f)


class LinCase(Case):
    """band_problems.banded_linear on a host-callback band ctx"""
    pivoting = True

    def __init__(self, n, ml, mu, B=None, seed=None):
        import idahip
        B = BP.setup_batch(n) if B is None else B
        self.prob = BP.banded_linear(n, ml, mu, B)
        ctx = idahip.Ctx("host_callback", n, B, band=(ml, mu))
        ctx.set_tolerances(self.prob["rtol"], self.prob["atol"])
        ctx.set_host_band_problem(*BP.host_callbacks(self.prob))
        super().__init__(ctx, n, (ml, mu), B, 7 * n + 31 * ml + mu if seed is None else seed)

    def residual(self, s, yy, yp):
        return DQ.linear_res(self.prob["A"][s], self.prob["B"][s], self.prob["c"][s], yy, yp)

    def jac(self, s, cj):
        return BP.jacobian(self.prob, s, cj)

    def ensure_factored(self, ids):
        if any(int(s) not in self.fac for s in ids):
            idx = np.arange(self.B, dtype=np.int32)[::-1].copy()
            cjs, tn = self.cjs(idx.size), self.rng.uniform(0.0, 1.0, idx.size)
            rc, info = self.ctx.nls_sys_setup(tn, cjs, False, idx)
            self.expect_sys(idx, cjs, False)
            assert rc == 0
            self.check_factors(idx, cjs, info, "setup for the Newton body")


class HeatCase(Case):
    """the heat problem on a device band ctx of any width with ml, mu >= 1"""
    pivoting = False   # (whether rows are swapped depends on coef; asserted where a test relies on it)

    def __init__(self, n, ml, mu, B=4):
        import idahip
        from idahip import problems
        self.prob = problems.heat1d(n=n, batch=B)
        self.coef = self.prob["params"][:, 0]
        ctx = idahip.Ctx("heat1d", n, B, band=(ml, mu))
        ctx.set_tolerances(self.prob["rtol"], self.prob["atol"])
        ctx.set_problem_params(self.prob["params"])
        super().__init__(ctx, n, (ml, mu), B, 11 * n + 31 * ml + mu)

    def residual(self, s, yy, yp):
        return DQ.heat_res(float(self.coef[s]), yy, yp)

    def jac(self, s, cj):
        return DQ.analytic_jac("heat1d", {"coef": self.coef[s]}, cj, self.v["yy"][s])


@pytest.fixture(scope="module", params=BP.setup_cases(), ids=lambda c: "n%d-ml%d-mu%d" % c)
def lin(request):
    case = LinCase(*request.param)
    yield case
    case.close()


# ------------------------------------------------------------------------------------------------ (a) setups through band callbacks
def test_ctx_setups_through_band_callbacks(lin):
    """nls_sys then nls_lsetup, and nls_sys_setup, on permuted partial lists with a cj per list position; then the second list's
    setup on a fresh ctx: the same storage, fill rows included."""
    B, n = lin.B, lin.n
    first, second = lists_of(B)
    cj1, tn1 = lin.cjs(first.size), lin.rng.uniform(0.0, 1.0, first.size)
    ee0 = lin.v["ee"].copy()
    for reset in (False, True):
        lin.ctx.nls_sys(tn1, cj1, reset, first)
        lin.expect_sys(first, cj1, reset)
        lin.check_vectors(("nls_sys", reset))
        lin.check_others([], "nls_sys writes no factors")
    lin.set_ee(ee0)
    rc, info = lin.ctx.nls_lsetup(tn1, cj1, first)
    assert rc == 0
    lin.check_factors(first, cj1, info, "nls_lsetup")
    lin.check_vectors("nls_lsetup writes no vector")
    # the second list, other cj, over the first factors: its systems are factored anew, the others keep what they have
    cj2, tn2 = lin.cjs(second.size), lin.rng.uniform(0.0, 1.0, second.size)
    before = {f: lin.v[f].copy() for f in VEC}
    rc, info = lin.ctx.nls_sys_setup(tn2, cj2, False, second)
    assert rc == 0
    lin.expect_sys(second, cj2, False)
    lin.check_vectors("nls_sys_setup")
    lin.check_factors(second, cj2, info, "nls_sys_setup")
    if n <= 1100:
        fresh = LinCase(n, *lin.band, B=B)
        for f in VEC:
            fresh.ctx.upload(fid(f), before[f])
        rc, info = fresh.ctx.nls_sys_setup(tn2, cj2, False, second)
        assert rc == 0
        for s in second:
            ab, piv = fresh.storage(s)
            assert np.array_equal(bits(ab), bits(lin.raw[s][0])) and np.array_equal(piv, lin.raw[s][1]), s  # fill rows included
        fresh.close()


@pytest.mark.parametrize("n,ml,mu", [(17, 1, 1), (64, 2, 3), (64, 0, 2), (257, 7, 5)])
def test_a_zero_column_in_one_system(n, ml, mu):
    """System 2's Jacobian has an exactly zero column: its info is the oracle's 1-based column, the call returns 1, the other
    systems' factors are the oracle's."""
    case = LinCase(n, ml, mu, B=5)
    col = n // 2
    case.prob["A"][2, col, :] = 0.0   # (column-major: [s, j, :] is column j)
    case.prob["B"][2, col, :] = 0.0
    idx = np.array([3, 2, 0, 4], dtype=np.int32)
    cjs, tn = case.cjs(4), np.zeros(4)
    rc, info = case.ctx.nls_sys_setup(tn, cjs, True, idx)
    assert rc == 1
    case.expect_sys(idx, cjs, True)
    case.check_vectors("zero column")
    oinfo = case.check_factors(idx, cjs, info, "zero column")
    assert oinfo[1] == col + 1 and not oinfo[[0, 2, 3]].any()
    rc, info = case.ctx.nls_lsetup(tn[:1], cjs[:1], idx[1:2])  # the singular system alone
    assert rc == 1 and info[0] == oinfo[1]
    case.close()


# ------------------------------------------------------------------------------------------------ (c) idahip_newton_iter
def newton_inputs(case):
    B, n = case.B, case.n
    ids = np.array([s for s in range(B - 1, -1, -1) if s != 1], dtype=np.int32)
    ids[1:] = ids[:0:-1].copy()
    scale = np.array([2.0 / (1.0 + 1.3), 1.0, 2.0 / (1.0 + 0.7), 1.0, 0.25, 1.0, 1.75])
    return ids, scale


def test_newton_iter_on_a_band_ctx(lin):
    """delta = -delta, band getrs, *= scale, ee += delta, ||delta||: on the oracle's dense factors. Right-hand sides: random, and
    with the +0.0 / -0.0 runs of rhs_of."""
    B, n = lin.B, lin.n
    ids, scale = newton_inputs(lin)
    lin.ensure_factored(ids)
    scale = np.resize(scale, ids.size)
    assert (scale == 1.0).any() and (scale != 1.0).any()
    zeros, _ = rhs_of(lin.rng, B, n)
    for k, rhs in enumerate((zeros, lin.rng.standard_normal((B, n)) * 10.0 ** lin.rng.uniform(-3, 3, (B, n)))):
        ee = signed_zeros(lin.rng, lin.rng.standard_normal((B, n)))
        lin.newton(ids, rhs, ee, scale, ("newton_iter", k))
    lin.check_others([], "newton_iter writes no factors")


# ------------------------------------------------------------------------------------------------ (b) the heat band Jacobian kernel
@pytest.mark.parametrize("n,ml,mu", HEAT_WIDTHS, ids=lambda v: str(v))
def test_heat_band_jacobian_at_every_width(n, ml, mu):
    """stencil_band_jac_kernel<Heat1D> writes the whole ldab x n block of a listed system (three entries per column, +0.0 elsewhere, fill rows
    included) over whatever the last factorisation left there: three setups in a row with different cj, list lengths B, 3 and 1."""
    case = HeatCase(n, ml, mu, B=4)
    for k, (idx, how) in enumerate((([2, 0, 3, 1], "lsetup"), ([3, 0, 2], "sys_setup"), ([1], "lsetup"), ([0, 1, 3], "lsetup"))):
        idx = np.array(idx, dtype=np.int32)
        cjs = 10.0 ** case.rng.uniform(1.0, 5.0, idx.size)
        tn = case.rng.uniform(0.0, 1.0, idx.size)
        if how == "lsetup":
            rc, info = case.ctx.nls_lsetup(tn, cjs, idx)
        else:
            rc, info = case.ctx.nls_sys_setup(tn, cjs, False, idx)
            case.expect_sys(idx, cjs, False)
        assert rc == 0
        case.check_vectors((how, k))
        case.check_factors(idx, cjs, info, (how, k), want_info=np.zeros(idx.size, dtype=np.int32))
    if ml + mu > 2:  # the earlier factors had entries outside rows j - 1 .. j + 1 of a column, which the next Jacobian had to clear
        lu, piv = case.fac[0]
        ii, jj = np.indices((n, n)) if n <= 1100 else np.indices((64, 64))
        assert (piv != np.arange(n)).any() and np.any(lu[:ii.shape[0], :ii.shape[0]][np.abs(ii - jj) > 1])
    case.close()


# ------------------------------------------------------------------------------------------------ (d) idahip_newton_iter2
@pytest.mark.parametrize("ml,mu", [(1, 1), (2, 3), (16, 16)])
def test_newton_iter2_on_a_heat_band_ctx(ml, mu):
    """The first two Newton iterations with their convergence tests on the device. Systems that end at m = 0 are skipped by the
    second residual and the second pass (stencil_sys_kernel's and band_newton_iter_kernel's `skip`): their delta and ee stay."""
    n, B = 257, 16
    case = HeatCase(n, ml, mu, B=B)
    ids = np.arange(B, dtype=np.int32)[::-1].copy()
    cj = 10.0 ** case.rng.uniform(2.0, 4.0, B)
    tn = np.zeros(B)
    rc, info = case.ctx.nls_sys_setup(tn, cj, True, ids)
    assert rc == 0
    case.expect_sys(ids, cj, True)
    case.check_vectors("setup")
    case.check_factors(ids, cj, info, "setup")
    # scale < 1 leaves a part of the (linear) residual for the second iteration: rate = 1 - scale
    group = np.arange(B) % 4                       # by list position: 0 ends at m = 0, 1 at m = 1, 2 goes on, 3 diverges
    scale = np.where(group == 3, 0.05, 0.75)
    ewt, yyp, ypp = case.v["ewt"], case.v["yypredict"], case.v["yppredict"]
    r0 = case.v["delta"]
    d0, d1 = np.zeros(B), np.zeros(B)
    del1, ee1, del2, ee2 = (np.zeros((B, n)) for _ in range(4))
    for q, s in enumerate(ids):
        lu, piv = case.fac[int(s)]
        del1[s], ee1[s], d0[q] = SR.newton_iter(lu, piv, r0[s], np.zeros(n), ewt[s], scale[q])
        r1 = DQ.heat_res(float(case.coef[s]), yyp[s] + ee1[s], ypp[s] + cj[q] * ee1[s])
        del2[s], ee2[s], d1[q] = SR.newton_iter(lu, piv, r1, ee1[s], ewt[s], scale[q])
    toldel = np.zeros(B)
    ss = np.ones(B)
    eps = np.where(group == 0, np.inf, np.where(group == 1, 0.5 * d0, 0.0))
    toldel[group == 0] = np.where(np.arange((group == 0).sum()) % 2 == 0, 0.0, 1.0e5 * d0[group == 0])  # (both m = 0 tests)
    eps[(group == 0) & (toldel != 0.0)] = 0.0
    dn, conv = case.ctx.newton_iter2(scale, tn, cj, toldel, ss, eps, ids)
    got_d, got_e = case.ctx.download(fid("delta")), case.ctx.download(fid("ee"))
    want = np.array([SR.newton_ctest(d0[q], d1[q], toldel[q], ss[q], eps[q]) for q in range(B)])
    assert np.array_equal(want, np.array([1, 2, 0, 3])[group]), (want, d0, d1)   # the inputs do what they were chosen for
    assert np.array_equal(conv, want), (conv, want)
    for q, s in enumerate(ids):
        assert SR.same_bits(np.float64(dn[q, 0]), np.float64(d0[q])), (q, dn[q, 0], d0[q])
        if want[q] == 1:
            assert dn[q, 1] == 0.0 and np.array_equal(got_e[s], ee1[s]) and np.array_equal(got_d[s], del1[s]), q
            assert SR.same_bits(case.ctx.download(fid("savres"))[s], r0[s]), q   # no second residual either
        else:
            assert SR.same_bits(np.float64(dn[q, 1]), np.float64(d1[q])), (q, dn[q, 1], d1[q])
            assert np.array_equal(got_e[s], ee2[s]) and np.array_equal(got_d[s], del2[s]), q
    case.close()


# ------------------------------------------------------------------------------------------------ (e) launch widths
@pytest.mark.parametrize("spw", [1, 4, 64])
def test_launch_widths_give_the_same_results(spw, monkeypatch):
    """band_spw puts one system on a wavefront up to 1024 listed systems, so everything else in this file runs at width 1.
    IDAHIP_BAND_SPW (read at every call) packs 4 and 64 systems into a workgroup; 131 listed systems leave the last workgroup
    partial, and systems 131.. are not on the list."""
    monkeypatch.setenv("IDAHIP_BAND_SPW", str(spw))
    n, B, m = 17, 200, 131
    case = LinCase(n, 2, 3, B=B, seed=4242)
    idx = case.rng.permutation(m).astype(np.int32)
    cjs, tn = case.cjs(m), case.rng.uniform(0.0, 1.0, m)
    rc, info = case.ctx.nls_sys_setup(tn, cjs, False, idx)
    assert rc == 0
    case.expect_sys(idx, cjs, False)
    case.check_vectors("setup")
    case.check_factors(idx, cjs, info, "setup")          # (systems 131.. untouched: check_others)
    scale = np.where(np.arange(m) % 3 == 0, 1.0, 2.0 / (1.0 + case.rng.uniform(0.5, 1.5, m)))
    rhs, _ = rhs_of(case.rng, B, n)
    ee = signed_zeros(case.rng, case.rng.standard_normal((B, n)))
    case.newton(idx, rhs, ee, scale, "newton_iter")       # (systems 131.. untouched)
    case.check_others([], "newton_iter")
    case.close()


# ------------------------------------------------------------------------------------------------ (f) whole integrations, callbacks
@pytest.mark.parametrize("n,ml,mu", BP.INTEGRATIONS)
def test_banded_linear_integrations_through_band_callbacks(n, ml, mu):
    """The host stepper on a band ctx with changing cj, row swaps and fill, against the oracle's dense run of the same A, B, c."""
    import idahip
    from idahip import problems
    B = 3 if n > 1000 else 4
    q = BP.as_host_callback(BP.banded_linear(n, ml, mu, B))
    ctx = problems.make_ctx(q, band=True)
    assert ctx.band_query() == (ml, mu)
    ens = idahip.Ensemble(ctx, q["yy0"], q["yp0"])
    assert ens.device_controller_active() == 0
    ref = integrate_and_compare(ens, q, [float(t) for t in q["touts"]], np.arange(B))
    assert (ref["counters"]["nsetups"] >= 10).all(), ref["counters"]["nsetups"]  # re-factored with changing cj
    ens.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------ (g) heat on a wide band, both steppers
@pytest.mark.parametrize("n,ml,mu,B,device,period", [(257, 2, 3, 5, True, 0), (257, 2, 3, 5, False, 0), (1100, 3, 1, 4, True, 3),
                                                     (1100, 3, 1, 4, False, 0), (4096, 1, 2, 3, True, 0), (4096, 1, 2, 3, False, 0)])
def test_heat_on_a_wide_band_ctx_matches_the_dense_oracle(n, ml, mu, B, device, period):
    import idahip
    from idahip import problems
    p = problems.heat1d(n=n, batch=B)
    ctx = problems.make_ctx(p, band=(ml, mu))
    assert ctx.band_query() == (ml, mu) and ctx.ldab == 2 * ml + mu + 1
    if period:
        ctx.set_lu_period(period)
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    if not device:
        ens.set_device_controller(0)
    assert ens.device_controller_active() == (2 if device else 0)
    integrate_and_compare(ens, p, [float(t) for t in p["touts"][:5]], np.arange(B))
    ens.close()
    ctx.close()


def test_stream_state_wide_band_equals_dense():
    import idahip
    from idahip import problems
    n, B = 257, 6
    p = problems.heat1d(n=n, batch=B)
    touts = [float(t) for t in p["touts"][:3]]
    out = []
    for band in (False, (2, 3)):
        ctx = problems.make_ctx(p, band=band)
        ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
        assert ens.device_controller_active() == 2
        done = ens.stream(touts, 120)
        out.append((done, ens.yy(), ens.yp(), ens.counters(), ens.real("hused"), ens.real("tn"), ens.total_newton_iters()))
        ens.close()
        ctx.close()
    (d0, y0, yp0, c0, h0, t0, it0), (d1, y1, yp1, c1, h1, t1, it1) = out
    assert d0 == d1 and it0 == it1
    assert np.array_equal(y0, y1) and np.array_equal(yp0, yp1)  # by value
    assert np.array_equal(bits(h0), bits(h1)) and np.array_equal(bits(t0), bits(t1))
    for k in c0:
        assert np.array_equal(c0[k], c1[k]), k
