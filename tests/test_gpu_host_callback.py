"""IDAHIP_HOST_CALLBACK above n = 8: the heat and linear dense problems written as numpy callbacks, in the operation order of
oracle/problems.hpp, must give the built-in device kinds' bits on the same data -- states, hused, kused and every counter
at each output of a whole integration, and the NLProblem entry points (nls_sys, nls_lsetup, nls_sys_setup) one by one.
The built-in kinds are pinned on the oracle elsewhere (test_gpu_ensemble.py, test_gpu_fullsize.py), so this reaches the
callback route's own parts: the packing of y / y' / residual, the work matrix jw, the chunked Jacobian upload (<= 64 MB per
chunk, callback_jac), the large-n LU pipelines, and at n >= 2048 the dirty / zero-block maps and jwzero."""
import numpy as np
import pytest

import stepper_ref as R

pytestmark = pytest.mark.gpu


def linear_problem(n, batch):
    from idahip import problems
    p = problems.linear_dense(n=n, batch=batch)
    A, B, c = p["A"], p["B"], p["c"]   # column-major per system: A[s, j] is column j

    def res(sys, t, yy, yp):
        ra, rb = np.zeros(n), np.zeros(n)
        for j in range(n):            # two chains over ascending j, product then sum (problems.hpp LinearDense::res)
            ra = ra + A[sys, j] * yp[j]
            rb = rb + B[sys, j] * yy[j]
        return (ra + rb) - c[sys]

    def jac(sys, t, cj, yy, yp, r):
        return (B[sys] + cj * A[sys]).T   # J = B + cj A, logical (row, column)

    return p, res, jac


def heat_problem(n, batch, touts):
    from idahip import problems
    p = problems.heat1d(n=n, batch=batch)
    p["touts"] = np.asarray(touts)
    coef = p["params"][:, 0]

    def res(sys, t, y, yp):
        f = np.empty(n)
        f[0] = y[0]
        f[1:-1] = yp[1:-1] - coef[sys] * ((y[:-2] - 2.0 * y[1:-1]) + y[2:])   # problems.hpp Heat1D::res
        f[-1] = y[-1]
        return f

    def jac(sys, t, cj, y, yp, r):
        J = np.zeros((n, n))
        J[0, 0] = 1.0
        i = np.arange(1, n - 1)
        J[i, i - 1] = -coef[sys]
        J[i, i] = cj + 2.0 * coef[sys]
        J[i, i + 1] = -coef[sys]
        J[n - 1, n - 1] = 1.0
        return J

    return p, res, jac


def callback_twin(p, res, jac):
    from idahip import problems
    q = dict(p, kind="host_callback", res=res, jac=jac)
    return problems.make_ctx(q)


def run_both(p, res, jac, superpanel=None):
    import idahip
    from idahip import problems
    ctx_b, ctx_c = problems.make_ctx(p), callback_twin(p, res, jac)
    if superpanel is not None:
        ctx_b.set_lu_superpanel(superpanel)
        ctx_c.set_lu_superpanel(superpanel)
    eb, ec = idahip.Ensemble(ctx_b, p["yy0"], p["yp0"]), idahip.Ensemble(ctx_c, p["yy0"], p["yp0"])
    eb.set_device_controller(0)   # the host stepper on both sides
    eb.set_fused_newton(0)        # (newton_iter2 needs a device residual: the callback route never fuses)
    ec.set_fused_newton(0)
    for t in p["touts"]:
        sb, _ = eb.solve(float(t))
        sc, _ = ec.solve(float(t))
        assert np.array_equal(sb, sc) and (sb >= 0).all(), (t, sb, sc)
        assert np.array_equal(ec.yy().view(np.uint64), eb.yy().view(np.uint64)), t
        assert np.array_equal(ec.yp().view(np.uint64), eb.yp().view(np.uint64)), t
        assert np.array_equal(ec.real("hused").view(np.uint64), eb.real("hused").view(np.uint64)), t
        cb, cc = eb.counters(), ec.counters()
        for k in cb:
            assert np.array_equal(cb[k], cc[k]), (t, k, cb[k], cc[k])
    assert (eb.counter("nst") > 0).all() and (eb.counter("nsetups") > 0).all()
    eb.close()
    ec.close()
    ctx_b.close()
    ctx_c.close()


@pytest.mark.parametrize("n", [24, 257])
def test_linear_dense_through_callbacks_matches_the_device_kind(n):
    p, res, jac = linear_problem(n, 3)
    p["touts"] = np.array([0.05, 0.1])
    run_both(p, res, jac)


@pytest.mark.parametrize("n", [24, 257])
def test_heat_through_callbacks_matches_the_device_kind(n):
    p, res, jac = heat_problem(n, 3, [0.002, 0.005])
    run_both(p, res, jac)


def test_jacobians_in_two_64mb_chunks():
    """n = 1100, batch 8: a Jacobian is 9.7 MB, so a setup of all eight systems goes up in two chunks with a synchronisation
    between them (callback_jac)."""
    p, res, jac = linear_problem(1100, 8)
    assert 8 * 1100 * 1100 * 8 > 64 << 20
    p["touts"] = np.array([0.02])
    run_both(p, res, jac)


@pytest.mark.parametrize("superpanel", [0, 1])
def test_heat_beyond_2048_rows_on_both_lu_pipelines(superpanel):
    """n = 2050 (a partial last 64 x 64 block): with set_lu_superpanel(1) the factorisation clears jw behind itself (jwzero)
    and the next callback writes its matrix into what that left."""
    p, res, jac = heat_problem(2050, 2, [0.0005, 0.001])
    run_both(p, res, jac, superpanel)


@pytest.mark.parametrize("n,superpanel", [(24, None), (257, None), (2050, 0), (2050, 1)])
def test_nls_entry_points_on_a_subset_match_the_device_kind(n, superpanel):
    """nls_sys (reset_ee 0 and 1), nls_lsetup and nls_sys_setup on an unordered subset: delta, savres, yy, yp, ee, and the
    factors and pivots of download_lu, bit for bit against the built-in kind; systems off the list unchanged on both sides."""
    import idahip
    from idahip import problems
    B = 3
    if n < 2048:
        p, res, jac = linear_problem(n, B)
    else:
        p, res, jac = heat_problem(n, B, [0.001])
    ctx_b, ctx_c = problems.make_ctx(p), callback_twin(p, res, jac)
    if superpanel is not None:
        ctx_b.set_lu_superpanel(superpanel)
        ctx_c.set_lu_superpanel(superpanel)
    rng = np.random.default_rng(n)
    fields = {idahip.F_YYPREDICT: p["yy0"] + 1e-3 * rng.standard_normal((B, n)), idahip.F_YPPREDICT: p["yp0"],
              idahip.F_EE: 1e-4 * rng.standard_normal((B, n)), idahip.F_EWT: np.ones((B, n)),
              idahip.F_YY: p["yy0"], idahip.F_YP: p["yp0"], idahip.F_DELTA: np.zeros((B, n)), idahip.F_SAVRES: np.zeros((B, n))}
    for ctx in (ctx_b, ctx_c):
        for f, v in fields.items():
            ctx.upload(f, v)
    ids = np.array([2, 0], dtype=np.int32)
    tn, cj = np.array([0.01, 0.02]), np.array([150.0, 2.5e3])

    def same(what):
        for f in (idahip.F_DELTA, idahip.F_SAVRES, idahip.F_YY, idahip.F_YP, idahip.F_EE):
            a, b = ctx_b.download(f), ctx_c.download(f)
            assert R.same_bits(b, a), (what, f)
            assert R.same_bits(a[1], fields[f][1]), (what, f)   # system 1 is never listed

    for reset in (0, 1):
        ctx_b.nls_sys(tn, cj, reset, ids)
        ctx_c.nls_sys(tn, cj, reset, ids)
        same(("sys", reset))
    for step in ("lsetup", "sys_setup0", "sys_setup1"):
        if step == "lsetup":
            rb, ib = ctx_b.nls_lsetup(tn, cj, ids)
            rc, ic = ctx_c.nls_lsetup(tn, cj, ids)
        else:
            reset = step.endswith("1")
            rb, ib = ctx_b.nls_sys_setup(tn, cj * 1.5, reset, ids)
            rc, ic = ctx_c.nls_sys_setup(tn, cj * 1.5, reset, ids)
        assert rb == rc == 0 and np.array_equal(ib, ic)
        same(step)
        for s in ids:
            lb, pb = ctx_b.download_lu(int(s))
            lc, pc = ctx_c.download_lu(int(s))
            assert np.array_equal(pb, pc) and R.same_bits(lc, lb), (step, s)
    ctx_b.close()
    ctx_c.close()
