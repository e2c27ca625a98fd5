"""Whole integrations on a band ctx (idahip_create_band) against the oracle's dense run of the same problem: steps, orders, step
sizes and counters bit-identical, y and y' equal by value at every output (band_kernels.hpp's contract), on the device lock-step
stepper and on the host stepper; the heat problem through band host callbacks; and a batch no dense ctx can hold."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
CNT = ("nst", "nre", "nje", "nsetups", "nni", "netf", "ncfn", "n_attempts")


def sample(p, ids):
    B = p["yy0"].shape[0]
    return {k: (v[ids] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B else v) for k, v in p.items()}


def integrate_and_compare(ens, p, touts, ids):
    """ens integrates every system of p; the systems `ids` are checked against the oracle at every output. A host-callback problem
    names the oracle's problem in p["oracle_kind"] (heat1d when absent). Returns the oracle's run."""
    q = sample(p, ids)
    kind = q["kind"] if q["kind"] != "host_callback" else q.get("oracle_kind", "heat1d")
    ref = O.run_ensemble(kind, q["n"], q["yy0"], q["yp0"], q["rtol"], q["atol"], touts, params=q.get("params"), A=q.get("A"), B=q.get("B"),
                         c=q.get("c"), nthreads=min(len(ids), 16))
    assert (ref["status"] == 0).all()
    for i, t in enumerate(touts):
        status, tret = ens.solve(float(t))
        assert (status == 0).all() and (tret == t).all()
        assert np.array_equal(ens.yy()[ids], ref["yy"][i]) and np.array_equal(ens.yp()[ids], ref["yp"][i]), i  # by value
    c = ens.counters()
    for k in CNT:
        assert np.array_equal(c[k][ids], ref["counters"][k]), k
    assert np.array_equal(c["kused"][ids], ref["kused"]) and np.array_equal(ens.real("hused")[ids], ref["hused"])
    return ref


def spread(B, k=8):
    return np.unique(np.r_[0, B - 1, np.linspace(0, B - 1, k).astype(int)])


@pytest.mark.parametrize("n,B,device", [(1024, 4, True), (4096, 256, True), (4096, 256, False)])
def test_heat_on_a_band_ctx_matches_the_dense_oracle(n, B, device):
    import idahip
    from idahip import problems
    p = problems.heat1d(n=n, batch=B)
    ctx = problems.make_ctx(p, band=True)
    assert ctx.band_query() == (1, 1) and ctx.ldab == 4
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    if not device:
        ens.set_device_controller(0)
    assert ens.device_controller_active() == (2 if device else 0)
    integrate_and_compare(ens, p, [float(t) for t in p["touts"]], np.arange(B) if B <= 8 else spread(B))
    ens.close()
    ctx.close()


def test_lu_period_on_a_band_ctx():
    import idahip
    from idahip import problems
    p = problems.heat1d(n=2048, batch=24)
    ctx = problems.make_ctx(p, band=True)
    ctx.set_lu_period(5)
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    assert ens.device_controller_active() == 2
    integrate_and_compare(ens, p, [float(t) for t in p["touts"][:4]], spread(24, 6))
    ens.close()
    ctx.close()


@pytest.mark.parametrize("n", [64, 256])
def test_heat_through_band_host_callbacks(n):
    import idahip
    from idahip import problems
    B = 3
    p = problems.heat1d(n=n, batch=B)
    coef = p["params"][:, 0]

    def res(sys, t, y, yp):  # Heat1D::row's operation order (stencil_sys_kernel)
        f = np.empty(n)
        f[0] = y[0]
        f[1:-1] = yp[1:-1] - coef[sys] * ((y[:-2] - 2.0 * y[1:-1]) + y[2:])
        f[-1] = y[-1]
        return f

    def bjac(sys, t, cj, y, yp, r, ab):  # ab[j, ml + mu + i - j] = J(i, j), ml = mu = 1
        ab[0, 2] = 1.0
        ab[n - 1, 2] = 1.0
        i = np.arange(1, n - 1)
        ab[i, 2] = cj + 2.0 * coef[sys]
        ab[i - 1, 3] = -coef[sys]  # J(i, i - 1)
        ab[i + 1, 1] = -coef[sys]  # J(i, i + 1)

    q = dict(p, kind="host_callback", res=res, bjac=bjac, band=(1, 1))
    ctx = problems.make_ctx(q, band=True)
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    assert ens.device_controller_active() == 0
    integrate_and_compare(ens, q, [0.002, 0.005, 0.01], np.arange(B))
    ens.close()
    ctx.close()


def test_stream_state_band_equals_dense():
    import idahip
    from idahip import problems
    n, B = 1100, 6
    p = problems.heat1d(n=n, batch=B)
    touts = [float(t) for t in p["touts"][:3]]
    out = []
    for band in (False, True):
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
    assert np.array_equal(h0, h1) and np.array_equal(t0, t1)
    for k in c0:
        assert np.array_equal(c0[k], c1[k]), k


def test_a_batch_no_dense_ctx_can_hold():
    """N = 4096, B = 4096: the dense ctx would need 2 x 4096 x 128 MiB of factors and work matrices; the band ctx holds 512 MiB."""
    import idahip
    from idahip import problems
    n, B = 4096, 4096
    p = problems.heat1d(n=n, batch=B)
    ctx = problems.make_ctx(p, band=True)
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    assert ens.device_controller_active() == 2
    integrate_and_compare(ens, p, [float(t) for t in p["touts"]], spread(B, 10))
    ens.close()
    ctx.close()


def test_dense_only_calls_on_a_band_ctx_are_refused():
    import idahip
    H, _ = idahip.load()
    for kind in ("heat1d", "host_callback"):
        ctx = idahip.Ctx(kind, 64, 2, band=(1, 1))
        lu, piv = np.zeros(64 * 64), np.zeros(64, dtype=np.int64)
        assert H.idahip_download_lu(ctx.h, 0, idahip._p(lu), idahip._p(piv, idahip.i64p)) == -2
        a = np.zeros(64 * 64 * 2)
        assert H.idahip_set_linear_dense(ctx.h, 0, 1, idahip._p(a), idahip._p(a), idahip._p(a)) == -2
        res_cb = idahip.RES_FN(lambda *a: 0)
        jac_cb = idahip.JAC_FN(lambda *a: 0)
        assert H.idahip_set_host_problem(ctx.h, res_cb, jac_cb, None) == -2
        info = np.zeros(1, dtype=np.int32)
        idx = np.zeros(1, dtype=np.int32)
        d = ctx.dev_empty(8 * 64 * 64)
        assert H.idahip_ls_setup(ctx.h, d, d, idahip._p(info, idahip.i32p), idahip._p(idx, idahip.i32p), 1) == -2
        ctx.dev_free(d)
        ab, pv = ctx.download_lu_band(1)
        assert ab.shape == (64, 4) and pv.shape == (64,)
        ctx.close()
    dense = idahip.Ctx("heat1d", 64, 1)
    assert dense.band_query() is None
    bj = idahip.BAND_JAC_FN(lambda *a: 0)
    assert H.idahip_set_host_band_problem(dense.h, idahip.RES_FN(lambda *a: 0), bj, None) == -2
    assert H.idahip_download_lu_band(dense.h, 0, None, None) == -2
    dense.close()
    for kind, n, band in (("linear_dense", 64, (1, 1)), ("lorenz63", 3, (1, 1)), ("heat1d", 8, (1, 1)), ("heat1d", 4097, (1, 1)),
                          ("heat1d", 64, (0, 1)), ("host_callback", 64, (64, 0))):
        with pytest.raises(idahip.IdaHipError):
            idahip.Ctx(kind, n, 1, band=band)
