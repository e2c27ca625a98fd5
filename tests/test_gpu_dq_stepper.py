"""Whole integrations with difference-quotient Jacobians (idahip_set_jacobian_dq): the steppers that run them agree bit for bit --
the device lock-step stepper, the host stepper and a Python residual on the host stepper for heat (dense and band ctx); the device
and host steppers for linear dense; the one-thread device stepper and the host stepper for Roberts and Lorenz63. Every DQ run stays
close to the oracle's analytic-Jacobian run, and a ctx switched on and off again is a fresh analytic ctx."""
import numpy as np
import pytest

import dq_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu
CNT = ("nst", "nre", "nre_dq", "nje", "nsetups", "nni", "netf", "ncfn", "n_attempts", "kused")


def run(p, touts, dq=True, device=True, band=None, host_res=False):
    import idahip
    from idahip import problems
    B, n = p["yy0"].shape
    if host_res:
        coef = p["params"][:, 0]
        ctx = idahip.Ctx("host_callback", n, B, band=band)
        ctx.set_tolerances(p["rtol"], p["atol"])
        ctx.set_host_residual(lambda s, t, y, yp: R.heat_res(float(coef[s]), y, yp))
    else:
        ctx = problems.make_ctx(p, band=band if band else False)
    if dq:
        ctx.set_jacobian_dq(True)
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    if not device:
        ens.set_device_controller(0)
    active = ens.device_controller_active()
    out = []
    for t in touts:
        st, _ = ens.solve(float(t))
        assert (st == 0).all(), st
        out.append((ens.yy(), ens.yp()))
    res = {"out": out, "c": ens.counters(), "hused": ens.real("hused"), "active": active}
    ens.close()
    ctx.close()
    return res


def bits_equal(a, b):
    for (y1, p1), (y2, p2) in zip(a["out"], b["out"]):
        assert np.array_equal(y1.view(np.uint64), y2.view(np.uint64)) and np.array_equal(p1.view(np.uint64), p2.view(np.uint64))
    assert np.array_equal(a["hused"].view(np.uint64), b["hused"].view(np.uint64))
    for k in CNT:
        assert np.array_equal(a["c"][k], b["c"][k]), k


def close_to_oracle(r, p, touts, rel=1e-3):
    ref = O.run_ensemble(p["kind"], p["n"], p["yy0"], p["yp0"], p["rtol"], p["atol"], touts, params=p.get("params"), A=p.get("A"),
                         B=p.get("B"), c=p.get("c"), nthreads=4)
    assert (ref["status"] == 0).all()
    for i, (y, _) in enumerate(r["out"]):
        scale = np.maximum(np.abs(ref["yy"][i]).max(axis=1, keepdims=True), 1e-12)
        assert (np.abs(y - ref["yy"][i]) / scale).max() < rel, i
    assert (r["c"]["nre_dq"] > 0).all()


@pytest.mark.parametrize("band,n", [(None, 257), ((1, 1), 257), ((2, 3), 257), (None, 2048)])
def test_heat_three_paths_agree(band, n):
    from idahip import problems
    p = problems.heat1d(n=n, batch=4 if n < 1024 else 2)
    touts = [0.01, 0.03]
    dev = run(p, touts, device=True, band=band)
    assert dev["active"] == 2
    host = run(p, touts, device=False, band=band)
    assert host["active"] == 0
    cb = run(p, touts, device=False, band=band, host_res=True)
    bits_equal(dev, host)
    bits_equal(host, cb)
    w = R.dq_evals(n, band)
    assert np.array_equal(dev["c"]["nre_dq"], dev["c"]["nje"] * w)
    close_to_oracle(host, p, touts)


@pytest.mark.parametrize("n", [24, 257, 1100])
def test_linear_dense_device_and_host_agree(n):
    from idahip import problems
    p = problems.linear_dense(n=n, batch=3 if n < 1000 else 2)
    touts = [0.1, 0.2]
    dev = run(p, touts, device=True)
    assert dev["active"] == 2
    host = run(p, touts, device=False)
    bits_equal(dev, host)
    assert np.array_equal(dev["c"]["nre_dq"], dev["c"]["nje"] * n)
    close_to_oracle(host, p, touts)


@pytest.mark.parametrize("kind", ["roberts", "lorenz63"])
def test_tiny_device_and_host_agree(kind):
    from idahip import problems
    if kind == "roberts":
        p = problems.roberts()
        p = dict(p, yy0=np.tile(p["yy0"], (8, 1)), yp0=np.tile(p["yp0"], (8, 1)))
        # 0.4 .. 4e4: with the example's tolerances the DQ run stops short of 4e10 (DESIGN.md section 4e,
        # test_gpu_dq_jacobian.py::test_roberts_dq_column_error_at_late_times)
        touts = [float(t) for t in p["touts"][:6]]
    else:
        p = problems.lorenz63(batch=64)
        touts = [0.1, 0.5]
    dev = run(p, touts, device=True)
    assert dev["active"] == 1
    host = run(p, touts, device=False)
    bits_equal(dev, host)
    assert np.array_equal(dev["c"]["nre_dq"], dev["c"]["nje"] * 3)
    close_to_oracle(host, p, touts, rel=1e-3)


def test_switched_on_and_off_is_a_fresh_analytic_ctx():
    import idahip
    from idahip import problems
    p = problems.heat1d(n=257, batch=3)
    fresh = run(p, [0.02], dq=False)
    ctx = problems.make_ctx(p)
    ctx.set_jacobian_dq(True)
    ctx.set_jacobian_dq(False)
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    ens.solve(0.02)
    again = {"out": [(ens.yy(), ens.yp())], "c": ens.counters(), "hused": ens.real("hused")}
    bits_equal(fresh, again)
    assert (again["c"]["nre_dq"] == 0).all()
    ens.close()
    ctx.close()
