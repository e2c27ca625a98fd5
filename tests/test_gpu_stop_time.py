"""Stop times (idaens_set_stop_time, C IDA's IDASetStopTime) on the device against the oracle's own stop tests, switched on through
tests/tstop_oracle.py:
  * the cases of tests/tstop_cases.py -- per-system stop times by b % 7 (none, inside the first call, tiny, equal to the first tout,
    between later touts, far beyond, behind t0) on Roberts with its two roots (B = 70), linear dense n = 12 and n = 300, heat n = 20 on
    a dense and on a band ctx -- on the host stepper and on the device stepper each problem has: after every call status, tret, yy, yp,
    tn, hh, hused, kused, nst, nre, nni, netf, ncfn, nsetups and the stop time left, bit for bit (yy / yp by value on a band ctx);
  * stop times set between calls, at tn and just beyond it, in both tasks, on a host-callback problem (the ONE_STEP quirk Q15);
  * a masked case; a Krylov ctx with the band preconditioner, by property (the oracle's solver is direct);
  * in every case: no step beyond the stop time, tret == tstop exactly at a TSTOP return, NaN from get_stop_time after it;
  * the setter's refusals, idaens_stream's refusal, a schedule that ends at the TSTOP return."""
import numpy as np
import pytest

import stepper_ref as R
import tstop_cases as K
import tstop_oracle as T

pytestmark = pytest.mark.gpu

_REF = {}


def open_case(case, device_ctl, band=False, callbacks=None, krylov=None):
    import idahip
    from idahip import problems
    prob = case["prob"] if callbacks is None else dict(case["prob"], kind="host_callback", res=callbacks[0], jac=callbacks[1])
    ctx = problems.make_ctx(prob, band=band, krylov=krylov)
    if case.get("id") is not None:
        ctx.set_id(case["id"])
        ctx.set_suppress_alg(True)
    ens = idahip.Ensemble(ctx, prob["yy0"], prob["yp0"])
    ens.set_device_controller(device_ctl)
    if case["prob"]["kind"] == "roberts":
        ens.set_roots([0, 2], [1e-4, 0.01])  # the reference example's two functions: the oracle's Roberts has them built in
    return ctx, ens


def run_case(name, device_ctl, expect_active, band=False, callbacks=None):
    case = K.stop_case(name)
    ctx, ens = open_case(case, device_ctl, band=band, callbacks=callbacks)
    assert ens.device_controller_active() == expect_active
    d = K.ProductDriver(ens)
    ops = K.drive(case, d)
    key = (name, tuple((o[0], o[1] if o[0] != "stop" else None if o[1] is None else o[1].tobytes()) + tuple(map(str, o[2:])) for o in ops))
    if key not in _REF:  # the same ops on the harness, once for the steppers that made the same calls
        _REF[key] = T.run_ops(case["prob"], ops, **case["how"])[0]
    K.compare(d.rec, _REF[key], by_value=band, what="%s ctl=%d band=%s" % (name, device_ctl, band))
    assert any((r["status"] == T.TSTOP_RETURN).any() for r in d.rec)
    ens.close()
    ctx.close()
    return d.rec


@pytest.mark.parametrize("device_ctl", [0, 1])
@pytest.mark.parametrize("name", ["roberts", "linear12", "linear300", "heat20"])
def test_stop_times_by_residue_equal_the_oracle(name, device_ctl):
    active = 0 if not device_ctl else (1 if name == "roberts" else 2)
    rec = run_case(name, device_ctl, active)
    B = rec[0]["status"].size
    assert (rec[0]["status"][np.arange(B) % 7 == 2] == T.TSTOP_RETURN).all()  # the tiny stop time: reached in the first call


@pytest.mark.parametrize("device_ctl", [0, 1])
def test_stop_times_on_a_band_ctx(device_ctl):
    run_case("heat20", device_ctl, 2 if device_ctl else 0, band=True)


def test_stop_times_with_the_masked_norms():
    run_case("linear12_masked", 1, 2)
    run_case("linear12_masked", 0, 0)


def test_stop_times_between_calls_in_both_tasks_on_a_host_callback_problem():
    """tests/tstop_cases.py's "entry" script: a stop time just beyond tn (clipped at the entry of the call), at tn itself (TSTOP with
    no step), in IDA_NORMAL and in IDA_ONE_STEP, where the return consumes the stop time (quirk Q15)."""
    case = K.stop_case("entry")
    p = case["prob"]
    n, A, B, c = p["n"], p["A"], p["B"], p["c"]

    def res(sys, t, yy, yp):
        ra, rb = np.zeros(n), np.zeros(n)
        for j in range(n):  # two chains over ascending j, product then sum (the oracle's LinearDense::res)
            ra = ra + A[sys, j] * yp[j]
            rb = rb + B[sys, j] * yy[j]
        return (ra + rb) - c[sys]

    def jac(sys, t, cj, yy, yp, r):
        return (B[sys] + cj * A[sys]).T

    run_case("entry", 0, 0, callbacks=(res, jac))
    run_case("entry", 0, 0)  # and on the device kind, host stepper (ONE_STEP is the host stepper's)


def test_krylov_ctx_with_the_band_preconditioner_stops_at_tstop():
    """The oracle's solver is direct, so by property: TSTOP with tret == tstop exactly, no step beyond it, then on to tout."""
    case = K.stop_case("heat20")
    ctx, ens = open_case(case, 1, krylov=0)
    ctx.set_krylov_band_prec(1, 1)
    assert ens.device_controller_active() == 0
    t1 = case["touts"][0]
    ts = np.array([0.25 * t1, np.nan, 0.5 * t1])
    ens.set_stop_time(ts)
    ens.trace_system(0)
    st, tret = ens.solve(t1)
    assert st.tolist() == [T.TSTOP_RETURN, T.SUCCESS, T.TSTOP_RETURN], st
    assert tret[0] == ts[0] and tret[2] == ts[2] and tret[1] == t1
    tr = ens.trace()
    assert len(tr) > 0 and (tr[:, 0] <= ts[0]).all()
    assert (ens.real("tn")[[0, 2]] <= ts[[0, 2]]).all()
    assert np.isnan(ens.stop_time()).all()
    st, tret = ens.solve(t1)
    assert (st == T.SUCCESS).all() and (tret == t1).all()
    assert (ens.counter("npe") > 0).all()
    ens.close()
    ctx.close()


def test_no_traced_step_lies_beyond_the_stop_time():
    """The per-step trace of the host stepper (system 1 of linear12: stop time 0.25 of the first tout)."""
    case = K.stop_case("linear12")
    ctx, ens = open_case(case, 0)
    t1 = case["touts"][0]
    ens.set_stop_time(np.array([np.nan, 0.25 * t1, np.nan, np.nan, np.nan]))
    ens.trace_system(1)
    st, tret = ens.solve(t1)
    assert st[1] == T.TSTOP_RETURN and tret[1] == 0.25 * t1
    tr = ens.trace()
    assert len(tr) > 1 and (tr[:, 0] <= 0.25 * t1).all() and abs(tr[-1, 0] - 0.25 * t1) <= 100 * T.EPS * (abs(tr[-1, 0]) + abs(tr[-1, 1]))
    ens.close()
    ctx.close()


def test_refusals_and_the_schedule():
    import idahip
    case = K.stop_case("linear12")
    t1 = case["touts"][0]
    for device_ctl in (0, 1):
        ctx, ens = open_case(case, device_ctl)
        B = ctx.batch
        assert np.isnan(ens.stop_time()).all()
        for bad in (np.inf, -np.inf, np.array([1.0, 2.0])):
            with pytest.raises(idahip.IdaHipError):
                ens.set_stop_time(bad)
        assert np.isnan(ens.stop_time()).all()
        ens.set_stop_time(5.0)
        assert (ens.stop_time() == 5.0).all()
        with pytest.raises(idahip.IdaHipError, match="stop time"):  # a restarted system is Ida::new, which has none
            ens.stream(case["touts"], 4)
        assert (ens.counter("nst") == 0).all()
        ens.set_stop_time(None)
        assert np.isnan(ens.stop_time()).all()
        # inside a round-limited call
        st, _ = ens.solve(t1, max_rounds=3)
        assert (st == 99).all()
        with pytest.raises(idahip.IdaHipError, match="UNFINISHED"):
            ens.set_stop_time(1.0)
        st, _ = ens.solve(t1)
        assert (st == 0).all()
        # behind the current t of a system that has stepped: C IDA's check in IDASetStopTime; nothing changes
        ens.set_stop_time(np.array([np.nan, 7.0, np.nan, np.nan, np.nan]))
        with pytest.raises(idahip.IdaHipError, match="system 2"):
            ens.set_stop_time(np.array([9.0, 9.0, 0.5 * t1, 0.5 * t1, 9.0]))
        assert R.same_bits(ens.stop_time(), np.array([np.nan, 7.0, np.nan, np.nan, np.nan]))
        # a schedule ends at the TSTOP return exactly as at a root return
        ts = np.full(B, np.nan)
        ts[1] = 2.5 * t1
        ens.set_stop_time(ts)
        touts = [2 * t1, 3 * t1, 4 * t1]
        st, tret, reached = ens.solve_schedule(touts)
        assert st.tolist() == [0, T.TSTOP_RETURN, 0, 0, 0] and reached.tolist() == [3, 1, 3, 3, 3]
        assert tret[1] == 2.5 * t1 and (np.delete(tret, 1) == 4 * t1).all()
        assert np.isnan(ens.stop_time()).all()
        ens.close()
        ctx.close()
