"""idaens_calc_ic (C IDA's IDACalcIC) on the GPU against calcic_ref.py, on the inputs that test_calcic_ref.py
pins on the CPU: dense contexts bit for bit, band contexts by value; statuses and every counter identical. Then the hand-over to the
three steppers against the oracle, idaens_stream's restarts, the batching of the lock-step driver and the refusals."""
import numpy as np
import pytest

import calcic_cases as K
import calcic_ref as IC
import oracle_lib as O

pytestmark = pytest.mark.gpu
IC_COUNTERS = IC.COUNTERS
OTHER_COUNTERS = ("nst", "netf", "n_attempts", "nls_nconvfails", "nge", "nlufail", "nconv_jcur", "nfail_first", "nli", "ncfl")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def open_case(c, yy0=None, yp0=None):
    import idahip
    ctx = K.make_ctx(c)
    ens = idahip.Ensemble(ctx, c["yy0"] if yy0 is None else yy0, c["yp0"] if yp0 is None else yp0)
    return ctx, ens


def device_state(ctx, ens):
    import idahip
    return {"yy": ens.yy(), "yp": ens.yp(), "phi0": ctx.download(idahip.F_PHI0), "phi1": ctx.download(idahip.F_PHI0 + 1),
            "ewt": ctx.download(idahip.F_EWT), "c": ens.counters()}


def launches(ctx):
    return {k: v["launches"] for k, v in ctx.timing_get().items()}


def check_against_reference(name, exact):
    c, r = K.case(name), K.reference(name)
    ctx, ens = open_case(c)
    status = ens.calc_ic(c["icopt"], c["tout1"])
    d = device_state(ctx, ens)
    ens.close()
    ctx.close()
    same = (lambda a, b: np.array_equal(bits(a), bits(b))) if exact else np.array_equal
    print(name, "status", status.tolist(), {k: d["c"][k].tolist() for k in IC_COUNTERS})
    assert np.array_equal(status, r["status"]), (status, r["status"])
    for k in IC_COUNTERS:
        assert np.array_equal(d["c"][k], r["counters"][k]), (k, d["c"][k], r["counters"][k])
    for k in OTHER_COUNTERS:
        assert (d["c"][k] == 0).all(), k
    # corrected values where the reference succeeded, the created ones where it failed (the reference returns those)
    for f, ref in (("yy", r["yy"]), ("phi0", r["yy"]), ("yp", r["yp"]), ("phi1", r["yp"])):
        assert same(d[f], ref), f
    for b in np.flatnonzero(r["status"] == 0):
        assert same(d["ewt"][b], r["ewt"][b]), ("ewt", b)
    for b in np.flatnonzero(r["status"] != 0):
        assert np.array_equal(bits(d["yy"][b]), bits(c["yy0"][b])) and np.array_equal(bits(d["yp"][b]), bits(c["yp0"][b]))
    return status, d


@pytest.mark.parametrize("name", K.DENSE_DEVICE)
def test_dense_ctx_bit_identical_to_reference(name):
    status, _ = check_against_reference(name, exact=True)
    assert (status == 0).all()


@pytest.mark.parametrize("name", K.BAND)
def test_band_ctx_equal_by_value(name):
    status, _ = check_against_reference(name, exact=False)
    assert (status == 0).all()


@pytest.mark.parametrize("name", K.DQ)
def test_dq_ctx(name):
    status, d = check_against_reference(name, exact=K.case(name)["band"] is None)
    assert (status == 0).all() and (d["c"]["nre_dq"] > 0).all()


def test_line_search_and_failures_share_rounds():
    """The two-unknown host-callback DAE: one batch of five in which a plain convergence, a backtracking one, CONV_FAIL,
    LINESEARCH_FAIL and NO_RECOVERY run side by side; the failed systems keep the values they were created with."""
    status, d = check_against_reference("linesearch", exact=True)
    assert status.tolist() == [0, 0, IC.CONV_FAIL, IC.LINESEARCH_FAIL, IC.NO_RECOVERY]
    assert d["c"]["nbacktr"][1] > 0 and d["c"]["nni"][4] == 0


@pytest.mark.parametrize("name", sorted(K.MIXED))
def test_mixed_fates_on_device_kinds(name):
    """The batches of K.MIXED (test_calcic_ref.py pins what each shows on the reference): successes, backtracking, retries at a
    smaller step size, CONV_FAIL, LINESEARCH_FAIL, NO_RECOVERY and BAD_EWT side by side on kinds whose trial runs in the fused
    kernels, every system with its own hic; status, values, weights and every counter as calcic_ref, bit for bit."""
    status, d = check_against_reference(name, exact=True)
    assert status.tolist() == K.MIXED_STATUS[name]


# ------------------------------------------------------------------------------------------------ hand-over to the steppers
RUN_COUNTERS = ("nst", "nre", "nje", "nsetups", "nni", "netf", "ncfn", "n_attempts")


def hand_over(name, touts, device, expect_active):
    c = K.case(name)
    ctx, ens = open_case(c)
    if not device:
        ens.set_device_controller(0)
    status = ens.calc_ic(c["icopt"], c["tout1"])
    assert (status == 0).all(), status
    yy, yp, c0 = ens.yy(), ens.yp(), ens.counters()
    assert ens.device_controller_active() == expect_active
    d = c["data"]
    ref = O.run_ensemble(c["kind"], c["n"], yy, yp, c["rtol"], c["atol"], touts, params=d.get("params"), A=d.get("A"), B=d.get("B"),
                         c=d.get("c"), nthreads=4)
    assert (ref["status"] == 0).all(), ref["status"]
    for i, t in enumerate(touts):
        st, _ = ens.solve(float(t))
        assert (st == 0).all(), st
        assert np.array_equal(bits(ens.yy()), bits(ref["yy"][i])) and np.array_equal(bits(ens.yp()), bits(ref["yp"][i])), t
    c1 = ens.counters()
    for k in RUN_COUNTERS:  # the integration's own work: what the IC counted is taken off
        assert np.array_equal(c1[k] - c0[k], ref["counters"][k]), (k, c1[k] - c0[k], ref["counters"][k])
    assert np.array_equal(c1["kused"], ref["kused"]) and np.array_equal(bits(ens.real("hused")), bits(ref["hused"]))
    assert np.array_equal(c1["nbacktr"], c0["nbacktr"])
    ens.close()
    ctx.close()


def test_hand_over_roberts_one_thread_device_stepper():
    hand_over("roberts_satol", [0.4, 4.0], True, 1)


def test_hand_over_linear_device_lock_step_stepper():
    hand_over("linear40_mixed", [0.05, 0.1], True, 2)


def test_hand_over_linear_host_stepper():
    hand_over("linear40_mixed", [0.05, 0.1], False, 0)


def test_stream_restarts_from_the_corrected_values():
    """An ensemble that computed its initial conditions and one that was created with them stream alike: the restarts of the first
    begin from the renewed snapshot, not from the guesses it was created with."""
    c = K.case("roberts_satol")
    ctx, ens = open_case(c)
    assert (ens.calc_ic(c["icopt"], c["tout1"]) == 0).all()
    yy, yp = ens.yy(), ens.yp()
    ctx2, ens2 = open_case(c, yy, yp)
    out = []
    for e in (ens, ens2):
        passes = e.stream([0.4], 200)
        out.append((passes, e.yy(), e.yp(), e.real("tn"), e.real("hused"), e.counter("nst")))
    assert out[0][0] == out[1][0] and out[0][0] >= ctx.batch  # every system has started over at least once on average
    for a, b in zip(out[0][1:5], out[1][1:5]):
        assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(out[0][5], out[1][5])
    for e, x in ((ens, ctx), (ens2, ctx2)):
        e.close()
        x.close()


# ------------------------------------------------------------------------------------------------ batching
@pytest.mark.parametrize("name", ["linear40_mixed", "roberts_vatol", "heat16_band"])
def test_launch_count_does_not_depend_on_the_batch(name):
    c = K.case(name)
    counts = []
    for B in (1, 32):
        rep = dict(c, yy0=np.tile(c["yy0"][:1], (B, 1)), yp0=np.tile(c["yp0"][:1], (B, 1)),
                   data={k: (np.tile(v[:1], (B,) + (1,) * (v.ndim - 1)) if isinstance(v, np.ndarray) else v) for k, v in c["data"].items()})
        ctx, ens = open_case(rep)
        ctx.timing_reset()
        assert (ens.calc_ic(c["icopt"], c["tout1"]) == 0).all()
        counts.append(launches(ctx))
        ens.close()
        ctx.close()
    print(name, counts[0])
    assert counts[0] == counts[1]
    assert sum(counts[0].values()) > 0


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_and_change_nothing():
    import idahip
    c = K.case("linear9_one_alg")
    ctx, ens = open_case(c)
    before = device_state(ctx, ens)

    def untouched():
        assert all(v == 0 for v in launches(ctx).values()), launches(ctx)
        now = device_state(ctx, ens)
        for f in ("yy", "yp", "phi0", "phi1"):
            assert np.array_equal(bits(now[f]), bits(before[f])), f
        for k in idahip.COUNTERS:
            assert np.array_equal(now["c"][k], before["c"][k]), k

    # an id entry that is neither 0 nor 1: refused, the id that was set stays
    with pytest.raises(idahip.IdaHipError):
        ctx.set_id(np.where(np.arange(c["n"]) == 1, 0.5, 1.0))
    assert np.array_equal(ctx.id(), c["id"])
    # YA_YDP_INIT without an id
    ctx.set_id(None)
    assert ctx.id() is None
    ctx.timing_reset()
    with pytest.raises(idahip.IdaHipError):
        ens.calc_ic(idahip.YA_YDP_INIT, c["tout1"])
    untouched()
    ctx.set_id(c["id"])
    # an unknown icopt
    with pytest.raises(idahip.IdaHipError):
        ens.calc_ic(3, c["tout1"])
    untouched()
    # tout1 == t0: every system reports ILL_INPUT
    assert (ens.calc_ic(idahip.YA_YDP_INIT, 0.0) == IC.ILL_INPUT).all()
    untouched()
    # after a solve call
    assert (ens.calc_ic(idahip.YA_YDP_INIT, c["tout1"]) == 0).all()
    ens.solve(0.01)
    after = device_state(ctx, ens)
    ctx.timing_reset()
    with pytest.raises(idahip.IdaHipError):
        ens.calc_ic(idahip.YA_YDP_INIT, c["tout1"])
    assert all(v == 0 for v in launches(ctx).values())
    now = device_state(ctx, ens)
    for f in ("yy", "yp", "phi0", "phi1"):
        assert np.array_equal(bits(now[f]), bits(after[f])), f
    ens.close()
    ctx.close()
