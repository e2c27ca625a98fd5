"""The steppers' failure and recovery paths against the oracle: the restore kernel after a failed error test, the three branches of
handle_n_flag (first failure: pow-based rr; second: rr = 0.25; third and later: order 1), the ERR_FAIL exit, failures before the first
step (quirk Q5: reset() rescales phi[1], idahip_scale_phi1), a linear setup that fails at every attempt, TOO_MUCH_ACC, and idaens_stream
with a system that recovers or dies -- on the host stepper, the device lock-step stepper and the one-thread-per-system stepper, at every
LU launch shape, on band and difference-quotient ctxs. The recipes are tests/failure_recipes.py's; tests/test_failure_recipes.py proves on
the oracle alone that each takes the path it is named for.

Bar: np.array_equal against the oracle on status, t_ret, y, y' at every tout, on every counter of CNT, on kused and hused; device
stepper == host stepper on state(); nfail_first == the oracle's failures at nst == 0; nlufail + nconv_jcur == ncfn. Every batch keeps
untouched systems next to the failing ones, and those equal a run without the failing ones."""
import numpy as np
import pytest

import failure_recipes as F
from test_gpu_device_controller import make, same, state
from test_gpu_ensemble import CNT, run_oracle

pytestmark = pytest.mark.gpu


def open_on(case, device_ctl, band=False, dq=False, period=0):
    """(ctx, ens) for the case's problem on the stepper asked for -- asserted, so that no comparison is host against host."""
    import idahip
    from idahip import problems
    prob = case["prob"]
    if not band and not dq and not period:
        ctx, ens = make(prob, device_ctl)
    else:
        ctx = problems.make_ctx(prob, band=band)
        if dq:
            ctx.set_jacobian_dq(True)
        if period:
            ctx.set_lu_period(period)
        ens = idahip.Ensemble(ctx, prob["yy0"], prob["yp0"])
        ens.set_device_controller(device_ctl)
    want = 0 if (not device_ctl or prob["kind"] == "host_callback") else 1 if prob["kind"] == "lorenz63" else 2
    assert ens.device_controller_active() == want, (ens.device_controller_active(), want)
    if case["mxstep"]:
        ens.set_max_num_steps(case["mxstep"])
    return ctx, ens


def run_calls(case, ctx, ens):
    """Ida::solve(tout) for every tout, the edit between the touts before and after the jump -> [(status, tret, yy, yp)] per tout."""
    rec = []
    for i, t in enumerate(case["before"] + case["after"]):
        if i == len(case["before"]) and case["edit"] is not None:
            F.apply_to_ctx(ctx, case)
        st, tret = ens.solve(t)
        rec.append((st.copy(), tret.copy(), ens.yy(), ens.yp()))
    return rec


def run_schedule(case, ctx, ens, max_rounds):
    """The same through idaens_solve_schedule cut into slices of max_rounds rounds: the touts before the jump as one schedule, the
    edit, the touts after it as another -> (status, tret, yy [ntout][B][n], yp) with NaN rows where a tout was not reached."""
    B, n = case["prob"]["yy0"].shape
    T = len(case["before"]) + len(case["after"])
    Y, YP = np.full((T, B, n), np.nan), np.full((T, B, n), np.nan)
    off = 0
    for part, after in ((case["before"], False), (case["after"], True)):
        if after and case["edit"] is not None:
            F.apply_to_ctx(ctx, case)
        if not part:
            continue
        for _ in range(100000):
            s, t, r, yo, ypo = ens.solve_schedule(part, max_rounds=max_rounds, outputs=True)
            m = ~np.isnan(yo)
            Y[off:off + len(part)][m] = yo[m]
            YP[off:off + len(part)][m] = ypo[m]
            if (s != 99).all():
                break
        else:
            raise AssertionError("the schedule does not end")
        off += len(part)
    return s, t, Y, YP


def same_calls(a, b, ids=None):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        for u, v in zip(x, y):
            assert np.array_equal(u if ids is None else u[ids], v), i


def counters_equal_oracle(ens, ref):
    c = ens.counters()
    print("netf", c["netf"], "ncfn", c["ncfn"], "nfail_first", c["nfail_first"], "oracle:", ref["counters"]["netf"], ref["counters"]["ncfn"],
          ref["nfail_first"])
    for k in CNT:
        assert np.array_equal(c[k], ref["counters"][k]), (k, c[k], ref["counters"][k])
    assert np.array_equal(c["kused"], ref["kused"]) and np.array_equal(ens.real("hused"), ref["hused"])
    assert np.array_equal(c["nfail_first"], ref["nfail_first"]), (c["nfail_first"], ref["nfail_first"])
    assert np.array_equal(c["nlufail"] + c["nconv_jcur"], c["ncfn"])


def equals_oracle(rec, ens, ref):
    for i, (st, tret, yy, yp) in enumerate(rec):
        print("tout", i, "status", st, "oracle", ref["status"][i])
        assert np.array_equal(st, ref["status"][i]), (i, st, ref["status"][i])
        assert np.array_equal(tret, ref["tret"][i]), (i, tret, ref["tret"][i])
        assert np.array_equal(yy, ref["yy"][i]) and np.array_equal(yp, ref["yp"][i]), i
    counters_equal_oracle(ens, ref)


def untouched_equal_a_run_alone(case, rec, ens, **how):
    """The systems the recipe leaves alone, integrated as a batch of their own on the device stepper: same returns, same state."""
    B = case["prob"]["yy0"].shape[0]
    ids = np.array([s for s in range(B) if s not in case["edited"]])
    assert 0 < ids.size < B
    alone = dict(case, prob=F.sub_problem(case["prob"], ids), edited=[], edit=None)
    c2, e2 = open_on(alone, 1, **how)
    same_calls(rec, run_calls(alone, c2, e2), ids)
    a, b = state(ens), state(e2)
    for k in a:
        assert np.array_equal(a[k][ids], b[k]), k
    e2.close()
    c2.close()


def both_steppers_against_the_oracle(case, **how):
    ref = F.oracle_reference(case)
    cd, dev = open_on(case, 1, **how)
    ch, host = open_on(case, 0, **how)
    rd, rh = run_calls(case, cd, dev), run_calls(case, ch, host)
    same_calls(rd, rh)
    same(state(dev), state(host))
    equals_oracle(rd, dev, ref)
    untouched_equal_a_run_alone(case, rd, dev, **how)
    return ref, (cd, dev), (ch, host)


# ------------------------------------------------------------------------------------------------ jumps
@pytest.mark.parametrize("name,n", F.GPU_JUMPS)
def test_jump_recipes_on_both_lock_step_steppers(name, n):
    """linear_dense to t = 0.3, the recipe's edit for three (n = 1100: two) systems of the batch through idahip_set_linear_dense, then
    on: the next step fails its error test up to ten times (restore kernel, every branch of handle_n_flag; terminal and mixed recipes:
    the ERR_FAIL exit, sticky at the following tout). n = 24 / 200: vector kernels of one / several wavefronts; 704: workgroup-per-matrix
    LU panels; 1100: the large-n pipeline. Up to n = 200 also through idaens_solve_schedule cut into slices of seven rounds."""
    case = F.jump_case(name, n)
    ref, (cd, dev), (ch, host) = both_steppers_against_the_oracle(case)
    ed = case["edited"]
    assert (ref["counters"]["netf"][ed] >= 3).all()
    if case["expect"] in ("terminal", "mixed"):
        assert (ref["status"][-1][ed] == -3).any() and ((ref["status"][-1][ed] == -3) == (ref["counters"]["netf"][ed] == 10)).all()
    if case["expect"] == "deep":
        assert (ref["status"] == 0).all()
    if n <= 256:
        for device_ctl in (1, 0):
            cs, sl = open_on(case, device_ctl)
            s, t, Y, YP = run_schedule(case, cs, sl, 7)
            assert np.array_equal(s, ref["status"][-1]) and np.array_equal(t, ref["tret"][-1])
            ok = ref["status"] == 0
            assert np.array_equal(Y[ok], ref["yy"][ok]) and np.array_equal(YP[ok], ref["yp"][ok])
            assert np.isnan(Y[~ok]).all()
            counters_equal_oracle(sl, ref)
            same(state(sl), state(dev))


def test_a_long_recovery_with_a_hundred_failures():
    """A *= 0.01 at n = 24: about 1800 steps to t = 1 and 60 to 110 failed error tests per edited system, up to seven in one step."""
    name, n = F.LONG_JUMP
    case = F.jump_case(name, n, after=(0.4, 0.5, 1.0), mxstep=100000)
    ref, _, _ = both_steppers_against_the_oracle(case)
    assert (ref["status"] == 0).all() and (ref["counters"]["netf"][case["edited"]] >= 50).all()


@pytest.mark.parametrize("n", [24, 200])
def test_jump_inside_a_round_limited_schedule_with_the_steppers_alternating(n):
    """One schedule over all ten touts cut by max_rounds, the edit (c *= 1.01 for three systems) after thirty rounds -- every system
    has made thirty attempts then, on either stepper -- on the device stepper alone, on the host stepper alone, and with the stepper
    alternating per one-round call: a system is then handed over in the middle of a failing step (nef > 0, the restart the device
    stepper deferred to the next round is the host stepper's to serve, and the other way round)."""
    case = F.jump_case("c*1.01", n)
    p, ed = case["prob"], case["edited"]
    touts, R0 = p["touts"], 30
    B = p["yy0"].shape[0]

    def sliced(ens, ctx, rounds_of, stepper_of=None):
        Y = np.full((len(touts), B, n), np.nan)
        handed = 0
        for i in range(20000):
            if i == 1:
                F.apply_to_ctx(ctx, case)
            if stepper_of is not None:
                ens.set_device_controller(stepper_of(i))
                assert ens.device_controller_active() == (2 if stepper_of(i) else 0)
            before = ens.counter("netf").sum()
            s, t, r, yo, ypo = ens.solve_schedule(touts, max_rounds=rounds_of(i), outputs=True)
            if i >= 1 and ens.counter("netf").sum() > before and (s == 99).any():
                handed += 1  # a call ended right after a failed error test: the next call repeats that step
            m = ~np.isnan(yo)
            Y[m] = yo[m]
            if i == 0:
                assert (s == 99).all(), "thirty rounds do not finish the schedule"
            if (s != 99).all():
                return s, Y, handed
        raise AssertionError("the schedule does not end")

    cd, dev = open_on(case, 1)
    sd, Yd, _ = sliced(dev, cd, lambda i: R0 if i == 0 else 50)
    ch, host = open_on(case, 0)
    sh, Yh, _ = sliced(host, ch, lambda i: R0 if i == 0 else 50)
    cm, mix = open_on(case, 1)
    sm, Ym, handed = sliced(mix, cm, lambda i: R0 if i == 0 else 1, stepper_of=lambda i: 1 if i % 2 == 0 else 0)
    assert (sd == 0).all() and (sh == 0).all() and (sm == 0).all()
    netf = dev.counter("netf")
    print("netf", netf, "handed over", handed)
    assert (netf[ed] >= 3).all(), "the jump made no step fail three times: the path under test was not taken"
    assert np.array_equal(Yd, Yh) and np.array_equal(Yd, Ym) and not np.isnan(Yd).any()
    same(state(dev), state(host))
    same(state(dev), state(mix))
    assert handed >= 3, "no one-round call ended inside a failing step"
    # the oracle: thirty steps one by one (a round is one attempt of every system, and none fails before the jump), the edit, the touts
    ref = F.jump_after_attempts(case, touts, R0)
    assert np.array_equal(Yd, ref["yy"])
    c = dev.counters()
    for k in CNT:
        assert np.array_equal(c[k], ref["counters"][k]), (k, c[k], ref["counters"][k])
    assert np.array_equal(c["kused"], ref["kused"]) and np.array_equal(dev.real("hused"), ref["hused"])


def test_jump_with_factorisations_batched_over_rounds():
    """idahip_set_lu_period(3): a system whose repeated attempt asks for a setup may wait for it, its failure count kept. Same returns
    and state as with period 1 (and so the oracle's), only more rounds."""
    case = F.jump_case("c*1.01", 200)
    ref = F.oracle_reference(case)
    c1, plain = open_on(case, 1)
    c3, held = open_on(case, 1, period=3)
    assert c3.lu_period() == 3
    r1, r3 = run_calls(case, c1, plain), run_calls(case, c3, held)
    same_calls(r1, r3)
    same(state(plain), state(held))
    equals_oracle(r3, held, ref)
    assert held.total_rounds() >= plain.total_rounds() > 0
    assert (ref["counters"]["netf"][case["edited"]] >= 3).all()


# ------------------------------------------------------------------------------------------------ failures before the first step
@pytest.mark.parametrize("kind,n,tout,expect", F.GPU_FIRST_STEPS)
def test_failures_before_the_first_step_on_all_three_steppers(kind, n, tout, expect):
    """y'(0) = 0 for some systems of the batch and a first tout so far away that h0 = 0.001 tout fails five to ten times at nst == 0:
    every failure there rescales phi[1] (Q5; oracle and product follow C IDA). linear_dense and heat1d on the lock-step device stepper,
    lorenz63 (64 systems: several per wavefront) on the one-thread-per-system stepper, all on the host stepper. The terminal variants end
    with -3 at nst == 0; Lorenz meets Newton convergence failures with a current Jacobian on the way (nconv_jcur), and its untouched
    systems stop at the step limit (-1) long before t = 1e4."""
    case = F.first_step_case(kind, n, tout, later=(1.5 * tout,) if expect == "recover" else (), expect=expect)
    ref, (cd, dev), _ = both_steppers_against_the_oracle(case)
    ed = np.array(case["edited"])
    un = np.array([s for s in range(case["prob"]["yy0"].shape[0]) if s not in case["edited"]])
    assert (ref["nfail_first"][ed] > 0).all() and (ref["nfail_first"][un] == 0).all()
    if expect == "recover":
        assert (ref["status"] == 0).all() and (ref["counters"]["nst"] > 0).all()
    else:
        assert (ref["status"][0][ed] == -3).all() and (ref["counters"]["nst"][ed] == 0).all() and (ref["counters"]["netf"][ed] == 10).all()
        assert (ref["status"][0][un] != -3).all()
        if kind == "lorenz63":
            assert (dev.counter("nconv_jcur")[ed] > 0).all()


@pytest.mark.parametrize("n,band", F.BAND_FIRST_STEPS)
def test_failures_before_the_first_step_on_a_band_ctx(n, band):
    """The same through the band LU: hh shrinks between the attempts, every one sets up anew. By value against the oracle's dense run."""
    case = F.first_step_case("heat1d", n, 1.0, later=(1.5,))
    ref, _, _ = both_steppers_against_the_oracle(case, band=band)
    assert (ref["nfail_first"][case["edited"]] > 0).all() and (ref["status"] == 0).all()


@pytest.mark.parametrize("what,kind,n", [("first", k, n) for k, n in F.DQ_FIRST_STEPS] + [("jump", "linear_dense", 24)])
def test_failures_with_difference_quotient_Jacobians(what, kind, n):
    """idahip_set_jacobian_dq(1): the increments of a DQ Jacobian depend on hh, which every failed attempt cuts. The oracle has no DQ
    Jacobian; device stepper == host stepper on every return, on state() and on nre_dq, and the run takes the path (the product's own
    counters say so: that is a condition, the comparison is between the two steppers)."""
    case = F.first_step_case(kind, n, 1.0, later=(1.5,)) if what == "first" else F.jump_case("c*1.01", n)
    cd, dev = open_on(case, 1, dq=True)
    ch, host = open_on(case, 0, dq=True)
    rd, rh = run_calls(case, cd, dev), run_calls(case, ch, host)
    same_calls(rd, rh)
    same(state(dev), state(host))
    c, ed = dev.counters(), case["edited"]
    print("netf", c["netf"], "nfail_first", c["nfail_first"], "nre_dq", c["nre_dq"])
    assert np.array_equal(c["nre_dq"], host.counter("nre_dq")) and (c["nre_dq"] > 0).all()
    assert np.array_equal(c["nfail_first"], host.counter("nfail_first"))
    assert (rd[-1][0] == 0).all() and (c["netf"][ed] >= 3).all()
    if what == "first":
        assert (c["nfail_first"][ed] >= 3).all()
    untouched_equal_a_run_alone(case, rd, dev, dq=True)


# ------------------------------------------------------------------------------------------------ singular Jacobians
@pytest.mark.parametrize("n,when", [(n, w) for n in F.SINGULAR_SIZES for w in ("start", "mid")])
def test_singular_jacobian_at_every_lu_pipeline(n, when):
    """System 1 of the batch with an exactly zero column in A and in B, from the start or from t = 0.3 on: the factorisation reports a
    zero pivot at every attempt (Q2: recoverable, as in C IDA; the reference unwraps), ten times, then the step fails for good with the
    oracle's status (-4). n = 200, 704 and 1100: the three LU pipelines beyond the one the n = 12 test takes."""
    case = F.singular_case(n, when)
    ref, (cd, dev), _ = both_steppers_against_the_oracle(case)
    assert ref["status"][-1][1] == -4 and (np.delete(ref["status"][-1], 1) == 0).all()
    c = dev.counters()
    assert c["nlufail"][1] == 10 and c["ncfn"][1] == 10 and (np.delete(c["nlufail"], 1) == 0).all()


@pytest.mark.parametrize("when", ["start", "mid"])
def test_singular_jacobian_through_band_callbacks(when):
    """band_problems' banded linear DAE on a band ctx with host callbacks (the host stepper: callbacks have no device stepper), one
    system with a zero column: the band factorisation's zero pivot takes the same path. By value against the oracle's dense run."""
    n, ml, mu = F.SINGULAR_BAND
    ref = F.oracle_reference(F.singular_case(n, when, band=(ml, mu)))
    case = F.singular_case(n, when, band=(ml, mu))  # (the edit is made in place in a callback problem: a case of its own per run)
    ctx, ens = open_on(case, 0, band=True)
    assert ctx.band_query() == (ml, mu)
    rec = run_calls(case, ctx, ens)
    equals_oracle(rec, ens, ref)
    assert ref["status"][-1][1] == -4 and (np.delete(ref["status"][-1], 1) == 0).all() and ens.counter("nlufail")[1] == 10
    others = [0, 2, 3]
    alone = F.singular_case(n, when, band=(ml, mu), only=others)
    c2, e2 = open_on(alone, 0, band=True)
    same_calls(rec, run_calls(alone, c2, e2), others)


# ------------------------------------------------------------------------------------------------ TOO_MUCH_ACC
@pytest.mark.parametrize("kind", ["linear_dense", "lorenz63"])
def test_too_much_accuracy_is_refused_like_the_oracle_and_stays_refused(kind):
    """rtol = 1e-17, atol = 1e-20: the loop-top check before the first step returns TOO_MUCH_ACC (-2) with nst == 0, on all three
    steppers as in the oracle (status, t_ret and every counter: no step was attempted, so there is no solution to return and y is not
    compared); a negative status is sticky (include/ida_ensemble.h): a second call reports it again and changes nothing."""
    case = F.too_much_acc_case(kind)
    p = case["prob"]
    ref = run_oracle(p, touts=case["after"])
    assert (ref["status"] == -2).all() and (ref["counters"]["nst"] == 0).all()
    mine = F.oracle_reference(case)
    assert np.array_equal(mine["status"][0], ref["status"])
    for device_ctl in (1, 0):
        ctx, ens = open_on(case, device_ctl)
        rec = run_calls(case, ctx, ens)
        assert np.array_equal(rec[0][0], ref["status"]) and np.array_equal(rec[0][1], mine["tret"][0])
        counters_equal_oracle(ens, mine)
        for k in CNT:
            assert np.array_equal(ens.counter(k), ref["counters"][k]), k
        assert (ens.counter("nst") == 0).all() and (ens.counter("n_attempts") == 0).all()
        before = state(ens)
        st, tret = ens.solve(float(p["touts"][1]))
        assert (st == -2).all() and np.array_equal(tret, rec[0][1])
        same(state(ens), before)


# ------------------------------------------------------------------------------------------------ streaming
@pytest.mark.parametrize("kind,slices", [("linear_dense", ((150, 40), (1, 0), (1, 0), (77, 0), (120, 0))),
                                         ("lorenz63", ((300, 40), (1, 0), (1, 0), (77, 0), (400, 0)))])
def test_streaming_restarts_fail_before_the_first_step_again(kind, slices):
    """idaens_stream with a recovering first-step recipe: every restart (Ida::new again) takes the Q5 path again. Device stepper ==
    host stepper on totals and state() after the same rounds (the lock-step stepper under the guard of the existing stream tests: no
    Newton solve had to start over), and every system that has stepped since its last restart shows the oracle's nfail_first."""
    case = F.first_step_case(kind, 24, 1.0)
    touts, ed = case["after"], case["edited"]
    nff = F.oracle_reference(case)["nfail_first"]
    cd, dev = open_on(case, 1)
    ch, host = open_on(case, 0)
    compared = 0
    for k, stag in slices:
        pd = dev.stream(touts, k, stagger_rounds=stag)
        ph = host.stream(touts, k, stagger_rounds=stag)
        assert dev.total_rounds() == host.total_rounds()
        if kind == "lorenz63" or ((host.counter("nls_nconvfails") == 0).all() and host.total_newton_iters() == dev.total_newton_iters()):
            assert pd == ph and dev.total_newton_iters() == host.total_newton_iters()
            same(state(dev), state(host))
            compared += 1
    assert compared >= 3 and pd >= len(ed), (compared, pd)  # every system has restarted at least once
    c = dev.counters()
    stepped = c["nst"] > 0
    print("passes", pd, "nst", c["nst"], "nfail_first", c["nfail_first"])
    assert stepped[ed].any() and np.array_equal(c["nfail_first"][stepped], nff[stepped]) and (nff[ed] > 0).all()


@pytest.mark.parametrize("kind,device_ctl", [("linear_dense", 0), ("linear_dense", 1), ("lorenz63", 1)])
def test_stream_reports_the_system_that_died(kind, device_ctl):
    """A terminal first-step recipe in system 1 only: idaens_stream fails with -5 and names that system and its status, on the host
    stepper, the lock-step and the one-thread device steppers; it ran no more rounds than it was asked for, and says so again when
    called again (the other systems are still on their way)."""
    import idahip
    case = F.first_step_case(kind, 24, 1.0e2 if kind == "linear_dense" else 1.0e4, expect="first_terminal", edited=[1])
    nff = F.census(case)[0]
    assert nff["status"] == -3 and nff["nst"] == 0
    ctx, ens = open_on(case, device_ctl)
    with pytest.raises(idahip.IdaHipError, match=r"\(-5\): system 1 failed with status -3 while streaming"):
        ens.stream(case["after"], 40)
    rounds = ens.total_rounds()
    assert 0 < rounds <= 40
    c = ens.counters()
    assert c["nst"][1] == 0 and c["netf"][1] == 10 and c["nfail_first"][1] == nff["nfail_first"]
    assert (np.delete(c["nst"], 1) > 0).all() and (np.delete(c["nfail_first"], 1) == 0).all()
    with pytest.raises(idahip.IdaHipError, match=r"system 1 failed with status -3 while streaming"):
        ens.stream(case["after"], 5)
    assert ens.total_rounds() <= rounds + 5
    c2 = ens.counters()
    assert c2["n_attempts"][1] == c["n_attempts"][1] and (np.delete(c2["n_attempts"], 1) > np.delete(c["n_attempts"], 1)).all()
