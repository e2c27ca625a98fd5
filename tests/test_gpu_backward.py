"""Integration in the negative time direction (tout < t0, hh < 0) on all three steppers, against the references of
tests/backward_cases.py whose census is tests/test_backward_oracle.py's:

  a. whole backward runs (every tout, one solve_schedule call, ONE_STEP with an interpolation inside the last step);
  b. roots while going backward (component thresholds, a user root function, a root exactly at a tout, masked norms);
  c. stop times behind t0 (per-system, NaN = none, the clip, TSTOP_RETURN, the wrong side, set_stop_time's refusal);
  d. get_dky after backward steps (every k, t inside the last step, beyond tn, behind the last step);
  e. DQ Jacobians with hh < 0 (one setup against tests/dq_ref.py with per-system negative hh; whole runs);
  f. calc_ic with tout1 < t0 (negative hic and cj), calc_ic_systems with tout1 of both signs, then the first backward solve;
  g. a Krylov ctx going backward (plain and with the band preconditioner, host stepper and lock-step rounds);
  h. constraints that become active on a backward run;
  i. the mirror property on the product: a forward run of P and a backward run of mirror(P) in one process, no reference at all;
  j. changing direction: a tout inside the last step interpolates, a tout behind it is IDAENS_BAD_T and sticky, in both directions.

Dense contexts are compared bit for bit, band contexts (and the band preconditioner) by value, as everywhere in this suite. There is
no tolerance in this file."""
import numpy as np
import pytest

import backward_cases as BC
import stepper_ref as R
import tstop_oracle as T

pytestmark = pytest.mark.gpu
STEPPERS = ["host_plain", "host_fused", "device"]
F_YY, F_YP, F_YYPREDICT, F_YPPREDICT, F_EWT, F_EE, F_DELTA, F_SAVRES = range(8)


def open_case(c, stepper, band=False, dq=False, krylov=None, constr=None, rounds=False, prob=None, mxstep=None):
    """-> (ctx, ens) of the case on a stepper, with the expected stepper asserted as tests/test_gpu_reinit.open_case does."""
    import idahip
    from idahip import problems
    prob = BC.product_problem(c["kind"], c["prob"] if prob is None else prob)
    ctx = problems.make_ctx(prob, band=c["band"] if band else False, krylov=5 if krylov else None)
    if krylov and krylov != "plain":
        ctx.set_krylov_band_prec(*krylov)
    if rounds:
        ctx.set_krylov_rounds(True)
    if c["id"] is not None:
        ctx.set_id(c["id"])
        ctx.set_suppress_alg(True)
    if dq:
        ctx.set_jacobian_dq(True)
    if constr is not None:
        ctx.set_constraints(constr)
    ens = idahip.Ensemble(ctx, prob["yy0"], prob["yp0"])
    ens.set_device_controller(1 if stepper == "device" else 0)
    if stepper != "device":
        ens.set_fused_newton(stepper == "host_fused")
    if len(c["roots"][0]):
        ens.set_roots(*c["roots"])
    if mxstep is not None:
        ens.set_max_num_steps(mxstep)
    want = 0 if stepper != "device" or (krylov and not rounds) else c["stepper"]
    assert ens.device_controller_active() == want, (c["name"], stepper, ens.device_controller_active())
    return ctx, ens


def replay(d, ops):
    for op in ops:
        if op[0] == "stop":
            d.stop(op[1])
        elif op[0] == "stop_rel":
            d.stop_rel(op[1], op[2])
        else:
            d.solve(op[1], op[2])
    return d.rec


def run(c, stepper, ops=None, how=None, by_value=False, counters=False, **form):
    """The case on a stepper and in a form (open_case's switches): its own script (ops None) or the given ops, every call compared
    with the reference; counters: the DQ and Krylov counters as well. -> (records, ops)."""
    ctx, ens = open_case(c, stepper, **form)
    d = BC.Product(ens)
    if ops is None:
        ops = BC.drive(c, d)
    else:
        replay(d, ops)
    ens.close()
    ctx.close()
    BC.compare(d.rec, BC.reference(c, ops, how), by_value=by_value, what="%s %s %s" % (c["name"], stepper, form), krylov=counters)
    assert (d.rec[-1]["hh"][d.rec[-1]["nst"] > 0] < 0.0).all()
    return d.rec, ops


def steppers_of(name):
    return STEPPERS[:2] if name == "heat20_twin" else STEPPERS


# ------------------------------------------------------------------------------------------------ a. whole backward runs
PLAIN = [(n, s) for n in BC.CASES for s in steppers_of(n)]


@pytest.mark.parametrize("name,stepper", PLAIN)
def test_whole_backward_runs_equal_the_reference(name, stepper):
    c = BC.case(name)
    rec, _ = run(c, stepper, ops=BC.plain_ops(c), how={} if c["ref"] == "python" else None)
    assert (rec[-1]["status"] == T.SUCCESS).all() and (rec[-1]["tret"] == c["touts"][-1]).all() and (rec[-1]["nst"] >= 20).all()


@pytest.mark.parametrize("stepper", ["host_fused", "device"])
@pytest.mark.parametrize("name", ["heat20", "bruss6"])
def test_whole_backward_runs_on_a_band_ctx(name, stepper):
    c = BC.case(name)
    run(c, stepper, ops=BC.plain_ops(c), how={} if c["ref"] == "python" else None, by_value=True, band=True)


@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("name", ["lorenz", "linear24", "chain12"])
def test_the_touts_as_one_schedule(name, stepper):
    c = BC.case(name)
    ref = BC.reference(c, BC.plain_ops(c), {} if c["ref"] == "python" else None)
    ctx, ens = open_case(c, stepper)
    st, tret, reached, yo, ypo = ens.solve_schedule(c["touts"], outputs=True)
    assert (st == T.SUCCESS).all() and (tret == c["touts"][-1]).all() and (reached == len(c["touts"])).all()
    for i, r in enumerate(ref):
        assert R.same_bits(yo[i], r["yy"]) and R.same_bits(ypo[i], r["yp"]), (name, stepper, i)
    last = ref[-1]
    assert R.same_bits(ens.yy(), last["yy"]) and R.same_bits(ens.yp(), last["yp"])
    for k in ("tn", "hh", "hused"):
        assert R.same_bits(ens.real(k), last[k]), k
    for k in ("kused", "nst", "nre", "nni", "nje", "netf", "ncfn", "nsetups", "n_attempts", "nls_nconvfails"):
        assert np.array_equal(ens.counter(k), last[k].astype(np.int64)), k
    ens.close()
    ctx.close()


@pytest.mark.parametrize("stepper", ["host_plain", "host_fused"])
@pytest.mark.parametrize("name", ["roberts", "linear24", "heat20_twin"])
def test_one_step_mode_and_an_interpolation_inside_the_last_step(name, stepper):
    """Twelve IDA_ONE_STEP calls (tret = tn each), then IDA_NORMAL with a tout inside system 0's last step -- stop_test1's
    (tn - tout) * hh >= 0 with hh < 0: an interpolation for it; for the others an interpolation, further steps or IDAENS_BAD_T,
    whichever the reference says -- then ONE_STEP again."""
    c = BC.case(name)
    ctx, ens = open_case(c, stepper)
    d = BC.Product(ens)
    far = c["touts"][-1] * 100.0
    ops = [("solve", far, T.ONE_STEP)] * 12
    replay(d, ops)
    assert all((r["tret"] == r["tn"]).all() and (r["status"] == T.SUCCESS).all() for r in d.rec)
    assert (np.diff(np.array([r["tn"] for r in d.rec]), axis=0) < 0.0).all()  # tn goes down, step by step
    tn, hused = ens.real("tn"), ens.real("hused")
    inside = float(tn[0] - 0.5 * hused[0])
    assert tn[0] < inside < tn[0] - hused[0]
    more = [("solve", inside, T.NORMAL), ("solve", far, T.ONE_STEP), ("solve", far, T.ONE_STEP)]
    replay(d, more)
    assert d.rec[12]["status"][0] == T.SUCCESS and d.rec[12]["tret"][0] == inside and d.rec[12]["nst"][0] == 12
    ens.close()
    ctx.close()
    BC.compare(d.rec, BC.reference(c, ops + more), what="%s %s one_step" % (name, stepper))


# ------------------------------------------------------------------------------------------------ b. roots while going backward
ROOT_RUNS = [(n, v, s) for n in ("lorenz", "roberts", "linear24", "heat20") for v in ("roots", "root_at_tout", "roots_tstop")
             for s in STEPPERS]


@pytest.mark.parametrize("name,variant,stepper", ROOT_RUNS)
def test_roots_while_going_backward(name, variant, stepper):
    c = BC.case(name, variant)
    rec, _ = run(c, stepper)
    found = [(r["status"] == T.ROOT_RETURN) & (r["hh"] < 0.0) for r in rec]
    assert sum(int(f.sum()) for f in found) >= 1 and any(r["iroots"][f].any() for r, f in zip(rec, found))
    if variant == "root_at_tout":
        assert any(r["status"][0] == T.ROOT_RETURN and r["tret"][0] == c["touts"][0] and r["iroots"][0][0] != 0 for r in rec)
    if variant == "roots_tstop":
        assert any((r["status"] == T.TSTOP_RETURN).any() for r in rec)


@pytest.mark.parametrize("stepper", ["host_fused", "device"])
def test_roots_on_a_band_ctx_and_with_masked_norms(stepper):
    run(BC.case("heat20", "roots"), stepper, by_value=True, band=True)
    run(BC.case("linear24", "masked"), stepper)


def test_a_user_root_function_through_the_callback():
    """idaens_set_root_fn with the case's own functions written in numpy: the same returns, iroots and nge as the reference."""
    c = BC.case("linear24", "roots")
    comps, thr = np.array(c["roots"][0]), np.array(c["roots"][1])
    plain = dict(c, roots=([], []))
    ctx, ens = open_case(plain, "host_fused")
    ens.set_root_fn(len(comps), lambda s, t, yy, yp: yy[comps] - thr)
    d = BC.Product(ens)
    ops = BC.drive(c, d)
    assert ctx.take_callback_error() is None
    ens.close()
    ctx.close()
    BC.compare(d.rec, BC.reference(c, ops), what="linear24 root_fn")
    assert any((r["status"] == T.ROOT_RETURN).any() for r in d.rec)


# ------------------------------------------------------------------------------------------------ c. stop times behind t0
@pytest.mark.parametrize("stepper", ["host_fused", "device"])
@pytest.mark.parametrize("name", ["roberts", "linear24", "heat20"])
def test_stop_times_behind_t0(name, stepper):
    """tests/tstop_cases.py's "residues" script with a negative first tout: a per-system array with NaN for none, the clip of the
    first and of a later step, TSTOP_RETURN with tret == tstop, and a stop time on the wrong side: ILL_INPUT before the first step."""
    c = BC.case(name, "tstop")
    rec, _ = run(c, stepper)
    B = rec[0]["status"].size
    assert any((r["status"] == T.TSTOP_RETURN).any() for r in rec)
    assert (rec[0]["status"][np.arange(B) % 7 == 2] == T.TSTOP_RETURN).all()  # the tiny stop time: the first step is clipped to it
    wrong = np.arange(B) % 7 == 6
    assert (rec[0]["status"][wrong] == T.ILL_INPUT).all() and (rec[0]["nst"][wrong] == 0).all() and (rec[0]["tret"][wrong] == 0.0).all()
    if name == "heat20":
        run(c, stepper, by_value=True, band=True)


@pytest.mark.parametrize("stepper", ["host_plain", "host_fused"])
def test_stop_times_between_calls_in_both_tasks(stepper):
    run(BC.case("linear24", "entry"), stepper)


@pytest.mark.parametrize("stepper", ["host_fused", "device"])
def test_set_stop_time_after_backward_steps(stepper):
    """IDASetStopTime's check with hh < 0: a stop time between t0 and tn is behind the system and refused, nothing changed; one
    beyond tn is taken, and a schedule ends at its TSTOP return."""
    import idahip
    c = BC.case("linear24")
    t1 = c["touts"][0]
    ctx, ens = open_case(c, stepper)
    B = ctx.batch
    st, _ = ens.solve(t1)
    assert (st == 0).all() and (ens.real("tn") <= t1).all() and (ens.real("hh") < 0.0).all()
    keep = np.full(B, np.nan)
    keep[1] = 7.0 * t1
    ens.set_stop_time(keep)
    bad = np.full(B, 9.0 * t1)
    bad[2] = 0.5 * t1
    with pytest.raises(idahip.IdaHipError, match="system 2 is behind its current t"):
        ens.set_stop_time(bad)
    with pytest.raises(idahip.IdaHipError, match="system 0 is behind"):
        ens.set_stop_time(-t1)  # the other side of t0 altogether
    assert R.same_bits(ens.stop_time(), keep)
    ts = np.full(B, np.nan)
    ts[1] = 2.5 * t1
    ens.set_stop_time(ts)
    st, tret, reached = ens.solve_schedule([2 * t1, 3 * t1, 4 * t1])
    want = np.zeros(B, dtype=np.int32)
    want[1] = T.TSTOP_RETURN
    assert np.array_equal(st, want) and reached.tolist() == [3 if b != 1 else 1 for b in range(B)]
    assert tret[1] == 2.5 * t1 and (np.delete(tret, 1) == 4 * t1).all() and np.isnan(ens.stop_time()).all()
    assert ens.real("tn")[1] >= 2.5 * t1 - 1e-12  # no step beyond the stop time
    ens.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------ d. get_dky after backward steps
@pytest.mark.parametrize("stepper", ["host_fused", "device"])
@pytest.mark.parametrize("name", ["lorenz", "linear24"])
def test_get_dky_after_backward_steps(name, stepper):
    """Every k up to kused + 1 at t inside the last step, at tret, beyond tn (an extrapolation, allowed) and behind the last step
    (IDAENS_BAD_T: the sign of (t - tp) * hh), for every system against the oracle's get_dky on the same state."""
    c = BC.case(name)
    ops = BC.plain_ops(c)
    ctx, ens = open_case(c, stepper)
    replay(BC.Product(ens), ops)
    hs = BC.reference_systems(c, ops)
    tn, hused, kused = ens.real("tn"), ens.real("hused"), ens.counter("kused")
    assert (hused < 0.0).all() and kused.max() >= 3
    seen = set()
    for t in (c["touts"][-1], float(tn[0] - 0.5 * hused[0]), float(tn[0] + 0.5 * hused[0]), float(tn[0] - 3.0 * hused[0]),
              float(tn.max() - 3.0 * hused.min())):
        for k in range(0, int(kused.max()) + 2):
            status, dky = ens.get_dky(t, k)
            for s, h in enumerate(hs):
                st_o, d_o = BC.harness_get_dky(h, t, k)
                assert status[s] == st_o, (name, t, k, s, status[s], st_o)
                seen.add(int(st_o))
                if st_o == 0:
                    assert R.same_bits(dky[s], d_o), (name, t, k, s)
                else:
                    assert np.isnan(dky[s]).all()
    assert seen == {0, -25, -26}, seen
    status, _ = ens.get_dky(float(tn.max() - 3.0 * hused.min()), 0)  # behind the last step of every system
    assert (status == -26).all()
    status, _ = ens.get_dky(float(tn.min() + 0.25 * hused.max()), 0)  # beyond every tn: the polynomial extrapolates
    assert (status == 0).all()
    ens.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------ e. DQ Jacobians with hh < 0
def dq_state(name):
    """-> (prob, yy, yp, ewt, cj [B], hh [B] all negative): the case's start, y' made non-zero in every component so that dq_inc's
    sign(hh * yp_j) takes both values, a negative step size of its own per system and cj = 1 / hh."""
    prob = BC.problem(name)
    B, n = prob["yy0"].shape
    g = np.random.Generator(np.random.PCG64([11, n, B]))
    yy = prob["yy0"] + 1.0e-3 * g.uniform(-1.0, 1.0, (B, n))
    yp = prob["yp0"] + g.uniform(-1.0, 1.0, (B, n))
    atol = np.broadcast_to(prob["atol"], (n,)) if np.size(prob["atol"]) == n else float(np.ravel(prob["atol"])[0])
    ewt = 1.0 / (prob["rtol"] * np.abs(yy) + atol)
    hh = -(10.0 ** g.uniform(-5.0, -2.0, B))
    return prob, yy, yp, ewt, 1.0 / hh, hh


def load_state(ctx, yy, yp, ewt, cj):
    ctx.upload(F_YYPREDICT, yy)
    ctx.upload(F_YPPREDICT, yp)
    ctx.upload(F_EWT, ewt)
    ctx.nls_sys(0.0, cj, True)
    return ctx.download(F_YY), ctx.download(F_YP), ctx.download(F_SAVRES)


@pytest.mark.parametrize("name,band", [("lorenz", None), ("linear24", None), ("heat20", None), ("heat20", (1, 1)), ("chain12", None)], ids=str)
def test_one_dq_setup_with_negative_step_sizes(name, band):
    """idahip_jac_dq on uploaded state with per-system hh < 0 (and cj = 1 / hh < 0) against tests/dq_ref.py: the tiny, dense, band
    and table-driven forms of dq_inc."""
    import dq_ref as DQ
    from idahip import problems
    prob, yy, yp, ewt, cj, hh = dq_state(name)
    ctx = problems.make_ctx(prob, band=band or False)
    ctx.set_jacobian_dq(True)
    yy, yp, rr = load_state(ctx, yy, yp, ewt, cj)
    B = yy.shape[0]
    idx = np.arange(B, dtype=np.int32)[::-1].copy()
    J = ctx.jac_dq(0.0, cj[idx], hh[idx], idx)
    ctx.close()
    signs = np.sign(hh[:, None] * yp)
    assert (signs < 0).any() and (signs > 0).any()
    shows = False
    for q, s in enumerate(idx):
        res, _ = BC.res_jac_of(prob, s)
        assert R.same_bits(res(yy[s], yp[s]), rr[s]), ("residual restatement", name, s)
        a = (yy[s], yp[s], ewt[s], rr[s], cj[s], hh[s])
        if band is not None:
            want = DQ.band_dq(res, *a, *band)
        elif prob["kind"] == "linear_dense":
            want = DQ.linear_dense_dq(prob["A"][s], prob["B"][s], prob["c"][s], *a)
        elif prob["kind"] == "heat1d":
            want = DQ.heat_dense_dq_banded(float(prob["params"][s, 0]), *a)
        else:
            want = DQ.dense_dq(res, *a)
        assert R.same_bits(J[q], want), (name, band, s)
        # with the other sign of hh the increments are mirrored: the restatement itself gives other bits for this state
        ref = (lambda h: DQ.dense_dq(res, *a[:5], h)) if band is None else (lambda h: DQ.band_dq(res, *a[:5], h, *band))
        shows = shows or not R.same_bits(ref(-hh[s]), ref(hh[s]))
    assert shows, "the sign of hh does not show in this state"


def test_the_preconditioner_band_dq_with_negative_step_sizes():
    import krylov_prec_ref as PR
    from idahip import problems
    prob, yy, yp, ewt, cj, hh = dq_state("heat20")
    ctx = problems.make_ctx(prob, krylov=5)
    ctx.set_krylov_band_prec(1, 1)
    yy, yp, rr = load_state(ctx, yy, yp, ewt, cj)
    info = ctx.krylov_psetup(0.0, cj, hh)
    assert not info.any()
    for s in range(yy.shape[0]):
        res, _ = BC.res_jac_of(prob, s)
        ri, rab, rpiv = PR.psetup(res, yy[s], yp[s], ewt[s], rr[s], cj[s], hh[s], 1, 1)
        ab, piv = ctx.krylov_download_prec(s)
        assert ri == 0 and np.array_equal(piv, rpiv) and np.array_equal(ab, rab), s
    ctx.close()


DQ_RUNS = [("lorenz", "dense", False), ("linear24", "dense", False), ("heat20", "dense", False), ("heat20", (1, 1), True), ("chain12", "dense", False)]


@pytest.mark.parametrize("stepper", ["host_fused", "device"])
@pytest.mark.parametrize("name,dq,band", DQ_RUNS, ids=str)
def test_whole_backward_runs_with_dq_jacobians(name, dq, band, stepper):
    c = BC.case(name)
    rec, _ = run(c, stepper, ops=BC.plain_ops(c), how={"dq": dq}, by_value=band, counters=True, dq=True, band=band)
    assert (rec[-1]["nre_dq"] > 0).all() and (rec[-1]["status"] == 0).all()


# ------------------------------------------------------------------------------------------------ f. calc_ic with tout1 < t0
IC_CASES = ["roberts_satol", "linear40_mixed", "linear40_yinit", "linear9_dq", "heat16_band", "heat16_band_dq", "linear40_singular", "bruss32_mixed"]


@pytest.mark.parametrize("name", IC_CASES)
def test_calc_ic_with_a_first_tout_behind_t0(name):
    """tests/calcic_cases.py's cases with tout1 negated: hic < 0, cj = 1 / hic < 0. YA_YDP_INIT and Y_INIT, analytic and DQ
    Jacobians, dense and band ctx, and two batches of the mixed-fates table: linear40_singular (one NO_RECOVERY after retries at
    hic / 10) and bruss32_mixed (successes, backtracking, CONV_FAIL and LINESEARCH_FAIL side by side)."""
    import calcic_cases as K
    import calcic_ref as IC
    import idahip
    c, r = K.case(name), BC.calcic_reference(name)
    exact = c["band"] is None
    ctx = K.make_ctx(c)
    ens = idahip.Ensemble(ctx, c["yy0"], c["yp0"])
    status = ens.calc_ic(c["icopt"], -c["tout1"])
    yy, yp, cnt, ewt = ens.yy(), ens.yp(), ens.counters(), ctx.download(F_EWT)
    ens.close()
    ctx.close()
    same = R.same_bits if exact else np.array_equal
    assert np.array_equal(status, r["status"]), (status, r["status"])
    assert (r["hic"][r["status"] == 0] < 0.0).all() and (r["status"] == 0).any()
    for k in IC.COUNTERS:
        assert np.array_equal(cnt[k], r["counters"][k]), (k, cnt[k], r["counters"][k])
    assert same(yy, r["yy"]) and same(yp, r["yp"])
    for b in np.flatnonzero(r["status"] == 0):
        assert same(ewt[b], r["ewt"][b]), ("ewt", b)


@pytest.mark.parametrize("stepper", STEPPERS)
def test_calc_ic_systems_with_tout1_of_both_signs_then_the_first_backward_solve(stepper):
    """Roberts from inconsistent values: every second listed system is corrected with tout1 < t0, the others with tout1 > t0, each
    against calcic_ref with its own tout1; the ensemble then integrates backwards, bit for bit as the oracle does from the
    corrected values."""
    import calcic_cases as K
    import calcic_ref as IC
    import idahip
    import reinit_oracle as RI
    c = K.case("roberts_satol")
    B = 16
    yy0, yp0 = c["yy0"][:B], c["yp0"][:B]
    ctx = K.make_ctx(dict(c, yy0=yy0, yp0=yp0))
    ens = idahip.Ensemble(ctx, yy0, yp0)
    ens.set_device_controller(1 if stepper == "device" else 0)
    if stepper != "device":
        ens.set_fused_newton(stepper == "host_fused")
    listed = np.array([9, 2, 5, 14, 0, 11, 7, 15, 3, 12, 1, 6, 13, 4, 10, 8], dtype=np.int32)
    tout1 = np.where(np.arange(B) % 2 == 0, -0.4, 0.4) * (1.0 + np.arange(B))
    status = ens.calc_ic_systems(idahip.YA_YDP_INIT, listed, tout1)
    yy, yp = ens.yy(), ens.yp()
    hic = np.zeros(B)
    for q, b in enumerate(listed):
        ref = IC.calc_ic(IC.device_problem("roberts", 3, {}), yy0[b], yp0[b], c["rtol"], c["atol"], IC.YA_YDP_INIT, float(tout1[q]), id=c["id"])
        hic[q] = ref["hic"]
        assert status[q] == ref["status"] == 0, (b, status[q], ref["status"])
        assert R.same_bits(yy[b], ref["yy"]) and R.same_bits(yp[b], ref["yp"]), b
    assert (hic[::2] < 0.0).all() and (hic[1::2] > 0.0).all()
    prob = {"kind": "roberts", "n": 3, "yy0": yy, "yp0": yp, "rtol": c["rtol"], "atol": c["atol"]}
    c0 = ens.counters()  # what calc_ic counted stays counted
    assert (c0["nst"] == 0).all() and (c0["nni"] > 0).all()
    d = BC.Product(ens)
    ops = [("solve", t, T.NORMAL) for t in (-0.02, -0.04)]
    replay(d, ops)
    assert ens.device_controller_active() == (1 if stepper == "device" else 0)
    ens.close()
    ctx.close()
    ref = T.run_ops(prob, ops, harness=RI.Harness, roots=([], []))[0]
    for r in d.rec:
        for k in ("nre", "nsetups", "nni", "nje", "ncfn"):
            r[k] = r[k] - c0[k]
    BC.compare(d.rec, ref, what="roberts after calc_ic %s" % stepper)
    assert (d.rec[-1]["status"] == 0).all() and (d.rec[-1]["hh"] < 0.0).all()


# ------------------------------------------------------------------------------------------------ g. a Krylov ctx going backward
@pytest.mark.parametrize("rounds", [False, True], ids=["host", "rounds"])
@pytest.mark.parametrize("krylov", ["plain", (1, 1)], ids=str)
def test_krylov_heat_going_backward(krylov, rounds):
    c = BC.case("heat20")
    rec, _ = run(c, "device", ops=BC.plain_ops(c), how={"krylov": krylov}, by_value=krylov != "plain", counters=True, krylov=krylov, rounds=rounds)
    assert (rec[-1]["status"] == 0).all() and (rec[-1]["nli"] > 0).all()
    assert krylov == "plain" or ((rec[-1]["npe"] > 0).all() and (rec[-1]["nps"] > 0).all())


# ------------------------------------------------------------------------------------------------ h. constraints
@pytest.mark.parametrize("stepper", ["host_plain", "host_fused"])
def test_a_constraint_becomes_active_going_backward(stepper):
    """(The lock-step device rounds have no constraint check: a ctx with constraints steps on the host for n > 8.)"""
    c = BC.case("heat20")
    how = BC.constraint_how()
    rec, ops = run(c, stepper, ops=BC.plain_ops(c), how=how, constr=how["constr"])
    free = BC.reference(c, ops, {})
    assert not np.array_equal(rec[-1]["yy"], free[-1]["yy"]) and (rec[-1]["yy"] >= 0.0).all()


@pytest.mark.parametrize("stepper", ["host_fused", "device"])
def test_a_constraint_stops_lorenz_going_backward(stepper):
    """The one-thread device stepper's own constraint check with hh < 0: corrections, recoveries with the step-size factor, and
    TOO_MUCH_WORK after mxstep steps of each call, as the reference."""
    c, how = BC.lorenz_constraint_case()
    rec, _ = run(c, stepper, ops=BC.plain_ops(c), how=how, constr=how["constr"], mxstep=how["mxstep"])
    assert (rec[-1]["status"] != 0).any() and (rec[-1]["ncfn"] > 0).any() and (rec[-1]["yy"][:, 1] > -1.0e-6).all()


# ------------------------------------------------------------------------------------------------ i. the mirror property on the product
MIRROR_RUNS = [(n, v, s) for n, v in [(n, "plain") for n in BC.MIRROR_EXACT] + [("linear24", "roots"), ("heat20", "roots")]
               for s in steppers_of(n)]


@pytest.mark.parametrize("name,variant,stepper", MIRROR_RUNS)
def test_mirror_property_on_the_product(name, variant, stepper):
    """A forward run of P and a backward run of mirror(P), the touts negated, on the same stepper in one process: yy and every
    counter bit for bit, tn, hh, hused, tret, yp negated. No reference takes part: a sign slip that a restatement shares shows here."""
    bwd = BC.case(name, variant)
    fwd = dict(bwd, prob=BC.forward_problem(name), touts=[-t for t in bwd["touts"]])
    recs = {}
    ops = None
    for key, c in (("bwd", bwd), ("fwd", fwd)):
        ctx, ens = open_case(c, stepper)
        d = BC.Product(ens)
        if ops is None:
            ops = BC.drive(c, d)
        else:
            replay(d, [(o[0], -o[1], o[2]) for o in ops])
        ens.close()
        ctx.close()
        recs[key] = d.rec
    assert (recs["bwd"][-1]["hh"] < 0.0).all() and (recs["fwd"][-1]["hh"] > 0.0).all() and (recs["bwd"][-1]["nst"] >= 20).all()
    BC.mirrored(recs["fwd"], recs["bwd"], what="%s %s %s" % (name, variant, stepper))


# ------------------------------------------------------------------------------------------------ j. changing direction
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("roots", [False, True], ids=["noroots", "roots"])
@pytest.mark.parametrize("direction", ["forward", "backward"])
@pytest.mark.parametrize("name", ["lorenz", "linear24"])
def test_a_tout_behind_the_last_step(name, direction, roots, stepper):
    """After steps in one direction: a tout inside system 0's last step interpolates, a tout behind the last step of every system is
    IDAENS_BAD_T -- with root functions from r_check3 at the call's entry, which does not evaluate them at the refused tout
    (include/ida_ensemble.h; these calls follow a SUCCESS, so r_check2 evaluates nothing either and nge stays) -- and the status is sticky: the next call, with a tout ahead, changes nothing. Status, tret, every counter and nge against the
    oracle harness (tests/roots_oracle.py models the evaluation the reference makes and the library does not)."""
    if direction == "backward":
        c = BC.case(name, "roots" if roots else "plain")
    else:  # tests/roots_cases.py's forward case of the same problem
        import roots_cases as RC
        c = dict(RC.case(name), kind=name, ref="oracle", band=None, script=None)
        if not roots:
            c.update(name=c["name"] + "/noroots", roots=([], []), how={"roots": ([], [])})
    t1, t2, t3 = c["touts"]
    ctx, ens = open_case(c, stepper)
    d = BC.Product(ens)
    ops = []

    def call(t):
        ops.append(("solve", float(t), T.NORMAL))
        return d.solve(float(t), T.NORMAL)

    for t in (t1, t2):  # to the second tout, through every root return on the way
        for _ in range(12):
            st = call(t)
            if ((st == T.SUCCESS) | (st < 0)).all():
                break
    alive = d.rec[-1]["status"] == T.SUCCESS
    assert alive.any()
    tn, hused = ens.real("tn"), ens.real("hused")
    sign = -1.0 if direction == "backward" else 1.0
    assert (sign * hused[alive] > 0.0).all()
    inside = float(tn[0] - 0.75 * hused[0])
    st = call(inside)
    assert st[0] == T.SUCCESS and d.rec[-1]["tret"][0] == inside and d.rec[-1]["nst"][0] == d.rec[-2]["nst"][0]
    before = d.rec[-1]
    st = call(0.5 * t1)  # behind every system's last step
    assert (st[alive] == -26).all(), st
    assert np.array_equal(d.rec[-1]["nge"], before["nge"]) and R.same_bits(d.rec[-1]["tret"], before["tret"])
    for t in (t3, t3):  # sticky: a tout ahead is not integrated to
        st = call(t)
        assert (st[alive] == -26).all()
        for k in ("nst", "nge", "nre", "nni"):
            assert np.array_equal(d.rec[-1][k], before[k]), k
    ens.close()
    ctx.close()
    BC.compare(d.rec, BC.reference(c, ops), what="%s %s roots=%s %s" % (name, direction, roots, stepper))


@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("name", ["lorenz", "linear24"])
def test_a_tout_behind_the_last_step_right_after_a_root_return(name, stepper):
    """The refused call directly after a ROOT_RETURN: r_check2 comes before r_check3 and evaluates g at tlo, and once more next to
    it where a function is zero there -- one or two evaluations that the refused call does make and count, on both sides. Only
    r_check3's evaluation at the refused tout is the one the library leaves out."""
    c = BC.case(name, "roots")
    ops = [("solve", float(t), T.NORMAL) for t in (c["touts"][-1], -c["touts"][0], c["touts"][-1])]
    ctx, ens = open_case(c, stepper)
    rec = replay(BC.Product(ens), ops)
    ens.close()
    ctx.close()
    assert (rec[0]["status"] == T.ROOT_RETURN).all() and (rec[1]["status"] == -26).all() and (rec[2]["status"] == -26).all()
    moved = rec[1]["nge"] - rec[0]["nge"]
    assert set(moved.tolist()) <= {1, 2} and R.same_bits(rec[1]["tret"], rec[0]["tret"]), moved
    for k in ("nge", "nst", "nre", "nni"):
        assert np.array_equal(rec[2][k], rec[1][k]), k  # sticky
    BC.compare(rec, BC.reference(c, ops), what="%s %s BAD_T after a root return" % (name, stepper))
