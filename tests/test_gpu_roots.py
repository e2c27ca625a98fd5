"""Root finding (idaens_set_roots) on both device steppers and on the host stepper against the oracle's own root finding, switched on
for every problem the oracle has through tests/roots_oracle.py (g_i = y[comp_i] - thr_i behind oracle::Problem's num_roots / root).
The cases are tests/roots_cases.py's, whose census tests/test_roots_oracle.py takes on the CPU. After every call: status, tret, yy, yp,
tn, hh, hused, kused, nst, nre, nni, netf, ncfn, nsetups, the stop time left, rootsfound and the root-function evaluations, bit for bit
(yy / yp by value on a band ctx, whose linear solver is not the oracle's). There is no tolerance in this file.

Which kernel instantiation each test runs (every test asserts idaens_device_controller_active() before it trusts its run):
  test_every_case_equals_the_oracle        tiny_ida_kernel<ROBERTS, true, false> (roberts, roberts012), <LORENZ63, true, false> (lorenz);
                                           round_begin / round_end_kernel<true, false> (linear24, linear300, heat20, heat1100: plain,
                                           zero_at_t0, masked, 1 and 4 functions) and <true, true> (their tstop variants); five functions:
                                           the host stepper (IDAHIP_MAX_ROOTS = 4)
  test_heat20_on_a_band_ctx                round_*_kernel<true, false> and <true, true> over the band solver
  test_constraint_twins_of_the_tiny_kernel tiny_ida_kernel<ROBERTS, true, true>, <LORENZ63, true, true>
  test_lorenz_x_nonneg_with_roots          tiny_ida_kernel<LORENZ63, true, true> with a constraint that bites
  test_round_limited_calls                 tiny_ida_kernel<LORENZ63, true, false>, round_*_kernel<true, false>, one launch per k rounds
  test_schedules_end_at_the_first_root     the same two through idaens_solve_schedule
  test_brusselator_rounds_equal_the_host_stepper  round_*_kernel<true, false> on the BRUSS1D residual
"""
import numpy as np
import pytest

import roots_cases as RC
import roots_oracle as RO
import stepper_ref as R
import tstop_cases as K
import tstop_oracle as T

pytestmark = pytest.mark.gpu

IDAHIP_MAX_ROOTS = 4


def open_case(c, device_ctl, band=False, constraints=None, mxstep=None, prob=None):
    import idahip
    from idahip import problems
    prob = c["prob"] if prob is None else prob
    ctx = problems.make_ctx(prob, band=band)
    if c["id"] is not None:
        ctx.set_id(c["id"])
        ctx.set_suppress_alg(True)
    if constraints is not None:
        ctx.set_constraints(constraints)
    ens = idahip.Ensemble(ctx, prob["yy0"], prob["yp0"])
    ens.set_device_controller(device_ctl)
    if mxstep is not None:
        ens.set_max_num_steps(mxstep)
    ens.set_roots(*c["roots"])
    return ctx, ens


def expected_stepper(c, device_ctl):
    return c["stepper"] if device_ctl and len(c["roots"][0]) <= IDAHIP_MAX_ROOTS else 0


def run_case(c, device_ctl, band=False, constraints=None):
    ctx, ens = open_case(c, device_ctl, band=band, constraints=constraints)
    assert ens.device_controller_active() == expected_stepper(c, device_ctl)
    d = RC.ProductDriver(ens)
    ops = RC.drive(c, d)
    assert ens.device_controller_active() == expected_stepper(c, device_ctl)
    RC.compare(d.rec, RC.reference(c, ops), by_value=band, what="%s ctl=%d band=%s" % (c["name"], device_ctl, band))
    assert any((r["status"] == T.ROOT_RETURN).any() for r in d.rec)
    ens.close()
    ctx.close()
    return d.rec


@pytest.mark.parametrize("device_ctl", [0, 1])
@pytest.mark.parametrize("name,variant,nroots", RC.all_cases(), ids=lambda v: "" if v is None else str(v))
def test_every_case_equals_the_oracle(name, variant, nroots, device_ctl):
    c = RC.case(name, variant, nroots)
    rec = run_case(c, device_ctl)
    if variant == "tstop":
        assert any((r["status"] == T.TSTOP_RETURN).any() for r in rec)
    if variant == "zero_at_t0":
        assert (rec[0]["tret"] > 0.0).all() and rec[0]["nge"][0] >= 2  # nobody reports a root at t0; system 0 took r_check1's second look


@pytest.mark.parametrize("device_ctl", [0, 1])
@pytest.mark.parametrize("variant", RC.VARIANTS)
def test_heat20_on_a_band_ctx(variant, device_ctl):
    run_case(RC.case("heat20", variant), device_ctl, band=True)


@pytest.mark.parametrize("name,constraints", [("roberts", [1.0, 1.0, 1.0]), ("roberts012", [1.0, 1.0, 1.0]), ("lorenz", [0.0, 0.0, 1.0])])
def test_constraint_twins_of_the_tiny_kernel(name, constraints):
    """Constraints the oracle's trajectory never violates (every Roberts concentration >= 0; Lorenz' z >= 0) change nothing: with roots on,
    the constrained instantiation of the one-thread stepper still equals the unconstrained oracle in every return and counter, ncfn
    included (a constraint failure would count there)."""
    c = RC.case(name)
    rec = run_case(c, 1, constraints=np.array(constraints))
    assert (rec[-1]["ncfn"] == 0).all()


def test_lorenz_x_nonneg_with_roots():
    """THE WEAKER CHECK OF THIS FILE: tests/constr_cases.py's lorenz_x_nonneg (x >= 0 on an attractor whose x changes sign: corrections
    and constraint failures until mxstep) with roots on y and z. The constraint bites, and no oracle has both constraints and roots, so
    the one-thread device stepper is compared with the host stepper only -- which instantiates the same ida_solve_flow.hpp text: every
    return and counter equal, root returns and constraint failures both seen."""
    import constr_cases as CC
    cc = CC.lorenz_x_nonneg()
    c = {"name": "lorenz_x_nonneg", "prob": cc["prob"], "touts": [float(t) for t in cc["touts"]], "id": None, "stops": None, "stepper": 1,
         "roots": ([1, 2], RC.thresholds("lorenz", [1, 2]))}
    recs = {}
    for device_ctl in (1, 0):
        ctx, ens = open_case(c, device_ctl, constraints=cc["c"], mxstep=cc["mxstep"])
        assert ens.device_controller_active() == device_ctl
        d = RC.ProductDriver(ens)
        RC.drive(c, d, max_returns=400)  # (the attractor crosses the two thresholds many times before t = 5)
        recs[device_ctl] = d.rec
        ens.close()
        ctx.close()
    RC.compare(recs[1], recs[0], what="lorenz_x_nonneg: device against host stepper")
    assert any((r["status"] == T.ROOT_RETURN).any() for r in recs[1]) and (recs[1][-1]["ncfn"] > 0).any()


def _row(r, b):
    return {k: v[b:b + 1] for k, v in r.items()}


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", ["linear24", "lorenz"])
def test_round_limited_calls(name, k):
    """solve(t, max_rounds=k) repeated while any system is unfinished: the root state travels host -> device -> host around every
    launch (copy_roots / wg_copy_root). A system that has returned enters its next call while the others are still inside theirs, so
    every system makes its own sequence of calls: each is replayed on the oracle by itself and every completed return must equal it,
    nge, rootsfound and the returns after a root included. The root returns (tret, yy, yp, rootsfound, nst) are those of the
    unlimited run, which test_every_case_equals_the_oracle compares with the oracle."""
    c = RC.case(name)
    B = c["prob"]["yy0"].shape[0]
    ctx, ens = open_case(c, 1)
    assert ens.device_controller_active() == c["stepper"]
    d = RC.ProductDriver(ens, max_rounds=k)
    ops = [[] for _ in range(B)]
    got = [[] for _ in range(B)]
    idle = np.ones(B, dtype=bool)
    ncalls = unfinished = 0
    for t in c["touts"]:
        for _ in range(20000):
            st = d.solve(float(t), T.NORMAL)
            ncalls += 1
            unfinished += int((st == 99).sum())
            for b in range(B):
                if idle[b]:
                    ops[b].append(("solve", float(t), T.NORMAL))
                if st[b] != 99:
                    got[b].append(_row(d.rec[-1], b))
            idle = st != 99
            d.rec.clear()
            if ((st == T.SUCCESS) | (st < 0)).all():
                break
        else:
            raise AssertionError("no end of round-limited calls at tout %g: %s" % (t, st))
    assert ens.device_controller_active() == c["stepper"]
    ens.close()
    ctx.close()
    print(name, "k", k, "calls", ncalls, "entries per system", [len(o) for o in ops])
    assert unfinished > 0  # the limit did cut calls short
    plain = RC.reference(c, RC.ops_on_harness(c))
    for b in range(B):
        want = RO.run_ops(c["prob"], ops[b], ids=[b], **c["how"])[0]
        RC.compare(got[b], want, what="%s k=%d system %d" % (name, k, b))
        roots = lambda rec, q: [(r["tret"][q], r["yy"][q].tobytes(), r["yp"][q].tobytes(), r["iroots"][q].tolist(), r["nst"][q])
                                for r in rec if r["status"][q] == T.ROOT_RETURN]
        assert roots(got[b], 0) == roots(plain, b) and len(roots(plain, b)) >= 1, (name, k, b)


@pytest.mark.parametrize("name", ["linear24", "lorenz"])
def test_schedules_end_at_the_first_root(name):
    """idaens_solve_schedule with roots on both device steppers: every system walks the touts by itself and its schedule ends at its
    first root return. reached, status, tret, yy, yp, rootsfound and nge equal the oracle's call-by-call replay of that system."""
    c = RC.case(name)
    prob, touts = c["prob"], c["touts"]
    B = prob["yy0"].shape[0]
    ctx, ens = open_case(c, 1)
    assert ens.device_controller_active() == c["stepper"]
    st, tret, reached = ens.solve_schedule(touts)
    assert ens.device_controller_active() == c["stepper"]
    yy, yp, iroots, nge = ens.yy(), ens.yp(), ens.roots_found(), ens.counter("nge")
    ens.close()
    ctx.close()
    assert (st == T.ROOT_RETURN).all(), st
    for b in range(B):
        h = RO.Harness(prob, b, **c["how"])
        nreached = 0
        for t in touts:
            st_o, tret_o = h.solve(t)
            if st_o != T.SUCCESS:
                break
            nreached += 1
        s = h.state()
        assert (st[b], reached[b]) == (st_o, nreached), (b, st[b], reached[b], st_o, nreached)
        assert R.same_bits(tret[b], np.float64(tret_o)) and R.same_bits(yy[b], s["yy"]) and R.same_bits(yp[b], s["yp"]), b
        assert np.array_equal(iroots[b], s["iroots"]) and nge[b] == s["nge"], (b, iroots[b], s["iroots"], nge[b], s["nge"])
    print(name, "reached", reached.tolist())


def test_brusselator_rounds_equal_the_host_stepper():
    """bruss1d n = 16 (the systems tests/test_gpu_bruss.py integrates) with roots on components 1, 8 and 15: the oracle has no
    Brusselator, so this is the device lock-step rounds against the host stepper only, every return and counter. Thresholds: the
    recipe of tests/roots_cases.py, with the host stepper's own run without roots in the oracle's place."""
    import idahip
    from idahip import problems
    import bruss_ref as BR
    ids = [1, 3, 4, 6]
    prob = BR.select(problems.bruss1d(m=8, batch=max(ids) + 1), ids)
    touts, comps = [0.25, 0.5], [1, 8, 15]
    ctx = problems.make_ctx(prob)
    ens = idahip.Ensemble(ctx, prob["yy0"], prob["yp0"])
    ens.set_device_controller(0)
    st, _ = ens.solve(touts[-1])
    assert (st == 0).all()
    thr = [0.5 * (float(prob["yy0"][0, q]) + float(ens.yy()[0, q])) for q in comps]
    ens.close()
    ctx.close()
    c = {"name": "bruss16", "prob": prob, "touts": touts, "id": None, "stops": None, "stepper": 2, "roots": (comps, thr)}
    recs = {}
    for device_ctl in (1, 0):
        ctx, ens = open_case(c, device_ctl)
        assert ens.device_controller_active() == (2 if device_ctl else 0)
        d = RC.ProductDriver(ens)
        RC.drive(c, d)
        recs[device_ctl] = d.rec
        ens.close()
        ctx.close()
    RC.compare(recs[1], recs[0], what="bruss16: device rounds against host stepper")
    nroot = np.sum([r["status"] == T.ROOT_RETURN for r in recs[1]], axis=0)
    print("bruss16 thresholds", thr, "root returns per system", nroot.tolist())
    assert (nroot >= 1).any(), nroot
