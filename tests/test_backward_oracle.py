"""The census of tests/backward_cases.py on the references alone (no GPU): every backward run that tests/test_gpu_backward.py compares
with is shown here not to be trivial, and the mirror property the GPU tests rely on is established for each kind that can be mirrored.

Per case: every system takes at least 20 steps, some system reaches order 3, at least three quarters of the systems end with SUCCESS
at the last tout; cases with roots return ROOT_RETURN while hh < 0; cases with a stop time return TSTOP_RETURN with tret == tstop
exactly; DQ cases see both signs of hh * yp_j at a Jacobian evaluation (both branches of dq_inc's mirrored increment).

Mirror property (tests/backward_cases.py): found exact -- yy and every counter bit for bit, tn, hh, hused, tret, yp negated -- for linear
dense (A -> -A), heat (coef -> -coef), its hand-written callback twin and mass-action networks (every rate constant negated), with and
without roots, with analytic and DQ Jacobians (dq_inc takes the sign of hh * yp_j, which a mirror keeps). Those are all the kinds that
can be mirrored through their parameters; Roberts, Lorenz63 and the Brusselator have constants in the kernel and no mirror, so none
is asserted for them. NOT exact: a Krylov ctx. SPGMR's difference quotient J v = (F(y + sigma z) - F(y)) / sigma perturbs y by
+sigma z in both runs while the mirror negates z (the right-hand side -F is negated), so a forward difference becomes a backward one:
equal in exact arithmetic for a linear F, not to the bit. test_krylov_has_no_exact_mirror holds that down, and no mirror assertion is
made for a Krylov ctx on the device."""
import numpy as np
import pytest

import backward_cases as BC
import tstop_oracle as T

PLAIN = list(BC.CASES)
ROOTS = ["lorenz", "roberts", "linear24", "heat20"]
DQ_CASES = [("lorenz", "dense"), ("linear24", "dense"), ("heat20", "dense"), ("heat20", (1, 1)), ("chain12", "dense")]


def steps_of(c, ops, how=None):
    """Per system the accepted steps [nsteps][5] (tn, hused, kused, nni, nsetups) of the reference's run."""
    sy = BC.reference_systems(c, ops, how)
    return [np.array(s.steps, dtype=np.float64).reshape(-1, 5) if hasattr(s, "steps") else s.recorded_steps() for s in sy]


def not_trivial(c, ops, how=None, ends_at_tout=True):
    rec = BC.reference(c, ops, how)
    steps = steps_of(c, ops, how)
    last = rec[-1]
    assert (last["nst"] >= 20).all(), (c["name"], last["nst"])
    assert max(s[:, 2].max() for s in steps) >= 3, c["name"]
    assert (last["hh"] < 0.0).all() and all((s[:, 1] < 0.0).all() for s in steps), c["name"]
    assert 4 * int((last["status"] == T.SUCCESS).sum()) >= 3 * last["status"].size, (c["name"], last["status"])
    assert not ends_at_tout or (last["tret"][last["status"] == T.SUCCESS] == c["touts"][-1]).all()
    return rec


@pytest.mark.parametrize("name", PLAIN)
def test_plain_backward_runs_are_not_trivial(name):
    c = BC.case(name)
    assert all(t < 0.0 for t in c["touts"]) and c["touts"] == sorted(c["touts"], reverse=True)
    not_trivial(c, BC.plain_ops(c), {} if c["ref"] == "python" else None)


ROOT_VARIANTS = [(n, v) for n in ROOTS for v in ("roots", "root_at_tout", "roots_tstop")]


@pytest.mark.parametrize("name,variant", ROOT_VARIANTS)
def test_root_returns_while_going_backward(name, variant):
    c = BC.case(name, variant)
    ops = BC.ops_on_harness(c)
    rec = not_trivial(c, ops)
    found = [(r["status"] == T.ROOT_RETURN) & (r["hh"] < 0.0) for r in rec]
    assert sum(int(f.sum()) for f in found) >= 1, c["name"]
    assert any(r["iroots"][f].any() for r, f in zip(rec, found))
    assert rec[-1]["nge"].min() > 0
    if variant == "root_at_tout":  # system 0's first function is zero at the first tout, to the bit
        assert any(r["status"][0] == T.ROOT_RETURN and r["tret"][0] == c["touts"][0] and r["iroots"][0][0] != 0 for r in rec), c["name"]
    if variant == "roots_tstop":
        assert any((r["status"] == T.TSTOP_RETURN).any() for r in rec)


def test_masked_norms_with_roots_while_going_backward():
    c = BC.case("linear24", "masked")
    rec = not_trivial(c, BC.ops_on_harness(c))
    plain = BC.case("linear24", "roots")
    assert not np.array_equal(rec[-1]["nst"], BC.reference(plain, BC.ops_on_harness(plain))[-1]["nst"])  # the mask changes the steps


@pytest.mark.parametrize("name", ["roberts", "linear24", "heat20"])
def test_stop_times_behind_t0(name):
    """tests/tstop_cases.py's "residues" script with a negative first tout: by b % 7 none, inside the first call, tiny, the first
    tout itself, between the touts, far behind the last, and on the wrong side (ILL_INPUT before the first step)."""
    c = BC.case(name, "tstop")
    ops = BC.ops_on_harness(c)
    rec = not_trivial(c, ops)
    B = rec[0]["status"].size
    hit = 0
    hs = BC.reference_systems(c, ops)
    cur, k = np.full(B, np.nan), 0
    for op in ops:
        if op[0] == "stop":
            cur = np.full(B, np.nan) if op[1] is None else np.broadcast_to(op[1], (B,)).copy()
            continue
        r, k = rec[k], k + 1
        m = r["status"] == T.TSTOP_RETURN
        hit += int(m.sum())
        assert (r["tret"][m] == cur[m]).all() and (r["tret"][m] < 0.0).all(), (name, r["tret"], cur)  # tret == tstop exactly
    assert hit >= min(B, 7) - 3
    assert (rec[0]["status"][np.arange(B) % 7 == 6] == T.ILL_INPUT).all() and (rec[0]["nst"][np.arange(B) % 7 == 6] == 0).all()
    seen = set().union(*(h.census() for h in hs))
    assert {"first_clip", "tstop_stop_test2_normal"} <= seen, seen
    assert B < 7 or "first_ill_input" in seen, seen  # heat20 has three systems: the wrong side is Roberts' and linear24's
    assert seen & {"clip_stop_test1", "clip_stop_test2"}, seen


def test_stop_times_between_calls_in_both_tasks():
    c = BC.case("linear24", "entry")
    ops = BC.ops_on_harness(c)  # the script asserts its own TSTOP / SUCCESS sequence
    not_trivial(c, ops, ends_at_tout=False)  # (its last calls are IDA_ONE_STEP: tret = tn)
    hs = BC.reference_systems(c, ops)
    seen = set().union(*(h.census() for h in hs))
    assert {"clip_stop_test1", "tstop_stop_test1_normal", "tstop_stop_test1_one_step", "tstop_stop_test2_one_step"} <= seen, seen
    assert all(h.get("hh") < 0.0 for h in hs)


@pytest.mark.parametrize("name,dq", DQ_CASES, ids=str)
def test_dq_runs_see_both_signs_of_hh_yp(name, dq):
    c = BC.case(name)
    how = {"dq": dq}
    not_trivial(c, BC.plain_ops(c), how)
    evals = [e for s in BC.reference_systems(c, BC.plain_ops(c), how) for e in s.dq_signs]
    both = [bool((e < 0).any() and (e > 0).any()) for e in evals]  # within ONE Jacobian evaluation
    assert any(both), c["name"]
    print(c["name"], dq, "%d of %d Jacobian evaluations see both signs of hh * yp_j" % (sum(both), len(both)))
    rec = BC.reference(c, BC.plain_ops(c), how)
    assert (rec[-1]["nre_dq"] > 0).all()


@pytest.mark.parametrize("krylov", ["plain", (1, 1)], ids=str)
def test_krylov_heat_backward(krylov):
    c = BC.case("heat20")
    rec = not_trivial(c, BC.plain_ops(c), {"krylov": krylov})
    assert (rec[-1]["nli"] > 0).all()
    if krylov != "plain":
        assert (rec[-1]["npe"] > 0).all() and (rec[-1]["nps"] > 0).all()


def test_a_constraint_becomes_active_going_backward():
    c = BC.case("heat20")
    how = BC.constraint_how()
    not_trivial(c, BC.plain_ops(c), how)
    census = [s.census for s in BC.reference_systems(c, BC.plain_ops(c), how)]
    assert sum(k["corrected"] + k["recovered"] for k in census) >= 1, census
    free = BC.reference(c, BC.plain_ops(c), {})
    assert not np.array_equal(free[-1]["yy"], BC.reference(c, BC.plain_ops(c), how)[-1]["yy"])


def test_a_constraint_stops_lorenz_going_backward():
    """The one case the census exempts from "three quarters end with SUCCESS": the constraint y1 >= 0 contradicts the backward
    solution, so the run cannot get past it and every call ends with TOO_MUCH_WORK -- which is what it is there to show on the
    one-thread device stepper (the required constrained run that finishes is heat20's, above). The other conditions hold."""
    c, how = BC.lorenz_constraint_case()
    rec = BC.reference(c, BC.plain_ops(c), how)
    assert max(np.array(s.steps)[:, 2].max() for s in BC.reference_systems(c, BC.plain_ops(c), how)) >= 3
    census = [s.census for s in BC.reference_systems(c, BC.plain_ops(c), how)]
    assert sum(k["corrected"] for k in census) >= 1 and sum(k["recovered"] for k in census) >= 1, census
    assert (rec[-1]["nst"] >= 20).all() and (rec[-1]["hh"] < 0.0).all() and (rec[-1]["tn"] < 0.0).all()
    assert set(rec[-1]["status"].tolist()) <= {T.TOO_MUCH_WORK, -11, 0}, rec[-1]["status"]  # (-11: IDAENS_CONSTR_FAIL)
    assert (rec[-1]["yy"][:, 1] > -1.0e-6).all()  # held at zero within the tolerances; unconstrained it is -0.5 at t = -0.05


# ------------------------------------------------------------------------------------------------ the mirror property
def test_mirror_is_an_involution():
    for name in BC.MIRROR_EXACT:
        p = BC.forward_problem(name)
        q = BC.mirror(BC.mirror(p))
        for k in ("yy0", "yp0", "params", "A", "B", "c"):
            assert k not in p or np.array_equal(np.asarray(p[k]).view(np.uint64), np.asarray(q[k]).view(np.uint64)), (name, k)


@pytest.mark.parametrize("name", BC.MIRROR_EXACT)
def test_mirror_property_on_the_reference(name):
    bwd, fwd = BC.case(name), BC.forward_case(name)
    how = {} if bwd["ref"] == "python" else None
    BC.mirrored(BC.reference(fwd, BC.plain_ops(fwd), how), BC.reference(bwd, BC.plain_ops(bwd), how), what=name)


@pytest.mark.parametrize("name", ["linear24", "heat20"])
def test_mirror_property_with_roots(name):
    bwd = BC.case(name, "roots")
    fwd = dict(bwd, name=bwd["name"] + "/forward", prob=BC.forward_problem(name), touts=[-t for t in bwd["touts"]])
    ops_b = BC.ops_on_harness(bwd)
    ops_f = [(o[0], -o[1], o[2]) for o in ops_b]
    BC.mirrored(BC.reference(fwd, ops_f), BC.reference(bwd, ops_b), what=name)


@pytest.mark.parametrize("name,how", [("heat20", {"dq": "dense"}), ("heat20", {"dq": (1, 1)}), ("linear24", {"dq": "dense"}),
                                      ("chain12", {"dq": "dense"})], ids=str)
def test_mirror_property_with_dq(name, how):
    bwd, fwd = BC.case(name), BC.forward_case(name)
    BC.mirrored(BC.reference(fwd, BC.plain_ops(fwd), how), BC.reference(bwd, BC.plain_ops(bwd), how), what="%s %s" % (name, how))


def test_krylov_has_no_exact_mirror():
    bwd, fwd = BC.case("heat20"), BC.forward_case("heat20")
    how = {"krylov": "plain"}
    f, b = BC.reference(fwd, BC.plain_ops(fwd), how)[-1], BC.reference(bwd, BC.plain_ops(bwd), how)[-1]
    assert not np.array_equal(f["yy"], b["yy"])
    assert np.abs(f["yy"] - b["yy"]).max() < 1e-4 * np.abs(f["yy"]).max()  # the same solution within the tolerances all the same


CALCIC = ["roberts_satol", "linear40_mixed", "linear40_yinit", "linear9_dq", "heat16_band", "heat16_band_dq", "linear40_singular", "bruss32_mixed"]


@pytest.mark.parametrize("name", CALCIC)
def test_calc_ic_references_with_tout1_behind_t0(name):
    """tests/calcic_cases.py's cases with tout1 negated: every system's hic (and with it cj) is negative, at least three quarters
    succeed, and the corrected values are not the forward ones wherever cj enters (YA_YDP_INIT). The two cases of the mixed-fates
    table keep their mixed fates: linear40_singular one NO_RECOVERY after retries at hic / 10, bruss32_mixed (Y_INIT) successes,
    backtracking, CONV_FAIL and LINESEARCH_FAIL side by side."""
    import calcic_cases as CK
    import calcic_ref as IC
    c, r, f = CK.case(name), BC.calcic_reference(name), CK.reference(name)
    assert c["n"] <= 64
    ok = r["status"] == 0
    assert (r["hic"][ok] < 0.0).all() and (r["counters"]["nni"][ok] > 0).any()
    if name == "bruss32_mixed":
        assert {0, IC.CONV_FAIL, IC.LINESEARCH_FAIL} <= set(r["status"].tolist()) and (r["counters"]["nbacktr"] > 0).any()
    else:
        assert 4 * int(ok.sum()) >= 3 * ok.size, r["status"]
    if name == "linear40_singular":
        assert r["status"].tolist().count(IC.NO_RECOVERY) == 1 and (r["counters"]["ncfn"] > 0).any()
    if c["icopt"] == IC.YA_YDP_INIT and name != "roberts_satol":
        assert not np.array_equal(r["yp"], f["yp"])


def test_get_dky_of_a_harness_after_backward_steps():
    c = BC.case("linear24")
    h = BC.reference_systems(c, BC.plain_ops(c))[0]
    tn, hused, kused = h.get("tn"), h.get("hused"), int(h.get("kused"))
    assert hused < 0.0 and kused >= 3
    assert BC.harness_get_dky(h, tn - 0.5 * hused, 0)[0] == 0 and BC.harness_get_dky(h, tn + 0.5 * hused, 1)[0] == 0
    assert BC.harness_get_dky(h, tn - 3.0 * hused, 0)[0] == -26 and BC.harness_get_dky(h, tn, kused + 1)[0] == -25
    st, d0 = BC.harness_get_dky(h, c["touts"][-1], 0)
    assert st == 0 and np.array_equal(d0, h.getv("yy"))  # k = 0 at tret is the solution returned there
