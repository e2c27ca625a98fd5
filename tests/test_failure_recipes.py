"""Every recipe of tests/failure_recipes.py that tests/test_gpu_failure_paths.py uses, at every size it uses it at, takes the path it
is named for -- asserted on the CPU oracle alone. These are the conditions that keep the GPU tests from passing vacuously (a jump that
no longer makes a step fail would leave them comparing ordinary integrations); they are not tolerances. A recipe that misses its
condition at some size is to be changed, not the condition."""
import numpy as np
import pytest

import failure_recipes as F


def holds(case, systems=None):
    rows = F.census(case, systems)
    ok, what = F.meets(case["expect"], rows)
    assert ok, "%s: expected %s, the oracle did %s" % (case["name"], what, rows)
    return rows


@pytest.mark.parametrize("name,n", F.GPU_JUMPS + [("c*1.0001", 24), ("c*1.0001", 200)])
def test_jump_recipes_fail_the_next_step_as_often_as_they_are_named_for(name, n):
    """deep: >= 3 error-test failures inside one step (the third and later ones force order 1: the lowest order after the jump is 1)
    and status 0 with steps taken after the jump; second: >= 2; terminal: -3 with exactly 10; mixed: both in one batch."""
    case = F.jump_case(name, n)
    rows = holds(case)
    if case["expect"] in ("deep", "second"):
        assert all(r["nst"] > r["nst_jump"] and r["status"] == 0 for r in rows)
    # the untouched neighbours run their ordinary integration: at most a single failed error test (n = 704 has one), no second one
    quiet = F.census(case, [s for s in range(case["prob"]["yy0"].shape[0]) if s not in case["edited"]][:1])
    assert all(r["status"] == 0 and r["max_etf"] <= 1 and r["ncfn"] == 0 for r in quiet), quiet


def test_the_long_recovery_takes_many_steps_and_failures():
    name, n = F.LONG_JUMP
    rows = holds(F.jump_case(name, n, after=(0.4, 0.5, 1.0), mxstep=100000))
    assert all(r["nst"] - r["nst_jump"] > 1000 and r["netf"] >= 50 for r in rows), rows


@pytest.mark.parametrize("n", [24, 200])
def test_a_jump_after_thirty_rounds_fails_the_next_step_too(n):
    """The jump the GPU tests make inside a round-limited schedule (after thirty lock-step rounds, t about 0.05): deep recovery there
    as well, and the run in NORMAL mode that the GPU test compares with counts the same."""
    case = F.jump_case("c*1.01", n)
    rows = F.jump_after_attempts(case, case["prob"]["touts"], 30, one_step=True)
    ok, what = F.meets("deep", rows)
    assert ok, (what, rows)
    ref = F.jump_after_attempts(case, case["prob"]["touts"], 30)
    for r in rows:
        assert ref["counters"]["nst"][r["sys"]] == r["nst"] and ref["counters"]["netf"][r["sys"]] == r["netf"]


@pytest.mark.parametrize("n", F.REPEATED_SIZES)
def test_the_repeated_jump_restarts_newton_with_a_stale_jacobian_more_than_once(n):
    """The condition of tests/test_gpu_newton_restarts.py: every edited system takes Newton's restart (ConvergenceRecover with a stale
    Jacobian: nls_nconvfails counts it, ncfn does not) at least twice, and every system ends with status 0. The oracle gives 5 / 3 / 4
    restarts at n = 24 and 5 / 4 / 4 at n = 200, no ncfn, in about 190 to 200 steps."""
    case = F.repeated_jump_case(n)
    ref = F.oracle_reference(case)
    c, ed = ref["counters"], case["edited"]
    restarts = c["nls_nconvfails"] - c["ncfn"]
    print("restarts", restarts, "ncfn", c["ncfn"], "nst", c["nst"])
    assert (ref["status"] == 0).all(), ref["status"]
    assert (restarts[ed] >= 2).all(), restarts


@pytest.mark.parametrize("kind,n,tout,expect", F.GPU_FIRST_STEPS + [("heat1d", n, 1.0, "recover") for n, _ in F.BAND_FIRST_STEPS[:1]])
def test_first_step_recipes_fail_before_the_first_step(kind, n, tout, expect):
    """recover: failures at nst == 0 and the integration goes on to tout; first_terminal: -3 with ten error-test failures at nst == 0."""
    case = F.first_step_case(kind, n, tout, expect=expect)
    rows = holds(case, case["edited"][:3])
    assert all(r["nfail_first"] > 0 for r in rows)
    B = case["prob"]["yy0"].shape[0]
    assert 0 < len(case["edited"]) < B, "a batch keeps untouched systems next to the failing ones"


def test_lorenz_first_step_recipe_meets_newton_failures_too():
    """With the first tout at 1e4 the attempts before the first step also fail in Newton's iteration (quirks Q3/Q4: recoverable with a
    current Jacobian), and after recovering from tout = 1 a later step fails its error test several times."""
    rows = F.census(F.first_step_case("lorenz63", 3, 1.0e4, expect="first_terminal"), [0, 1])
    assert all(r["max_cf"] > 0 and r["nfail_first"] == r["netf"] + r["ncfn"] for r in rows), rows
    rows = F.census(F.first_step_case("lorenz63", 3, 1.0), [0, 1])
    assert all(r["netf"] > r["nfail_first"] for r in rows), rows


@pytest.mark.parametrize("n,when", [(n, w) for n in F.SINGULAR_SIZES for w in ("start", "mid")])
def test_zero_column_fails_every_setup_of_the_step(n, when):
    rows = holds(F.singular_case(n, when))
    assert all(r["status"] == -4 for r in rows), rows
    if when == "start":
        assert all(r["nfail_first"] == 10 for r in rows)


@pytest.mark.parametrize("when", ["start", "mid"])
def test_zero_column_in_a_banded_problem(when):
    n, ml, mu = F.SINGULAR_BAND
    case = F.singular_case(n, when, band=(ml, mu))
    holds(case)
    p = case["prob"]
    assert p["A"][1, 5].any() and p["B"][1, 5].any(), "the column the edit zeroes is not zero to begin with"


@pytest.mark.parametrize("kind", ["linear_dense", "lorenz63"])
def test_tolerances_below_roundoff_are_refused_at_the_first_step(kind):
    case = F.too_much_acc_case(kind)
    holds(case, case["edited"][:4])


@pytest.mark.parametrize("which", ["jump", "first", "first_terminal", "singular"])
def test_the_reference_run_in_normal_mode_agrees_with_the_census(which):
    """oracle_reference (what the GPU tests compare with: NORMAL mode, every system, fatal returns kept) against census (ONE_STEP):
    same final status, step and failure counts and failures at nst == 0; a system that failed keeps its return at the later touts."""
    case = {"jump": lambda: F.jump_case("B*1.5", 24), "first": lambda: F.first_step_case("heat1d", 40, 1.0e2, later=(150.0,)),
            "first_terminal": lambda: F.first_step_case("lorenz63", 3, 1.0e4, batch=8, expect="first_terminal"),
            "singular": lambda: F.singular_case(200, "mid")}[which]()
    ref = F.oracle_reference(case, nthreads=4)
    B = case["prob"]["yy0"].shape[0]
    for r in F.census(case):
        s = r["sys"]
        assert ref["status"][-1][s] == r["status"] and ref["nfail_first"][s] == r["nfail_first"]
        for k in ("nst", "netf", "ncfn"):
            assert ref["counters"][k][s] == r[k], (k, s)
    for s in range(B):
        failed = np.flatnonzero((ref["status"][:, s] < 0) & (ref["status"][:, s] != -1))
        if failed.size:
            i = failed[0]
            assert (ref["status"][i:, s] == ref["status"][i, s]).all() and (ref["tret"][i:, s] == ref["tret"][i, s]).all()
            assert (ref["yy"][i:, s] == ref["yy"][i, s]).all()
        if s not in case["edited"]:
            assert ref["nfail_first"][s] == 0 and (ref["status"][:, s] == 0).all() or which == "first_terminal"


def test_the_editor_changes_the_oracle_problem_as_set_linear_dense_would():
    """apply_to_oracle edits, in place, the arrays the oracle reads: the named field only, with the values the product is given
    (factor * array), and the oracle's next step sees the change."""
    case = F.jump_case("c*1.01", 24)
    p = case["prob"]
    a = F.oracle_of(p, 0)
    for t in case["before"]:
        assert a.solve(t)[0] == 0
    A0, c0 = a._keep[4].copy(), a._keep[6].copy()
    F.apply_to_oracle(a, case["edit"])
    assert np.array_equal(a._keep[4], A0) and np.array_equal(a._keep[6], 1.01 * c0)
    q = dict(p, c=p["c"].copy())
    F.edit_arrays(case["edit"], q["A"][0].copy(), q["B"][0].copy(), q["c"][0])
    assert np.array_equal(q["c"][0], a._keep[6]) and np.array_equal(q["c"][1], p["c"][1])
    sa, ta = a.solve(0.4)
    assert sa == 0 and a.get("netf") >= 3
