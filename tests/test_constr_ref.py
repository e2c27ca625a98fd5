"""tests/constr_ref.py on the CPU: (1) with an all-zero constraint vector its restated Ida::solve equals the oracle's own, bit for
bit, over the standard schedules; (2) the census -- the cases tests/test_gpu_constraints.py runs (tests/constr_cases.py) reach every
branch of DESIGN.md section 4g on each stepper's list; (3) the host-side checks of the new entry points that need no device."""
import ctypes as C

import numpy as np
import pytest

import constr_cases as K
import constr_ref as CR
import oracle_lib as O


def _oracle_run(prob, touts, ids):
    """OracleIda.solve over the schedule with the oracle's own step recording -> the fields of constr_ref.run."""
    out = {"status": [], "tret": [], "yy": [], "yp": [], "steps": [], "counters": [], "scal": []}
    sy = []
    for s in ids:
        data = {k: prob[k][s] for k in ("params", "A", "B", "c") if prob.get(k) is not None}
        o = O.OracleIda(prob["kind"], prob["n"], prob["yy0"][s], prob["yp0"][s], prob["rtol"], prob["atol"], **data)
        o.L.oracle_ida_record_steps(o.h, 1)
        sy.append(o)
    for t in touts:
        r = []
        for o in sy:  # the oracle's Roberts has the reference's two root functions: a root return is reported and the call repeated,
            x = o.solve(float(t))  # as oracle_run_ensemble does (the steps are the same with or without them)
            while x[0] == 2:
                x = o.solve(float(t))
            r.append(x)
        out["status"].append([x[0] for x in r])
        out["tret"].append([x[1] for x in r])
        out["yy"].append([o.getv("yy") for o in sy])
        out["yp"].append([o.getv("yp") for o in sy])
    out["steps"] = [o.recorded_steps() for o in sy]
    out["counters"] = [o.counters() for o in sy]
    out["scal"] = [[o.get(k) for k in ("kused", "hused", "hh", "tn", "kk", "tretlast", "cj", "ss")] for o in sy]
    out["vec"] = [np.concatenate([o.getv(k) for k in ("phi", "psi", "ee", "ewt")]) for o in sy]
    return out


def _pinning_problems():
    from idahip import problems
    rob = problems.roberts()
    return [("roberts", rob, rob["touts"], [0]),
            ("lorenz63", problems.lorenz63(batch=2), problems.lorenz63(batch=2)["touts"][:20], [0, 1]),
            ("linear_dense", problems.linear_dense(n=24, batch=2), problems.linear_dense(n=24, batch=2)["touts"], [0, 1]),
            ("heat1d", problems.heat1d(n=40, batch=2), problems.heat1d(n=40, batch=2)["touts"], [0, 1])]


@pytest.mark.parametrize("which", range(4), ids=["roberts", "lorenz63", "linear_dense_24", "heat1d_40"])
def test_reference_loop_with_zero_constraints_is_the_oracles_solve(which):
    """Statuses, tret, yy / yp after every call, every counter, the recorded steps and the state the next step starts from: np.array_equal
    on the bits (no NaN occurs)."""
    name, prob, touts, ids = _pinning_problems()[which]
    want = _oracle_run(prob, touts, ids)
    for constr in (np.zeros(prob["n"]), None):
        got = CR.run(prob, constr, touts, ids=ids)
        sy = CR.systems(prob, constr, ids=ids)  # (a second set, to read the scalars and vectors run() does not return)
        for t in touts:
            for s in sy:
                s.solve(t)
        assert np.array_equal(got["status"], np.array(want["status"])) and (got["status"] == 0).all()
        assert np.array_equal(got["tret"], np.array(want["tret"]))
        assert np.array_equal(got["yy"].view(np.uint64), np.array(want["yy"]).view(np.uint64))
        assert np.array_equal(got["yp"].view(np.uint64), np.array(want["yp"]).view(np.uint64))
        for b in range(len(ids)):
            for k in CR.CNT:
                assert got["counters"][k][b] == want["counters"][b][k], (k, b)
            assert np.array_equal(got["steps"][b], want["steps"][b]) and len(got["steps"][b]) == want["counters"][b]["nst"]
            assert [sy[b].o.get(k) for k in ("kused", "hused", "hh", "tn", "kk", "tretlast", "cj", "ss")] == want["scal"][b]
            mine = np.concatenate([sy[b].o.getv(k) for k in ("phi", "psi", "ee", "ewt")])
            assert np.array_equal(mine.view(np.uint64), want["vec"][b].view(np.uint64))
            assert got["census"][b]["passed"] == (want["counters"][b]["n_attempts"] - want["counters"][b]["ncfn"] if constr is not None else 0)


@pytest.mark.parametrize("cases", [K.HOST_CASES, K.TINY_CASES], ids=["host_stepper", "one_thread_stepper"])
def test_census_every_branch_is_reached_on_each_steppers_case_list(cases):
    total = dict.fromkeys(CR.CENSUS, 0)
    finished_after_a_correction = 0
    for name in cases:
        case, ref = K.reference(name)
        tot = CR.census_total(ref)
        print(name, "status", ref["status"][-1], "tret", ref["tret"][-1], tot)
        for k in total:
            total[k] += tot[k]
        finished_after_a_correction += sum(1 for b, c in enumerate(ref["census"]) if ref["status"][-1][b] == 0 and c["corrected"] >= 1)
        # CONSTR_FAIL is reported exactly where the tenth failure was a constraint failure, ILL_INPUT exactly where the start check fired
        for b, c in enumerate(ref["census"]):
            assert (ref["status"][-1][b] == CR.CONSTR_FAIL) == (c["constr_fail"] == 1)
            assert (c["start_ill"] > 0) == (ref["status"][-1][b] == CR.ILL_INPUT and ref["counters"]["n_attempts"][b] == 0)
    assert all(total[k] > 0 for k in total), total
    assert finished_after_a_correction >= 1


def test_the_named_cases_take_the_paths_they_are_named_for():
    _, r = K.reference("roberts_loose")
    assert (r["status"][-1] == 0).all() and all(c["corrected"] >= 1 for c in r["census"])
    _, r = K.reference("roberts_inconsistent")  # the ten failures are mixed: constraint and convergence failures share ncf
    assert (r["status"] == CR.CONSTR_FAIL).all() and (r["tret"] == 0.0).all() and (r["counters"]["ncfn"] == 10).all()
    assert all(0 < c["recovered"] < 10 for c in r["census"]) and (r["nfail_first"] == 10).all()
    _, r = K.reference("lorenz_x_nonneg")
    assert (r["status"] == CR.TOO_MUCH_WORK).all() and all(c["corrected"] > 100 and c["recovered"] > 50 for c in r["census"])
    _, r = K.reference("lorenz_start_violated")
    assert (r["status"] == CR.ILL_INPUT).all() and (r["counters"]["n_attempts"] == 0).all()
    _, r = K.reference("heat_nonneg")
    assert (r["status"] == 0).all() and all(c["corrected"] >= 1 for c in r["census"])
    _, r = K.reference("heat_positive")
    assert (r["status"] == CR.ILL_INPUT).all()
    for name in ("linear_negated_24", "linear_negated_200"):
        _, r = K.reference(name)
        assert r["status"][-1][0] == CR.CONSTR_FAIL and r["census"][0]["recovered"] == 10 and r["tret"][-1][0] == 0.0
    for name in ("linear_monotone_24", "linear_monotone_200"):
        _, r = K.reference(name)
        assert sum(c["corrected"] for c in r["census"]) > 100 and sum(c["recovered"] for c in r["census"]) > 30


def test_kernel_restatement_branches():
    """post_newton_constr's three outcomes on a hand-made state, and check = 0 / no violation == stepper_ref.post_newton."""
    import stepper_ref as R
    n = 4
    phi = np.zeros((6, n))
    phi[0] = [1.0, 1.0, 1.0, 1.0]
    ewt = np.full(n, 10.0)
    yyp, ypp = phi[0].copy(), np.zeros(n)
    c = np.array([1.0, 2.0, 0.0, -1.0])
    ee = np.array([-1.0 - 1e-3, 0.0, 0.0, -2.0])  # yy = (-1e-3, 1, 1, -1): component 0 violated, slightly
    yy, yp, e2, nrm, flag, rr = CR.post_newton_constr(yyp, ypp, ee, ewt, phi, 2.0, 1, c, 0.33, 1)
    assert flag == 1 and rr == 0.0 and e2[0] == ee[0] - yy[0] and np.array_equal(e2[1:], ee[1:]) and yy[0] == yyp[0] + ee[0]
    assert nrm[0] == O.wrms(e2, ewt)
    yy, yp, e2, nrm, flag, rr = CR.post_newton_constr(yyp, ypp, ee, ewt, phi, 2.0, 1, c, 1e-6, 1)
    q = phi[0][0] / (phi[0][0] - yy[0])
    assert flag == 2 and rr == max(0.9 * q, 0.1) and np.array_equal(e2, ee) and not nrm.any()
    for chk, cc in ((0, c), (1, np.zeros(n))):
        yy, yp, e2, nrm, flag, rr = CR.post_newton_constr(yyp, ypp, ee, ewt, phi, 2.0, 1, cc, 1e-6, chk)
        y0, yp0, n0 = R.post_newton(yyp, ypp, ee, ewt, phi, 2.0, 1)
        assert flag == 0 and rr == 0.0 and np.array_equal(e2, ee) and np.array_equal(nrm, n0) and np.array_equal(yy, y0)
    # strict constraints: zero is violated, and the correction moves it inside by 0.1 / ewt
    m = CR.violated(np.array([2.0, -2.0, 1.0, -1.0]), np.zeros(4))
    assert m.tolist() == [True, True, False, False]
    v = CR.correction(np.array([2.0, -2.0]), np.zeros(2), np.array([10.0, 10.0]), np.array([True, True]))
    assert v.tolist() == [-0.1 * (2.0 / 10.0), -0.1 * (-2.0 / 10.0)]
    assert not CR.violated(np.array([2.0, 1.0]), np.array([np.nan, np.nan])).any()


def test_host_side_of_the_new_entry_points():
    """idahip_set_constraints(NULL ctx) returns -1 without touching a device; the getter likewise."""
    import idahip
    H, _ = idahip.load()
    c = np.ones(3)
    assert H.idahip_set_constraints(None, c.ctypes.data_as(C.POINTER(C.c_double))) == -1
    assert H.idahip_constraints(None, None) == -1
    for sym in ("idahip_set_constraints", "idahip_constraints", "idahip_post_newton_constr", "idahip_constr_check"):
        assert sym in idahip.HIP_SYMBOLS and hasattr(H, sym)
