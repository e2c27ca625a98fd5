"""tests/krylov_ref.py on the CPU: (a) with the direct-solve switch its restated Newton solve and stepper loop equal the oracle's own,
bit for bit; (b) the SPGMR restatement is pinned on something independent -- the true scaled residual of its solutions with the
analytic Jacobian; (c) the census: the case list of tests/krylov_cases.py makes the reference take every branch of DESIGN.md
section 4h (QRSOL_FAIL excepted); and the reference runs of the stepper cases contain linear failures that the stepper recovers from."""
import numpy as np
import pytest

import krylov_cases as K
import krylov_ref as KR
import oracle_lib as O
import stepper_ref as R


@pytest.mark.parametrize("kind,n", [("linear_dense", 12), ("heat1d", 16)], ids=["linear_dense_12", "heat1d_16"])
def test_direct_switch_reproduces_the_oracle_bit_for_bit(kind, n):
    from idahip import problems
    p = problems.linear_dense(n=n, batch=2) if kind == "linear_dense" else problems.heat1d(n=n, batch=2)
    touts = p["touts"][:5]
    got = KR.run(p, touts, direct=True)
    oracles = []
    for s in range(2):
        data = {k: p[k][s] for k in ("params", "A", "B", "c") if p.get(k) is not None}
        o = O.OracleIda(p["kind"], n, p["yy0"][s], p["yp0"][s], p["rtol"], p["atol"], **data)
        o.L.oracle_ida_record_steps(o.h, 1)
        oracles.append(o)
    for i, t in enumerate(touts):
        for s, o in enumerate(oracles):
            st, tret = o.solve(float(t))
            assert (st, tret) == (got["status"][i, s], got["tret"][i, s]) and st == 0
            assert np.array_equal(got["yy"][i, s].view(np.uint64), o.getv("yy").view(np.uint64))
            assert np.array_equal(got["yp"][i, s].view(np.uint64), o.getv("yp").view(np.uint64))
            c = o.counters()
            for k in KR.CR.CNT:
                assert got["counters"][k][i, s] == c[k], (k, i, s)
            assert got["kused"][i, s] == int(o.get("kused")) and got["hused"][i, s] == o.get("hused") and got["tn"][i, s] == o.get("tn")
    for s, o in enumerate(oracles):
        assert np.array_equal(got["steps"][s], o.recorded_steps()) and len(got["steps"][s]) > 10  # steps and orders
        mine = got["systems"][s].o
        for k in ("phi", "psi", "ee", "ewt"):
            assert np.array_equal(mine.getv(k).view(np.uint64), o.getv(k).view(np.uint64)), k
        assert [mine.get(k) for k in ("kk", "hh", "cj", "ss", "cjold", "jcur")] == [o.get(k) for k in ("kk", "hh", "cj", "ss", "cjold", "jcur")]
        assert got["counters"]["nli"][-1, s] == 0 and got["counters"]["ncfl"][-1, s] == 0


def test_solver_is_pinned_on_the_true_residual_with_the_analytic_jacobian():
    """Linear dense problems: the residual is linear, so the DQ J v is (B + cj A) v up to rounding. With maxl = n (n = 9, 12; four
    systems, cj = 10 and 1000, eps_newt = 0.33, 1e-3, 1e-6: 48 solves) every solve ends with flag 0, and the true scaled residual
    ||w o (b - J x)||_2 with J = B + cj A formed in numpy is compared with the solver's own rho and with tol.
    Measured here: true / tol between 9.5e-6 and 0.99999 (largest: n = 12, system 1, cj = 1000, eps_newt = 0.33, where rho / tol is
    0.99999 too); true / rho is 1 +- 3e-4 wherever rho is not far below tol (below 1e-6 tol the DQ's rounding is all that is left
    and true / rho grows to 1e8, with true / tol <= 0.08). The assertion is a factor 2 over the largest measured ratio, which covers
    the DQ's rounding: true <= 2.0 tol."""
    from idahip import problems
    worst = 0.0
    for n in (9, 12):
        p = problems.linear_dense(n=n, batch=4)
        for s in range(4):
            for cj in (10.0, 1000.0):
                for eps in (0.33, 1e-3, 1e-6):
                    rng = np.random.Generator(np.random.PCG64(100 * n + s))
                    yy = p["yy0"][s] + 1e-3 * rng.uniform(-1, 1, n)
                    yp = p["yp0"][s] + 1e-3 * rng.uniform(-1, 1, n)
                    w = R.ewt_set(yy, p["rtol"], p["atol"])
                    res = KR.make_res(p, s)
                    rr = res(0.1, yy, yp)
                    b = rng.uniform(-1, 1, n) / w
                    tol = KR.eplin(n, eps)
                    r = KR.spgmr_solve(res, b, w, yy, yp, rr, 0.1, cj, tol, n)
                    J = (p["B"][s] + cj * p["A"][s]).T  # logical (row, column)
                    true = float(np.linalg.norm(w * (b - J @ r["x"])))
                    print(n, s, cj, eps, "nli", r["nli"], "rho/tol", r["res_norm"] / tol, "true/tol", true / tol)
                    assert r["flag"] == KR.SUCCESS and r["res_norm"] <= tol
                    assert true <= 2.0 * tol, (n, s, cj, eps, true / tol)
                    if eps >= 1e-3 and r["res_norm"] > 1e-3 * tol:  # the solver's own estimate is the true residual where rounding does not dominate
                        assert abs(true / r["res_norm"] - 1.0) < 1e-2
                    worst = max(worst, true / tol)
    print("largest true / tol", worst)


def test_kdot_order_and_values():
    rng = np.random.Generator(np.random.PCG64(5))
    for n in (1, 9, 63, 64, 65, 257, 300):
        x, y = rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 8, n), rng.standard_normal(n)
        p = x * y
        part = [0.0] * 64
        for i in range(n):  # element by element, the definition as written
            part[i % 64] = part[i % 64] + p[i]
        r = 0.0
        for q in range(64):
            r = r + part[q]
        assert KR.kdot(x, y) == r
        assert abs(KR.kdot(x, y) - float(np.dot(x, y))) <= 1e-12 * float(np.dot(np.abs(x), np.abs(y)))
    assert KR.kdot(np.array([-0.0]), np.array([1.0])) == 0.0 and np.signbit(KR.kdot(np.array([-0.0]), np.array([1.0]))) == False  # noqa: E712


def test_census_every_branch_is_taken_on_the_case_list():
    total = KR.new_census()
    for case in K.solve_cases():
        _, out, census = K.solve_reference(*case)
        print(case, [(o["flag"], o["nli"]) for o in out], {k: v for k, v in census.items() if v})
        for k in total:
            total[k] += census[k]
    missing = [k for k in KR.CENSUS if total[k] == 0 and k != "qrsol_fail"]
    assert not missing, (missing, total)
    # each of the two lists of the device test reaches every flag but QRSOL_FAIL, and the zero-iteration return
    for maxl in K.MAXLS:
        idx = set(K.idx_for(maxl).tolist())
        seen = set()
        for case in K.solve_cases():
            if case[2] == maxl:
                _, out, _ = K.solve_reference(*case)
                seen |= {(out[s]["flag"], out[s]["nli"] == 0) for s in idx}
        assert {(0, True), (0, False), (1, False)} <= seen, (maxl, seen)
    _, out, _ = K.solve_reference("heat1d", 64, 1)
    assert out[4]["flag"] == KR.CONV_FAIL and 4 in K.idx_for(1)


def test_stepper_cases_contain_recovered_linear_failures():
    recovered = 0
    for kind, n, maxl in K.STEP_CASES:
        _, r = K.step_reference(kind, n, maxl)
        last = {k: r["counters"][k][-1] for k in KR.CNT}
        print(kind, n, maxl, "status", r["status"][-1], {k: last[k].tolist() for k in ("nst", "nni", "nli", "ncfl", "ncfn", "nsetups")})
        assert (last["nje"] == 0).all() and (last["nre_dq"] == last["nli"]).all() and (last["nli"] > 0).all()
        recovered += int(((r["status"][-1] == 0) & (last["ncfl"] > 0)).sum())
    assert recovered >= 3, recovered
    _, r = K.step_reference("heat1d", 65, 5)
    assert (r["status"] == 0).all() and (r["counters"]["ncfl"][-1] > 0).sum() >= 3
