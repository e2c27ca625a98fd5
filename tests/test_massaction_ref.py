"""tests/massaction_ref.py (the float64 restatement of IDAHIP_MASS_ACTION that tests/test_gpu_mass_action.py holds the device to) pinned
on things independent of it -- the Brusselator restatement, the oracle's Roberts and Lorenz problems, a central difference --, the
networks of idahip.problems integrated against the built-in kinds they restate, and the Python binding's own checks of a network.
No GPU."""
import json
import os

import numpy as np
import pytest

import bruss_ref as BR
import massaction_ref as MA
import oracle_lib as O

EPS = np.finfo(np.float64).eps
HERE = os.path.dirname(os.path.abspath(__file__))


def abs_net(net):
    """the network with |nu| and |d|: evaluated at |k|, |y|, -|y'| (cj: -|cj|) its residual (Jacobian) is minus the sum of the
    magnitudes of a row's (a position's) terms"""
    import copy
    a = copy.copy(net)
    a.rows = [[(abs(nu), r) for nu, r in row] for row in net.rows]
    a.d = [abs(x) for x in net.d]
    return a


def res_terms(net, k, y, yp):
    return np.abs(MA.res(abs_net(net), np.abs(k), np.abs(y), -np.abs(yp)))


def jac_terms(net, k, cj, y):
    return np.abs(MA.jac(abs_net(net), np.abs(k), -abs(cj), np.abs(y)))


def points(n, count, seed):
    rng = np.random.default_rng(seed)
    return [(rng.uniform(-1.0e3, 1.0e3, n), rng.uniform(-1.0e3, 1.0e3, n), float(rng.uniform(1.0, 1.0e3))) for _ in range(count)]


# ------------------------------------------------------------------------------------------------ 1. the restatement is pinned
def check_against(net, k, sign, ref_res, ref_jac, n, seed):
    """row by row within 16 eps sum|terms of the row| (no row of these problems has more than 16 operations in either form, each
    with a relative error of at most eps/2 of a partial sum that the sum of the magnitudes bounds); sign: the network's rows are
    sign[i] times the reference's"""
    for y, yp, cj in points(n, 8, seed):
        r, rt = MA.res(net, k, y, yp), res_terms(net, k, y, yp)
        assert (np.abs(r - sign * ref_res(y, yp)) <= 16.0 * EPS * rt).all(), (r, ref_res(y, yp))
        J, Jt = MA.jac(net, k, cj, y), jac_terms(net, k, cj, y)
        assert (np.abs(J - sign[None, :] * ref_jac(cj, y, yp)) <= 16.0 * EPS * Jt).all()
        assert (J[Jt == 0.0] == 0.0).all() and not np.signbit(J[Jt == 0.0]).any()  # +0.0 where there is no term


def test_bruss1d_network_is_the_brusselator():
    from idahip import problems
    p, q = problems.bruss1d_network(8, 5), problems.bruss1d(8, 5)
    net = MA.Net(p)
    for s in (0, 4):
        prm = q["params"][s]
        check_against(net, p["params"][s], np.ones(16), lambda y, yp: BR.res(prm, y, yp), lambda cj, y, yp: BR.jac(prm, cj, y), 16, 10 + s)
    assert np.array_equal(p["yy0"], q["yy0"]) and np.array_equal(p["yp0"], q["yp0"])


def test_roberts_network_is_roberts():
    """the differential rows with the opposite sign (y' - f against the reference's f - y'), the conservation row as it is"""
    from idahip import problems
    p = problems.roberts_network()
    sign = np.array([-1.0, -1.0, 1.0])
    check_against(MA.Net(p), p["params"][0], sign, lambda y, yp: O.problem_res("roberts", 3, y, yp),
                  lambda cj, y, yp: O.problem_jac("roberts", 3, cj, y, yp), 3, 3)


def test_lorenz63_network_is_lorenz63():
    from idahip import problems
    p, q = problems.lorenz63_network(4), problems.lorenz63(4)
    prm = q["params"][2]
    check_against(MA.Net(p), p["params"][2], np.ones(3), lambda y, yp: O.problem_res("lorenz63", 3, y, yp, params=prm),
                  lambda cj, y, yp: O.problem_jac("lorenz63", 3, cj, y, yp, params=prm), 3, 63)
    assert np.array_equal(p["yy0"], q["yy0"]) and np.array_equal(p["yp0"], q["yp0"])


def test_jac_is_the_derivative_of_res_on_a_reaction_chain():
    """reaction_chain(n = 12) has reactions of order <= 2, so a central difference of res is exact but for rounding: each of its two
    residuals is within 16 eps of the sum S_i of the magnitudes of its row's terms (the hub row and the conservation row have more
    terms than 16: the bound is taken per term count, ceil(terms / 16) times as wide), so the quotient is within
    w_i 16 eps S_i / h of the derivative; jac itself within w_i 16 eps of its own terms' magnitudes."""
    from idahip import problems
    p = problems.reaction_chain(12, 3)
    net = MA.Net(p)
    assert max(len(net.slots[r]) for r in range(net.nreac)) == 2
    width = np.array([max(1, -(-(len(row) + 2) // 16)) for row in net.rows], dtype=np.float64)
    rng = np.random.default_rng(12)
    for s in range(3):
        k = p["params"][s]
        y, yp, cj = rng.uniform(-1.0e3, 1.0e3, 12), rng.uniform(-1.0e3, 1.0e3, 12), 37.0
        J, Jt = MA.jac(net, k, cj, y), jac_terms(net, k, cj, y)
        for j in range(12):
            h = 2.0 ** -17 * max(1.0, abs(y[j]))
            yl, yr, pl, pr = y.copy(), y.copy(), yp.copy(), yp.copy()
            yr[j], yl[j] = y[j] + h, y[j] - h
            h = (yr[j] - yl[j]) / 2.0
            pr[j], pl[j] = yp[j] + cj * h, yp[j] - cj * h
            cd = (MA.res(net, k, yr, pr) - MA.res(net, k, yl, pl)) / (2.0 * h)
            S = np.maximum(res_terms(net, k, yr, pr), res_terms(net, k, yl, pl))
            bound = width * 16.0 * EPS * (S / h + Jt[j])
            assert (np.abs(J[j] - cd) <= bound).all(), (s, j, np.abs(J[j] - cd) / bound)
        assert np.count_nonzero(J) > 12


def test_dense_dq_is_dq_ref_on_the_restated_residual():
    from idahip import problems
    import dq_ref as DQ
    p = problems.reaction_chain(9, 2)
    net, k = MA.Net(p), p["params"][1]
    y, yp = p["yy0"][1], p["yp0"][1]
    ewt = 1.0 / (p["rtol"] * np.abs(y) + p["atol"][0])
    rr = MA.res(net, k, y, yp)
    J = MA.dense_dq(net, k, y, yp, ewt, rr, 50.0, -1.0e-3)
    A = MA.jac(net, k, 50.0, y)
    assert np.abs(J - A).max() <= 1.0e-4 * np.abs(A).max()  # (a difference quotient of a quadratic: a sanity check, not a pin)
    assert np.array_equal(J, DQ.dense_dq(MA.prob_res(p, 1), y, yp, ewt, rr, 50.0, -1.0e-3))


# ------------------------------------------------------------------------------------------------ 2. integrations, by value
def wrms_of(diff, y, rtol, atol):
    atol = np.asarray(atol, dtype=np.float64)
    return float(O.wrms(diff, 1.0 / (rtol * np.abs(y) + (atol if atol.size == y.size else atol[0]))))


def test_roberts_network_integrates_as_roberts():
    """DirectIda on roberts_network against OracleIda on IDAHIP_ROBERTS at the first three outputs of the reference's example
    (t = 0.4, 4, 40). Yardstick: the built-in kind's own truncation error, its run at rtol against its run at rtol / 100, both
    differences in the WRMS norm of the network run's ewt. Measured (network - built-in, built-in - built-in at rtol / 100):
    t = 0.4: 0.0 / 2.651e-02;  t = 4: 0.0 / 3.972e-01;  t = 40: 0.0 / 8.813e-01 -- reversing the sign of a row changes no bit of a
    Newton correction, and these three rows round the same in both forms along this run."""
    from idahip import problems
    g = json.load(open(os.path.join(HERE, "golden", "roberts_example.json")))
    p = problems.roberts_network()
    assert p["rtol"] == g["rtol"] and list(p["atol"]) == g["atol"]
    touts = [g["tout0"] * g["tout_factor"] ** i for i in range(3)]
    net_run = MA.run(p, touts)
    coarse = O.OracleIda("roberts", 3, p["yy0"][0], p["yp0"][0], p["rtol"], p["atol"])
    fine = O.OracleIda("roberts", 3, p["yy0"][0], p["yp0"][0], p["rtol"] / 100.0, p["atol"])
    def to(ida, t):  # (the oracle's Roberts carries the example's two root functions: a root return is reported, then it goes on)
        st = 2
        while st == 2:
            st = ida.solve(t)[0]
        return st

    for i, t in enumerate(touts):
        assert to(coarse, t) == 0 and to(fine, t) == 0 and net_run["status"][i, 0] == 0
        y = net_run["yy"][i, 0]
        mine = wrms_of(y - coarse.getv("yy"), y, p["rtol"], p["atol"])
        yard = wrms_of(coarse.getv("yy") - fine.getv("yy"), y, p["rtol"], p["atol"])
        print("roberts t = %g: network - built-in %.3e, built-in - built-in(rtol/100) %.3e" % (t, mine, yard))
        assert mine <= yard, (t, mine, yard)


def test_bruss1d_network_integrates_as_bruss1d():
    """DirectIda on bruss1d_network(m = 8) against bruss_ref.DirectIda on IDAHIP_BRUSS1D to t = 0.1, systems 1, 3, 4, 6; the same
    yardstick. Measured (network - built-in, built-in - built-in at rtol / 100): system 1: 0.0 / 6.067e-01; 3: 0.0 / 9.013e-01;
    4: 3.734e-11 / 1.063e+00; 6: 0.0 / 1.345e+00."""
    from idahip import problems
    ids = [1, 3, 4, 6]
    p, q = problems.bruss1d_network(8, 7), problems.bruss1d(8, 7)
    net_run = MA.run(p, [0.1], ids=ids)
    coarse = BR.run(q, [0.1], mode="direct", ids=ids)
    fine = BR.run(dict(q, rtol=q["rtol"] / 100.0), [0.1], mode="direct", ids=ids)
    assert (net_run["status"] == 0).all() and (coarse["status"] == 0).all() and (fine["status"] == 0).all()
    for b, s in enumerate(ids):
        y = net_run["yy"][0, b]
        mine = wrms_of(y - coarse["yy"][0, b], y, p["rtol"], p["atol"])
        yard = wrms_of(coarse["yy"][0, b] - fine["yy"][0, b], y, p["rtol"], p["atol"])
        print("bruss1d system %d: network - built-in %.3e, built-in - built-in(rtol/100) %.3e" % (s, mine, yard))
        assert mine <= yard, (s, mine, yard)


# ------------------------------------------------------------------------------------------------ 3. the binding's own checks
def test_flatten_refuses_what_the_library_refuses():
    from idahip import mass_action as M
    ok = [((0, 1), {0: -1.0, 1: 1.0}), ((), {2: 1.0})]
    d = [1.0, 1.0, 0.0]
    s, rows, reacs, nu, dd = M.flatten(3, ok, d)
    assert s.tolist() == [[0, 1, -1], [-1, -1, -1]] and rows.tolist() == [0, 1, 2] and reacs.tolist() == [0, 0, 1]
    assert nu.tolist() == [-1.0, 1.0, 1.0] and dd.tolist() == d
    for bad, dv, text in (
            ([], d, "nreac = 0"),
            ([((0, 1, 2, 0), {0: 1.0})], d, "order 4"),
            ([((0, 3), {0: 1.0})], d, "reaction 0, slot 1: species 3"),
            ([((0,), {0: 1.0}), ((-2,), {0: 1.0})], d, "reaction 1, slot 0: species -2"),
            ([((0, -1, 1), {0: 1.0})], d, "reaction 0, slot 2: a species after an unused slot"),
            (ok + [((1,), {3: 1.0})], d, "entry 3: row 3"),
            (ok + [((1,), {-1: 1.0})], d, "entry 3: row -1"),
            (ok + [((1,), {0: float("nan")})], d, "entry 3: nu = nan"),
            (ok + [((1,), {0: float("inf")})], d, "entry 3: nu = inf"),
            (ok, [1.0, float("inf"), 0.0], "d[1] = inf"),
            (ok, [1.0, 1.0], "d has shape"),
    ):
        with pytest.raises(M.NetworkError, match=text.replace("[", r"\[").replace("]", r"\]")):
            M.flatten(3, bad, dv)
    assert M.flatten(3, [((0, -1, -1), {0: 1.0})], d)[0].tolist() == [[0, -1, -1]]  # trailing -1 written out: fine


def test_entry_order_within_a_row_survives():
    """row 0 = 1e16 + 1 - 1e16 summed in the caller's order is 0.0; in any order that adds 1 last it is 1.0"""
    from idahip import mass_action as M
    reactions = [((), {0: 1.0e16}), ((), {1: 2.0, 0: 1.0}), ((), {0: -1.0e16})]
    prob = {"n": 2, "reactions": reactions, "d": [1.0, 1.0]}
    t = M.tables(2, reactions, [1.0, 1.0])
    assert t["rows"][0] == [(1.0e16, 0), (1.0, 1), (-1.0e16, 2)] and t["rows"][1] == [(2.0, 1)]
    k = np.ones(3)
    assert M.rhs(t, k, np.zeros(2)).tolist() == [0.0, 2.0]
    assert MA.res(MA.Net(prob), k, np.zeros(2), np.zeros(2)).tolist() == [-0.0, -2.0]
    swapped = [reactions[0], reactions[2], reactions[1]]
    assert M.rhs(M.tables(2, swapped, [1.0, 1.0]), k, np.zeros(2)).tolist() == [1.0, 2.0]


def test_patterns_and_bandwidths():
    from idahip import mass_action as M, problems
    p = problems.bruss1d_network(8, 1)
    t = M.tables(p["n"], p["reactions"], p["d"])
    assert (t["ml"], t["mu"]) == (2, 2)
    J = BR.jac(problems.bruss1d(8, 1)["params"][0], 3.0, p["yy0"][0])
    want = {(i, j) for j in range(16) for i in range(16) if J[j, i] != 0.0 or i == j}
    assert set(t["order"]) == want and t["nnz"] == len(want)
    assert t["order"] == sorted(t["order"], key=lambda ij: (ij[1], ij[0]))  # column-major
    r = problems.roberts_network()
    t = M.tables(3, r["reactions"], r["d"])
    assert t["nnz"] == 9 and (t["ml"], t["mu"]) == (2, 2)
    assert t["pattern"][(1, 1)] == [(-1.0, 1, (2,)), (-1.0, 2, (1,)), (-1.0, 2, (1,))]  # y1^2: one term per slot, in slot order
    c = problems.reaction_chain(12, 1)
    t = M.tables(12, c["reactions"], c["d"])
    sizes = [len(row) for row in t["rows"]]
    assert sizes[10] == 0 and sizes[0] > 64 and c["d"][11] == 0.0 and (c["d"][:11] == 1.0).all()
    assert t["pattern"][(10, 10)] == [] and all(i == 10 and j == 10 for i, j in t["order"] if 10 in (i, j))
    k = c["params"][0]
    assert k[:-13].min() < 1.0e-2 and k[:-13].max() > 1.0e2  # spread over the six decades
