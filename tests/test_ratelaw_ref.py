"""tests/ratelaw_ref.py (the float64 restatement of a network with rate laws that tests/test_gpu_rate_laws.py holds the device to) and
idahip.mass_action's flatten_laws / tables_laws pinned on things independent of them: a hand-written pattern, a central difference,
the polynomial restatement, the library's refusal texts; and the reference runs the GPU tests compare with end well. No GPU."""
import numpy as np
import pytest

import massaction_ref as MA
import ratelaw_ref as RL


def same_bits(a, b):
    a, b = (np.ascontiguousarray(np.asarray(x, dtype=np.float64)) for x in (a, b))
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


HAND = RL.HAND


def test_tables_of_a_hand_written_network():
    from idahip import mass_action
    tab = mass_action.tables_laws(4, HAND, [1.0, 1.0, 1.0, 0.0], 2)
    assert tab["order"] == [(0, 0), (1, 0), (1, 1), (3, 1), (2, 2), (3, 2), (2, 3), (3, 3)]
    assert (tab["nnz"], tab["ml"], tab["mu"]) == (8, 2, 1)
    assert tab["pattern"][(0, 0)] == [(-1.0, 0, (), -1), (-1.0, 0, (0,), 0)]  # the slot's term, then the factor's
    assert tab["pattern"][(1, 0)] == [(1.0, 0, (), -1), (1.0, 0, (0,), 0)]
    assert tab["pattern"][(2, 3)] == [(1.0, 1, (), 0)]
    assert tab["pattern"][(3, 1)] == [(1.0, 2, (2,), -1)] and tab["pattern"][(3, 2)] == [(1.0, 2, (1,), -1)]
    assert tab["pattern"][(1, 1)] == [] and tab["pattern"][(3, 3)] == []
    assert tab["factors"] == [[(1, 0, 0, 1)], [(2, 3, 1, 2)], []] and (tab["nreac"], tab["nconst"]) == (3, 2)
    # by value: row 0 = -k0 y0 * y0/(K0 + y0), row 2 = k1 * K1^2/(K1^2 + y3^2)
    prm, y = np.array([2.0, 3.0, 5.0, 0.5, 4.0]), np.array([1.5, 0.25, 2.0, 3.0])
    f = mass_action.rhs_laws(tab, prm, y)
    assert f[0] == -(2.0 * 1.5) * (1.5 / (0.5 + 1.5)) and f[1] == -f[0] and f[2] == 3.0 * (16.0 / (16.0 + 9.0)) and f[3] == 5.0 * 0.25 * 2.0
    net = RL.Net({"n": 4, "reactions": HAND, "d": [1.0, 1.0, 1.0, 0.0], "nconst": 2})
    assert same_bits(RL.res(net, prm, y, np.zeros(4)), -f)
    J = RL.jac(net, prm, 7.0, y)
    for i, j in [(i, j) for i in range(4) for j in range(4)]:
        assert ((i, j) in tab["pattern"]) or (J[j, i] == 0.0 and not np.signbit(J[j, i])), (i, j)


def test_jacobian_against_central_differences():
    """enzyme_chain(9): dF/dy by central differences of res with the step 1e-6 max(1, |y_j|) -- truncation of order step^2, rounding of
    order eps/step = 2e-10 -- against jac at cj = 0, relative to the largest entry of the matrix. The issue's prototype: 1.2e-10."""
    from idahip import problems
    p = problems.enzyme_chain(9, 4)
    net = RL.Net(p)
    worst = 0.0
    for s in range(4):
        y, yp, k = p["yy0"][s], p["yp0"][s], p["params"][s]
        J = RL.jac(net, k, 0.0, y)
        for j in range(9):
            h = 1.0e-6 * max(1.0, abs(y[j]))
            a, b = y.copy(), y.copy()
            a[j], b[j] = y[j] + h, y[j] - h
            fd = (RL.res(net, k, a, yp) - RL.res(net, k, b, yp)) / (a[j] - b[j])
            worst = max(worst, np.abs(fd - J[j]).max() / np.abs(J).max())
        Jc = RL.jac(net, k, 3.0, y)  # cj enters the diagonal alone
        assert np.array_equal(Jc - np.diag(np.diag(Jc)), J - np.diag(np.diag(J)))
    print("max relative deviation %.3g" % worst)
    assert worst < 1.0e-7, worst


def test_without_factors_it_is_the_polynomial_restatement():
    from idahip import mass_action, problems
    p = problems.reaction_chain(12, 3)
    a, b = MA.Net(p), RL.Net(p)
    rng = np.random.default_rng(12)
    for s in range(3):
        y, yp, cj = rng.uniform(-2.0, 2.0, 12), rng.uniform(-2.0, 2.0, 12), 10.0 ** rng.uniform(0.0, 3.0)
        assert same_bits(RL.res(b, p["params"][s], y, yp), MA.res(a, p["params"][s], y, yp))
        assert same_bits(RL.jac(b, p["params"][s], cj, y), MA.jac(a, p["params"][s], cj, y))
    flat, laws = mass_action.flatten(12, p["reactions"], p["d"]), mass_action.flatten_laws(12, p["reactions"], p["d"], 0)
    assert laws[1].shape == (0, 5) and all(np.array_equal(x, y) for x, y in zip(flat, laws[:1] + laws[2:]))
    ta, tb = mass_action.tables(12, p["reactions"], p["d"]), mass_action.tables_laws(12, p["reactions"], p["d"], 0)
    assert ta["order"] == tb["order"] and (ta["nnz"], ta["ml"], ta["mu"]) == (tb["nnz"], tb["ml"], tb["mu"])
    assert all([t[:3] for t in tb["pattern"][ij]] == ta["pattern"][ij] for ij in ta["order"])
    assert same_bits(mass_action.rhs_laws(tb, p["params"][0], p["yy0"][0]), mass_action.rhs(ta, p["params"][0], p["yy0"][0]))


REFUSALS, refused_network = RL.REFUSALS, RL.refused_network


@pytest.mark.parametrize("text,kw", REFUSALS, ids=[t.split(":")[-1].strip().replace(" ", "_")[:28] for t, _ in REFUSALS])
def test_flatten_laws_refuses(text, kw):
    from idahip import mass_action
    reactions, d, nconst = refused_network(kw)
    with pytest.raises(mass_action.NetworkError) as e:
        mass_action.flatten_laws(4, reactions, d, nconst)
    assert str(e.value) == text
    mass_action.flatten_laws(4, HAND, [1.0, 1.0, 1.0, 0.0], 3)  # (a constant no factor uses is allowed)


@pytest.mark.parametrize("name", list(RL.CASES))
def test_reference_runs_end_well(name):
    """the integrations tests/test_gpu_rate_laws.py compares with: status 0 at every output, Newton iterations beyond one per step,
    and error-test failures in the n = 16 case (a network that dies early would be compared, not caught, otherwise)"""
    p, touts, ref = RL.case(name)
    c = ref["counters"]
    print(name, "nst %d..%d" % (c["nst"][-1].min(), c["nst"][-1].max()), "netf", int(c["netf"][-1].sum()), "ncfn", int(c["ncfn"][-1].sum()))
    assert (ref["status"] == 0).all()
    assert (c["nni"][-1] > c["nst"][-1]).all()
    if name == "n16":
        assert c["netf"][-1].sum() > 0
