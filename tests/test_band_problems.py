"""CPU checks of what the band-width GPU tests (tests/test_gpu_band_widths.py) stand on.

1. tests/band_problems.py's banded linear DAE does what it is for, asserted from the oracle alone: the oracle integrates every
   case the GPU tests integrate (status 0 at every output, ten or more linear setups per system), and for every case with
   ml, mu >= 1 every system's Jacobian -- the first one the oracle forms, and those at cj = 10 and 1000 -- has swapped rows and
   non-zero entries of U above the mu-th super-diagonal. Without these a band solve that ignored the fill would pass.
2. The Python restatements of the residuals and analytic Jacobians (tests/dq_ref.py), which three GPU test files use as the
   reference, are the oracle's functions bit for bit (oracle_problem_res / oracle_problem_jac over oracle/problems.hpp), on
   inputs with zeros of both signs, subnormals, infinities and NaN."""
import numpy as np
import pytest

import band_problems as BP
import dq_ref as R
import oracle_lib as O
import stepper_ref as S


def swaps_and_fill(prob, s, cj):
    """(rows swapped, non-zero entries of U above the mu-th super-diagonal, info) of the oracle's getrf of B_s + cj A_s."""
    n, (ml, mu) = prob["n"], prob["band"]
    cm = np.ascontiguousarray(BP.jacobian(prob, s, cj)[None])
    info, piv = O.getrf_batch(cm, nthreads=1)
    ii, jj = np.indices((n, n))
    lu = cm[0].T
    assert not np.any(lu[(jj - ii) > ml + mu])  # the theory: U has at most ml + mu super-diagonals
    return int((piv[0] != np.arange(n)).sum()), int(np.count_nonzero(lu[(jj - ii) > mu])), int(info[0])


@pytest.mark.parametrize("n,ml,mu", BP.INTEGRATIONS)
def test_the_oracle_integrates_every_case_and_refactors(n, ml, mu):
    B = 3
    p = BP.banded_linear(n, ml, mu, B)
    ref = O.run_ensemble("linear_dense", n, p["yy0"], p["yp0"], p["rtol"], p["atol"], p["touts"], A=p["A"], B=p["B"], c=p["c"], nthreads=B)
    assert (ref["status"] == 0).all(), ref["status"]
    assert np.isfinite(ref["yy"]).all() and np.isfinite(ref["yp"]).all()
    assert (ref["counters"]["nsetups"] >= 10).all(), ref["counters"]["nsetups"]
    assert (ref["counters"]["nst"] >= 20).all()


@pytest.mark.parametrize("n,ml,mu", [c for c in BP.INTEGRATIONS + BP.setup_cases() if c[1] >= 1 and c[2] >= 1 and c[0] <= 1100])
def test_every_jacobian_swaps_rows_and_fills(n, ml, mu):
    B = 3
    p = BP.banded_linear(n, ml, mu, B)
    for s in range(B):
        o = O.OracleIda("linear_dense", n, p["yy0"][s], p["yp0"][s], p["rtol"], p["atol"], A=p["A"][s], B=p["B"][s], c=p["c"][s])
        st, _ = o.solve(float(p["touts"][0]), itask=1)  # one step: cj is the first Jacobian's
        assert st == 0 and o.get("nsetups") >= 1
        for cj in (o.get("cj"), 10.0, 1000.0):
            swaps, fill, info = swaps_and_fill(p, s, cj)
            assert info == 0 and swaps >= 1, (s, cj, swaps, info)
            assert fill >= 1 or mu == n - 1, (s, cj, fill)  # (the full band has no entry above its mu-th super-diagonal)


def test_the_generator_keeps_to_its_band_and_is_consistent():
    for n, ml, mu in ((64, 2, 3), (24, 23, 23), (17, 0, 2), (17, 3, 0), (9, 0, 0)):
        p = BP.banded_linear(n, ml, mu, 2)
        out = ~BP.in_band(n, ml, mu)
        for s in range(2):
            assert not np.any(p["A"][s].T[out]) and not np.any(p["B"][s].T[out])
            r = O.problem_res("linear_dense", n, p["yy0"][s], p["yp0"][s], A=p["A"][s], B=p["B"][s], c=p["c"][s])
            assert np.abs(r).max() < 1e-12  # consistent initial values
        q = BP.banded_linear(n, ml, mu, 2)
        assert all(np.array_equal(p[k], q[k]) for k in ("A", "B", "c", "yy0", "yp0"))  # the same systems at every call


# ------------------------------------------------------------------------------------------------ the restatements, bit for bit
def nasty_pair(rng, n):
    """yy, yp with zeros of both signs and subnormals (stepper_ref.nasty), then an infinity and a NaN placed."""
    yy, yp = S.nasty(rng, n), S.nasty(rng, n)
    plain = (S.nasty(rng, n, special=False), S.nasty(rng, n, special=False))
    spiked = (yy.copy(), yp.copy())
    spiked[0][n // 2] = np.inf
    spiked[1][0] = -np.inf
    spiked[0][n - 1] = np.nan
    spiked[1][n // 3] = np.nan
    return [plain, (yy, yp), spiked]


def systems(rng):
    """(kind, n, oracle keyword arguments, dq_ref sysdata) of the four device problems."""
    out = [("roberts", 3, {}, {}),
           ("lorenz63", 3, {"params": np.array([10.0, 28.0, 8.0 / 3.0])}, None),
           ("lorenz63", 3, {"params": rng.uniform(0.5, 30.0, 3)}, None)]
    for n in (9, 64, 257):
        out.append(("heat1d", n, {"params": np.array([rng.uniform(0.5, 2.0) * (n - 1) ** 2])}, None))
    for n, ml, mu in ((9, 8, 8), (64, 2, 3), (257, 0, 2)):
        p = BP.banded_linear(n, ml, mu, 1)
        out.append(("linear_dense", n, {"A": p["A"][0], "B": p["B"][0], "c": p["c"][0]}, None))
    A, Bm = S.nasty(rng, (24, 24)), S.nasty(rng, (24, 24))  # (a dense system with zeros of both signs and huge entries)
    out.append(("linear_dense", 24, {"A": A, "B": Bm, "c": S.nasty(rng, 24)}, None))
    res = []
    for kind, n, kw, _ in out:
        data = dict(kw)
        if kind == "heat1d":
            data["coef"] = kw["params"][0]
        res.append((kind, n, kw, data))
    return res


def test_residual_restatements_are_the_oracles_bits():
    rng = np.random.default_rng(20240)
    for kind, n, kw, data in systems(rng):
        fn = R.residual_fn(kind, data)
        for yy, yp in nasty_pair(rng, n):
            assert S.same_bits(fn(yy, yp), O.problem_res(kind, n, yy, yp, **kw)), (kind, n)


def test_named_residuals_are_the_oracles_bits():
    """roberts_res, lorenz_res, linear_res and heat_res called by name (residual_fn only dispatches to them)."""
    rng = np.random.default_rng(20241)
    for kind, n, kw, data in systems(rng):
        for yy, yp in nasty_pair(rng, n):
            want = O.problem_res(kind, n, yy, yp, **kw)
            got = {"roberts": lambda: R.roberts_res(yy, yp), "lorenz63": lambda: R.lorenz_res(kw["params"], yy, yp),
                   "linear_dense": lambda: R.linear_res(kw["A"], kw["B"], kw["c"], yy, yp),
                   "heat1d": lambda: R.heat_res(float(kw["params"][0]), yy, yp)}[kind]()
            assert S.same_bits(got, want), (kind, n)


def test_analytic_jacobian_restatement_is_the_oracles_bits():
    rng = np.random.default_rng(20242)
    for kind, n, kw, data in systems(rng):
        for yy, yp in nasty_pair(rng, n):
            for cj in (0.0, 3.7, 1.0e6, -2.5):
                with np.errstate(all="ignore"):
                    got = R.analytic_jac(kind, data, cj, yy)
                assert S.same_bits(got, O.problem_jac(kind, n, cj, yy, yp, **kw)), (kind, n, cj)


def test_band_callbacks_are_the_oracles_functions():
    """host_callbacks' res is the oracle's residual; its bjac, unpacked, is the oracle's Jacobian (every entry outside the band is
    +0.0 in both)."""
    import idahip
    rng = np.random.default_rng(20243)
    for n, ml, mu in ((17, 2, 3), (64, 7, 5), (24, 23, 23), (17, 0, 2), (17, 3, 0)):
        p = BP.banded_linear(n, ml, mu, 2)
        res, bjac = BP.host_callbacks(p)
        for s in range(2):
            kw = {"A": p["A"][s], "B": p["B"][s], "c": p["c"][s]}
            for yy, yp in nasty_pair(rng, n)[:2]:
                assert S.same_bits(res(s, 0.0, yy, yp), O.problem_res("linear_dense", n, yy, yp, **kw))
                for cj in (12.5, 1.0e4):
                    ab = bjac(s, 0.0, cj, yy, yp, None, None)
                    assert ab.shape == (n, idahip.band_ldab(ml, mu)) and not np.any(ab[:, :ml])  # fill rows +0.0
                    dense = idahip.band_unpack(ab, n, ml, mu)  # logical (row, column)
                    assert S.same_bits(np.ascontiguousarray(dense.T), O.problem_jac("linear_dense", n, cj, yy, yp, **kw)), (n, ml, mu, s, cj)
