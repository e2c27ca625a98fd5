"""IDACalcIC on the CPU: the numpy restatement (calcic_ref.py) against the properties the algorithm of DESIGN.md section 4f must
have, on exactly the inputs the GPU tests use (calcic_cases.py) -- so that those inputs are pinned before any GPU sees them -- and
the parts of the public interface that need no GPU."""
import ctypes as C

import numpy as np
import pytest

import calcic_cases as K
import calcic_ref as IC
import oracle_lib as O


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_steptol_bits():
    assert IC.STEPTOL.hex() == "0x1.428a2f98d7292p-35"
    assert IC.STEPTOL == 3.666852862501036e-11
    assert IC.EPS_NEWT == 0.01 * 0.33


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_reference_on_the_gpu_tests_inputs(name):
    c, r = K.case(name), K.reference(name)
    B = c["yy0"].shape[0]
    ok = r["status"] == 0
    failed = {int(b): int(r["status"][b]) for b in np.flatnonzero(~ok)}
    assert failed == K.EXPECTED_FAILURES.get(name, {}), failed
    assert ok.sum() * 4 >= 3 * B or name == "linesearch"
    diff = c["id"] == 1.0
    for b in np.flatnonzero(ok):
        if c["icopt"] == IC.YA_YDP_INIT:
            assert np.array_equal(bits(r["yy"][b][diff]), bits(c["yy0"][b][diff]))    # differential y: untouched
            assert np.array_equal(bits(r["yp"][b][~diff]), bits(c["yp0"][b][~diff]))  # algebraic y': untouched
        else:
            assert np.array_equal(bits(r["yp"][b]), bits(c["yp0"][b]))
        # a second run from the result has nothing to do
        again = IC.calc_ic(K.ref_problem(c, int(b)), r["yy"][b], r["yp"][b], c["rtol"], c["atol"], c["icopt"], c["tout1"], id=c["id"])
        assert again["status"] == 0 and again["counters"]["nni"] == 0
        # and the result is consistent: the residual is small against the weights' scale
        res = K.ref_problem(c, int(b)).res(r["yy"][b], r["yp"][b])
        assert np.isfinite(res).all()
    for b in np.flatnonzero(~ok):  # a failed system keeps what it was given
        assert np.array_equal(bits(r["yy"][b]), bits(c["yy0"][b])) and np.array_equal(bits(r["yp"][b]), bits(c["yp0"][b]))


def test_the_cases_reach_the_paths_they_are_meant_for():
    ls = K.reference("linesearch")
    assert ls["status"].tolist() == [0, 0, IC.CONV_FAIL, IC.LINESEARCH_FAIL, IC.NO_RECOVERY]
    assert ls["counters"]["nbacktr"][0] == 0 and ls["counters"]["nbacktr"][1] > 0
    assert ls["counters"]["nni"][4] == 0 and ls["counters"]["ncfn"][4] == IC.MAXNH
    assert ls["counters"]["nre"][3] > 500  # the no-root case backtracks to the end, step size after step size
    # step-size retries: some Roberts systems, and the first step size of the 65-node heat problem
    for name in ("roberts_satol", "roberts_vatol"):
        r = K.reference(name)
        assert (r["status"] == 0).all()
        nni = r["counters"]["nni"]
        assert nni.min() >= 5 and nni.max() > nni.min()  # the lists of the lock-step driver shrink unevenly
    assert (K.reference("heat65")["counters"]["ncfn"] > 0).all() and (K.reference("heat65")["status"] == 0).all()
    assert any((K.reference(n)["counters"]["ncfn"] > 0).any() for n in ("roberts_satol", "roberts_vatol"))
    for name in K.DQ:
        r = K.reference(name)
        assert (r["counters"]["nre_dq"] > 0).all() and (r["status"] == 0).all()
    assert (K.reference("linear40_yinit")["status"] == 0).all()


def test_mixed_cases_keep_the_properties_they_were_chosen_for():
    """The batches of K.MIXED on the reference alone: what each must show for its GPU test (test_gpu_calc_ic.py) to reach the fused
    trial kernels with a per-position lambda and cj, lists that shrink unevenly, ic_reset on a sublist and every failure status."""
    for name in K.MIXED:
        c, r = K.case(name), K.reference(name)
        assert r["status"].tolist() == K.MIXED_STATUS[name], (name, r["status"].tolist())
        for b in np.flatnonzero(r["status"] != 0):  # a failed system keeps what it was given
            assert np.array_equal(bits(r["yy"][b]), bits(c["yy0"][b])) and np.array_equal(bits(r["yp"][b]), bits(c["yp0"][b]))
        for b in np.flatnonzero(r["status"] == 0):
            again = IC.calc_ic(K.ref_problem(c, int(b)), r["yy"][b], r["yp"][b], c["rtol"], c["atol"], c["icopt"], c["tout1"], id=c["id"])
            assert again["status"] == 0, (name, b)  # (a second run has another hic, so it may iterate again; it must not fail)
    # Brusselator, Y_INIT: successes and failures side by side, backtracking in both, a different hic per system
    r = K.reference("bruss32_mixed")
    ok, cnt = r["status"] == 0, r["counters"]
    assert ok.any() and (r["status"] == IC.CONV_FAIL).any() and (r["status"] == IC.LINESEARCH_FAIL).any()
    assert (cnt["nbacktr"][ok] > 0).any() and (cnt["nbacktr"][~ok] > 0).any() and (cnt["nbacktr"][ok] == 0).any()  # lambda < 1 beside lambda = 1
    assert (cnt["nsetups"][ok] > 2).any()  # slow convergence: a second Jacobian at the same step size (delta <- savres)
    assert np.unique(r["hic"]).size == ok.size and len(set(cnt["nni"][ok].tolist())) >= 3
    assert (np.abs(K.case("bruss32_mixed")["yp0"]).max(axis=1) > 0.0).all()
    # heat, YA_YDP_INIT: part of the batch retries at hic/10 (ic_reset on a sublist, two cj in one launch) and then succeeds
    for name, hard in (("heat65_mixed", [1, 3]), ("heat1030", [1])):
        r = K.reference(name)
        assert (r["status"] == 0).all() and np.flatnonzero(r["counters"]["ncfn"] > 0).tolist() == hard, name
        assert np.unique(r["hic"]).size == r["hic"].size - len(hard) + 1  # (the hard ones start from y' = 0 and share theirs)
        assert (r["counters"]["nni"][hard] > 0).all() and np.delete(r["counters"]["nni"], hard).max() == 0
    # a singular system runs through all five step sizes while the others converge
    r = K.reference("linear40_singular")
    assert r["counters"]["ncfn"][5] == IC.MAXNH and r["counters"]["nni"][5] == 0 and r["counters"]["nsetups"][5] == IC.MAXNH
    assert (np.delete(r["status"], 5) == 0).all() and (np.delete(r["counters"]["ncfn"], 5) == 0).all()
    # +inf in y(0): the weight is +0.0, BAD_EWT before anything is counted; the rest of the batch as without it
    r, plain = K.reference("linear40_inf"), K.reference("linear40_mixed")
    assert all(r["counters"][k][3] == 0 for k in IC.COUNTERS) and r["ewt"][3] is None
    keep = np.arange(16) != 3
    assert np.array_equal(bits(r["yy"][keep]), bits(plain["yy"][keep])) and np.array_equal(bits(r["yp"][keep]), bits(plain["yp"][keep]))
    # the benchmark's size: a different hic per system from a non-zero y'(0)
    r = K.reference("linear512_mixed")
    assert (r["status"] == 0).all() and np.unique(r["hic"]).size == 4 and (r["hic"] < 1.0e-4).all()


def test_step_functions_are_what_calc_ic_is_made_of():
    """begin / commit on the weights' edge: a weight of +0.0 (an infinite component) or below zero (a negative entry of a vector
    atol) is bad, a NaN is not; trial_point moves y where diff is false and y' where it is true."""
    y, yp = np.array([1.0, -2.0, 3.0]), np.array([0.5, 0.25, -1.0])
    ewt, bad, nrm = IC.begin(y, yp, 1e-3, np.full(3, 1e-6))
    assert not bad and np.array_equal(bits(ewt), bits(IC.ewt_set(y, 1e-3, 1e-6))) and nrm == O.wrms(yp, ewt)
    assert IC.begin(np.array([1.0, np.inf, 3.0]), yp, 1e-3, np.full(3, 1e-6))[1]
    assert IC.begin(y, yp, 1e-3, np.array([1e-6, -1.0, 1e-6]))[1]
    assert not IC.begin(np.array([1.0, np.nan, 3.0]), yp, 1e-3, np.full(3, 1e-6))[1]
    assert IC.commit(np.array([1.0, np.inf, 3.0]), 1e-3, np.full(3, 1e-6))[1] and not IC.commit(np.array([np.nan, 1.0, 1.0]), 1e-3, np.full(3, 1e-6))[1]
    d = np.array([1.0, 2.0, 4.0])
    yn, ypn = IC.trial_point(y, yp, d, 0.5, 8.0, np.array([True, False, True]))
    assert yn.tolist() == [1.0, -3.0, 3.0] and ypn.tolist() == [-3.5, 0.25, -17.0]
    a = IC.accept(y, yp, yn, ypn, d, IC.Y_INIT)
    assert a[0] is yn and a[1] is yp and a[2] is d and IC.accept(y, yp, yn, ypn, d, IC.YA_YDP_INIT)[1] is ypn


def test_tout1_at_t0_is_ill_input_at_every_t0():
    """At t0 == tout1 == 0 the bound 2*eps*(|t0| + |tout1|) is 0 as well, so the distance 0 is refused by name."""
    c = K.case("linear9_one_alg")
    for t0, tout1, status in ((0.0, 0.0, IC.ILL_INPUT), (-0.0, 0.0, IC.ILL_INPUT), (1.0, 1.0, IC.ILL_INPUT),
                              (1.0, 1.0 + 2.0**-52, IC.ILL_INPUT), (0.0, 1e-300, None), (1.0, 1.0 + 2.0**-49, None)):
        r = IC.calc_ic(K.ref_problem(c, 0), c["yy0"][0], c["yp0"][0], c["rtol"], c["atol"], c["icopt"], tout1, id=c["id"], t0=t0)
        if status is None:
            assert r["status"] != IC.ILL_INPUT, (t0, tout1)
        else:
            assert r["status"] == status and sum(r["counters"].values()) == 0, (t0, tout1)
            assert np.array_equal(bits(r["yy"]), bits(c["yy0"][0])) and np.array_equal(bits(r["yp"]), bits(c["yp0"][0]))


def test_public_interface_without_a_gpu():
    import idahip
    assert callable(idahip.Ensemble.calc_ic) and callable(idahip.Ctx.set_id) and callable(idahip.Ctx.id)
    assert idahip.COUNTERS["nbacktr"] == 18 and (idahip.YA_YDP_INIT, idahip.Y_INIT) == (1, 2)
    H, E = idahip.load()
    st = np.zeros(1, dtype=np.int32)
    assert E.idaens_calc_ic(None, idahip.YA_YDP_INIT, 1.0, st.ctypes.data_as(C.POINTER(C.c_int32))) < 0
    assert H.idahip_set_id(None, None) < 0 and H.idahip_id(None, None) < 0
