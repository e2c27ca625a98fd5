"""IDACalcIC on the CPU: the numpy restatement (calcic_ref.py) against the properties the algorithm of DESIGN.md section 4f must
have, on exactly the inputs the GPU tests use (calcic_cases.py) -- so that those inputs are pinned before any GPU sees them -- and
the parts of the public interface that need no GPU."""
import ctypes as C

import numpy as np
import pytest

import calcic_cases as K
import calcic_ref as IC


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
