"""The ground truth of the root-finding tests (tests/test_gpu_roots.py), on the CPU: the oracle itself with the product's function
family g_i = y[comp_i] - thr_i on every problem it has, through tests/native/roots_oracle.cpp (tests/roots_oracle.py).
  (a) around Roberts with the reference example's two functions the wrapper IS the oracle's built-in Roberts, bit for bit after
      every call: the decorator adds nothing of its own;
  (b) the committed cases (tests/roots_cases.py) meet what the GPU tests rely on, by the oracle alone: every system of every
      roots-only case returns a root; some return reports several functions at once; with a stop time at a system's own first root
      time the TSTOP and the ROOT return follow each other directly, in both orders; a TSTOP lies strictly between two root returns; a
      function that is exactly zero at t0 reports no root there; root finding itself fails at least once (CLOSE_ROOTS).
The two returns at a root time never carry an IDENTICAL tret (the count is printed: 0 in every case, also with one threshold set per
system): the step that is clipped to end at the stop time is another step than the one the roots-only run bracketed the root with, the
solution differs at the level of the tolerances, and the root moves by far more than the bracketing tolerance of 100 eps (|tn| + |hh|).
What is asserted is that no other return lies between the two, in either order."""
import numpy as np

import oracle_lib as O
import roots_cases as RC
import roots_oracle as RO
import stepper_ref as R
import tstop_oracle as T


def test_the_wrapper_around_roberts_is_the_builtin_roberts():
    from idahip import problems
    p = problems.roberts()
    w = RO.Harness(p, 0, roots=([0, 2], [1e-4, 0.01]))
    ref = O.OracleIda("roberts", 3, p["yy0"][0], p["yp0"][0], p["rtol"], p["atol"])
    nroot = 0
    for tout in p["touts"]:
        for _ in range(4):
            st_w, tret_w = w.solve(float(tout))
            st, tret = ref.solve(float(tout))
            assert st_w == st and R.same_bits(np.float64(tret_w), np.float64(tret))
            s = w.state()
            assert R.same_bits(s["yy"], ref.getv("yy")) and R.same_bits(s["yp"], ref.getv("yp"))
            assert np.array_equal(s["iroots"], ref.getv("iroots").astype(np.int32)) and s["nge"] == ref.get("nge")
            for k in T.SCALARS:
                assert R.same_bits(np.float64(s[k]), np.float64(ref.get(k))), k
            nroot += st == T.ROOT_RETURN
            if st == T.SUCCESS:
                break
        else:
            raise AssertionError("no end of root returns")
    assert nroot == 2 and ref.get("nge") == 404 and ref.get("nst") == 362  # the reference example's own figures


def test_the_committed_cases_meet_what_the_gpu_tests_rely_on():
    several = root_then_tstop = tstop_then_root = identical = tstop_between = close_roots = 0
    for name, variant, nroots in RC.all_cases():
        c = RC.case(name, variant, nroots)
        rec = RC.reference(c, RC.ops_on_harness(c))
        B = c["prob"]["yy0"].shape[0]
        status = np.array([r["status"] for r in rec])  # [calls][B]
        tret = np.array([r["tret"] for r in rec])
        nz = np.array([(r["iroots"] != 0).sum(axis=1) for r in rec])
        is_root = status == T.ROOT_RETURN
        print(c["name"], "thr", c["roots"][1], "root returns per system", is_root.sum(axis=0).tolist(), "negative",
              sorted(set(status[status < 0].tolist())))
        if nroots is None and variant in ("plain", "masked"):
            assert (is_root.sum(axis=0) >= 1).all(), (c["name"], is_root.sum(axis=0))
        assert is_root.any(), c["name"]
        several += int((nz[is_root] >= 2).sum())
        close_roots += int((status == RO.CLOSE_ROOTS).sum())
        assert ((status >= 0) | (status == RO.CLOSE_ROOTS)).all(), (c["name"], status[status < 0])
        if variant == "zero_at_t0":
            t0 = 0.0
            assert not (is_root & (tret == t0)).any() and (tret > t0).all()
            assert rec[0]["nge"][0] >= 2  # system 0 went through r_check1's second evaluation
        if variant == "tstop":
            assert (status == T.TSTOP_RETURN).any(), c["name"]
            for b in range(B):
                seq = [(int(status[i, b]), float(tret[i, b])) for i in range(len(rec))]
                for (s0, t0_), (s1, t1_) in zip(seq, seq[1:]):
                    if {s0, s1} == {T.ROOT_RETURN, T.TSTOP_RETURN}:
                        identical += t0_ == t1_
                        if b % 4 == 2:  # the stop time is this system's first root time
                            root_then_tstop += s0 == T.ROOT_RETURN
                            tstop_then_root += s0 == T.TSTOP_RETURN
                both = [(s_, t_) for s_, t_ in seq if s_ in (T.ROOT_RETURN, T.TSTOP_RETURN)]
                for i, (s0, t0_) in enumerate(both):
                    if s0 == T.TSTOP_RETURN:
                        before = [t for s_, t in both[:i] if s_ == T.ROOT_RETURN and t < t0_]
                        after = [t for s_, t in both[i + 1:] if s_ == T.ROOT_RETURN and t > t0_]
                        tstop_between += bool(before and after)
    print("returns with several functions", several, "ROOT then TSTOP", root_then_tstop, "TSTOP then ROOT", tstop_then_root,
          "at an identical tret", identical, "TSTOP between roots", tstop_between, "CLOSE_ROOTS", close_roots)
    assert several >= 1 and tstop_between >= 1 and close_roots >= 1
    assert root_then_tstop >= 1 and tstop_then_root >= 1


def test_roots_none_leaves_the_problem_as_the_oracle_has_it():
    """roots=None: Roberts keeps its own two functions; roots=([], []): none at all."""
    from idahip import problems
    p = problems.roberts()
    own, none = RO.Harness(p, 0), RO.Harness(p, 0, roots=([], []))
    assert own.solve(0.4)[0] == T.ROOT_RETURN and none.solve(0.4) == (T.SUCCESS, 0.4)
    assert own.state()["iroots"].tolist() == [0, -1] and none.state()["iroots"].size == 0 and none.state()["nge"] == 0
