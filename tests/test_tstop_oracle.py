"""The ground truth of the stop-time and masked-norm tests, on the CPU: the oracle itself with both switched on through
tests/native/tstop_oracle.cpp (tests/tstop_oracle.py), and the masked restatement of single kernel calls (tests/masked_ref.py).
  (a) with no stop time and suppressalg off the harness IS oracle_lib, bit for bit;
  (b) the committed stop-time cases (tests/tstop_cases.py) take every branch of the oracle's stop-time text at least once;
  (c) every case the GPU tests run with a mask takes another number of steps with it than without: otherwise those tests prove nothing;
  (d) masked_ref's sums are the oracle's norm_wrms_masked, and with an all-ones mask masked_ref is stepper_ref."""
import numpy as np
import pytest

import masked_ref as M
import oracle_lib as O
import stepper_ref as R
import tstop_cases as K
import tstop_oracle as T


def test_harness_without_switches_is_the_oracle():
    from idahip import problems
    for prob, touts in ((problems.roberts(), [0.4, 4.0]), (problems.linear_dense(n=12, batch=2), [0.1, 0.2])):
        ops = [("solve", t, T.NORMAL) for t in touts]
        if prob["kind"] == "roberts":  # its two roots are reported and the integration goes on, as oracle_run_ensemble does
            ops = [("solve", t, T.NORMAL) for t in touts for _ in range(3)]
        rec, hs = T.run_ops(prob, ops)
        kw = {k: prob[k] for k in ("A", "B", "c") if k in prob}
        ref = O.run_ensemble(prob["kind"], prob["n"], prob["yy0"], prob["yp0"], prob["rtol"], prob["atol"], touts, **kw)
        last = rec[-1]
        assert (last["status"] == 0).all() and (ref["status"] == 0).all()
        assert R.same_bits(last["yy"], ref["yy"][-1]) and R.same_bits(last["yp"], ref["yp"][-1])
        for k in ("nst", "nre", "nni", "netf", "ncfn", "nsetups"):
            assert np.array_equal(last[k].astype(np.int64), ref["counters"][k]), k
        assert np.array_equal(last["kused"].astype(np.int64), ref["kused"]) and R.same_bits(last["hused"], ref["hused"])
        assert all(h.census() == set() for h in hs)


def test_every_stop_time_branch_is_taken_by_the_committed_cases():
    seen = {}
    for name in K.STOP_CASES:
        case = K.stop_case(name)
        ops = K.ops_on_harness(case)
        rec, hs = T.run_ops(case["prob"], ops, **case["how"])
        got = set().union(*[h.census() for h in hs])
        print(name, sorted(got), "statuses", [r["status"].tolist() for r in rec])
        seen[name] = got
        # the property the GPU tests check on the product's trace: no accepted step ends beyond the stop time it was taken under
        for h in hs:
            steps = h.recorded_steps()
            for c in h.calls:
                if c["tstop0"] == c["tstop0"]:
                    for i in range(c["nst0"], c["nst1"]):
                        assert (steps[i, 0] - c["tstop0"]) * steps[i, 1] <= 0.0, (name, i)
        for r in rec:
            ts = r["status"] == T.TSTOP_RETURN
            assert np.isnan(r["tstop"][ts]).all()  # consumed
    assert set().union(*seen.values()) == T.BRANCHES, T.BRANCHES - set().union(*seen.values())


@pytest.mark.parametrize("name", sorted(K.MASK_CASES))
def test_the_mask_changes_the_step_count_of_every_masked_case(name):
    case = K.mask_case(name)
    prob, t = case["prob"], case["touts"][0]
    ops = [("solve", t, T.NORMAL)]
    plain, _ = T.run_ops(prob, ops)
    masked, _ = T.run_ops(prob, ops, id=case["id"], suppress=True)
    print(name, "steps at the first return: unmasked", plain[0]["nst"], "masked", masked[0]["nst"])
    differ = plain[0]["nst"] != masked[0]["nst"]
    assert differ.any()
    # (linear12's system 4 takes 34 steps either way -- other steps: no system is left untouched by the mask)
    assert all(differ[s] or not R.same_bits(plain[0]["yy"][s], masked[0]["yy"][s]) for s in range(differ.size))
    for s, (u, m) in K.MEASURED[name].items():  # the figures the cases were chosen by
        assert (int(plain[0]["nst"][s]), int(masked[0]["nst"][s])) == (u, m), s


def test_masked_ref_is_the_oracles_masked_norm():
    rng = np.random.default_rng(7)
    for n in (1, 3, 9, 300):
        x, w = R.nasty(rng, n), R.nasty(rng, n)
        ones, zeros, third = np.ones(n), np.zeros(n), (np.arange(n) % 3 != 2).astype(np.float64)
        with np.errstate(all="ignore"):
            assert R.same_bits(np.float64(M.wrms_masked(x, w, ones)), np.float64(O.wrms(x, w)))
            assert M.wrms_masked(x, w, zeros) == 0.0 or np.isnan(M.wrms_masked(x, w, zeros))
            p = (x * w) * third
            acc = 0.0
            for v in p:
                acc = acc + v * v
            assert R.same_bits(np.float64(M.wrms_masked(x, w, third)), np.sqrt(np.float64(acc) / n))
        # a NaN under a masked element still makes the norm NaN
        x2 = x.copy()
        x2[n - 1] = np.nan
        m = ones.copy()
        m[n - 1] = 0.0
        assert np.isnan(M.wrms_masked(x2, w, m))
    # with an all-ones mask the masked entry points are stepper_ref's
    n = 9
    phi = rng.uniform(-1, 1, (6, n))
    ee, ewt, yyp, ypp = rng.uniform(-1, 1, n), rng.uniform(1, 9, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    for kk in range(1, 6):
        a = R.post_newton(yyp, ypp, ee, ewt, phi, 2.5, kk)
        b = M.post_newton(yyp, ypp, ee, ewt, phi, 2.5, kk, np.ones(n))
        assert all(R.same_bits(u, v) for u, v in zip(a, b))
    a, b = R.init_first(phi, 1e-5, 1e-8), M.init_first(phi, 1e-5, 1e-8, np.ones(n))
    assert all(R.same_bits(np.float64(u), np.float64(v)) for u, v in zip(a, b))
    a, b = R.complete_step(phi, ee, 2, 0.7, 5, 1e-5, 1e-8), M.complete_step(phi, ee, 2, 0.7, 5, 1e-5, 1e-8, np.ones(n))
    assert all(R.same_bits(np.float64(u), np.float64(v)) for u, v in zip(a, b))
