"""tests/reinit_oracle.py on the CPU: the creator with a start time against roots_oracle's own creator, the first step of a system
created at t0 != 0, and the census of the event runs that tests/test_gpu_reinit.py compares with the product -- taken on the oracle's
records alone, so that the GPU tests are known to cross the paths they are meant to cross.

The jump of the event runs is reinit_oracle.JUMP = -0.5: dy = -0.5 * y at the component of every root function that fired. On roberts,
linear24 and heat20 that is enough: some system takes a failed error test or a Newton convergence failure within the first ten steps
after its first jump (test_census_of_the_event_runs asserts it). On lorenz it is not -- the first step after a restart is 0.001 of the
distance to tout, and the ten steps that follow it are smooth for dy = -0.5 y, -0.9 y and +1 y alike (netf = ncfn = 0 on every system
tried); dy = +4 y is the smallest of the values tried (4, 20, 100, 1000) at which the oracle fails an error test in those steps, so
reinit_oracle.JUMPS["lorenz"] = 4.0.
"""
import numpy as np
import pytest

import oracle_lib as O
import reinit_oracle as RI
import roots_cases as RC
import roots_oracle as RO
import stepper_ref as R
import tstop_oracle as T

EVENT_CASES = ("lorenz", "roberts", "linear24", "heat20")


@pytest.mark.parametrize("name", ["lorenz", "linear24"])
def test_creator_at_t0_zero_is_roots_oracles(name):
    c = RC.case(name)
    ops = RC.ops_on_harness(c)
    want = RC.reference(c, ops)
    got, _ = T.run_ops(c["prob"], ops, ids=[0, 1, 2], harness=RI.Harness, **c["how"])
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for k in w:
            assert R.same_bits(np.asarray(g[k], dtype=np.float64), np.asarray(w[k][:3], dtype=np.float64)), (name, k)


def test_reinit_to_the_problems_own_values_is_a_new_object():
    c = RC.case("lorenz")
    ops = RC.ops_on_harness(c)
    want = RC.reference(c, ops)
    h = RI.Harness(c["prob"], 1, **c["how"])
    assert h.solve(c["touts"][0])[0] in (T.SUCCESS, T.ROOT_RETURN)
    h.reinit(0.0, c["prob"]["yy0"][1], c["prob"]["yp0"][1])
    for op, w in zip(ops, want):
        st, tret = h.solve(op[1], op[2])
        s = h.state()
        assert st == w["status"][1] and tret == w["tret"][1]
        for k in w:
            if k in s:
                assert R.same_bits(np.asarray(s[k], dtype=np.float64), np.asarray(w[k][1], dtype=np.float64)), k


@pytest.mark.parametrize("t0,tout", [(0.75, 0.85), (2.0, 1.5), (-1.0, -0.5)])
def test_first_step_from_t0(t0, tout):
    """h0u is first_call_scalars' from tout - t0: 0.001 * |tout - t0|, or 0.5 / ||y0'|| where that norm exceeds 2 / h, signed by the
    direction; tn starts at t0."""
    from idahip import problems
    prob = problems.lorenz63(batch=4)
    for s in range(4):
        h = RI.Harness(prob, s, roots=([], []))
        h.reinit(t0, prob["yy0"][s], prob["yp0"][s])
        assert h.get("tn") == t0 and h.t0 == t0 and h.get("nst") == 0
        ewt = 1.0 / (prob["rtol"] * np.abs(prob["yy0"][s]) + prob["atol"])
        ypnorm = O.wrms(prob["yp0"][s], ewt)
        hh = 0.001 * abs(tout - t0)
        if ypnorm > 2.0 / hh:
            hh = 0.5 / ypnorm
        if tout < t0:
            hh = -hh
        st, _ = h.solve(tout, T.ONE_STEP)
        assert st == T.SUCCESS
        assert h.get("h0u") == hh, (h.get("h0u"), hh)
        steps = h.recorded_steps()
        assert steps[0, 0] == t0 + steps[0, 1] and steps[0, 1] * hh > 0.0 and abs(steps[0, 1]) <= abs(hh)  # tn = t0 + hused


@pytest.mark.parametrize("how", ["at_return", "host"])
@pytest.mark.parametrize("name", EVENT_CASES)
def test_census_of_the_event_runs(name, how):
    c = RC.case(name)
    B = c["prob"]["yy0"].shape[0]
    d = RI.HarnessEvents(c)
    # ten ONE_STEP calls on a twin of every system right after its first jump: failed error tests and Newton failures of those steps
    rough = []

    class Probe(RI.HarnessEvents):
        def jump(self, who, how_):
            RI.HarnessEvents.jump(self, who, how_)
            for b in who:
                if b in probed:
                    continue
                probed.add(b)
                h = self.hs[self.ids.index(b)]
                twin = RI.Harness(c["prob"], b, **c["how"])
                twin.reinit(h.t0, h._keep[0], h._keep[1])
                t_far = h.t0 + 10.0
                for _ in range(10):
                    if twin.solve(t_far, T.ONE_STEP)[0] < 0:
                        break
                rough.append(twin.get("netf") + twin.get("ncfn") + twin.get("nls_nconvfails"))

    probed = set()
    d = Probe(c)
    ops = RI.drive_events(c, d, how=how)
    rec = d.rec
    times = [set() for _ in range(B)]
    for r in rec:
        for b in np.nonzero(r["status"] == T.ROOT_RETURN)[0]:
            times[b].add(float(r["tret"][b]))
    assert sum(1 for o in ops if o[0] == "jump") >= 1
    if how == "host" and name in ("lorenz", "heat20"):
        # a system restarted beyond the first tout went back towards it: a later tout lies behind it and the call is refused. Lorenz
        # gets there from a SUCCESS at the first tout (r_check3 is entered: the evaluation the library does not make); heat, unstable
        # backwards, from TOO_MUCH_WORK (tretlast == tn: stop_test1 refuses, no root check on either side). Roberts and linear24 fail
        # their error tests on the way back and never see a later tout.
        bad = rec[-1]["status"] == RO.BAD_T
        assert bad.any() and (rec[-1]["hh"][bad] < 0.0).all(), rec[-1]["status"]
        assert sum(h.refused_evals for h in d.hs) >= (int(bad.sum()) if name == "lorenz" else 0)
        assert name != "heat20" or sum(h.refused_evals for h in d.hs) == 0
    if how == "at_return":  # (how = "host" restarts whoever has a root before the first tout, and those systems end there)
        assert all(len(t) >= 1 for t in times), "a system without a root return"
        first = {min(t) for t in times}
        assert len(first) >= 3, first
        assert len(probed) == B and max(rough) > 0, rough
    # the replay of the ops gives the same records (what the GPU tests rely on)
    again = RI.replay(c, ops, how=how)
    for g, w in zip(again, rec):
        for k in w:
            assert R.same_bits(np.asarray(g[k], dtype=np.float64), np.asarray(w[k], dtype=np.float64)), k
