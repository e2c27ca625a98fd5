"""Newton's restart with a stale Jacobian, several times per system, on every stepper against the oracle. The other oracle-backed
recipes take that restart at most once per system on the lock-step rounds; failure_recipes.repeated_jump_case scales A by 3 and by 1/3
alternately before each of eight touts, and every edited system restarts three to five times (tests/test_failure_recipes.py asserts
at least twice, on the oracle alone). The restart is ida_controller.hpp's newton_after_ctest on every stepper; what differs is
where it continues: the host stepper's list R in the same call, the lock-step rounds' newton_retry in the next round -- which may
be the next CALL (slices of one round), or a later round still when the round's setups are held back (idahip_set_lu_period).

Bar: np.array_equal against the oracle on status, t_ret, y, y' at every tout, on every counter of REF_COUNTERS, on kused and hused."""
import functools

import numpy as np
import pytest

import failure_recipes as F

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference(n):
    case = F.repeated_jump_case(n)
    ref = F.oracle_reference(case)
    for a in [ref["status"], ref["tret"], ref["yy"], ref["yp"], ref["kused"], ref["hused"]] + list(ref["counters"].values()):
        a.setflags(write=False)
    return ref


def run(case, how):
    """-> (ens, [(status, tret, yy, yp)] per tout) on the stepper `how`: host | device | sliced | held"""
    import idahip
    from idahip import problems
    p = case["prob"]
    B, n = p["yy0"].shape
    ctx = problems.make_ctx(p)
    if how == "held":
        ctx.set_lu_period(3)
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    ens.set_device_controller(0 if how == "host" else 1)
    assert ens.device_controller_active() == (0 if how == "host" else 2), ens.device_controller_active()
    cur, rec = {}, []
    for i, t in enumerate(case["before"] + case["after"]):
        F.apply_edits_to_ctx(ctx, case, i, cur)
        if how != "sliced":
            st, tret = ens.solve(t)
            rec.append((st.copy(), tret.copy(), ens.yy(), ens.yp()))
            continue
        Y, YP = np.full((B, n), np.nan), np.full((B, n), np.nan)
        for _ in range(100000):  # one round per call: a restart's second pass is the next call's
            st, tret, r, yo, ypo = ens.solve_schedule([t], max_rounds=1, outputs=True)
            m = ~np.isnan(yo[0])
            Y[m], YP[m] = yo[0][m], ypo[0][m]
            if (st != 99).all():
                break
        else:
            raise AssertionError("the schedule does not end")
        rec.append((st.copy(), tret.copy(), Y, YP))
    return ens, rec


@pytest.mark.parametrize("how", ["host", "device", "sliced", "held"])
@pytest.mark.parametrize("n", F.REPEATED_SIZES)
def test_repeated_restarts_equal_the_oracle(n, how):
    case = F.repeated_jump_case(n)
    ref = reference(n)
    ed = case["edited"]
    restarts = ref["counters"]["nls_nconvfails"] - ref["counters"]["ncfn"]
    assert (restarts[ed] >= 2).all() and (ref["status"] == 0).all(), (restarts, ref["status"])
    ens, rec = run(case, how)
    c = ens.counters()
    print(how, "n", n, "restarts", c["nls_nconvfails"] - c["ncfn"], "oracle", restarts, "nst", c["nst"], "rounds", ens.total_rounds())
    for i, (st, tret, yy, yp) in enumerate(rec):
        assert np.array_equal(st, ref["status"][i]), (i, st, ref["status"][i])
        assert np.array_equal(tret, ref["tret"][i]), (i, tret, ref["tret"][i])
        assert np.array_equal(yy, ref["yy"][i]) and np.array_equal(yp, ref["yp"][i]), i
    for k in F.REF_COUNTERS:
        assert np.array_equal(c[k], ref["counters"][k]), (k, c[k], ref["counters"][k])
    assert np.array_equal(c["kused"], ref["kused"]) and np.array_equal(ens.real("hused"), ref["hused"])
