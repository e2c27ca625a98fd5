"""A reaction network of n <= 8 species on the one-thread stepper (idahip_set_mass_action_tiny; tiny_net_ida_kernel of
csrc/tiny_net_ida.hpp: a whole solve call in one launch, one thread per system interpreting the network's tables) against
tests/massaction_ref.py and tests/ratelaw_ref.py, bit for bit (view(np.uint64) equality: no tolerance appears in this file) and with
no system left out: status, tret, yy, yp, hused, tn, kused and every counter at every output. Where the two references do not model a
feature -- roots, a stop time, masked norms, a tout behind t0, reinit, calc_ic, a step limit -- the reference is the host stepper on
the same ctx with the switch off, which the existing tests pin to the oracle for each of them."""
import ctypes as C
import re

import numpy as np
import pytest

import massaction_ref as MA
import ratelaw_ref as RL
from test_gpu_mass_action import assert_equals_reference, roberts_batch, same_bits, snapshot

pytestmark = pytest.mark.gpu
CNT = MA.RUN_CNT
_CACHE = {}


class TinyCall(C.Structure):  # idahip_tiny_call of include/ida_hip.h
    _fields_ = [("touts", C.c_void_p), ("ntout", C.c_int), ("recycle", C.c_int), ("resume", C.c_int), ("max_rounds", C.c_long),
                ("mxstep", C.c_long), ("maxord", C.c_int), ("maxnef", C.c_long), ("maxncf", C.c_long), ("epcon", C.c_double),
                ("hmax_inv", C.c_double), ("t0", C.c_double), ("start_round", C.c_void_p), ("round_base", C.c_int64),
                ("nroots", C.c_int), ("root_comps", C.c_void_p), ("root_thresholds", C.c_void_p), ("root_states", C.c_void_p)]


def ab_network(B=5):
    """A <-> B with the total conserved: y0' = -k0 y0 + k1 y1 (differential) and 0 = y0 + y1 - T (algebraic, as roberts_network
    writes its conservation row): n = 2, the smallest the kind admits. System s has k0 scaled by 1 + s/4."""
    from idahip import problems
    reactions = [((0,), {0: -1.0}), ((1,), {0: 1.0}), ((0,), {1: -1.0}), ((1,), {1: -1.0}), ((), {1: 1.0})]
    k = np.tile(np.array([3.0, 1.0, 1.0, 1.0, 2.0]), (B, 1))
    k[:, 0] *= 1.0 + np.arange(B) / 4.0
    yy0 = np.tile(np.array([1.5, 0.5]), (B, 1))
    f0 = -k[:, 0] * yy0[:, 0] + k[:, 1] * yy0[:, 1]
    yp0 = np.stack([f0, -f0], axis=1)
    return problems._network(2, reactions, [1.0, 0.0], k, yy0, yp0, 1e-6, np.array([1e-8]), np.array([0.1, 0.2, 0.4]))


def _problem(name):
    from idahip import problems
    if name == "roberts":
        return roberts_batch(5), (0.4, 4.0)
    if name == "lorenz":
        return problems.lorenz63_network(67), (0.1, 0.2)
    if name == "ab2":
        return ab_network(5), (0.1, 0.2, 0.4)
    if name == "chain7dq":
        return problems.reaction_chain(7, 9, seed=7), (0.01, 0.02)
    if name == "enzyme8dq":
        return problems.enzyme_chain(8, 5), (0.01, 0.02)
    if name.startswith("chain"):
        n = int(name[5:])
        return problems.reaction_chain(n, 67, seed=n), (0.01, 0.02, 0.03)
    if name.startswith("bruss"):
        return problems.bruss1d_network(int(name[5:]), 9), (0.05, 0.1)
    if name == "enzyme8":
        return problems.enzyme_chain(8, 9), (0.01, 0.02, 0.03)
    raise KeyError(name)


def ref_module(p):
    return RL if "nconst" in p else MA


def case(name, **kw):
    """(problem, touts, the reference run): computed once per process, shared and left unchanged"""
    if name == "law5":
        return RL.case("n5", **kw)
    key = (name,) + tuple(sorted((k, tuple(v) if hasattr(v, "__len__") else v) for k, v in kw.items()))
    if key not in _CACHE:
        p, touts = _problem(name)
        _CACHE[key] = (p, touts, ref_module(p).run(p, touts, **kw))
    return _CACHE[key]


def ended_well(name, ref):
    c = ref["counters"]
    assert (ref["status"] == 0).all() and (c["nni"][-1] > c["nst"][-1]).all(), name


def open_ens(ctx, p, tiny):
    """an ensemble on the ctx with the switch as asked, and the stepper that will really run asserted"""
    import idahip
    ctx.set_mass_action_tiny(tiny)
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    assert ens.device_controller_active() == (1 if tiny else 0)
    return ens


def integrate(p, touts, tiny=True, prepare=None):
    from idahip import problems
    ctx = problems.make_ctx(p)
    if prepare:
        prepare(ctx)
    ens = open_ens(ctx, p, tiny)
    out = []
    for t in touts:
        st, tret = ens.solve(float(t))
        out.append((st.copy(), tret.copy(), snapshot(ens)))
    ens.close()
    ctx.close()
    return out


def rows(ref, ids):
    """the reference run of the listed systems alone (a system's integration does not depend on its neighbours)"""
    out = {k: ref[k][:, ids] for k in ("status", "tret", "yy", "yp", "kused", "hused", "tn")}
    out["counters"] = {k: v[:, ids] for k, v in ref["counters"].items()}
    return out


# ------------------------------------------------------------------------------------------------ 1. the switch and the refusals
def test_switch_and_refusals():
    import idahip
    from idahip import problems
    p = problems.roberts_network()
    ctx = problems.make_ctx(p)
    assert ctx.mass_action_tiny() is False
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    assert ens.device_controller_active() == 0  # the default: the host stepper, as before there was a switch
    ctx.set_mass_action_tiny()
    assert ctx.mass_action_tiny() is True and ens.device_controller_active() == 1  # (read anew: the ensemble exists already)
    ctx.set_mass_action_tiny(False)
    assert ctx.mass_action_tiny() is False and ens.device_controller_active() == 0
    # idahip_tiny_solve itself, the switch off: refused as every ctx that is not Roberts or Lorenz63 is (on: sections 2 to 8)
    st, touts, rounds, acc = np.zeros(4096, dtype=np.uint8), np.array([0.4]), np.zeros(1, dtype=np.int64), np.zeros(2, dtype=np.uint64)
    call = TinyCall(touts.ctypes.data, 1, 0, 0, 0, 500, 5, 10, 10, 0.33, 0.0, 0.0, None, 0, 0, None, None, None)
    fn = ctx.H.idahip_tiny_solve
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    args = (C.byref(call), rounds.ctypes.data, acc.ctypes.data, None, None)
    assert fn(ctx.h, st.ctypes.data, 8, *args) == -2  # (the size of the controller record: the library's text names it)
    size = int(re.search(r"expects (\d+)", ctx.H.idahip_last_error(ctx.h).decode()).group(1))
    assert 8 < size <= st.size
    assert fn(ctx.h, st.ctypes.data, size, *args) == -2
    assert "takes the Roberts and Lorenz63 problems" in ctx.H.idahip_last_error(ctx.h).decode()
    ens.close()
    ctx.close()
    # the setter's refusals: -2, a text, nothing changed
    heat = idahip.Ctx("heat1d", 16, 2)
    with pytest.raises(idahip.IdaHipError, match=r"\(-2\).*not an IDAHIP_MASS_ACTION ctx"):
        heat.set_mass_action_tiny()
    assert heat.mass_action_tiny() is False
    heat.close()
    nine = idahip.Ctx("mass_action", 9, 2)
    with pytest.raises(idahip.IdaHipError, match=r"\(-2\).*n = 9.*n <= 8"):
        nine.set_mass_action_tiny()
    assert nine.mass_action_tiny() is False
    nine.close()
    # before the network is set: the switch is taken, and creating an ensemble still answers "not set"
    bare = idahip.Ctx("mass_action", 3, 1)
    bare.set_tolerances(p["rtol"], p["atol"])
    bare.set_mass_action_tiny()
    assert bare.mass_action_tiny() is True
    with pytest.raises(idahip.IdaHipError, match=r"\(-2\).*not set \(idahip_set_mass_action\)"):
        idahip.Ensemble(bare, p["yy0"], p["yp0"])
    bare.set_mass_action(p["reactions"], p["d"])
    bare.set_problem_params(p["params"])
    ens = idahip.Ensemble(bare, p["yy0"], p["yp0"])
    assert ens.device_controller_active() == 1
    st, _ = ens.solve(0.4)
    assert (st == 0).all()
    ens.close()
    bare.close()


# ------------------------------------------------------------------------------------------------ 2. whole integrations
WHOLE = ["roberts", "lorenz", "ab2", "chain6", "chain7", "chain8", "bruss3", "bruss4", "law5", "enzyme8"]


@pytest.mark.parametrize("name", WHOLE)
def test_whole_integrations_equal_the_reference(name):
    p, touts, ref = case(name)
    ended_well(name, ref)
    assert_equals_reference(integrate(p, touts), ref, CNT, name)


@pytest.mark.parametrize("shape", ["B1", "spw1", "spw4", "spw64"])
@pytest.mark.parametrize("name", ["chain7", "enzyme8"])
def test_results_do_not_depend_on_the_launch_shape(name, shape, monkeypatch):
    """one system alone, and the whole batch with 1, 4 and 64 systems per wavefront (IDAHIP_TINY_SPW is read by every call)"""
    p, touts, ref = case(name)
    if shape == "B1":
        ids = [3]
        p, ref = ref_module(p).select(p, ids), rows(ref, ids)
    else:
        monkeypatch.setenv("IDAHIP_TINY_SPW", shape[3:])
    assert_equals_reference(integrate(p, touts), ref, CNT, (name, shape))


# ------------------------------------------------------------------------------------------------ 3. the host stepper, switch off
@pytest.mark.parametrize("name", ["roberts", "chain7", "chain8", "enzyme8"])
def test_the_host_stepper_gives_the_same_bits(name):
    p, touts, ref = case(name)
    assert_equals_reference(integrate(p, touts, tiny=False), ref, CNT, name)


# ------------------------------------------------------------------------------------------------ 4. schedules
def assert_final_state(ens, ref, counters=CNT):
    x = snapshot(ens)
    for k in ("yy", "yp", "hused", "tn"):
        assert same_bits(x[k], ref[k][-1]), k
    assert np.array_equal(x["c"]["kused"], ref["kused"][-1])
    for k in counters:
        assert np.array_equal(x["c"][k], ref["counters"][k][-1]), k


@pytest.mark.parametrize("mode", ["whole", "resumed", "switching"])
def test_solve_schedule(mode):
    """chain7: the schedule in one call with its outputs; cut into calls of 11 rounds; and one round per call with the stepper
    changing from call to call (host, one-thread, host, ...): outputs and final state are the uninterrupted run's, the reference's."""
    from idahip import problems
    p, touts, ref = case("chain7")
    ctx = problems.make_ctx(p)
    ens = open_ens(ctx, p, True)
    if mode == "whole":
        st, tret, reached, yo, ypo = ens.solve_schedule(touts, outputs=True)
        assert (reached == len(touts)).all()
    else:
        yo, ypo = np.full(ref["yy"].shape, np.nan), np.full(ref["yp"].shape, np.nan)
        for i in range(4000):
            if mode == "switching":
                ctx.set_mass_action_tiny(i % 2 == 1)
                assert ens.device_controller_active() == i % 2
            st, tret, reached, y1, yp1 = ens.solve_schedule(touts, max_rounds=11 if mode == "resumed" else 1, outputs=True)
            m = ~np.isnan(y1)
            assert not (m & ~np.isnan(yo)).any()  # an output is handed out once
            yo[m], ypo[m] = y1[m], yp1[m]
            if (st != 99).all():
                break
        assert i > 3, "the schedule ended before it was resumed"
    assert np.array_equal(st, ref["status"][-1]) and same_bits(tret, ref["tret"][-1])
    assert same_bits(yo, ref["yy"]) and same_bits(ypo, ref["yp"])
    assert_final_state(ens, ref)
    ens.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. idaens_stream
def full_state(ens):
    c = ens.counters()
    return {**c, "hused": ens.real("hused"), "hh": ens.real("hh"), "tn": ens.real("tn"), "yy": ens.yy(), "yp": ens.yp()}


def assert_same_state(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        if np.asarray(a[k]).dtype.kind == "f":
            assert same_bits(a[k], b[k]), (what, k)
        else:
            assert np.array_equal(a[k], b[k]), (what, k)


def pair(p, prepare=None):
    """the same problem on two contexts: (ctx, ensemble on the one-thread stepper), (ctx, ensemble on the host stepper)"""
    from idahip import problems
    out = []
    for tiny in (True, False):
        ctx = problems.make_ctx(p)
        if prepare:
            prepare(ctx)
        out.append((ctx, open_ens(ctx, p, tiny)))
    return out


def close(pr):
    for ctx, ens in pr:
        ens.close()
        ctx.close()


@pytest.mark.parametrize("name", ["roberts", "chain8"])
def test_stream_equals_the_host_stepper(name):
    """finished systems restart at once, staggered first starts: same totals and states as the host stepper's stream"""
    p, touts, _ = case(name)
    if name == "chain8":
        p = MA.select(p, range(9))
    (cd, dev), (ch, host) = pr = pair(p)
    for k, stag in ((150, 40), (1, 0), (1, 0), (77, 0)):
        pd, ph = dev.stream(touts, k, stagger_rounds=stag), host.stream(touts, k, stagger_rounds=stag)
        assert pd == ph
        assert dev.total_rounds() == host.total_rounds() and dev.total_newton_iters() == host.total_newton_iters()
        assert_same_state(full_state(dev), full_state(host), (name, k))
    assert pd > 0
    close(pr)


# ------------------------------------------------------------------------------------------------ 6. DQ Jacobians
@pytest.mark.parametrize("name,n", [("chain7dq", 7), ("enzyme8dq", 8)])
def test_dq_integration(name, n):
    p, touts, ref = case(name, dq=True)
    ended_well(name, ref)
    c = ref["counters"]
    assert np.array_equal(c["nre_dq"][-1], n * c["nje"][-1]) and (c["nje"][-1] > 0).all()
    run = integrate(p, touts, prepare=lambda ctx: ctx.set_jacobian_dq(True))
    assert_equals_reference(run, ref, CNT + ("nre_dq",), name)


# ------------------------------------------------------------------------------------------------ 7. constraints
def census_of(ref):
    return {k: sum(c[k] for c in ref["census"]) for k in ref["census"][0]}


def lorenz_constrained(c):
    from idahip import problems
    key = ("lorenz5",) + tuple(c)
    if key not in _CACHE:
        p = problems.lorenz63_network(5)
        touts = (1.0, 5.0)
        _CACHE[key] = (p, touts, MA.run(p, touts, constr=np.array(c)))
    return _CACHE[key]


def test_constraints_correct_recover_and_fail():
    """Lorenz63 with y0 >= 0: the trajectory wants to cross, the check corrects and recovers until the step budget of each call is
    spent (TOO_MUCH_WORK for every system at both outputs)"""
    c = (1.0, 0.0, 0.0)
    p, touts, ref = lorenz_constrained(c)
    census = census_of(ref)
    assert census["corrected"] > 0 and census["recovered"] > 0, census
    assert (ref["status"] == -1).all()
    run = integrate(p, touts, prepare=lambda ctx: ctx.set_constraints(np.array(c)))
    assert_equals_reference(run, ref, CNT, "lorenz y0 >= 0")


def test_constraints_violated_at_the_start():
    c = (0.0, -1.0, 0.0)
    p, touts, ref = lorenz_constrained(c)
    assert (ref["status"] == -22).all()
    run = integrate(p, touts, prepare=lambda ctx: ctx.set_constraints(np.array(c)))
    assert_equals_reference(run, ref, CNT, "lorenz y1 <= 0")


def test_constraints_on_roberts_over_twelve_decades():
    from idahip import problems
    p = problems.roberts_network()
    p["rtol"], p["atol"] = 1e-2, np.array([1e-6, 1e-4, 1e-4])
    touts = tuple(0.4 * 10.0 ** k for k in range(12))
    assert touts[-1] == 4e10
    ref = MA.run(p, touts, constr=np.ones(3))
    census = census_of(ref)
    assert (ref["status"] == 0).all() and census["corrected"] > 0, census
    run = integrate(p, touts, prepare=lambda ctx: ctx.set_constraints(np.ones(3)))
    assert_equals_reference(run, ref, CNT, "roberts constrained")


def test_dq_with_constraints_stays_refused():
    import idahip
    from idahip import problems
    p = roberts_batch(5)
    ctx = problems.make_ctx(p)
    ctx.set_constraints(np.ones(3))
    ctx.set_jacobian_dq(True)
    ens = open_ens(ctx, p, True)
    with pytest.raises(idahip.IdaHipError, match=r"difference-quotient"):
        ens.solve(0.4)
    ens.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------ 8. against the host stepper
def both(p, script, prepare=None):
    """script(ctx, ens) -> records, on the one-thread stepper and on the host stepper: the same records and the same state after"""
    (cd, dev), (ch, host) = pr = pair(p, prepare)
    rd, rh = script(cd, dev), script(ch, host)
    assert dev.device_controller_active() == 1 and host.device_controller_active() == 0
    assert len(rd) == len(rh)
    for i, (a, b) in enumerate(zip(rd, rh)):
        assert_same_state(a, b, i)
    assert_same_state(full_state(dev), full_state(host), "end")
    close(pr)
    return rh


def record(ens, st, tret, **more):
    return {"status": st.copy(), "tret": tret.copy(), **full_state(ens), **more}


def test_roots_with_a_continued_solve():
    """the reference example's two functions on the Roberts network: every return with its rootsfound, and the calls after it"""
    def script(ctx, ens):
        ens.set_roots([0, 2], [1e-4, 0.01])
        rec = []
        for t in (0.4, 4.0, 40.0):
            for _ in range(20):
                st, tret = ens.solve(t)
                rec.append(record(ens, st, tret, roots=ens.roots_found().copy()))
                assert (st >= 0).all()
                if (st == 0).all():
                    break
            else:
                raise AssertionError("no end of root returns")
        return rec

    rec = both(roberts_batch(5), script)
    assert any((r["status"] == 2).any() for r in rec), "no root return in this run"
    assert (rec[-1]["nge"] > 0).all()


def test_a_stop_time_inside_the_horizon():
    def script(ctx, ens):
        ens.set_stop_time(np.array([0.1, np.nan, 0.25, 0.4, 1.0]))
        rec = []
        for t in (0.4, 0.4, 4.0):
            st, tret = ens.solve(t)
            rec.append(record(ens, st, tret))
        return rec

    rec = both(roberts_batch(5), script)
    assert (rec[0]["status"] == 1).sum() >= 2 and (rec[0]["status"] == 0).any()


def test_suppress_alg():
    def prepare(ctx):
        ctx.set_id(np.array([1.0, 1.0, 0.0]))
        ctx.set_suppress_alg(1)

    def script(ctx, ens):
        return [record(ens, *ens.solve(t)) for t in (0.4, 4.0, 40.0)]

    p = roberts_batch(5)
    masked = both(p, script, prepare)
    assert (masked[-1]["status"] == 0).all()
    plain = integrate(p, (0.4, 4.0, 40.0))
    assert not same_bits(masked[-1]["hused"], plain[-1][2]["hused"]), "the masked norms changed nothing: the mask is not under test"


def test_a_tout_behind_t0():
    from idahip import problems
    p = MA.select(problems.lorenz63_network(9), range(9))

    def script(ctx, ens):
        return [record(ens, *ens.solve(t)) for t in (-0.05, -0.1)]

    rec = both(p, script)
    assert (rec[-1]["status"] == 0).all() and (rec[-1]["tn"] < 0.0).all() and (rec[-1]["hused"] < 0.0).all()


def test_reinit_of_a_strict_subset():
    p, _, ref = case("chain8")
    p = MA.select(p, range(9))
    listed = np.array([6, 1, 4], dtype=np.int32)

    def script(ctx, ens):
        rec = [record(ens, *ens.solve(0.01))]
        ens.reinit(listed, 0.005, p["yy0"][listed], p["yp0"][listed])
        rec.append(record(ens, *ens.solve(0.02)))
        rec.append(record(ens, *ens.solve(0.03)))
        return rec

    rec = both(p, script)
    assert (rec[-1]["status"] == 0).all()
    # the systems off the list are the uninterrupted run's, bit for bit; the listed ones started over at t0 = 0.005 and are not
    off = np.setdiff1d(np.arange(9), listed)
    for i in range(3):
        assert same_bits(rec[i]["yy"][off], ref["yy"][i][off]) and np.array_equal(rec[i]["nst"][off], ref["counters"]["nst"][i][off]), i
    assert same_bits(rec[0]["yy"], ref["yy"][0][:9])
    for i in (1, 2):
        assert all(not same_bits(rec[i]["yy"][s], ref["yy"][i][s]) for s in listed), i


def test_calc_ic_then_a_solve():
    import idahip
    p = roberts_batch(5)
    p["yy0"] = p["yy0"].copy()
    p["yy0"][:, 2] += 0.01 * (1.0 + np.arange(5))
    p["yp0"] = np.zeros((5, 3))

    def script(ctx, ens):
        st = ens.calc_ic(idahip.YA_YDP_INIT, 0.4)
        rec = [record(ens, st, np.zeros(5))]
        return rec + [record(ens, *ens.solve(t)) for t in (0.4, 4.0)]

    rec = both(p, script, lambda ctx: ctx.set_id(np.array([1.0, 1.0, 0.0])))
    assert (rec[0]["status"] == 0).all() and (rec[-1]["status"] == 0).all()


def test_a_step_limit_some_systems_reach():
    """reaction_chain(8), nine systems, to t = 3e-5 with at most 20 steps a call: the unlimited reference needs 17 to 24 steps there,
    so the systems that need fewer than 20 finish in the first call and those that need more than 20 end it in TOO_MUCH_WORK and
    go on in the second"""
    from idahip import problems
    p = problems.reaction_chain(8, 9, seed=8)
    tout = 3e-5
    need = MA.run(p, (tout,))["counters"]["nst"][-1]
    assert (need < 20).any() and (need > 20).any(), need

    def script(ctx, ens):
        ens.set_max_num_steps(20)
        return [record(ens, *ens.solve(t)) for t in (tout, tout, 1e-4)]

    rec = both(p, script)
    assert (rec[0]["status"][need < 20] == 0).all() and (rec[0]["status"][need > 20] == -1).all(), (rec[0]["status"], need)
    assert (rec[1]["status"] == 0).all() and np.array_equal(rec[1]["nst"], need), (rec[1]["status"], rec[1]["nst"], need)
