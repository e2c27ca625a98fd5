"""IDAReInit for listed systems of a running ensemble: idahip_reinit (the device entry point and its kernel), idaens_reinit /
idaens_reinit_at_return on all three steppers, and idaens_calc_ic_systems.

  1. idahip_reinit on uploaded state, every field against numpy, every list shape, add = 0 / 1 and the null sides, the snapshot's rows,
     -0.0 and NaN payloads, the frame's protocol;
  2. event runs against the oracle (tests/reinit_oracle.py; the census of these runs is tests/test_reinit_oracle.py's): after every
     root return a jump through reinit_at_return, or through reinit with host arrays at t0 = tret + 0.25;
  3. no influence: a system that is never reinitialised equals its run on an ensemble where reinit is never called;
  4. fresh equivalence on the forms the oracle does not cover: a system reinitialised at t0 = 0 with the problem's own values equals a
     fresh ensemble's at every output, all counters included; idaens_stream after a reinit;
  5. a dead system comes back;
  6. idaens_calc_ic_systems against tests/calcic_ref.py;
  7. the refusals.
Everything is bit for bit (stepper_ref.same_bits; NaN payloads through the integer view) except a band ctx against the oracle's dense
solver, where yy / yp are compared by value as tests/test_gpu_bruss.py does. There is no tolerance in this file.
"""
import numpy as np
import pytest

import reinit_oracle as RI
import roots_cases as RC
import stepper_ref as R
import tstop_oracle as T

pytestmark = pytest.mark.gpu

F_YY, F_YP, F_YYPREDICT, F_YPPREDICT, F_EWT, F_EE, F_DELTA, F_SAVRES, F_PHI0 = range(9)
ALL_FIELDS = list(range(F_PHI0)) + [F_PHI0 + j for j in range(6)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_exact(a, b):
    """bit for bit, NaN payloads and signs included"""
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def all_fields(ctx):
    return {f: ctx.download(f) for f in ALL_FIELDS}


# ------------------------------------------------------------------------------------------------ 1. idahip_reinit directly
def rng(*key):
    return np.random.Generator(np.random.PCG64([7] + list(key)))


def special(a, g):
    """-0.0 and quiet NaNs with a payload at a few places"""
    a = a.copy()
    flat = a.reshape(-1)
    k = g.choice(flat.size, size=min(4, flat.size), replace=False)
    flat[k[0]] = -0.0
    if k.size > 1:
        flat[k[1:2]] = np.array([0x7FF8000000001234], dtype=np.int64).view(np.float64)
    if k.size > 2:
        flat[k[2:3]] = np.array([-0x0008000000000ABC], dtype=np.int64).view(np.float64)  # sign bit set, quiet, payload
    return a


def lists_of(B):
    out = {"whole": np.arange(B, dtype=np.int32), "single": np.array([B // 2], dtype=np.int32), "empty": np.zeros(0, dtype=np.int32)}
    if B > 2:
        out["subset"] = rng(B).permutation(B)[: max(2, B // 2)].astype(np.int32)
    return out


def make_direct_ctx(form, n, B):
    import idahip
    if form == "dense":
        return idahip.Ctx("linear_dense", n, B)
    if form == "band":
        return idahip.Ctx("heat1d", n, B, band=(1, 1))
    return idahip.Ctx("heat1d", n, B, krylov=0)


def check_reinit(form, n, B, snap):
    import idahip
    ctx = make_direct_ctx(form, n, B)
    g = rng(n, B, int(snap))
    try:
        for lname, idx in lists_of(B).items():
            for mode in ("set", "add", "add_y_null", "add_yp_null", "add_both_null"):
                for f in ALL_FIELDS:
                    ctx.upload(f, special(g.standard_normal((B, n)), g))
                if snap:
                    ctx.snapshot_initial()
                    ctx.upload(F_PHI0, g.standard_normal((B, n)))
                    ctx.upload(F_PHI0 + 1, g.standard_normal((B, n)))
                before = all_fields(ctx)
                if snap:  # the snapshot's rows are read through restore_initial on a copy of the state: put the state back after
                    ctx.restore_initial()
                    snap0, snap1 = ctx.download(F_PHI0), ctx.download(F_PHI0 + 1)
                    for f in ALL_FIELDS:
                        ctx.upload(f, before[f])
                y = special(g.standard_normal((idx.size, n)), g) if idx.size else np.zeros((0, n))
                yp = special(g.standard_normal((idx.size, n)), g) if idx.size else np.zeros((0, n))
                if mode != "set":  # NaN payloads pass through the copies; the additions are checked on numbers and signed zeros
                    y, yp = np.nan_to_num(y, nan=-0.0), np.nan_to_num(yp, nan=-0.0)
                    for f in (F_YY, F_YP):
                        before[f] = np.nan_to_num(before[f], nan=-0.0)
                        ctx.upload(f, before[f])
                a_y = None if mode in ("add_y_null", "add_both_null") else y
                a_yp = None if mode in ("add_yp_null", "add_both_null") else yp
                want = {f: v.copy() for f, v in before.items()}
                if mode == "set":
                    new_y, new_yp = y, yp
                else:
                    new_y = before[F_YY][idx] if a_y is None else before[F_YY][idx] + y
                    new_yp = before[F_YP][idx] if a_yp is None else before[F_YP][idx] + yp
                want[F_YY][idx], want[F_PHI0][idx] = new_y, new_y
                want[F_YP][idx], want[F_PHI0 + 1][idx] = new_yp, new_yp
                for j in range(2, 6):
                    want[F_PHI0 + j][idx] = 0.0
                ctx.reinit(idx, a_y, a_yp, add=mode != "set")
                got = all_fields(ctx)
                for f in ALL_FIELDS:
                    assert same_exact(got[f], want[f]), (form, n, B, snap, lname, mode, "field", f)
                if snap:
                    ctx.restore_initial()
                    w0, w1 = snap0.copy(), snap1.copy()
                    w0[idx], w1[idx] = new_y, new_yp
                    assert same_exact(ctx.download(F_PHI0), w0) and same_exact(ctx.download(F_PHI0 + 1), w1), (form, n, B, lname, mode)
                else:  # no snapshot has been taken, and reinit takes none
                    with pytest.raises(idahip.IdaHipError, match="before idahip_snapshot_initial"):
                        ctx.restore_initial()
    finally:
        ctx.close()


@pytest.mark.parametrize("snap", [False, True], ids=["nosnap", "snap"])
@pytest.mark.parametrize("B", [1, 5, 67])
@pytest.mark.parametrize("n", [3, 9, 65, 300])
def test_reinit_kernel_dense(n, B, snap):
    check_reinit("dense", n, B, snap)


@pytest.mark.parametrize("snap", [False, True], ids=["nosnap", "snap"])
@pytest.mark.parametrize("form", ["band", "krylov"])
def test_reinit_kernel_band_and_krylov(form, snap):
    check_reinit(form, 16, 5, snap)


def test_reinit_passes_nan_payloads_of_the_state_through():
    """add = 1 with a null side takes yy / yp as they are: payloads and a -0.0 included."""
    import idahip
    n, B = 9, 5
    ctx = idahip.Ctx("linear_dense", n, B)
    g = rng(99)
    yy, yp = special(g.standard_normal((B, n)), g), special(g.standard_normal((B, n)), g)
    ctx.upload(F_YY, yy)
    ctx.upload(F_YP, yp)
    ctx.reinit(None, None, None, add=True)
    assert same_exact(ctx.download(F_PHI0), yy) and same_exact(ctx.download(F_PHI0 + 1), yp)
    assert same_exact(ctx.download(F_YY), yy) and same_exact(ctx.download(F_YP), yp)
    assert np.isnan(yy).any() and np.signbit(yy[yy == 0.0]).any()
    ctx.close()


def test_reinit_frame_protocol():
    import ctypes as C
    import idahip
    n, B = 9, 4
    ctx = idahip.Ctx("linear_dense", n, B)
    g = rng(5)
    for f in ALL_FIELDS:
        ctx.upload(f, g.standard_normal((B, n)))
    before = all_fields(ctx)
    H, h = ctx.H, ctx.h
    i32p, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    y = np.ones((B, n))

    def call(idx, nsys, yy, yp, add):
        a = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
        rc = H.idahip_reinit(h, None if a is None else a.ctypes.data_as(i32p), nsys, None if yy is None else yy.ctypes.data_as(dp),
                             None if yp is None else yp.ctypes.data_as(dp), add)
        return [rc, H.idahip_last_error(h).decode()]

    assert call(None, 2, y, y, 0) == [-2, "null system list"]
    assert call([0, 4], 2, y, y, 0) == [-2, "system id 4 out of range at list position 1"]
    assert call([0, -1], 2, y, y, 0) == [-2, "system id -1 out of range at list position 1"]
    assert call([1, 1], 2, y, y, 0) == [-2, "system id 1 listed twice (again at list position 1)"]
    assert call([0, 1, 2, 3, 0], 5, y, y, 0) == [-2, "nsys = 5 out of range (batch = 4)"]
    assert call([0], -1, y, y, 0) == [-2, "nsys = -1 out of range (batch = 4)"]
    assert call([2, 0], 2, None, y, 0) == [-2, "null argument"]
    assert call([2, 0], 2, y, None, 0) == [-2, "null argument"]
    assert call([1, 1], 2, None, y, 0)[1].startswith("system id 1 listed twice")  # the list's refusal wins
    t0 = ctx.timing_get()
    assert call(None, 0, y, y, 0)[0] == 0 and call([3], 0, None, None, 1)[0] == 0  # an empty list launches nothing
    assert ctx.timing_get() == t0
    got = all_fields(ctx)
    for f in ALL_FIELDS:
        assert same_exact(got[f], before[f]), f
    assert call([2, 0], 2, None, None, 1)[0] == 0
    t1 = ctx.timing_get()
    assert t1["vector"]["launches"] == t0["vector"]["launches"] + 1 and t1["vector"]["systems"] == t0["vector"]["systems"] + 2
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. event runs against the oracle
EVENT_CASES = [("lorenz", False), ("roberts", False), ("linear24", False), ("heat20", False), ("heat20", True)]
STEPPERS = ["host_plain", "host_fused", "device"]
_REPLAYS = {}


def open_case(c, stepper, band=False):
    import idahip
    from idahip import problems
    prob = c["prob"]
    ctx = problems.make_ctx(prob, band=band)
    ens = idahip.Ensemble(ctx, prob["yy0"], prob["yp0"])
    ens.set_device_controller(1 if stepper == "device" else 0)
    if stepper != "device":
        ens.set_fused_newton(stepper == "host_fused")
    ens.set_roots(*c["roots"])
    assert ens.device_controller_active() == (c["stepper"] if stepper == "device" else 0)
    return ctx, ens


def oracle_replay(c, ops, how):
    key = (c["name"], how, repr(ops))
    if key not in _REPLAYS:
        _REPLAYS[key] = RI.replay(c, ops, how=how)
    return _REPLAYS[key]


def event_run(name, band, stepper, how, only=None):
    c = RC.case(name)
    ctx, ens = open_case(c, stepper, band=band)
    d = RI.ProductEvents(c, ens)
    ops = RI.drive_events(c, d, how=how, only=only)
    assert ens.device_controller_active() == (c["stepper"] if stepper == "device" else 0)
    ens.close()
    ctx.close()
    return c, ops, d.rec


@pytest.mark.parametrize("how", ["at_return", "host"])
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("name,band", EVENT_CASES, ids=lambda v: {True: "band", False: "dense"}.get(v, v))
def test_event_runs_equal_the_oracle(name, band, stepper, how):
    c, ops, rec = event_run(name, band, stepper, how)
    assert sum(1 for o in ops if o[0] == "jump") >= 1
    RI.compare(rec, oracle_replay(c, ops, how), by_value=band, what="%s band=%s %s %s" % (name, band, stepper, how))


# ------------------------------------------------------------------------------------------------ 3. no influence
NO_INFLUENCE_KEYS = ("status", "tret", "yy", "yp", "tn", "hh", "hused", "iroots", "nge") + RI.EXTRA_COUNTERS


@pytest.mark.parametrize("stepper", ["host_fused", "device"])
@pytest.mark.parametrize("name,band", EVENT_CASES, ids=lambda v: {True: "band", False: "dense"}.get(v, v))
def test_systems_never_reinitialised_are_not_influenced(name, band, stepper):
    """Only the systems with b % 3 == 0 are ever reinitialised; a twin ensemble makes the same solve calls and no reinit. Every other
    system is the same in both, per call, bit for bit and counter for counter (the solve calls are the same, so nge is too)."""
    import tstop_cases as K
    c, ops, rec = event_run(name, band, stepper, "at_return", only=lambda b: b % 3 == 0)
    assert sum(1 for o in ops if o[0] == "jump") >= 1
    ctx, ens = open_case(c, stepper, band=band)
    d = RI.ProductEvents(c, ens)
    for op in ops:
        if op[0] == "solve":
            d.solve(op[1])
    ens.close()
    ctx.close()
    B = c["prob"]["yy0"].shape[0]
    rest = np.array([b for b in range(B) if b % 3 != 0])
    assert len(d.rec) == len(rec)
    for i, (g, w) in enumerate(zip(rec, d.rec)):
        for k in NO_INFLUENCE_KEYS + K.INT_FIELDS:
            assert R.same_bits(np.asarray(g[k][rest], dtype=np.float64), np.asarray(w[k][rest], dtype=np.float64)), (name, stepper, i, k)


# ------------------------------------------------------------------------------------------------ 4. fresh equivalence
def record(ens, st, tret):
    r = {"status": st.copy(), "tret": tret.copy(), "yy": ens.yy(), "yp": ens.yp()}
    r.update(ens.counters())
    for k in ("tn", "hused", "hh", "h0u", "tolsf"):
        r[k] = ens.real(k)
    return r


def fresh_equivalence(p, make, touts, listed=None, prepare=None, active=None, what=""):
    import idahip
    B = p["yy0"].shape[0]
    listed = np.array([B - 1, 0] if B > 2 else [B - 1], dtype=np.int32) if listed is None else np.asarray(listed, dtype=np.int32)
    assert 0 < listed.size < B
    runs = {}
    for again in (False, True):
        ctx = make()
        ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
        if prepare is not None:
            prepare(ctx, ens)
        if again:
            ens.solve(float(touts[0]))
            ens.reinit(listed, 0.0, p["yy0"][listed], p["yp0"][listed])
        out = []
        for t in touts:
            st, tret = ens.solve(float(t))
            out.append(record(ens, st, tret))
        if active is not None:
            assert ens.device_controller_active() == active, (what, ens.device_controller_active())
        runs[again] = out
        ens.close()
        ctx.close()
    rest = np.array([b for b in range(B) if b not in listed.tolist()])
    all_ok = all((r["status"] == 0).all() for r in runs[False])
    for i, (g, w) in enumerate(zip(runs[True], runs[False])):
        for k in w:
            assert R.same_bits(np.asarray(g[k][listed], dtype=np.float64), np.asarray(w[k][listed], dtype=np.float64)), (what, i, k, g[k], w[k])
            if all_ok and k != "nge":  # the others made one call more (their first tout twice): nothing but a root check differs
                assert R.same_bits(np.asarray(g[k][rest], dtype=np.float64), np.asarray(w[k][rest], dtype=np.float64)), (what, "rest", i, k)
    return runs[False]


def _bruss():
    from idahip import problems
    return problems.bruss1d(m=5, batch=5)


@pytest.mark.parametrize("device_ctl", [0, 1])
@pytest.mark.parametrize("form", ["dense", "band"])
def test_fresh_equivalence_bruss_direct(form, device_ctl):
    from idahip import problems
    p = _bruss()
    fresh_equivalence(p, lambda: problems.make_ctx(p, band=form == "band"), p["touts"],
                      prepare=lambda ctx, ens: ens.set_device_controller(device_ctl), active=2 * device_ctl, what="bruss %s" % form)


@pytest.mark.parametrize("rounds", [0, 1])
def test_fresh_equivalence_bruss_krylov_with_the_band_preconditioner(rounds):
    from idahip import problems
    p = _bruss()

    def make():
        ctx = problems.make_ctx(p, krylov=5)
        ctx.set_krylov_band_prec(2, 2)
        ctx.set_krylov_rounds(bool(rounds))
        return ctx

    ref = fresh_equivalence(p, make, p["touts"], active=2 * rounds, what="bruss krylov rounds=%d" % rounds)
    assert (ref[-1]["npe"] > 0).all() and (ref[-1]["nps"] > 0).all() and (ref[-1]["nli"] > 0).any()


@pytest.mark.parametrize("device_ctl", [0, 1])
@pytest.mark.parametrize("net", ["reaction_chain", "enzyme_chain"])
def test_fresh_equivalence_reaction_networks(net, device_ctl):
    from idahip import problems
    p = problems.reaction_chain(12, 6) if net == "reaction_chain" else problems.enzyme_chain(9, 6)
    fresh_equivalence(p, lambda: problems.make_ctx(p), p["touts"], listed=[4, 1, 5],
                      prepare=lambda ctx, ens: ens.set_device_controller(device_ctl), active=2 * device_ctl, what=net)


def test_fresh_equivalence_dq_ctx():
    from idahip import problems
    p = problems.heat1d(n=16, batch=3)

    def make():
        ctx = problems.make_ctx(p)
        ctx.set_jacobian_dq(True)
        return ctx

    ref = fresh_equivalence(p, make, [0.1, 0.2], what="heat16 dq")
    assert (ref[-1]["nre_dq"] > 0).all()


def test_fresh_equivalence_host_callback_twin():
    import bruss_ref as BR
    from idahip import problems
    p = _bruss()
    tw = BR.twin(p)
    ref = fresh_equivalence(tw, lambda: problems.make_ctx(tw), p["touts"], active=0, what="bruss callback twin")
    assert (ref[-1]["nst"] > 0).all()


@pytest.mark.parametrize("device_ctl", [0, 1])
def test_fresh_equivalence_with_constraints(device_ctl):
    import constr_cases as CC
    from idahip import problems
    cc = CC.lorenz_x_nonneg()
    p = cc["prob"]

    def make():
        ctx = problems.make_ctx(p)
        ctx.set_constraints(cc["c"])
        return ctx

    def prepare(ctx, ens):
        ens.set_device_controller(device_ctl)
        ens.set_max_num_steps(cc["mxstep"])

    ref = fresh_equivalence(p, make, [float(t) for t in cc["touts"]], prepare=prepare, active=device_ctl, what="lorenz x >= 0")
    assert (ref[-1]["ncfn"] > 0).any()


def test_fresh_equivalence_with_a_start_that_violates_the_constraints():
    """the constraints check of y0 belongs to the first-call block: a reinitialised system whose y0 violates them does not start"""
    import constr_cases as CC
    import idahip
    from idahip import problems
    cc = CC.lorenz_x_nonneg()
    p = cc["prob"]
    ctx = problems.make_ctx(p)
    ctx.set_constraints(cc["c"])
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    ens.set_max_num_steps(cc["mxstep"])
    t1 = float(cc["touts"][0])
    ens.solve(t1)
    bad = p["yy0"][[2]].copy()
    bad[0, 0] = -1.0
    ens.reinit([2], 0.25, bad, p["yp0"][[2]])
    before = ens.counters()
    st, tret = ens.solve(0.25 + t1)
    assert st[2] == T.ILL_INPUT and tret[2] == 0.25 and ens.counter("nst")[2] == 0
    assert all(np.array_equal(before[k][2], ens.counters()[k][2]) for k in before)
    ens.close()
    ctx.close()


def test_fresh_equivalence_lu_period_heat1100():
    from idahip import problems
    p = problems.heat1d(n=1100, batch=2)
    fresh_equivalence(p, lambda: problems.make_ctx(p), [0.1, 0.2], listed=[1], prepare=lambda ctx, ens: ctx.set_lu_period(4), active=2,
                      what="heat1100 lu_period 4")


def test_stream_after_a_reinit():
    import idahip
    from idahip import problems
    p = problems.lorenz63(batch=6)
    touts = [0.05, 0.1]
    listed = np.array([4, 1], dtype=np.int32)
    new_y = p["yy0"][listed] * (1.0 + 2.0 ** -20)
    for device_ctl in (0, 1):
        ctx = problems.make_ctx(p)
        ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
        ens.set_device_controller(device_ctl)
        ens.solve(touts[0])
        ens.reinit(listed, 0.5, new_y, p["yp0"][listed])
        with pytest.raises(idahip.IdaHipError, match=r"\(-2\).*idaens_stream does not combine with a start time of a system's own \(system 1 "):
            ens.stream(touts, 4)
        ens.reinit(listed, 0.0, new_y, p["yp0"][listed])
        assert ens.stream(touts, 200) >= 1
        ens.close()
        ctx.restore_initial()  # what the restarts began from: the new values for the listed systems
        want = p["yy0"].copy()
        want[listed] = new_y
        assert same_exact(ctx.download(F_PHI0), want) and same_exact(ctx.download(F_PHI0 + 1), p["yp0"])
        ctx.close()


# ------------------------------------------------------------------------------------------------ 5. a dead system comes back
@pytest.mark.parametrize("device_ctl", [0, 1])
def test_a_dead_system_comes_back(device_ctl):
    """tests/failure_recipes.py's first_terminal recipe: y'(0) = 0 and a first tout of 100 end systems 1 and 3 with ERR_FAIL (-3) before
    their first step; with mxstep = 50 the others return TOO_MUCH_WORK (-1, which the next call continues) after 50 steps of every
    call. The dead ones, reinitialised with the problem's own y0, y0', integrate: after the third call every system equals the oracle
    harness -- the dead ones a harness on the good values that has made one call, the others a harness that has made all three, as if
    nothing had been called in between."""
    import failure_recipes as F
    import idahip
    from idahip import problems
    dead, mxstep = [3, 1], 50
    case = F.first_step_case("linear_dense", 24, 1.0e2, expect="first_terminal", edited=dead)
    p = case["prob"]
    B = p["yy0"].shape[0]
    good = problems.linear_dense(n=24, batch=B, procs=1)
    ctx = problems.make_ctx(p)
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    ens.set_device_controller(device_ctl)
    ens.set_max_num_steps(mxstep)
    assert ens.device_controller_active() == 2 * device_ctl
    tout = case["after"][0]
    st, _ = ens.solve(tout)
    assert (st[dead] == -3).all() and (np.delete(st, dead) == T.TOO_MUCH_WORK).all(), st
    st2, _ = ens.solve(tout)
    assert np.array_equal(st2, st) and (ens.counter("nst")[dead] == 0).all()  # sticky
    ens.reinit(dead, 0.0, good["yy0"][dead], good["yp0"][dead])
    c = ens.counters()
    assert all((c[k][dead] == 0).all() for k in c)
    st3, tret3 = ens.solve(tout)
    after = record(ens, st3, tret3)
    ens.close()
    ctx.close()
    assert (st3 == T.TOO_MUCH_WORK).all() and (after["nst"][dead] == mxstep).all() and (np.delete(after["nst"], dead) == 3 * mxstep).all(), st3
    for b in range(B):
        h = RI.Harness(good, b, roots=([], []), mxstep=mxstep)  # (no root function: the harness reads no rootsfound)
        for _ in range(1 if b in dead else 3):
            hst, htret = h.solve(tout)
        s = h.state()
        assert hst == st3[b] and htret == tret3[b], (b, hst, st3[b], htret, tret3[b])
        assert R.same_bits(after["yy"][b], s["yy"]) and R.same_bits(after["yp"][b], s["yp"]), b
        for k in T.SCALARS + RI.EXTRA_COUNTERS:
            assert float(after[k][b]) == s[k], (b, k, after[k][b], s[k])


# ------------------------------------------------------------------------------------------------ 6. calc_ic_systems
IC_COUNTERS = ("nre", "nsetups", "nje", "nni", "ncfn", "nbacktr", "nre_dq")


def check_calc_ic_systems(p, id_, probs_at, t1, listed, move):
    """probs_at(b, t0) -> calcic_ref.Problem of system b at t0; move(yy) -> the reported yy with differential components changed."""
    import calcic_ref as IC
    import idahip
    from idahip import problems
    listed = np.asarray(listed, dtype=np.int32)
    B = p["yy0"].shape[0]
    ctx = problems.make_ctx(p)
    ctx.set_id(id_)
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    st, tret = ens.solve(t1)
    assert (st == 0).all()
    yy, yp = ens.yy(), ens.yp()
    new_y = move(yy[listed])
    ens.reinit(listed, tret[listed], new_y, yp[listed])
    tout1 = tret[listed] + t1 * (1.0 + np.arange(listed.size))
    before = all_fields(ctx)
    cnt0 = ens.counters()
    status = ens.calc_ic_systems(idahip.YA_YDP_INIT, listed, tout1)
    after = all_fields(ctx)
    cnt = ens.counters()
    rest = np.array([b for b in range(B) if b not in listed.tolist()])
    for f in ALL_FIELDS:  # a running system's every field, phi included
        assert same_exact(after[f][rest], before[f][rest]), ("field", f)
    for k in cnt:
        assert np.array_equal(cnt[k][rest], cnt0[k][rest]), k
    moved = False
    for q, b in enumerate(listed):
        ref = IC.calc_ic(probs_at(int(b), float(tret[b])), new_y[q], yp[b], p["rtol"], p["atol"], IC.YA_YDP_INIT, float(tout1[q]), id=id_,
                         t0=float(tret[b]))
        assert status[q] == ref["status"] == 0, (b, status[q], ref["status"])
        assert R.same_bits(after[F_YY][b], ref["yy"]) and R.same_bits(after[F_YP][b], ref["yp"]), b
        assert same_exact(after[F_PHI0][b], after[F_YY][b]) and same_exact(after[F_PHI0 + 1][b], after[F_YP][b])
        for j in range(2, 6):
            assert not after[F_PHI0 + j][b].any() and not np.signbit(after[F_PHI0 + j][b]).any()
        for k in IC_COUNTERS:
            assert cnt[k][b] == ref["counters"][k], (b, k, cnt[k][b], ref["counters"][k])
        moved = moved or not same_exact(after[F_YY][b], new_y[q])
    assert moved
    # the corrected systems step on from their t0, the others from where they were
    st2, tret2 = ens.solve(float(tret.max()) + 8.0 * t1)
    assert (st2 == 0).all() and (ens.counter("nst")[listed] > 0).all()
    # refusal: a started system in the list; nothing changed
    snap = all_fields(ctx)
    with pytest.raises(idahip.IdaHipError, match=r"\(-2\).*idaens_calc_ic_systems: system %d has started" % listed[0]):
        ens.calc_ic_systems(idahip.YA_YDP_INIT, listed, tout1 + 10.0)
    now = all_fields(ctx)
    assert all(same_exact(now[f], snap[f]) for f in ALL_FIELDS)
    with pytest.raises(idahip.IdaHipError, match="idaens_calc_ic: only before the first solve, solve_schedule or stream call"):
        ens.calc_ic(idahip.YA_YDP_INIT, 1.0)
    ens.close()
    ctx.close()


def test_calc_ic_systems_roberts():
    import calcic_ref as IC
    import tstop_cases as K
    p = K.roberts_batch(16)

    def move(yy):
        out = yy.copy()
        out[:, 0] *= 0.9  # y0 and y1 are differential (id = 1, 1, 0): y2 and the derivatives are then inconsistent
        out[:, 1] *= 1.5
        return out

    check_calc_ic_systems(p, np.array([1.0, 1.0, 0.0]), lambda b, t0: IC.device_problem("roberts", 3, {}, t0=t0), 0.4, [9, 2, 5], move)


def test_calc_ic_systems_reaction_chain():
    import calcic_ref as IC
    import massaction_ref as MA
    from idahip import problems
    n = 12
    p = problems.reaction_chain(n, 6)
    net = MA.Net(p)

    def probs_at(b, t0):
        return IC.Problem(n, MA.prob_res(p, b), lambda cj, y, ypv, rr, hic, ewt: MA.jac(net, p["params"][b], cj, y))

    def move(yy):
        out = yy.copy()
        out[:, 0] += 0.5  # a dose of the hub species: the conservation row (the last, algebraic) no longer holds
        out[:, 3] *= 0.5
        return out

    check_calc_ic_systems(p, p["d"].copy(), probs_at, 0.01, [4, 0, 3], move)


def test_calc_ic_systems_refusals():
    import constr_cases as CC
    import idahip
    import tstop_cases as K
    from idahip import problems
    p = K.roberts_batch(4)
    ctx = problems.make_ctx(p)
    ctx.set_id([1.0, 1.0, 0.0])
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    ens.solve(0.4)
    ens.reinit([1], 0.4, p["yy0"][[1]], p["yp0"][[1]])
    ctx.set_constraints([1.0, 1.0, 1.0])
    with pytest.raises(idahip.IdaHipError, match=r"\(-2\).*idaens_calc_ic_systems: a ctx with constraints is not supported"):
        ens.calc_ic_systems(idahip.YA_YDP_INIT, [1], 0.8)
    ctx.set_constraints(None)
    ctx.set_suppress_alg(True)
    with pytest.raises(idahip.IdaHipError, match=r"\(-2\).*idaens_calc_ic_systems: not with suppress_alg on"):
        ens.calc_ic_systems(idahip.YA_YDP_INIT, [1], 0.8)
    ctx.set_suppress_alg(False)
    with pytest.raises(idahip.IdaHipError, match=r"\(-2\).*idaens_calc_ic_systems: system id 1 listed twice"):
        ens.calc_ic_systems(idahip.YA_YDP_INIT, [1, 1], 0.8)
    with pytest.raises(idahip.IdaHipError, match=r"\(-2\).*idaens_calc_ic_systems: system id 4 out of range"):
        ens.calc_ic_systems(idahip.YA_YDP_INIT, [4], 0.8)
    with pytest.raises(idahip.IdaHipError, match=r"\(-2\).*idaens_calc_ic_systems: unknown icopt 7"):
        ens.calc_ic_systems(7, [1], 0.8)
    st = ens.calc_ic_systems(idahip.YA_YDP_INIT, [1], 0.4)  # tout1 == t0: ILL_INPUT for the system, not a refusal of the call
    assert st.tolist() == [T.ILL_INPUT]
    assert ens.calc_ic_systems(idahip.YA_YDP_INIT, [1], 0.8).tolist() == [0]
    ens.close()
    ctx.close()
    hp = problems.heat1d(n=16, batch=3)
    ctx = problems.make_ctx(hp, krylov=5)
    ens = idahip.Ensemble(ctx, hp["yy0"], hp["yp0"])
    with pytest.raises(idahip.IdaHipError, match=r"\(-2\).*idaens_calc_ic_systems: a Krylov ctx is not supported"):
        ens.calc_ic_systems(idahip.Y_INIT, [0], 0.1)
    ens.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------ 7. the refusals of reinit
def test_reinit_refusals():
    import idahip
    from idahip import problems
    p = problems.linear_dense(n=24, batch=5, procs=1)
    for device_ctl in (0, 1):
        ctx = problems.make_ctx(p)
        ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
        ens.set_device_controller(device_ctl)
        y, yp = p["yy0"], p["yp0"]

        def unchanged(snap):
            now = (all_fields(ctx), ens.counters(), {k: ens.real(k) for k in ("tn", "hh", "hused", "h0u", "tolsf")})
            return (all(same_exact(now[0][f], snap[0][f]) for f in ALL_FIELDS) and all(np.array_equal(now[1][k], snap[1][k]) for k in snap[1])
                    and all(same_exact(now[2][k], snap[2][k]) for k in snap[2]))

        def state():
            return (all_fields(ctx), ens.counters(), {k: ens.real(k) for k in ("tn", "hh", "hused", "h0u", "tolsf")})

        s0 = state()
        with pytest.raises(idahip.IdaHipError, match="idaens_reinit_at_return: system 3 has not returned from a solve call"):
            ens.reinit_at_return([0, 3][::-1])
        assert unchanged(s0)
        st, _ = ens.solve(0.1, max_rounds=2)
        assert (st == 99).all()
        s1 = state()
        with pytest.raises(idahip.IdaHipError, match=r"idaens_reinit: system 2 is inside a round-limited call \(IDAENS_UNFINISHED\)"):
            ens.reinit([2], 0.0, y[[2]], yp[[2]])
        with pytest.raises(idahip.IdaHipError, match=r"idaens_reinit_at_return: system 2 is inside a round-limited call"):
            ens.reinit_at_return([2])
        assert unchanged(s1)
        st, _ = ens.solve(0.1)
        assert (st == 0).all()
        s2 = state()
        for bad in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(idahip.IdaHipError, match="idaens_reinit: the t0 of system 4 is not finite"):
                ens.reinit([1, 4], [0.0, bad], y[[1, 4]], yp[[1, 4]])
        with pytest.raises(idahip.IdaHipError, match="idaens_reinit: system id 5 out of range at list position 1"):
            ens.reinit([1, 5], 0.0, y[[1, 4]], yp[[1, 4]])
        with pytest.raises(idahip.IdaHipError, match="listed twice"):
            ens.reinit([1, 1], 0.0, y[[1, 1]], yp[[1, 1]])
        assert unchanged(s2)
        ens.reinit_at_return([4, 0])  # no jump at all: the systems restart where they are
        assert (ens.counter("nst")[[0, 4]] == 0).all() and (ens.real("tn")[[0, 4]] == 0.1).all() and ens.counter("nst")[1] > 0
        with pytest.raises(idahip.IdaHipError, match="idaens_reinit_at_return: system 4 has not returned"):
            ens.reinit_at_return([4])
        st, tret = ens.solve(0.2)
        assert (st == 0).all() and (tret == 0.2).all()
        ens.close()
        ctx.close()
