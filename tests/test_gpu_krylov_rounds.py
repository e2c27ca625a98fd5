"""A Krylov ctx on the device lock-step rounds (idahip_set_krylov_rounds, off by default; DESIGN.md section 4h/4i addendum): the switch
and its refusals; whole integrations against the restated stepper (tests/krylov_ref.py) bit for bit; the band preconditioner
against the host stepper on a twin ctx (and tests/krylov_prec_ref.py where it has the case); schedules, round-limited calls, the
stepper switched between them, streams; root functions, stop times, masked norms and maxord; n = 4096; a group of two contexts.
Bit for bit means view(np.uint64) equality. Every run asserts device_controller_active() before it is trusted."""
import ctypes as C

import numpy as np
import pytest

import krylov_cases as K
import krylov_prec_ref as PR

pytestmark = pytest.mark.gpu
MAXL = PR.STEP_MAXL
UNFINISHED = 99


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def heat_problem(n, batch, kappa0, touts=(0.002, 0.004, 0.006)):
    """krylov_cases.step_problem's heat family for any n and batch: kappa_b = kappa0 (1 + b mod 11). kappa0 = 0.02, B = 6 is
    krylov_cases.step_problem itself, kappa0 = 0.5, n = 65, B = 6 is krylov_prec_ref.step_problem."""
    from idahip import problems
    p = problems.heat1d(n=n, batch=batch)
    kappa = kappa0 * (1.0 + np.arange(batch) % 11)
    dx = 1.0 / (n - 1)
    coef = kappa / (dx * dx)
    y = p["yy0"][0]
    p["params"] = coef.reshape(batch, 1)
    p["yp0"][:] = 0.0
    p["yp0"][:, 1:-1] = coef[:, None] * ((y[None, :-2] - 2.0 * y[None, 1:-1]) + y[None, 2:])
    p["touts"] = np.asarray(touts, dtype=np.float64)
    return p


def bruss_problem(n, batch=6):
    from idahip import problems
    p = problems.bruss1d(m=n // 2, batch=batch)
    p["touts"] = np.array([0.25, 0.5])
    return p


def open_ens(p, width, rounds, maxl=MAXL, stream=None, before_create=None):
    """-> (ctx, ens) on a Krylov ctx with the band preconditioner `width` (None: plain) and the device rounds on or off."""
    import idahip
    from idahip import problems
    ctx = problems.make_ctx(p, krylov=maxl, stream=stream)
    if width is not None:
        ctx.set_krylov_band_prec(*width)
    assert not ctx.krylov_rounds()  # off by default
    ctx.set_krylov_rounds(rounds)
    assert ctx.krylov_rounds() == bool(rounds)
    if before_create:
        before_create(ctx)
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    assert ens.device_controller_active() == (2 if rounds else 0)
    return ctx, ens


def state(ens):
    return {**ens.counters(), "hused": ens.real("hused"), "hh": ens.real("hh"), "tn": ens.real("tn"), "yy": ens.yy(), "yp": ens.yp()}


def same(a, b, what=""):
    for k in a:
        if a[k].dtype == np.float64:
            assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)
        else:
            assert np.array_equal(a[k], b[k]), (what, k, a[k], b[k])


def close(*objs):
    for o in objs:
        o.close()


# ------------------------------------------------------------------------------------------------ 1. the switch and its refusals
def test_switch_and_refusals():
    import idahip
    from idahip import problems
    H, _ = idahip.load()
    P = C.CDLL(idahip.LIB_HIP)  # a handle of this test's own for the nine-pointer call
    P.idahip_round_solve.argtypes = [C.c_void_p] * 9
    assert H.idahip_krylov_rounds(None) == -1
    heat = heat_problem(16, 3, 0.02)
    for p in (heat, bruss_problem(10, 3), K.step_problem("linear_dense", 12)):
        ctx = problems.make_ctx(p, krylov=MAXL)
        ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
        # off by default: the host stepper, and the refusal of idahip_round_solve launches nothing
        assert H.idahip_krylov_rounds(ctx.h) == 0 and ens.device_controller_active() == 0
        before = ctx.timing_get()
        assert P.idahip_round_solve(ctx.h, None, 0, None, None, None, None, None, None) == -2
        assert "idahip_round_solve" in H.idahip_last_error(ctx.h).decode()
        assert ctx.timing_get() == before
        ctx.set_krylov_rounds(True)
        assert H.idahip_krylov_rounds(ctx.h) == 1 and ens.device_controller_active() == 2
        ens.set_device_controller(0)
        assert ens.device_controller_active() == 0
        ens.set_device_controller(1)
        assert ens.device_controller_active() == 2
        ctx.set_krylov_rounds(False)
        assert H.idahip_krylov_rounds(ctx.h) == 0 and ens.device_controller_active() == 0
        close(ens, ctx)
    # root functions: a user callback and more than four of the built-in family stay on the host stepper
    ctx = problems.make_ctx(heat, krylov=MAXL)
    ctx.set_krylov_rounds(True)
    e1 = idahip.Ensemble(ctx, heat["yy0"], heat["yp0"])
    e1.set_roots([1, 2], [0.5, 0.5])
    assert e1.device_controller_active() == 2
    e1.set_roots([1, 2, 3, 4, 5], [0.5] * 5)
    assert e1.device_controller_active() == 0
    e1.set_root_fn(1, lambda s, t, yy, yp: [yy[1] - 0.5])
    assert e1.device_controller_active() == 0
    close(e1, ctx)
    # the setter on a ctx that cannot have the rounds
    dense, band = problems.make_ctx(heat), problems.make_ctx(heat, band=True)
    host = idahip.Ctx("host_callback", 16, 3, krylov=MAXL)
    for other in (dense, band, host):
        assert H.idahip_set_krylov_rounds(other.h, 1) == -2
        assert "idahip_set_krylov_rounds" in H.idahip_last_error(other.h).decode()
        assert H.idahip_krylov_rounds(other.h) == 0
        assert H.idahip_set_krylov_rounds(other.h, 0) == -2
        other.close()


# ------------------------------------------------------------------------------------------------ 2. against the restated stepper
STEP_CNT = ("nst", "nre", "nre_dq", "nsetups", "nje", "nni", "nli", "ncfl", "ncfn", "netf")


@pytest.mark.parametrize("kind,n,maxl", K.STEP_CASES, ids=lambda v: str(v))
def test_rounds_against_the_restated_stepper(kind, n, maxl):
    """Per system and at every output: status, tret, every counter, kused, hused, tn, yy, yp -- bit for bit against krylov_ref."""
    p, ref = K.step_reference(kind, n, maxl)
    ctx, ens = open_ens(p, None, True, maxl=maxl)
    for i, t in enumerate(p["touts"]):
        status, tret = ens.solve(float(t))
        assert ens.device_controller_active() == 2
        assert np.array_equal(status, ref["status"][i]), (i, status, ref["status"][i])
        assert np.array_equal(bits(tret), bits(ref["tret"][i]))
        c = ens.counters()
        for k in STEP_CNT:
            assert np.array_equal(c[k], ref["counters"][k][i]), (k, i, c[k], ref["counters"][k][i])
        assert np.array_equal(c["kused"], ref["kused"][i])
        assert np.array_equal(bits(ens.real("hused")), bits(ref["hused"][i])) and np.array_equal(bits(ens.real("tn")), bits(ref["tn"][i]))
        assert np.array_equal(bits(ens.yy()), bits(ref["yy"][i])) and np.array_equal(bits(ens.yp()), bits(ref["yp"][i]))
    if (kind, n) == ("heat1d", 65):  # recovered linear failures: flag != SUCCESS -> ConvergenceRecover -> setup and retry in the next round
        last = ref["counters"]["ncfl"][-1]
        assert (ref["status"] == 0).all() and (last > 0).sum() >= 3 and np.array_equal(ens.counter("ncfl"), last)
    assert not ens.counter("npe").any() and not ens.counter("nps").any()
    close(ens, ctx)


# ------------------------------------------------------------------------------------------------ 3. preconditioned, against the host twin
def prec_problem(kind, n, batch):
    if kind == "bruss1d":
        return bruss_problem(n, batch)
    return heat_problem(n, batch, PR.STEP_KAPPA0, touts=(0.002,) if batch > 100 else (0.002, 0.004, 0.006))


PREC_CASES = [("heat1d", 16, (1, 1), 6), ("heat1d", 16, (2, 3), 6), ("heat1d", 65, (1, 1), 6), ("heat1d", 65, (2, 3), 6),
              ("heat1d", 300, (1, 1), 6), ("heat1d", 300, (2, 3), 6), ("bruss1d", 10, (2, 2), 6), ("bruss1d", 130, (2, 2), 6),
              ("heat1d", 16, (1, 1), 70), ("heat1d", 16, (1, 1), 1100)]


@pytest.mark.parametrize("kind,n,width,batch", PREC_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_preconditioned_rounds_against_the_host_stepper(kind, n, width, batch):
    """Per system, at every output: status, tret, yy, yp, tn, hused, hh and every counter equal those of the host stepper on a twin ctx,
    bit for bit (the number of rounds may differ); the per-class system counts of the timing interface too."""
    p = prec_problem(kind, n, batch)
    cd, dev = open_ens(p, width, True)
    ch, host = open_ens(p, width, False)
    ref = None
    if (kind, n, width, batch) == ("heat1d", PR.STEP_N, PR.STEP_WIDTH, K.STEP_B):  # the case krylov_prec_ref has
        pr, ref = PR.step_reference()
        assert np.array_equal(pr["params"], p["params"]) and np.array_equal(pr["yp0"], p["yp0"]) and np.array_equal(pr["touts"], p["touts"])
    for i, t in enumerate(p["touts"]):
        sd, td = dev.solve(float(t))
        sh, th = host.solve(float(t))
        assert dev.device_controller_active() == 2 and host.device_controller_active() == 0
        assert np.array_equal(sd, sh) and np.array_equal(bits(td), bits(th)), (i, sd, sh)
        same(state(dev), state(host), "output %d" % i)
        if ref is not None:  # by value, as tests/test_gpu_krylov_prec.py compares the host stepper
            assert np.array_equal(sd, ref["status"][i]) and np.array_equal(td, ref["tret"][i])
            c = dev.counters()
            for k in STEP_CNT + ("npe", "nps"):
                assert np.array_equal(c[k], ref["counters"][k][i]), (k, i)
            assert np.array_equal(c["kused"], ref["kused"][i]) and np.array_equal(dev.real("hused"), ref["hused"][i])
            assert np.array_equal(dev.yy(), ref["yy"][i]) and np.array_equal(dev.yp(), ref["yp"][i])
    c = host.counters()
    assert c["npe"].sum() > 0 and c["nps"].sum() > 0 and c["nli"].sum() > 0, "the branches under test did not run"
    assert (sh == 0).all()
    # systems actually served, per class, as the host stepper's calls book them
    td_, th_ = cd.timing_get(), ch.timing_get()
    for k in ("newton_iter", "sys", "jac", "lu"):
        assert td_[k]["systems"] == th_[k]["systems"], (k, td_[k], th_[k])
    assert td_["newton_iter"]["systems"] == c["nni"].sum() and td_["jac"]["systems"] == c["npe"].sum() and td_["sys_jac"]["systems"] == 0
    # the ready flags: the stand-alone psolve runs on the factors the rounds have left, and they are the host twin's
    if batch <= 70:
        r = np.linspace(-1.0, 1.0, batch * n).reshape(batch, n)
        assert np.array_equal(bits(cd.krylov_psolve(r)), bits(ch.krylov_psolve(r)))
    close(dev, host, cd, ch)


def test_singular_preconditioner_is_a_recoverable_setup_failure():
    """A stepper case that reaches lu_info != 0, found on the CPU with krylov_prec_ref: heat n = 17 (odd), (1, 1), system 1 with
    y0 = y0' = 0 and the coefficient -cj/2 for the first step's cj = 1 / (0.001 tout). Perturbing column i alone gives the diagonal
    entry cj inc + 2 coef inc == 0 exactly, and a tridiagonal matrix with a zero interior diagonal is singular for odd n: the first
    psetup reports a zero pivot, the attempt fails like a convergence failure, h shrinks and the next setup succeeds. The solution
    stays zero and the pattern repeats, so the branch runs again and again until mxstep (60) ends both calls."""
    n, B, width, mxstep = 17, 3, (1, 1), 60
    p = heat_problem(n, B, PR.STEP_KAPPA0, touts=(0.002, 0.004))
    cj0 = 1.0 / (0.001 * p["touts"][0])
    p["params"][1, 0] = -(cj0 / 2.0)
    p["yy0"][1] = 0.0
    p["yp0"][1] = 0.0
    ref = PR.run(p, p["touts"], *width, maxl=MAXL, mxstep=mxstep)
    assert ref["counters"]["ncfn"][-1][1] > 10 and (ref["status"][:, 1] == -1).all() and (ref["status"][:, [0, 2]] == 0).all()
    out = []
    for rounds in (True, False):
        ctx, ens = open_ens(p, width, rounds)
        ens.set_max_num_steps(mxstep)
        for i, t in enumerate(p["touts"]):
            status, tret = ens.solve(float(t))
            assert ens.device_controller_active() == (2 if rounds else 0)
            out.append((status, tret, state(ens)))
            if rounds:  # by value against the restated stepper
                assert np.array_equal(status, ref["status"][i]) and np.array_equal(tret, ref["tret"][i])
                for k in STEP_CNT + ("npe", "nps"):
                    assert np.array_equal(out[-1][2][k], ref["counters"][k][i]), (k, i)
                assert np.array_equal(ens.yy(), ref["yy"][i]) and np.array_equal(ens.real("hused"), ref["hused"][i])
        close(ens, ctx)
    for (sd, td, std), (sh, th, sth) in zip(out[:2], out[2:]):
        assert np.array_equal(sd, sh) and np.array_equal(bits(td), bits(th))
        same(std, sth)
    last = out[1][2]
    assert last["nlufail"][1] > 10 and last["nlufail"][1] == last["ncfn"][1] and not last["nlufail"][[0, 2]].any()


# ------------------------------------------------------------------------------------------------ 4. schedules, resume, switching, stream
def sched_problem(width):
    return heat_problem(65, K.STEP_B, 0.02 if width is None else PR.STEP_KAPPA0)


@pytest.mark.parametrize("width", [None, (1, 1)], ids=["plain", "prec11"])
def test_schedule_outputs_and_round_limited_resume(width):
    p = sched_problem(width)
    touts = p["touts"]
    cd, dev = open_ens(p, width, True)
    ch, host = open_ens(p, width, False)
    sd, td, rd, yd, ypd = dev.solve_schedule(touts, outputs=True)
    sh, th, rh, yh, yph = host.solve_schedule(touts, outputs=True)
    assert (sd == 0).all() and np.array_equal(sd, sh) and np.array_equal(rd, rh) and (rd == len(touts)).all()
    assert np.array_equal(bits(yd), bits(yh)) and np.array_equal(bits(ypd), bits(yph)) and np.array_equal(bits(td), bits(th))
    same(state(dev), state(host))
    cs, sl = open_ens(p, width, True)
    ys = np.full_like(yd, np.nan)
    calls = 0
    for _ in range(1000):
        s, t, r, yo, ypo = sl.solve_schedule(touts, max_rounds=7, outputs=True)
        calls += 1
        m = ~np.isnan(yo)
        ys[m] = yo[m]
        if (s != UNFINISHED).all():
            break
    assert calls > 2 and (s == 0).all() and np.array_equal(bits(ys), bits(yd))
    same(state(sl), state(dev))
    close(dev, host, sl, cd, ch, cs)


@pytest.mark.parametrize("first_on_device", [True, False], ids=["device_first", "host_first"])
@pytest.mark.parametrize("width", [None, (1, 1)], ids=["plain", "prec11"])
def test_switching_steppers_between_round_limited_calls(width, first_on_device):
    """One round per call, the stepper alternating from call to call -- by idahip_set_krylov_rounds in one direction of the
    parametrisation, by idaens_set_device_controller in the other -- against the device rounds run alone. The plain case has Newton
    solves that start over after a linear failure (newton_retry): the host stepper's next call continues such an attempt."""
    p = sched_problem(width)
    touts = p["touts"]
    cd, dev = open_ens(p, width, True)
    sd, td, rd, yd, ypd = dev.solve_schedule(touts, outputs=True)
    assert (sd == 0).all()
    if width is None:
        assert dev.counter("ncfl").sum() > 0, "no Newton solve started over: the hand-over is not exercised"
    cm, mix = open_ens(p, width, True)
    ym = np.full_like(yd, np.nan)
    for i in range(4000):
        on_device = (i % 2 == 0) == first_on_device
        if first_on_device:
            cm.set_krylov_rounds(on_device)
        else:
            mix.set_device_controller(1 if on_device else 0)
        assert mix.device_controller_active() == (2 if on_device else 0)
        s, t, r, yo, ypo = mix.solve_schedule(touts, max_rounds=1, outputs=True)
        m = ~np.isnan(yo)
        ym[m] = yo[m]
        if (s != UNFINISHED).all():
            break
    assert i > 10 and (s == 0).all() and np.array_equal(bits(ym), bits(yd))
    same(state(mix), state(dev))
    close(dev, mix, cd, cm)


@pytest.mark.parametrize("width", [None, (1, 1)], ids=["plain", "prec11"])
def test_stream_with_a_stagger(width):
    """idaens_stream on the rounds (no synchronisation inside) against the host stepper: the same number of rounds; the same passes,
    totals and states as long as no Newton solve had to start over (that costs the device a round). The counters kept outside the
    record restart with their system: npe == nsetups and nps == nni + nli hold for the running pass of every system."""
    p = sched_problem(width)
    touts = p["touts"]
    cd, dev = open_ens(p, width, True)
    ch, host = open_ens(p, width, False)
    compared = 0
    for k, stag in ((60, 18), (1, 0), (45, 0)):
        pd = dev.stream(touts, k, stagger_rounds=stag)
        ph = host.stream(touts, k, stagger_rounds=stag)
        assert dev.device_controller_active() == 2 and host.device_controller_active() == 0
        assert dev.total_rounds() == host.total_rounds()
        c = dev.counters()
        if width is not None:
            assert np.array_equal(c["npe"], c["nsetups"]) and np.array_equal(c["nps"], c["nni"] + c["nli"])
        else:
            assert not c["npe"].any() and not c["nps"].any()
        if (host.counter("nls_nconvfails") == 0).all() and host.total_newton_iters() == dev.total_newton_iters():
            assert pd == ph
            same(state(dev), state(host))
            compared += 1
    assert pd > 0, "no system was created anew"
    if width is not None:
        assert compared > 0 and c["npe"].sum() > 0
    close(dev, host, cd, ch)


# ------------------------------------------------------------------------------------------------ 5. options that ride on the flow
def run_twins(p, width, touts, before_create=None, after_create=None):
    """The same calls on the rounds and on the host twin -> [(status, tret, state, roots)] per call, compared bit for bit."""
    out = []
    for rounds in (True, False):
        ctx, ens = open_ens(p, width, rounds, before_create=before_create)
        if after_create:
            after_create(ens)
        assert ens.device_controller_active() == (2 if rounds else 0)
        calls = []
        for t in touts:
            status, tret = ens.solve(float(t))
            calls.append((status, tret, state(ens), ens.roots_found()))
        out.append(calls)
        close(ens, ctx)
    for i, ((sd, td, std, rd), (sh, th, sth, rh)) in enumerate(zip(*out)):
        assert np.array_equal(sd, sh) and np.array_equal(bits(td), bits(th)) and np.array_equal(rd, rh), (i, sd, sh)
        same(std, sth, "call %d" % i)
    return out[0]


def test_two_root_functions():
    p = heat_problem(65, K.STEP_B, PR.STEP_KAPPA0)
    calls = run_twins(p, (1, 1), [0.002, 0.002, 0.004], after_create=lambda e: e.set_roots([32, 16], [0.995, 0.70]))
    assert (calls[0][0] == 2).any() and calls[0][3].any(), "no root was found"  # IDAENS_ROOT_RETURN


def test_stop_time_per_system_with_one_nan():
    p = heat_problem(65, K.STEP_B, PR.STEP_KAPPA0)
    ts = np.array([0.0011, 0.0015, np.nan, 0.0013, 0.0019, 0.0017])
    calls = run_twins(p, (1, 1), [0.002, 0.004], after_create=lambda e: e.set_stop_time(ts))
    status, tret = calls[0][0], calls[0][1]
    has = ~np.isnan(ts)
    assert (status[has] == 1).all() and np.array_equal(bits(tret[has]), bits(ts[has])) and status[2] == 0  # TSTOP_RETURN at tstop


def test_suppress_alg_with_the_id_vector():
    n = 16
    p = heat_problem(n, K.STEP_B, PR.STEP_KAPPA0)
    id_ = np.ones(n)
    id_[0] = id_[-1] = 0.0

    def masked(ctx):
        ctx.set_id(id_)
        ctx.set_suppress_alg(True)
    calls = run_twins(p, (1, 1), p["touts"], before_create=masked)
    assert (calls[-1][0] == 0).all()


def test_max_ord_two():
    p = heat_problem(65, K.STEP_B, PR.STEP_KAPPA0)
    calls = run_twins(p, (1, 1), p["touts"], after_create=lambda e: e.set_max_ord(2))
    assert (calls[-1][0] == 0).all() and (calls[-1][2]["kused"] <= 2).all()


# ------------------------------------------------------------------------------------------------ 6. the LDS limit
def test_heat_4096_six_rounds():
    """n = 4096 with (1, 1), B = 2: the largest LDS requests of the round (the fused solve's 3 n doubles, begin / end's 4 n + 8). Six
    rounds on either stepper; with the preconditioner no Newton solve starts over, so six rounds are six attempts on both: asserted,
    then every counter and the whole state are compared."""
    from idahip import problems
    p = problems.heat1d(n=4096, batch=2)
    cd, dev = open_ens(p, (1, 1), True)
    ch, host = open_ens(p, (1, 1), False)
    sd, td = dev.solve(0.01, max_rounds=6)
    sh, th = host.solve(0.01, max_rounds=6)
    assert dev.device_controller_active() == 2
    assert np.array_equal(dev.counter("n_attempts"), host.counter("n_attempts")) and (dev.counter("n_attempts") == 6).all()
    assert np.array_equal(dev.counter("nst"), host.counter("nst")) and (dev.counter("nst") > 0).all()
    assert np.array_equal(sd, sh) and np.array_equal(bits(td), bits(th))
    same(state(dev), state(host))
    # (the (1, 1) preconditioner is the heat Jacobian itself up to the difference quotients: these first solves return without an iteration)
    assert dev.counter("npe").sum() > 0 and dev.counter("nps").sum() > 0
    close(dev, host, cd, ch)


def test_heat_4096_plain_to_an_early_tout():
    """The same size without the preconditioner, where the solver's loop runs (nli > 0): equal attempts cannot be arranged by a round
    limit here (a linear failure costs the device a round), so both steppers run one call to a very early tout, at most 40 steps."""
    from idahip import problems
    p = problems.heat1d(n=4096, batch=2)
    cd, dev = open_ens(p, None, True)
    ch, host = open_ens(p, None, False)
    for e in (dev, host):
        e.set_max_num_steps(40)
    sd, td = dev.solve(1.0e-6)
    sh, th = host.solve(1.0e-6)
    assert dev.device_controller_active() == 2
    assert np.array_equal(sd, sh) and np.array_equal(bits(td), bits(th)), (sd, sh)
    same(state(dev), state(host))
    assert host.counter("nli").sum() > 0 and (host.counter("nst") > 0).all()
    close(dev, host, cd, ch)


# ------------------------------------------------------------------------------------------------ 7. a group of two contexts
def test_group_of_two_krylov_contexts():
    """idaens_solve_schedule_group with two Krylov contexts (one plain, one preconditioned) on their own streams, the rounds on: the
    per-system results of each alone."""
    import idahip
    n = 16
    probs = [heat_problem(n, K.STEP_B, 0.02), heat_problem(n, K.STEP_B, PR.STEP_KAPPA0)]
    widths = [None, (1, 1)]
    touts = probs[0]["touts"]
    streams, _ = idahip.concurrent_streams(2)
    side = [open_ens(p, w, True, stream=s) for p, w, s in zip(probs, widths, streams)]
    alone = [open_ens(p, w, True) for p, w in zip(probs, widths)]
    res = idahip.solve_schedule_group([e for _, e in side], touts)
    for (_, a), (_, b), r in zip(side, alone, res):
        st, tr, re_ = b.solve_schedule(touts)
        assert a.device_controller_active() == 2
        assert (st == 0).all() and np.array_equal(r[0], st) and np.array_equal(bits(r[1]), bits(tr)) and np.array_equal(r[2], re_)
        same(state(a), state(b))
    assert side[1][1].counter("npe").sum() > 0 and side[0][1].counter("nli").sum() > 0
    for c, e in side + alone:
        close(e, c)
    idahip.release_streams(streams)
