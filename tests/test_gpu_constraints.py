"""Inequality constraints (DESIGN.md section 4g, C IDA's IDASetConstraints) on the device against tests/constr_ref.py:
  * idahip_post_newton_constr / idahip_constr_check against the numpy restatement, bit for bit, at every launch shape;
  * the host stepper and the one-thread-per-system device stepper on the cases of tests/constr_cases.py (whose census
    tests/test_constr_ref.py takes on the CPU) against the reference loop: statuses, tret, yy / yp after every call, every counter,
    kused, hused, hh, tn, the failures before the first step and the trace -- bit for bit on a dense ctx, by value on a band ctx;
  * the refusals (difference-quotient Jacobians, calc_ic, bad values) and the fallback of n > 8 to the host stepper."""
import ctypes as C

import numpy as np
import pytest

import constr_cases as K
import constr_ref as CR

pytestmark = pytest.mark.gpu

CYCLE = np.array([0.0, 1.0, -1.0, 2.0, -2.0])
KINDS = ("clean", "corrected", "recovering", "unchecked", "only_first", "only_last")
FIELDS = ("yy", "yp", "yypredict", "yppredict", "ewt", "ee")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ the kernels
def constraint_vector(n):
    c = CYCLE[(np.arange(n) + 1) % 5]  # c_0 = 1
    if c[n - 1] == 0.0:
        c[n - 1] = -2.0
    return c


def make_state(rng, n, c, kind):
    """One system's vectors such that yy = yypredict + ee is: feasible (clean); infeasible by 1e-9 in a few components (corrected);
    infeasible by 5 in every third constrained component (recovering, unchecked); infeasible at i = 0 only, by 5 (only_first);
    infeasible at i = n - 1 only, by 1e-9 (only_last). phi[0] is feasible throughout, as the start check guarantees."""
    sgn = np.where(c != 0.0, np.sign(c), rng.choice([-1.0, 1.0], size=n))
    yy = sgn * rng.uniform(0.5, 2.0, n)
    con = np.flatnonzero(c != 0.0)
    if kind == "corrected":
        pick = con[:: max(1, con.size // 3)][:3]
        yy[pick] = -sgn[pick] * 1e-9
    elif kind in ("recovering", "unchecked"):
        pick = con[::3]
        yy[pick] = -sgn[pick] * 5.0
    elif kind == "only_first":
        yy[0] = -sgn[0] * 5.0
    elif kind == "only_last":
        yy[n - 1] = -sgn[n - 1] * 1e-9
    yypredict = rng.uniform(-2.0, 2.0, n)
    st = {"yypredict": yypredict, "yppredict": rng.uniform(-2.0, 2.0, n), "ee": yy - yypredict,
          "ewt": rng.uniform(0.5, 50.0, n), "yy": rng.uniform(-1, 1, n), "yp": rng.uniform(-1, 1, n)}
    phi = rng.uniform(-0.1, 0.1, (6, n))
    phi[0] = sgn * rng.uniform(0.5, 2.0, n)
    return st, phi


def upload_state(ctx, states, phis):
    import idahip
    fid = {"yy": idahip.F_YY, "yp": idahip.F_YP, "yypredict": idahip.F_YYPREDICT, "yppredict": idahip.F_YPPREDICT, "ewt": idahip.F_EWT,
           "ee": idahip.F_EE}
    for k in FIELDS:
        ctx.upload(fid[k], np.stack([s[k] for s in states]))
    for j in range(6):
        ctx.upload(idahip.F_PHI0 + j, np.stack([p[j] for p in phis]))


def download_state(ctx):
    import idahip
    fid = {"yy": idahip.F_YY, "yp": idahip.F_YP, "yypredict": idahip.F_YYPREDICT, "yppredict": idahip.F_YPPREDICT, "ewt": idahip.F_EWT,
           "ee": idahip.F_EE}
    out = {k: ctx.download(fid[k]) for k in FIELDS}
    out["phi"] = np.stack([ctx.download(idahip.F_PHI0 + j) for j in range(6)])
    return out


@pytest.mark.parametrize("n", [3, 24, 200, 704, 4096])
def test_post_newton_constr_and_constr_check_equal_the_restatement(n):
    """n = 3 / 24: less than a wavefront; 200: less than the workgroup; 704: several passes of the workgroup; 4096: the LDS limit (the
    four sums reuse the buffer of the correction's norm). Batch 5 (3 at n = 4096), a strict sub-list in permuted order, kk = 1, 2, 3, 5
    (every combination of norms), c cycling through 1, -1, 2, -2, 0, and the listed systems in turn clean, corrected, recovering,
    unchecked, violated at i = 0 only, violated at i = n - 1 only."""
    import idahip
    batch = 3 if n == 4096 else 5
    idx = np.array([2, 0] if batch == 3 else [3, 0, 4, 1], dtype=np.int32)
    c = constraint_vector(n)
    eps_newt = 0.33
    ctx = idahip.Ctx("lorenz63", 3, batch) if n == 3 else idahip.Ctx("heat1d", n, batch)
    ctx.set_tolerances(1e-6, np.array([1e-8]))
    ctx.set_constraints(c)
    assert same_bits(ctx.constraints(), c)
    rng = np.random.Generator(np.random.PCG64(4000 + n))
    seen = set()
    for r, kk in enumerate((1, 2, 3, 5)):
        kinds = ["clean"] * batch
        for q, b in enumerate(idx):
            kinds[b] = KINDS[(len(idx) * r + q) % len(KINDS)]
        seen.update(kinds[b] for b in idx)
        made = [make_state(rng, n, c, kinds[b]) for b in range(batch)]
        states, phis = [m[0] for m in made], [m[1] for m in made]
        cj = rng.uniform(0.5, 20.0, len(idx))
        check = np.array([0 if kinds[b] == "unchecked" else 1 for b in idx], dtype=np.int32)
        upload_state(ctx, states, phis)
        before = download_state(ctx)
        assert not ctx.constr_check(idahip.F_PHI0).any()
        norms, flag, rr = ctx.post_newton_constr(cj, kk, eps_newt, check, idx=idx)
        after = download_state(ctx)
        viol_yy = ctx.constr_check(idahip.F_YY, idx=idx)
        for q, b in enumerate(idx):
            s = states[b]
            yy, yp, ee, nrm, fl, rr_ref = CR.post_newton_constr(s["yypredict"], s["yppredict"], s["ee"], s["ewt"], phis[b], cj[q], kk, c,
                                                                  eps_newt, check[q])
            print("n", n, "kk", kk, "system", b, kinds[b], "flag", flag[q], fl, "rr", rr[q], rr_ref, "norms", norms[q], nrm)
            assert flag[q] == fl == {"clean": 0, "corrected": 1, "recovering": 2, "unchecked": 0, "only_first": 2, "only_last": 1}[kinds[b]]
            assert same_bits(rr[q], rr_ref) and same_bits(norms[q], nrm)
            assert same_bits(after["yy"][b], yy) and same_bits(after["yp"][b], yp) and same_bits(after["ee"][b], ee)
            assert viol_yy[q] == int(CR.violated(c, yy).any())
            for k in ("yypredict", "yppredict", "ewt"):
                assert same_bits(after[k][b], before[k][b])
            assert same_bits(after["phi"][:, b], before["phi"][:, b])
            if kinds[b] == "corrected":
                assert (bits(ee) != bits(s["ee"])).sum() == CR.violated(c, yy).sum() > 0
        for b in set(range(batch)) - set(idx.tolist()):  # systems outside the list
            for k in before:
                assert same_bits(after[k][b] if k != "phi" else after[k][:, b], before[k][b] if k != "phi" else before[k][:, b]), (k, b)
        # clean and unchecked systems: idahip_post_newton's results, bit for bit
        plain = [q for q, b in enumerate(idx) if kinds[b] in ("clean", "unchecked")]
        if plain:
            upload_state(ctx, states, phis)
            pn = ctx.post_newton(cj[plain], kk, idx=idx[plain])
            again = download_state(ctx)
            for j, q in enumerate(plain):
                b = idx[q]
                assert same_bits(pn[j], norms[q])
                for k in ("yy", "yp", "ee"):
                    assert same_bits(again[k][b], after[k][b])
    assert seen == set(KINDS)
    ctx.close()


# ------------------------------------------------------------------------------------------------ the steppers
def open_case(case, device_ctl, band=False, callbacks=None, constrained=True):
    import idahip
    from idahip import problems
    prob = case["prob"] if callbacks is None else dict(case["prob"], kind="host_callback", res=callbacks[0], jac=callbacks[1])
    ctx = problems.make_ctx(prob, band=band)
    if constrained:
        ctx.set_constraints(case["c"])
    ens = idahip.Ensemble(ctx, prob["yy0"], prob["yp0"])
    ens.set_device_controller(device_ctl)
    ens.set_max_num_steps(case["mxstep"])
    return ctx, ens


def run_calls(ens, touts, itask=0):
    rec = []
    for t in touts:
        st, tret = ens.solve(float(t), itask=itask)
        rec.append((st.copy(), tret.copy(), ens.yy(), ens.yp()))
    return rec


def equals_reference(rec, ens, ref, by_value=False, ids=None):
    """The product's returns and state against constr_ref.run's; ids: the systems of the batch the reference holds."""
    eq = np.array_equal if by_value else same_bits
    sel = slice(None) if ids is None else list(ids)
    for i, (st, tret, yy, yp) in enumerate(rec):
        print("call", i, "status", st[sel], "reference", ref["status"][i])
        assert np.array_equal(st[sel], ref["status"][i]), (i, st[sel], ref["status"][i])
        assert same_bits(tret[sel], ref["tret"][i]), (i, tret[sel], ref["tret"][i])
        assert eq(yy[sel], ref["yy"][i]) and eq(yp[sel], ref["yp"][i]), i
    c = ens.counters()
    for k in CR.CNT:
        assert np.array_equal(c[k][sel], ref["counters"][k]), (k, c[k][sel], ref["counters"][k])
    assert np.array_equal(c["kused"][sel], ref["kused"]) and np.array_equal(c["nfail_first"][sel], ref["nfail_first"])
    for k in ("hused", "hh", "tn"):
        assert same_bits(ens.real(k)[sel], ref[k]), k
    assert np.array_equal((c["nlufail"] + c["nconv_jcur"])[sel] + np.array([x["recovered"] for x in ref["census"]]), ref["counters"]["ncfn"])


def product_state(ens):
    c = ens.counters()
    return {**c, "hused": ens.real("hused"), "hh": ens.real("hh"), "tn": ens.real("tn"), "yy": ens.yy(), "yp": ens.yp()}


def same_state(a, b):
    for k in a:
        assert same_bits(a[k], b[k]) if a[k].dtype == np.float64 else np.array_equal(a[k], b[k]), k


def host_case(name, **how):
    case, ref = K.reference(name)
    ctx, ens = open_case(case, 0, **how)
    assert ens.device_controller_active() == 0
    rec = run_calls(ens, case["touts"])
    equals_reference(rec, ens, ref, by_value=bool(how.get("band")))
    ens.close()
    ctx.close()
    return case, ref


@pytest.mark.parametrize("name", sorted(K.HOST_CASES))
def test_host_stepper_equals_the_reference_on_every_case_of_the_census(name):
    """linear_dense n = 24 (batch 5) and n = 200 (batch 4), heat1d n = 40, Roberts and Lorenz63 on the lock-step host stepper."""
    host_case(name)


@pytest.mark.parametrize("name", ["heat_nonneg", "heat_positive"])
def test_host_stepper_on_a_band_ctx(name):
    host_case(name, band=True)


def roberts_callbacks():
    def res(sys, t, y, yp):
        r0 = -0.04 * y[0] + 1.0e4 * y[1] * y[2]
        r1 = -r0 - 3.0e7 * y[1] * y[1] - yp[1]
        r0 -= yp[0]
        return [r0, r1, y[0] + y[1] + y[2] - 1.0]

    def jac(sys, t, cj, y, yp, r):
        return [[-0.04 - cj, 1.0e4 * y[2], 1.0e4 * y[1]], [0.04, -1.0e4 * y[2] - 6.0e7 * y[1] - cj, -1.0e4 * y[1]], [1.0, 1.0, 1.0]]

    return res, jac


@pytest.mark.parametrize("name", ["roberts_loose", "roberts_inconsistent"])
def test_host_callbacks_with_constraints(name):
    """Roberts as an IDAHIP_HOST_CALLBACK problem: the check never touches the residual or the Jacobian."""
    host_case(name, callbacks=roberts_callbacks())


def test_trace_one_step_walk_and_schedule_on_the_host_stepper():
    """The per-step trace of a corrected system; IDAENS_ONE_STEP calls; idaens_solve_schedule with outputs."""
    case, ref = K.reference("heat_nonneg")
    ctx, ens = open_case(case, 0)
    ens.trace_system(1)
    rec = run_calls(ens, case["touts"])
    equals_reference(rec, ens, ref)
    assert same_bits(ens.trace(), ref["steps"][1][:, :3]) and ref["census"][1]["corrected"] > 0
    ens.close()
    ctx.close()
    ncalls = 12
    case, walk = K.reference("roberts_loose", None, None, 1, ncalls)
    ctx, ens = open_case(case, 0)
    rec = run_calls(ens, [case["touts"][0]] * ncalls, itask=1)
    equals_reference(rec, ens, walk)
    assert (walk["counters"]["nst"] == ncalls).all()
    ens.close()
    ctx.close()
    case, ref = K.reference("roberts_loose")
    ctx, ens = open_case(case, 0)
    s, t, r, yo, ypo = ens.solve_schedule(case["touts"], outputs=True)
    assert (s == 0).all() and (r == len(case["touts"])).all() and same_bits(t, ref["tret"][-1])
    assert same_bits(yo, ref["yy"]) and same_bits(ypo, ref["yp"])
    for k in CR.CNT:
        assert np.array_equal(ens.counter(k), ref["counters"][k]), k
    ens.close()
    ctx.close()


WAVE_IDS = (0, 1, 3, 4, 63, 64, 127, 128, 129)


@pytest.mark.parametrize("batch", [5, 130])
@pytest.mark.parametrize("name", sorted(K.TINY_CASES))
def test_one_thread_stepper_equals_the_reference_and_the_host_stepper(name, batch):
    """Roberts and Lorenz63 with the whole of Ida::solve on the device, the constraint check compiled in. Batch 130 is more than one
    wavefront at four systems per wavefront; there the reference is computed for nine systems around the wavefront boundaries and the
    host stepper covers the rest."""
    ids = None if batch == 5 else WAVE_IDS
    case, ref = K.reference(name, batch, ids)
    cd, dev = open_case(case, 1)
    assert dev.device_controller_active() == 1
    ch, host = open_case(case, 0)
    rd, rh = run_calls(dev, case["touts"]), run_calls(host, case["touts"])
    for x, y in zip(rd, rh):
        for u, v in zip(x, y):
            assert same_bits(u, v) if u.dtype == np.float64 else np.array_equal(u, v)
    same_state(product_state(dev), product_state(host))
    equals_reference(rd, dev, ref, ids=ids)
    for e in (dev, host):
        e.close()
    for c in (cd, ch):
        c.close()


def test_one_thread_stepper_without_constraints_and_after_clearing_them():
    """The plain kernels next to their constrained twins: an unconstrained Lorenz63 ensemble equals the oracle, and so does one whose
    ctx had constraints that were cleared (NULL) before the first solve; constraints set between two calls hold from the next call."""
    from test_gpu_ensemble import CNT, run_oracle
    case = K.lorenz_x_nonneg(5)
    prob, touts = case["prob"], case["prob"]["touts"][:4]
    want = run_oracle(prob, touts)
    for cleared in (False, True):
        ctx, ens = open_case(case, 1, constrained=cleared)
        if cleared:
            assert ctx.constraints() is not None
            ctx.set_constraints(None)
            assert ctx.constraints() is None
        assert ens.device_controller_active() == 1
        for i, t in enumerate(touts):
            st, _ = ens.solve(float(t))
            assert (st == 0).all() and same_bits(ens.yy(), want["yy"][i]) and same_bits(ens.yp(), want["yp"][i])
        for k in CNT:
            assert np.array_equal(ens.counter(k), want["counters"][k]), k
        if cleared:  # y <= 0 from now on: y is about 5 at t = 0.4, the next attempt fails its check
            ctx.set_constraints(np.array([0.0, -1.0, 0.0]))
            st, _ = ens.solve(float(prob["touts"][5]))
            assert (st == CR.CONSTR_FAIL).all() and (ens.counter("ncfn") - want["counters"]["ncfn"] == 10).all()
        ens.close()
        ctx.close()


def test_stream_on_the_one_thread_stepper_equals_the_host_stepper():
    case = K.roberts_loose(6)
    touts = case["touts"][:3]
    cd, dev = open_case(case, 1)
    ch, host = open_case(case, 0)
    for k, stag in ((90, 12), (1, 0), (45, 0)):
        pd, ph = dev.stream(touts, k, stagger_rounds=stag), host.stream(touts, k, stagger_rounds=stag)
        assert pd == ph and dev.total_rounds() == host.total_rounds() and dev.total_newton_iters() == host.total_newton_iters()
        same_state(product_state(dev), product_state(host))
    assert pd > 0
    for e in (dev, host):
        e.close()
    for c in (cd, ch):
        c.close()


# ------------------------------------------------------------------------------------------------ refusals and fallback
def launches(ctx):
    return sum(v["launches"] for v in ctx.timing_get().values())


def test_refusals_and_the_fallback_to_the_host_stepper():
    import idahip
    from idahip import problems
    # a bad value: -2, and the vector in force stays; NULL clears
    case = K.lorenz_x_nonneg(3)
    ctx, ens = open_case(case, 1)
    bad = np.array([1.0, 0.5, 0.0])
    assert ctx.H.idahip_set_constraints(ctx.h, bad.ctypes.data_as(C.POINTER(C.c_double))) == -2
    with pytest.raises(idahip.IdaHipError):
        ctx.set_constraints([0.0, 3.0, 0.0])
    assert same_bits(ctx.constraints(), case["c"])
    # calc_ic with constraints: refused, nothing launched
    ctx.set_id(np.ones(3))
    n0 = launches(ctx)
    with pytest.raises(idahip.IdaHipError):
        ens.calc_ic(idahip.Y_INIT, 0.1)
    assert launches(ctx) == n0
    # a DQ ctx with constraints: every solve call is refused, nothing launched; without the constraints it runs
    ctx.set_jacobian_dq(True)
    for call in (lambda: ens.solve(0.1), lambda: ens.solve_schedule([0.1, 0.2]), lambda: ens.stream([0.1, 0.2], 5)):
        with pytest.raises(idahip.IdaHipError):
            call()
    assert launches(ctx) == n0 and (ens.counter("n_attempts") == 0).all()
    ctx.set_constraints(None)
    st, _ = ens.solve(0.1)
    assert (st == 0).all() and launches(ctx) > n0
    ens.close()
    ctx.close()
    # the entry points on a ctx without constraints: -2
    ctx = idahip.Ctx("lorenz63", 3, 2)
    with pytest.raises(idahip.IdaHipError):
        ctx.post_newton_constr(1.0, 1, 0.33)
    with pytest.raises(idahip.IdaHipError):
        ctx.constr_check()
    ctx.close()
    # linear_dense n = 24: the device lock-step rounds without constraints, the host stepper with them -- and the reference's results
    case, ref = K.reference("linear_negated_24")
    ctx = problems.make_ctx(case["prob"])
    ens = idahip.Ensemble(ctx, case["prob"]["yy0"], case["prob"]["yp0"])
    assert ens.device_controller_active() == 2
    ctx.set_constraints(case["c"])
    assert ens.device_controller_active() == 0
    equals_reference(run_calls(ens, case["touts"]), ens, ref)
    ens.close()
    ctx.close()
