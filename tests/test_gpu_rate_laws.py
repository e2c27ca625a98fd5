"""A reaction network with rate laws (idahip_set_rate_network: Michaelis-Menten and Hill factors, the LAWS instantiations of
csrc/mass_action.hpp) on the device against tests/ratelaw_ref.py, bit for bit (view(np.uint64) equality: no tolerance appears in this
file): the residual, the analytic and the difference-quotient Jacobian at every launch shape -- n = 5 (host stepper), 9 and 16 (one
wavefront per system), 64 (the last n of that layout), 65 (one workgroup per system); B = 67 (the last workgroup holds 3 of 4
systems), 3 and 5 --, whole integrations on the host stepper, the fused Newton, the device lock-step rounds and a schedule, DQ
integrations, constraints, calc_ic, the host-callback twin, polynomial networks through the new setter, a zero denominator, the
parameters, and the refusals. The network is idahip.problems.enzyme_chain."""
import re

import numpy as np
import pytest

import calcic_ref as IC
import massaction_ref as MA
import ratelaw_ref as RL

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


def entry_state(p, seed):
    import idahip
    B, n = p["yy0"].shape
    rng = np.random.default_rng(seed)
    yypred = p["yy0"] * (1.0 + 1e-3 * rng.standard_normal((B, n)))
    return {idahip.F_YYPREDICT: yypred, idahip.F_YPPREDICT: p["yp0"] + 1e-2 * rng.standard_normal((B, n)),
            idahip.F_EE: 1e-4 * rng.standard_normal((B, n)), idahip.F_EWT: 1.0 / (p["rtol"] * np.abs(yypred) + p["atol"][0]),
            idahip.F_YY: p["yy0"].copy(), idahip.F_YP: p["yp0"].copy(), idahip.F_DELTA: np.zeros((B, n)), idahip.F_SAVRES: np.zeros((B, n))}


def lists(B, seed):
    """the whole batch in order, and a permuted strict subset (the systems off it are skipped)"""
    return [np.arange(B, dtype=np.int32), np.random.default_rng(seed).permutation(B)[:max(2, (2 * B) // 3)].astype(np.int32)]


SHAPES = [(5, 5), (9, 67), (64, 67), (65, 3)]


# ------------------------------------------------------------------------------------------------ 1. residual
@pytest.mark.parametrize("n,B", SHAPES)
def test_residual(n, B):
    """nls_sys on the whole batch and on a permuted strict subset, with and without the correction ee; systems off the list unchanged"""
    import idahip
    from idahip import problems
    p = problems.enzyme_chain(n, B)
    net = RL.Net(p)
    ctx = problems.make_ctx(p)
    fields = entry_state(p, 100 * n + B)
    watch = (idahip.F_DELTA, idahip.F_SAVRES, idahip.F_YY, idahip.F_YP, idahip.F_EE)
    rng = np.random.default_rng(n + B)
    for idx in lists(B, n):
        for f, v in fields.items():
            ctx.upload(f, v)
        m = idx.size
        tn, cj = rng.uniform(0.0, 1.0, m), 10.0 ** rng.uniform(1.0, 4.0, m)
        listed = np.zeros(B, dtype=bool)
        listed[idx] = True
        for reset in (0, 1):
            ctx.nls_sys(tn, cj, reset, idx)
            got = {f: ctx.download(f) for f in watch}
            for q, s in enumerate(idx):
                ee = np.zeros(n) if reset else fields[idahip.F_EE][s]
                yy, yp = fields[idahip.F_YYPREDICT][s] + ee, fields[idahip.F_YPPREDICT][s] + cj[q] * ee
                r = RL.res(net, p["params"][s], yy, yp)
                assert same_bits(got[idahip.F_YY][s], yy) and same_bits(got[idahip.F_YP][s], yp), (n, B, s, reset)
                assert same_bits(got[idahip.F_DELTA][s], r) and same_bits(got[idahip.F_SAVRES][s], r), (n, B, s, reset, np.abs(got[idahip.F_DELTA][s] - r).max())
            for f in watch:
                assert same_bits(got[f][~listed], fields[f][~listed]), (n, B, f)  # off the list
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. analytic Jacobian and pattern
@pytest.mark.parametrize("n,B", SHAPES)
def test_analytic_jacobian_and_pattern(n, B):
    """mass_action_jac at two values of cj per system against ratelaw_ref.jac, every entry with the sign of its zero; the pattern the
    library reports is tables_laws'; and position (2, 0), which row 2 reaches only through reaction m + 1 -- species 0 in a slot AND
    in a factor of it --, holds the two terms of the header: the slot's term, then the factor's."""
    import idahip
    from idahip import mass_action, problems
    p = problems.enzyme_chain(n, B)
    net = RL.Net(p)
    m = n - 1
    tab = mass_action.tables_laws(n, p["reactions"], p["d"], p["nconst"])
    assert [t[1:] for t in tab["pattern"][(2, 0)]] == [(m + 1, (1,), -1), (m + 1, (0, 1), 1)]
    ctx = problems.make_ctx(p)
    assert ctx.mass_action_pattern() == (tab["nnz"], tab["ml"], tab["mu"])
    ctx.upload(idahip.F_YY, p["yy0"] * (1.0 + 1e-3 * np.random.default_rng(n).standard_normal((B, n))))
    yy = ctx.download(idahip.F_YY)
    idx = np.random.default_rng(B).permutation(B)[:3].astype(np.int32)
    for cj in (np.array([3.0, 250.0, 4.0e3]), np.array([1.0e5, 0.0, 17.0])):
        J = ctx.mass_action_jac(cj, idx)
        for q, s in enumerate(idx):
            prm, y = p["params"][s], yy[s]
            ref = RL.jac(net, prm, cj[q], y)
            assert same_bits(J[q], ref), (n, B, s, np.abs(J[q] - ref).max())
            k, K, Y = np.float64(prm[m + 1]), [np.float64(v) for v in prm[net.nreac:]], [np.float64(v) for v in y]
            finh, fsat, dsat = RL.f_val((RL.INH, 2, 0, 1), K, Y), RL.f_val((RL.SAT, 0, 1, 2), K, Y), RL.f_der((RL.SAT, 0, 1, 2), K, Y)
            t1 = np.float64(1.0) * (((k * Y[1]) * finh) * fsat)
            t2 = np.float64(1.0) * ((((k * Y[0]) * Y[1]) * finh) * dsat)
            assert same_bits(J[q][0, 2], np.float64(0.0) - (t1 + t2)) and t1 != 0.0 and t2 != 0.0
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. DQ Jacobian
@pytest.mark.parametrize("n,B", [(9, 67), (65, 3)])
def test_dq_jacobian(n, B):
    import idahip
    from idahip import problems
    p = problems.enzyme_chain(n, B)
    net = RL.Net(p)
    ctx = problems.make_ctx(p)
    fields = entry_state(p, n)
    for f, v in fields.items():
        ctx.upload(f, v)
    rng = np.random.default_rng(n)
    idx = rng.permutation(B)[:3 if n == 9 else 2].astype(np.int32)
    m = idx.size
    tn, cj, hh = np.zeros(m), 10.0 ** rng.uniform(1.0, 4.0, m), np.array([1.0, -1.0, 1.0])[:m] * 10.0 ** rng.uniform(-4.0, -1.0, m)
    ctx.nls_sys(tn, cj, 0, idx)
    yy, yp, rr = (ctx.download(f) for f in (idahip.F_YY, idahip.F_YP, idahip.F_SAVRES))
    D = ctx.jac_dq(tn, cj, hh, idx)
    for q, s in enumerate(idx):
        ref = RL.dense_dq(net, p["params"][s], yy[s], yp[s], fields[idahip.F_EWT][s], rr[s], cj[q], hh[q])
        assert same_bits(D[q], ref), (n, s, np.abs(D[q] - ref).max())
    ctx.close()


# ------------------------------------------------------------------------------------------------ 4. integrations
CNT = RL.RUN_CNT


def snapshot(ens):
    return {"yy": ens.yy(), "yp": ens.yp(), "hused": ens.real("hused"), "tn": ens.real("tn"), "c": ens.counters()}


def integrate(ctx, p, touts, host=True, fused=None):
    import idahip
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    if host:
        ens.set_device_controller(0)
    if fused is not None:
        ens.set_fused_newton(fused)
    active = ens.device_controller_active()
    out = []
    for t in touts:
        st, tret = ens.solve(float(t))
        out.append((st.copy(), tret.copy(), snapshot(ens)))
    ens.close()
    return out, active


def assert_equals_reference(run, ref, counters, what):
    for i, (st, tret, x) in enumerate(run):
        assert np.array_equal(st, ref["status"][i]) and same_bits(tret, ref["tret"][i]), (what, i, st, ref["status"][i])
        for k in ("yy", "yp", "hused", "tn"):
            assert same_bits(x[k], ref[k][i]), (what, i, k, np.abs(x[k] - ref[k][i]).max())
        assert np.array_equal(x["c"]["kused"], ref["kused"][i]), (what, i)
        for k in counters:
            assert np.array_equal(x["c"][k], ref["counters"][k][i]), (what, i, k, x["c"][k], ref["counters"][k][i])


def ended_well(name, ref):
    c = ref["counters"]
    assert (ref["status"] == 0).all() and (c["nni"][-1] > c["nst"][-1]).all(), name
    if name == "n16":
        assert c["netf"][-1].sum() > 0


def test_n5_on_the_host_stepper():
    from idahip import problems
    p, touts, ref = RL.case("n5")
    ended_well("n5", ref)
    ctx = problems.make_ctx(p)
    run, active = integrate(ctx, p, touts, host=False)  # n <= 8: the host stepper by itself
    ctx.close()
    assert active == 0
    assert_equals_reference(run, ref, CNT, "n5")


@pytest.mark.parametrize("name", ["n9", "n16"])
@pytest.mark.parametrize("mode", ["host", "host_fused", "rounds", "schedule"])
def test_integrations_on_every_stepper(name, mode):
    """the host stepper with the fused first two Newton iterations off and on, the device lock-step rounds, and a schedule over the
    outputs, each against the reference stepper: status, tret, yy, yp, hused, tn, kused and every counter at every output"""
    import idahip
    from idahip import problems
    p, touts, ref = RL.case(name)
    ended_well(name, ref)
    ctx = problems.make_ctx(p)
    if mode == "schedule":
        ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
        assert ens.device_controller_active() == 2
        st, tret, reached, yo, ypo = ens.solve_schedule(touts, outputs=True)
        x = snapshot(ens)
        ens.close()
        assert np.array_equal(st, ref["status"][-1]) and (reached == len(touts)).all() and same_bits(tret, ref["tret"][-1])
        assert same_bits(yo, ref["yy"]) and same_bits(ypo, ref["yp"])
        for k in ("yy", "yp", "hused", "tn"):
            assert same_bits(x[k], ref[k][-1]), k
        assert np.array_equal(x["c"]["kused"], ref["kused"][-1])
        for k in CNT:
            assert np.array_equal(x["c"][k], ref["counters"][k][-1]), k
    else:
        run, active = integrate(ctx, p, touts, host=mode != "rounds", fused={"host": 0, "host_fused": 1}.get(mode))
        assert active == (2 if mode == "rounds" else 0)
        assert_equals_reference(run, ref, CNT, (name, mode))
    ctx.close()


def test_n65_on_the_device_rounds():
    """the workgroup-per-system residual inside the rounds"""
    from idahip import problems
    p, touts, ref = RL.case("n65")
    ended_well("n65", ref)
    ctx = problems.make_ctx(p)
    run, active = integrate(ctx, p, touts, host=False)
    ctx.close()
    assert active == 2
    assert_equals_reference(run, ref, CNT, "n65 rounds")


@pytest.mark.parametrize("host", [True, False], ids=["host", "rounds"])
def test_dq_integration(host):
    from idahip import problems
    p, touts, ref = RL.case("n9", dq=True)
    ended_well("n9 dq", ref)
    ctx = problems.make_ctx(p)
    ctx.set_jacobian_dq(True)
    run, active = integrate(ctx, p, touts, host=host, fused=0 if host else None)
    ctx.close()
    assert active == (0 if host else 2)
    assert_equals_reference(run, ref, CNT + ("nre_dq",), "DQ")
    assert np.array_equal(ref["counters"]["nre_dq"][-1], 9 * ref["counters"]["nje"][-1]) and (ref["counters"]["nje"][-1] > 0).all()


# ------------------------------------------------------------------------------------------------ 5. constraints, calc_ic
def test_constraints():
    """n = 9, B = 16, c_i = 1 on every component: the reference's checks all pass (none corrected, none recovered -- that path is
    test_gpu_mass_action.py's); this pins that the factors and the check coexist"""
    from idahip import problems
    p, touts, ref = RL.case("n9", constr=tuple([1.0] * 9))
    ended_well("n9 constr", ref)
    census = {k: sum(c[k] for c in ref["census"]) for k in ref["census"][0]}
    assert census["passed"] > 0 and census["corrected"] + census["recovered"] + census["constr_fail"] == 0, census
    ctx = problems.make_ctx(p)
    ctx.set_constraints(np.ones(9))
    run, active = integrate(ctx, p, touts, host=False)  # constraints put n > 8 on the host stepper by themselves
    ctx.close()
    assert active == 0
    assert_equals_reference(run, ref, CNT, "constraints")


@pytest.mark.parametrize("n,B", [(9, 5), (65, 3)], ids=["wave9", "workgroup65"])
def test_calc_ic(n, B):
    """YA_YDP_INIT with id = d (the total's row algebraic), the algebraic component of y0 moved and y' = 0, against calcic_ref, every
    counter (nbacktr included). n = 9: the wave-per-system residual at the trial points, the solve a launch of its own; n = 65: the
    workgroup-per-system residual with the solve in the same launch."""
    import idahip
    from idahip import problems
    p = problems.enzyme_chain(n, B)
    net = RL.Net(p)
    id_ = p["d"].copy()
    yy0, yp0 = p["yy0"].copy(), np.zeros((B, n))
    yy0[:, n - 1] += 0.5 * (1.0 + np.arange(B)) / B
    ctx = problems.make_ctx(p)
    ctx.set_id(id_)
    ens = idahip.Ensemble(ctx, yy0, yp0)
    status = ens.calc_ic(idahip.YA_YDP_INIT, 0.01)
    yy, yp, cnt = ens.yy(), ens.yp(), ens.counters()
    ens.close()
    ctx.close()
    probs = [IC.Problem(n, RL.prob_res(p, s), lambda cj, y, ypv, rr, hic, ewt, s=s: RL.jac(net, p["params"][s], cj, y)) for s in range(B)]
    ref = IC.calc_ic_batch(probs, yy0, yp0, p["rtol"], p["atol"], IC.YA_YDP_INIT, 0.01, id=id_)
    assert (ref["status"] == 0).all() and np.array_equal(status, ref["status"]), (status, ref["status"])
    assert same_bits(yy, ref["yy"]) and same_bits(yp, ref["yp"]), (np.abs(yy - ref["yy"]).max(), np.abs(yp - ref["yp"]).max())
    for k in IC.COUNTERS:
        assert np.array_equal(cnt[k], ref["counters"][k]), (k, cnt[k], ref["counters"][k])
    assert (ref["counters"]["nni"] >= 1).all() and np.abs(yp).max() > 0.0
    assert np.abs(yy[:, n - 1] - p["yy0"][:, n - 1]).max() < 1e-6  # the total is back on its row


# ------------------------------------------------------------------------------------------------ 6. the twin
def test_twin_on_a_host_callback_ctx_gives_identical_bits():
    from idahip import problems
    p, touts, ref = RL.case("n9")
    twin = problems.make_ctx(RL.twin(p))
    run, active = integrate(twin, p, touts, host=True)
    twin.close()
    assert active == 0
    assert_equals_reference(run, ref, CNT, "twin")  # (and the device kind equals the same reference: the two agree bit for bit)


# ------------------------------------------------------------------------------------------------ 7. polynomial networks
def test_polynomial_network_through_the_new_setter():
    """reaction_chain(12) through set_rate_network (no factor, no constant) and through set_mass_action: the same pattern, and the
    same bits from the residual, the analytic Jacobian and an integration on the rounds"""
    import idahip
    from idahip import problems
    B = 5
    p = problems.reaction_chain(12, B)
    q = dict(p, nconst=0)  # (make_ctx takes the new setter)
    old, new = problems.make_ctx(p), problems.make_ctx(q)
    assert old.mass_action_pattern() == new.mass_action_pattern()
    fields = entry_state(p, 12)
    idx, tn, cj = np.array([3, 0, 4], dtype=np.int32), np.zeros(3), np.array([10.0, 200.0, 3.0e3])
    got = []
    for c in (old, new):
        for f, v in fields.items():
            c.upload(f, v)
        c.nls_sys(tn, cj, 0, idx)
        got.append((c.download(idahip.F_SAVRES), c.download(idahip.F_DELTA), c.mass_action_jac(cj, idx)))
    assert all(same_bits(a, b) for a, b in zip(*got))
    net = MA.Net(p)
    for k, s in enumerate(idx):
        ee = fields[idahip.F_EE][s]
        assert same_bits(got[1][0][s], MA.res(net, p["params"][s], fields[idahip.F_YYPREDICT][s] + ee, fields[idahip.F_YPPREDICT][s] + cj[k] * ee))
    runs = [integrate(c, p, p["touts"], host=False) for c in (old, new)]
    for (a, act_a), (b, act_b) in [runs]:
        assert act_a == act_b == 2
        for (sa, ta, xa), (sb, tb, xb) in zip(a, b):
            assert np.array_equal(sa, sb) and (sa == 0).all() and same_bits(ta, tb)
            assert all(same_bits(xa[k], xb[k]) for k in ("yy", "yp", "hused", "tn"))
            assert all(np.array_equal(xa["c"][k], xb["c"][k]) for k in xa["c"])
    old.close()
    new.close()


# ------------------------------------------------------------------------------------------------ 8. a zero denominator
@pytest.mark.parametrize("n", [9, 65])
def test_zero_denominator(n):
    """K = 0 and y_s = 0: the factor is 0/0. System 1 has every constant and every y at 0, system 2 only K_0 and the two species its
    factors read (the feed's inh(m-1, K_0, 2) and reaction m+1's inh(2, K_0, 1)); systems 0 and 3 are as generated. The residual has
    the reference's bits, NaNs included (residual only: nothing integrates through a NaN)."""
    import idahip
    from idahip import problems
    B, m = 4, n - 1
    p = problems.enzyme_chain(n, B)
    net = RL.Net(p)
    prm = p["params"].copy()
    fields = entry_state(p, n)
    prm[1, net.nreac:] = 0.0
    fields[idahip.F_YYPREDICT][1] = 0.0
    prm[2, net.nreac] = 0.0
    fields[idahip.F_YYPREDICT][2, [2, m - 1]] = 0.0
    ctx = problems.make_ctx(p)
    ctx.set_problem_params(prm)
    for f, v in fields.items():
        ctx.upload(f, v)
    idx, cj = ctx.all_idx(), np.full(B, 100.0)
    ctx.nls_sys(np.zeros(B), cj, 1, idx)
    got = ctx.download(idahip.F_SAVRES)
    ctx.close()
    ref = np.stack([RL.res(net, prm[s], fields[idahip.F_YYPREDICT][s], fields[idahip.F_YPPREDICT][s]) for s in range(B)])
    assert np.isnan(ref[1]).any() and np.isnan(ref[2]).any() and np.isfinite(ref[[0, 3]]).all() and np.isfinite(ref[2]).any()
    print("NaN bit patterns: device", sorted({hex(v) for v in bits(got[np.isnan(got)])}), "reference", sorted({hex(v) for v in bits(ref[np.isnan(ref)])}))
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (np.isnan(got), np.isnan(ref))
    assert same_bits(got, ref), [(s, i, hex(bits(got)[s, i]), hex(bits(ref)[s, i])) for s, i in zip(*np.nonzero(bits(got) != bits(ref)))]


# ------------------------------------------------------------------------------------------------ 9. parameters
def test_parameters():
    import idahip
    from idahip import problems
    n, B = 9, 5
    p = problems.enzyme_chain(n, B)
    net = RL.Net(p)
    nparam = net.nreac + net.nconst
    assert p["params"].shape == (B, nparam) and net.nconst == n - 1
    ctx = problems.make_ctx(p)
    for bad in (net.nreac, nparam + 1):
        with pytest.raises(idahip.IdaHipError, match=r"takes %d parameters" % nparam):
            ctx.set_problem_params(np.ones((B, bad)))
    fields = entry_state(p, 9)
    for f, v in fields.items():
        ctx.upload(f, v)
    idx, z, cj = ctx.all_idx(), np.zeros(B), np.full(B, 50.0)
    ctx.nls_sys(z, cj, 1, idx)
    before = ctx.download(idahip.F_SAVRES)
    prm = p["params"].copy()
    prm[3, net.nreac + 2] *= 1.5  # one system's K_2 (the factor of the chain step 1 -> 2)
    ctx.set_problem_params(prm[3:4], first=3)
    ctx.nls_sys(z, cj, 1, idx)
    after = ctx.download(idahip.F_SAVRES)
    ctx.close()
    assert same_bits(after[[0, 1, 2, 4]], before[[0, 1, 2, 4]]) and not same_bits(after[3], before[3])
    assert same_bits(after[3], RL.res(net, prm[3], fields[idahip.F_YYPREDICT][3], fields[idahip.F_YPPREDICT][3]))


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals():
    import idahip
    from idahip import problems
    d = [1.0, 1.0, 1.0, 0.0]
    ctx = idahip.Ctx("mass_action", 4, 2)
    for text, kw in RL.REFUSALS:
        reactions, dd, nconst = RL.refused_network(kw)
        slots, fac, rows, reacs, nu, dv = RL.raw_arrays(reactions, dd)
        with pytest.raises(idahip.IdaHipError, match=r"\(-2\).*idahip_set_rate_network: " + re.escape(text)):
            ctx.set_rate_network_raw(slots, fac, nconst, rows, reacs, nu, dv)
        with pytest.raises(idahip.IdaHipError, match=r"not set \(idahip_set_mass_action\)"):  # nothing was changed
            ctx.mass_action_pattern()
    slots, fac, rows, reacs, nu, dv = RL.raw_arrays(RL.HAND, d)
    bad = fac.copy()
    bad[1, 0] = 3
    with pytest.raises(idahip.IdaHipError, match=r"factor 1: reaction 3 outside \[0, 3\)"):
        ctx.set_rate_network_raw(slots, bad, 2, rows, reacs, nu, dv)
    with pytest.raises(idahip.IdaHipError, match=r"nreac = 0"):
        ctx.set_rate_network_raw(np.zeros((0, 3), dtype=np.int32), fac[:0], 0, rows[:0], reacs[:0], nu[:0], dv)
    # factors given out of reaction order keep the caller's order within a reaction; a constant no factor uses is allowed
    ctx.set_rate_network_raw(slots, fac[::-1], 3, rows, reacs, nu, dv)
    tab = idahip.mass_action.tables_laws(4, RL.HAND, d, 3)
    assert ctx.mass_action_pattern() == (tab["nnz"], tab["ml"], tab["mu"]) == (8, 2, 1)
    with pytest.raises(idahip.IdaHipError, match=r"takes 6 parameters"):
        ctx.set_problem_params(np.ones((2, 3)))
    # once per ctx, across the two setters
    with pytest.raises(idahip.IdaHipError, match=r"idahip_set_rate_network: the reaction network is already set"):
        ctx.set_rate_network(RL.HAND, d, 2)
    with pytest.raises(idahip.IdaHipError, match=r"idahip_set_mass_action: the reaction network is already set"):
        ctx.set_mass_action([(r[0], r[1]) for r in RL.HAND], d)
    ctx.close()
    ctx = idahip.Ctx("mass_action", 4, 2)
    ctx.set_mass_action([(r[0], r[1]) for r in RL.HAND], d)
    with pytest.raises(idahip.IdaHipError, match=r"idahip_set_rate_network: the reaction network is already set"):
        ctx.set_rate_network(RL.HAND, d, 2)
    ctx.close()
    heat = idahip.Ctx("heat1d", 16, 2)
    with pytest.raises(idahip.IdaHipError, match=r"idahip_set_rate_network: not an IDAHIP_MASS_ACTION ctx"):
        heat.set_rate_network(problems.enzyme_chain(16, 2)["reactions"], np.ones(16), 15)
    heat.set_problem_params(np.ones((2, 1)))  # (and the heat ctx goes on working)
    heat.close()


def test_factor_order_within_a_reaction_is_the_callers():
    """the same reaction's two factors listed in either order give different roundings of the product: the device follows the list"""
    import idahip
    n, B = 4, 2
    d = [1.0, 1.0, 1.0, 0.0]
    rng = np.random.default_rng(4)
    y, yp, prm = rng.uniform(0.5, 1.5, (B, n)), rng.uniform(-1.0, 1.0, (B, n)), rng.uniform(0.5, 2.0, (B, 3))
    for order in ([("sat", 1, 0, 3), ("inh", 2, 1, 2), ("sat", 3, 0, 1)], [("sat", 3, 0, 1), ("inh", 2, 1, 2), ("sat", 1, 0, 3)]):
        reactions = [((0,), {0: -1.0, 1: 1.0, 3: 0.5}, order)]
        net = RL.Net({"n": n, "reactions": reactions, "d": d, "nconst": 2})
        ctx = idahip.Ctx("mass_action", n, B)
        ctx.set_rate_network(reactions, d, 2)
        ctx.set_problem_params(prm)
        ctx.upload(idahip.F_YYPREDICT, y)
        ctx.upload(idahip.F_YPPREDICT, yp)
        ctx.upload(idahip.F_EE, np.zeros((B, n)))
        ctx.nls_sys(np.zeros(B), np.ones(B), 1, ctx.all_idx())
        got, J = ctx.download(idahip.F_SAVRES), ctx.mass_action_jac(np.array([2.0, 30.0]))
        ctx.close()
        for s in range(B):
            assert same_bits(got[s], RL.res(net, prm[s], y[s], yp[s])), (order, s)
            assert same_bits(J[s], RL.jac(net, prm[s], [2.0, 30.0][s], y[s])), (order, s)
