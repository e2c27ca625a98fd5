"""IDAHIP_MASS_ACTION (a reaction network as tables, interpreted by the kernels of csrc/mass_action.hpp) on the device against
tests/massaction_ref.py, bit for bit (view(np.uint64) equality: no tolerance appears in this file): the residual, the analytic and
the difference-quotient Jacobian at every launch shape, whole integrations on the host stepper, the fused Newton, the device
lock-step rounds and a schedule, DQ integrations, constraints, calc_ic, the host-callback twin, and the refusals."""
import numpy as np
import pytest

import calcic_ref as IC
import massaction_ref as MA
import oracle_lib as O
import stepper_ref as SR

pytestmark = pytest.mark.gpu
_CACHE = {}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


def roberts_batch(B):
    """roberts_network for B systems: the three kinetic constants of system s scaled by 1 + s/8, y'(0) to match"""
    from idahip import mass_action, problems
    p = problems.roberts_network()
    k = np.tile(p["params"], (B, 1))
    k[:, :3] *= (1.0 + np.arange(B) / 8.0)[:, None]
    tab = mass_action.tables(3, p["reactions"], p["d"])
    p["params"], p["yy0"] = k, np.tile(p["yy0"], (B, 1))
    p["yp0"] = np.stack([mass_action.rhs(tab, k[s], p["yy0"][s]) * p["d"] for s in range(B)])
    return p


def network(n, B):
    from idahip import problems
    if n == 3:
        return roberts_batch(B)
    if n == 16:
        return problems.bruss1d_network(8, B)
    return problems.reaction_chain(n, B, seed=n)


def entry_state(p, seed):
    import idahip
    B, n = p["yy0"].shape
    rng = np.random.default_rng(seed)
    yypred = p["yy0"] * (1.0 + 1e-3 * rng.standard_normal((B, n)))
    return {idahip.F_YYPREDICT: yypred, idahip.F_YPPREDICT: p["yp0"] + 1e-2 * rng.standard_normal((B, n)),
            idahip.F_EE: 1e-4 * rng.standard_normal((B, n)), idahip.F_EWT: 1.0 / (p["rtol"] * np.abs(yypred) + p["atol"][0]),
            idahip.F_YY: p["yy0"].copy(), idahip.F_YP: p["yp0"].copy(), idahip.F_DELTA: np.zeros((B, n)), idahip.F_SAVRES: np.zeros((B, n))}


def lists(B, seed):
    """the whole batch in order, and for B > 1 a permuted strict subset"""
    out = [np.arange(B, dtype=np.int32)]
    if B > 1:
        out.append(np.random.default_rng(seed).permutation(B)[:max(2, (2 * B) // 3)].astype(np.int32))
    return out


# ------------------------------------------------------------------------------------------------ 4. kernels
@pytest.mark.parametrize("B", [1, 5, 67])
@pytest.mark.parametrize("n", [3, 9, 16, 64, 65, 130])
def test_residual_and_jacobians(n, B):
    """nls_sys, the analytic Jacobian (idahip_mass_action_jac: the setup's kernel into a buffer of its own, every entry with the sign
    of its zero) and idahip_jac_dq against massaction_ref, on the whole batch and on a permuted strict subset; systems off the list
    unchanged; the work-matrix path of nls_lsetup through its factors (by value against the oracle's getrf, as everywhere)."""
    import idahip
    from idahip import problems
    p = network(n, B)
    net = MA.Net(p)
    ctx = problems.make_ctx(p)
    assert ctx.mass_action_pattern()[0] >= n
    fields = entry_state(p, 100 * n + B)
    watch = (idahip.F_DELTA, idahip.F_SAVRES, idahip.F_YY, idahip.F_YP, idahip.F_EE)
    rng = np.random.default_rng(n + B)
    few = 3 if n >= 64 else B  # systems whose Jacobians are restated: all of them up to n = 16 (a DQ Jacobian is n residuals)
    for idx in lists(B, n):
        for f, v in fields.items():
            ctx.upload(f, v)
        m = idx.size
        tn, cj, hh = rng.uniform(0.0, 1.0, m), 10.0 ** rng.uniform(1.0, 4.0, m), rng.choice([-1.0, 1.0], m) * 10.0 ** rng.uniform(-4.0, -1.0, m)
        listed = np.zeros(B, dtype=bool)
        listed[idx] = True
        for reset in (0, 1):
            ctx.nls_sys(tn, cj, reset, idx)
            got = {f: ctx.download(f) for f in watch}
            for q, s in enumerate(idx):
                ee = np.zeros(n) if reset else fields[idahip.F_EE][s]
                yy, yp = fields[idahip.F_YYPREDICT][s] + ee, fields[idahip.F_YPPREDICT][s] + cj[q] * ee
                r = MA.res(net, p["params"][s], yy, yp)
                assert same_bits(got[idahip.F_YY][s], yy) and same_bits(got[idahip.F_YP][s], yp), (n, B, s, reset)
                assert same_bits(got[idahip.F_DELTA][s], r) and same_bits(got[idahip.F_SAVRES][s], r), (n, B, s, reset, np.abs(got[idahip.F_DELTA][s] - r).max())
                assert same_bits(got[idahip.F_EE][s], ee)
            for f in watch:
                assert same_bits(got[f][~listed], fields[f][~listed]), (n, B, f)  # off the list
        sub = idx[:few]
        J = ctx.mass_action_jac(cj[:sub.size], sub)
        D = ctx.jac_dq(tn[:sub.size], cj[:sub.size], hh[:sub.size], sub)
        for q, s in enumerate(sub):
            k, yy, yp = p["params"][s], got[idahip.F_YY][s], got[idahip.F_YP][s]
            ref = MA.jac(net, k, cj[q], yy)
            assert same_bits(J[q], ref), ("jac", n, B, s, np.abs(J[q] - ref).max())
            ref = MA.dense_dq(net, k, yy, yp, fields[idahip.F_EWT][s], got[idahip.F_SAVRES][s], cj[q], hh[q])
            assert same_bits(D[q], ref), ("jac_dq", n, B, s, np.abs(D[q] - ref).max())
        off_before = ctx.download_lu(int(np.flatnonzero(~listed)[0])) if not listed.all() else None
        rc, info = ctx.nls_lsetup(tn, cj, idx)
        assert rc >= 0
        for q, s in enumerate(sub):
            cm = np.ascontiguousarray(MA.jac(net, p["params"][s], cj[q], got[idahip.F_YY][s]))[None]
            oinfo, opiv = O.getrf_batch(cm)
            lu, piv = ctx.download_lu(int(s))
            assert info[q] == oinfo[0] and (oinfo[0] != 0 or (np.array_equal(piv, opiv[0]) and np.array_equal(lu, cm[0].T))), ("lsetup", n, B, s)
        if off_before is not None:
            a, b = ctx.download_lu(int(np.flatnonzero(~listed)[0]))
            assert same_bits(a, off_before[0]) and np.array_equal(b, off_before[1])
    ctx.close()


@pytest.mark.parametrize("n", [9, 65])
def test_skip_mask_of_the_fused_newton_iterations(n):
    """idahip_newton_iter2 on B = 5: list positions 0, 2, 4 converge at m = 0 and are skipped by the second residual (their savres,
    delta and ee stay), 1 and 3 go on: their savres is the residual at the corrected point, bit for bit."""
    import idahip
    from idahip import problems
    B = 5
    p = network(n, B)
    net = MA.Net(p)
    ctx = problems.make_ctx(p)
    fields = entry_state(p, n)
    for f, v in fields.items():
        ctx.upload(f, v)
    idx = np.array([4, 1, 0, 3, 2], dtype=np.int32)
    tn, cj = np.zeros(B), np.full(B, 1.0e3)
    rc, info = ctx.nls_sys_setup(tn, cj, True, idx)
    assert rc == 0 and not info.any()
    r0 = ctx.download(idahip.F_SAVRES)
    ends = np.arange(B) % 2 == 0
    scale = np.full(B, 0.75)
    dn, conv = ctx.newton_iter2(scale, tn, cj, np.zeros(B), np.ones(B), np.where(ends, np.inf, 0.0), idx)
    sav, dl, ee = (ctx.download(f) for f in (idahip.F_SAVRES, idahip.F_DELTA, idahip.F_EE))
    for q, s in enumerate(idx):
        lu, piv = ctx.download_lu(int(s))
        assert same_bits(r0[s], MA.res(net, p["params"][s], fields[idahip.F_YYPREDICT][s], fields[idahip.F_YPPREDICT][s])), s
        d1, e1, n0 = SR.newton_iter(lu, piv, r0[s], np.zeros(n), fields[idahip.F_EWT][s], scale[q])
        assert same_bits(np.float64(dn[q, 0]), np.float64(n0)), (q, dn[q, 0], n0)
        if ends[q]:
            assert conv[q] == 1 and dn[q, 1] == 0.0
            assert same_bits(sav[s], r0[s]) and np.array_equal(dl[s], d1) and np.array_equal(ee[s], e1), q
        else:
            r1 = MA.res(net, p["params"][s], fields[idahip.F_YYPREDICT][s] + e1, fields[idahip.F_YPPREDICT][s] + cj[q] * e1)
            assert conv[q] != 1 and same_bits(sav[s], r1), (q, conv[q], np.abs(sav[s] - r1).max())
            d2, e2, n1 = SR.newton_iter(lu, piv, r1, e1, fields[idahip.F_EWT][s], scale[q])
            assert np.array_equal(dl[s], d2) and np.array_equal(ee[s], e2) and same_bits(np.float64(dn[q, 1]), np.float64(n1)), q
    ctx.close()


@pytest.mark.parametrize("superpanel", [0, 1])
def test_residual_and_jacobian_at_the_size_limit(superpanel):
    """n = 4096, B = 2: the residual and the analytic Jacobian (16.8 million entries per system, signs of zeros included); then two
    setups in a row against the host-callback twin's factors, on both LU pipelines for n > 1024 (idahip_set_lu_superpanel; 0 is the
    kind's default). The Jacobian kernel writes the whole matrix at every setup, whatever the last factorisation left in it."""
    import idahip
    from idahip import problems
    n, B = 4096, 2
    p = network(n, B)
    net = MA.Net(p)
    ctx, twin = problems.make_ctx(p), problems.make_ctx(MA.twin(p))
    assert ctx.lu_superpanel() == 0
    for c in (ctx, twin):
        c.set_lu_superpanel(superpanel)
    fields = entry_state(p, n)
    idx, tn, cj = np.array([1, 0], dtype=np.int32), np.zeros(B), np.array([300.0, 2.0e3])
    for c in (ctx, twin):
        for f, v in fields.items():
            c.upload(f, v)
        c.nls_sys(tn, cj, 1, idx)
    yy, rr = ctx.download(idahip.F_YY), ctx.download(idahip.F_SAVRES)
    for q, s in enumerate(idx):
        assert same_bits(rr[s], MA.res(net, p["params"][s], yy[s], ctx.download(idahip.F_YP)[s])), s
    J = ctx.mass_action_jac(cj, idx)
    for q, s in enumerate(idx):
        assert same_bits(J[q], MA.jac(net, p["params"][s], cj[q], yy[s])), s
    del J
    for rep in range(2):
        for c in (ctx, twin):
            rc, info = c.nls_lsetup(tn, cj * (1.0 + rep), idx)
            assert rc == 0 and not info.any()
        for s in idx:
            lu, piv = np.empty(n * n), np.empty(n, dtype=np.int64)
            tl, tp = np.empty(n * n), np.empty(n, dtype=np.int64)
            assert ctx.H.idahip_download_lu(ctx.h, int(s), idahip._p(lu), idahip._p(piv, idahip.i64p)) == 0
            assert twin.H.idahip_download_lu(twin.h, int(s), idahip._p(tl), idahip._p(tp, idahip.i64p)) == 0
            assert np.array_equal(piv, tp) and same_bits(lu, tl), (rep, s)
    twin.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. integrations
CNT = MA.RUN_CNT


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


CASES = {"roberts": (3, 5, (0.4, 4.0)), "chain9": (9, 67, (0.01, 0.02, 0.03)), "bruss": (16, 67, (0.05, 0.1, 0.15)), "chain65": (65, 5, (0.005, 0.01))}


def case(name, **kw):
    """(problem, touts, the reference run): computed once, shared and left unchanged"""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _CACHE:
        n, B, touts = CASES[name]
        p = network(n, B)
        _CACHE[key] = (p, touts, MA.run(p, touts, **kw))
    return _CACHE[key]


def test_roberts_network_on_the_host_stepper():
    from idahip import problems
    p, touts, ref = case("roberts")
    assert (ref["status"] == 0).all()
    ctx = problems.make_ctx(p)
    run, active = integrate(ctx, p, touts, host=False)  # n <= 8: the host stepper by itself
    ctx.close()
    assert active == 0
    assert_equals_reference(run, ref, CNT, "roberts_network")


@pytest.mark.parametrize("name", ["chain9", "bruss"])
@pytest.mark.parametrize("mode", ["host", "host_fused", "rounds", "schedule"])
def test_integrations_on_every_stepper(name, mode):
    """B = 67: the host stepper with the fused first two Newton iterations off and on, the device lock-step rounds, and a schedule
    over the three outputs, each against DirectIda: status, tret, yy, yp, hused, tn, kused and every counter at every output."""
    import idahip
    from idahip import problems
    p, touts, ref = case(name)
    assert (ref["status"] == 0).all() and (ref["counters"]["nni"][-1] > ref["counters"]["nst"][-1]).all()
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


def test_chain65_on_the_device_rounds():
    """the workgroup-per-system residual inside the rounds"""
    from idahip import problems
    p, touts, ref = case("chain65")
    ctx = problems.make_ctx(p)
    run, active = integrate(ctx, p, touts, host=False)
    ctx.close()
    assert active == 2 and (ref["status"] == 0).all()
    assert_equals_reference(run, ref, CNT, "chain65 rounds")


# ------------------------------------------------------------------------------------------------ 6. DQ Jacobians
@pytest.mark.parametrize("host", [True, False], ids=["host", "rounds"])
def test_dq_integration(host):
    from idahip import problems
    p, touts, ref = case("chain9", dq=True)
    ctx = problems.make_ctx(p)
    ctx.set_jacobian_dq(True)
    run, active = integrate(ctx, p, touts, host=host, fused=0 if host else None)
    ctx.close()
    assert active == (0 if host else 2) and (ref["status"] == 0).all()
    assert_equals_reference(run, ref, CNT + ("nre_dq",), "DQ")
    assert np.array_equal(ref["counters"]["nre_dq"][-1], 9 * ref["counters"]["nje"][-1]) and (ref["counters"]["nje"][-1] > 0).all()


# ------------------------------------------------------------------------------------------------ 7. constraints
def test_constraints():
    """reaction_chain(n = 12, seed 2), B = 8, c_i = 1 on every species, rtol 0.1, atol 0.01: the reference's census has one
    "recovered" attempt (tests run it first; another seed if this one ever has none)."""
    from idahip import problems
    p = problems.reaction_chain(12, 8, seed=2)
    p["rtol"], p["atol"] = 0.1, np.array([0.01])
    touts = (0.05, 0.5)
    ref = MA.run(p, touts, constr=np.ones(12))
    census = {k: sum(c[k] for c in ref["census"]) for k in ref["census"][0]}
    assert census["corrected"] + census["recovered"] >= 1, census
    ctx = problems.make_ctx(p)
    ctx.set_constraints(np.ones(12))
    run, active = integrate(ctx, p, touts, host=False)  # constraints put n > 8 on the host stepper by themselves
    ctx.close()
    assert active == 0
    assert_equals_reference(run, ref, CNT, "constraints")


# ------------------------------------------------------------------------------------------------ 8. calc_ic
def test_calc_ic_on_the_roberts_network():
    """YA_YDP_INIT with id = (1, 1, 0) from a perturbed y0[2] (and y' = 0) against calcic_ref, status and nbacktr included"""
    import idahip
    from idahip import problems
    B = 5
    p = roberts_batch(B)
    net = MA.Net(p)
    id_ = np.array([1.0, 1.0, 0.0])
    yy0, yp0 = p["yy0"].copy(), np.zeros((B, 3))
    yy0[:, 2] += 0.01 * (1.0 + np.arange(B))
    ctx = problems.make_ctx(p)
    ctx.set_id(id_)
    ens = idahip.Ensemble(ctx, yy0, yp0)
    status = ens.calc_ic(idahip.YA_YDP_INIT, 0.4)
    yy, yp, cnt = ens.yy(), ens.yp(), ens.counters()
    ens.close()
    ctx.close()
    probs = [IC.Problem(3, MA.prob_res(p, s), lambda cj, y, ypv, rr, hic, ewt, s=s: MA.jac(net, p["params"][s], cj, y)) for s in range(B)]
    ref = IC.calc_ic_batch(probs, yy0, yp0, p["rtol"], p["atol"], IC.YA_YDP_INIT, 0.4, id=id_)
    assert (ref["status"] == 0).all() and np.array_equal(status, ref["status"]), (status, ref["status"])
    assert same_bits(yy, ref["yy"]) and same_bits(yp, ref["yp"]), (np.abs(yy - ref["yy"]).max(), np.abs(yp - ref["yp"]).max())
    for k in IC.COUNTERS:
        assert np.array_equal(cnt[k], ref["counters"][k]), (k, cnt[k], ref["counters"][k])
    assert np.abs(yy[:, 2] - p["yy0"][:, 2]).max() < 1e-6 and np.abs(yp).max() > 0.0


@pytest.mark.parametrize("n,force_wg", [(12, False), (12, True), (65, False)], ids=["wave12", "workgroup12", "workgroup65"])
def test_calc_ic_on_a_reaction_chain(n, force_wg, monkeypatch):
    """YA_YDP_INIT with id = d (the conservation row algebraic), the conservation component moved and y' = 0, against calcic_ref,
    every counter (nbacktr included). n = 12: the wave-per-system residual at the trial points, the solve a launch of its own;
    n = 65: the workgroup-per-system residual with the solve in the same launch; n = 12 with the measurement switch IDAHIP_MA_WG=1
    (read at idahip_create): that kernel at n <= 64 -- and nls_sys through it, against the restated residual."""
    import idahip
    from idahip import problems
    if force_wg:
        monkeypatch.setenv("IDAHIP_MA_WG", "1")
    B = 5
    p = problems.reaction_chain(n, B, seed=n)
    net = MA.Net(p)
    id_ = p["d"].copy()
    yy0, yp0 = p["yy0"].copy(), np.zeros((B, n))
    yy0[:, n - 1] += 3.0 * (1.0 + np.arange(B)) / B
    ctx = problems.make_ctx(p)
    ctx.set_id(id_)
    ens = idahip.Ensemble(ctx, yy0, yp0)
    status = ens.calc_ic(idahip.YA_YDP_INIT, 0.01)
    yy, yp, cnt = ens.yy(), ens.yp(), ens.counters()
    ens.close()
    probs = [IC.Problem(n, MA.prob_res(p, s), lambda cj, y, ypv, rr, hic, ewt, s=s: MA.jac(net, p["params"][s], cj, y)) for s in range(B)]
    ref = IC.calc_ic_batch(probs, yy0, yp0, p["rtol"], p["atol"], IC.YA_YDP_INIT, 0.01, id=id_)
    assert (ref["status"] == 0).all() and np.array_equal(status, ref["status"]), (status, ref["status"])
    assert same_bits(yy, ref["yy"]) and same_bits(yp, ref["yp"]), (np.abs(yy - ref["yy"]).max(), np.abs(yp - ref["yp"]).max())
    for k in IC.COUNTERS:
        assert np.array_equal(cnt[k], ref["counters"][k]), (k, cnt[k], ref["counters"][k])
    assert (ref["counters"]["nni"] >= 4).all() and np.abs(yp).max() > 0.0
    if force_wg:
        fields = entry_state(p, n)
        for f, v in fields.items():
            ctx.upload(f, v)
        idx, cj = np.array([3, 0, 4], dtype=np.int32), np.array([10.0, 200.0, 3.0e3])
        ctx.nls_sys(np.zeros(3), cj, 0, idx)
        got = ctx.download(idahip.F_SAVRES)
        for q, s in enumerate(idx):
            ee = fields[idahip.F_EE][s]
            r = MA.res(net, p["params"][s], fields[idahip.F_YYPREDICT][s] + ee, fields[idahip.F_YPPREDICT][s] + cj[q] * ee)
            assert same_bits(got[s], r), s
        assert same_bits(got[[1, 2]], fields[idahip.F_SAVRES][[1, 2]])
    ctx.close()


# ------------------------------------------------------------------------------------------------ 9. the twin
def test_twin_on_a_host_callback_ctx_gives_identical_bits():
    from idahip import problems
    p, touts, ref = case("chain9")
    twin = problems.make_ctx(MA.twin(p))
    run, active = integrate(twin, p, touts, host=True)
    twin.close()
    assert active == 0
    assert_equals_reference(run, ref, CNT, "twin")  # (and the device kind equals the same reference: the two agree bit for bit)


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals(capfd):
    import idahip
    from idahip import problems
    p = network(9, 5)
    B, n = 5, 9
    ctx = idahip.Ctx("mass_action", n, B)
    ctx.set_tolerances(p["rtol"], p["atol"])
    idx, z, o = ctx.all_idx(), np.zeros(B), np.ones(B)
    for f, v in entry_state(p, 1).items():
        ctx.upload(f, v)
    before = {f: ctx.download(f) for f in (idahip.F_DELTA, idahip.F_SAVRES, idahip.F_YY, idahip.F_YP)}
    launches = ctx.timing_get()
    calls = {
        "nls_sys": lambda: ctx.nls_sys(z, o, 0, idx), "nls_lsetup": lambda: ctx.nls_lsetup(z, o, idx),
        "nls_sys_setup": lambda: ctx.nls_sys_setup(z, o, True, idx), "jac_dq": lambda: ctx.jac_dq(z, o, o, idx),
        "newton_iter2": lambda: ctx.newton_iter2(o, z, o, z, o, o, idx), "mass_action_pattern": ctx.mass_action_pattern,
        "mass_action_jac": lambda: ctx.mass_action_jac(o, idx), "set_problem_params": lambda: ctx.set_problem_params(p["params"]),
        "ic_res": lambda: ctx._chk(ctx.H.idahip_ic_res(ctx.h, idahip._p(z), idahip._p(o), idahip._p(idx, idahip.i32p), B), "ic_res"),
        "ic_setup": lambda: ctx._chk(ctx.H.idahip_ic_setup(ctx.h, idahip._p(z), idahip._p(o), idahip._p(np.zeros(B, dtype=np.int32), idahip.i32p),
                                                           idahip._p(idx, idahip.i32p), B), "ic_setup"),
        "ic_trial": lambda: ctx._chk(ctx.H.idahip_ic_trial(ctx.h, 2, idahip._p(z), idahip._p(o), idahip._p(o), idahip._p(np.zeros(B)),
                                                           idahip._p(idx, idahip.i32p), B), "ic_trial"),
        "idaens_create": lambda: idahip.Ensemble(ctx, p["yy0"], p["yp0"]),
    }
    for name, call in calls.items():
        with pytest.raises(idahip.IdaHipError, match=r"\(-2\).*not set \(idahip_set_mass_action\)"):
            call()
    ctx.set_jacobian_dq(True)
    with pytest.raises(idahip.IdaHipError, match=r"\(-2\).*not set"):
        ctx.nls_lsetup_dq(z, o, o, idx)
    ctx.set_jacobian_dq(False)
    assert ctx.timing_get() == launches  # nothing was launched
    for f, v in before.items():
        assert same_bits(ctx.download(f), v)
    # the setter's own refusals: each names its first offending item and changes nothing
    slots, rows, reacs, nu, d = idahip.mass_action.flatten(n, p["reactions"], p["d"])

    def bad(text, **kw):
        a = dict(slots=slots.copy(), rows=rows.copy(), reacs=reacs.copy(), nu=nu.copy(), d=d.copy())
        for k, (i, v) in kw.items():
            a[k][i] = v
        with pytest.raises(idahip.IdaHipError, match=text):
            ctx.set_mass_action_raw(a["slots"], a["rows"], a["reacs"], a["nu"], a["d"])

    bad(r"reaction 2, slot 0: species 9 outside", slots=((2, 0), 9))
    assert slots[2, 1] >= 0  # (a second-order reaction)
    bad(r"reaction 2, slot 1: a species after an unused slot", slots=((2, 0), -1))
    bad(r"entry 4: row -1 outside", rows=(4, -1))
    bad(r"entry 3: reaction %d outside" % slots.shape[0], reacs=(3, slots.shape[0]))
    bad(r"entry 7: nu = nan", nu=(7, np.nan))
    bad(r"d\[8\] = inf", d=(8, np.inf))
    with pytest.raises(idahip.IdaHipError, match=r"nreac = 0"):
        ctx.set_mass_action_raw(np.zeros((0, 3), dtype=np.int32), rows[:0], reacs[:0], nu[:0], d)
    with pytest.raises(idahip.IdaHipError, match=r"not set"):
        ctx.mass_action_pattern()
    # a later correct call works
    ctx.set_mass_action(p["reactions"], p["d"])
    tab = idahip.mass_action.tables(n, p["reactions"], p["d"])
    assert ctx.mass_action_pattern() == (tab["nnz"], tab["ml"], tab["mu"])
    with pytest.raises(idahip.IdaHipError, match=r"already set"):
        ctx.set_mass_action(p["reactions"], p["d"])
    with pytest.raises(idahip.IdaHipError, match=r"takes %d parameters" % slots.shape[0]):
        ctx.set_problem_params(np.ones((B, 3)))
    ctx.set_problem_params(p["params"])
    ctx.nls_sys(z, o, 1, idx)
    net = MA.Net(p)
    yy, yp, r = (ctx.download(f) for f in (idahip.F_YY, idahip.F_YP, idahip.F_SAVRES))
    for s in range(B):
        assert same_bits(r[s], MA.res(net, p["params"][s], yy[s], yp[s])), s
    ctx.close()
    # the other kinds and the other ctx forms
    capfd.readouterr()
    for kw, text in (({"band": (2, 2)}, "has no band form"), ({"krylov": 5}, "idahip_create_krylov: problem kind 6")):
        with pytest.raises(idahip.IdaHipError, match=r"\(-2\)"):
            idahip.Ctx("mass_action", 16, 2, **kw)
        assert text in capfd.readouterr().err
    for n_bad in (1, 4097):
        with pytest.raises(idahip.IdaHipError, match=r"\(-2\)"):
            idahip.Ctx("mass_action", n_bad, 2)
        assert ("IDAHIP_MASS_ACTION: n = %d outside" % n_bad) in capfd.readouterr().err
    heat = idahip.Ctx("heat1d", 16, 2)
    with pytest.raises(idahip.IdaHipError, match=r"not an IDAHIP_MASS_ACTION ctx"):
        heat.set_mass_action(problems.bruss1d_network(8, 2)["reactions"], np.ones(16))
    with pytest.raises(idahip.IdaHipError, match=r"not an IDAHIP_MASS_ACTION ctx"):
        heat.mass_action_pattern()
    heat.set_problem_params(np.ones((2, 1)))  # (and the heat ctx goes on working)
    heat.close()
