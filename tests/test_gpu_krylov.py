"""The Krylov ctx (idahip_create_krylov: matrix-free SPGMR) on the device against tests/krylov_ref.py, bit for
bit: idahip_krylov_solve on the case list of tests/krylov_cases.py (the census list: every flag except QRSOL_FAIL is met), fused and
split path, heat / linear dense / a host-callback residual; idahip_newton_iter_krylov; whole integrations on the host stepper; and
every refusal."""
import ctypes as C

import numpy as np
import pytest

import krylov_cases as K
import krylov_ref as KR
import oracle_lib as O

pytestmark = pytest.mark.gpu
F_YY, F_YP, F_YYPREDICT, F_YPPREDICT, F_EWT, F_EE, F_DELTA, F_SAVRES = range(8)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def make_ctx(c, maxl, host=False):
    """A Krylov ctx of the case's problem with the case's state in its fields."""
    import idahip
    from idahip import problems
    prob = c["prob"]
    if host:
        res = [KR.make_res(prob, s) for s in range(prob["yy0"].shape[0])]
        ctx = idahip.Ctx("host_callback", prob["n"], prob["yy0"].shape[0], krylov=maxl)
        ctx.set_tolerances(prob["rtol"], prob["atol"])
        ctx.set_host_residual(lambda s, t, y, yp: res[s](t, y, yp))
    else:
        ctx = problems.make_ctx(prob, krylov=maxl)
    for f, k in ((F_YY, "yy"), (F_YP, "yp"), (F_EWT, "ewt"), (F_SAVRES, "savres")):
        ctx.upload(f, c[k])
    return ctx


def check_solve(ctx, c, ref, idx):
    x, nli, flag, rn = ctx.krylov_solve(c["tn"][idx], c["cj"][idx], c["tol"][idx], c["b"][idx], idx=idx)
    for q, s in enumerate(idx):
        r = ref[s]
        assert (nli[q], flag[q]) == (r["nli"], r["flag"]), (s, nli[q], flag[q], r["nli"], r["flag"])
        assert bits(rn[q]) == bits(r["res_norm"]), (s, rn[q], r["res_norm"])
        assert np.array_equal(bits(x[q]), bits(r["x"])), (s, np.abs(x[q] - r["x"]).max())
    assert ctx.ls_type() == 1 and ctx.ls_num_iters() == int(nli.sum()) and ctx.ls_res_norm() == rn.max()


@pytest.mark.parametrize("kind,n,maxl", K.solve_cases(), ids=lambda v: str(v))
def test_krylov_solve_fused_and_split(kind, n, maxl):
    c, ref, _ = K.solve_reference(kind, n, maxl)
    idx = K.idx_for(maxl)
    ctx = make_ctx(c, maxl)
    assert ctx.krylov == maxl and ctx.krylov_fused()
    check_solve(ctx, c, ref, idx)
    ctx.set_krylov_fused(False)
    assert not ctx.krylov_fused()
    check_solve(ctx, c, ref, idx)
    ctx.close()


@pytest.mark.parametrize("kind,n,maxl", K.solve_cases(), ids=lambda v: str(v))
def test_krylov_solve_host_callback_residual(kind, n, maxl):
    c, ref, _ = K.solve_reference(kind, n, maxl)
    ctx = make_ctx(c, maxl, host=True)
    assert not ctx.krylov_fused()
    check_solve(ctx, c, ref, K.idx_for(maxl))
    ctx.close()


def test_krylov_solve_heat_4096_lds_size():
    """n = 4096, B = 3, maxl = 5: the largest LDS request of the fused kernel."""
    import idahip
    from idahip import problems
    n, B, maxl = 4096, 3, 5
    prob = problems.heat1d(n=n, batch=B)
    rng = np.random.Generator(np.random.PCG64(4096))
    yy = prob["yy0"] + 1.0e-3 * rng.uniform(-1.0, 1.0, size=(B, n))
    yp = prob["yp0"].copy()
    ewt = 1.0 / (prob["rtol"] * np.abs(yy) + prob["atol"][0])
    tn, cj = np.array([0.01, 0.02, 0.03]), np.array([1.0e3, 1.0e5, 1.0e7])
    b = rng.uniform(-1.0, 1.0, size=(B, n)) / ewt
    tol = np.array([KR.eplin(n, 0.33), 40.0, 1.0e-3])
    res = [KR.make_res(prob, s) for s in range(B)]
    savres = np.stack([res[s](tn[s], yy[s], yp[s]) for s in range(B)])
    ref = [KR.spgmr_solve(res[s], b[s], ewt[s], yy[s], yp[s], savres[s], tn[s], cj[s], tol[s], maxl) for s in range(B)]
    c = {"prob": prob, "yy": yy, "yp": yp, "ewt": ewt, "savres": savres, "tn": tn, "cj": cj, "tol": tol, "b": b}
    ctx = make_ctx(c, maxl)
    idx = np.array([2, 0, 1], dtype=np.int32)
    check_solve(ctx, c, ref, idx)
    ctx.set_krylov_fused(False)
    check_solve(ctx, c, ref, idx)
    ctx.close()


@pytest.mark.parametrize("kind,n,maxl,fused", [("heat1d", 65, 5, True), ("heat1d", 65, 1, False), ("linear_dense", 63, 16, True),
                                                ("linear_dense", 300, 16, False)], ids=lambda v: str(v))
def test_newton_iter_krylov(kind, n, maxl, fused):
    """delta = -delta, the solve with tol from eps_newt, ee += delta and the norm for flag 0; ee untouched where the flag is not 0."""
    c, _, _ = K.solve_reference(kind, n, maxl)
    prob = c["prob"]
    rng = np.random.Generator(np.random.PCG64(n))
    ee0 = 1.0e-4 * rng.uniform(-1.0, 1.0, size=(K.B, n))
    # eps_newt such that the tolerance is the case's tol: the flags of the case list come back
    eps = c["tol"] / (np.sqrt(float(n)) * 0.05)
    idx = K.idx_for(maxl)
    ctx = make_ctx(c, maxl)
    ctx.set_krylov_fused(fused)
    ctx.upload(F_EE, ee0)
    ctx.upload(F_DELTA, -c["b"])
    nrm, nli, flag = ctx.newton_iter_krylov(c["tn"][idx], c["cj"][idx], eps[idx], idx=idx)
    ee, delta = ctx.download(F_EE), ctx.download(F_DELTA)
    flags = set()
    for q, s in enumerate(idx):
        d, e, dn, rl, rf = KR.newton_iter_krylov(KR.make_res(prob, s), -c["b"][s], ee0[s], c["ewt"][s], c["yy"][s], c["yp"][s],
                                                 c["savres"][s], c["tn"][s], c["cj"][s], eps[s], maxl)
        assert (nli[q], flag[q]) == (rl, rf) and bits(nrm[q]) == bits(dn), (s, nli[q], flag[q], rl, rf, nrm[q], dn)
        assert np.array_equal(bits(ee[s]), bits(e)) and np.array_equal(bits(delta[s]), bits(d)), s
        if rf != 0:
            assert np.array_equal(bits(ee[s]), bits(ee0[s])) and nrm[q] == 0.0
        flags.add(rf)
    rest = [s for s in range(K.B) if s not in idx]
    assert np.array_equal(bits(ee[rest]), bits(ee0[rest])) and np.array_equal(bits(delta[rest]), bits(-c["b"][rest]))
    assert 0 in flags and len(flags) > 1, flags
    ctx.close()


def test_refusals_on_a_krylov_ctx():
    import idahip
    H, _ = idahip.load()
    dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    h = C.c_void_p()
    # creation: n <= 8, n > 4096, maxl > 16, maxl > n, a kind without a Krylov form
    for n, maxl, kind in ((8, 5, 3), (4097, 5, 3), (64, 17, 3), (9, 10, 3), (3, 1, 0)):
        assert H.idahip_create_krylov(C.byref(h), 0, n, 2, kind, None, maxl) == -2 and not h.value
    n, Bn = 12, 3
    ctx = idahip.Ctx("heat1d", n, Bn, krylov=0)
    assert ctx.krylov == 5 and ctx.ls_type() == 1
    one = np.ones(Bn)
    vec = np.ones((Bn, n))
    info = np.zeros(Bn, dtype=np.int32)
    i64 = np.zeros(n, dtype=np.int64)
    idx = np.arange(Bn, dtype=np.int32)
    d, ip, xp = one.ctypes.data_as(dp), info.ctypes.data_as(i32p), idx.ctypes.data_as(i32p)
    v = vec.ctypes.data_as(dp)
    before = ctx.timing_get()
    calls = {
        "idahip_ls_setup": lambda: H.idahip_ls_setup(ctx.h, C.cast(v, C.c_void_p), C.cast(v, C.c_void_p), ip, xp, Bn),
        "idahip_nls_lsetup": lambda: H.idahip_nls_lsetup(ctx.h, d, d, ip, xp, Bn),
        "idahip_nls_lsetup_dq": lambda: H.idahip_nls_lsetup_dq(ctx.h, d, d, d, ip, xp, Bn),
        "idahip_nls_sys_setup": lambda: H.idahip_nls_sys_setup(ctx.h, d, d, 1, ip, xp, Bn),
        "idahip_newton_iter": lambda: H.idahip_newton_iter(ctx.h, d, d, xp, Bn),
        "idahip_newton_iter2": lambda: H.idahip_newton_iter2(ctx.h, d, d, d, d, d, d, v, ip, xp, Bn),
        "idahip_download_lu": lambda: H.idahip_download_lu(ctx.h, 0, v, i64.ctypes.data_as(C.POINTER(C.c_int64))),
        "idahip_download_lu_band": lambda: H.idahip_download_lu_band(ctx.h, 0, v, i64.ctypes.data_as(C.POINTER(C.c_int64))),
        "idahip_set_jacobian_dq": lambda: H.idahip_set_jacobian_dq(ctx.h, 1),
        "idahip_set_constraints": lambda: H.idahip_set_constraints(ctx.h, v),
        "idahip_ic_begin": lambda: H.idahip_ic_begin(ctx.h, d, ip, xp, Bn),
        "idahip_ic_reset": lambda: H.idahip_ic_reset(ctx.h, xp, Bn),
        "idahip_ic_res": lambda: H.idahip_ic_res(ctx.h, d, d, xp, Bn),
        "idahip_ic_setup": lambda: H.idahip_ic_setup(ctx.h, d, d, ip, xp, Bn),
        "idahip_ic_setup_dq": lambda: H.idahip_ic_setup_dq(ctx.h, d, d, d, ip, xp, Bn),
        "idahip_ic_solve": lambda: H.idahip_ic_solve(ctx.h, d, xp, Bn),
        "idahip_ic_trial": lambda: H.idahip_ic_trial(ctx.h, 2, d, d, d, d, xp, Bn),
        "idahip_ic_accept": lambda: H.idahip_ic_accept(ctx.h, 2, xp, Bn),
        "idahip_ic_commit": lambda: H.idahip_ic_commit(ctx.h, ip, xp, Bn),
    }
    for name, call in calls.items():
        assert call() == -2, name
        assert name in H.idahip_last_error(ctx.h).decode(), (name, H.idahip_last_error(ctx.h))
    P = C.CDLL(idahip.LIB_HIP)  # a handle of this test's own: the argument types set here do not reach the shared one
    P.idahip_round_solve.argtypes = [C.c_void_p] * 9
    assert P.idahip_round_solve(ctx.h, None, 0, None, None, None, None, None, None) == -2
    assert "idahip_round_solve" in H.idahip_last_error(ctx.h).decode()
    assert ctx.timing_get() == before, "a refused call launches nothing"
    assert H.idahip_set_jacobian_dq(ctx.h, 0) == 0
    ctx.close()
    # a host-callback Krylov ctx takes a residual only, and runs the split path only
    hc = idahip.Ctx("host_callback", n, Bn, krylov=3)
    res = idahip.RES_FN(lambda *a: 0)
    jac = idahip.JAC_FN(lambda *a: 0)
    assert H.idahip_set_host_problem(hc.h, res, jac, None) == -2 and "idahip_set_host_problem" in H.idahip_last_error(hc.h).decode()
    assert H.idahip_set_krylov_fused(hc.h, 1) == -2 and not hc.krylov_fused()
    assert H.idahip_set_host_residual(hc.h, res, None) == 0 and not hc.jacobian_dq()
    hc.close()
    # the solve calls on a ctx that is not a Krylov ctx; idahip_ls_type there
    dn = idahip.Ctx("heat1d", n, Bn)
    assert dn.krylov is None and dn.ls_type() == 0 and dn.ls_num_iters() == 0
    nl = np.zeros(Bn, dtype=np.int32)
    assert H.idahip_krylov_solve(dn.h, d, d, d, v, v, nl.ctypes.data_as(i32p), ip, d, xp, Bn) == -2
    assert H.idahip_newton_iter_krylov(dn.h, d, d, d, d, nl.ctypes.data_as(i32p), ip, xp, Bn) == -2
    assert H.idahip_set_krylov_fused(dn.h, 0) == -2
    dn.close()


# ------------------------------------------------------------------------------------------------ the host stepper on a Krylov ctx
STEP_CNT = ("nst", "nre", "nre_dq", "nsetups", "nje", "nni", "nli", "ncfl", "ncfn", "netf")


def step_ensemble(p, maxl, fused):
    import idahip
    from idahip import problems
    ctx = problems.make_ctx(p, krylov=maxl)
    ctx.set_krylov_fused(fused)
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    assert ens.device_controller_active() == 0
    return ctx, ens


def check_state(ens, ref, i):
    c = ens.counters()
    for k in STEP_CNT:
        assert np.array_equal(c[k], ref["counters"][k][i]), (k, i, c[k], ref["counters"][k][i])
    assert np.array_equal(c["kused"], ref["kused"][i])
    assert np.array_equal(bits(ens.real("hused")), bits(ref["hused"][i])) and np.array_equal(bits(ens.real("tn")), bits(ref["tn"][i]))
    assert np.array_equal(bits(ens.yy()), bits(ref["yy"][i])) and np.array_equal(bits(ens.yp()), bits(ref["yp"][i]))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "split"])
@pytest.mark.parametrize("kind,n,maxl", K.STEP_CASES, ids=lambda v: str(v))
def test_host_stepper_integrations(kind, n, maxl, fused):
    """Per system and at every output: every counter, kused, hused, tn, yy, yp -- bit for bit against the restated stepper."""
    p, ref = K.step_reference(kind, n, maxl)
    ctx, ens = step_ensemble(p, maxl, fused)
    for i, t in enumerate(p["touts"]):
        status, tret = ens.solve(float(t))
        assert np.array_equal(status, ref["status"][i]), (i, status, ref["status"][i])
        assert np.array_equal(bits(tret), bits(ref["tret"][i]))
        check_state(ens, ref, i)
    if (kind, n) == ("heat1d", 65):  # linear convergence failures that the stepper recovered from (asserted from the reference's census)
        last = ref["counters"]["ncfl"][-1]
        assert (ref["status"] == 0).all() and (last > 0).sum() >= 3 and np.array_equal(ens.counter("ncfl"), last)
        assert sum(c["res_reduced"] + c["conv_fail"] for c in ref["census"]) == last.sum()
    ens.close()
    ctx.close()


def test_host_stepper_schedule_and_stream():
    kind, n, maxl = "heat1d", 65, 5
    p, ref = K.step_reference(kind, n, maxl)
    ctx, ens = step_ensemble(p, maxl, True)
    status, tret, reached = ens.solve_schedule(p["touts"])
    assert (status == 0).all() and (reached == len(p["touts"])).all() and np.array_equal(bits(tret), bits(ref["tret"][-1]))
    check_state(ens, ref, len(p["touts"]) - 1)
    ens.close()
    ctx.close()
    # Throughput mode: finished systems start over. This part is a SELF-COMPARISON, not a comparison with krylov_ref: the restated
    # stepper (RefIda) runs one system's whole Ida::solve call at a time, while idaens_stream cuts the integrations into lock-step
    # rounds of one attempt each and recreates a finished system inside the same call, so its state after R rounds is that of an
    # integration stopped in mid-schedule, which the reference loop has no seam for. What the stream adds to the solve and schedule
    # cases above (both pinned on krylov_ref) is the recycling, which never touches the linear solver; the check here is that the
    # fused and the split path leave the same state after the same rounds and that the Krylov branch ran in them.
    out = []
    for fused in (True, False):
        ctx, ens = step_ensemble(p, maxl, fused)
        done = ens.stream(p["touts"], 40)
        out.append((done, ens.counters(), ens.yy(), ens.real("tn"), ens.total_newton_iters()))
        ens.close()
        ctx.close()
    (d0, c0, y0, t0, it0), (d1, c1, y1, t1, it1) = out
    assert d0 == d1 and d0 > 0 and it0 == it1 and np.array_equal(bits(y0), bits(y1)) and np.array_equal(bits(t0), bits(t1))
    for k in c0:
        assert np.array_equal(c0[k], c1[k]), k
    assert c0["nli"].sum() > 0 and not c0["nje"].any()


def test_calc_ic_is_refused_and_a_dense_ctx_is_unchanged():
    import idahip
    from idahip import problems
    p = K.step_problem("heat1d", 16)
    ctx, ens = step_ensemble(p, 5, True)
    with pytest.raises(idahip.IdaHipError, match="Krylov"):
        ens.calc_ic(idahip.Y_INIT, 0.001)
    ens.set_fused_newton(1)  # stays off on a Krylov ctx: the solve below still runs the Krylov Newton body
    status, _ = ens.solve(float(p["touts"][0]))
    assert (status == 0).all() and ens.counter("nli").sum() > 0
    ens.close()
    ctx.close()
    dn = problems.make_ctx(p)
    assert dn.ls_type() == 0 and dn.krylov is None
    e2 = idahip.Ensemble(dn, p["yy0"], p["yp0"])
    status, _ = e2.solve(float(p["touts"][0]))
    assert (status == 0).all() and not e2.counter("nli").any() and e2.counter("nje").sum() > 0
    e2.close()
    dn.close()
