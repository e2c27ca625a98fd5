"""The band preconditioner of a Krylov ctx and the left-preconditioned SPGMR solve on the device against
tests/krylov_prec_ref.py: psetup, psolve, the solve (fused and split, heat and a host-callback residual, factors from psetup and
uploaded ones), the Newton body, the host stepper, and every refusal. The band kernels equal the dense LU by value (-0.0 == +0.0), so
the comparison with the numpy restatement is by value (np.array_equal); two device paths that run the same device functions are
compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import band_problems as BP
import dq_ref as DQ
import krylov_cases as K
import krylov_prec_ref as PR
import krylov_ref as KR

pytestmark = pytest.mark.gpu
F_YY, F_YP, F_YYPREDICT, F_YPPREDICT, F_EWT, F_EE, F_DELTA, F_SAVRES = range(8)
HH = 1.0e-3
ALL = np.array([2, 4, 0, 1, 3], dtype=np.int32)  # every recipe of krylov_cases, reordered


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def make_ctx(c, maxl, width, host=False):
    """A Krylov ctx of the case's heat problem with the case's state in its fields and the band preconditioner on."""
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
    if width is not None:
        ctx.set_krylov_band_prec(*width)
        assert ctx.krylov_band_prec() == tuple(width)
    return ctx


# ------------------------------------------------------------------------------------------------ psetup
def ref_psetup(c, s, ml, mu, cj=None):
    res = KR.make_res(c["prob"], s)
    tn = c["tn"][s]
    return PR.psetup(lambda y, yp: res(tn, y, yp), c["yy"][s], c["yp"][s], c["ewt"][s], c["savres"][s], c["cj"][s] if cj is None else cj,
                     HH, ml, mu)


@pytest.mark.parametrize("width", [(1, 1), (0, 0), (2, 1), (3, 5)], ids=str)
@pytest.mark.parametrize("n", [9, 64, 65, 300])
def test_psetup_heat(n, width):
    ml, mu = width
    c = K.solve_inputs("heat1d", n, 5)
    ctx = make_ctx(c, 5, width)
    idx = np.array([3, 0, 4, 2], dtype=np.int32)  # system 1 gets no preconditioner
    info = ctx.krylov_psetup(c["tn"][idx], c["cj"][idx], HH, idx=idx)
    assert not info.any(), info
    for s in idx:
        ri, rab, rpiv = ref_psetup(c, s, ml, mu)
        ab, piv = ctx.krylov_download_prec(int(s))
        assert ri == 0 and np.array_equal(piv, rpiv), s
        assert np.array_equal(ab, rab), (s, np.abs(ab - rab).max())
    ab, piv = ctx.krylov_download_prec(1)
    assert not ab.any() and not piv.any()
    ctx.close()


def test_psetup_reports_a_singular_preconditioner():
    """cj = 0: system 3 (heat coefficient 0) has an all-zero interior and stops at the reference's column; the others factor."""
    n = 65
    c = K.solve_inputs("heat1d", n, 5)
    ctx = make_ctx(c, 5, (1, 1))
    info = ctx.krylov_psetup(c["tn"], 0.0, HH)
    want = [ref_psetup(c, s, 1, 1, cj=0.0)[0] for s in range(K.B)]
    assert want[3] != 0 and not any(want[s] for s in (0, 1, 2, 4))
    assert info.tolist() == want
    ctx.close()


def banded_state(n, ml, mu, B=5):
    prob = BP.banded_linear(n, ml, mu, B)
    rng = np.random.Generator(np.random.PCG64(7 * n + ml))
    yy = prob["yy0"] + 1.0e-2 * rng.uniform(-1.0, 1.0, size=(B, n))
    yp = prob["yp0"] + 1.0e-2 * rng.uniform(-1.0, 1.0, size=(B, n))
    ewt = 1.0 / (prob["rtol"] * np.abs(yy) + prob["atol"][0])
    res = [(lambda y, ypv, s=s: DQ.linear_res(prob["A"][s], prob["B"][s], prob["c"][s], y, ypv)) for s in range(B)]
    savres = np.stack([res[s](yy[s], yp[s]) for s in range(B)])
    return prob, yy, yp, ewt, savres, res


def test_psetup_host_callback_with_swaps_and_fill():
    import idahip
    n, ml, mu, B = 64, 3, 5, 5
    prob, yy, yp, ewt, savres, res = banded_state(n, ml, mu, B)
    ctx = idahip.Ctx("host_callback", n, B, krylov=5)
    ctx.set_tolerances(prob["rtol"], prob["atol"])
    ctx.set_host_residual(lambda s, t, y, ypv: res[s](y, ypv))
    for f, v in ((F_YY, yy), (F_YP, yp), (F_EWT, ewt), (F_SAVRES, savres)):
        ctx.upload(f, v)
    ctx.set_krylov_band_prec(ml, mu)
    cj = 10.0 * (1.0 + np.arange(B))
    idx = np.array([4, 1, 0, 3, 2], dtype=np.int32)
    info = ctx.krylov_psetup(0.1, cj[idx], HH, idx=idx)
    assert not info.any()
    swaps = fill = 0
    for s in range(B):
        ri, rab, rpiv = PR.psetup(res[s], yy[s], yp[s], ewt[s], savres[s], cj[s], HH, ml, mu)
        ab, piv = ctx.krylov_download_prec(s)
        assert ri == 0 and np.array_equal(piv, rpiv) and np.array_equal(ab, rab), s
        swaps += int((rpiv != np.arange(n)).sum())
        fill += int(np.count_nonzero(rab[:, :ml]))
    assert swaps > 0 and fill > 0
    ctx.close()


# ------------------------------------------------------------------------------------------------ psolve
def banded_factors(n, ml, mu, B=5):
    import idahip
    prob = BP.banded_linear(n, ml, mu, B)
    facs = []
    for s in range(B):
        info, ab, piv = PR.band_getrf(idahip.band_pack(BP.jacobian(prob, s, 30.0 * (1 + s)).T, ml, mu), n, ml, mu)
        assert info == 0
        facs.append((ab, piv))
    return facs


@pytest.mark.parametrize("host", [False, True], ids=["heat", "host_callback"])
@pytest.mark.parametrize("n,ml,mu", [(65, 1, 1), (65, 0, 0), (65, 3, 5), (257, 70, 70)], ids=str)
def test_psolve_equals_ls_solve_band_bitwise_and_the_reference_by_value(n, ml, mu, host):
    import idahip
    B = 5
    facs = banded_factors(n, ml, mu, B)
    ctx = idahip.Ctx("host_callback" if host else "heat1d", n, B, krylov=5)
    ctx.set_krylov_band_prec(ml, mu)
    for s in range(B):
        ctx.krylov_upload_prec(s, *facs[s])
        ab, piv = ctx.krylov_download_prec(s)
        assert np.array_equal(bits(ab), bits(facs[s][0])) and np.array_equal(piv, facs[s][1])
    rng = np.random.Generator(np.random.PCG64(n + ml))
    r = rng.uniform(-1.0, 1.0, size=(B, n)) * 10.0 ** rng.uniform(-3, 3, size=(B, n))
    idx = np.array([3, 0, 4, 1], dtype=np.int32)
    z = ctx.krylov_psolve(r[idx], idx=idx)
    dA, dP = ctx.dev_array(np.stack([f[0] for f in facs])), ctx.dev_array(np.stack([f[1] for f in facs]))
    dB, dX = ctx.dev_array(r), ctx.dev_array(np.zeros((B, n)))
    ctx.ls_solve_band(ml, mu, dA, dP, dX, dB, idx)
    x = ctx.to_host(dX, (B, n))
    for d in (dA, dP, dB, dX):
        ctx.dev_free(d)
    swaps = 0
    for q, s in enumerate(idx):
        assert np.array_equal(bits(z[q]), bits(x[s])), (s, np.abs(z[q] - x[s]).max())
        assert np.array_equal(z[q], PR.band_getrs(facs[s][0], facs[s][1], n, ml, mu, r[s])), s
        swaps += int((facs[s][1] != np.arange(n)).sum())
    assert swaps > 0 or ml == 0
    ctx.close()


# ------------------------------------------------------------------------------------------------ the solve
def check_solve(ctx, c, ref, idx):
    """-> (x, nli, flag, res_norm) after the comparison with the reference by value."""
    x, nli, flag, rn = ctx.krylov_solve(c["tn"][idx], c["cj"][idx], c["tol"][idx], c["b"][idx], idx=idx)
    for q, s in enumerate(idx):
        r = ref[s]
        assert (nli[q], flag[q]) == (r["nli"], r["flag"]), (s, nli[q], flag[q], r["nli"], r["flag"])
        assert rn[q] == r["res_norm"], (s, rn[q], r["res_norm"])
        assert np.array_equal(x[q], r["x"]), (s, np.abs(x[q] - r["x"]).max())
    assert ctx.ls_num_iters() == int(nli.sum()) and ctx.ls_res_norm() == rn.max()
    return x, nli, flag, rn


def same_bits(a, b):
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(bits(a[3]), bits(b[3]))


@pytest.mark.parametrize("width", [(1, 1), (0, 0)], ids=str)
@pytest.mark.parametrize("n,maxl", [(n, m) for n in K.NS for m in K.MAXLS if m <= n], ids=str)
def test_preconditioned_solve_fused_and_split(n, maxl, width):
    c, facs, ref, _ = PR.solve_reference(n, maxl, *width, hh=HH)
    ctx = make_ctx(c, maxl, width)
    assert ctx.krylov_fused()
    assert not ctx.krylov_psetup(c["tn"], c["cj"], HH).any()
    fused = check_solve(ctx, c, ref, ALL)
    ctx.set_krylov_fused(False)
    split = check_solve(ctx, c, ref, ALL)
    same_bits(fused, split)
    ctx.close()


def uploaded_case(n=65, maxl=5, ml=3, mu=5):
    """The heat case with pivoting factors of banded_linear's Jacobians as the user-supplied preconditioner."""
    c = K.solve_inputs("heat1d", n, maxl)
    facs = banded_factors(n, ml, mu, K.B)
    assert sum(int((f[1] != np.arange(n)).sum()) for f in facs) > 0
    ref = []
    for s in range(K.B):
        ab, piv = facs[s]
        ref.append(PR.spgmr_solve_prec(KR.make_res(c["prob"], s), lambda v: PR.band_getrs(ab, piv, n, ml, mu, v), c["b"][s], c["ewt"][s],
                                       c["yy"][s], c["yp"][s], c["savres"][s], c["tn"][s], c["cj"][s], c["tol"][s], maxl))
    return c, facs, ref


def test_solve_with_uploaded_pivoting_factors():
    n, maxl, ml, mu = 65, 5, 3, 5
    c, facs, ref = uploaded_case(n, maxl, ml, mu)
    ctx = make_ctx(c, maxl, (ml, mu))
    for s in range(K.B):
        ctx.krylov_upload_prec(s, *facs[s])
    fused = check_solve(ctx, c, ref, ALL)
    ctx.set_krylov_fused(False)
    split = check_solve(ctx, c, ref, ALL)
    same_bits(fused, split)
    assert max(r["nli"] for r in ref) >= 2  # psolve ran inside an iteration l >= 1
    ctx.close()
    hc = make_ctx(c, maxl, (ml, mu), host=True)
    for s in range(K.B):
        hc.krylov_upload_prec(s, *facs[s])
    assert not hc.krylov_fused()
    same_bits(check_solve(hc, c, ref, ALL), split)
    hc.close()


def test_solve_heat_4096_lds_size_still_launches():
    """n = 4096, (1, 1), maxl = 5, B = 2: the fused kernel's LDS request is what it is without a preconditioner."""
    from idahip import problems
    n, B, maxl = 4096, 2, 5
    prob = problems.heat1d(n=n, batch=B)
    rng = np.random.Generator(np.random.PCG64(4096))
    yy = prob["yy0"] + 1.0e-3 * rng.uniform(-1.0, 1.0, size=(B, n))
    yp = prob["yp0"].copy()
    ewt = 1.0 / (prob["rtol"] * np.abs(yy) + prob["atol"][0])
    tn, cj = np.array([0.01, 0.02]), np.array([1.0e3, 1.0e5])
    b = rng.uniform(-1.0, 1.0, size=(B, n)) / ewt
    tol = np.array([KR.eplin(n, 0.33), 1.0e-3])
    res = [KR.make_res(prob, s) for s in range(B)]
    savres = np.stack([res[s](tn[s], yy[s], yp[s]) for s in range(B)])
    c = {"prob": prob, "yy": yy, "yp": yp, "ewt": ewt, "savres": savres, "tn": tn, "cj": cj, "tol": tol, "b": b}
    ref = []
    for s in range(B):
        info, ab, piv = PR.psetup(lambda y, ypv, s=s: res[s](tn[s], y, ypv), yy[s], yp[s], ewt[s], savres[s], cj[s], HH, 1, 1)
        assert info == 0
        ref.append(PR.spgmr_solve_prec(res[s], lambda v: PR.band_getrs(ab, piv, n, 1, 1, v), b[s], ewt[s], yy[s], yp[s], savres[s],
                                       tn[s], cj[s], tol[s], maxl))
    ctx = make_ctx(c, maxl, (1, 1))
    assert not ctx.krylov_psetup(tn, cj, HH).any()
    check_solve(ctx, c, ref, np.array([1, 0], dtype=np.int32))
    assert max(r["nli"] for r in ref) >= 1
    ctx.close()


# ------------------------------------------------------------------------------------------------ the Newton body
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "split"])
@pytest.mark.parametrize("maxl", [1, 5])
def test_newton_iter_krylov_preconditioned(maxl, fused):
    """n = 65, (0, 0): system 1 returns at once (delta = P^-1 (-res)); system 0 ends in RES_REDUCED with maxl = 1 (ee untouched, delta
    the negated residual) and converges after three iterations with maxl = 5."""
    n, width = 65, (0, 0)
    c, facs, _, _ = PR.solve_reference(n, maxl, *width, hh=HH)
    prob = c["prob"]
    rng = np.random.Generator(np.random.PCG64(n))
    ee0 = 1.0e-4 * rng.uniform(-1.0, 1.0, size=(K.B, n))
    eps = c["tol"] / (np.sqrt(float(n)) * 0.05)
    idx = np.array([4, 0, 3, 1], dtype=np.int32)
    ctx = make_ctx(c, maxl, width)
    ctx.set_krylov_fused(fused)
    assert not ctx.krylov_psetup(c["tn"], c["cj"], HH).any()
    ctx.upload(F_EE, ee0)
    ctx.upload(F_DELTA, -c["b"])
    nrm, nli, flag = ctx.newton_iter_krylov(c["tn"][idx], c["cj"][idx], eps[idx], idx=idx)
    ee, delta = ctx.download(F_EE), ctx.download(F_DELTA)
    seen = set()
    for q, s in enumerate(idx):
        psolve = lambda v, s=s: PR.band_getrs(facs[s][1], facs[s][2], n, 0, 0, v)
        d, e, dn, rl, rf = PR.newton_iter_krylov_prec(KR.make_res(prob, s), psolve, -c["b"][s], ee0[s], c["ewt"][s], c["yy"][s],
                                                      c["yp"][s], c["savres"][s], c["tn"][s], c["cj"][s], eps[s], maxl)
        assert (nli[q], flag[q]) == (rl, rf) and nrm[q] == dn, (s, nli[q], flag[q], rl, rf, nrm[q], dn)
        assert np.array_equal(ee[s], e) and np.array_equal(delta[s], d), s
        if rf != 0:
            assert np.array_equal(bits(ee[s]), bits(ee0[s])) and nrm[q] == 0.0 and np.array_equal(bits(delta[s]), bits(c["b"][s]))
        if rl == 0:
            assert rf == 0 and np.array_equal(delta[s], psolve(c["b"][s])) and not np.array_equal(delta[s], c["b"][s])
        seen.add((rl == 0, rf != 0))
    assert (True, False) in seen and ((False, True) if maxl == 1 else (False, False)) in seen, seen
    assert np.array_equal(bits(ee[2]), bits(ee0[2])) and np.array_equal(bits(delta[2]), bits(-c["b"][2]))
    ctx.close()


# ------------------------------------------------------------------------------------------------ the host stepper
STEP_CNT = ("nst", "nre", "nre_dq", "nsetups", "nje", "nni", "nli", "ncfl", "ncfn", "netf", "npe", "nps")


def step_ensemble(p, fused, width=PR.STEP_WIDTH):
    import idahip
    from idahip import problems
    ctx = problems.make_ctx(p, krylov=PR.STEP_MAXL)
    ctx.set_krylov_fused(fused)
    if width is not None:
        ctx.set_krylov_band_prec(*width)
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    assert ens.device_controller_active() == 0
    return ctx, ens


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "split"])
def test_host_stepper_integration_with_the_preconditioner(fused):
    """The integration of test_krylov_prec_ref.py: per system and at every output every counter, kused exactly; hused, tn, yy, yp by
    value."""
    p, ref = PR.step_reference()
    ctx, ens = step_ensemble(p, fused)
    for i, t in enumerate(p["touts"]):
        status, tret = ens.solve(float(t))
        assert np.array_equal(status, ref["status"][i]), (i, status, ref["status"][i])
        assert np.array_equal(tret, ref["tret"][i])
        c = ens.counters()
        for k in STEP_CNT:
            assert np.array_equal(c[k], ref["counters"][k][i]), (k, i, c[k], ref["counters"][k][i])
        assert np.array_equal(c["kused"], ref["kused"][i])
        assert np.array_equal(ens.real("hused"), ref["hused"][i]) and np.array_equal(ens.real("tn"), ref["tn"][i])
        assert np.array_equal(ens.yy(), ref["yy"][i]) and np.array_equal(ens.yp(), ref["yp"][i])
    assert (ref["status"] == 0).all() and not ens.counter("ncfl").any() and not ens.counter("nlufail").any()
    assert (ens.counter("npe") > 0).all() and np.array_equal(ens.counter("nps"), ens.counter("nni") + ens.counter("nli"))
    ens.close()
    ctx.close()


def test_host_stepper_stream_fused_against_split():
    """idaens_stream recycles finished systems inside one call: a self-comparison of the two device paths, as section 4h has."""
    p, _ = PR.step_reference()
    out = []
    for fused in (True, False):
        ctx, ens = step_ensemble(p, fused)
        done = ens.stream(p["touts"], 40)
        out.append((done, ens.counters(), ens.yy(), ens.real("tn"), ens.total_newton_iters()))
        ens.close()
        ctx.close()
    (d0, c0, y0, t0, it0), (d1, c1, y1, t1, it1) = out
    assert d0 == d1 and d0 > 0 and it0 == it1 and np.array_equal(bits(y0), bits(y1)) and np.array_equal(bits(t0), bits(t1))
    for k in c0:
        assert np.array_equal(c0[k], c1[k]), k
    assert c0["npe"].sum() > 0 and c0["nps"].sum() > 0 and not c0["nje"].any()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_and_the_plain_krylov_ctx_is_unchanged():
    import idahip
    from idahip import problems
    H, _ = idahip.load()
    n, maxl = 65, 5
    c, ref, _ = K.solve_reference("heat1d", n, maxl)
    idx = K.idx_for(maxl)

    def plain_solve(ctx):
        x, nli, flag, rn = ctx.krylov_solve(c["tn"][idx], c["cj"][idx], c["tol"][idx], c["b"][idx], idx=idx)
        for q, s in enumerate(idx):
            assert (nli[q], flag[q]) == (ref[s]["nli"], ref[s]["flag"]) and bits(rn[q]) == bits(ref[s]["res_norm"])
            assert np.array_equal(bits(x[q]), bits(ref[s]["x"]))

    def refused(call, word):
        with pytest.raises(idahip.IdaHipError, match=word):
            call()

    ctx = make_ctx(c, maxl, None)
    assert ctx.krylov_band_prec() is None
    # the stand-alone calls with the mode off
    before = ctx.timing_get()
    refused(lambda: ctx.krylov_psetup(c["tn"], c["cj"], HH), "idahip_krylov_psetup")
    refused(lambda: ctx.krylov_psolve(c["b"]), "idahip_krylov_psolve")
    refused(lambda: ctx.krylov_download_prec(0), "idahip_krylov_download_prec")
    refused(lambda: ctx.krylov_upload_prec(0, np.zeros((n, 4)), np.arange(n)), "idahip_krylov_upload_prec")
    # widths out of range
    for ml, mu in ((n, 0), (0, n), (-1, 0), (0, -1), (-2, -2)):
        refused(lambda: ctx.set_krylov_band_prec(ml, mu), "bandwidths")
        assert ctx.krylov_band_prec() is None
    assert ctx.timing_get() == before, "a refused call launches nothing"
    plain_solve(ctx)  # the plain ctx computes what it computed before, bit for bit
    # a solve before any psetup or upload; then only the systems that have factors
    ctx.set_krylov_band_prec(1, 1)
    before = ctx.timing_get()
    refused(lambda: ctx.krylov_solve(c["tn"][idx], c["cj"][idx], c["tol"][idx], c["b"][idx], idx=idx), "no preconditioner yet")
    refused(lambda: ctx.newton_iter_krylov(c["tn"][idx], c["cj"][idx], 0.33, idx=idx), "no preconditioner yet")
    refused(lambda: ctx.krylov_psolve(c["b"][idx], idx=idx), "no preconditioner yet")
    assert ctx.timing_get() == before, "a refused call launches nothing"
    assert not ctx.krylov_psetup(c["tn"][idx[:2]], c["cj"][idx[:2]], HH, idx=idx[:2]).any()
    refused(lambda: ctx.krylov_solve(c["tn"][idx], c["cj"][idx], c["tol"][idx], c["b"][idx], idx=idx), "no preconditioner yet")
    ctx.krylov_solve(c["tn"][idx[:2]], c["cj"][idx[:2]], c["tol"][idx[:2]], c["b"][idx[:2]], idx=idx[:2])
    # pivots outside dgbtrf's range are not uploaded
    bad = np.arange(n)
    bad[5] = 7
    refused(lambda: ctx.krylov_upload_prec(0, np.ones((n, 4)), bad), "pivot")
    # off again: the plain solve, bit for bit
    ctx.set_krylov_band_prec(-1, -1)
    assert ctx.krylov_band_prec() is None
    plain_solve(ctx)
    ctx.close()
    # kinds and contexts without the mode
    ld = problems.make_ctx(problems.linear_dense(n=12, batch=2), krylov=5)
    refused(lambda: ld.set_krylov_band_prec(1, 1), "IDAHIP_LINEAR_DENSE")
    assert ld.krylov_band_prec() is None
    ld.close()
    heat = problems.heat1d(n=16, batch=2)
    for other in (problems.make_ctx(heat), problems.make_ctx(heat, band=True)):
        refused(lambda: other.set_krylov_band_prec(1, 1), "not a Krylov ctx")
        refused(lambda: other.krylov_psetup(0.0, 1.0, HH), "not a Krylov ctx")
        assert other.krylov_band_prec() is None
        other.close()


def test_constraints_and_calc_ic_stay_refused_with_the_preconditioner():
    import idahip
    p, _ = PR.step_reference()
    ctx, ens = step_ensemble(p, True)
    with pytest.raises(idahip.IdaHipError, match="Krylov"):
        ens.calc_ic(idahip.Y_INIT, 0.001)
    with pytest.raises(idahip.IdaHipError):
        ctx.set_constraints(np.ones(p["n"]))
    ens.close()
    ctx.close()
