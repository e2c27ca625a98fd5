"""IDAHIP_BRUSS1D (the 1-D Brusselator: nonlinear, stiff, bandwidths (2, 2)) on the device against tests/bruss_ref.py and against
the same problem written as host callbacks (bruss_ref.twin): the NLProblem entry points and Jacobians at every launch shape, whole
integrations on the dense, band and Krylov ctx, on the host stepper, the fused Newton and the device lock-step rounds, difference-
quotient Jacobians, calc_ic and constraints. Bit for bit means view(np.uint64) equality, by value np.array_equal.

The systems are 1, 3, 4 and 6 of idahip.problems.bruss1d: distinct parameters; system 0 passes every error test in the reference run
(tests/test_bruss_ref.py), these fail one (3, 4, 6 at every size used here, 1 from m = 16 on), and all take second Newton iterations."""
import numpy as np
import pytest

import bruss_ref as BR
import calcic_ref as IC
import dq_ref as DQ
import krylov_prec_ref as PR
import oracle_lib as O

pytestmark = pytest.mark.gpu
IDS = [1, 3, 4, 6]
B = len(IDS)
SIZES = [10, 24, 514, 1026, 4096]  # both sides of the 256-lane stride and of 1024, and the limit
RUN_CNT = ("nst", "nre", "nje", "nsetups", "nni", "netf", "ncfn", "n_attempts")
_REF = {}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


def raw_lu(ctx, s):
    """idahip_download_lu's own buffers (column-major factors, pivots): what two ctxs are compared by, without the 134 MB transpose
    that Ctx.download_lu makes of each matrix at n = 4096"""
    import idahip
    lu, piv = np.empty(ctx.n * ctx.n), np.empty(ctx.n, dtype=np.int64)
    assert ctx.H.idahip_download_lu(ctx.h, int(s), idahip._p(lu), idahip._p(piv, idahip.i64p)) == 0
    return lu, piv


def problem(n, touts=(0.25, 0.5), ids=IDS):
    from idahip import problems
    p = BR.select(problems.bruss1d(m=n // 2, batch=max(ids) + 1), ids)
    p["touts"] = np.asarray(touts, dtype=np.float64)
    return p


def reference(n, mode, width=None):
    """computed once per (n, mode, width), shared and left unchanged"""
    key = (n, mode, width)
    if key not in _REF:
        p = problem(n)
        _REF[key] = BR.run(p, p["touts"], mode=mode, width=width)
    return _REF[key]


def entry_state(p, seed):
    """the fields of an NLProblem call: a predicted state near the initial one, a nonzero ee, the ewt of the tolerances"""
    import idahip
    n = p["n"]
    rng = np.random.default_rng(seed)
    yypred = p["yy0"] * (1.0 + 1e-3 * rng.standard_normal((B, n)))
    return {idahip.F_YYPREDICT: yypred, idahip.F_YPPREDICT: p["yp0"] + 1e-2 * rng.standard_normal((B, n)),
            idahip.F_EE: 1e-4 * rng.standard_normal((B, n)), idahip.F_EWT: 1.0 / (p["rtol"] * np.abs(yypred) + p["atol"][0]),
            idahip.F_YY: p["yy0"].copy(), idahip.F_YP: p["yp0"].copy(), idahip.F_DELTA: np.zeros((B, n)), idahip.F_SAVRES: np.zeros((B, n))}


IDX = np.array([3, 0, 2], dtype=np.int32)  # unordered, system 1 is never listed
TN = np.array([0.01, 0.02, 0.03])
CJ = np.array([150.0, 2.5e3, 40.0])
HH = np.array([1.0e-3, -2.0e-3, 0.37])


def expect_sys(fields, p, reset, ee_now, idx, cj):
    """-> (yy, yp, res, ee) the listed systems must hold after nls_sys, per list position"""
    import idahip
    out = []
    for q, s in enumerate(idx):
        ee = np.zeros(p["n"]) if reset else ee_now[s]
        yy = fields[idahip.F_YYPREDICT][s] + ee
        yp = fields[idahip.F_YPPREDICT][s] + cj[q] * ee
        out.append((yy, yp, BR.res(p["params"][s], yy, yp), ee))
    return out


# ------------------------------------------------------------------------------------------------ entry points, dense ctx
@pytest.mark.parametrize("n", SIZES)
def test_entry_points_dense_ctx(n):
    """nls_sys (reset_ee 0 and 1), nls_lsetup, nls_sys_setup, jac_dq and nls_lsetup_dq on an unordered subset, against bruss_ref bit
    for bit (factors: against the oracle's getrf of bruss_ref's Jacobian up to n = 1026, where it is affordable) and against the
    callback twin at every n (factors and pivots of download_lu: bit for bit for the analytic setups, by value for the DQ setup,
    whose zeros outside the band differ in sign by definition); systems off the list unchanged by every call."""
    import idahip
    from idahip import problems
    p = problem(n)
    idx, tn, cj, hh = IDX, TN, CJ, HH
    ctx, twin = problems.make_ctx(p), problems.make_ctx(BR.twin(p))
    fields = entry_state(p, n)
    for c in (ctx, twin):
        for f, v in fields.items():
            c.upload(f, v)
    watch = (idahip.F_DELTA, idahip.F_SAVRES, idahip.F_YY, idahip.F_YP, idahip.F_EE)

    def check_sys(reset, what):
        ee_before = fields[idahip.F_EE] if check_sys.ee is None else check_sys.ee
        want = expect_sys(fields, p, reset, ee_before, idx, cj)
        got = {f: ctx.download(f) for f in watch}
        for q, s in enumerate(idx):
            yy, yp, r, ee = want[q]
            assert same_bits(got[idahip.F_YY][s], yy) and same_bits(got[idahip.F_YP][s], yp), (what, s)
            assert same_bits(got[idahip.F_DELTA][s], r) and same_bits(got[idahip.F_SAVRES][s], r), (what, s, np.abs(got[idahip.F_DELTA][s] - r).max())
            assert same_bits(got[idahip.F_EE][s], ee), (what, s)
        for f in watch:
            assert same_bits(got[f][1], fields[f][1]), (what, f)  # off the list
            assert same_bits(twin.download(f), got[f]), (what, f)
        check_sys.ee = got[idahip.F_EE]
        return got

    check_sys.ee = None

    def check_factors(J_of, what, by_oracle):
        """J_of(q, s) -> the reference Jacobian [n][n] column-major"""
        for q, s in enumerate(idx):
            (lu, piv), (tl, tp) = raw_lu(ctx, s), raw_lu(twin, s)
            assert np.array_equal(piv, tp) and same_bits(lu, tl), (what, s)
            if by_oracle:
                lu, piv = ctx.download_lu(int(s))
                cm = np.ascontiguousarray(J_of(q, s))[None]
                oinfo, opiv = O.getrf_batch(cm)
                assert oinfo[0] == 0 and np.array_equal(piv, opiv[0]), (what, s)
                assert np.array_equal(lu, cm[0].T), (what, s)  # by value: the factors of a banded matrix are full of signed zeros
    by_oracle = n <= 1026
    off_before = raw_lu(ctx, 1)
    for reset in (0, 1):
        for c in (ctx, twin):
            c.nls_sys(tn, cj, reset, idx)
        got = check_sys(reset, ("sys", reset))
    yy_now = got[idahip.F_YY]
    rc, info = ctx.nls_lsetup(tn, cj, idx)
    rt, it = twin.nls_lsetup(tn, cj, idx)
    assert rc == rt == 0 and not info.any() and not it.any()
    check_factors(lambda q, s: BR.jac(p["params"][s], cj[q], yy_now[s]), "lsetup", by_oracle)
    for reset in (False, True):  # a second and third setup: n > 1024 writes into the work matrix the factorisation left zeroed
        rc, info = ctx.nls_sys_setup(tn, cj * 1.5, reset, idx)
        rt, it = twin.nls_sys_setup(tn, cj * 1.5, reset, idx)
        assert rc == rt == 0 and not info.any()
        want = expect_sys(fields, p, reset, check_sys.ee, idx, cj * 1.5)
        got = {f: ctx.download(f) for f in watch}
        for q, s in enumerate(idx):
            assert same_bits(got[idahip.F_YY][s], want[q][0]) and same_bits(got[idahip.F_YP][s], want[q][1]), ("sys_setup", reset, s)
            assert same_bits(got[idahip.F_SAVRES][s], want[q][2]) and same_bits(got[idahip.F_DELTA][s], want[q][2]), ("sys_setup", reset, s)
        check_sys.ee = got[idahip.F_EE]
        check_factors(lambda q, s: BR.jac(p["params"][s], cj[q] * 1.5, got[idahip.F_YY][s]), ("sys_setup", reset), by_oracle and reset)
    a, b = raw_lu(ctx, 1)
    assert same_bits(a, off_before[0]) and np.array_equal(b, off_before[1])
    # difference quotients at the state nls_sys_setup left (savres is the residual there)
    yy, yp, rr, ewt = got[idahip.F_YY], got[idahip.F_YP], got[idahip.F_SAVRES], fields[idahip.F_EWT]
    dq_idx = idx[:2] if n == 4096 else idx  # (a compact Jacobian is 134 MB there, and its restatement 4096 residuals)
    J = ctx.jac_dq(tn[:dq_idx.size], cj[:dq_idx.size], hh[:dq_idx.size], dq_idx)
    ref = [BR.dense_dq_banded(p["params"][s], yy[s], yp[s], ewt[s], rr[s], cj[q], hh[q]) for q, s in enumerate(dq_idx)]
    for q, s in enumerate(dq_idx):
        assert same_bits(J[q], ref[q]), ("jac_dq", s, np.abs(J[q] - ref[q]).max())
    del J
    # nls_lsetup_dq on the whole unordered list at every n, against the twin's DQ setup (pack / host residual / scatter). The twin
    # writes the full definition, the device kind +0.0 outside rows j-2..j+2 where the definition gives -0.0 for a negative
    # increment (include/ida_hip.h), so the factors agree by value, not bit for bit; the pivots are identical.
    for c in (ctx, twin):
        c.set_jacobian_dq(True)
    rc, info = ctx.nls_lsetup_dq(tn, cj, hh, idx)
    rt, it = twin.nls_lsetup_dq(tn, cj, hh, idx)
    assert rc == rt == 0 and not info.any() and not it.any()
    for q, s in enumerate(idx):
        (lu, piv), (tl, tp) = raw_lu(ctx, s), raw_lu(twin, s)
        assert np.array_equal(piv, tp) and np.array_equal(lu, tl), ("lsetup_dq against the twin", s)
        assert np.count_nonzero(lu) >= 2 * n  # (not two empty matrices)
        if by_oracle and q < len(ref):
            lu, piv = ctx.download_lu(int(s))
            cm = np.ascontiguousarray(ref[q])[None]
            oinfo, opiv = O.getrf_batch(cm)
            assert np.array_equal(piv, opiv[0]) and np.array_equal(lu, cm[0].T), ("lsetup_dq", s)
    a, b = raw_lu(ctx, 1)
    assert same_bits(a, off_before[0]) and np.array_equal(b, off_before[1])  # off the list: untouched by the DQ setup too
    twin.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------ band ctx Jacobians
@pytest.mark.parametrize("width", [(2, 2), (3, 4), (2, 5)], ids=str)
@pytest.mark.parametrize("n", SIZES)
def test_band_ctx_jacobians(n, width):
    """The analytic band Jacobian through its factors: by value against krylov_prec_ref.band_getrf of band_pack(bruss_ref.jac), bit for
    bit against the callback twin whose bjac writes exactly that matrix. This check is indirect: no entry point returns the
    unfactored band matrix of an analytic setup, so a wrong sign of a zero entry that does not survive the factorisation would not
    be seen here. The band DQ Jacobian itself (jac_dq) bit for bit against dq_ref.band_dq; its factors by value."""
    import idahip
    from idahip import problems
    ml, mu = width
    p = problem(n)
    ctx, twin = problems.make_ctx(p, band=width), problems.make_ctx(BR.twin(p, band=width), band=True)
    fields = entry_state(p, n + ml)
    for c in (ctx, twin):
        for f, v in fields.items():
            c.upload(f, v)
        c.nls_sys(TN, CJ, 0, IDX)
    yy, yp, rr, ewt = (ctx.download(f) for f in (idahip.F_YY, idahip.F_YP, idahip.F_SAVRES, idahip.F_EWT))
    for q, s in enumerate(IDX):
        assert same_bits(rr[s], BR.res(p["params"][s], yy[s], yp[s])), s
    off_before = ctx.download_lu_band(1)
    for k in range(2):  # the second setup overwrites the factors and fill of the first
        cj = CJ * (1.0 + k)
        rc, info = ctx.nls_lsetup(TN, cj, IDX)
        rt, it = twin.nls_lsetup(TN, cj, IDX)
        assert rc == rt == 0 and not info.any()
        for q, s in enumerate(IDX):
            ab, piv = ctx.download_lu_band(int(s))
            tb, tp = twin.download_lu_band(int(s))
            assert np.array_equal(piv, tp) and same_bits(ab, tb), (k, s)
            ri, rab, rpiv = PR.band_getrf(idahip.band_pack(BR.jac(p["params"][s], cj[q], yy[s]).T, ml, mu), n, ml, mu)
            assert ri == 0 and np.array_equal(piv, rpiv) and np.array_equal(ab, rab), (k, s)
    a, b = ctx.download_lu_band(1)
    assert same_bits(a, off_before[0]) and np.array_equal(b, off_before[1])
    twin.close()
    J = ctx.jac_dq(TN, CJ, HH, IDX)
    for q, s in enumerate(IDX):
        ref = DQ.band_dq(BR.prob_res(p, s), yy[s], yp[s], ewt[s], rr[s], CJ[q], HH[q], ml, mu)
        assert same_bits(J[q], ref), (s, np.abs(J[q] - ref).max())
        if q == 0:
            ctx.set_jacobian_dq(True)
            rc, info = ctx.nls_lsetup_dq(TN, CJ, HH, IDX)
            assert rc == 0 and not info.any()
        ri, rab, rpiv = PR.band_getrf(ref, n, ml, mu)
        ab, piv = ctx.download_lu_band(int(s))
        assert ri == 0 and np.array_equal(piv, rpiv) and np.array_equal(ab, rab), ("dq factors", s)
    ctx.close()


def test_constructors_refuse_odd_and_small_n(capfd):
    """-2 and a text (the constructors have no ctx to keep it in: it goes to stderr) for odd n, n < 10 and band widths below (2, 2)"""
    import idahip
    capfd.readouterr()
    for kw in ({}, {"band": (2, 2)}, {"krylov": 5}):
        for n in (11, 8, 4097):
            with pytest.raises(idahip.IdaHipError, match=r"\(-2\)"):
                idahip.Ctx("bruss1d", n, 2, **kw)
            err = capfd.readouterr().err
            # (a band or Krylov ctx refuses n = 8 and n = 4097 by its own size limits first)
            assert ("IDAHIP_BRUSS1D: n = %d" % n) in err or ("n = %d outside" % n) in err, (kw, n, err)
            if n == 11 or not kw:
                assert ("IDAHIP_BRUSS1D: n = %d" % n) in err, (kw, n, err)
    for width in ((1, 2), (2, 1), (0, 0)):
        with pytest.raises(idahip.IdaHipError, match=r"\(-2\)"):
            idahip.Ctx("bruss1d", 24, 2, band=width)
        assert ">= 2 for IDAHIP_BRUSS1D" in capfd.readouterr().err
    c = idahip.Ctx("bruss1d", 2050, 2)
    assert c.H.idahip_lu_superpanel(c.h) == 1  # banded content: the heat default
    with pytest.raises(idahip.IdaHipError, match=r"5 parameters"):
        c.set_problem_params(np.ones((2, 1)))
    c.close()
    from idahip import problems
    c = problems.make_ctx(problem(24), band=True)
    assert c.band_query() == (2, 2)
    c.close()


# ------------------------------------------------------------------------------------------------ whole integrations
def snapshot(ens):
    return {"yy": ens.yy(), "yp": ens.yp(), "hused": ens.real("hused"), "tn": ens.real("tn"), "c": ens.counters()}


def integrate(ctx, p, host=True, fused=None, constr=None):
    """-> per tout (status, snapshot)"""
    import idahip
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    if host:
        ens.set_device_controller(0)
    if fused is not None:
        ens.set_fused_newton(fused)
    active = ens.device_controller_active()
    out = []
    for t in p["touts"]:
        st, tret = ens.solve(float(t))
        out.append((st.copy(), snapshot(ens)))
    rounds = ens.total_rounds()
    ens.close()
    return out, active, rounds


def assert_same_run(a, b, exact, counters=None, what=""):
    eq = same_bits if exact else np.array_equal
    assert len(a) == len(b)
    for i, ((sa, xa), (sb, xb)) in enumerate(zip(a, b)):
        assert np.array_equal(sa, sb), (what, i, sa, sb)
        for k in ("yy", "yp", "hused", "tn"):
            assert eq(xa[k], xb[k]), (what, i, k, np.abs(xa[k] - xb[k]).max())
        for k in (counters or xa["c"]):
            assert np.array_equal(xa["c"][k], xb["c"][k]), (what, i, k, xa["c"][k], xb["c"][k])


def assert_equals_reference(run, ref, exact, counters, what=""):
    eq = same_bits if exact else np.array_equal
    for i, (st, x) in enumerate(run):
        assert np.array_equal(st, ref["status"][i]), (what, i, st, ref["status"][i])
        for k in ("yy", "yp", "hused", "tn"):
            assert eq(x[k], ref[k][i]), (what, i, k, np.abs(x[k] - ref[k][i]).max())
        assert np.array_equal(x["c"]["kused"], ref["kused"][i]), (what, i)
        for k in counters:
            assert np.array_equal(x["c"][k], ref["counters"][k][i]), (what, i, k, x["c"][k], ref["counters"][k][i])


@pytest.mark.parametrize("n", [10, 130, 514])
def test_dense_ctx_integration_on_every_stepper(n):
    """The host stepper against bruss_ref's direct=True reference (y, y', hused, tn, kused and every counter at each tout, bit for
    bit); the fused first two Newton iterations against one round trip per iteration; the device lock-step rounds against the host
    stepper (a round more is allowed)."""
    from idahip import problems
    p, ref = problem(n), reference(n, "direct")
    assert (ref["status"] == 0).all()
    c = ref["counters"]
    assert (c["nni"][-1] > c["nst"][-1]).all() and (c["netf"][-1] >= 1).sum() >= 3, (c["nni"][-1], c["nst"][-1], c["netf"][-1])
    runs = {}
    for name, host, fused in (("host", True, 0), ("host_fused", True, 1), ("rounds", False, None)):
        ctx = problems.make_ctx(p)
        runs[name], active, rounds = integrate(ctx, p, host=host, fused=fused)
        ctx.close()
        assert active == (0 if host else 2), (name, active)
        runs[name + "_rounds"] = rounds
    assert_equals_reference(runs["host"], ref, True, RUN_CNT, "host stepper against the reference")
    assert_same_run(runs["host_fused"], runs["host"], True, what="fused Newton against unfused")
    assert_same_run(runs["rounds"], runs["host"], True, what="device rounds against the host stepper")
    assert runs["rounds_rounds"] >= runs["host_rounds"] > 0


@pytest.mark.parametrize("superpanel", [0, 1])
def test_dense_ctx_beyond_2048_rows_against_the_callback_twin(superpanel):
    """n = 2050, batch 2, two short touts: the zero-matrix shortcut (jwzero) with entries that change from setup to setup."""
    from idahip import problems
    p = problem(2050, touts=(0.0005, 0.001), ids=[3, 6])
    runs = []
    for q in (p, BR.twin(p)):
        ctx = problems.make_ctx(q)
        ctx.set_lu_superpanel(superpanel)
        r, _, _ = integrate(ctx, p, host=True, fused=0)
        ctx.close()
        runs.append(r)
    assert_same_run(runs[0], runs[1], True, what="device kind against the callback twin")
    assert (runs[0][-1][1]["c"]["nsetups"] >= 2).all() and (runs[0][-1][0] == 0).all()


@pytest.mark.parametrize("width", [(2, 2), (3, 4)], ids=str)
@pytest.mark.parametrize("n", [10, 514])
def test_band_ctx_integration_equals_the_dense_ctx(n, width):
    from idahip import problems
    p = problem(n)
    ctx = problems.make_ctx(p)
    dense, _, _ = integrate(ctx, p, host=True)
    ctx.close()
    for host in (True, False):
        ctx = problems.make_ctx(p, band=width)
        band, active, _ = integrate(ctx, p, host=host)
        ctx.close()
        assert active == (0 if host else 2)
        assert_same_run(band, dense, False, what=("band", width, "host" if host else "rounds"))


@pytest.mark.parametrize("band", [None, (2, 2)], ids=str)
def test_dq_integration_equals_the_callback_twin(band):
    """n = 130: device DQ Jacobians against the twin's pack / host residual / scatter round trip, bit for bit, with equal nre_dq."""
    from idahip import problems
    p = problem(130)
    t = BR.twin(p)
    runs = []
    for q in (p, t):
        if q is p:
            ctx = problems.make_ctx(p, band=band or False)
            ctx.set_jacobian_dq(True)
        else:
            import idahip
            ctx = idahip.Ctx("host_callback", 130, B, band=band)
            ctx.set_tolerances(p["rtol"], p["atol"])
            ctx.set_host_residual(t["res"])
        assert ctx.jacobian_dq()
        r, _, _ = integrate(ctx, p, host=True, fused=0)
        ctx.close()
        runs.append(r)
    assert_same_run(runs[0], runs[1], True, what="DQ against the twin")
    c = runs[0][-1][1]["c"]
    assert np.array_equal(c["nre_dq"], c["nje"] * DQ.dq_evals(130, band)) and (c["nre_dq"] > 0).all() and (runs[0][-1][0] == 0).all()


# ------------------------------------------------------------------------------------------------ Krylov ctx
KRY_CNT = RUN_CNT + ("nli", "ncfl", "nre_dq")


def krylov_run(p, fused, width=None):
    from idahip import problems
    ctx = problems.make_ctx(p, krylov=5)
    ctx.set_krylov_fused(fused)
    if width is not None:
        ctx.set_krylov_band_prec(*width)
    r, active, _ = integrate(ctx, p, host=False)  # (a Krylov ctx has no device stepper: the host stepper either way)
    ctx.close()
    assert active == 0
    return r


@pytest.mark.parametrize("n", [10, 130])
def test_krylov_plain_against_the_reference(n):
    p, ref = problem(n), reference(n, "krylov")
    fused = krylov_run(p, True)
    assert_equals_reference(fused, ref, True, KRY_CNT, "plain SPGMR")
    assert (ref["counters"]["nli"][-1] > 0).all()
    assert_same_run(krylov_run(p, False), fused, True, what="split against fused")


@pytest.mark.parametrize("width", [(2, 2), (1, 1)], ids=str)
@pytest.mark.parametrize("n", [10, 130])
def test_krylov_band_preconditioner_against_the_reference(n, width):
    p, ref = problem(n), reference(n, "prec", width)
    fused = krylov_run(p, True, width)
    assert_equals_reference(fused, ref, False, KRY_CNT + ("npe", "nps"), "preconditioned SPGMR")
    assert (ref["status"] == 0).all() and (ref["counters"]["npe"][-1] > 0).all()
    assert_same_run(krylov_run(p, False, width), fused, True, what="split against fused")


# ------------------------------------------------------------------------------------------------ calc_ic
@pytest.mark.parametrize("band", [None, (2, 2)], ids=str)
def test_calc_ic_from_moved_end_values(band):
    """YA_YDP_INIT, id = 0 at the four end components, end values moved by 0.05, y' = 0, n = 32: the analytic Jacobian on a dense ctx
    (bit for bit), the DQ one on a band ctx (by value)."""
    import idahip
    from idahip import problems
    n, tout1 = 32, 0.25
    p = problem(n)
    ends = [0, 1, n - 2, n - 1]
    id_ = np.ones(n)
    id_[ends] = 0.0
    yy0, yp0 = p["yy0"].copy(), np.zeros((B, n))
    yy0[:, ends] += 0.05
    ctx = problems.make_ctx(p, band=band or False)
    if band:
        ctx.set_jacobian_dq(True)
    ctx.set_id(id_)
    ens = idahip.Ensemble(ctx, yy0, yp0)
    status = ens.calc_ic(idahip.YA_YDP_INIT, tout1)
    yy, yp, cnt = ens.yy(), ens.yp(), ens.counters()
    ens.close()
    ctx.close()
    probs = []
    for s in range(B):
        prm = p["params"][s]
        r = BR.prob_res(p, s)
        if band:
            jac = lambda cj, y, ypv, rr, hic, ewt, r=r: np.ascontiguousarray(
                idahip.band_unpack(DQ.band_dq(r, y, ypv, ewt, rr, cj, hic, *band), n, *band).T)
            probs.append(IC.Problem(n, r, jac, DQ.dq_evals(n, band)))
        else:
            probs.append(IC.Problem(n, r, lambda cj, y, ypv, rr, hic, ewt, prm=prm: BR.jac(prm, cj, y)))
    ref = IC.calc_ic_batch(probs, yy0, yp0, p["rtol"], p["atol"], IC.YA_YDP_INIT, tout1, id=id_)
    assert (ref["status"] == 0).all() and np.array_equal(status, ref["status"]), (status, ref["status"])
    eq = np.array_equal if band else same_bits
    assert eq(yy, ref["yy"]) and eq(yp, ref["yp"]), (np.abs(yy - ref["yy"]).max(), np.abs(yp - ref["yp"]).max())
    for k in IC.COUNTERS:
        assert np.array_equal(cnt[k], ref["counters"][k]), (k, cnt[k], ref["counters"][k])
    assert np.abs(yy[:, ends] - p["yy0"][:, ends]).max() < 1e-6 and np.abs(yp).max() > 0.0  # the ends came back, y' was computed


# ------------------------------------------------------------------------------------------------ constraints
def test_constraints_on_the_host_stepper():
    """c = 1.0 everywhere, n = 130: bit for bit the callback twin with the same constraints; a y0 with one negative entry gives
    ILL_INPUT for that system only."""
    import idahip
    from idahip import problems
    n = 130
    p = problem(n)
    runs = []
    for q in (p, BR.twin(p)):
        ctx = problems.make_ctx(q)
        ctx.set_constraints(np.ones(n))
        r, active, _ = integrate(ctx, p, host=False, fused=0)  # constraints put n > 8 on the host stepper by themselves
        ctx.close()
        assert active == 0
        runs.append(r)
    assert_same_run(runs[0], runs[1], True, what="constraints against the twin")
    assert (runs[0][-1][0] == 0).all()
    bad = dict(p, yy0=p["yy0"].copy())
    bad["yy0"][2, 7] = -1.0e-3
    ctx = problems.make_ctx(bad)
    ctx.set_constraints(np.ones(n))
    r, _, _ = integrate(ctx, bad, host=True)
    ctx.close()
    assert r[0][0].tolist() == [0, 0, -22, 0] and r[-1][0].tolist() == [0, 0, -22, 0]  # ILL_INPUT
    for s in (0, 1, 3):
        assert same_bits(r[-1][1]["yy"][s], runs[0][-1][1]["yy"][s])
