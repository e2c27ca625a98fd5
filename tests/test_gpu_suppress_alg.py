"""Masked error norms (idahip_set_suppress_alg, C IDA's IDASetSuppressAlg) on the device:
  * the entry points that form a local error norm -- idahip_wrms_masked, _init_first, _post_newton (kk = 1..5), _post_newton_constr,
    _complete_step -- against tests/masked_ref.py (pinned on the oracle's norm_wrms_masked by tests/test_tstop_oracle.py), same bits,
    at sizes on both sides of a wavefront, of the 256-thread stride and of the tiny kernels, batch 7 with a 5-entry list in permuted
    order, masks all ones / all zeros / i % 3 == 2 / first element only / last element only, data with the whole exponent range,
    zeros, subnormals and a NaN under a masked element; with the switch off the same calls give stepper_ref's unmasked results;
  * whole integrations against the oracle with suppressalg on (tests/tstop_oracle.py), bit for bit after every call, on the host
    stepper and on the device stepper each problem has; one case with constraints as well;
  * the refusals."""
import numpy as np
import pytest

import constr_ref as CR
import masked_ref as M
import stepper_ref as R
import tstop_cases as K
import tstop_oracle as T

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 8, 9, 64, 255, 256, 257, 300, 1024]
BATCH = 7
IDX = np.array([5, 0, 6, 2, 3], dtype=np.int32)
RTOL, ATOL = 1.0e-5, 1.0e-8
FIELDS = ("yy", "yp", "yypredict", "yppredict", "ewt", "ee")


def masks(n):
    first, last = np.ones(n), np.ones(n)
    first[0] = 0.0
    last[n - 1] = 0.0
    return {"ones": np.ones(n), "zeros": np.zeros(n), "third": (np.arange(n) % 3 != 2).astype(np.float64), "first": first, "last": last}


def fid(name):
    import idahip
    return {"yy": idahip.F_YY, "yp": idahip.F_YP, "yypredict": idahip.F_YYPREDICT, "yppredict": idahip.F_YPPREDICT, "ewt": idahip.F_EWT,
            "ee": idahip.F_EE}[name]


def upload(ctx, v, phi):
    import idahip
    for k in FIELDS:
        ctx.upload(fid(k), v[k])
    for j in range(R.MXORDP1):
        ctx.upload(idahip.F_PHI0 + j, phi[j])


def download(ctx):
    import idahip
    return {k: ctx.download(fid(k)) for k in FIELDS}, np.stack([ctx.download(idahip.F_PHI0 + j) for j in range(R.MXORDP1)])


def nasty_state(rng, n, mask):
    """Every field nasty; system IDX[1] carries a NaN in ee and in phi[0], phi[1] under a masked element (if the mask has one) and
    system IDX[2] an infinity under a counted one."""
    v = {k: R.nasty(rng, (BATCH, n)) for k in FIELDS}
    phi = R.nasty(rng, (R.MXORDP1, BATCH, n))
    off = np.flatnonzero(mask == 0.0)
    on = np.flatnonzero(mask != 0.0)
    if off.size:
        i = off[off.size // 2]
        v["ee"][IDX[1], i] = np.nan
        phi[0, IDX[1], i] = np.nan
        phi[1, IDX[1], i] = np.nan
    if on.size:
        v["ee"][IDX[2], on[-1]] = np.inf
    return v, phi


@pytest.mark.parametrize("n", SIZES)
def test_entry_points_equal_the_masked_restatement(n):
    import idahip
    ctx = idahip.Ctx("heat1d", n, BATCH)
    ctx.set_problem_params(np.ones((BATCH, 1)))
    ctx.set_tolerances(RTOL, np.array([ATOL]))
    rng = np.random.default_rng(9000 + n)
    nan_seen = 0
    for mname, mask in masks(n).items():
        ctx.set_id(mask)
        ctx.set_suppress_alg(True)
        assert ctx.suppress_alg()
        with np.errstate(all="ignore"):
            # ---- wrms_masked (takes the id whether the switch is on or not)
            x, w = R.nasty(rng, (BATCH, n)), R.nasty(rng, (BATCH, n))
            if (mask == 0.0).any():
                x[IDX[0], np.flatnonzero(mask == 0.0)[0]] = np.nan
            dX, dW = ctx.dev_array(x), ctx.dev_array(w)
            got = ctx.wrms_masked(dX, dW, idx=IDX)
            plain = ctx.wrms(dX, dW, idx=IDX)
            for q, s in enumerate(IDX):
                assert R.same_bits(np.float64(got[q]), np.float64(M.wrms_masked(x[s], w[s], mask))), ("wrms_masked", n, mname, s)
                assert R.same_bits(np.float64(plain[q]), np.float64(R.O.wrms(x[s], w[s]))), ("wrms stays unmasked", n, mname, s)
            nan_seen += int(np.isnan(got).sum())
            ctx.dev_free(dX)
            ctx.dev_free(dW)
            # ---- init_first
            v, phi = nasty_state(rng, n, mask)
            upload(ctx, v, phi)
            ypn, p0n = ctx.init_first(IDX)
            after, _ = download(ctx)
            for q, s in enumerate(IDX):
                ewt, a, b = M.init_first(phi[:, s], RTOL, ATOL, mask)
                assert R.same_bits(np.float64(ypn[q]), np.float64(a)) and R.same_bits(np.float64(p0n[q]), np.float64(b)), ("init_first", n, mname, s)
                assert R.same_bits(after["ewt"][s], ewt)
            nan_seen += int(np.isnan(ypn).sum())
            # ---- post_newton, every order
            for kk in range(1, 6):
                upload(ctx, v, phi)
                cj = rng.uniform(0.5, 20.0, IDX.size)
                norms = ctx.post_newton(cj, kk, idx=IDX)
                after, _ = download(ctx)
                for q, s in enumerate(IDX):
                    yy, yp, nrm = M.post_newton(v["yypredict"][s], v["yppredict"][s], v["ee"][s], v["ewt"][s], phi[:, s], cj[q], kk, mask)
                    assert R.same_bits(norms[q], nrm), ("post_newton", n, mname, kk, s, norms[q], nrm)
                    assert R.same_bits(after["yy"][s], yy) and R.same_bits(after["yp"][s], yp)
                nan_seen += int(np.isnan(norms).sum())
            # ---- complete_step
            upload(ctx, v, phi)
            kused = np.array([1, 2, 3, 4, 5], dtype=np.int32)
            ck = rng.uniform(0.1, 2.0, IDX.size)
            p0, bad = ctx.complete_step(kused, ck, 5, idx=IDX)
            after, phi_after = download(ctx)
            for q, s in enumerate(IDX):
                phi2, ee2, ewt2, nrm, b = M.complete_step(phi[:, s], v["ee"][s], int(kused[q]), ck[q], 5, RTOL, ATOL, mask)
                assert R.same_bits(np.float64(p0[q]), np.float64(nrm)) and bool(bad[q]) == b, ("complete_step", n, mname, s)
                assert R.same_bits(phi_after[:, s], phi2) and R.same_bits(after["ee"][s], ee2) and R.same_bits(after["ewt"][s], ewt2)
            # ---- post_newton_constr: its four sums are masked, the norm of its correction is not. Ordinary magnitudes; system IDX[0] and
            # IDX[3] violate their constraints by 1e-9 in a few components (flag 1: the sums are those of the corrected ee)
            c = np.array([0.0, 1.0, -1.0, 2.0, -2.0])[(np.arange(n) + 1) % 5]
            sgn = np.where(c != 0.0, np.sign(c), 1.0)
            vv = {k: rng.uniform(-2.0, 2.0, (BATCH, n)) for k in FIELDS}
            vv["ewt"] = rng.uniform(0.5, 50.0, (BATCH, n))
            yy_t = sgn * rng.uniform(0.5, 2.0, (BATCH, n))
            for s in (IDX[0], IDX[3]):
                yy_t[s, ::3] = -sgn[::3] * 1e-9
            vv["ee"] = yy_t - vv["yypredict"]
            ph = rng.uniform(-0.1, 0.1, (R.MXORDP1, BATCH, n))
            ctx.set_constraints(c)
            upload(ctx, vv, ph)
            cj = rng.uniform(0.5, 20.0, IDX.size)
            norms, flag, rr = ctx.post_newton_constr(cj, 3, 0.33, 1, idx=IDX)
            after, _ = download(ctx)
            flags = []
            for q, s in enumerate(IDX):
                yy, yp, ee2, nrm, fl, rr_ref = M.post_newton_constr(vv["yypredict"][s], vv["yppredict"][s], vv["ee"][s], vv["ewt"][s], ph[:, s],
                                                                    cj[q], 3, c, 0.33, 1, mask)
                flags.append(fl)
                assert flag[q] == fl and R.same_bits(np.float64(rr[q]), np.float64(rr_ref)), ("constr", n, mname, s, flag[q], fl)
                assert R.same_bits(norms[q], nrm), ("post_newton_constr", n, mname, s, norms[q], nrm)
                assert R.same_bits(after["ee"][s], ee2) and R.same_bits(after["yy"][s], yy)
            assert 0 in flags or n < 3
            assert 1 in flags or 2 in flags
            ctx.set_constraints(None)
            # ---- the switch off: stepper_ref's unmasked results from the same state, the id still set
            ctx.set_suppress_alg(False)
            upload(ctx, v, phi)
            norms = ctx.post_newton(cj, 2, idx=IDX)
            for q, s in enumerate(IDX):
                _, _, nrm = R.post_newton(v["yypredict"][s], v["yppredict"][s], v["ee"][s], v["ewt"][s], phi[:, s], cj[q], 2)
                assert R.same_bits(norms[q], nrm), ("switch off", n, mname, s)
    assert nan_seen > 0 or n == 1  # the NaN under a masked element reached the norms
    ctx.close()


# ------------------------------------------------------------------------------------------------ whole integrations
def open_case(case, device_ctl, band=False, constraints=None):
    import idahip
    from idahip import problems
    ctx = problems.make_ctx(case["prob"], band=band)
    ctx.set_id(case["id"])
    ctx.set_suppress_alg(True)
    if constraints is not None:
        ctx.set_constraints(constraints)
    ens = idahip.Ensemble(ctx, case["prob"]["yy0"], case["prob"]["yp0"])
    ens.set_device_controller(device_ctl)
    if case["roots"]:
        ens.set_roots([0, 2], [1e-4, 0.01])
    return ctx, ens


_REF = {}


def run_masked(name, device_ctl, expect_active, band=False, constraints=None):
    case = K.mask_case(name)
    ctx, ens = open_case(case, device_ctl, band=band, constraints=constraints)
    assert ens.device_controller_active() == expect_active
    d = K.ProductDriver(ens)
    ops = []
    for t in case["touts"]:
        for _ in range(3):  # Roberts reports its roots and goes on
            ops.append(("solve", float(t), T.NORMAL))
            st = d.solve(float(t), T.NORMAL)
            if (st == T.SUCCESS).all():
                break
    key = (name, tuple(o[1] for o in ops))
    if key not in _REF:
        _REF[key] = T.run_ops(case["prob"], ops, id=case["id"], suppress=True)[0]
        plain = T.run_ops(case["prob"], ops[:1])[0]
        assert (plain[0]["nst"] != _REF[key][0]["nst"]).any()  # the mask matters here (tests/test_tstop_oracle.py has the figures)
    K.compare(d.rec, _REF[key], by_value=band, what="%s ctl=%d band=%s" % (name, device_ctl, band))
    assert (d.rec[-1]["status"] == T.SUCCESS).all()
    ens.close()
    ctx.close()


@pytest.mark.parametrize("device_ctl", [0, 1])
@pytest.mark.parametrize("name", ["roberts", "linear12", "linear300", "heat20"])
def test_masked_integrations_equal_the_oracle(name, device_ctl):
    run_masked(name, device_ctl, 0 if not device_ctl else (1 if name == "roberts" else 2))


@pytest.mark.parametrize("device_ctl", [0, 1])
def test_masked_integration_on_a_band_ctx(device_ctl):
    run_masked("heat20", device_ctl, 2 if device_ctl else 0, band=True)


@pytest.mark.parametrize("device_ctl", [0, 1])
def test_masked_integration_with_constraints(device_ctl):
    """Roberts with y >= 0 on every component, which its solution never violates at these tolerances: the constraint kernels' own
    masked sums run (the CONSTR instantiation of the one-thread stepper, idahip_post_newton_constr on the host stepper) and the
    results are still the oracle's."""
    run_masked("roberts", device_ctl, device_ctl, constraints=np.ones(3))


def test_refusals():
    import idahip
    case = K.mask_case("linear12")
    from idahip import problems
    for device_ctl in (0, 1):
        ctx = problems.make_ctx(case["prob"])
        ens = idahip.Ensemble(ctx, case["prob"]["yy0"], case["prob"]["yp0"])
        ens.set_device_controller(device_ctl)
        assert not ctx.suppress_alg()
        ctx.set_suppress_alg(True)
        x = ctx.dev_array(np.ones((ctx.batch, ctx.n)))
        with pytest.raises(idahip.IdaHipError, match="id"):  # IDA_MISSING_ID
            ens.solve(0.1)
        with pytest.raises(idahip.IdaHipError, match="id"):
            ens.solve_schedule([0.1, 0.2])
        with pytest.raises(idahip.IdaHipError, match="id"):
            ctx.wrms_masked(x, x)
        with pytest.raises(idahip.IdaHipError, match="id"):
            ctx.init_first()
        with pytest.raises(idahip.IdaHipError, match="id"):
            ctx.post_newton(1.0, 1)
        with pytest.raises(idahip.IdaHipError, match="id"):
            ctx.complete_step(1, 1.0)
        assert (ens.counter("nst") == 0).all() and (ens.counter("nre") == 0).all()
        ctx.set_id(case["id"])
        with pytest.raises(idahip.IdaHipError, match="suppress_alg"):  # set_id, calc_ic, set_suppress_alg(1), solve is the order
            ens.calc_ic(idahip.YA_YDP_INIT, 0.1)
        ctx.set_suppress_alg(False)
        ens.calc_ic(idahip.YA_YDP_INIT, 0.1)  # accepted with the switch off (a system that fails keeps its values)
        ctx.set_suppress_alg(True)
        st, _ = ens.solve(0.1)
        assert (st == 0).all()
        ctx.dev_free(x)
        ens.close()
        ctx.close()
