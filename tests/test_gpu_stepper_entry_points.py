"""GPU parity of the stepper's vector entry points (idahip_init_first, _scale_phi1, _predict, _post_newton, _restore,
_complete_step, _get_solution, _get_dky, _snapshot_initial / _restore_initial) and of the Newton iteration body
(idahip_newton_iter, _newton_iter2), called one by one through idahip.Ctx on random ctx state and compared field by field,
bit for bit, with tests/stepper_ref.py (pinned on the oracle by tests/test_stepper_ref.py).

Sizes sit on both sides of the 256-thread stride and of every launch path of the Newton iteration (tiny n <= 8; 256 threads
with VEC = 1 for odd n, VEC = 2 for even n; even n >= 2048: 1024 threads, LDS-staged diagonal blocks and the factors'
zero-block map). Systems off the list must come back unchanged in every field."""
import numpy as np
import pytest

import stepper_ref as R

pytestmark = pytest.mark.gpu

SIZES = [3, 9, 63, 64, 65, 255, 256, 257, 511, 1025, 2047, 2048, 2050, 4095, 4096]
EXHAUSTIVE = {3, 64, 257, 2050, 4096}  # every order combination here; a sample at the other sizes
RTOL = 1.0e-5
VEC_FIELDS = ["yy", "yp", "yypredict", "yppredict", "ewt", "ee", "delta", "savres"]


def batch_of(n):
    return 5 if n <= 1025 else 3


def idx_of(B):
    """Unordered, non-contiguous, at least one system left off."""
    return np.array([4, 1, 2] if B == 5 else [2, 0], dtype=np.int32)


def field_id(name):
    import idahip
    return {"yy": idahip.F_YY, "yp": idahip.F_YP, "yypredict": idahip.F_YYPREDICT, "yppredict": idahip.F_YPPREDICT,
            "ewt": idahip.F_EWT, "ee": idahip.F_EE, "delta": idahip.F_DELTA, "savres": idahip.F_SAVRES}[name]


class Mirror:
    """Device state of a ctx and its host mirror, which the tests update with stepper_ref for the listed systems only."""

    def __init__(self, ctx, rng):
        B, n = ctx.batch, ctx.n
        self.ctx = ctx
        self.v = {f: R.nasty(rng, (B, n)) for f in VEC_FIELDS}
        self.phi = R.nasty(rng, (R.MXORDP1, B, n))
        # one system carries infinities, another NaN, in phi and ee
        self.phi[2, 0, n // 2] = np.inf
        self.phi[0, 0, n - 1] = -np.inf
        self.v["ee"][0, 0] = np.inf
        if B > 1:
            self.phi[1, 1, n // 3] = np.nan
            self.v["ee"][1, n - 1] = np.nan
        self.upload()

    def upload(self):
        import idahip
        for f in VEC_FIELDS:
            self.ctx.upload(field_id(f), self.v[f])
        for j in range(R.MXORDP1):
            self.ctx.upload(idahip.F_PHI0 + j, self.phi[j])

    def check(self, what):
        import idahip
        for f in VEC_FIELDS:
            got = self.ctx.download(field_id(f))
            for s in range(self.ctx.batch):
                assert R.same_bits(got[s], self.v[f][s]), (what, f, s)
        for j in range(R.MXORDP1):
            got = self.ctx.download(idahip.F_PHI0 + j)
            for s in range(self.ctx.batch):
                assert R.same_bits(got[s], self.phi[j, s]), (what, "phi", j, s)

    def sys_phi(self, s):
        return self.phi[:, s, :]


_CTXS = {}


@pytest.fixture(scope="module")
def ctxs():
    yield _CTXS
    for c in _CTXS.values():
        c.close()
    _CTXS.clear()


def vec_ctx(ctxs, n, atol_kind="scalar"):
    import idahip
    if n not in ctxs:
        if n == 3:
            ctxs[n] = idahip.Ctx("lorenz63", 3, batch_of(n))
        else:
            ctxs[n] = idahip.Ctx("heat1d", n, batch_of(n))
            ctxs[n].set_problem_params(np.ones((batch_of(n), 1)))
    ctx = ctxs[n]
    atol = atol_of(n, atol_kind)
    ctx.set_tolerances(RTOL, atol)
    return ctx, atol


def atol_of(n, kind):
    """scalar, or a different value per component (TolControlSV, natol == n)"""
    return 1.0e-8 if kind == "scalar" else 10.0 ** -np.linspace(4.0, 10.0, n)


def combos(n, full):
    """Run the order combinations `full` in groups of the list length; a sample of them at the non-exhaustive sizes."""
    if n not in EXHAUSTIVE:
        rng = np.random.default_rng(n)
        keep = sorted(rng.choice(len(full), size=min(len(full), 4), replace=False))
        full = [full[k] for k in keep]
    return full


def groups(items, k):
    return [items[i:i + k] for i in range(0, len(items), k)]


def coeffs(rng, m, k=R.MXORDP1):
    return rng.uniform(0.25, 4.0, (m, k)) * rng.choice([1.0, -1.0], (m, k))


@pytest.mark.parametrize("n", SIZES)
def test_init_first_and_scale_phi1(ctxs, n):
    for atol_kind in ("scalar", "vector"):
        ctx, atol = vec_ctx(ctxs, n, atol_kind)
        rng = np.random.default_rng(1000 + n)
        st = Mirror(ctx, rng)
        idx = idx_of(ctx.batch)
        ypn, p0n = ctx.init_first(idx)
        for q, s in enumerate(idx):
            ewt, a, b = R.init_first(st.sys_phi(s), RTOL, atol)
            st.v["ewt"][s] = ewt
            assert R.same_bits(np.float64(ypn[q]), np.float64(a)) and R.same_bits(np.float64(p0n[q]), np.float64(b)), (n, s)
        st.check("init_first")
        fac = rng.uniform(-3.0, 3.0, idx.size)
        ctx.scale_phi1(fac, idx)
        for q, s in enumerate(idx):
            st.phi[:, s, :] = R.scale_phi1(st.sys_phi(s), fac[q])
        st.check("scale_phi1")


@pytest.mark.parametrize("n", SIZES)
def test_predict_every_kk_ns(ctxs, n):
    ctx, _ = vec_ctx(ctxs, n)
    rng = np.random.default_rng(2000 + n)
    st = Mirror(ctx, rng)
    idx = idx_of(ctx.batch)
    for grp in groups(combos(n, [(kk, ns) for kk in range(1, 6) for ns in range(0, kk + 2)]), idx.size):
        ids = idx[:len(grp)]
        kk, ns = np.array([g[0] for g in grp]), np.array([g[1] for g in grp])
        beta, gamma = coeffs(rng, len(grp)), coeffs(rng, len(grp))
        ctx.predict(kk, ns, beta, gamma, ids)
        for q, s in enumerate(ids):
            phi, yyp, ypp = R.predict(st.sys_phi(s), kk[q], ns[q], beta[q], gamma[q])
            st.phi[:, s, :] = phi
            st.v["yypredict"][s], st.v["yppredict"][s] = yyp, ypp
        st.check(("predict", grp))


@pytest.mark.parametrize("n", SIZES)
def test_restore_every_kk_ns(ctxs, n):
    ctx, _ = vec_ctx(ctxs, n)
    rng = np.random.default_rng(3000 + n)
    st = Mirror(ctx, rng)
    idx = idx_of(ctx.batch)
    for grp in groups(combos(n, [(kk, ns) for kk in range(1, 6) for ns in range(0, kk + 2)]), idx.size):
        ids = idx[:len(grp)]
        kk, ns = np.array([g[0] for g in grp]), np.array([g[1] for g in grp])
        cvals = coeffs(rng, len(grp))
        ctx.restore(kk, ns, cvals, ids)
        for q, s in enumerate(ids):
            st.phi[:, s, :] = R.restore(st.sys_phi(s), kk[q], ns[q], cvals[q])
        st.check(("restore", grp))


@pytest.mark.parametrize("n", SIZES)
def test_post_newton_every_kk(ctxs, n):
    """The four norms with their "0 where undefined" slots (kk = 1: two of them; kk = 5: no ||ee - phi[kk+1]||). Ordinary
    magnitudes for the norms' inputs, so the squared sums stay finite and their order shows in the bits."""
    for atol_kind in ("scalar", "vector"):
        ctx, _ = vec_ctx(ctxs, n, atol_kind)
        rng = np.random.default_rng(4000 + n)
        st = Mirror(ctx, rng)
        st.v["ee"] = R.nasty(rng, st.v["ee"].shape, special=False)
        st.v["ewt"] = np.abs(R.nasty(rng, st.v["ewt"].shape, special=False))
        st.phi = R.nasty(rng, st.phi.shape, special=False)
        st.v["ee"][0, 1] = -0.0
        st.upload()
        idx = idx_of(ctx.batch)
        for grp in groups(combos(n, list(range(1, 6))), idx.size):
            ids = idx[:len(grp)]
            kk = np.array(grp)
            cj = 10.0 ** rng.uniform(-2, 6, len(grp))
            norms = ctx.post_newton(cj, kk, ids)
            for q, s in enumerate(ids):
                yy, yp, want = R.post_newton(st.v["yypredict"][s], st.v["yppredict"][s], st.v["ee"][s], st.v["ewt"][s], st.sys_phi(s), cj[q], kk[q])
                st.v["yy"][s], st.v["yp"][s] = yy, yp
                assert R.same_bits(norms[q], want), (n, kk[q], norms[q], want)
            st.check(("post_newton", grp))


@pytest.mark.parametrize("n", SIZES)
def test_complete_step_every_kused_maxord(ctxs, n):
    for atol_kind in ("scalar", "vector"):
        ctx, atol = vec_ctx(ctxs, n, atol_kind)
        rng = np.random.default_rng(5000 + n + (atol_kind == "vector"))
        st = Mirror(ctx, rng)
        idx = idx_of(ctx.batch)
        for maxord in range(1, 6):
            for grp in groups(combos(n, list(range(1, maxord + 1))), idx.size):
                ids = idx[:len(grp)]
                kused = np.array(grp)
                ck = rng.uniform(0.1, 3.0, len(grp))
                nrm, bad = ctx.complete_step(kused, ck, maxord, ids)
                for q, s in enumerate(ids):
                    phi, ee, ewt, want, wbad = R.complete_step(st.sys_phi(s), st.v["ee"][s], kused[q], ck[q], maxord, RTOL, atol)
                    st.phi[:, s, :], st.v["ee"][s], st.v["ewt"][s] = phi, ee, ewt
                    assert R.same_bits(np.float64(nrm[q]), np.float64(want)), (n, maxord, kused[q])
                    assert bool(bad[q]) == wbad, (n, maxord, kused[q])
                st.check(("complete_step", maxord, grp))
                st.phi = R.nasty(rng, st.phi.shape)  # fresh values: the recurrence would otherwise overflow everything
                st.v["ee"] = R.nasty(rng, st.v["ee"].shape)
                st.upload()


@pytest.mark.parametrize("n", SIZES)
def test_get_solution_every_kord_and_get_dky_every_range(ctxs, n):
    ctx, _ = vec_ctx(ctxs, n)
    rng = np.random.default_rng(6000 + n)
    st = Mirror(ctx, rng)
    idx = idx_of(ctx.batch)
    for grp in groups(combos(n, list(range(1, 6))), idx.size):
        ids = idx[:len(grp)]
        kord = np.array(grp)
        cv, dv = coeffs(rng, len(grp)), coeffs(rng, len(grp), 5)
        ctx.get_solution(kord, cv, dv, ids)
        for q, s in enumerate(ids):
            st.v["yy"][s], st.v["yp"][s] = R.get_solution(st.sys_phi(s), kord[q], cv[q], dv[q])
        st.check(("get_solution", grp))
    for grp in groups(combos(n, [(a, b) for b in range(6) for a in range(b + 1)]), idx.size):
        ids = idx[:len(grp)]
        k0, k1 = np.array([g[0] for g in grp]), np.array([g[1] for g in grp])
        cjk = coeffs(rng, len(grp))
        out = ctx.get_dky(k0, k1, cjk, ids)
        for q, s in enumerate(ids):
            assert R.same_bits(out[q], R.get_dky(st.sys_phi(s), k0[q], k1[q], cjk[q])), (n, grp[q])
    st.check("get_dky")


@pytest.mark.parametrize("n", [3, 257, 2050, 4096])
def test_complete_step_ewt_bad_follows_the_reference(ctxs, n):
    """impl_solve.rs:272 tests `x <= 0`: a new phi[0] component of +inf (ewt = 0) and a negative atol component make the state
    bad; a NaN component does not (NaN <= 0 is false), nor does a finite state. Before the fix the device tested !(w > 0),
    which reports the NaN system as bad."""
    import idahip
    ctx, _ = vec_ctx(ctxs, n)
    B = ctx.batch
    rng = np.random.default_rng(7000 + n)
    for case in ("finite", "inf", "negative_atol", "nan"):
        atol = atol_of(n, "vector")
        if case == "negative_atol":
            atol = atol.copy()
            atol[n // 2] = -1.0
        ctx.set_tolerances(RTOL, atol)
        phi = rng.uniform(-1.0, 1.0, (R.MXORDP1, B, n))
        ee = rng.uniform(-1e-3, 1e-3, (B, n))
        if case == "inf":
            phi[0, :, n - 1] = np.inf
        if case == "nan":
            ee[:, n // 3] = np.nan
        for j in range(R.MXORDP1):
            ctx.upload(idahip.F_PHI0 + j, phi[j])
        ctx.upload(idahip.F_EE, ee)
        ids = np.arange(B, dtype=np.int32)[::-1].copy()
        nrm, bad = ctx.complete_step(2, 0.5, 5, ids)
        for q, s in enumerate(ids):
            _, _, ewt, want, wbad = R.complete_step(phi[:, s, :], ee[s], 2, 0.5, 5, RTOL, atol)
            assert wbad == (case in ("inf", "negative_atol"))
            assert bool(bad[q]) == wbad, (n, case)
            assert R.same_bits(ctx.download(idahip.F_EWT)[s], ewt) and R.same_bits(np.float64(nrm[q]), np.float64(want)), (n, case)


@pytest.mark.parametrize("n", [3, 257, 4096])
def test_single_and_empty_lists_touch_nothing_else(ctxs, n):
    ctx, _ = vec_ctx(ctxs, n)
    rng = np.random.default_rng(8000 + n)
    st = Mirror(ctx, rng)
    empty = np.zeros(0, dtype=np.int32)
    ctx.predict([], [], np.zeros((0, 6)), np.zeros((0, 6)), empty)
    ctx.restore([], [], np.zeros((0, 6)), empty)
    ctx.scale_phi1([], empty)
    ctx.get_solution([], np.zeros((0, 6)), np.zeros((0, 5)), empty)
    assert ctx.post_newton([], [], empty).shape == (0, 4)
    assert ctx.complete_step([], [], 5, empty)[0].size == 0
    assert ctx.init_first(empty)[0].size == 0
    assert ctx.get_dky([], [], np.zeros((0, 6)), empty).shape == (0, n)
    st.check("empty lists")
    s = ctx.batch - 1
    beta, gamma = coeffs(rng, 1), coeffs(rng, 1)
    ctx.predict([3], [1], beta, gamma, [s])
    phi, st.v["yypredict"][s], st.v["yppredict"][s] = R.predict(st.sys_phi(s), 3, 1, beta[0], gamma[0])
    st.phi[:, s, :] = phi
    st.check("single system")


@pytest.mark.parametrize("n", [3, 257])
def test_bad_orders_are_refused_before_any_launch(ctxs, n):
    """Out-of-range kk / ns / kused / maxord / kord / derivative ranges are refused on the host and leave every field alone."""
    import idahip
    ctx, _ = vec_ctx(ctxs, n)
    st = Mirror(ctx, np.random.default_rng(9000 + n))
    ids = idx_of(ctx.batch)[:1]
    c6, c5 = np.ones((1, 6)), np.ones((1, 5))
    calls = [
        lambda: ctx.predict([0], [0], c6, c6, ids), lambda: ctx.predict([6], [0], c6, c6, ids), lambda: ctx.predict([2], [-1], c6, c6, ids),
        lambda: ctx.restore([0], [0], c6, ids), lambda: ctx.restore([6], [1], c6, ids), lambda: ctx.restore([3], [-1], c6, ids),
        lambda: ctx.post_newton([1.0], [0], ids), lambda: ctx.post_newton([1.0], [6], ids),
        lambda: ctx.complete_step([0], [1.0], 5, ids), lambda: ctx.complete_step([4], [1.0], 3, ids),
        lambda: ctx.complete_step([1], [1.0], 0, ids), lambda: ctx.complete_step([1], [1.0], 6, ids),
        lambda: ctx.get_solution([0], c6, c5, ids), lambda: ctx.get_solution([6], c6, c5, ids),
        lambda: ctx.get_dky([-1], [2], c6, ids), lambda: ctx.get_dky([3], [2], c6, ids), lambda: ctx.get_dky([0], [6], c6, ids),
    ]
    for k, call in enumerate(calls):
        with pytest.raises(idahip.IdaHipError):
            call()
        st.check(("refused", k))


@pytest.mark.parametrize("n", [3, 257, 4096])
def test_restore_initial_puts_back_phi01_yy_yp_of_the_listed_systems_only(ctxs, n):
    import idahip
    ctx, _ = vec_ctx(ctxs, n)
    rng = np.random.default_rng(9500 + n)
    st = Mirror(ctx, rng)
    ctx.snapshot_initial()
    y0, yp0 = st.phi[0].copy(), st.phi[1].copy()
    st.phi = R.nasty(rng, st.phi.shape)
    for f in VEC_FIELDS:
        st.v[f] = R.nasty(rng, st.v[f].shape)
    st.upload()
    ids = idx_of(ctx.batch)
    ctx.restore_initial(ids)
    for s in ids:
        st.phi[0, s], st.phi[1, s] = y0[s], yp0[s]
        st.v["yy"][s], st.v["yp"][s] = y0[s], yp0[s]
    st.check("restore_initial")
    with pytest.raises(idahip.IdaHipError):
        ctx.restore_initial([ctx.batch])
    st.check("restore_initial refused")


# ------------------------------------------------------------------------------------------------ Newton iteration body
def colmajor(mats):
    return np.ascontiguousarray(np.transpose(mats, (0, 2, 1)))


def block_sparse(rng, n, B):
    """Factors with all-zero 64 x 64 blocks for n >= 2048 (the zero-block map of the 1024-thread path): diagonal blocks, some
    sub- and super-diagonal blocks, one far block. The last (partial, when 64 does not divide n) block row carries a
    sub-diagonal block in system 0 and nothing but its diagonal block in system 1. System 2 is diagonal with positive entries:
    its L and U are all +0.0 off the diagonal, so every off-diagonal block is a zero block and a -0.0 entry of the right-hand
    side keeps its sign through the diagonal blocks. Where the reference subtracts 0 * b_k with b_k < 0 from it (the -0.0 run
    of rhs_of starts right after a run of ordinary values), -0.0 becomes +0.0; a skip of that zero block without the kernel's
    -0.0 guard would leave -0.0."""
    nb = (n + 63) // 64
    M = np.zeros((B, n, n))
    for s in range(B):
        for q in range(nb):
            r = slice(q * 64, min(n, (q + 1) * 64))
            w = r.stop - r.start
            M[s, r, r] = rng.standard_normal((w, w)) + 8.0 * np.eye(w)
            if q % 3 == 1:
                M[s, r, (q - 1) * 64:q * 64] = rng.standard_normal((w, 64))
            if q % 5 == 2 and q + 1 < nb - 1:
                M[s, r, (q + 1) * 64:(q + 2) * 64] = rng.standard_normal((w, 64))
        M[s, 20 * 64:21 * 64, 3 * 64:4 * 64] = rng.standard_normal((64, 64))
        last = slice((nb - 1) * 64, n)
        M[s, last, :(nb - 1) * 64] = 0.0
        if s == 0:
            M[s, last, (nb - 2) * 64:(nb - 1) * 64] = rng.standard_normal((n - (nb - 1) * 64, 64))
    if B > 2:
        M[2] = np.diag(rng.uniform(0.5, 4.0, n))
    return M


NEWTON_SIZES = [3, 8, 9, 511, 10, 512, 2047, 4095, 2048, 2050, 2120, 4094, 4096]


def newton_ctx(n, B, seed):
    """linear_dense ctx with A = 0 and J = B factored by nls_lsetup; returns (ctx, [(lu, piv)] per system)."""
    import idahip
    rng = np.random.default_rng(seed)
    if n >= 2048:
        Bm = block_sparse(rng, n, B)
    else:
        Bm = rng.standard_normal((B, n, n)) + 4.0 * np.eye(n)
    ctx = idahip.Ctx("linear_dense", n, B)
    ctx.set_tolerances(1e-6, 1e-8)
    ctx.set_linear_dense(np.zeros((B, n, n)), colmajor(Bm), np.zeros((B, n)))
    del Bm
    ctx.upload(idahip.F_YY, np.zeros((B, n)))
    ctx.upload(idahip.F_YP, np.zeros((B, n)))
    rc, info = ctx.nls_lsetup(0.0, 1.0)
    assert rc == 0 and not info.any()
    return ctx, [ctx.download_lu(s) for s in range(B)], rng


def rhs_of(rng, B, n):
    """-0.0 and +0.0 runs (after the negation) in systems 0 and 2; a second set with an infinity in system 2."""
    rhs = rng.standard_normal((B, n))
    for s in (0, 2):
        rhs[s, n // 8:n // 2] = 0.0      # -0.0 after the negation
        rhs[s, n // 2 + 1:] = -0.0       # +0.0 after the negation, the partial last block among them
    inf = rhs.copy()
    inf[2, n // 3] = np.inf              # spreads NaN / inf down the forward sweep and back up
    return rhs, inf


@pytest.mark.parametrize("n", NEWTON_SIZES)
def test_newton_iter_every_launch_path(n):
    """delta = -delta, getrs, *= scale (scale != 1), ee += delta (ee non-zero on entry), ||delta||: delta, ee and hDelnrm against
    stepper_ref, the system off the list unchanged."""
    import idahip
    B = 4 if n < 2048 else 3
    ctx, lus, rng = newton_ctx(n, B, 31 * n)
    ids = np.array([2, 0, 3] if B == 4 else [2, 0], dtype=np.int32)
    scale = np.array([2.0 / (1.0 + 1.3), 1.0, 2.0 / (1.0 + 0.7)])[:ids.size]
    ewt = rng.uniform(0.5, 2.0, (B, n))
    ctx.upload(idahip.F_EWT, ewt)
    for rhs in rhs_of(rng, B, n):
        ee = rng.standard_normal((B, n))
        ctx.upload(idahip.F_DELTA, rhs)
        ctx.upload(idahip.F_EE, ee)
        dn = ctx.newton_iter(scale, ids)
        got_d, got_e = ctx.download(idahip.F_DELTA), ctx.download(idahip.F_EE)
        for q, s in enumerate(ids):
            d, e, nrm = R.newton_iter(lus[s][0], lus[s][1], rhs[s], ee[s], ewt[s], scale[q])
            assert R.same_bits(got_d[s], d) and R.same_bits(got_e[s], e), (n, s)
            assert R.same_bits(np.float64(dn[q]), np.float64(nrm)), (n, s)
        assert R.same_bits(got_d[1], rhs[1]) and R.same_bits(got_e[1], ee[1])
    ctx.close()


@pytest.mark.parametrize("n", [3, 10, 511, 2050])
def test_newton_iter2_norms_and_exact_ties(n):
    """idahip_newton_iter2 decides idaNlsConvTest's m = 0 and m = 1 tests on the device with its own sqrt(sum / n). The linear
    problem with A = 0: the residual after the first correction is B (y + d) - c, so the second correction and its norm are
    computed by the reference too. hToldel, hSs and hEpsNewt are set so that each comparison is met with equality, and one ulp
    away on either side; systems that ended at m = 0 must not be touched by the second pass."""
    import idahip
    B = 12
    rng = np.random.default_rng(777 + n)
    Bm = rng.standard_normal((B, n, n)) + 4.0 * np.eye(n)
    c = rng.standard_normal((B, n))
    ctx = idahip.Ctx("linear_dense", n, B)
    ctx.set_tolerances(1e-6, 1e-8)
    ctx.set_linear_dense(np.zeros((B, n, n)), colmajor(Bm), c)
    yyp = rng.standard_normal((B, n))
    ewt = rng.uniform(0.5, 2.0, (B, n))
    ctx.upload(idahip.F_YYPREDICT, yyp)
    ctx.upload(idahip.F_YPPREDICT, rng.standard_normal((B, n)))
    ctx.upload(idahip.F_EWT, ewt)
    ids = np.arange(B, dtype=np.int32)
    rc, info = ctx.nls_sys_setup(0.0, 1.0, True, ids)
    assert rc == 0
    r0 = ctx.download(idahip.F_DELTA)
    lus = [ctx.download_lu(s) for s in range(B)]
    d0 = np.zeros(B)
    d1 = np.zeros(B)
    ee1 = np.zeros((B, n))
    ee2 = np.zeros((B, n))
    del2 = np.zeros((B, n))
    del1 = np.zeros((B, n))
    for s in range(B):
        del1[s], ee1[s], d0[s] = R.newton_iter(lus[s][0], lus[s][1], r0[s], np.zeros(n), ewt[s], 1.0)
        y = yyp[s] + ee1[s]
        acc = np.zeros(n)
        bm = colmajor(Bm[s:s + 1])[0]
        for j in range(n):                      # (ra + rb) - c with ra = 0 + A yp = +0.0 sums (A = 0), oracle/problems.hpp
            acc = acc + bm[j] * y[j]
        r1 = (np.zeros(n) + acc) - c[s]
        del2[s], ee2[s], d1[s] = R.newton_iter(lus[s][0], lus[s][1], r1, ee1[s], ewt[s], 1.0)
    # ties: system 3q + 0 on the toldel test, 3q + 1 on ss * d0 <= eps, 3q + 2 on ss1 * d1 <= eps (m = 1)
    toldel, ss, eps = np.full(B, 0.0), np.full(B, 0.0), np.full(B, 0.0)
    nudge = [0.0, 1.0, -1.0, -1.0]
    for s in range(B):
        which, side = s % 3, nudge[(s // 3) % 4]
        toldel[s] = d0[s] / 0.0001 * 0.5   # not met unless this system ties on it
        ss[s] = [1e-300, 3.0, 1.0][which]    # ss * d0 > eps unless this system ties on it
        eps[s] = 0.0
        if which == 0:
            t = d0[s] / 0.0001                # the smallest t with 0.0001 t >= d0 (the product is monotone in t) ...
            while 0.0001 * t >= d0[s]:
                t = np.nextafter(t, 0.0)
            lo = t                            # ... the t just below it, whose product is < d0 ...
            t = np.nextafter(t, np.inf)
            hi = t
            while 0.0001 * hi <= d0[s]:       # ... and the smallest t whose product is > d0
                hi = np.nextafter(hi, np.inf)
            toldel[s] = {0.0: t, 1.0: hi, -1.0: lo}[side]
        elif which == 1:
            ss[s] = 3.0
            e = ss[s] * d0[s]
            eps[s] = e if side == 0.0 else np.nextafter(e, np.inf if side > 0 else 0.0)
        else:
            rate = d1[s] / d0[s]
            e = (rate / (1.0 - rate)) * d1[s]
            eps[s] = e if side == 0.0 else np.nextafter(e, np.inf if side > 0 else 0.0)
    dn, conv = ctx.newton_iter2(1.0, 0.0, 1.0, toldel, ss, eps, ids)
    got_ee = ctx.download(idahip.F_EE)
    got_d = ctx.download(idahip.F_DELTA)
    for s in range(B):
        which, side = s % 3, nudge[(s // 3) % 4]
        # the comparison each system is set up on, evaluated as ctest_kernel does: equal at side 0, met one ulp up, not one down
        lhs, rhs_ = [(d0[s], 0.0001 * toldel[s]), (ss[s] * d0[s], eps[s]), ((d1[s] / d0[s]) / (1.0 - d1[s] / d0[s]) * d1[s], eps[s])][which]
        assert (lhs <= rhs_) == (side >= 0) and (lhs == rhs_) == (side == 0), (n, s, which, side, lhs, rhs_)
        assert d1[s] / d0[s] <= R.RATEMAX
        want = R.newton_ctest(d0[s], d1[s], toldel[s], ss[s], eps[s])
        assert want == ([1, 1, 2][which] if side >= 0 else [0, 2, 0][which]), (n, s, want)
        assert conv[s] == want, (n, s, conv[s], want)
        assert R.same_bits(np.float64(dn[s, 0]), np.float64(d0[s])), (n, s)
        if want == 1:   # ended at m = 0: the second pass leaves delta, ee and the second norm alone
            assert dn[s, 1] == 0.0 and R.same_bits(got_ee[s], ee1[s]) and R.same_bits(got_d[s], del1[s]), (n, s)
        else:
            assert R.same_bits(np.float64(dn[s, 1]), np.float64(d1[s])) and R.same_bits(got_ee[s], ee2[s]) and R.same_bits(got_d[s], del2[s]), (n, s)
    assert sorted(set(conv.tolist())) != [conv[0]], conv   # the ties go both ways
    ctx.close()


def test_newton_iter2_norms_bit_for_bit_over_many_systems():
    """The device's sqrt(sum / n) (ctest_kernel) against the oracle's norm over some hundreds of systems at random magnitudes."""
    import idahip
    n, B = 24, 384
    rng = np.random.default_rng(4242)
    Bm = rng.standard_normal((B, n, n)) + 4.0 * np.eye(n)
    ctx = idahip.Ctx("linear_dense", n, B)
    ctx.set_tolerances(1e-6, 1e-8)
    ctx.set_linear_dense(np.zeros((B, n, n)), colmajor(Bm), 10.0 ** rng.uniform(-100, 100, (B, 1)) * rng.standard_normal((B, n)))
    ctx.upload(idahip.F_YYPREDICT, np.zeros((B, n)))
    ctx.upload(idahip.F_YPPREDICT, np.zeros((B, n)))
    ewt = 10.0 ** rng.uniform(-3, 3, (B, n))
    ctx.upload(idahip.F_EWT, ewt)
    rc, _ = ctx.nls_sys_setup(0.0, 1.0, True)
    assert rc == 0
    r0 = ctx.download(idahip.F_DELTA)
    dn, conv = ctx.newton_iter2(1.0, 0.0, 1.0, 0.0, 0.0, np.inf, ctx.all_idx())  # every system converges at m = 0 (ss d0 <= inf)
    assert (conv == 1).all()
    for s in range(B):
        lu, piv = ctx.download_lu(s)
        _, _, d0 = R.newton_iter(lu, piv, r0[s], np.zeros(n), ewt[s], 1.0)
        assert R.same_bits(np.float64(dn[s, 0]), np.float64(d0)), s
    ctx.close()
