"""Pins tests/stepper_ref.py -- the float64 restatement the GPU tests of the stepper's entry points compare with -- on the CPU
oracle: random states are injected into an oracle `Ida` (OracleIda.setv / set) and the oracle's own seams are called
(set_coeffs + predict, restore, get_solution, get_dky, test_error, complete_step, and the first-call ewt_set of solve).
Where the oracle has no seam for a part, the test restates the reference text it follows. Runs without a GPU."""
import numpy as np
import pytest

import oracle_lib as O
import stepper_ref as R

N = 11            # >= 6: get_dky's coefficients are read back through unit vectors
RTOL = 1.0e-4


def atols(n):
    return {"scalar": 1.0e-6, "vector": 10.0 ** -np.linspace(3.0, 9.0, n)}


def oracle_ida(n=N, atol=1.0e-6, yy0=None, rtol=RTOL):
    yy0 = np.zeros(n) if yy0 is None else yy0
    return O.OracleIda("heat1d", n, yy0, np.zeros(n), rtol, atol, params=[1.0])


def inject(ida, phi, **scalars):
    ida.setv("phi", phi.ravel())
    for k, v in scalars.items():
        ida.set(k, v)


def state(seed, n=N, special=True):
    rng = np.random.default_rng(seed)
    return rng, R.nasty(rng, (R.MXORDP1, n), special)


def psi_of(rng, h):
    """psi_j = t_n - t_{n-j-1}: positive and increasing, as the stepper keeps it (lib.rs:722-782)."""
    return np.cumsum(h * rng.uniform(0.5, 2.0, size=R.MXORDP1))


@pytest.mark.parametrize("kk", [1, 2, 3, 4, 5])
def test_predict_matches_set_coeffs_and_predict(kk):
    """set_coeffs (lib.rs:722-782) computes ns = min(ns + 1, kused + 2) and beta, scales phi[ns..kk]; predict (lib.rs:894-959)
    sums. Every ns the reference reaches (1 .. kk + 1 with kused = kk; a changed order or step resets it to 1)."""
    cases = [(s, kk) for s in range(1, kk + 2)] + [(1, kk - 1)]
    for (ns_target, kused), special in [(c, sp) for c in cases for sp in (True, False)]:
        rng, phi = state(100 * kk + ns_target + 7 * kused + 1000 * special, special=special)
        h = 10.0 ** rng.uniform(-6, 1)
        ida = oracle_ida()
        inject(ida, phi, kk=kk, kused=kused, hh=h, hused=h, ns=ns_target - 1)
        ida.setv("psi", psi_of(rng, h))
        O.lib().oracle_ida_set_coeffs(ida.h)
        ns = int(ida.get("ns"))
        assert ns == ns_target
        beta, gamma = ida.getv("beta"), ida.getv("gamma")
        O.lib().oracle_ida_predict(ida.h)
        phi_r, yyp, ypp = R.predict(phi, kk, ns, beta, gamma)
        assert R.same_bits(phi_r, ida.getv("phi").reshape(R.MXORDP1, N)), (kk, ns)
        assert R.same_bits(yyp, ida.getv("yypredict")), (kk, ns)
        assert R.same_bits(ypp, ida.getv("yppredict")), (kk, ns)


def test_predict_with_ns_zero_scales_phi0_by_beta0():
    """ns = 0 never comes out of set_coeffs (ns >= 1), but the entry point accepts it: phi[0] *= beta[0] = 1 leaves phi[0]'s bits
    as they are, so the result is the set_coeffs + predict result with ns = 1."""
    rng, phi = state(5)
    beta = np.concatenate([[1.0], rng.uniform(0.5, 2.0, 5)])
    gamma = rng.uniform(-2.0, 2.0, 6)
    for kk in range(1, 6):
        a = R.predict(phi, kk, 0, beta, gamma)
        b = R.predict(phi, kk, 1, beta, gamma)
        assert all(R.same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("kk", [1, 2, 3, 4, 5])
def test_restore_matches_the_oracle(kk):
    """IDARestore (lib.rs:1044-1083): cvals[j - ns] = 1 / beta[j], phi[j] *= cvals[j - ns] for j = ns..kk; every 0 <= ns <= kk + 1."""
    for ns in range(0, kk + 2):
        rng, phi = state(200 * kk + ns)
        h = 10.0 ** rng.uniform(-6, 1)
        beta = rng.uniform(0.25, 4.0, R.MXORDP1) * rng.choice([1.0, -1.0], R.MXORDP1)
        ida = oracle_ida()
        inject(ida, phi, kk=kk, ns=ns, hh=h)
        ida.setv("beta", beta)
        ida.setv("psi", psi_of(rng, h))
        ida.setv("cvals", np.zeros(R.MXORDP1))
        O.lib().oracle_ida_restore(ida.h, 0.5)
        cvals = ida.getv("cvals")
        for j in range(ns, kk + 1):
            assert cvals[j - ns] == 1.0 / beta[j]
        assert R.same_bits(R.restore(phi, kk, ns, cvals), ida.getv("phi").reshape(R.MXORDP1, N)), (kk, ns)


@pytest.mark.parametrize("special", [True, False], ids=["spread", "ordinary"])
@pytest.mark.parametrize("kused", [0, 1, 2, 3, 4, 5])
def test_get_solution_matches_the_oracle(kused, special):
    """IDAGetSolution (lib.rs:1274-1343): kord = kused (1 when kused = 0); cvals / dvals from psi, then the two scaled sums.
    Ordinary magnitudes make the summation order show in the bits; the spread values bring zeros, subnormals and overflow."""
    rng, phi = state(300 + kused + 1000 * special, special=special)
    h = 10.0 ** rng.uniform(-6, 1)
    ida = oracle_ida()
    inject(ida, phi, kused=kused, hh=h, hused=h, tn=1.0)
    ida.setv("psi", psi_of(rng, h))
    assert O.lib().oracle_ida_get_solution(ida.h, 1.0 - 0.3 * h) == 0
    kord = max(kused, 1)
    yy, yp = R.get_solution(phi, kord, ida.getv("cvals"), ida.getv("dvals"))
    assert R.same_bits(yy, ida.getv("yy")) and R.same_bits(yp, ida.getv("yp"))


@pytest.mark.parametrize("special", [True, False], ids=["spread", "ordinary"])
@pytest.mark.parametrize("kused", [0, 1, 2, 3, 4, 5])
def test_get_dky_matches_the_oracle(kused, special):
    """IDAGetDky (lib.rs:424-529) through oracle_ida_get_dky for every k <= kused: the coefficients c_j^(k) are read back by a
    first call on unit vectors (phi[j] = e_j gives dky_j = 0 + 1 * c_j), the second call on a random state is compared with
    stepper_ref.get_dky(phi, k, kused, c). Ordinary magnitudes as well as spread ones, as for get_solution."""
    rng, phi = state(400 + kused + 1000 * special, special=special)
    h = 10.0 ** rng.uniform(-6, 1)
    psi = psi_of(rng, h)
    t = 1.0 - 0.3 * h
    for k in range(0, kused + 1):
        ida = oracle_ida()
        inject(ida, np.eye(R.MXORDP1, N), kused=kused, hh=h, hused=h, tn=1.0)
        ida.setv("psi", psi)
        st, unit = ida.get_dky(t, k)
        assert st == 0
        cjk = np.zeros(R.MXORDP1)
        cjk[k:kused + 1] = unit[k:kused + 1]
        inject(ida, phi)
        st, dky = ida.get_dky(t, k)
        assert st == 0
        assert R.same_bits(R.get_dky(phi, k, kused, cjk), dky), (kused, k)


@pytest.mark.parametrize("atol", ["scalar", "vector"])
def test_ewt_set_and_init_first_match_the_oracle(atol):
    """ewt_set (tol_control.rs:36-44, 71-82) through the oracle's first solve call: it sets ewt from phi[0] and returns
    IDA_ILL_INPUT at tout == tn before anything else (impl_solve.rs:120-140). Values with zeros of both signs, subnormals,
    infinities and NaN."""
    rng, phi = state(500)
    phi[0, 1], phi[0, 2], phi[0, 3] = np.inf, -np.inf, np.nan
    a = atols(N)[atol]
    ida = oracle_ida(atol=a, yy0=phi[0])
    st, _ = ida.solve(0.0)
    assert st < 0
    ewt, ypn, p0n = R.init_first(phi, RTOL, a)
    assert R.same_bits(ewt, ida.getv("ewt"))
    assert ewt[1] == 0.0 and ewt[2] == 0.0 and np.isnan(ewt[3])
    assert R.same_bits(np.float64(ypn), np.float64(O.wrms(phi[1], ewt))) and np.isnan(p0n)  # inf * 0 in the sum


@pytest.mark.parametrize("kk", [1, 2, 3, 4, 5])
def test_post_newton_norms_match_test_error(kk):
    """The first three norms against the oracle's test_error (lib.rs:967-1039) with sigma = 1 (err_k = ||ee||, err_km1 =
    ||phi[kk] + ee||; the delta it leaves behind is phi[kk] + ee, + phi[kk-1] when kk > 2). The fourth against the text of
    impl_complete_step.rs:74-77 (temp = ee - phi[kk+1], only when kk + 1 < 6). yy / yp against lib.rs:845-849."""
    for atol in ("scalar", "vector"):
        rng, phi = state(600 + kk, special=False)
        ee = R.nasty(rng, N, special=False)
        ewt = R.ewt_set(phi[0], RTOL, atols(N)[atol])
        yyp, ypp = R.nasty(rng, N), R.nasty(rng, N)
        cj = 10.0 ** rng.uniform(-3, 6)
        ida = oracle_ida()
        inject(ida, phi, kk=kk)
        ida.setv("ee", ee)
        ida.setv("ewt", ewt)
        ida.setv("sigma", np.ones(R.MXORDP1))
        ek, ekm1 = O.C.c_double(), O.C.c_double()
        O.lib().oracle_ida_test_error(ida.h, 1.0, O.C.byref(ek), O.C.byref(ekm1))
        yy, yp, norms = R.post_newton(yyp, ypp, ee, ewt, phi, cj, kk)
        assert norms[0] == ek.value
        assert norms[1] == (ekm1.value if kk > 1 else 0.0)
        assert norms[2] == (O.wrms(ida.getv("delta"), ewt) if kk > 2 else 0.0)
        assert norms[3] == (O.wrms(ee - phi[kk + 1], ewt) if kk < 5 else 0.0)
        assert R.same_bits(yy, yyp + ee) and R.same_bits(yp, ypp + cj * ee)


@pytest.mark.parametrize("maxord", [1, 2, 3, 4, 5])
def test_complete_step_matches_the_oracle(maxord):
    """complete_step (impl_complete_step.rs:22-177) on an injected state with its scalar decisions fixed (nst = 0, phase 0: no
    order or step change that reads phi): kused = kk, phi[kused + 1] = ee when kused < maxord, then the recurrence. The oracle
    applies ee *= ck in step() after complete_step (lib.rs:708) and ewt_set at the next pass of the solve loop (impl_solve.rs:
    266-272): both checked on their own, the second through the first-call seam of solve."""
    for kused in range(1, maxord + 1):
        for atol in ("scalar", "vector"):
            rng, phi = state(700 + 10 * maxord + kused)
            ee = R.nasty(rng, N)
            ck = rng.uniform(0.1, 2.0)
            a = atols(N)[atol]
            ida = oracle_ida(atol=a)
            inject(ida, phi, kk=kused, kused=kused, knew=kused, maxord=maxord, nst=0, phase=0, hh=1.0)
            ida.setv("ee", ee)
            ewt_before = ida.getv("ewt")
            O.lib().oracle_ida_complete_step(ida.h, 0.0, 0.0)
            phi_r, ee_r, ewt_r, nrm, bad = R.complete_step(phi, ee, kused, ck, maxord, RTOL, a)
            assert R.same_bits(phi_r, ida.getv("phi").reshape(R.MXORDP1, N)), (maxord, kused)
            assert R.same_bits(ida.getv("ee"), ee) and R.same_bits(ida.getv("ewt"), ewt_before)
            assert R.same_bits(ee_r, ee * ck)
            nxt = oracle_ida(atol=a, yy0=phi_r[0])
            assert nxt.solve(0.0)[0] < 0
            assert R.same_bits(ewt_r, nxt.getv("ewt"))
            assert R.same_bits(np.float64(nrm), np.float64(O.wrms(phi_r[0], ewt_r)))


def test_ewt_check_follows_the_reference_predicate():
    """impl_solve.rs:272: `ewt.iter().any(|&x| x <= 0)` -- an infinite phi[0] component (ewt = 0) or a negative atol component
    makes the state bad; a NaN component does not (NaN <= 0 is false), nor does a finite state."""
    n = 5
    phi = np.zeros((R.MXORDP1, n))
    phi[0] = [1.0, -2.0, 0.5, 3.0, 1e-300]
    ee = np.zeros(n)

    def bad(p0, atol):
        ph = phi.copy()
        ph[0] = p0
        return R.complete_step(ph, ee, 1, 1.0, 5, RTOL, atol)[4]

    assert not bad(phi[0], 1e-6)
    assert bad(np.where(np.arange(n) == 2, np.inf, phi[0]), 1e-6)
    assert bad(phi[0], np.array([1e-6, 1e-6, -1e-3, 1e-6, 1e-6]))
    assert not bad(np.where(np.arange(n) == 2, np.nan, phi[0]), 1e-6)


def test_newton_iter_matches_the_oracle_solver():
    """Newton loop body (newton.rs:98-110) against the oracle's Dense LSolver (dense.rs:15-64: x <- b, getrs) on a factored
    random matrix; the scale and the ee update against ida_ls.rs:406-410 and newton.rs:106."""
    rng = np.random.default_rng(800)
    n = 17
    a = rng.standard_normal((n, n)) + 4 * np.eye(n)
    info, lu, piv = O.getrf(a)
    assert info == 0
    delta = R.nasty(rng, n, special=False)
    delta[3], delta[4] = 0.0, -0.0
    ee, ewt = rng.standard_normal(n), rng.uniform(0.5, 2.0, n)
    x = np.zeros(n)
    cm = np.asfortranarray(a).copy(order="F")
    b = -delta
    assert O.lib().oracle_dense_lsolver(cm.ctypes.data_as(O.dp), n, b.ctypes.data_as(O.dp), x.ctypes.data_as(O.dp),
                                        np.zeros(n, dtype=np.int64).ctypes.data_as(O.i64p)) == 0
    for scale in (1.0, 2.0 / (1.0 + 1.3)):
        d, e, nrm = R.newton_iter(lu, piv, delta, ee, ewt, scale)
        assert R.same_bits(d, x * scale) and R.same_bits(e, ee + x * scale) and nrm == O.wrms(x * scale, ewt)


def test_newton_ctest_follows_ida_nls_conv_test():
    """idaNlsConvTest (ida_nls.rs:218-266) for m = 0 and m = 1: the codes at and around every tie."""
    toldel, eps = 1e-3, 1e-2
    d0 = 0.0001 * toldel
    assert R.newton_ctest(d0, None, toldel, 0.0, 0.0) == 1
    assert R.newton_ctest(np.nextafter(d0, 1.0), 1.0, toldel, 1.0, 0.0) == 3
    d0 = 0.5
    assert R.newton_ctest(d0, None, toldel, eps / d0, eps) == 1
    d1 = np.nextafter(0.9 * d0, 1.0)
    assert d1 / d0 > 0.9 and R.newton_ctest(d0, d1, toldel, 100.0, eps) == 3
    d1 = 0.25 * d0
    rate = d1 / d0
    e1 = (rate / (1.0 - rate)) * d1
    assert R.newton_ctest(d0, d1, toldel, 100.0, e1) == 2
    assert R.newton_ctest(d0, d1, toldel, 100.0, np.nextafter(e1, 0.0)) == 0

