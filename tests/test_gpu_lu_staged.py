"""Staged L (idahip_set_lu_staged): the ctx's own factors keep L21 of every 64-column super-panel in the order of the live list
behind it -- written by lu_wavepanel_kernel's epilogue (diagonal block, maps, perm) and by the first column block's workgroup of
lu_trail64w_kernel<1024> --, the factorisation launches no lu_finalize_kernel, and the solves (wg_getrs<.., true> in
newton_iter_kernel and the IC solves) permute their right-hand side block by block with the maps.

Bar: array_equal on bit patterns (signs of zeros count) against
  * the oracle's getrf / getrs of J = B + cj*A formed on the host (a multiply, then an add). Where the oracle has a NaN the GPU
    must have a NaN: sign and payload of a NaN are not part of the contract (tests/test_gpu_lsolver.py draws the same line);
  * the same ctx with the switch off: every bit, NaNs included.
Sizes: one super-panel and no trailing launch (64); a one-column and an eight-column last super-panel, SLOW path with a partial
block (65, 72); two super-panels (128); a partial trailing block (130, 200); every slot count up to eight (448, 512). Batch 9: the
trailing grid's (slot / wpm) * 8 + xcd dealing wraps.
"""
import numpy as np
import pytest

import calcic_cases as K
import oracle_lib as O

pytestmark = pytest.mark.gpu

U64 = np.uint64
SIZES = [64, 65, 72, 128, 130, 200, 448, 512]
BATCH = 9
LIST = [7, 2, 5]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(U64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def same_as_oracle(got, want):
    """bit for bit where the oracle has numbers, NaN where it has NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(want[~nan]))


def rand_ab(n, batch, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    A = rng.standard_normal((batch, n, n))
    B = rng.standard_normal((batch, n, n)) + 3.0 * np.eye(n)
    return A, B


def ctx_of(A, B, staged, jac_in_lu=None):
    import idahip
    batch, n = A.shape[0], A.shape[1]
    ctx = idahip.Ctx("linear_dense", n, batch)
    ctx.set_tolerances(1.0e-6, np.array([1.0e-8]))
    ctx.set_linear_dense(A, B, np.zeros((batch, n)))
    ctx.set_lu_staged(staged)
    assert ctx.lu_staged() == (1 if staged else 0)
    if jac_in_lu is not None:
        ctx.set_jac_in_lu(jac_in_lu)
    return ctx


def oracle(A, B, cj, idx):
    """-> info, factors [len(idx)][n][n] in column-major storage, pivots"""
    cj = np.broadcast_to(np.asarray(cj, dtype=np.float64), (len(idx),))
    with np.errstate(all="ignore"):
        J = np.ascontiguousarray(B[idx] + cj[:, None, None] * A[idx])  # multiply, then add
    info, piv = O.getrf_batch(J, nthreads=4)
    return info, J, piv


def rhs_of(rng, batch, n):
    """random, with -0.0 and +0.0 runs in systems 0 and 2 (the negation turns them round)"""
    rhs = rng.standard_normal((batch, n))
    for s in (0, 2):
        if s < batch:
            rhs[s, n // 8:n // 2] = 0.0
            rhs[s, n // 2 + 1:] = -0.0
    return rhs


def oracle_newton(lu, piv, rhs, ee, ewt, scale):
    """newton.rs:98-110 for every listed system: delta = -delta; getrs; *= scale; ee += delta; wrms -> delta, ee, norms"""
    with np.errstate(all="ignore"):
        x = O.getrs_batch(np.ascontiguousarray(lu), piv, -rhs, nthreads=4) * scale[:, None]
        e = ee + x
    return x, e, np.array([O.wrms(x[q], ewt[q]) for q in range(x.shape[0])])


def factor_and_solve(ctx, cj, idx, rhs, ee, ewt, scale):
    """idahip_nls_lsetup of the list, download_lu, idahip_newton_iter of the list -> info, factors (storage order), pivots, delta, ee, norms"""
    import idahip
    rc, info = ctx.nls_lsetup(0.0, cj, idx)
    lus, pivs = [], []
    for s in idx:
        lu, piv = ctx.download_lu(int(s))
        lus.append(lu.T.copy())
        pivs.append(piv)
    ctx.upload(idahip.F_EWT, ewt)
    ctx.upload(idahip.F_DELTA, rhs)
    ctx.upload(idahip.F_EE, ee)
    dn = ctx.newton_iter(scale, idx)
    return info, np.array(lus), np.array(pivs), ctx.download(idahip.F_DELTA), ctx.download(idahip.F_EE), dn


def check(A, B, cj, idx=None, expect_info=None, jac_in_lu=None, seed=1):
    """staged == oracle and staged == reference layout, factors and a Newton iteration; unlisted systems untouched -> info"""
    batch, n = A.shape[0], A.shape[1]
    idx = np.arange(batch, dtype=np.int32) if idx is None else np.asarray(idx, dtype=np.int32)
    rng = np.random.Generator(np.random.PCG64(seed))
    rhs, ee, ewt = rhs_of(rng, batch, n), rng.standard_normal((batch, n)), rng.uniform(0.5, 2.0, (batch, n))
    scale = np.linspace(0.8, 1.0, idx.size)
    i_o, lu_o, piv_o = oracle(A, B, cj, idx)
    if expect_info is not None:
        assert np.array_equal(i_o, expect_info), i_o
    ok = i_o == 0  # (a matrix with a zero pivot: the verdict is the result; what its factors hold afterwards is not specified -- include/ida_hip.h)
    d_o, e_o, n_o = oracle_newton(lu_o[ok], piv_o[ok], rhs[idx][ok], ee[idx][ok], ewt[idx][ok], scale[ok])
    got = {}
    for staged in (True, False):
        ctx = ctx_of(A, B, staged, jac_in_lu)
        ctx.timing(True)
        got[staged] = factor_and_solve(ctx, cj, idx, rhs, ee, ewt, scale)
        fin = ctx.timing_get()["lu_finalize"]["launches"]
        assert (fin == 0) if staged else (fin > 0), fin
        ctx.close()
        info, lu, piv, d, e, dn = got[staged]
        assert np.array_equal(info, i_o), (staged, info, i_o)
        assert np.array_equal(piv[ok], piv_o[ok]), staged
        assert same_as_oracle(lu[ok], lu_o[ok]), staged
        assert same_as_oracle(d[idx][ok], d_o) and same_as_oracle(e[idx][ok], e_o) and same_as_oracle(dn[ok], n_o), staged
        off = np.setdiff1d(np.arange(batch), idx)
        assert same_bits(d[off], rhs[off]) and same_bits(e[off], ee[off])
    on, of = got[True], got[False]
    assert same_bits(on[1][ok], of[1][ok]) and np.array_equal(on[2][ok], of[2][ok])
    assert same_bits(on[3][idx][ok], of[3][idx][ok]) and same_bits(on[4][idx][ok], of[4][idx][ok]) and same_bits(on[5][ok], of[5][ok])
    return i_o


# ---------------------------------------------------------------------------------------------------------------- sizes and lists
@pytest.mark.parametrize("idx", [None, LIST], ids=["all", "list"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_lists(n, idx):
    A, B = rand_ab(n, BATCH, 100 + n)
    cj = np.linspace(0.5, 120.0, BATCH if idx is None else len(idx))
    assert (check(A, B, cj, idx) == 0).all()


@pytest.mark.parametrize("n", [9, 40, 63])
def test_a_single_partial_super_panel(n):
    """fewer than 64 rows: one super-panel, SLOW launch, no trailing launch, one map"""
    A, B = rand_ab(n, BATCH, 150 + n)
    assert (check(A, B, 7.0) == 0).all()
    assert (check(A, B, np.linspace(1.0, 3.0, len(LIST)), LIST) == 0).all()


@pytest.mark.parametrize("n", [130, 200, 512])
def test_with_j_formed_inside_the_factorisation(n):
    """idahip_set_jac_in_lu: the J-forming instantiations of the panel and trailing kernels write the staged layout too."""
    A, B = rand_ab(n, BATCH, 200 + n)
    assert (check(A, B, np.linspace(1.0, 9.0, len(LIST)), LIST, jac_in_lu=True) == 0).all()
    assert (check(A, B, 3.0, None, jac_in_lu=True) == 0).all()


def test_default_and_refusals():
    """Never set: staged where n > 448, on request below. n = 513, n = 8: refused; LU variant 3: the reference layout while it lasts."""
    import idahip
    for n, want in ((512, 1), (449, 1), (448, 0), (130, 0), (9, 0)):
        c = idahip.Ctx("linear_dense", n, 2)
        assert c.lu_staged() == want, n
        c.close()
    ctx = idahip.Ctx("linear_dense", 130, 2)
    ctx.set_lu_staged(True)
    assert ctx.lu_staged() == 1
    ctx.set_lu_staged(False)
    assert ctx.lu_staged() == 0
    ctx.set_lu_staged(True)
    ctx.set_lu_variant(3)
    assert ctx.lu_staged() == 0
    ctx.set_lu_variant(4)
    assert ctx.lu_staged() == 1
    ctx.close()
    for n in (513, 8):
        c = idahip.Ctx("linear_dense", n, 2)
        assert c.lu_staged() == 0 and c.H.idahip_set_lu_staged(c.h, 1) == -2 and c.H.idahip_set_lu_staged(c.h, 0) == 0
        c.close()
    assert ctx.H.idahip_set_lu_staged(None, 1) == -1 and ctx.H.idahip_lu_staged(None) == -1


# ---------------------------------------------------------------------------------------------------------------- matrices
def first_pivot_rows(A, B, cj, s, upto=64):
    """the rows of system s that become the first `upto` pivot rows (from the oracle's pivots)"""
    n = A.shape[1]
    _, _, piv = oracle(A, B, cj, np.array([s]))
    rows = np.arange(n)
    for k in range(min(upto, n)):
        p = int(piv[0, k])
        rows[[k, p]] = rows[[p, k]]
    return rows[: min(upto, n)]


@pytest.mark.parametrize("n", [72, 130, 200])
def test_ties_in_absolute_value(n):
    A, B = rand_ab(n, BATCH, 41 + n)
    A[:] = np.sign(A)
    B[:] = np.sign(B)          # every entry of J is +-1 +- cj: ties in |a| in every column
    check(A, B, 2.0)
    A2, B2 = rand_ab(n, BATCH, 42 + n)
    B2[0, 0, :] = 3.0; A2[0, 0, :] = 1.0       # column 0 constant: the first pivot is a tie of all rows
    B2[1, :70, 7] = -B2[1, :70, 11]; A2[1, :70, 7] = -A2[1, :70, 11]  # two rows of opposite sign across the first super-panel
    assert (check(A2, B2, 0.75) == 0).all()


@pytest.mark.parametrize("n", [130, 200])
def test_exact_zeros_in_pivot_rows(n):
    """An exact zero among a pivot row's entries right of the first super-panel (the trailing prologue's per-entry path), a pivot
    row that is zero right of the super-panel, the 64 pivot rows zero across the whole first column block (that block's workgroup
    leaves before its strips and must still write L21), and a zero U entry inside the super-panel (FAST -> SLOW hand-over)."""
    cj = 2.0  # (a power of two: cj*a is exact, b = -cj*a gives +0.0)
    A, B = rand_ab(n, BATCH, 300 + n)
    pr = first_pivot_rows(A, B, cj, 0)
    B[0, 64 + (n - 64) // 2, pr[5]] = -cj * A[0, 64 + (n - 64) // 2, pr[5]]
    pr1 = first_pivot_rows(A, B, cj, 1)
    B[1, 64:, pr1[9]] = -cj * A[1, 64:, pr1[9]]
    pr2 = first_pivot_rows(A, B, cj, 2)
    B[2, 20, pr2[3]] = -cj * A[2, 20, pr2[3]]
    pr3 = first_pivot_rows(A, B, cj, 3)
    B[3, 64:128, pr3] = -cj * A[3, 64:128, pr3]  # U12 of the first column block is all zeros; the rows below it are not
    assert np.array_equal(first_pivot_rows(A, B, cj, 3), pr3)
    pr8 = first_pivot_rows(A, B, cj, 8)
    B[8, 64:128, pr8[:32]] = -cj * A[8, 64:128, pr8[:32]]  # its first 32 pivot rows only
    info = check(A, B, cj)
    assert (info == 0).all(), info
    assert (check(A, B, cj, LIST + [3, 8]) == 0).all()


@pytest.mark.parametrize("n", [72, 130])
def test_nan_and_infinity(n):
    A, B = rand_ab(n, BATCH, 500 + n)
    c2 = n - 3  # a column right of the first super-panel
    A[0, 5, 5] = np.nan
    B[1, 9, n - 2] = np.nan
    A[2, 3, 17] = np.inf
    B[3, c2, 20] = -np.inf
    A[4, c2, 33] = np.nan
    B[5, 2, 2] = np.inf
    check(A, B, 1.5)


@pytest.mark.parametrize("n", [72, 130, 200])
def test_one_singular_system_among_healthy_ones(n):
    """info is the reference's 1-based column; the neighbours are factored and solved."""
    cj = 4.0
    A, B = rand_ab(n, BATCH, 600 + n)
    B[1, 10, :] = -cj * A[1, 10, :]            # column 10 of J is zero: zero pivot at step 11
    B[4, n - 2, :] = -cj * A[4, n - 2, :]      # in the last super-panel
    B[6, 64, :] = -cj * A[6, 64, :]            # the second super-panel's first column: found after a trailing update
    info = check(A, B, cj)
    assert info[1] == 11 and info[4] == n - 1 and info[6] == 65 and (info[[0, 2, 3, 5, 7, 8]] == 0).all(), info
    check(A, B, cj, [7, 1, 5, 4])


# ---------------------------------------------------------------------------------------------------------------- partial updates
@pytest.mark.parametrize("n", [72, 130, 512])
def test_refactoring_a_subset_leaves_the_others_factors_and_maps(n):
    """All systems at one cj, a subset again at another, then a Newton iteration of all: every system answers with the factors it
    was last given."""
    import idahip
    A, B = rand_ab(n, BATCH, 700 + n)
    allidx = np.arange(BATCH, dtype=np.int32)
    sub = np.array(LIST, dtype=np.int32)
    cj1, cj2 = 2.5, 40.0
    rng = np.random.Generator(np.random.PCG64(n))
    rhs, ee, ewt = rhs_of(rng, BATCH, n), rng.standard_normal((BATCH, n)), rng.uniform(0.5, 2.0, (BATCH, n))
    scale = np.ones(BATCH)
    cjs = np.full(BATCH, cj1)
    cjs[sub] = cj2
    i_o, lu_o, piv_o = oracle(A, B, cjs, allidx)
    assert (i_o == 0).all()
    d_o, e_o, n_o = oracle_newton(lu_o, piv_o, rhs, ee, ewt, scale)
    for staged in (True, False):
        ctx = ctx_of(A, B, staged)
        rc, info = ctx.nls_lsetup(0.0, cj1, allidx)
        assert not info.any()
        rc, info = ctx.nls_lsetup(0.0, cj2, sub)
        assert not info.any()
        for s in range(BATCH):
            lu, piv = ctx.download_lu(s)
            assert same_bits(lu.T, lu_o[s]) and np.array_equal(piv, piv_o[s]), (staged, s)
        ctx.upload(idahip.F_EWT, ewt); ctx.upload(idahip.F_DELTA, rhs); ctx.upload(idahip.F_EE, ee)
        dn = ctx.newton_iter(scale, allidx)
        assert same_bits(ctx.download(idahip.F_DELTA), d_o) and same_bits(ctx.download(idahip.F_EE), e_o) and same_bits(dn, n_o), staged
        ctx.close()


@pytest.mark.parametrize("n", [72, 200])
def test_user_buffers_keep_the_reference_layout(n):
    """idahip_ls_setup / idahip_ls_solve on caller-owned matrices on a staged ctx, between two uses of the ctx's own factors."""
    import idahip
    A, B = rand_ab(n, BATCH, 800 + n)
    idx = np.array(LIST, dtype=np.int32)
    ctx = ctx_of(A, B, True)
    rc, info = ctx.nls_lsetup(0.0, 2.0)
    assert not info.any()
    rng = np.random.Generator(np.random.PCG64(5 + n))
    M = np.ascontiguousarray(rng.standard_normal((BATCH, n, n)) + 2.0 * np.eye(n))  # column-major storage of each matrix
    rhs = rng.standard_normal((BATCH, n))
    lu_o = M[idx].copy()
    i_o, piv_o = O.getrf_batch(lu_o, nthreads=4)
    x_o = O.getrs_batch(lu_o, piv_o, rhs[idx], nthreads=4)
    dA, dP = ctx.dev_array(M), ctx.dev_empty(8 * BATCH * n)
    dB, dX = ctx.dev_array(rhs), ctx.dev_array(np.zeros((BATCH, n)))
    rc, info = ctx.ls_setup(dA, dP, idx)
    assert not info.any()
    assert same_bits(ctx.to_host(dA, (BATCH, n, n))[idx], lu_o)
    assert np.array_equal(ctx.to_host(dP, (BATCH, n), dtype=np.int64)[idx], piv_o)
    ctx.ls_solve(dA, dP, dX, dB, idx)
    assert same_bits(ctx.to_host(dX, (BATCH, n))[idx], x_o)
    for d in (dA, dP, dB, dX):
        ctx.dev_free(d)
    # the ctx's own factors are what they were
    i2, lu2, piv2 = oracle(A, B, 2.0, np.arange(BATCH))
    for s in range(BATCH):
        lu, piv = ctx.download_lu(s)
        assert same_bits(lu.T, lu2[s]) and np.array_equal(piv, piv2[s])
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- full schedules
def run_schedule(prob, device_ctl, staged):
    import idahip
    from idahip import problems
    ctx = problems.make_ctx(prob)
    ctx.set_lu_staged(staged)
    ctx.timing(True)
    ens = idahip.Ensemble(ctx, prob["yy0"], prob["yp0"])
    ens.set_device_controller(device_ctl)
    sts = []
    for t in prob["touts"][:3]:
        status, tret = ens.solve(t)
        sts.append(status.copy())
    c = ens.counters()
    fin = ctx.timing_get()["lu_finalize"]["launches"]
    assert set(c) == set(idahip.COUNTERS)  # every counter the ensemble keeps
    out = {**c, "status": np.array(sts), "yy": ens.yy(), "yp": ens.yp(), "tn": ens.real("tn"), "hh": ens.real("hh")}
    ens.close()
    ctx.close()
    return out, fin


@pytest.fixture(scope="module")
def ensembles():
    from idahip import problems
    return {n: problems.linear_dense(n=n, batch=BATCH, procs=1) for n in (64, 200)}


@pytest.mark.parametrize("device_ctl", [1, 0], ids=["device_rounds", "host_stepper"])
@pytest.mark.parametrize("n", [64, 200])
def test_full_schedule_switch_on_equals_switch_off(ensembles, n, device_ctl):
    s1, f1 = run_schedule(ensembles[n], device_ctl, True)
    s0, f0 = run_schedule(ensembles[n], device_ctl, False)
    assert (s1["status"] == 0).all()
    for k in s1:
        assert same_bits(s1[k], s0[k]) if s1[k].dtype == np.float64 else np.array_equal(s1[k], s0[k]), k
    assert f1 == 0 and f0 > 0


@pytest.mark.parametrize("name", ["linear40_mixed", "linear40_singular", "linear512_mixed"])
def test_calc_ic_switch_on_equals_switch_off(name):
    import idahip
    c = K.case(name)
    out = []
    for staged in (True, False):
        ctx = K.make_ctx(c)
        ctx.set_lu_staged(staged)
        ens = idahip.Ensemble(ctx, c["yy0"], c["yp0"])
        status = ens.calc_ic(c["icopt"], c["tout1"])
        out.append((status, ens.yy(), ens.yp(), ctx.download(idahip.F_EWT), ens.counters()))
        ens.close()
        ctx.close()
    (st1, y1, p1, w1, c1), (st0, y0, p0, w0, c0) = out
    assert np.array_equal(st1, st0)
    assert (st1 != 0).sum() == (1 if name == "linear40_singular" else 0), st1
    assert same_bits(y1, y0) and same_bits(p1, p0) and same_bits(w1, w0)
    for k in c1:
        assert np.array_equal(c1[k], c0[k]), k
