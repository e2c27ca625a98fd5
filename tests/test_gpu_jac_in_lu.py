"""J = B + cj*A formed inside the first launches of the batched LU (idahip_set_jac_in_lu; lu_wavepanel_kernel<.., LuJac> and
lu_trail64w_kernel<1024, LuJac>) instead of by the residual / Jacobian kernels into the work matrix.

Bar: array_equal on bit patterns (signs of zeros count) against two references --
  * the oracle's getrf of J formed on the host as B + cj*A in numpy (a multiply, then an add: no FMA). Where the oracle has a NaN
    the GPU must have a NaN: sign and payload of a NaN are not part of the contract (x86 and the GPU generate different default
    NaNs; tests/test_gpu_lsolver.py draws the same line);
  * the same ctx with the switch off: every bit, NaNs included.
Shapes are the smallest at which each code path exists: one super-panel (64), a two-column partial block (66), two column blocks
(128, 130), a third (192), the flagship's eight row slots with the slot count folded (512), and partial first super-panels (9, 63).
"""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

U64 = np.uint64


def bits(a):
    return np.ascontiguousarray(a).view(U64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def same_as_oracle(got, want):
    """bit for bit where the oracle has numbers, NaN where it has NaN"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(want[~nan]))


def rand_ab(n, batch, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    A = rng.standard_normal((batch, n, n))
    B = rng.standard_normal((batch, n, n)) + 3.0 * np.eye(n)
    return A, B


def ctx_of(A, B, on):
    import idahip
    batch, n = A.shape[0], A.shape[1]
    ctx = idahip.Ctx("linear_dense", n, batch)
    ctx.set_tolerances(1.0e-6, np.array([1.0e-8]))
    ctx.set_linear_dense(A, B, np.zeros((batch, n)))
    assert ctx.jac_in_lu() == (1 if n > 448 else 0)  # never set: the device rounds alone, and only at the size that was measured
    ctx.set_jac_in_lu(on)
    assert ctx.jac_in_lu() == (2 if on else 0)
    return ctx


def factor(ctx, cj, idx):
    """idahip_nls_lsetup of the listed systems -> info [len(idx)], factors [len(idx)][n][n] in column-major storage, pivots"""
    rc, info = ctx.nls_lsetup(0.0, cj, idx)
    lus, pivs = [], []
    for s in idx:
        lu, piv = ctx.download_lu(int(s))
        lus.append(lu.T.copy())  # (download_lu hands out the logical view: back to storage order, as the oracle's batch entry has it)
        pivs.append(piv)
    return info, np.array(lus), np.array(pivs)


def oracle(A, B, cj, idx):
    cj = np.broadcast_to(np.asarray(cj, dtype=np.float64), (len(idx),))
    with np.errstate(all="ignore"):
        J = np.ascontiguousarray(B[idx] + cj[:, None, None] * A[idx])  # multiply, then add
    info, piv = O.getrf_batch(J, nthreads=4)
    return info, J, piv


def check(A, B, cj, idx=None, expect_info=None):
    """switch on == oracle, switch on == switch off; -> info"""
    idx = np.arange(A.shape[0], dtype=np.int32) if idx is None else np.asarray(idx, dtype=np.int32)
    i_o, lu_o, piv_o = oracle(A, B, cj, idx)
    i_on, lu_on, piv_on = factor(ctx_of(A, B, True), cj, idx)
    i_off, lu_off, piv_off = factor(ctx_of(A, B, False), cj, idx)
    assert np.array_equal(i_on, i_o) and np.array_equal(i_off, i_o), (i_on, i_off, i_o)
    if expect_info is not None:
        assert np.array_equal(i_o, expect_info), i_o
    ok = i_o == 0  # (a matrix with a zero pivot: the verdict is the result, the factors are left as they were)
    assert np.array_equal(piv_on[ok], piv_o[ok])
    assert same_as_oracle(lu_on[ok], lu_o[ok])
    assert np.array_equal(piv_on[ok], piv_off[ok]) and same_bits(lu_on[ok], lu_off[ok])
    return i_o


# ---------------------------------------------------------------------------------------------------------------- sizes and lists
@pytest.mark.parametrize("n", [64, 66, 128, 130, 192, 512, 9, 63])
def test_sizes(n):
    batch = 3 if n == 512 else 5
    A, B = rand_ab(n, batch, 100 + n)
    cj = np.linspace(0.5, 120.0, batch)  # a cj per list entry
    assert (check(A, B, cj) == 0).all()


@pytest.mark.parametrize("batch", [1, 9, 17])
def test_lists_shorter_than_the_batch(batch):
    """Lists that are not the whole batch, in an order of their own: launches padded to multiples of eight matrices, workgroups
    without a matrix, cj by list position."""
    n = 130
    A, B = rand_ab(n, batch, 7 * batch)
    rng = np.random.Generator(np.random.PCG64(batch))
    idx = rng.permutation(batch)[: max(1, (2 * batch) // 3)].astype(np.int32)
    cj = 1.0 + np.arange(idx.size, dtype=np.float64)
    assert (check(A, B, cj, idx) == 0).all()


# ---------------------------------------------------------------------------------------------------------------- hand-overs at k0 = 0
def first_pivot_rows(A, B, cj, s):
    """the rows of system s that become the first super-panel's pivot rows (from the oracle's pivots of the unmodified matrix)"""
    n = A.shape[1]
    _, _, piv = oracle(A, B, cj, np.array([s]))
    rows = np.arange(n)
    for k in range(min(64, n)):
        p = int(piv[0, k])
        rows[[k, p]] = rows[[p, k]]
    return rows[: min(64, n)]


@pytest.mark.parametrize("n", [66, 130, 192])
def test_zeros_among_the_pivot_rows_force_the_slow_paths(n):
    """An exact zero among a pivot row's entries right of the first super-panel (the trailing prologue's per-entry fallback), a pivot
    row that is zero across a whole column block, and an exact zero inside the first super-panel (the panel's FAST -> SLOW
    hand-over): J's entry is made zero by B = -cj*A there, so only the combination shows it."""
    cj = 2.0  # (a power of two: cj*a is exact, b = -cj*a gives +0.0)
    A, B = rand_ab(n, 4, 300 + n)
    pr = first_pivot_rows(A, B, cj, 0)
    # storage is column-major: X[s, j, i] = X_s(i, j)
    B[0, 64 + (n - 64) // 2, pr[5]] = -cj * A[0, 64 + (n - 64) // 2, pr[5]]        # one zero in U12's source
    pr1 = first_pivot_rows(A, B, cj, 1)
    B[1, 64:, pr1[9]] = -cj * A[1, 64:, pr1[9]]                                      # a pivot row that is zero right of the super-panel
    pr2 = first_pivot_rows(A, B, cj, 2)
    B[2, 20, pr2[3]] = -cj * A[2, 20, pr2[3]]                                        # a zero U entry inside the super-panel (block 2, pivot 3)
    B[3, 64:, :] = -cj * A[3, 64:, :]                                                # everything right of the super-panel is zero
    info = check(A, B, cj)
    assert (info[:3] == 0).all()  # (system 3: a zero pivot at column 65 is the reference's verdict, and must be ours)


def test_a_column_block_whose_pivot_rows_are_all_zero_still_reaches_the_work_matrix():
    """The plain trailing kernel leaves a column block early when its 64 pivot rows are zero across the block (nothing to subtract);
    the J-forming one must go on and store the tile it formed, or the rows below never reach the work matrix. Here the first
    super-panel's pivot rows are zero in columns 128..191 and the rows below are not: info is 0 and the factors are compared."""
    n, cj = 192, 2.0
    A, B = rand_ab(n, 3, 1234)
    for s in (0, 2):
        pr = first_pivot_rows(A, B, cj, s)  # (they depend on columns 0..63 alone: changing columns >= 128 leaves them the pivot rows)
        B[s, 128:, pr] = -cj * A[s, 128:, pr]
    pr = first_pivot_rows(A, B, cj, 1)
    B[1, 64:128, pr] = -cj * A[1, 64:128, pr]  # the same in the first column block, whose rows below feed the second super-panel
    assert np.array_equal(first_pivot_rows(A, B, cj, 1), pr)
    info = check(A, B, cj)
    assert (info == 0).all(), info


def test_ties_in_absolute_value():
    n = 130
    A, B = rand_ab(n, 3, 41)
    A[:] = np.sign(A)          # every entry of J is +-1 +- cj: ties in |a| in every column
    B[:] = np.sign(B)
    check(A, B, 2.0)
    A2, B2 = rand_ab(n, 2, 42)
    B2[0, 0, :] = 3.0; A2[0, 0, :] = 1.0       # column 0 constant: the first pivot is a tie of all rows
    B2[1, :70, 7] = -B2[1, :70, 11]; A2[1, :70, 7] = -A2[1, :70, 11]  # two rows of opposite sign across the first super-panel
    assert (check(A2, B2, 0.75) == 0).all()


@pytest.mark.parametrize("n", [64, 130])
def test_nan_and_infinity(n):
    """A NaN and an infinity in A, in B, and produced only by cj*a (overflow), inside the first super-panel and right of it."""
    A, B = rand_ab(n, 7, 500 + n)
    c2 = n - 3  # a column right of the first super-panel where there is one
    A[0, 5, 5] = np.nan
    B[1, 9, n - 2] = np.nan
    A[2, 3, 17] = np.inf
    B[3, c2, 20] = -np.inf
    A[4, c2, 33] = np.nan
    B[5, 2, 2] = np.inf
    A[6, 11, 40] = 1.0e300; A[6, c2, 41] = -1.0e300  # cj*a overflows
    check(A, B, 1.0e10)


@pytest.mark.parametrize("n", [64, 130])
def test_zero_pivot_inside_the_first_super_panel(n):
    """info is the reference's 1-based column and the later launches leave the system alone; its neighbours are factored."""
    cj = 4.0
    A, B = rand_ab(n, 4, 600 + n)
    B[1, 10, :] = -cj * A[1, 10, :]                      # column 10 of J is zero: zero pivot at step 11
    B[2, 0, :] = -cj * A[2, 0, :]                        # column 0
    B[3, 63, :] = -cj * A[3, 63, :]                      # the super-panel's last column
    info = check(A, B, cj)
    assert info[0] == 0 and info[1] == 11 and info[2] == 1 and info[3] == 64, info


def test_signed_zeros():
    """b = -0.0 with cj*a = +0.0 gives +0.0, b = -0.0 with cj*a = -0.0 gives -0.0, b = +0.0 with cj*a = -0.0 gives +0.0: the factors
    keep the signs the reference's add gives them."""
    n = 130
    A, B = rand_ab(n, 3, 77)
    for s, (b0, a0) in enumerate([(-0.0, 0.0), (-0.0, -0.0), (0.0, -0.0)]):
        B[s, 100, :] = np.where(np.arange(n) % 3 == 0, b0, B[s, 100, :]); A[s, 100, :] = np.where(np.arange(n) % 3 == 0, a0, A[s, 100, :])
        B[s, 70:, 5] = b0; A[s, 70:, 5] = a0       # a row of signed zeros right of the super-panel
        B[s, 30, 1::2] = b0; A[s, 30, 1::2] = a0   # and half a column inside it
    check(A, B, 3.0)
    check(A, B, -3.0)


@pytest.mark.parametrize("cj", [0.0, -0.0, -17.5, 1.0e-300, 1.0e300])
def test_extreme_cj(cj):
    n = 66
    A, B = rand_ab(n, 2, 900)
    check(A, B, cj)


# ---------------------------------------------------------------------------------------------------------------- the entry points
@pytest.mark.parametrize("n", [64, 130])
def test_sys_setup_entry_leaves_the_same_residual_and_factors(n):
    """idahip_nls_sys_setup (the host stepper's call): delta and savres of the plain sweep are those of the fused sweep."""
    import idahip
    from idahip import problems
    p = problems.linear_dense(n=n, batch=6, procs=1)
    out = []
    for on in (True, False):
        ctx = problems.make_ctx(p)
        ctx.set_jac_in_lu(on)
        ctx.upload(idahip.F_YY, p["yy0"]); ctx.upload(idahip.F_YP, p["yp0"])
        ctx.upload(idahip.F_YYPREDICT, p["yy0"]); ctx.upload(idahip.F_YPPREDICT, p["yp0"])
        ctx.timing(True)
        idx = np.array([4, 0, 3], dtype=np.int32)
        rc, info = ctx.nls_sys_setup(0.0, np.array([10.0, 20.0, 30.0]), True, idx)
        t = ctx.timing_get()
        out.append((info, ctx.download(idahip.F_DELTA), ctx.download(idahip.F_SAVRES), [ctx.download_lu(int(s)) for s in idx],
                    {k: t[k]["systems"] for k in ("sys", "sys_jac", "jac", "lu")}))
    (i1, d1, s1, f1, k1), (i0, d0, s0, f0, k0) = out
    assert (i1 == 0).all() and np.array_equal(i1, i0)
    assert same_bits(d1[[4, 0, 3]], d0[[4, 0, 3]]) and same_bits(s1[[4, 0, 3]], s0[[4, 0, 3]])
    for (lu1, p1), (lu0, p0) in zip(f1, f0):
        assert same_bits(lu1, lu0) and np.array_equal(p1, p0)
    assert k1 == {"sys": 3, "sys_jac": 0, "jac": 0, "lu": 3} and k0 == {"sys": 0, "sys_jac": 3, "jac": 0, "lu": 3}, (k1, k0)


# ---------------------------------------------------------------------------------------------------------------- full schedule
CNT = ("nst", "nre", "nni", "nsetups", "netf", "ncfn", "n_attempts", "kused", "kk", "nls_nconvfails")


def run_schedule(prob, device_ctl, on):
    import idahip
    from idahip import problems
    ctx = problems.make_ctx(prob)
    if on is not None:
        ctx.set_jac_in_lu(on)
    ctx.timing(True)
    ens = idahip.Ensemble(ctx, prob["yy0"], prob["yp0"])
    ens.set_device_controller(device_ctl)
    assert (ens.device_controller_active() != 0) == bool(device_ctl)
    for t in prob["touts"][:3]:
        status, tret = ens.solve(t)
        assert (status == 0).all()
    c = ens.counters()
    t = ctx.timing_get()
    return ({**{k: c[k] for k in CNT}, "yy": ens.yy(), "yp": ens.yp(), "tn": ens.real("tn"), "hused": ens.real("hused"), "hh": ens.real("hh")},
            {k: t[k]["systems"] for k in ("sys", "sys_jac", "jac", "lu", "newton_iter")})


@pytest.fixture(scope="module")
def ensembles():
    from idahip import problems
    return {n: problems.linear_dense(n=n, batch=24, procs=1) for n in (64, 130)}


@pytest.mark.parametrize("device_ctl", [1, 0], ids=["device_rounds", "host_stepper"])
@pytest.mark.parametrize("n", [64, 130])
def test_full_schedule_switch_on_equals_switch_off(ensembles, n, device_ctl):
    """24 systems over three output times on the device lock-step stepper (the LU list's length lives on the device and is shorter
    than the launches' bound in most rounds) and on the host stepper: states, step sizes and every counter bit for bit; the setups'
    residual sweeps move from class sys_jac to class sys and nothing else moves."""
    s1, k1 = run_schedule(ensembles[n], device_ctl, True)
    s0, k0 = run_schedule(ensembles[n], device_ctl, False)
    for k in s1:
        assert same_bits(s1[k], s0[k]) if s1[k].dtype == np.float64 else np.array_equal(s1[k], s0[k]), k
    assert k1["sys_jac"] == 0 and k0["sys_jac"] > 0
    assert k1["sys"] == k0["sys"] + k0["sys_jac"]
    assert k1["lu"] == k0["lu"] == k0["sys_jac"] and k1["jac"] == k0["jac"] == 0 and k1["newton_iter"] == k0["newton_iter"]


def test_a_ctx_left_alone(ensembles):
    """Never set: the device lock-step stepper takes the path where the first panel is the eight-slot instantiation (n > 448, the
    size that was measured) and nowhere else; idahip_nls_sys_setup -- and with it the host stepper -- launches the kernel classes
    it always launched at every size."""
    from idahip import problems
    big = problems.linear_dense(n=512, batch=4, procs=1)
    sd, kd = run_schedule(big, 1, None)
    s1, k1 = run_schedule(big, 1, True)
    s0, k0 = run_schedule(big, 1, False)
    assert kd == k1 and kd["sys_jac"] == 0 and k0["sys_jac"] > 0
    sh, kh = run_schedule(big, 0, None)
    assert kh["sys_jac"] > 0 and kh["sys_jac"] == kh["lu"]
    for k in sd:
        assert np.array_equal(sd[k], s1[k]) and np.array_equal(sd[k], s0[k]) and np.array_equal(sd[k], sh[k]), k
    for device_ctl in (1, 0):  # a small matrix: both steppers on the old path until told otherwise
        sn, kn = run_schedule(ensembles[64], device_ctl, None)
        sf, kf = run_schedule(ensembles[64], device_ctl, False)
        assert kn == kf and kn["sys_jac"] > 0
        for k in sn:
            assert np.array_equal(sn[k], sf[k]), k


@pytest.mark.parametrize("batch", [1, 9, 17])
def test_device_rounds_at_small_batches(batch):
    """The device-built list (its length on the device, the launches sized for the whole batch and padded to eight) at batches of
    1, 9 and 17."""
    from idahip import problems
    prob = problems.linear_dense(n=130, batch=batch, procs=1)
    s1, k1 = run_schedule(prob, 1, True)
    s0, k0 = run_schedule(prob, 1, False)
    for k in s1:
        assert same_bits(s1[k], s0[k]) if s1[k].dtype == np.float64 else np.array_equal(s1[k], s0[k]), k
    assert k1["sys_jac"] == 0 and k1["sys"] == k0["sys"] + k0["sys_jac"]


# ---------------------------------------------------------------------------------------------------------------- refusals and fallbacks
def test_refusals_and_fallbacks():
    import idahip
    from idahip import problems
    # n = 513: not eligible -- off, turning it on is refused, turning it off is accepted, and the old path factors J
    A, B = rand_ab(513, 2, 5)
    ctx = idahip.Ctx("linear_dense", 513, 2)
    ctx.set_tolerances(1.0e-6, np.array([1.0e-8]))
    ctx.set_linear_dense(A, B, np.zeros((2, 513)))
    assert not ctx.jac_in_lu()
    assert ctx.H.idahip_set_jac_in_lu(ctx.h, 1) == -2 and ctx.H.idahip_set_jac_in_lu(ctx.h, 0) == 0 and not ctx.jac_in_lu()
    idx = np.arange(2, dtype=np.int32)
    i_o, lu_o, piv_o = oracle(A, B, 5.0, idx)
    i_g, lu_g, piv_g = factor(ctx, 5.0, idx)
    assert (i_g == 0).all() and np.array_equal(piv_g, piv_o) and same_bits(lu_g, lu_o)
    # a DQ ctx keeps the setting and uses the other path while DQ lasts
    p = problems.linear_dense(n=64, batch=2, procs=1)
    dq = problems.make_ctx(p)
    assert dq.jac_in_lu() == 0  # (n <= 448 and never set)
    dq.set_jac_in_lu(True)
    assert dq.jac_in_lu() == 2
    dq.set_jacobian_dq(True)
    assert dq.jac_in_lu() == 0
    dq.set_jacobian_dq(False)
    assert dq.jac_in_lu() == 2
    # LU variant 3 likewise
    dq.set_lu_variant(3)
    assert dq.jac_in_lu() == 0
    i3, lu3, piv3 = factor(dq, 7.0, idx)
    dq.set_lu_variant(4)
    assert dq.jac_in_lu() == 2
    i4, lu4, piv4 = factor(dq, 7.0, idx)
    assert (i3 == 0).all() and np.array_equal(i3, i4) and np.array_equal(piv3, piv4) and same_bits(lu3, lu4)
    # a heat ctx: another kind
    hc = problems.make_ctx(problems.heat1d(n=64, batch=2))
    assert not hc.jac_in_lu() and hc.H.idahip_set_jac_in_lu(hc.h, 1) == -2 and hc.H.idahip_set_jac_in_lu(hc.h, 0) == 0
    assert ctx.H.idahip_set_jac_in_lu(None, 1) == -1 and ctx.H.idahip_jac_in_lu(None) == -1
