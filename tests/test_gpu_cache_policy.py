"""The kernels whose loads and stores carry a cache policy (csrc/exp_switches.hpp, NT_*: the non-temporal bit on data a launch touches
once -- A, B and J in linear_sys_kernel, the factors in the triangular solves, both sides of lu_finalize_kernel's scatter; the
fourth switch, the A22 strips and the U12 store of lu_trail64w_kernel, is off in the product build, so that variant runs in no
test here, only the kernel around it). A policy changes no arithmetic, so every result stays what the CPU oracle
computes, bit for bit -- at the sizes where those kernels take their partial paths (one full and one partial 64-column block, partial
16-row strips and 16-column groups, odd n: one row per lane and load) and, for the one place where such kernels run beside
each other, a group of ensembles streamed side by side against the same ensembles streamed alone. Being bit-identity tests they
pass with every switch on or off: that a switch reaches the instructions is read from the assembly (`make asm`: the `nt` bit on
the loads and stores named above), what it is worth from profiles/r07_cache_policy_ab.txt."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
CNT = ("nst", "nre", "nje", "nsetups", "nni", "netf", "ncfn", "n_attempts", "kused", "kk")


def colmajor(mats):
    """[B][n][n] logical -> contiguous column-major storage per system."""
    return np.ascontiguousarray(np.transpose(mats, (0, 2, 1)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("n,B", [(65, 3), (130, 3), (200, 5), (512, 3)])
def test_lu_and_solve_bit_for_bit(n, B):
    """Factors, pivots, info and the solution of one right-hand side, as tests/test_gpu_lsolver.py compares them. Matrix 1 has a
    column right of the first super-panel that is zero but for one entry: the pivot rows' entries in it are exact zeros and the
    trailing update of its column block takes the prologue that applies dense.rs:148 per entry. Matrix 2 has a zero column: a zero
    pivot, reported with its 1-based column, the others unaffected. Of that matrix `info` is all there is to compare: the pipeline
    stops at the zero pivot and scatters no factors for it (lu_finalize_kernel returns on info != 0), as
    tests/test_gpu_lsolver.py's singular case has it."""
    import idahip
    rng = np.random.default_rng(7000 + n)
    mats = rng.standard_normal((B, n, n))
    cz = 64 if n < 130 else 70
    mats[1, :, cz] = 0.0
    mats[1, cz, cz] = 2.0
    mats[1, :, 3] = 0.0
    mats[1, 3, 3] = 2.0
    mats[2, :, 10] = 0.0
    rhs = rng.standard_normal((B, n))
    out = [O.getrf(m) for m in mats]
    info_o, lu_o, piv_o = np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])
    assert info_o[2] == 11 and not info_o[[s for s in range(B) if s != 2]].any()
    ctx = idahip.Ctx("linear_dense", n, B)
    dA = ctx.dev_array(colmajor(mats))
    dP = ctx.dev_empty(8 * B * n)
    rc, info = ctx.ls_setup(dA, dP, None)
    lu = np.transpose(ctx.to_host(dA, (B, n, n)), (0, 2, 1))
    piv = ctx.to_host(dP, (B, n), dtype=np.int64)
    assert rc == 1 and np.array_equal(info, info_o)
    ok = [s for s in range(B) if info_o[s] == 0]
    for s in ok:
        assert np.array_equal(piv[s], piv_o[s]), s
        assert np.array_equal(bits(lu[s]), bits(lu_o[s])), s
    dB = ctx.dev_array(rhs)
    dX = ctx.dev_empty(rhs.nbytes)
    ctx.ls_solve(dA, dP, dX, dB, ok)
    x = ctx.to_host(dX, (B, n))
    for s in ok:
        assert np.array_equal(bits(x[s]), bits(O.getrs(lu_o[s], piv_o[s], rhs[s]))), s
    ctx.close()


@pytest.mark.parametrize("n", [65, 130])
def test_residual_and_fused_residual_jacobian_bit_for_bit(n):
    """F = A y' + B y - c from the residual kernel alone and from the fused residual + Jacobian kernel, cj not a power of two. J = B + cj A
    leaves the device only as its factors: systems 0 and 1 (dense) are compared as the LU of the oracle's J; system 2 has upper
    triangular A and B, so that no row is exchanged, every multiplier is a zero and the upper triangle of the factors IS J -- compared
    with the oracle's J entry by entry."""
    import idahip
    B, cj = 3, 0.3
    rng = np.random.default_rng(8000 + n)
    A = rng.standard_normal((B, n, n))
    Bm = rng.standard_normal((B, n, n))
    A[2], Bm[2] = np.triu(A[2]), np.triu(Bm[2])
    c = rng.standard_normal((B, n))
    yyp, ypp = rng.standard_normal((B, n)), rng.standard_normal((B, n))
    Ac, Bc = colmajor(A), colmajor(Bm)
    F_o = np.array([O.problem_res("linear_dense", n, yyp[s], ypp[s], A=Ac[s], B=Bc[s], c=c[s]) for s in range(B)])
    J_o = np.array([O.problem_jac("linear_dense", n, cj, yyp[s], ypp[s], A=Ac[s], B=Bc[s], c=c[s]) for s in range(B)])  # column-major
    ctx = idahip.Ctx("linear_dense", n, B)
    ctx.set_tolerances(1e-6, 1e-8)
    ctx.set_linear_dense(Ac, Bc, c)
    ctx.upload(idahip.F_YYPREDICT, yyp)
    ctx.upload(idahip.F_YPPREDICT, ypp)
    ctx.upload(idahip.F_EE, rng.standard_normal((B, n)))  # reset_ee: zeroed by the kernel, the point is the predictor
    ctx.nls_sys(0.0, cj, True)
    for f in (idahip.F_DELTA, idahip.F_SAVRES):
        assert np.array_equal(bits(ctx.download(f)), bits(F_o))
    ctx.upload(idahip.F_DELTA, np.zeros((B, n)))
    ctx.upload(idahip.F_SAVRES, np.zeros((B, n)))
    rc, info = ctx.nls_sys_setup(0.0, cj, True)
    assert rc == 0 and not info.any()
    for f in (idahip.F_DELTA, idahip.F_SAVRES):
        assert np.array_equal(bits(ctx.download(f)), bits(F_o))
    for s in range(B):
        lu, piv = ctx.download_lu(s)
        info_o, lu_o, piv_o = O.getrf(J_o[s].T)
        assert info_o == 0 and np.array_equal(piv, piv_o), s
        assert np.array_equal(bits(lu), bits(lu_o)), s
    lu, piv = ctx.download_lu(2)
    assert np.array_equal(piv, np.arange(n))
    iu = np.triu_indices(n)
    assert np.array_equal(bits(lu[iu]), bits(J_o[2].T[iu]))
    ctx.close()


def test_group_stream_equals_its_members_streamed_alone():
    """Two groups of 8 systems at n = 130, twelve rounds side by side (idaens_stream_group) and one group after the other: state,
    step sizes, orders and counters identical. The one place where kernels with the policies run beside each other."""
    import idahip
    from idahip import problems
    n, total = 130, 16
    prob = problems.linear_dense(n=n, batch=total, procs=1)
    parts = [{k: (v[lo:lo + 8] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == total else v) for k, v in prob.items()}
             for lo in (0, 8)]

    def make():
        ctxs = [problems.make_ctx(p) for p in parts]
        return ctxs, [idahip.Ensemble(c, p["yy0"], p["yp0"]) for c, p in zip(ctxs, parts)]
    ca, side = make()
    cb, alone = make()
    done = idahip.stream_group(side, prob["touts"], 12)
    for g, e in enumerate(alone):
        assert e.stream(prob["touts"], 12) == done[g]
    for a, b in zip(side, alone):
        assert a.total_rounds() == b.total_rounds() == 12 and a.total_newton_iters() == b.total_newton_iters() > 0
        c_a, c_b = a.counters(), b.counters()
        for k in CNT:
            assert np.array_equal(c_a[k], c_b[k]), k
        assert c_a["nsetups"].sum() > 0 and c_a["nst"].sum() > 0
        assert np.array_equal(bits(a.yy()), bits(b.yy())) and np.array_equal(bits(a.yp()), bits(b.yp()))
        for r in ("tn", "hused", "hh"):
            assert np.array_equal(bits(a.real(r)), bits(b.real(r))), r
    for e in side + alone:
        e.close()
    for c in ca + cb:
        c.close()
