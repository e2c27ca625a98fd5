"""The trailing update of the 64-column super-panel LU (lu_trail64w_kernel) at the smallest sizes that have one, through the entry
points of test_gpu_lsolver.py (idahip_ls_setup) and against the same oracle (dense_get_rf): info, pivots and factors bit for bit.

n = 65 .. 257 puts one to four super-panels in front of trailing blocks of every kind: a last column block of 1, 63, 64 or 8
columns, a last strip of 1 to 16 rows, one strip or several per wave, odd and even n. The kernel reads and writes the work
matrix through buffer descriptors whose range check stands in for the row and column guards, so the partial blocks and strips
are where a wrong descriptor would show: a value stored in the name of a lane that has no row or column, or a row read past
the live list. The contents are the ones on which the kernel changes its path: an exact zero among the pivot-row entries (the
prologue in registers hands over to the per-entry path), a block of pivot rows that is all zero, a -0.0 multiplier, NaN and
infinity in the trailing part, ties in the pivot column.

One batch of 8 matrices per (pipeline, n) holds all contents; it is factored once on the GPU and once by the oracle, and every
(n, content, pipeline) is a test of its own on that shared result."""
import numpy as np
import pytest

import oracle_lib as O
from test_gpu_ensemble import CNT, run_oracle

pytestmark = pytest.mark.gpu

SIZES = [65, 127, 128, 129, 192, 200, 257]
VARIANTS = [3, 4]
CONTENTS = ["random", "zero_in_pivot_row", "zero_pivot_row_block", "negative_zero_multiplier", "nan_and_infinity", "pivot_ties"]
BATCH = 8
SLOT = {"random": (0, 7), "zero_in_pivot_row": (1,), "zero_pivot_row_block": (2,), "negative_zero_multiplier": (3,),
        "nan_and_infinity": (4,), "pivot_ties": (5, 6)}


def colmajor(mats):
    return np.ascontiguousarray(np.transpose(mats, (0, 2, 1)))


def matrices(n):
    rng = np.random.default_rng(6400 + n)
    m = rng.standard_normal((BATCH, n, n))
    # 1: exact zeros in the first pivot row (the row with the largest |a| in column 0 receives no update before it is used), in
    # the first, a middle and the last trailing column: the zero test of the solve in registers fires in step 0
    p0 = int(np.argmax(np.abs(m[1, :, 0])))
    for c in {64, (64 + n) // 2, n - 1}:
        m[1, p0, c] = 0.0
    # 2: rows 0..63 are the pivot rows of the first super-panel (dominant diagonal) and are zero right of it: U12 = 0 for every
    # column block, nothing is subtracted, and the rows stay zero
    m[2, np.arange(64), np.arange(64)] += 100.0
    m[2, :64, 64:] = 0.0
    # 3: multipliers that are -0.0 (a -0.0 below a positive pivot, a +0.0 below a negative one), in rows whose trailing entries
    # include -0.0: -0.0 - u * -0.0 has the sign the reference gives only if the update is really made
    p0 = int(np.argmax(np.abs(m[3, :, 0])))
    rows = [r for r in (1, 7, n - 1, n - 2, 40) if r != p0]
    for r in rows:
        m[3, r, 0] = -0.0 if m[3, p0, 0] > 0 else 0.0
        m[3, r, 64:] = np.where(np.arange(n - 64) % 2 == 0, -0.0, m[3, r, 64:])
    # 4: NaN and both infinities in the trailing part: in the last row and column, in a pivot row of the first super-panel or not
    m[4, n - 1, 64] = np.nan
    m[4, 5, n - 1] = np.inf
    m[4, n // 2, (64 + n) // 2] = -np.inf
    # 5, 6: equal magnitudes in the pivot column -- small integers (ties and zeros in every column), and a random matrix with
    # a three-way tie of both signs in column 0 and in the first column of the second super-panel's range
    m[5] = rng.integers(-2, 3, size=(n, n)).astype(float) + 3.0 * np.eye(n)
    for c in (0, 64):
        m[6, [3, 9, n - 1], c] = [7.0, -7.0, 7.0]
    return m


_CACHE = {}


def factored(variant, n):
    """(oracle info, factors, pivots, GPU rc, info, factors, pivots) of the batch, computed once per (pipeline, n)."""
    key = (variant, n)
    if key not in _CACHE:
        import idahip
        m = matrices(n)
        if n not in _CACHE:
            out = [O.getrf(x) for x in m]
            _CACHE[n] = (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]))
        ctx = idahip.Ctx("linear_dense", n, BATCH)
        ctx.set_lu_variant(variant)
        dA = ctx.dev_array(colmajor(m))
        dP = ctx.dev_empty(8 * BATCH * n)
        rc, info = ctx.ls_setup(dA, dP, None)
        lu = np.transpose(ctx.to_host(dA, (BATCH, n, n)), (0, 2, 1))
        piv = ctx.to_host(dP, (BATCH, n), dtype=np.int64)
        ctx.close()
        _CACHE[key] = _CACHE[n] + (rc, info, lu, piv)
    return _CACHE[key]


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("variant", VARIANTS, ids=["lu-panel2", "lu-wavepanel"])
def test_trailing_update_matches_the_oracle(variant, n, content):
    info_o, lu_o, piv_o, rc, info, lu, piv = factored(variant, n)
    assert np.array_equal(info, info_o)
    for s in SLOT[content]:
        if info_o[s] != 0:  # (a zero pivot: the factors are unspecified from that column on; none of these matrices is singular)
            pytest.fail("matrix %d of n = %d is singular for the oracle: the case checks nothing" % (s, n))
        assert np.array_equal(piv[s], piv_o[s]), (s, np.flatnonzero(piv[s] != piv_o[s])[:4])
        if content == "nan_and_infinity":  # sign and payload of a NaN are not part of the contract (test_gpu_lsolver.py)
            assert np.isnan(lu_o[s]).any()
            assert np.array_equal(np.isnan(lu[s]), np.isnan(lu_o[s]))
            assert np.array_equal(lu[s], lu_o[s], equal_nan=True)
        else:
            bad = np.argwhere(lu[s].view(np.uint64) != lu_o[s].view(np.uint64))  # bits: a zero with the wrong sign counts
            assert bad.size == 0, (s, bad[:4].tolist())
    if content == "zero_pivot_row_block":
        assert not lu_o[2, :64, 64:].any()
    if content == "negative_zero_multiplier":
        assert (np.signbit(lu_o[3][:, 0]) & (lu_o[3][:, 0] == 0.0)).any()  # a -0.0 multiplier is in the oracle's factors


def test_list_length_on_the_device_with_fewer_systems_than_the_launch():
    """The device lock-step stepper hands the LU its list of systems with the list's length in device memory (d_cnt) and sizes
    the launches for the whole batch: in most rounds fewer systems than that need a factorisation, and the surplus workgroups of
    the trailing update leave on reading the count -- after they have read the (clamped) list entry next to it. n = 129: two
    super-panels, a one-column last block. Every factorisation feeds a Newton iteration, so the integration equals the oracle's
    bit for bit only if each of them did; the systems' setup counts differ, so lists shorter than the batch did occur."""
    import idahip
    from idahip import problems
    prob = problems.linear_dense(n=129, batch=BATCH, procs=1)
    ctx = problems.make_ctx(prob)
    ctx.set_lu_variant(4)  # (the device-side list length needs this pipeline)
    ens = idahip.Ensemble(ctx, prob["yy0"], prob["yp0"])
    ens.set_device_controller(1)
    assert ens.device_controller_active() != 0
    touts = prob["touts"][:2]
    for t in touts:
        status, _ = ens.solve(t)
        assert (status == 0).all()
    ref = run_oracle(prob, touts)
    c = ens.counters()
    for k in CNT:
        assert np.array_equal(c[k], ref["counters"][k]), k
    assert np.array_equal(ens.yy(), ref["yy"][-1]) and np.array_equal(ens.yp(), ref["yp"][-1])
    assert len(set(c["nsetups"].tolist())) > 1, c["nsetups"]
