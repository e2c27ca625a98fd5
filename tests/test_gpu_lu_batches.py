"""The batched LU (idahip_ls_setup / idahip_ls_solve, idahip_nls_lsetup + idahip_newton_iter) at production launch sizes, with
special values inside large launches, under every list shape, and through sequences of setups on one ctx -- against the CPU
oracle run matrix by matrix (oracle_dense_getrf_batch). Every assertion is exact: info, pivots, factors and solutions bit for
bit where the oracle has a number, NaN where it has NaN (the payload of a NaN is not part of the contract)."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

SENT = 0x7ff80000deadbeef  # a NaN pattern no kernel produces: what is off the list must come back with exactly these bits
CHUNK = 32                 # systems compared per device step


def colmajor(mats):
    return np.ascontiguousarray(np.transpose(mats, (0, 2, 1)))


@pytest.fixture(params=[3, 4], ids=["lu-panel2", "lu-wavepanel"])
def lu_variant(request):
    """n <= 1024: the panel kernels with two rows per lane, or one wave per matrix and super-panel (the default)."""
    return request.param


@pytest.fixture(params=[1, 0], ids=["superpanel", "panel-by-panel"])
def large_n_pipeline(request):
    """n > 1024: a 64-column super-panel as one launch, or as eight 8-column panel launches with a narrow update after each."""
    return request.param


_DEV = {}  # device copies of the generated batches and their oracle results, shared by a test's pipelines


@pytest.fixture(scope="module", autouse=True)
def _release_device_batches():
    yield
    _DEV.clear()
    import torch
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ matrix families
FAMILIES = ("dense", "zeros", "banded", "ties", "nan", "inf", "singular")


def zero_column(n):
    """A column in the last super-panel (in the middle of the one panel when n <= 64): the trailing kernels have updated the
    matrix before the factorisation meets the zero pivot."""
    return ((n - 1) // 64) * 64 + ((n - 1) % 64) // 2


def family_matrix(rng, fam, n):
    if fam == "dense":
        return rng.standard_normal((n, n))
    if fam == "zeros":  # most entries exact zeros: the wave-per-matrix kernel's FAST mode hands the matrix to its SLOW launch
        m = rng.standard_normal((n, n))
        m[np.abs(m) < 0.9] = 0.0
        return m + np.diag(np.full(n, 4.0))
    if fam == "banded":  # a band of 7 with a weak diagonal: the pivots swap rows and widen U
        m = np.zeros((n, n))
        for d in range(-3, 4):
            k = np.arange(max(0, -d), min(n, n - d))
            m[k, k + d] = rng.standard_normal(k.size) * (0.3 if d == 0 else 1.0)
        return m
    if fam == "ties":  # small integers: exact ties in |a| between rows, zeros everywhere
        return rng.integers(-3, 4, size=(n, n)).astype(float) + np.eye(n) * 2.0
    if fam == "nan":  # NaN at a diagonal position (kept if the scan reaches it there) and one below the diagonal (never chosen)
        m = rng.standard_normal((n, n))
        p = int(rng.integers(0, n))
        m[p, p] = np.nan
        c = int(rng.integers(0, n - 1))
        m[int(rng.integers(c + 1, n)), c] = np.nan
        return m
    if fam == "inf":  # two infinities in one column (the first in scan order wins), one more elsewhere
        m = rng.standard_normal((n, n))
        c = int(rng.integers(0, n))
        r = rng.choice(n, size=2, replace=False)
        m[r[0], c], m[r[1], c] = np.inf, -np.inf
        m[int(rng.integers(0, n)), int(rng.integers(0, n))] = -np.inf
        return m
    if fam == "singular":
        m = rng.standard_normal((n, n))
        m[:, zero_column(n)] = 0.0
        return m
    raise ValueError(fam)


def tridiagonal(rng, n):
    m = np.zeros((n, n))
    i = np.arange(n)
    m[i, i] = 4.0 + rng.random(n)
    m[i[1:], i[:-1]] = -1.0 - rng.random(n - 1)
    m[i[:-1], i[1:]] = -1.0 - rng.random(n - 1)
    return m


def large_family_matrix(rng, fam, n):
    """The families of test_banded_and_partly_banded_matrices_beyond_1024_rows, and dense and singular matrices."""
    if fam == "tri":
        return tridiagonal(rng, n)
    if fam == "band7":
        return family_matrix(rng, "banded", n)
    if fam == "band-then-dense":  # banded where the band is measured (first super-panel), dense behind it
        m = tridiagonal(rng, n)
        m[64:, 64:] = rng.standard_normal((n - 64, n - 64))
        return m
    if fam == "dense-rows":  # dense leading rows: every column block has work
        m = tridiagonal(rng, n)
        m[:40, :] = rng.standard_normal((40, n))
        return m
    if fam == "dense":
        return rng.standard_normal((n, n))
    if fam == "singular":  # dense, zero column far right: every trailing kernel has run on it before the zero pivot
        m = rng.standard_normal((n, n))
        m[:, 700] = 0.0
        return m
    if fam == "singular-tri":
        m = tridiagonal(rng, n)
        m[:, 130] = 0.0
        return m
    raise ValueError(fam)


# ------------------------------------------------------------------------------------------------ device batches
class DevBatch:
    """A batch of matrices on the device next to the oracle's info, pivots, factors (column-major) and solutions."""

    def __init__(self, mats_cm, rng):
        import torch
        B, n, _ = mats_cm.shape
        self.B, self.n = B, n
        rhs = rng.standard_normal((B, n))
        self.orig = torch.from_numpy(mats_cm).cuda()
        lu = mats_cm  # factored in place: the caller's array is the oracle's from here on
        self.info, piv = O.getrf_batch(lu)
        x = O.getrs_batch(lu, piv, rhs)
        self.lu = torch.from_numpy(lu).cuda()
        self.piv = torch.from_numpy(piv).cuda()
        self.rhs = torch.from_numpy(rhs).cuda()
        self.x = torch.from_numpy(x).cuda()


def same_bits(got, want):
    """Per leading index: every entry has the oracle's bits, or is NaN where the oracle's is NaN."""
    import torch
    ok = torch.where(torch.isnan(want), torch.isnan(got), got.view(torch.int64) == want.view(torch.int64))
    return ok.reshape(ok.shape[0], -1).all(dim=1).cpu().numpy()


def untouched(got, orig):
    import torch
    return bool(torch.equal(got.view(torch.int64), orig.view(torch.int64)))


def check_launch(ctx, db, idx, tag):
    """ls_setup of the listed systems of `db` on a fresh copy of the batch, pivots preset to SENT, then ls_solve of the listed
    systems the oracle factors: everything against the oracle, everything off the list untouched."""
    import torch
    idx = np.asarray(idx, dtype=np.int32)
    dA = db.orig.clone()
    dP = torch.full((db.B, db.n), SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc, info = ctx.ls_setup(dA.data_ptr(), dP.data_ptr(), idx)
    want = db.info[idx]
    assert np.array_equal(info, want), (tag, np.nonzero(info != want)[0][:8])
    assert rc == (1 if want.any() else 0), tag
    ok = idx[want == 0]
    for q in range(0, ok.size, CHUNK):
        t = torch.from_numpy(ok[q:q + CHUNK].astype(np.int64)).cuda()
        good = same_bits(dA[t], db.lu[t])
        assert good.all(), (tag, "factors", ok[q:q + CHUNK][~good])
        assert torch.equal(dP[t], db.piv[t]), (tag, "pivots")
    off = np.setdiff1d(np.arange(db.B), idx)
    if off.size:
        for q in range(0, off.size, CHUNK):
            t = torch.from_numpy(off[q:q + CHUNK].astype(np.int64)).cuda()
            assert untouched(dA[t], db.orig[t]), (tag, "matrix off the list")
        assert bool((dP[torch.from_numpy(off.astype(np.int64)).cuda()] == SENT).all()), (tag, "pivots off the list")
    if ok.size:
        dX = torch.full((db.B, db.n), SENT, dtype=torch.int64, device="cuda").view(torch.float64)
        torch.cuda.synchronize()
        ctx.ls_solve(dA.data_ptr(), dP.data_ptr(), dX.data_ptr(), db.rhs.data_ptr(), ok)
        t = torch.from_numpy(ok.astype(np.int64)).cuda()
        good = same_bits(dX[t], db.x[t])
        assert good.all(), (tag, "solutions", ok[~good])
    del dA, dP


def family_of_position(p, perm):
    """Family at list position p: position 8q + r gets perm[(2q + r) % 7] -- the first seven positions hold every family, and
    each family meets every residue mod 8 (every XCD lane of the trailing kernels' dealing) within the first 56 positions."""
    return FAMILIES[perm[(2 * (p // 8) + p % 8) % 7]]


NSYS_SMALL = (1, 7, 9, 17, 65, 300)


def small_batch(n, B):
    key = ("small", n, B)
    if key not in _DEV:
        rng = np.random.default_rng(4000 + n)
        perm = rng.permutation(7)
        mats = np.empty((B, n, n))
        for p in range(B):
            mats[p] = family_matrix(rng, family_of_position(p, perm), n).T  # column-major in place
        _DEV[key] = DevBatch(mats, rng)
    return _DEV[key]


@pytest.mark.parametrize("n", [9, 64, 65, 200, 512, 513, 1000, 1024])
def test_batch_sizes_with_special_values_up_to_1024_rows(n, lu_variant):
    """Lists of 1 to 300 systems (the trailing kernels deal matrices to the 8 XCDs by list position on a grid padded to a multiple
    of 8), every launch mixing dense matrices, matrices of exact zeros, bands, ties, NaN, infinities and a singular matrix whose
    zero column lies in the last super-panel."""
    import idahip
    db = small_batch(n, max(NSYS_SMALL))
    ctx = idahip.Ctx("linear_dense", n, db.B)
    ctx.set_lu_variant(lu_variant)
    for nsys in NSYS_SMALL:
        check_launch(ctx, db, np.arange(nsys), (n, nsys))
    ctx.close()


def test_benchmark_batch_size_at_512_rows(lu_variant):
    """n = 512 at the benchmark's 1374 matrices per call, families as above."""
    import idahip
    db = small_batch(512, 1374)
    ctx = idahip.Ctx("linear_dense", 512, db.B)
    ctx.set_lu_variant(lu_variant)
    check_launch(ctx, db, np.arange(db.B), (512, db.B))
    ctx.close()


# ------------------------------------------------------------------------------------------------ n > 1024
NSYS_HELPERS = (9, 64, 65, 128, 129, 256, 257)  # the host halves the row-split helpers while nsys * nsplit > 512


def large_batch(n, B, seed, dense_only=False):
    key = ("large", n, B, dense_only)
    if key not in _DEV:
        for k in [k for k in _DEV if _DEV[k].orig.numel() > (1 << 27)]:  # one batch of more than 1 GB at a time
            del _DEV[k]
        rng = np.random.default_rng(seed)
        fams = []
        for p in range(B):
            fams.append("dense" if dense_only else "band7" if p % 5 == 4 else "dense-rows" if p % 23 == 11 else "tri")
        if not dense_only:
            for p in (2, 5, 6, 8, 77, 140, 203, 256):      # at least four dense matrices in every launch of a prefix list
                if p < B:
                    fams[p] = "dense"
            for p in (1, 70, 190):
                if p < B:
                    fams[p] = "band-then-dense"
            for p, f in ((3, "singular"), (64, "singular-tri"), (129, "singular-tri"), (255, "singular")):
                if p < B:
                    fams[p] = f
        else:
            fams[3] = "singular"
        mats = np.empty((B, n, n))
        for p in range(B):
            mats[p] = large_family_matrix(rng, fams[p], n).T
        _DEV[key] = DevBatch(mats, rng)
        del mats
    return _DEV[key]


def test_helper_thresholds_beyond_1024_rows(large_n_pipeline):
    """n = 1100, lists of 9 to 257 systems across the helper thresholds (65, 129, 257): mostly tridiagonal and banded matrices (the
    helpers engage), dense ones and singular ones at scattered positions in every launch."""
    import idahip
    db = large_batch(1100, max(NSYS_HELPERS), 1100)
    ctx = idahip.Ctx("linear_dense", 1100, db.B)
    ctx.set_lu_superpanel(large_n_pipeline)
    for nsys in NSYS_HELPERS:
        check_launch(ctx, db, np.arange(nsys), (1100, nsys))
    ctx.close()


@pytest.mark.parametrize("n,dense_only", [(1100, True), (2120, False)], ids=["1100-dense", "2120-mixed"])
def test_seventeen_systems_beyond_1024_rows(n, dense_only, large_n_pipeline):
    """17 systems (three slot groups, the last one with a single matrix): dense matrices only at n = 1100, the mixed families at
    n = 2120."""
    import idahip
    db = large_batch(n, 17, n + 17, dense_only)
    ctx = idahip.Ctx("linear_dense", n, db.B)
    ctx.set_lu_superpanel(large_n_pipeline)
    check_launch(ctx, db, np.arange(17), (n, 17))
    ctx.close()


# ------------------------------------------------------------------------------------------------ list shapes
def list_shapes(B, rng):
    sub = rng.permutation(B)[: B // 2 + 1]
    return {"reversed": np.arange(B)[::-1].copy(), "permuted-subset": sub, "stride-3": np.arange(1, B, 3), "single": np.array([B - 2])}


def check_list_shapes(ctx, n, B, seed):
    """Systems off the list hold the SENT pattern (matrix, pivot row, solution row) and keep its bits; a listed system's bits do
    not depend on the list's order or length: the same as in the call with the full ascending list, itself equal to the oracle."""
    import torch
    rng = np.random.default_rng(seed)
    perm = rng.permutation(7)
    mats = np.empty((B, n, n))
    for p in range(B):
        mats[p] = family_matrix(rng, family_of_position(p, perm), n).T
    db = DevBatch(mats, rng)
    del mats
    check_launch(ctx, db, np.arange(B), "full")
    full_A = db.orig.clone()
    full_P = torch.full((B, n), SENT, dtype=torch.int64, device="cuda")  # a failed system's pivots past its zero column stay unwritten
    torch.cuda.synchronize()
    _, full_info = ctx.ls_setup(full_A.data_ptr(), full_P.data_ptr(), np.arange(B))
    full_ok = np.nonzero(full_info == 0)[0].astype(np.int32)
    full_X = torch.zeros((B, n), dtype=torch.float64, device="cuda")
    ctx.ls_solve(full_A.data_ptr(), full_P.data_ptr(), full_X.data_ptr(), db.rhs.data_ptr(), full_ok)
    sent = torch.full((n, n), SENT, dtype=torch.int64, device="cuda")
    for name, idx in list_shapes(B, rng).items():
        idx = idx.astype(np.int32)
        off = torch.from_numpy(np.setdiff1d(np.arange(B), idx).astype(np.int64)).cuda()
        on = torch.from_numpy(idx.astype(np.int64)).cuda()
        dA = db.orig.clone()
        dA.view(torch.int64)[off] = sent
        dP = torch.full((B, n), SENT, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        rc, info = ctx.ls_setup(dA.data_ptr(), dP.data_ptr(), idx)
        assert np.array_equal(info, full_info[idx]), name
        assert bool((dA.view(torch.int64)[off] == SENT).all()) and bool((dP[off] == SENT).all()), name
        assert torch.equal(dA.view(torch.int64)[on], full_A.view(torch.int64)[on]), name   # failed systems too: the same partial factors
        assert torch.equal(dP[on], full_P[on]), name
        ok = idx[info == 0]
        dX = torch.full((B, n), SENT, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.ls_solve(dA.data_ptr(), dP.data_ptr(), dX.data_ptr(), db.rhs.data_ptr(), ok)
        t_ok = torch.from_numpy(ok.astype(np.int64)).cuda()
        rest = torch.from_numpy(np.setdiff1d(np.arange(B), ok).astype(np.int64)).cuda()
        assert torch.equal(dX[t_ok], full_X.view(torch.int64)[t_ok]), name
        assert bool((dX[rest] == SENT).all()), name
        del dA, dP, dX


@pytest.mark.parametrize("n", [96, 700])
def test_list_shapes_up_to_1024_rows(n, lu_variant):
    import idahip
    B = 21
    ctx = idahip.Ctx("linear_dense", n, B)
    ctx.set_lu_variant(lu_variant)
    check_list_shapes(ctx, n, B, 300 + n)
    ctx.close()


def test_list_shapes_beyond_1024_rows(large_n_pipeline):
    import idahip
    n, B = 1100, 11
    ctx = idahip.Ctx("linear_dense", n, B)
    ctx.set_lu_superpanel(large_n_pipeline)
    check_list_shapes(ctx, n, B, 1101)
    ctx.close()


# ------------------------------------------------------------------------------------------------ ctx state, n = 2048
def newton_matches_factors(ctx, rng, expect, tag):
    """newton_iter over every system whose last setup succeeded: the correction is O.getrs on the factors that setup left
    (right-hand sides with +0.0 and -0.0 stretches -- the solve leaves zero blocks of the factors out only where that is exact)."""
    import idahip
    n, B = ctx.n, ctx.batch
    idx = np.array(sorted(expect), dtype=np.int32)
    rhs = rng.standard_normal((B, n))
    rhs[:, 100:900] = 0.0
    rhs[::2, 1500:1700] = -0.0
    ctx.upload(idahip.F_DELTA, rhs)
    ctx.upload(idahip.F_EE, np.zeros((B, n)))
    ctx.upload(idahip.F_EWT, np.ones((B, n)))
    ctx.newton_iter(1.0, idx=idx)
    got = ctx.download(idahip.F_DELTA)
    for s in idx:
        lu, piv = expect[s]
        want = O.getrs(lu, piv, -rhs[s])
        assert np.array_equal(got[s].view(np.uint64), want.view(np.uint64)), (tag, s)


def check_setup(ctx, J, idx, info, expect, tag):
    """Listed systems against the oracle (pivots, factors with the signs of their zeros); unlisted systems still hold the factors of
    their last successful setup. `expect` (system -> factors) is updated."""
    cms = colmajor(J[idx])
    info_o, piv_o = O.getrf_batch(cms)
    assert np.array_equal(info, info_o), (tag, info, info_o)
    for q, s in enumerate(idx):
        if info_o[q] != 0:
            expect.pop(s, None)
            continue
        expect[s] = (cms[q].T.copy(), piv_o[q])
    for s, (lu_o, p_o) in expect.items():
        lu, piv = ctx.download_lu(s)
        assert np.array_equal(piv, p_o), (tag, s)
        assert np.array_equal(lu.view(np.uint64), lu_o.view(np.uint64)), (tag, s)  # bits: the signs of zeros included


def permuted_band(rng, n):
    p = (rng.permutation(n // 64)[:, None] * 64 + np.arange(64)[None, :]).ravel()
    return tridiagonal(rng, n)[p]


def test_setup_sequences_on_one_ctx_at_2048_rows(large_n_pipeline):
    """One ctx, twelve systems, J = B + cj A by nls_lsetup: (1) an unordered subset with row-permuted bands, (2) all systems, two of
    them singular with a zero column at 130 and at 1100 (their scatter is skipped after the trailing kernels have written U rows),
    (3) a subset with the two failed systems, tridiagonal, then (4) dense. After each step: the listed systems against the oracle,
    the others unchanged, and a Newton iteration over every system with factors through the zero-block map."""
    import idahip
    n, B = 2048, 12
    rng = np.random.default_rng(2048 + large_n_pipeline)
    ctx = idahip.Ctx("linear_dense", n, B)
    ctx.set_lu_superpanel(large_n_pipeline)
    ctx.set_tolerances(1e-6, 1e-8)
    ctx.upload(idahip.F_YY, np.zeros((B, n)))
    ctx.upload(idahip.F_YP, np.zeros((B, n)))
    A = np.array([np.eye(n) * 0.5 for _ in range(B)])
    A[:, 7, 7] = -0.0                 # -0.0 in A and B: J(7, 7) = -0.0 + cj * -0.0 = -0.0 (the pivot of column 7 comes from below)
    Bm = np.array([tridiagonal(rng, n) for _ in range(B)])
    Bm[:, 7, 7] = -0.0
    Bm[:, 7, 6] = -0.0                # -0.0 in B alone: J(7, 6) = -0.0 + cj * 0.0 = +0.0
    cj = 2.5
    expect = {}
    sing = (4, 9)

    def setup(Bm, A, idx, tag):
        ctx.set_linear_dense(colmajor(A), colmajor(Bm), np.zeros((B, n)))
        rc, info = ctx.nls_lsetup(0.0, cj, idx=idx)
        assert rc == (1 if info.any() else 0), tag
        check_setup(ctx, Bm + cj * A, np.asarray(idx), info, expect, tag)
        newton_matches_factors(ctx, rng, expect, tag)

    # (1) an unordered subset, row-permuted bands (multipliers far from the diagonal)
    sub1 = [10, 3, 7, 0, 5]
    for s in sub1:
        Bm[s] = permuted_band(rng, n)
    setup(Bm, A, sub1, "subset")
    # (2) every system: new bands, two singular with zero columns at 130 and 1100 (A's diagonal entry there is zero too)
    Bm = np.array([tridiagonal(rng, n) if s % 3 else permuted_band(rng, n) for s in range(B)])
    A2 = A.copy()
    for s, zc in zip(sing, (130, 1100)):
        Bm[s, :, zc] = 0.0
        A2[s, zc, zc] = 0.0
    setup(Bm, A2, list(range(B)), "all")
    assert not any(s in expect for s in sing)
    # (3) a subset with the failed systems, tridiagonal, then (4) dense
    sub3 = [9, 1, 4, 11]
    for s in sub3:
        Bm[s] = tridiagonal(rng, n)
    setup(Bm, A, sub3, "after failure: tridiagonal")
    for s in sub3:
        Bm[s] = rng.standard_normal((n, n))
    setup(Bm, A, sub3, "after failure: dense")
    ctx.close()


def heat_jacobian(n, coef, cj):
    """Heat1D::jac (oracle/problems.hpp) as a logical matrix."""
    J = np.zeros((n, n))
    J[0, 0] = 1.0
    i = np.arange(1, n - 1)
    J[i, i - 1] = -coef
    J[i, i] = cj + 2.0 * coef
    J[i, i + 1] = -coef
    J[n - 1, n - 1] = 1.0
    return J


def test_heat_setups_switching_the_pipeline_on_one_ctx():
    """heat1d at n = 2048 with per-system coefficients: a setup where one system has coef = 0 and cj = 0 (column 1 all zeros: info =
    2, its scatter skipped), then ordinary setups with the super-panel pipeline switched 1 -> 0 -> 1 between them (the flag that the
    work matrix is all +0.0 must be dropped when the panel-by-panel pipeline leaves it otherwise): every setup exact."""
    import idahip
    n, B = 2048, 5
    ctx = idahip.Ctx("heat1d", n, B)
    ctx.set_lu_superpanel(1)
    ctx.upload(idahip.F_YY, np.zeros((B, n)))
    ctx.upload(idahip.F_YP, np.zeros((B, n)))
    expect = {}
    steps = [(1, [0.0, 3.0, 7.5, 0.25, 40.0], [0.0, 2.0, 5.0, 1.0, 0.5], list(range(B))),
             (0, [1.5, 3.0, 7.5, 0.25, 40.0], [3.0, 2.0, 5.0, 1.0, 0.5], [0, 3]),
             (1, [2.0, 1.0, 0.5, 9.0, 4.0], [1.0, 6.0, 0.75, 2.5, 8.0], [3, 0, 1]),
             (0, [2.0, 1.0, 0.5, 9.0, 4.0], [4.0, 3.0, 2.0, 1.0, 0.5], list(range(B))),
             (1, [0.5, 2.0, 4.0, 8.0, 16.0], [1.0, 1.0, 1.0, 1.0, 1.0], list(range(B)))]
    for step, (sp, coef, cj, idx) in enumerate(steps):
        ctx.set_lu_superpanel(sp)
        ctx.set_problem_params(np.array(coef)[:, None])
        cjl = np.array(cj)[idx]
        rc, info = ctx.nls_lsetup(0.0, cjl, idx=idx)
        J = np.array([heat_jacobian(n, coef[s], cj[s]) for s in range(B)])
        check_setup(ctx, J, np.asarray(idx), info, expect, step)
        if step == 0:
            assert info[0] == 2 and rc == 1 and 0 not in expect
    ctx.close()
