"""The band LSolver pair (idahip_ls_setup_band / idahip_ls_solve_band) against the oracle's dense_get_rf / dense_get_rs on the same
matrices in dense storage: pivots and info identical, factors (expanded to the dense layout) and solutions equal by value
(-0.0 == +0.0: the band_kernels.hpp contract), for bands from diagonal to full, sizes from 1 to 8192 and batches up to 1024."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
GD = os.path.join(os.path.dirname(__file__), "golden")
BANDS = [(0, 0), (1, 1), (0, 3), (3, 0), (2, 5), (7, 3), (16, 16), "full"]
SIZES = [1, 2, 3, 17, 64, 511, 1025, 4096]


def make_ctx(n, batch):
    """A ctx to run the raw calls on: a band ctx where one may be made (it holds no n x n buffers), a dense one otherwise."""
    import idahip
    if 8 < n <= 4096:
        return idahip.Ctx("host_callback", n, batch, band=(0, 0))
    return idahip.Ctx("host_callback", n, batch)


def random_band(rng, B, n, ml, mu, ties=False):
    """[B][n][ldab] band storage: random entries in the band, the sub-diagonals larger (row swaps and upper fill), the fill rows
    garbage (the factorisation needs nothing in them). ties: small integers (equal magnitudes in pivot columns)."""
    import idahip
    ld, kv = idahip.band_ldab(ml, mu), ml + mu
    ab = rng.integers(-2, 3, (B, n, ld)).astype(np.float64) if ties else rng.standard_normal((B, n, ld))
    if not ties:
        ab[:, :, kv + 1:] *= 3.0  # below the diagonal: pivots often come from there
        ab[:, :, kv] += np.where(ab[:, :, kv] < 0, -3.0, 3.0)  # (random triangular factors are ill-conditioned: zero pivots by rounding)
    ab[:, :, :ml] = np.nan  # fill space
    for j in range(n):  # entries outside the matrix
        for r in range(ld):
            i = j + r - kv
            if r >= ml and not 0 <= i < n:
                ab[:, j, r] = 0.0
    return ab


def dense_of(ab, n, ml, mu):
    import idahip
    a = ab.copy()
    a[..., :ml] = 0.0
    return idahip.band_unpack(a, n, ml, mu)


def colmajor(m):
    return np.ascontiguousarray(np.transpose(m, (0, 2, 1)))


def run(ab, n, ml, mu, rhs, idx=None):
    """band setup + solve on the GPU -> (rc, info, factors [B][n][ldab], pivots, x)"""
    B = ab.shape[0]
    ctx = make_ctx(n, B)
    dA, dP = ctx.dev_array(ab), ctx.dev_array(np.zeros((B, n), dtype=np.int64))
    rc, info = ctx.ls_setup_band(ml, mu, dA, dP, idx)
    dB = ctx.dev_array(rhs)
    dX = ctx.dev_empty(8 * B * n)
    ok = np.arange(B) if idx is None else np.asarray(idx)
    ok = ok[info == 0]
    ctx.ls_solve_band(ml, mu, dA, dP, dX, dB, ok)
    out = ctx.to_host(dA, ab.shape), ctx.to_host(dP, (B, n), np.int64), ctx.to_host(dX, (B, n))
    for d in (dA, dP, dB, dX):
        ctx.dev_free(d)
    ctx.close()
    return (rc, info) + out


def check_against_oracle(ab0, n, ml, mu, rng, ties=False):
    import idahip
    B = ab0.shape[0]
    rhs = rng.standard_normal((B, n))
    rc, info, fac, piv, x = run(ab0, n, ml, mu, rhs)
    dense = dense_of(ab0, n, ml, mu)
    cm = colmajor(dense)
    oinfo, opiv = O.getrf_batch(cm)
    assert np.array_equal(info, oinfo) and rc == (1 if oinfo.any() else 0)
    good = np.flatnonzero(oinfo == 0)
    assert np.array_equal(piv[good], opiv[good])
    ox = O.getrs_batch(cm[good].copy(), opiv[good], rhs[good])
    assert np.array_equal(x[good], ox)  # by value
    ii, jj = np.indices((n, n))
    for q in good[:: max(1, len(good) // 16)]:
        olu = cm[q].T
        assert np.array_equal(idahip.band_expand_factors(fac[q], piv[q], n, ml, mu), olu), q
        # the theory: U has at most ml + mu super-diagonals, a column of L at most ml entries
        assert not np.any(olu[(jj - ii) > ml + mu]) and (np.count_nonzero(np.tril(olu, -1), axis=0) <= ml).all()
    return info


CASES = []
for n in SIZES:
    for band in BANDS:
        ml, mu = (n - 1, n - 1) if band == "full" else band
        if ml >= n or mu >= n or (band == "full" and n > 511):
            continue
        if n <= 64:
            B = 1024 if band in ((1, 1), (2, 5)) else 64
        else:
            B = {511: 32, 1025: 8, 4096: 4}[n] if band != "full" else 2
        CASES.append((n, ml, mu, B))
CASES = list(dict.fromkeys(CASES))  # (n = 1: the full band is the diagonal)


@pytest.mark.parametrize("n,ml,mu,B", CASES)
def test_band_lu_and_solve_equal_the_dense_oracle(n, ml, mu, B):
    rng = np.random.default_rng(n * 1009 + ml * 31 + mu)
    ab = random_band(rng, B, n, ml, mu)
    info = check_against_oracle(ab, n, ml, mu, rng)
    assert (info == 0).mean() >= 0.5  # (a zero pivot by rounding is allowed: the oracle's info is the yardstick)


@pytest.mark.parametrize("n,ml,mu", [(17, 1, 1), (64, 2, 5), (511, 3, 0), (1025, 1, 1)])
def test_pivot_ties_and_a_zero_pivot_in_one_system(n, ml, mu):
    rng = np.random.default_rng(5 * n + ml)
    B = 40
    ab = random_band(rng, B, n, ml, mu, ties=True)
    kv = ml + mu
    for q in range(B):  # no zero pivot by accident: a dominant diagonal keeps the small integers regular
        ab[q, :, kv] = np.where(np.arange(n) % 2 == 0, 7.0, -7.0) + (ab[q, :, kv] if q % 2 else 0.0)
        if q % 3 == 0:  # ... or ties against it on the sub-diagonal (the lowest row wins)
            ab[q, :, kv + 1:] = np.where(ab[q, :, kv + 1:] != 0.0, 7.0, 0.0)
    ab[11, 0, ml:] = 0.0  # system 11: column 0 is zero -> info 1
    info = check_against_oracle(ab, n, ml, mu, rng, ties=True)
    assert info[11] == 1  # (and every other system's info is the oracle's)


def test_subset_list_and_refused_lists():
    import idahip
    n, ml, mu, B = 100, 2, 3, 30
    rng = np.random.default_rng(77)
    ab = random_band(rng, B, n, ml, mu)
    idx = np.arange(1, B, 3)
    rhs = rng.standard_normal((B, n))
    rc, info, fac, piv, x = run(ab, n, ml, mu, rhs, idx)
    assert rc == 0 and not info.any()
    others = np.setdiff1d(np.arange(B), idx)
    assert np.array_equal(fac[others], ab[others], equal_nan=True)  # unlisted systems untouched
    cm = colmajor(dense_of(ab[idx], n, ml, mu))
    _, opiv = O.getrf_batch(cm)
    assert np.array_equal(piv[idx], opiv)
    assert np.array_equal(x[idx], O.getrs_batch(cm, opiv, rhs[idx]))
    ctx = make_ctx(n, B)
    dA, dP = ctx.dev_array(ab), ctx.dev_array(np.zeros((B, n), dtype=np.int64))
    for bad in ([0, 0], [3, 5, 3], [B], [-1]):
        with pytest.raises(idahip.IdaHipError):
            ctx.ls_setup_band(ml, mu, dA, dP, bad)
        with pytest.raises(idahip.IdaHipError):
            ctx.ls_solve_band(ml, mu, dA, dP, dA, dA, bad)
    for m_, u_ in ((n, 0), (0, n), (-1, 0)):
        with pytest.raises(idahip.IdaHipError):
            ctx.ls_setup_band(m_, u_, dA, dP, [0])
    assert np.array_equal(ctx.to_host(dA, ab.shape), ab, equal_nan=True)  # nothing launched
    ctx.close()


def test_reference_goldens_through_the_full_band():
    """The reference's LU and solve goldens (dense.rs:216-310, 3 x 3) as band matrices with ml = mu = n - 1."""
    import idahip
    G = json.load(open(os.path.join(GD, "dense_goldens.json")))
    mats = np.array([dict(G[k]["bindings"])["mat_a"] for k in ("test_get_rf1", "test_get_rf2")])
    exp = np.array([dict(G[k]["bindings"])["expect"] for k in ("test_get_rf1", "test_get_rf2")])
    ab = idahip.band_pack(mats, 2, 2)
    rc, info, fac, piv, _ = run(ab, 3, 2, 2, np.zeros((2, 3)))
    assert rc == 0 and not info.any() and piv.tolist() == [[2, 1, 2], [2, 1, 2]]
    for q in range(2):
        assert np.array_equal(idahip.band_expand_factors(fac[q], piv[q], 3, 2, 2), exp[q])
    names = ("test_get_rs1", "test_get_rs2")
    lus = np.array([dict(G[k]["bindings"])["mat_a"] for k in names])
    bs = np.array([dict(G[k]["bindings"])["b"] for k in names])
    pv = np.array([dict(G[k]["bindings"])["pivot"] for k in names], dtype=np.int64)
    sexp = np.array([dict(G[k]["bindings"])["expect"] for k in names])
    # the goldens' factors are in the dense layout; with ml = mu = n - 1 and these pivots, undo the later swaps of L (the inverse of
    # band_expand_factors) to get the band kernels' layout
    bands = []
    for q in range(2):
        L, U = np.tril(lus[q], -1), np.triu(lus[q])
        for j in reversed(range(3)):
            p = int(pv[q][j])
            if p != j:
                L[[j, p], :j] = L[[p, j], :j]
        ab_q = np.zeros((3, 7))  # ldab = 7, kv = 4: every entry of the 3 x 3 matrix is inside the band
        for j in range(3):
            for i in range(3):
                ab_q[j, 4 + i - j] = (L + U)[i, j]
        assert np.array_equal(idahip.band_expand_factors(ab_q, pv[q], 3, 2, 2), lus[q])
        bands.append(ab_q)
    ctx = make_ctx(3, 2)
    dA, dP, dB = ctx.dev_array(np.array(bands)), ctx.dev_array(pv), ctx.dev_array(bs)
    dX = ctx.dev_empty(8 * 2 * 3)
    ctx.ls_solve_band(2, 2, dA, dP, dX, dB)
    assert np.array_equal(ctx.to_host(dX, (2, 3)), sexp)  # the reference's exact bits (dense.rs:238,264)
    ctx.close()


def test_n_8192_two_systems_beyond_the_stepper_limit():
    n, ml, mu = 8192, 1, 1
    rng = np.random.default_rng(8192)
    ab = random_band(rng, 2, n, ml, mu)
    info = check_against_oracle(ab, n, ml, mu, rng)
    assert not info.any()
