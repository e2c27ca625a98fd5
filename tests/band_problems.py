"""A banded linear DAE F = A y' + B y - c whose Jacobians B + cj A make partial pivoting swap rows, for the band ctx tests.

TEST INFRASTRUCTURE ONLY. Every other band integration of the suite is the heat problem. Its Jacobian is tridiagonal; partial
pivoting swaps rows there only in a run of columns that starts at the algebraic boundary row (the oracle: 27 of 257 columns at
cj = 1e4), and U never reaches beyond its second super-diagonal. On a band ctx with mu >= 2 that lies inside the band: the fill
above the mu-th super-diagonal (the top ml rows of the band storage) stays zero and a solve that ignored it would pass every
heat test. Here the differential block carries 2 x 2 blocks [[0.3, 1], [1, 0.3]] on its diagonal: for
every cj of an integration the sub-diagonal entry of such a pair outweighs the diagonal one, the rows are swapped and U fills.
tests/test_band_problems.py asserts that on the oracle for every case the GPU tests use.

The systems come in the dict shape of idahip.problems.linear_dense (A, B column-major per system), so that
oracle_lib.run_ensemble("linear_dense", ...) integrates them as they are; host_callbacks gives the same systems to a band ctx."""
import numpy as np

import dq_ref

RTOL, ATOL = 1.0e-6, 1.0e-8
TOUTS = 0.1 * np.arange(1, 6)
# (n, ml, mu) of the whole integrations (test_gpu_band_widths.py): sizes on both sides of 256 and 1024, one-sided bands, a wide
# band, the full band
INTEGRATIONS = [(64, 2, 3), (257, 2, 3), (257, 0, 2), (257, 3, 0), (100, 7, 5), (1100, 2, 3), (24, 23, 23)]


# bandwidths and sizes of the setup / Newton-body tests: (1, 1) takes the register kernels (the control), every other width the
# generic ones; sizes on both sides of the 256-thread stride of the scatter / pack kernels, of 1024 and up to the band ctx limit
WIDTHS = [(1, 1), (0, 0), (0, 2), (3, 0), (2, 3), (7, 5), (16, 16), "full"]
SIZES = [9, 17, 64, 257, 1025, 4096]
TOP_WIDTHS = [(1, 1), (2, 3), (16, 16)]  # at n = 4096 (generating and factoring one case on the host takes 15 s there)


def setup_cases():
    """(n, ml, mu) of every width at every size where it fits; the full band at n <= 17, TOP_WIDTHS at n = 4096."""
    out = []
    for n in SIZES:
        for w in WIDTHS:
            ml, mu = (n - 1, n - 1) if w == "full" else w
            if ml >= n or mu >= n or (w == "full" and n > 17) or (n == 4096 and w not in TOP_WIDTHS):
                continue
            if (n, ml, mu) not in out:
                out.append((n, ml, mu))
    return out


def setup_batch(n):
    return 5 if n <= 257 else 4 if n <= 1025 else 3


def in_band(n, ml, mu):
    ii, jj = np.indices((n, n))
    return (ii - jj <= ml) & (jj - ii <= mu)


def _system(n, ml, mu, seed):
    """One system: (A column-major, B column-major, c, y0, yp0); idahip.problems._linear_system restricted to the band."""
    rng = np.random.default_rng(seed)
    band = in_band(n, ml, mu)
    nd = (3 * n) // 4  # differential unknowns first, algebraic last
    nd -= nd % 2
    A = np.where(band, 0.05 * rng.uniform(-1.0, 1.0, (n, n)), 0.0)
    A[nd:, :] = 0.0
    A[:, nd:] = 0.0
    k = np.arange(0, nd, 2)
    A[k, k] += 0.3
    A[k + 1, k + 1] += 0.3
    if ml >= 1 and mu >= 1:  # the pair (2k, 2k + 1): |A(2k + 1, 2k)| > |A(2k, 2k)|
        A[k + 1, k] += 1.0
        A[k, k + 1] += 1.0
    else:  # a one-sided band has no room for the pair: A += I
        A[k, k] += 0.7
        A[k + 1, k + 1] += 0.7
    Bm = np.where(band, -(0.5 / np.sqrt(ml + mu + 1)) * rng.standard_normal((n, n)), 0.0)
    Bm[np.arange(n), np.arange(n)] -= 1.0 + rng.uniform()
    c = rng.uniform(-1.0, 1.0, n)
    y0, yp0 = np.zeros(n), np.zeros(n)  # consistent initial values, as _linear_system computes them
    y0[nd:] = np.linalg.solve(Bm[nd:, nd:], c[nd:])
    yp0[:nd] = np.linalg.solve(A[:nd, :nd], c[:nd] - Bm[:nd, nd:] @ y0[nd:])
    return np.ascontiguousarray(A.T), np.ascontiguousarray(Bm.T), c, y0, yp0


def banded_linear(n, ml, mu, batch, seed=None):
    """`batch` systems with lower / upper bandwidths ml, mu (system s from the generator seed + s; seed defaults to 1000 n)."""
    assert 0 <= ml < n and 0 <= mu < n
    seed = 1000 * n if seed is None else seed
    S = [_system(n, ml, mu, seed + s) for s in range(batch)]
    A, Bm, c, y0, yp0 = (np.stack([s[i] for s in S]) for i in range(5))
    return {"kind": "linear_dense", "n": n, "A": A, "B": Bm, "c": c, "yy0": y0, "yp0": yp0, "rtol": RTOL, "atol": np.array([ATOL]),
            "touts": TOUTS.copy(), "band": (ml, mu)}


def jacobian(prob, s, cj):
    """B_s + cj A_s, [n][n] column-major: elementwise, the oracle's B[e] + cj * A[e]."""
    return prob["B"][s] + cj * prob["A"][s]


def host_callbacks(prob):
    """(res, bjac) for Ctx.set_host_band_problem: the oracle's residual (its summation order) and its Jacobian in band storage."""
    import idahip
    ml, mu = prob["band"]
    A, Bm, c = prob["A"], prob["B"], prob["c"]

    def res(s, t, y, yp):
        return dq_ref.linear_res(A[s], Bm[s], c[s], y, yp)

    def bjac(s, t, cj, y, yp, r, ab):
        return idahip.band_pack(jacobian(prob, s, cj).T, ml, mu)

    return res, bjac


def as_host_callback(prob):
    """The problem as idahip.problems.make_ctx(..., band=True) takes it; "oracle_kind" tells the comparing code what the oracle runs."""
    res, bjac = host_callbacks(prob)
    return dict(prob, kind="host_callback", oracle_kind="linear_dense", res=res, bjac=bjac)
