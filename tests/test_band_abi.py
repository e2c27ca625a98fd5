"""CPU checks of the band solver's boundary: the header declares the band entry points and the library exports them, the numpy
band-storage helpers round-trip, and the helper that expands band factors into dense_get_rf's layout does so on a hand-worked
4 x 4 factorisation with one row swap (checked against the oracle's dense_get_rf as well)."""
import ctypes as C
import os
import re

import numpy as np

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND_SYMBOLS = ["idahip_create_band", "idahip_band", "idahip_set_host_band_problem", "idahip_download_lu_band", "idahip_ls_setup_band",
                "idahip_ls_solve_band"]


def test_header_declares_and_library_exports_the_band_entry_points():
    import idahip
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ida_hip.h")).read(), flags=re.S)
    assert "idahip_band_jac_fn" in txt
    H = C.CDLL(idahip.LIB_HIP, mode=C.RTLD_GLOBAL)
    for s in BAND_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert s in idahip.HIP_SYMBOLS, s
        assert hasattr(H, s), s


def test_band_pack_unpack_round_trip():
    import idahip
    rng = np.random.default_rng(7)
    for n, ml, mu in [(1, 0, 0), (2, 1, 1), (5, 0, 3), (5, 3, 0), (9, 2, 5), (6, 5, 5), (17, 7, 3)]:
        full = rng.standard_normal((3, n, n))
        ii, jj = np.indices((n, n))
        inband = (ii - jj <= ml) & (jj - ii <= mu)
        dense = np.where(inband, full, 0.0)
        ab = idahip.band_pack(dense, ml, mu)
        assert ab.shape == (3, n, idahip.band_ldab(ml, mu))
        assert np.array_equal(ab[..., :ml], np.zeros_like(ab[..., :ml]))  # fill rows start empty
        assert np.array_equal(idahip.band_unpack(ab, n, ml, mu), dense)
        assert np.array_equal(idahip.band_unpack(idahip.band_pack(full, ml, mu), n, ml, mu), dense)  # outside the band: dropped
        for j in range(n):  # the storage rule: ab[j, ml + mu + i - j] = A(i, j)
            for i in range(max(0, j - mu), min(n, j + ml + 1)):
                assert ab[1, j, ml + mu + i - j] == dense[1, i, j]


# A (ml = mu = 1) and its band factorisation, worked by hand in dgbtf2's steps:
#   k = 0: pivot row 0 (2 > 1); l10 = 1 * (1/2) = 0.5; a11 = 1 - 1 * 0.5 = 0.5; a12 untouched (a02 == 0: skipped)
#   k = 1: pivot row 2 (|2| > |0.5|): rows 1 and 2 swap over columns 1..3 -> row 1 = [2, 2, 1], row 2 = [0.5, 1, 0];
#          l21 = 0.5 * (1/2) = 0.25; a22 = 1 - 2 * 0.25 = 0.5; a23 = 0 - 1 * 0.25 = -0.25 (U13 = 1 lands in the fill row)
#   k = 2: pivot row 2 (0.5 > 0.25); l32 = 0.25 * (1/0.5) = 0.5; a33 = 1 - (-0.25) * 0.5 = 1.125
#   k = 3: pivot row 3
A4 = np.array([[2.0, 1.0, 0.0, 0.0],
               [1.0, 1.0, 1.0, 0.0],
               [0.0, 2.0, 2.0, 1.0],
               [0.0, 0.0, 0.25, 1.0]])
# band storage, row j = column j: [fill (i = j - 2), i = j - 1, i = j, i = j + 1]; l10 stays where step 0 computed it
AB4 = np.array([[0.0, 0.0, 2.0, 0.5],
                [0.0, 1.0, 2.0, 0.25],
                [0.0, 2.0, 0.5, 0.5],
                [1.0, -0.25, 1.125, 0.0]])
PIV4 = np.array([0, 2, 2, 3], dtype=np.int64)
# dense_get_rf's factors: the same U, and L with step 1's swap applied to column 0 (l10 moves to row 2)
LU4 = np.array([[2.0, 1.0, 0.0, 0.0],
                [0.0, 2.0, 2.0, 1.0],
                [0.5, 0.25, 0.5, -0.25],
                [0.0, 0.0, 0.5, 1.125]])


def test_expand_band_factors_to_the_dense_layout():
    import idahip
    assert np.array_equal(idahip.band_pack(A4, 1, 1)[:, 1:], np.array([[0, 2, 1], [1, 1, 2], [1, 2, 0.25], [1, 1, 0]], dtype=float))
    got = idahip.band_expand_factors(AB4, PIV4, 4, 1, 1)
    assert np.array_equal(got, LU4)
    info, lu, piv = O.getrf(A4)
    assert info == 0 and np.array_equal(piv, PIV4) and np.array_equal(lu, LU4)


def test_expand_applies_every_later_swap_in_order():
    """A random band matrix factored by a numpy transcription of dgbtf2 (the band kernels' loops), expanded, equals dense_get_rf."""
    import idahip
    rng = np.random.default_rng(3)
    for n, ml, mu in [(7, 2, 1), (9, 3, 2), (12, 1, 1), (6, 5, 5)]:
        ii, jj = np.indices((n, n))
        A = np.where((ii - jj <= ml) & (jj - ii <= mu), rng.standard_normal((n, n)), 0.0)
        ab = idahip.band_pack(A, ml, mu)
        kv = ml + mu
        piv = np.zeros(n, dtype=np.int64)
        ju = 0
        for j in range(n):
            km = min(ml, n - 1 - j)
            jp = 0
            for r in range(1, km + 1):
                if abs(ab[j, kv + r]) > abs(ab[j, kv + jp]):
                    jp = r
            piv[j] = j + jp
            ju = max(ju, min(j + mu + jp, n - 1))
            for c in range(j, ju + 1):
                a, b = kv + j - c, kv + j + jp - c
                ab[c, a], ab[c, b] = ab[c, b], ab[c, a]
            mult = 1.0 / ab[j, kv]
            ab[j, kv + 1:kv + km + 1] *= mult
            for c in range(j + 1, ju + 1):
                akj = ab[c, kv + j - c]
                if akj != 0.0:
                    for r in range(1, km + 1):
                        ab[c, kv + j + r - c] -= akj * ab[j, kv + r]
        info, lu, opiv = O.getrf(A)
        assert info == 0 and np.array_equal(piv, opiv)
        assert np.array_equal(idahip.band_expand_factors(ab, piv, n, ml, mu), lu)  # by value
