"""The dense plug-point cases (dense_plug_cases.py) are what they claim — on
the CPU alone, so test_dense_plug_gpu.py cannot quietly test nothing: every
right-hand side is exact; the no-pivot acceptance rule takes ``dom`` and
refuses ``perm`` / ``antidiag`` / ``gauss`` (decisively: no verdict hangs on
a rounding); a spike of 10 passes and one of 10.5 does not; a zeroed column j
puts an exactly zero pivot at column j + 1 and nowhere else; the oracle
corrects every saddle once; and LAPACK's own backward and forward error on
every regular case, which is the yardstick the GPU test scales its bars by.
Every case prints one line (pytest -s)."""

import numpy as np
import pytest

import dense_plug_cases as dc
from oracle import nlp as onlp

PIN_ROWS = tuple(r for r in dc.BLOCK_ROWS) + (384,)   # acceptance pinned up to 384 rows
SEEDS = (0, 1)                                         # the two matrices of a batch


@pytest.mark.parametrize("family", dc.FAMILIES)
def test_rhs_exact(family):
    for rows in dc.BLOCK_ROWS + (dc.CHUNK_ROWS, dc.SPIKE_ROWS) + dc.PACK_ROWS:
        for seed in SEEDS:
            for trans in (False, True):
                assert dc.exact_rhs(dc.matrix(family, rows, seed), 3, seed, trans), (family, rows, seed, trans)
    M = dc.matrix(family, dc.CHUNK_ROWS, 0)
    assert dc.exact_rhs(M, 33, 0) and dc.exact_rhs(M, 33, 0, True)
    X = dc.solution(dc.CHUNK_ROWS, 33, 0)
    assert np.abs(X).max() <= 8 and (X == np.round(X)).all() and (np.abs(X).sum(axis=0) > 0).all()
    assert len({X[:, c].tobytes() for c in range(33)}) == 33      # no two seeds alike


@pytest.mark.parametrize("family", dc.STORAGE_FAMILIES)
@pytest.mark.parametrize("rows", (480, 1153, dc.PIVOT_MAX))
def test_rhs_exact_large(family, rows):
    assert dc.exact_rhs(dc.matrix(family, rows, 0), 3, 0) and dc.exact_rhs(dc.matrix(family, rows, 1), 3, 1, True)


@pytest.mark.parametrize("family", dc.FAMILIES)
def test_nopiv_rule(family):
    for rows in PIN_ROWS:
        for seed in SEEDS:
            M = dc.matrix(family, rows, seed)
            s = dc.nopiv_scan(M)
            plain = dc.nopiv_scan(M, nb=1)
            assert plain["accept"] == s["accept"] and plain["column"] == s["column"], (family, rows, seed, s, plain)
            assert dc.decisive(s) and dc.decisive(plain), (family, rows, seed, s, plain)
            # a 1 × 1 matrix has no multiplier to refuse; every other perm / antidiag / gauss case is refused
            want = family == "dom" or rows == 1
            assert s["accept"] == want == dc.accepts(family, rows, seed), (family, rows, seed, s)
            if family != "dom":
                assert dc.first_singular_column(M) == 0, (family, rows, seed)   # refused, yet regular
        print(f"[dense-plug] {family} rows {rows}: accept {s['accept']}, max |l| {s['lmax']:.3g}, "
              f"max |u| / bound {s['umax']:.2g}, stopped at column {s['column']}")


def test_storage_sizes():
    """The sizes of the storage table sit where qp_multi.hip and abi.hip put
    their thresholds (restated here)."""
    def lds_v(rows):
        return ((rows + 31) // 32 * 32) * (dc.MKC * 8 + 4)
    assert lds_v(480) <= 64 * 1024 < lds_v(481)
    assert lds_v(1152) <= 150 * 1024 < lds_v(1153)
    assert lds_v(1152) == 148.5 * 1024 and (1153 + 31) // 32 * 32 == 1184
    lo, hi = dc.PACK_ROWS
    assert (lo * lo + lo) * 8 <= dc.LHS_PACK_MAX < (hi * hi + hi) * 8 and hi == lo + 1
    assert max(dc.STORAGE_ROWS) == dc.PIVOT_MAX
    assert (dc.SPIKE_ROWS + 31) // 32 * 32 == 160


@pytest.mark.parametrize("site", dc.SPIKE_SITES)
def test_spike_threshold(site):
    i, j = site
    for c in dc.SPIKE_C:
        M = dc.spike(dc.SPIKE_ROWS, i, j, c)
        s = dc.nopiv_scan(M)
        assert s["accept"] == (abs(c) <= dc.NOPIV_LMAX) and s["lmax"] == abs(c), (site, c, s)
        assert dc.nopiv_scan(M, nb=1)["accept"] == s["accept"]
        assert dc.exact_rhs(M, 3) and dc.exact_rhs(M, 3, 0, True)
        # the exact solve: x_i = b_i − c·b_j, every other entry b itself; integers or halves below 2^8
        B, X = dc.rhs(M, 3)
        S = B.copy()
        S[i] -= c * B[j]
        np.testing.assert_array_equal(S, X)


@pytest.mark.parametrize("family", ("dom", "perm"))
@pytest.mark.parametrize("rows", dc.SINGULAR_ROWS)
def test_zero_column_pivot(family, rows):
    for j in dc.singular_columns(rows):
        Z = dc.zero_col(family, rows, 1, j)
        piv = dc.pivots(Z)
        assert piv[j] == 0.0, (family, rows, j)
        assert (np.delete(piv, j) > 1.0).all(), (family, rows, j, np.delete(piv, j).min())
        assert dc.first_singular_column(Z) == j + 1
        assert not dc.nopiv_accepts(Z)
    print(f"[dense-plug] zero_col({family}, rows {rows}): zero pivot at j + 1 for j in {dc.singular_columns(rows)}")


@pytest.mark.parametrize("family", ("dom", "perm"))
@pytest.mark.parametrize("rows", dc.SINGULAR_ROWS)
def test_tiny_column_pivot(family, rows):
    """Column j scaled by 2^-80: the pivots are those of the unscaled matrix
    but for u_jj, which is tiny and not zero; the no-pivot rule's verdict is
    the unscaled matrix's (its multipliers are the same numbers)."""
    M = dc.matrix(family, rows, 1)
    for j in dc.singular_columns(rows):
        T = dc.tiny_col(family, rows, 1, j)
        piv, ref = dc.pivots(T), dc.pivots(M)
        assert piv[j] == ref[j] * 2.0 ** -80 and piv[j] > 0.0
        np.testing.assert_array_equal(np.delete(piv, j), np.delete(ref, j))
        assert (np.delete(piv, j) > 1.0).all()
        assert dc.first_singular_column(T) == j + 1
        s = dc.nopiv_scan(T)
        assert s["accept"] == (family == "dom") and dc.decisive(s), (family, rows, j, s)


@pytest.mark.parametrize("rows", dc.SADDLE_ROWS + (129,))
def test_saddle_corrected_once(rows):
    nw, nc = dc.saddle_split(rows)
    assert nw + nc == rows
    for zr in (0, nc - 1):
        M = dc.saddle(nw, nc, zr)
        np.testing.assert_array_equal(M, M.T)
        assert not M[nw + zr].any() and not M[:, nw + zr].any()
        K, corr = onlp.lu_with_inertia_correction(M, nw, nc)
        assert K is not None and corr == 1, (rows, zr, corr)
        assert dc.first_singular_column(M) > 0
        C = dc.saddle_corrected(M, nw, nc, 1)
        assert dc.first_singular_column(C) == 0
        cond = np.linalg.cond(C)
        assert 1e7 <= cond <= 1e9, cond      # the 1e-6 shift alone carries the zero row: no forward-error bar
        print(f"[dense-plug] saddle rows {rows} (nw {nw}, nc {nc}), zero row {zr}: oracle corrections {corr}, "
              f"condition of the corrected matrix {cond:.2e}")


# LAPACK's own error on the cases: the yardstick of the GPU test's bars
# (max(c·LAPACK, rows·ε)).  The ceilings are those of a backward-stable LU:
# η of a few ε, and a forward error of condition × η — the dominant families'
# condition is below 10, the [−9, 9] integer matrices' (∞-norm) up to a few 1e5 at 257 rows.
ETA_MAX = 64 * dc.EPS


@pytest.mark.parametrize("family", dc.FAMILIES)
def test_lapack_yardstick(family):
    worst_eta = worst_fwd = 0.0
    for rows in dc.BLOCK_ROWS:
        for seed in SEEDS:
            M = dc.matrix(family, rows, seed)
            cond = np.linalg.cond(M, np.inf)
            assert cond <= (1e6 if family == "gauss" else 10.0), (family, rows, seed, cond)
            for trans in (False, True):
                e, f = (v.max() for v in dc.lapack(family, rows, seed, 3, trans))
                assert e <= ETA_MAX, (family, rows, seed, trans, e / dc.EPS)
                assert f <= 4 * cond * ETA_MAX, (family, rows, seed, trans, f, cond)
                worst_eta, worst_fwd = max(worst_eta, e), max(worst_fwd, f)
    assert worst_fwd <= (1e-11 if family == "gauss" else 1e-15), worst_fwd
    print(f"[dense-plug] LAPACK on {family}: worst η {worst_eta / dc.EPS:.2f} ε, worst forward error {worst_fwd:.2e}")
