"""_arrays.csc_pack: a batch of scipy-sparse matrices → the ABI's batched Julia
CSC arrays (int64, 1-based, running offsets) for the `_csc` calls — against
hand-written expectations (CPU only)."""

import numpy as np
import pytest
import scipy.sparse as sp

from diffopt_amd._arrays import csc_args, csc_pack, csc_split, is_sparse


def _m(rows, cols, vals, shape):
    return sp.csc_matrix((np.array(vals, float), (np.array(rows), np.array(cols))), shape=shape)


def test_ragged_batch_offsets():
    # problem 0: (0,0)=1, (2,0)=2, (1,2)=3      problem 1: (1,1)=4      problem 2: empty
    mats = [_m([0, 2, 1], [0, 0, 2], [1, 2, 3], (3, 3)), _m([1], [1], [4], (3, 3)), sp.csc_matrix((3, 3))]
    cp, rv, nz, nnz = csc_pack(mats, 3, (3, 3))
    assert nnz == 4
    assert cp.dtype == np.int64 and rv.dtype == np.int64 and nz.dtype == np.float64
    np.testing.assert_array_equal(cp, [1, 3, 3, 4,   4, 4, 5, 5,   5, 5, 5, 5])
    np.testing.assert_array_equal(rv, [1, 3, 2, 2])
    np.testing.assert_array_equal(nz, [1, 2, 3, 4])
    # ascending, disjoint ranges: cp_b[0] >= cp_{b-1}[n]
    for b in range(1, 3):
        assert cp[b * 4] >= cp[b * 4 - 1]
    parts = csc_split(nz, (cp, rv, nz, nnz), 3, 3)
    assert [list(p) for p in parts] == [[1, 2, 3], [4], []]


def test_shared_matrix_is_replicated_with_disjoint_ranges():
    M = _m([0, 1], [0, 1], [5, 6], (2, 2))
    cp, rv, nz, nnz = csc_pack(M, 3, (2, 2))
    assert nnz == 6
    np.testing.assert_array_equal(cp, [1, 2, 3,   3, 4, 5,   5, 6, 7])
    np.testing.assert_array_equal(rv, [1, 2] * 3)
    np.testing.assert_array_equal(nz, [5, 6] * 3)


def test_all_empty():
    cp, rv, nz, nnz = csc_pack(sp.csc_matrix((4, 2)), 2, (4, 2))
    assert nnz == 0 and rv.size == 0 and nz.size == 0
    np.testing.assert_array_equal(cp, np.ones(6, dtype=np.int64))
    assert csc_args((cp, rv, nz, nnz)) == [cp.ctypes.data, None, None, 0]
    assert csc_args(None) == [None, None, None, 0]
    assert csc_args(None, values=False) == [None, None, 0]


def test_unsorted_and_duplicated_input_comes_out_canonical():
    # column 0 holds rows [2, 0] unsorted; (1, 1) twice (3 + 4)
    M = sp.csc_matrix((np.array([7.0, 8.0, 3.0, 4.0]), np.array([2, 0, 1, 1]), np.array([0, 2, 4])), shape=(3, 2))
    assert not M.has_sorted_indices or not M.has_canonical_format
    before = (M.indices.copy(), M.data.copy(), M.indptr.copy())
    cp, rv, nz, nnz = csc_pack([M], 1, (3, 2))
    assert nnz == 3
    np.testing.assert_array_equal(cp, [1, 3, 4])
    np.testing.assert_array_equal(rv, [1, 3, 2])
    np.testing.assert_array_equal(nz, [8, 7, 7])
    # the caller's matrix is untouched
    np.testing.assert_array_equal(M.indices, before[0])
    np.testing.assert_array_equal(M.data, before[1])
    np.testing.assert_array_equal(M.indptr, before[2])
    # COO / CSR inputs are accepted
    cp2, rv2, nz2, _ = csc_pack([M.tocoo()], 1, (3, 2))
    np.testing.assert_array_equal(cp2, cp)
    np.testing.assert_array_equal(rv2, rv)
    np.testing.assert_array_equal(nz2, nz)


def test_wrong_shape_and_wrong_count():
    with pytest.raises(ValueError):
        csc_pack(sp.csc_matrix((3, 2)), 2, (2, 3))
    with pytest.raises(ValueError):
        csc_pack([sp.csc_matrix((3, 2)), sp.csc_matrix((3, 3))], 2, (3, 2))
    with pytest.raises(ValueError):
        csc_pack([sp.csc_matrix((3, 2))], 2, (3, 2))


def test_is_sparse():
    assert is_sparse(sp.csc_matrix((2, 2)))
    assert is_sparse([sp.csr_matrix((2, 2)), sp.coo_matrix((2, 2))])
    assert not is_sparse(None)
    assert not is_sparse(np.zeros((1, 2, 2)))
    assert not is_sparse([np.zeros((2, 2))])
