"""Array staging between numpy (host) / torch-CUDA (device) and the C ABI.

The ABI wants column-major, batch-major float64 buffers (include header).  A
numpy/torch array of shape (B, r, c) in the usual C order is transposed to
(B, c, r) C-contiguous, which is exactly (B, r, c) column-major per problem.
Device tensors are passed zero-copy (DOPT_MEM_DEVICE) on torch's current
stream; host arrays are passed by pointer and copied by the library.
"""

import numpy as np

from . import _lib


def _is_torch(x):
    return x is not None and type(x).__module__.startswith("torch")


def _is_cuda(x):
    return _is_torch(x) and x.is_cuda


def colmajor(X, shape):
    """Batch of matrices (B, r, c) → per-problem column-major contiguous buffer."""
    if X is None:
        return None
    B, r, c = shape
    if _is_torch(X):
        import torch
        X = X.reshape(B, r, c).to(torch.float64)
        return X.transpose(1, 2).contiguous()
    X = np.asarray(X, dtype=np.float64).reshape(B, r, c)
    return np.ascontiguousarray(np.swapaxes(X, 1, 2))


def vector(x, shape):
    if x is None:
        return None
    if _is_torch(x):
        import torch
        return x.reshape(shape).to(torch.float64).contiguous()
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(shape))


def is_sparse(x):
    """scipy.sparse matrix, or a list / tuple of them (a batch of sparse tangents)."""
    if x is None or _is_torch(x) or isinstance(x, np.ndarray):
        return False
    import scipy.sparse as sp
    if sp.issparse(x):
        return True
    return isinstance(x, (list, tuple)) and len(x) > 0 and all(sp.issparse(M) for M in x)


def csc_pack(mats, B, shape):
    """Batch of scipy-sparse matrices → the ABI's batched Julia CSC arrays
    ``(colptr, rowval, nzval, nnz)``: int64, 1-based; problem b's colptr is
    ``colptr[b*(ncols+1):(b+1)*(ncols+1)]`` and indexes the concatenated
    rowval / nzval (running offsets, so the problems' ranges are ascending and
    disjoint — a shared matrix is replicated).  Each matrix is canonicalised on
    a copy (duplicates summed, row indices sorted; the caller's is not
    modified); the values of problem b are
    ``nzval[colptr[b*(ncols+1)]-1 : colptr[(b+1)*(ncols+1)-1]-1]`` in that
    matrix's canonical CSC order.  ValueError on a shape mismatch."""
    import scipy.sparse as sp
    mats = [mats] * B if sp.issparse(mats) else list(mats)
    if len(mats) != B:
        raise ValueError(f"{len(mats)} sparse matrices for a batch of {B}")
    cps, rvs, nzs, off = [], [], [], 0
    for M in mats:
        if tuple(M.shape) != tuple(shape):
            raise ValueError(f"sparse matrix of shape {tuple(M.shape)}, expected {tuple(shape)}")
        M = sp.csc_matrix(M, dtype=np.float64, copy=True)
        M.sum_duplicates()
        M.sort_indices()
        cps.append(M.indptr.astype(np.int64) + (off + 1))
        rvs.append(M.indices.astype(np.int64) + 1)
        nzs.append(M.data.astype(np.float64))
        off += int(M.nnz)
    ncols = int(shape[1])
    colptr = np.ascontiguousarray(np.concatenate(cps)) if cps else np.zeros(0, dtype=np.int64)
    assert colptr.size == B * (ncols + 1)
    rowval = np.ascontiguousarray(np.concatenate(rvs)) if cps else np.zeros(0, dtype=np.int64)
    nzval = np.ascontiguousarray(np.concatenate(nzs)) if cps else np.zeros(0, dtype=np.float64)
    return colptr, rowval, nzval, off


def csc_args(packed, values=True):
    """ctypes arguments of one packed matrix (``None``: absent): colptr,
    rowval, [nzval,] nnz, with NULL rowval / nzval for nnz == 0."""
    if packed is None:
        return [None, None, None, 0] if values else [None, None, 0]
    cp, rv, nz, nnz = packed
    a = [cp.ctypes.data, rv.ctypes.data if nnz else None]
    if values:
        a.append(nz.ctypes.data if nnz else None)
    return a + [nnz]


def csc_split(values, packed, B, ncols):
    """Per-problem views of a packed value array: a list of B arrays."""
    cp = packed[0]
    return [values[cp[b * (ncols + 1)] - 1: cp[(b + 1) * (ncols + 1) - 1] - 1].copy() for b in range(B)]


class Staged:
    """Decides host vs device mode for one ABI call and yields raw pointers."""

    def __init__(self, arrays):
        present = [a for a in arrays if a is not None]
        cuda = [_is_cuda(a) for a in present]
        if any(cuda) and not all(cuda):
            raise TypeError("mix of host and device arrays in one call")
        self.mem = _lib.DOPT_MEM_DEVICE if (present and all(cuda)) else _lib.DOPT_MEM_HOST
        self.stream = None      # host mode: the handle's private stream
        self.set_stream = False
        if self.mem == _lib.DOPT_MEM_DEVICE:
            self.set_stream = True
            import torch
            self.stream = torch.cuda.current_stream(present[0].device).cuda_stream

    @staticmethod
    def ptr(a):
        if a is None:
            return None
        if _is_torch(a):
            return a.data_ptr()
        return a.ctypes.data

    @staticmethod
    def empty(shape, device):
        if device:
            import torch
            return torch.empty(shape, dtype=torch.float64, device="cuda")
        return np.empty(shape, dtype=np.float64)
