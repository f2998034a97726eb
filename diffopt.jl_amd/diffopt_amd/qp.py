"""QuadraticProgram back-end on the MI355X engine.

Mirrors ``DiffOpt.QuadraticProgram`` (reference
``src/QuadraticProgram/QuadraticProgram.jl``):

* ``QPBatch`` — the batched C-ABI handle (one KKT system per problem, all
  problems of one shape).  Accepts numpy arrays (host memory, copied into HBM)
  or torch CUDA tensors (device memory, zero-copy, inputs resident in HBM).
* ``Model`` — a single-problem model with the reference's plugin-interface
  vocabulary: ``VariablePrimalStart``/``ConstraintDualStart`` setters with the
  dual sign flip (:164-180), ``ReverseVariablePrimal`` inputs,
  ``reverse_differentiate`` (:316-351), ``forward_differentiate`` (:357-446),
  ``ForwardVariablePrimal`` (:299-305), ``ReverseObjectiveFunction``
  (:448-458), ``ReverseConstraintFunction`` (``_get_dA``/``_get_db``
  :307-314, :461-473) and ``DifferentiateTimeSec``.
"""

import ctypes

import numpy as np

from . import _lib
from ._arrays import Staged, colmajor, csc_args, csc_pack, csc_split, is_sparse, vector
from ._arrays import _is_torch as _is_t

LE, EQ = "LessThan", "EqualTo"


def _check_out(o, shape, device):
    """A caller-supplied output buffer must be exactly what the kernels write:
    float64, C-contiguous, `shape`, and in the memory kind of the call."""
    if _is_t(o):
        import torch
        ok = (o.dtype == torch.float64 and o.is_contiguous() and tuple(o.shape) == tuple(shape)
              and o.is_cuda == bool(device))
    else:
        ok = (not device and isinstance(o, np.ndarray) and o.dtype == np.float64
              and o.flags.c_contiguous and o.shape == tuple(shape))
    if not ok:
        raise TypeError(f"output buffer must be a C-contiguous float64 {'CUDA tensor' if device else 'numpy array'} "
                        f"of shape {tuple(shape)}")


class QPBatch:
    """Batched QP sensitivity engine (C-ABI handle wrapper)."""

    DENSE_MAX = 8192   # n + m + p of the dense route; above it the handle is sparse (dopt_set_sparse)

    def __init__(self, batch, n, m, p=0, device=0, sparse=False):
        self.lib = _lib.load()
        self.batch, self.n, self.m, self.p = int(batch), int(n), int(m), int(p)
        self.device = device
        h = ctypes.c_void_p()
        rc = self.lib.dopt_create(ctypes.byref(h), device, self.batch, self.n, self.m,
                                  self.p, _lib.DOPT_KIND_QP)
        if rc != 0:
            raise _lib.EngineError(rc, "dopt_create failed (no HIP device?)")
        self.h = h
        self._mem = None
        self._keep = None
        # the sparse route (sparse.hip): automatic above the dense cap, opt-in below
        self.sparse = bool(sparse) or self.L > self.DENSE_MAX
        if sparse:
            _lib.check(self.lib.dopt_set_sparse(self.h, 1), self.h)

    def lsqr_stats(self):
        """Sparse route: (B, 2, 2) int32 — [istop, iterations] of the last
        reverse (index 0) and forward (index 1) LSQR runs per problem."""
        out = np.zeros(4 * self.batch, dtype=np.int32)
        _lib.check(self.lib.dopt_qp_lsqr_stats(self.h, out.ctypes.data), self.h)
        return out.reshape(2, self.batch, 2).transpose(1, 0, 2)

    def close(self):
        if getattr(self, "h", None):
            self.lib.dopt_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    # ---- memory mode -------------------------------------------------------
    def _stage(self, arrays):
        st = Staged(arrays)
        if self._mem != st.mem:
            _lib.check(self.lib.dopt_set_memory(self.h, st.mem), self.h)
            self._mem = st.mem
        if st.set_stream and st.stream != getattr(self, "_stream", -1):
            _lib.check(self.lib.dopt_set_stream(self.h, st.stream), self.h)
            self._stream = st.stream
        return st

    @property
    def L(self):
        return self.n + self.m + self.p

    def set(self, Q, G=None, h=None, A=None, z=None, lam=None, nu=None):
        """Problem data and primal–dual point (λ, ν in OptNet sign)."""
        B, n, m, p = self.batch, self.n, self.m, self.p
        st = self._stage([Q, G, h, A, z, lam, nu])
        Qc = colmajor(Q, (B, n, n))
        Gc = colmajor(G, (B, m, n)) if m else None
        Ac = colmajor(A, (B, p, n)) if p else None
        args = [Qc, Gc, vector(h, (B, m)) if m else None, Ac, vector(z, (B, n)),
                vector(lam, (B, m)) if m else None, vector(nu, (B, p)) if p else None]
        self._keep = args  # device mode borrows: keep the staged tensors alive
        rc = self.lib.dopt_qp_set(self.h, *[st.ptr(a) for a in args])
        _lib.check(rc, self.h)

    def set_csc(self, Q, G=None, h=None, A=None, z=None, lam=None, nu=None):
        """``set`` with Q, G, A as sparse matrices in the reference's MOI
        matrix form (scipy.sparse, one per problem or one shared by all;
        converted to Julia CSC arrays: Int64, 1-based) — dopt_qp_set_csc
        densifies them on the device.  Host mode."""
        B, n, m, p = self.batch, self.n, self.m, self.p

        def csc(mats, rows):
            import scipy.sparse as sp
            if mats is None or rows == 0:
                return None, None, None, 0
            if sp.issparse(mats):
                mats = [mats] * B
            cps, rvs, nzs, off = [], [], [], 0
            for M in mats:
                M = sp.csc_matrix(M)
                if M.shape != (rows, n):
                    raise ValueError(f"sparse matrix of shape {M.shape}, expected {(rows, n)}")
                cps.append(M.indptr.astype(np.int64) + off + 1)
                rvs.append(M.indices.astype(np.int64) + 1)
                nzs.append(M.data.astype(np.float64))
                off += M.nnz
            return (np.ascontiguousarray(np.concatenate(cps)), np.ascontiguousarray(np.concatenate(rvs)),
                    np.ascontiguousarray(np.concatenate(nzs)), off)

        st = self._stage([z, h, lam, nu])
        if st.mem != _lib.DOPT_MEM_HOST:
            raise TypeError("set_csc takes host (numpy / scipy) arrays")
        mats = [csc(Q, n), csc(G, m), csc(A, p)]
        vecs = [vector(h, (B, m)) if m else None, vector(z, (B, n)),
                vector(lam, (B, m)) if m else None, vector(nu, (B, p)) if p else None]
        args = []
        for cp, rv, nz, nnz in mats:
            args += [st.ptr(cp), st.ptr(rv if nnz else None), st.ptr(nz if nnz else None), nnz]
        args += [st.ptr(v) for v in vecs]
        self._csc_keep = (mats, vecs)   # the arrays behind `args`
        self.set_csc_args(args)
        return args

    def set_csc_args(self, args):
        """dopt_qp_set_csc on the ctypes arguments a previous ``set_csc``
        returned (arrays kept alive by this object): the ABI call alone, as the
        Julia back-end issues it with the MOI matrix form already in hand."""
        rc = self.lib.dopt_qp_set_csc(self.h, *args)
        _lib.check(rc, self.h)

    def factor(self, singular_ok=False):
        return _lib.check(self.lib.dopt_qp_factor(self.h), self.h, singular_ok)

    def _out(self, like_device):
        return Staged.empty((self.batch, self.L), like_device)

    def reverse(self, dl_dz, singular_ok=False):
        """Returns (B, n+m+p) = [dz | dλ | dν]."""
        st = self._stage([dl_dz])
        d = vector(dl_dz, (self.batch, self.n))
        out = self._out(st.mem == _lib.DOPT_MEM_DEVICE)
        rc = self.lib.dopt_qp_reverse(self.h, st.ptr(d), st.ptr(out))
        _lib.check(rc, self.h, singular_ok)
        return out

    def _csc_tangents(self, dQ, dq, dG, dh, dA, db, extra=()):
        """The `_csc` calls' tangent arguments: scipy-sparse dQ / dG / dA (one
        shared matrix or a list of B, each with its own pattern; None = zero)
        packed, the vector tangents staged.  Returns (st, ctypes args, keep)."""
        B, n, m, p = self.batch, self.n, self.m, self.p
        for M in (dQ, dG, dA):
            if M is not None and not is_sparse(M):
                raise TypeError("dQ, dG and dA must all be scipy-sparse (or None) when one of them is")
        st = self._stage([dq, dh, db, *extra])
        if st.mem != _lib.DOPT_MEM_HOST:
            raise TypeError("scipy-sparse tangents go with host (numpy) vector tangents")
        packs = [csc_pack(dQ, B, (n, n)) if dQ is not None else None,
                 csc_pack(dG, B, (m, n)) if (dG is not None and m) else None,
                 csc_pack(dA, B, (p, n)) if (dA is not None and p) else None]
        vecs = [vector(dq, (B, n)) if dq is not None else None,
                vector(dh, (B, m)) if (dh is not None and m) else None,
                vector(db, (B, p)) if (db is not None and p) else None]
        args = []
        for pk, v in zip(packs, vecs):
            args += csc_args(pk) + [st.ptr(v)]
        return st, args, (packs, vecs)

    def forward(self, dQ=None, dq=None, dG=None, dh=None, dA=None, db=None,
                singular_ok=False):
        """``dQ`` / ``dG`` / ``dA``: dense (B, rows, n) arrays, or — on a
        sparse-route handle — scipy-sparse matrices with their own patterns
        (dopt_qp_forward_csc: no dense rows × n array anywhere)."""
        B, n, m, p = self.batch, self.n, self.m, self.p
        if any(is_sparse(M) for M in (dQ, dG, dA)):
            st, args, keep = self._csc_tangents(dQ, dq, dG, dh, dA, db)
            out = self._out(False)
            rc = self.lib.dopt_qp_forward_csc(self.h, *args, st.ptr(out))
            _lib.check(rc, self.h, singular_ok)
            return out
        st = self._stage([dQ, dq, dG, dh, dA, db])
        args = [colmajor(dQ, (B, n, n)) if dQ is not None else None,
                vector(dq, (B, n)) if dq is not None else None,
                colmajor(dG, (B, m, n)) if (dG is not None and m) else None,
                vector(dh, (B, m)) if (dh is not None and m) else None,
                colmajor(dA, (B, p, n)) if (dA is not None and p) else None,
                vector(db, (B, p)) if (db is not None and p) else None]
        out = self._out(st.mem == _lib.DOPT_MEM_DEVICE)
        rc = self.lib.dopt_qp_forward(self.h, *[st.ptr(a) for a in args], st.ptr(out))
        _lib.check(rc, self.h, singular_ok)
        return out

    def reverse_k(self, dl_dz, singular_ok=False):
        """k seeds per problem on one factorisation (dopt_qp_reverse_k):
        dl_dz (k, B, n) → (k, B, n+m+p); equal to k ``reverse`` calls to
        rounding, the blocked problems' k solves in one MFMA launch."""
        k = int(dl_dz.shape[0])
        B, n = self.batch, self.n
        st = self._stage([dl_dz])
        d = vector(dl_dz, (k, B, n))
        out = Staged.empty((k, B, self.L), st.mem == _lib.DOPT_MEM_DEVICE)
        rc = self.lib.dopt_qp_reverse_k(self.h, k, st.ptr(d), st.ptr(out))
        _lib.check(rc, self.h, singular_ok)
        return out

    def _dual_seeds(self, k, dl_dz, dl_dlam, dl_dnu):
        """The three seed blocks of a `_duals` call as the ABI takes them
        ((k·B, ·) vectors; None = zero, and for a block the model lacks)."""
        kb = k * self.batch
        st = self._stage([dl_dz, dl_dlam, dl_dnu])
        seeds = [vector(dl_dz, (kb, self.n)) if dl_dz is not None else None,
                 vector(dl_dlam, (kb, self.m)) if (dl_dlam is not None and self.m) else None,
                 vector(dl_dnu, (kb, self.p)) if (dl_dnu is not None and self.p) else None]
        return st, seeds

    def reverse_duals_k(self, dl_dz=None, dl_dlam=None, dl_dnu=None, singular_ok=False):
        """``reverse_k`` for a loss on the duals too (dopt_qp_reverse_duals_k):
        seeds (k, B, n) / (k, B, m) / (k, B, p), None = zero, with respect to
        the engine's λ and ν (OptNet sign: minus the MOI duals) →
        (k, B, n+m+p) = −LHS⁻¹·[dl/dz; dl/dλ; dl/dν] per seed.  The output feeds
        the same getters as ``reverse``'s.  A sparse-route handle takes k = 1."""
        given = [a for a in (dl_dz, dl_dlam, dl_dnu) if a is not None]
        if not given:
            raise ValueError("reverse_duals needs at least one seed block")
        k = int(given[0].shape[0])
        st, seeds = self._dual_seeds(k, dl_dz, dl_dlam, dl_dnu)
        out = Staged.empty((k, self.batch, self.L), st.mem == _lib.DOPT_MEM_DEVICE)
        rc = self.lib.dopt_qp_reverse_duals_k(self.h, k, *[st.ptr(a) for a in seeds], st.ptr(out))
        _lib.check(rc, self.h, singular_ok)
        return out

    def reverse_duals(self, dl_dz=None, dl_dlam=None, dl_dnu=None, singular_ok=False):
        """One seed per problem (``reverse_duals_k`` with k = 1): seeds (B, n) /
        (B, m) / (B, p) → (B, n+m+p)."""
        one = [None if a is None else a[None] for a in (dl_dz, dl_dlam, dl_dnu)]
        return self.reverse_duals_k(*one, singular_ok=singular_ok)[0]

    def forward_k(self, dQ=None, dq=None, dG=None, dh=None, dA=None, db=None, singular_ok=False):
        """k tangents per problem (dopt_qp_forward_k): each given tangent has a
        leading seed axis (k, B, …) → (k, B, n+m+p)."""
        given = [a for a in (dQ, dq, dG, dh, dA, db) if a is not None]
        if not given:
            raise ValueError("forward_k needs at least one tangent")
        k = int(given[0].shape[0])
        B, n, m, p = self.batch, self.n, self.m, self.p
        st = self._stage([dQ, dq, dG, dh, dA, db])
        kb = k * B
        args = [colmajor(dQ, (kb, n, n)) if dQ is not None else None,
                vector(dq, (kb, n)) if dq is not None else None,
                colmajor(dG, (kb, m, n)) if (dG is not None and m) else None,
                vector(dh, (kb, m)) if (dh is not None and m) else None,
                colmajor(dA, (kb, p, n)) if (dA is not None and p) else None,
                vector(db, (kb, p)) if (db is not None and p) else None]
        out = Staged.empty((k, B, self.L), st.mem == _lib.DOPT_MEM_DEVICE)
        rc = self.lib.dopt_qp_forward_k(self.h, k, *[st.ptr(a) for a in args], st.ptr(out))
        _lib.check(rc, self.h, singular_ok)
        return out

    def forward_reverse(self, dl_dz, dQ=None, dq=None, dG=None, dh=None, dA=None,
                        db=None, out_rev=None, out_fwd=None, singular_ok=False):
        """One full sensitivity solve per problem: factor + reverse + forward.
        scipy-sparse ``dQ`` / ``dG`` / ``dA`` as in ``forward``
        (dopt_qp_forward_reverse_csc)."""
        B, n, m, p = self.batch, self.n, self.m, self.p
        if any(is_sparse(M) for M in (dQ, dG, dA)):
            st, args, keep = self._csc_tangents(dQ, dq, dG, dh, dA, db, extra=(dl_dz,))
            o1 = out_rev if out_rev is not None else self._out(False)
            o2 = out_fwd if out_fwd is not None else self._out(False)
            for o in (o1, o2):
                _check_out(o, (B, self.L), False)
            d = vector(dl_dz, (B, n))
            rc = self.lib.dopt_qp_forward_reverse_csc(self.h, st.ptr(d), *args, st.ptr(o1), st.ptr(o2))
            _lib.check(rc, self.h, singular_ok)
            return o1, o2
        st = self._stage([dl_dz, dQ, dq, dG, dh, dA, db])
        dev = st.mem == _lib.DOPT_MEM_DEVICE
        args = [vector(dl_dz, (B, n)),
                colmajor(dQ, (B, n, n)) if dQ is not None else None,
                vector(dq, (B, n)) if dq is not None else None,
                colmajor(dG, (B, m, n)) if (dG is not None and m) else None,
                vector(dh, (B, m)) if (dh is not None and m) else None,
                colmajor(dA, (B, p, n)) if (dA is not None and p) else None,
                vector(db, (B, p)) if (db is not None and p) else None]
        o1 = out_rev if out_rev is not None else self._out(dev)
        o2 = out_fwd if out_fwd is not None else self._out(dev)
        for o in (o1, o2):
            _check_out(o, (B, self.L), dev)
        rc = self.lib.dopt_qp_forward_reverse(self.h, *[st.ptr(a) for a in args],
                                              st.ptr(o1), st.ptr(o2))
        _lib.check(rc, self.h, singular_ok)
        return o1, o2

    # ---- parameters (ParametricOptInterface glue, reference src/parameters.jl)
    @staticmethod
    def _terms(terms, with_var=False):
        """terms: iterable of (param, kind, index, coef) — kinds 0 LessThan row,
        1 EqualTo row, 2 objective, 3 objective parameter×variable (index = v) —
        or, for the ``_k`` calls, (param, kind, row, coef, var) — kinds 4 / 5: the
        parameter×variable term of LessThan / EqualTo row ``row`` and variable
        ``var``.  ``with_var``: also the variables' array (None when no term
        carries one)."""
        t = list(terms)
        par = np.ascontiguousarray([int(x[0]) for x in t], dtype=np.int32)
        kind = np.ascontiguousarray([int(x[1]) for x in t], dtype=np.int32)
        idx = np.ascontiguousarray([int(x[2]) for x in t], dtype=np.int32)
        coef = np.ascontiguousarray([float(x[3]) for x in t], dtype=np.float64)
        if not with_var:
            return len(t), par, kind, idx, coef
        var = None
        if any(len(x) > 4 for x in t):
            var = np.ascontiguousarray([int(x[4]) if len(x) > 4 else 0 for x in t], dtype=np.int32)
        return len(t), par, kind, idx, var, coef

    def params_reverse(self, rev, terms, nparam):
        """ReverseConstraintSet of every parameter of every problem, (B, nparam),
        from a reverse output ``rev`` (B, n+m+p) — dopt_qp_params_reverse."""
        B = self.batch
        nt, par, kind, idx, coef = self._terms(terms)
        st = self._stage([rev])
        r = vector(rev, (B, self.L))
        out = Staged.empty((B, nparam), st.mem == _lib.DOPT_MEM_DEVICE)
        p = Staged.ptr
        rc = self.lib.dopt_qp_params_reverse(self.h, st.ptr(r), nparam, nt, p(par), p(kind), p(idx), p(coef),
                                             st.ptr(out))
        _lib.check(rc, self.h)
        return out

    def params_forward(self, dp, terms):
        """Parameter tangents dp (B, nparam) → the forward tangents (dq, dh, db)
        the reference's POI glue sets (dopt_qp_params_forward), ready for
        ``forward(dq=…, dh=…, db=…)``."""
        B, n, m, p_ = self.batch, self.n, self.m, self.p
        nparam = int(dp.shape[1])
        nt, par, kind, idx, coef = self._terms(terms)
        st = self._stage([dp])
        d = vector(dp, (B, nparam))
        dev = st.mem == _lib.DOPT_MEM_DEVICE
        dq, dh, db = Staged.empty((B, n), dev), Staged.empty((B, m), dev), Staged.empty((B, p_), dev)
        pp = Staged.ptr
        rc = self.lib.dopt_qp_params_forward(self.h, st.ptr(d), nparam, nt, pp(par), pp(kind), pp(idx), pp(coef),
                                             st.ptr(dq), st.ptr(dh) if m else None, st.ptr(db) if p_ else None)
        _lib.check(rc, self.h)
        return dq, dh, db

    def params_forward_k(self, dp, terms, singular_ok=False):
        """k parameter tangents per problem, solves included
        (dopt_qp_params_forward_k): dp (k, B, nparam) → (k, B, n+m+p), seed j's
        block = ``forward`` on the tangents the terms define (kinds 4 / 5: dG /
        dA entries), the right-hand sides written straight from the term table."""
        k, B, nparam = int(dp.shape[0]), self.batch, int(dp.shape[2])
        nt, par, kind, idx, var, coef = self._terms(terms, True)
        st = self._stage([dp])
        d = vector(dp, (k, B, nparam))
        out = Staged.empty((k, B, self.L), st.mem == _lib.DOPT_MEM_DEVICE)
        pp = Staged.ptr
        rc = self.lib.dopt_qp_params_forward_k(self.h, k, st.ptr(d), nparam, nt, pp(par), pp(kind), pp(idx),
                                               pp(var), pp(coef), st.ptr(out))
        _lib.check(rc, self.h, singular_ok)
        return out

    def params_reverse_k(self, dl_dz, terms, nparam, want_rev=False, singular_ok=False):
        """k seeds per problem through the reverse solve and the parameter
        accumulation (dopt_qp_params_reverse_k): dl_dz (k, B, n) → out_dp
        (k, B, nparam), or (out_dp, rev (k, B, n+m+p)) with ``want_rev``."""
        k, B, nparam = int(dl_dz.shape[0]), self.batch, int(nparam)
        nt, par, kind, idx, var, coef = self._terms(terms, True)
        st = self._stage([dl_dz])
        d = vector(dl_dz, (k, B, self.n))
        dev = st.mem == _lib.DOPT_MEM_DEVICE
        out = Staged.empty((k, B, nparam), dev)
        rev = Staged.empty((k, B, self.L), dev) if want_rev else None
        pp = Staged.ptr
        rc = self.lib.dopt_qp_params_reverse_k(self.h, k, st.ptr(d), nparam, nt, pp(par), pp(kind), pp(idx),
                                               pp(var), pp(coef), st.ptr(rev), st.ptr(out))
        _lib.check(rc, self.h, singular_ok)
        return (out, rev) if want_rev else out

    def params_reverse_duals_k(self, dl_dz, dl_dlam, dl_dnu, terms, nparam, want_rev=False, singular_ok=False):
        """``params_reverse_k`` with seeds on the duals too
        (dopt_qp_params_reverse_duals_k): seeds as ``reverse_duals_k``'s →
        out_dp (k, B, nparam), or (out_dp, rev (k, B, n+m+p)) with ``want_rev``."""
        given = [a for a in (dl_dz, dl_dlam, dl_dnu) if a is not None]
        if not given:
            raise ValueError("params_reverse_duals_k needs at least one seed block")
        k, B, nparam = int(given[0].shape[0]), self.batch, int(nparam)
        nt, par, kind, idx, var, coef = self._terms(terms, True)
        st, seeds = self._dual_seeds(k, dl_dz, dl_dlam, dl_dnu)
        dev = st.mem == _lib.DOPT_MEM_DEVICE
        out = Staged.empty((k, B, nparam), dev)
        rev = Staged.empty((k, B, self.L), dev) if want_rev else None
        pp = Staged.ptr
        rc = self.lib.dopt_qp_params_reverse_duals_k(self.h, k, *[st.ptr(a) for a in seeds], nparam, nt, pp(par),
                                                     pp(kind), pp(idx), pp(var), pp(coef), st.ptr(rev), st.ptr(out))
        _lib.check(rc, self.h, singular_ok)
        return (out, rev) if want_rev else out

    def params_jacobian(self, terms, nparam, mode, device=False, singular_ok=False):
        """The parameter Jacobian of every problem by unit seeds, one call.
        ``mode`` 0 (or "forward"): (B, n+m+p, nparam), column j = [dz/dp_j;
        dλ/dp_j; dν/dp_j] (dopt_qp_params_forward_k with dp = NULL); 1 (or
        "reverse"): (B, n, nparam), row i = ReverseConstraintSet of every
        parameter for the seed e_i (dopt_qp_params_reverse_k with dl_dz = NULL).
        A numpy array, or with ``device`` a torch CUDA tensor written in place
        by the kernels (on torch's current stream); a view of the seed-major
        buffer either way."""
        mode = {"forward": 0, "reverse": 1}.get(mode, mode)
        if mode not in (0, 1):
            raise ValueError("mode must be 0 (forward) or 1 (reverse)")
        B, n, nparam = self.batch, self.n, int(nparam)
        nt, par, kind, idx, var, coef = self._terms(terms, True)
        K = n if mode == 1 else nparam
        J = Staged.empty((K, B, nparam if mode == 1 else self.L), device)
        self._stage([J] if device else [])   # the memory mode (and torch's stream) follow the output
        pp = Staged.ptr
        if mode == 0:
            rc = self.lib.dopt_qp_params_forward_k(self.h, K, None, nparam, nt, pp(par), pp(kind), pp(idx), pp(var),
                                                   pp(coef), pp(J))
        else:
            rc = self.lib.dopt_qp_params_reverse_k(self.h, K, None, nparam, nt, pp(par), pp(kind), pp(idx), pp(var),
                                                   pp(coef), None, pp(J))
        _lib.check(rc, self.h, singular_ok)
        if device:
            return J.permute(1, 2, 0) if mode == 0 else J.permute(1, 0, 2)
        return J.transpose(1, 2, 0) if mode == 0 else J.transpose(1, 0, 2)

    def reverse_grads(self, rev, dQ=True, dG=True, dA=True):
        """Materialised reverse gradients of every problem from a reverse
        output ``rev`` (B, n+m+p) — ``ReverseObjectiveFunction`` /
        ``ReverseConstraintFunction`` (QuadraticProgram.jl:448-473, :307-314):
        dict with dq (B, n), dQ (B, n, n), dG (B, m, n), g_const (B, m),
        dA (B, p, n), a_const (B, p); the gradients w.r.t. h and b are
        −g_const and −a_const.  Matrices are returned as (B, rows, cols)
        views of the column-major buffers."""
        B, n, m, p = self.batch, self.n, self.m, self.p
        st = self._stage([rev])
        dev = st.mem == _lib.DOPT_MEM_DEVICE
        r = vector(rev, (B, n + m + p))
        out = {"dq": Staged.empty((B, n), dev),
               "dQ": Staged.empty((B, n, n), dev) if dQ else None,
               "dG": Staged.empty((B, n, m), dev) if (dG and m) else None,
               "g_const": Staged.empty((B, m), dev) if m else None,
               "dA": Staged.empty((B, n, p), dev) if (dA and p) else None,
               "a_const": Staged.empty((B, p), dev) if p else None}
        rc = self.lib.dopt_qp_reverse_grads(
            self.h, st.ptr(r), *[st.ptr(out[k]) for k in ["dQ", "dq", "dG", "g_const", "dA", "a_const"]])
        _lib.check(rc, self.h)
        for k in ("dQ", "dG", "dA"):   # column-major (B, cols, rows) → (B, rows, cols) view
            if out[k] is not None:
                out[k] = out[k].transpose(1, 2) if _is_t(out[k]) else np.swapaxes(out[k], 1, 2)
        return out

    def reverse_grads_at(self, rev, G=None, A=None, Q=None):
        """``reverse_grads``' matrix gradients read at the entries of patterns
        (dopt_qp_reverse_grads_csc, sparse-route handles; the reference's lazy
        getters, QuadraticProgram.jl:461-473) — no dense rows × n array.
        ``G`` / ``A`` / ``Q``: scipy-sparse patterns (one shared or a list of
        B); ``None`` for G / A = the pattern the handle got from ``set_csc``,
        for Q = skipped.  Returns a dict of lists of B value arrays ("dG",
        "dA", and "dQ" when asked), problem b's aligned with its pattern's
        canonical CSC order (a given pattern: duplicates summed, rows sorted;
        the handle's own: the order ``set_csc`` passed)."""
        B, n, m, p = self.batch, self.n, self.m, self.p
        st = self._stage([rev])
        if st.mem != _lib.DOPT_MEM_HOST:
            raise TypeError("reverse_grads_at takes a host (numpy) rev")
        r = vector(rev, (B, self.L))
        own = getattr(self, "_csc_keep", (None, None))[0]

        def pick(pat, rows, slot):
            if rows == 0 or (pat is None and slot == 0):
                return None, [None, None, 0], None
            if pat is not None:
                pk = csc_pack(pat, B, (rows, n))
                return pk, csc_args(pk, values=False), np.zeros(max(pk[3], 1))
            if own is None or own[slot][0] is None:
                raise _lib.EngineError(-1, "reverse_grads_at: no pattern given and none kept from set_csc")
            return own[slot], [None, None, 0], np.zeros(max(own[slot][3], 1))

        picks = [pick(Q, n, 0), pick(G, m, 1), pick(A, p, 2)]
        args = []
        for pk, a, out in picks:
            args += a + [out.ctypes.data if out is not None else None]
        rc = self.lib.dopt_qp_reverse_grads_csc(self.h, st.ptr(r), *args)
        _lib.check(rc, self.h)
        res = {}
        for key, (pk, a, out) in zip(("dQ", "dG", "dA"), picks):
            if out is not None:
                res[key] = csc_split(out, pk, B, n)
        return res

    # ---- introspection -----------------------------------------------------
    def info(self):
        buf = np.zeros(self.batch, dtype=np.int32)
        _lib.check(self.lib.dopt_get_info(self.h, buf.ctypes.data), self.h)
        return buf

    def iterative(self):
        buf = np.zeros(self.batch, dtype=np.int8)
        _lib.check(self.lib.dopt_get_iterative(self.h, buf.ctypes.data), self.h)
        return buf.astype(bool)

    def system_size(self):
        buf = np.zeros(self.batch, dtype=np.int32)
        _lib.check(self.lib.dopt_get_system_size(self.h, buf.ctypes.data), self.h)
        return buf

    def last_time(self):
        return self.lib.dopt_last_time(self.h)

    def kept(self):
        """(B, m) bool mask of the inequality rows kept in the factorised
        system (False: eliminated exactly, λ_i == 0 and (Gz − h)_i != 0)."""
        buf = np.zeros((self.batch, self.m), dtype=np.int8)
        _lib.check(self.lib.dopt_qp_get_kept(self.h, buf.ctypes.data), self.h)
        return buf.astype(bool)

    def lu_kind(self):
        """Per-problem factorisation kind of the last factorisation:
        _lib.LU_KIND_LSQR / LU_KIND_NOPIV / LU_KIND_PIVOT, or LU_KIND_SMALL after a
        reverse call the one-workgroup small path served (qp_small.hip)."""
        buf = np.zeros(self.batch, dtype=np.int8)
        _lib.check(self.lib.dopt_qp_get_lu_kind(self.h, buf.ctypes.data), self.h)
        return buf

    def sym_route(self):
        """Per problem: 1 when the last factorisation took the P-symmetric
        no-pivot route (lower trailing tiles, U from L), else 0."""
        buf = np.zeros(self.batch, dtype=np.int8)
        _lib.check(self.lib.dopt_qp_get_sym(self.h, buf.ctypes.data), self.h)
        return buf

    def set_profiling(self, on=True, phases=None):
        """Per-phase HIP-event timing on (all phases, or only the phase names
        in `phases`) or off."""
        if phases is None:
            _lib.check(self.lib.dopt_set_profiling(self.h, int(bool(on))), self.h)
        else:
            mask = _lib.phase_mask(self.lib, phases) if on else 0
            _lib.check(self.lib.dopt_set_profiling_phases(self.h, mask), self.h)

    def phase_times(self):
        """{phase name: (total ms, launches)} since the last call (HIP events
        on the handle's stream)."""
        return _lib.phase_times(self.lib, self.h)

    def split(self, out):
        n, m = self.n, self.m
        return out[:, :n], out[:, n:n + m], out[:, n + m:]


class MI355XSolver:
    """The MI355X solver of the reference's ``LinearAlgebraSolver`` plug point
    (QuadraticProgram.jl:475-502; the Julia ``DiffOptMI355X.MI355XSolver``):
    ``solve_system(LHS, RHS, iterative)`` is ``iterative ? lsqr(LHS, RHS) :
    LHS \\ RHS`` on the device (dopt_lhs_solve).  The reference calls it twice
    per model (reverse with LHS, :335; forward with LHS', :438) and its
    callers loop models of one size, so the solver keeps one engine handle
    per (batch, rows) instead of creating one per call."""

    def __init__(self, device=0):
        self.device = device
        self._h = None
        self._key = None
        self._single = True    # the last solve_system's LHS was one matrix, not a batch (resolve)
        self._fact = None      # (memory key of the array factorised last, the array)
        self.resolves = 0      # calls served by dopt_lhs_resolve (introspection)
        self.lib = _lib.load()

    def close(self):
        if self._h is not None:
            self.lib.dopt_destroy(self._h)
            self._h = None
            self._key = None
            self._fact = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self, B, rows):
        if self._key != (B, rows):
            self.close()
            h = ctypes.c_void_p()
            rc = self.lib.dopt_create(ctypes.byref(h), self.device, B, rows, 0, 0, _lib.DOPT_KIND_NLP)
            if rc != 0:
                raise _lib.EngineError(rc, "dopt_create failed (no HIP device?)")
            self._h, self._key = h, (B, rows)
        return self._h

    def solve_system(self, LHS, RHS, iterative=False):
        """LHS (rows, rows) or a batch (B, rows, rows); RHS (rows,) / (rows, k)
        or batched (B, rows) / (B, rows, k).  A singular LHS raises
        SingularException(info), as ``\\`` does — on the engine's
        rank-revealing test |u_ii| ≤ rows·ε·max|M| (include/diffopt_mi355x.h,
        dopt_lhs_solve), which is stricter than ``\\``'s exactly-zero pivot."""
        M = np.asarray(LHS, dtype=np.float64)
        single = M.ndim == 2
        if single:
            M = M[None]
        B, rows = M.shape[0], M.shape[-1]
        if M.shape != (B, rows, rows):
            raise TypeError("LHS must be square")
        R = np.asarray(RHS, dtype=np.float64)
        if single:
            R = R[None]
        vec = R.ndim == 2
        Rk = R[..., None] if vec else R                     # (B, rows, k)
        if Rk.shape[:2] != (B, rows):
            raise TypeError("RHS does not match LHS")
        k = Rk.shape[2]
        rhs = np.ascontiguousarray(np.transpose(Rk, (2, 0, 1)))   # seed-major (k, B, rows)
        out = np.empty_like(rhs)
        h = self._handle(B, rows)
        self._single = single
        # the reference's second call per model passes LHS' (an adjoint of the
        # LHS it just solved with: QuadraticProgram.jl:335, :438): an array
        # that is exactly the transpose of the one factorised last (same
        # memory, shape and strides reversed) AND whose contents still equal
        # the matrix factorised (a copy kept at that call: an edit in place
        # between the two calls refactorises, as `\` would) is answered from
        # those factors, once per factorisation; any other call factorises
        lhs = LHS if isinstance(LHS, np.ndarray) else None
        key = None
        if lhs is not None and lhs.ndim == 2:
            key = (lhs.__array_interface__["data"][0], lhs.shape, lhs.strides)
        reuse = (not iterative and key is not None and self._fact is not None
                 and (key[0], key[1][::-1], key[2][::-1]) == self._fact[0]
                 and np.array_equal(lhs.T, self._fact[1]))
        if reuse:
            rc = self.lib.dopt_lhs_resolve(h, k, rhs.ctypes.data, out.ctypes.data, 1)
            self.resolves += 1
            self._fact = None
        else:
            Mc = np.ascontiguousarray(np.swapaxes(M, 1, 2))        # column-major per problem
            rc = self.lib.dopt_lhs_solve(h, rows, Mc.ctypes.data, k, rhs.ctypes.data, out.ctypes.data,
                                         int(bool(iterative)))
            # (the contents factorised, for the reuse check above)
            self._fact = None if iterative or key is None else (key, np.array(lhs, copy=True))
        _lib.check(rc, h)
        X = np.transpose(out, (1, 2, 0))                           # (B, rows, k)
        if vec:
            X = X[..., 0]
        return X[0] if single else X

    def resolve(self, RHS, trans=False):
        """A further solve on the factors of the last non-iterative
        ``solve_system`` (dopt_lhs_resolve): ``LHS \\ RHS``, or ``LHS' \\ RHS``
        with `trans`.  RHS shaped as that call's (batched exactly when its LHS
        was); raises SingularException(info) again if that LHS was singular."""
        if self._h is None:
            raise _lib.EngineError(-1, "resolve: no solve_system call on this solver yet")
        B, rows = self._key
        R = np.asarray(RHS, dtype=np.float64)
        single = self._single
        if single:
            R = R[None]
        vec = R.ndim == 2
        Rk = R[..., None] if vec else R
        if Rk.ndim != 3 or Rk.shape[:2] != (B, rows):
            raise TypeError("RHS does not match the factorised LHS")
        k = Rk.shape[2]
        rhs = np.ascontiguousarray(np.transpose(Rk, (2, 0, 1)))
        out = np.empty_like(rhs)
        rc = self.lib.dopt_lhs_resolve(self._h, k, rhs.ctypes.data, out.ctypes.data, int(bool(trans)))
        self.resolves += 1
        _lib.check(rc, self._h)
        X = np.transpose(out, (1, 2, 0))
        if vec:
            X = X[..., 0]
        return X[0] if single else X

    def lu_kind(self):
        """Per-problem factorisation kind of the last ``solve_system``:
        _lib.LU_KIND_NOPIV / LU_KIND_PIVOT (dopt_qp_get_lu_kind)."""
        if self._h is None:
            raise _lib.EngineError(-1, "lu_kind: no solve_system call on this solver yet")
        buf = np.zeros(self._key[0], dtype=np.int8)
        _lib.check(self.lib.dopt_qp_get_lu_kind(self._h, buf.ctypes.data), self._h)
        return buf


def solve_system(LHS, RHS, iterative=False, device=0, solver=None):
    """``QuadraticProgram.solve_system(solver, LHS, RHS, iterative)`` (see
    MI355XSolver): one call on `solver`'s cached handle, or on a temporary
    solver when none is given."""
    if solver is not None:
        return solver.solve_system(LHS, RHS, iterative)
    s = MI355XSolver(device)
    try:
        return s.solve_system(LHS, RHS, iterative)
    finally:
        s.close()


class Model:
    """Single-problem ``DiffOpt.QuadraticProgram.Model`` on the engine.

    Problem data is given in the matrix form the reference builds from MOI
    (``_gradient_cache``, :182-213): ``Q`` (symmetric Hessian), ``q``, ``G``,
    ``h`` (LessThan rows), ``A``, ``b`` (EqualTo rows).  Tangent sign handling
    of ``_fill`` (diff_opt.jl:594-656) happens in the setters below.
    """

    def __init__(self, device=0):
        self.device = device
        self.empty()

    # MOI.empty! (:126-137)
    def empty(self):
        self.Q = self.q = self.G = self.h = self.A = self.b = None
        self.x = None
        self.lam = None
        self.nu = None
        self._engine = None
        self.forw_grad_cache = None
        self.back_grad_cache = None
        self.diff_time = float("nan")
        self.input_dx = {}
        self.input_dy = {LE: {}, EQ: {}}   # ReverseConstraintDual: row -> seed on the engine's λ / ν
        self.input_objective = None      # (dQ, dq)
        self.input_le = {}               # row -> (coeffs, constant)
        self.input_eq = {}
        self.param_terms, self.nparam = [], 0
        self.input_dp = {}               # parameter -> ForwardConstraintSet direction
        self.back_param_cache = None

    def set_problem(self, Q, q, G=None, h=None, A=None, b=None, param_terms=(), nparam=0):
        """``param_terms``: the parametric terms of the problem's ``nparam``
        parameters (``QPBatch._terms``: 4-tuples of kinds 0-3, 5-tuples
        (param, kind, row, coef, var) of kinds 4 / 5), every constraint written
        as G z ≤ h / A z = b with its parametric part on the left."""
        self.param_terms = [tuple(t) for t in param_terms]
        self.nparam = int(nparam)
        self.input_dp = {}
        n = np.asarray(q).shape[0]
        self.Q = np.asarray(Q, dtype=np.float64).reshape(n, n)
        self.q = np.asarray(q, dtype=np.float64)
        self.G = np.zeros((0, n)) if G is None else np.asarray(G, float).reshape(-1, n)
        self.h = np.zeros(0) if h is None else np.asarray(h, float).ravel()
        self.A = np.zeros((0, n)) if A is None else np.asarray(A, float).reshape(-1, n)
        self.b = np.zeros(0) if b is None else np.asarray(b, float).ravel()
        self._engine = None

    @property
    def n(self):
        return self.q.shape[0]

    # ---- starts (diff_opt.jl:362-370, QuadraticProgram.jl:164-180) ---------
    def set_variable_primal_start(self, x):
        self.x = np.asarray(x, dtype=np.float64).copy()
        self._engine = None

    def set_constraint_dual_start(self, kind, duals):
        """MOI ``ConstraintDual`` values; stored with the OptNet sign flip."""
        d = -np.asarray(duals, dtype=np.float64)
        if kind == LE:
            self.lam = d
        elif kind == EQ:
            self.nu = d
        else:
            raise ValueError(kind)
        self._engine = None

    # ---- sensitivity inputs -------------------------------------------------
    def set_reverse_variable_primal(self, i, value):
        self.input_dx[int(i)] = float(value)

    def set_reverse_constraint_dual(self, kind, row, value):
        """``ReverseConstraintDual`` of row ``row`` (moi_wrapper.jl:532-533): the
        loss gradient with respect to the MOI ``ConstraintDual``, stored with
        the OptNet sign flip of ``set_constraint_dual_start``.  The reference's
        QP back-end ignores the attribute; here ``reverse_differentiate`` solves
        with it (QPBatch.reverse_duals_k)."""
        if kind not in (LE, EQ):
            raise ValueError(kind)
        self.input_dy[kind][int(row)] = -float(value)

    def set_forward_objective_function(self, dQ=None, dq=None):
        self.input_objective = (dQ, dq)

    def set_forward_constraint_function(self, kind, row, coeffs, constant):
        """Tangent of the constraint function ``coeffsᵀx + constant`` of row
        ``row`` (``func``-in-``set``).  ``_fill``: the constant is negated for
        both EqualTo and LessThan (it is the tangent of the set constant)."""
        tgt = self.input_le if kind == LE else self.input_eq
        tgt[int(row)] = (np.asarray(coeffs, dtype=np.float64), float(constant))

    def set_forward_parameter(self, p, value):
        """``ForwardConstraintSet`` of ``ParameterRef(p)``: the direction ``Parameter(value)``."""
        if not 0 <= int(p) < self.nparam:
            raise IndexError(f"parameter {p} of {self.nparam}")
        self.input_dp[int(p)] = float(value)

    def empty_input_sensitivities(self):
        self.input_dx = {}
        self.input_dy = {LE: {}, EQ: {}}
        self.input_objective = None
        self.input_le = {}
        self.input_eq = {}
        self.input_dp = {}

    # ---- engine ------------------------------------------------------------
    def _ensure(self):
        n, m, p = self.n, self.G.shape[0], self.A.shape[0]
        if self.x is None or len(self.x) < n or np.any(np.isnan(self.x)):
            raise ValueError("VariablePrimalStart missing")
        lam = np.zeros(m) if self.lam is None else self.lam
        nu = np.zeros(p) if self.nu is None else self.nu
        if self._engine is None:
            e = QPBatch(1, n, m, p, self.device)
            e.set(self.Q[None], self.G[None], self.h[None], self.A[None], self.x[None],
                  lam[None], nu[None])
            self._engine = e
            self._lam, self._nu = lam, nu
        return self._engine

    def reverse_differentiate(self):
        import time
        t0 = time.perf_counter()
        e = self._ensure()
        dl = np.zeros(self.n)
        for i, v in self.input_dx.items():
            dl[i] = v
        if self.input_dy[LE] or self.input_dy[EQ]:   # a loss on the duals too: the seeded solves
            gl, gn = np.zeros(self.G.shape[0]), np.zeros(self.A.shape[0])
            for i, v in self.input_dy[LE].items():
                gl[i] = v
            for i, v in self.input_dy[EQ].items():
                gn[i] = v
            seeds = (dl[None, None], gl[None, None], gn[None, None])
            if self.nparam:
                dp, rev = e.params_reverse_duals_k(*seeds, self.param_terms, self.nparam, want_rev=True)
                self.back_param_cache = np.asarray(dp)[0, 0]
            else:
                rev = e.reverse_duals_k(*seeds)
                self.back_param_cache = None
            out = np.asarray(rev)[0, 0]
        elif self.nparam:   # the parameters' ReverseConstraintSet beside the getters (parameters.jl:341-534)
            dp, rev = e.params_reverse_k(dl[None, None], self.param_terms, self.nparam, want_rev=True)
            out = np.asarray(rev)[0, 0]
            self.back_param_cache = np.asarray(dp)[0, 0]
        else:
            out = np.asarray(e.reverse(dl[None]))[0]
            self.back_param_cache = None
        n, m = self.n, self.G.shape[0]
        self.back_grad_cache = (out[:n], out[n:n + m], out[n + m:])
        self.diff_time = time.perf_counter() - t0

    def forward_differentiate(self):
        import time
        t0 = time.perf_counter()
        e = self._ensure()
        n, m, p = self.n, self.G.shape[0], self.A.shape[0]
        dQ, dq = (None, None) if self.input_objective is None else self.input_objective
        dG = np.zeros((m, n))
        dh = np.zeros(m)
        for r, (c, k) in self.input_le.items():
            dG[r] = c
            dh[r] = -k
        dA = np.zeros((p, n))
        db = np.zeros(p)
        for r, (c, k) in self.input_eq.items():
            dA[r] = c
            db[r] = -k
        functions = self.input_objective is not None or self.input_le or self.input_eq
        if functions or not self.input_dp:
            out = np.asarray(e.forward(
                None if dQ is None else np.asarray(dQ, float)[None],
                None if dq is None else np.asarray(dq, float)[None],
                dG[None] if m else None, dh[None] if m else None,
                dA[None] if p else None, db[None] if p else None))[0]
        else:
            out = np.zeros(n + m + p)
        if self.input_dp:   # the parameters' tangents on top of the functions' (parameters.jl:91-300): the
            dp = np.zeros((1, 1, self.nparam))   # solve is linear in the right-hand side, so the two solutions add
            for par, v in self.input_dp.items():
                dp[0, 0, par] = v
            out = out + np.asarray(e.params_forward_k(dp, self.param_terms))[0, 0]
        self.forw_grad_cache = (out[:n], out[n:n + m], out[n + m:])
        self.diff_time = time.perf_counter() - t0

    # ---- outputs -----------------------------------------------------------
    def forward_variable_primal(self, i):
        """``ForwardVariablePrimal`` (:299-305)."""
        return self.forw_grad_cache[0][i]

    def forward_constraint_dual(self, kind, row):
        """``ForwardConstraintDual``: the tangent of the MOI ``ConstraintDual`` of
        row ``row`` (minus the engine's dλ / dν)."""
        if kind == LE:
            return -self.forw_grad_cache[1][row]
        if kind == EQ:
            return -self.forw_grad_cache[2][row]
        raise ValueError(kind)

    def reverse_objective_function(self):
        """``ReverseObjectiveFunction`` (:448-458): (dq, dQ) with
        ``dq = ∇z`` and ``dQ = (∇z zᵀ + z ∇zᵀ)/2`` (materialised)."""
        dz = self.back_grad_cache[0]
        z = self.x
        return dz.copy(), 0.5 * (np.outer(dz, z) + np.outer(z, dz))

    def reverse_constraint_function(self, kind, row):
        """``ReverseConstraintFunction`` (diff_opt.jl:475-481): (coefficients,
        constant) from ``_get_dA``/``_get_db`` (:307-314, :461-473)."""
        dz, dlam, dnu = self.back_grad_cache
        z = self.x
        if kind == LE:
            l = self._lam[row]
            return l * dlam[row] * z + l * dz, l * dlam[row]
        if kind == EQ:
            return dnu[row] * z + self._nu[row] * dz, dnu[row]
        raise ValueError(kind)

    def reverse_parameter(self, p):
        """``ReverseConstraintSet`` of ``ParameterRef(p)`` (parameters.jl:341-534)."""
        return float(self.back_param_cache[p])

    def differentiate_time_sec(self):
        return self.diff_time
