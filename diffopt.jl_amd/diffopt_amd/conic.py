"""ConicProgram back-end on the MI355X engine.

Mirrors ``DiffOpt.ConicProgram`` (reference ``src/ConicProgram/ConicProgram.jl``):

* ``ConicBatch`` — batched C-ABI handle: geometric form ``A x + b ∈ K`` in MOI
  convention (the diffcp sign flip is applied by the engine), cone table in
  ``ProductOfSets`` row order, primal ``x``, slack ``s``, dual ``y``.
* ``Model`` — single problem with the reference vocabulary:
  ``forward_differentiate`` (:257-334), ``reverse_differentiate`` (:336-394),
  ``ForwardVariablePrimal`` (:403-412), ``ReverseObjectiveFunction``
  (:396-401), ``ReverseConstraintFunction`` (``_get_dA``/``_get_db``
  :414-443), and MAX-sense handling of ``c`` (:206-208); with a term table,
  ``ForwardConstraintSet`` / ``ReverseConstraintSet`` of parameters
  (``src/parameters.jl``).
"""

import ctypes
import time

import numpy as np

from . import _lib
from ._arrays import Staged, colmajor, csc_args, csc_pack, csc_split, is_sparse, vector

ZEROS, NONNEG, NONPOS, SOC, PSD = (_lib.CONE_ZEROS, _lib.CONE_NONNEG, _lib.CONE_NONPOS,
                                   _lib.CONE_SOC, _lib.CONE_PSD_TRI)


class ConicBatch:
    def __init__(self, batch, n, cones, device=0, sparse=False):
        self.lib = _lib.load()
        self.cones = [(int(c), int(d)) for c, d in cones]
        self.batch, self.n = int(batch), int(n)
        self.m = sum(d for _, d in self.cones)
        h = ctypes.c_void_p()
        rc = self.lib.dopt_create(ctypes.byref(h), device, self.batch, self.n, self.m, 0,
                                  _lib.DOPT_KIND_CONIC)
        if rc != 0:
            raise _lib.EngineError(rc, "dopt_create failed (no HIP device?)")
        self.h = h
        self._mem = None
        self._keep = None
        # the sparse route (dopt_set_sparse): set_csc keeps A_moi sparse, LSQR matrix-free on it.
        # sparse=True: one workgroup per problem, PSD sides up to 64; sparse="split": the split
        # LSQR on the sparse A_moi (DOPT_SPARSE_SPLIT), PSD sides up to 4096
        self.sparse = False
        self.sparse_split = False
        if isinstance(sparse, str) or sparse:
            self.set_sparse(sparse)

    def set_sparse(self, sparse):
        """Switch the handle's route (``False``, ``True`` or ``"split"``); the model is
        dropped and has to be set again."""
        if isinstance(sparse, str) and sparse != "split":
            raise ValueError(f'sparse={sparse!r}: expected False, True or "split"')
        mode = _lib.DOPT_SPARSE_SPLIT if sparse == "split" else 1 if sparse else 0
        _lib.check(self.lib.dopt_set_sparse(self.h, mode), self.h)
        self.sparse = mode != 0
        self.sparse_split = mode == _lib.DOPT_SPARSE_SPLIT

    def close(self):
        if getattr(self, "h", None):
            self.lib.dopt_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

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
    def N(self):
        return self.n + self.m + 1

    def set(self, A, b, c, x, s, y):
        """``A``: (B, m, n) MOI coefficients; ``c`` already sign-adjusted for MAX."""
        B, n, m = self.batch, self.n, self.m
        self._own_csc = None
        st = self._stage([A, b, c, x, s, y])
        args = [colmajor(A, (B, m, n)), vector(b, (B, m)), vector(c, (B, n)),
                vector(x, (B, n)), vector(s, (B, m)), vector(y, (B, m))]
        self._keep = args
        desc = np.array([v for cd in self.cones for v in cd], dtype=np.int32)
        rc = self.lib.dopt_conic_set(self.h, *[st.ptr(a) for a in args],
                                     desc.ctypes.data if desc.size else None, len(self.cones))
        _lib.check(rc, self.h)

    def set_csc(self, A, b, c, x, s, y):
        """``set`` with ``A`` (MOI coefficients, m × n) as scipy.sparse — one per
        problem or one shared — passed as Julia CSC arrays (Int64, 1-based) to
        dopt_conic_set_csc, which densifies on the device.  Host mode."""
        import scipy.sparse as sp
        B, n, m = self.batch, self.n, self.m
        mats = [A] * B if sp.issparse(A) else list(A)
        cps, rvs, nzs, off = [], [], [], 0
        for M in mats:
            M = sp.csc_matrix(M)
            if M.shape != (m, n):
                raise ValueError(f"sparse A of shape {M.shape}, expected {(m, n)}")
            cps.append(M.indptr.astype(np.int64) + off + 1)
            rvs.append(M.indices.astype(np.int64) + 1)
            nzs.append(M.data.astype(np.float64))
            off += M.nnz
        cp = np.ascontiguousarray(np.concatenate(cps))
        rv = np.ascontiguousarray(np.concatenate(rvs))
        nz = np.ascontiguousarray(np.concatenate(nzs))
        self._own_csc = None
        st = self._stage([b, c, x, s, y])
        if st.mem != _lib.DOPT_MEM_HOST:
            raise TypeError("set_csc takes host (numpy / scipy) arrays")
        vecs = [vector(b, (B, m)), vector(c, (B, n)), vector(x, (B, n)), vector(s, (B, m)),
                vector(y, (B, m))]
        desc = np.array([v for cd in self.cones for v in cd], dtype=np.int32)
        rc = self.lib.dopt_conic_set_csc(self.h, cp.ctypes.data, rv.ctypes.data if off else None,
                                         nz.ctypes.data if off else None, off,
                                         *[st.ptr(v) for v in vecs],
                                         desc.ctypes.data if desc.size else None, len(self.cones))
        _lib.check(rc, self.h)
        self._own_csc = (cp, rv, nz, off)   # the colptr reverse_grads_at(pattern=None) splits its values by

    def factor(self):
        _lib.check(self.lib.dopt_conic_factor(self.h), self.h)

    def forward(self, dA=None, db=None, dc=None):
        """Returns (out (B, N) = [du | dv | dw], dx (B, n) = ForwardVariablePrimal).
        ``dA``: dense (B, m, n), or scipy-sparse (one shared matrix or a list of
        B) with its own pattern — then dopt_conic_forward_csc, no dense m × n
        array anywhere."""
        B, n, m = self.batch, self.n, self.m
        if is_sparse(dA):
            return self._forward_csc(dA, db, dc)
        st = self._stage([dA, db, dc])
        dev = st.mem == _lib.DOPT_MEM_DEVICE
        args = [colmajor(dA, (B, m, n)) if dA is not None else None,
                vector(db, (B, m)) if db is not None else None,
                vector(dc, (B, n)) if dc is not None else None]
        out = Staged.empty((B, self.N), dev)
        dx = Staged.empty((B, n), dev)
        rc = self.lib.dopt_conic_forward(self.h, *[st.ptr(a) for a in args], st.ptr(out), st.ptr(dx))
        _lib.check(rc, self.h)
        return out, dx

    def _forward_csc(self, dA, db, dc):
        B, n, m = self.batch, self.n, self.m
        st = self._stage([db, dc])
        if st.mem != _lib.DOPT_MEM_HOST:
            raise TypeError("a scipy-sparse dA goes with host (numpy) db / dc")
        packed = csc_pack(dA, B, (m, n))
        vecs = [vector(db, (B, m)) if db is not None else None,
                vector(dc, (B, n)) if dc is not None else None]
        out = Staged.empty((B, self.N), False)
        dx = Staged.empty((B, n), False)
        rc = self.lib.dopt_conic_forward_csc(self.h, *csc_args(packed), *[st.ptr(a) for a in vecs],
                                             st.ptr(out), st.ptr(dx))
        _lib.check(rc, self.h)
        return out, dx

    def reverse_grads_at(self, g, pattern=None):
        """The reverse gradient dA read at the entries of a pattern
        (dopt_conic_reverse_grads_csc; the reference's lazy ``_get_dA``):
        ``g`` (B, N) is a reverse call's first output; ``pattern`` is one
        scipy-sparse m × n matrix or a list of B (only the patterns are used),
        ``None`` = the pattern the handle got from ``set_csc`` (sparse-route
        handles).  Returns a list of B value arrays, problem b's aligned with
        its pattern's canonical CSC order (duplicates summed, rows sorted):
        ``values[k] = g[n+i]·x[j] − vp[i]·g[j]`` for entry k = (i, j)."""
        B, n, m = self.batch, self.n, self.m
        st = self._stage([g])
        if st.mem != _lib.DOPT_MEM_HOST:
            raise TypeError("reverse_grads_at takes a host (numpy) g")
        gv = vector(g, (B, self.N))
        if pattern is None:
            cnt = getattr(self, "_own_csc", None)
            if cnt is None:
                raise _lib.EngineError(-1, "reverse_grads_at(pattern=None) needs a model given by set_csc")
            packed, args = cnt, [None, None, 0]
        else:
            packed = csc_pack(pattern, B, (m, n))
            args = csc_args(packed, values=False)
        out = np.zeros(max(packed[3], 1), dtype=np.float64)
        rc = self.lib.dopt_conic_reverse_grads_csc(self.h, st.ptr(gv), *args, out.ctypes.data)
        _lib.check(rc, self.h)
        return csc_split(out, packed, B, n)

    def reverse(self, dx, want_dA=True):
        """Returns (g (B, N), dA (B, m, n) | None, db (B, m), dc (B, n))."""
        B, n, m = self.batch, self.n, self.m
        st = self._stage([dx])
        dev = st.mem == _lib.DOPT_MEM_DEVICE
        d = vector(dx, (B, n))
        g = Staged.empty((B, self.N), dev)
        dA = Staged.empty((B, n, m), dev) if want_dA else None   # column-major (m×n)
        db = Staged.empty((B, m), dev)
        dc = Staged.empty((B, n), dev)
        rc = self.lib.dopt_conic_reverse(self.h, st.ptr(d), st.ptr(g), st.ptr(dA), st.ptr(db),
                                         st.ptr(dc))
        _lib.check(rc, self.h)
        if dA is not None:
            dA = dA.transpose(0, 2, 1) if not dev else dA.transpose(1, 2)
        return g, dA, db, dc

    def forward_reverse(self, dx, dA=None, db=None, dc=None, want_dA=True):
        """Both directions in one call, the two LSQR runs co-iterated
        (dopt_conic_forward_reverse): ((out, dx_fwd), (g, dA, db, dc)) as
        ``forward`` / ``reverse`` return them, bit-identical to those calls.
        A scipy-sparse ``dA`` (see ``forward``) goes to
        dopt_conic_forward_reverse_csc, which has no dense gradient: the
        reverse tuple's dA is ``None`` (read it with ``reverse_grads_at``)."""
        B, n, m = self.batch, self.n, self.m
        if is_sparse(dA):
            st = self._stage([db, dc, dx])
            if st.mem != _lib.DOPT_MEM_HOST:
                raise TypeError("a scipy-sparse dA goes with host (numpy) db / dc / dx")
            packed = csc_pack(dA, B, (m, n))
            vecs = [vector(db, (B, m)) if db is not None else None,
                    vector(dc, (B, n)) if dc is not None else None, vector(dx, (B, n))]
            out, fdx, g = (Staged.empty(s_, False) for s_ in ((B, self.N), (B, n), (B, self.N)))
            rb, rc_ = Staged.empty((B, m), False), Staged.empty((B, n), False)
            rc = self.lib.dopt_conic_forward_reverse_csc(self.h, *csc_args(packed), *[st.ptr(a) for a in vecs],
                                                         st.ptr(out), st.ptr(fdx), st.ptr(g), st.ptr(rb),
                                                         st.ptr(rc_))
            _lib.check(rc, self.h)
            return (out, fdx), (g, None, rb, rc_)
        st = self._stage([dA, db, dc, dx])
        dev = st.mem == _lib.DOPT_MEM_DEVICE
        args = [colmajor(dA, (B, m, n)) if dA is not None else None,
                vector(db, (B, m)) if db is not None else None,
                vector(dc, (B, n)) if dc is not None else None,
                vector(dx, (B, n))]
        out = Staged.empty((B, self.N), dev)
        fdx = Staged.empty((B, n), dev)
        g = Staged.empty((B, self.N), dev)
        rA = Staged.empty((B, n, m), dev) if want_dA else None
        rb = Staged.empty((B, m), dev)
        rc_ = Staged.empty((B, n), dev)
        rc = self.lib.dopt_conic_forward_reverse(self.h, *[st.ptr(a) for a in args], st.ptr(out), st.ptr(fdx),
                                                 st.ptr(g), st.ptr(rA), st.ptr(rb), st.ptr(rc_))
        _lib.check(rc, self.h)
        if rA is not None:
            rA = rA.transpose(0, 2, 1) if not dev else rA.transpose(1, 2)
        return (out, fdx), (g, rA, rb, rc_)

    def reverse_k(self, dx, want_dA=True):
        """k seeds per solved cone program in one call (dopt_conic_reverse_k):
        dx (k, B, n) → (g (k, B, N), dA (k, B, m, n) | None, db (k, B, m),
        dc (k, B, n)); seed j bit-identical to ``reverse(dx[j])``.  On the
        dense persistent route groups of seeds share each sweep over A."""
        k = int(dx.shape[0])
        B, n, m = self.batch, self.n, self.m
        st = self._stage([dx])
        dev = st.mem == _lib.DOPT_MEM_DEVICE
        d = vector(dx, (k, B, n))
        g = Staged.empty((k, B, self.N), dev)
        dA = Staged.empty((k, B, n, m), dev) if want_dA else None   # column-major (m×n)
        db = Staged.empty((k, B, m), dev)
        dc = Staged.empty((k, B, n), dev)
        rc = self.lib.dopt_conic_reverse_k(self.h, k, st.ptr(d), st.ptr(g), st.ptr(dA), st.ptr(db),
                                           st.ptr(dc))
        _lib.check(rc, self.h)
        if dA is not None:
            dA = dA.transpose(0, 1, 3, 2) if not dev else dA.transpose(2, 3)
        return g, dA, db, dc

    def forward_k(self, dA=None, db=None, dc=None):
        """k tangents per problem (dopt_conic_forward_k): each given tangent
        has a leading seed axis (k, B, …) → (out (k, B, N), dx (k, B, n));
        seed j bit-identical to ``forward`` on its tangents."""
        given = [a for a in (dA, db, dc) if a is not None]
        if not given:
            raise ValueError("forward_k needs at least one tangent")
        k = int(given[0].shape[0])
        B, n, m = self.batch, self.n, self.m
        st = self._stage([dA, db, dc])
        dev = st.mem == _lib.DOPT_MEM_DEVICE
        kb = k * B
        args = [colmajor(dA, (kb, m, n)) if dA is not None else None,
                vector(db, (kb, m)) if db is not None else None,
                vector(dc, (kb, n)) if dc is not None else None]
        out = Staged.empty((k, B, self.N), dev)
        dx = Staged.empty((k, B, n), dev)
        rc = self.lib.dopt_conic_forward_k(self.h, k, *[st.ptr(a) for a in args], st.ptr(out), st.ptr(dx))
        _lib.check(rc, self.h)
        return out, dx

    def lsqr_stats_k(self, k):
        """(istop, iterations) per seed of the last ``reverse_k`` /
        ``forward_k`` call with this k: dict of (k, B) arrays."""
        k, B = int(k), self.batch
        buf = np.zeros(2 * B * max(k, 1), dtype=np.int32)
        _lib.check(self.lib.dopt_conic_lsqr_stats_k(self.h, k, buf.ctypes.data), self.h)
        buf = buf.reshape(k, 2, B)
        return {"istop": buf[:, 0, :], "iterations": buf[:, 1, :]}

    # ---- parameters (ParametricOptInterface glue, reference src/parameters.jl)
    @staticmethod
    def _terms(terms):
        """terms: iterable of (param, kind, index, coef) — kinds 0 constraint row
        (ProductOfSets order), 2 objective, 3 objective parameter×variable
        (index = v); kind 1 is the QP's and is refused here."""
        t = list(terms)
        par = np.ascontiguousarray([int(x[0]) for x in t], dtype=np.int32)
        kind = np.ascontiguousarray([int(x[1]) for x in t], dtype=np.int32)
        idx = np.ascontiguousarray([int(x[2]) for x in t], dtype=np.int32)
        coef = np.ascontiguousarray([float(x[3]) for x in t], dtype=np.float64)
        return len(t), par, kind, idx, coef

    def params_forward(self, dp, terms):
        """Parameter tangents dp (B, nparam) → (db (B, m), dc (B, n)), ready for
        ``forward(None, db, dc)`` — dopt_conic_params_forward.  db is NOT
        negated (the conic ``_fill`` runs with ``S -> false``)."""
        B, n, m = self.batch, self.n, self.m
        nparam = int(dp.shape[1])
        nt, par, kind, idx, coef = self._terms(terms)
        st = self._stage([dp])
        d = vector(dp, (B, nparam))
        dev = st.mem == _lib.DOPT_MEM_DEVICE
        db, dc = Staged.empty((B, m), dev), Staged.empty((B, n), dev)
        p = Staged.ptr
        rc = self.lib.dopt_conic_params_forward(self.h, st.ptr(d) if nparam else None, nparam, nt, p(par), p(kind),
                                                p(idx), p(coef), st.ptr(db) if m else None,
                                                st.ptr(dc) if n else None)
        _lib.check(rc, self.h)
        return db, dc

    def params_reverse(self, g, terms, nparam):
        """ReverseConstraintSet of every parameter of every problem, (B, nparam),
        from a reverse call's ``g`` (B, N) — dopt_conic_params_reverse."""
        B = self.batch
        nparam = int(nparam)
        nt, par, kind, idx, coef = self._terms(terms)
        st = self._stage([g])
        gv = vector(g, (B, self.N))
        out = Staged.empty((B, nparam), st.mem == _lib.DOPT_MEM_DEVICE)
        p = Staged.ptr
        rc = self.lib.dopt_conic_params_reverse(self.h, st.ptr(gv), nparam, nt, p(par), p(kind), p(idx), p(coef),
                                                st.ptr(out) if nparam else None)
        _lib.check(rc, self.h)
        return out

    def params_jacobian(self, terms, nparam, mode, device=False):
        """dx/dp of every problem by unit seeds (dopt_conic_params_jacobian) →
        (J (B, n, nparam), stats).  ``mode`` 0 (or "forward"): column j is
        ``forward(None, *params_forward(e_j))``'s dx; 1 (or "reverse"): row i is
        ``params_reverse(reverse(e_i).g)``; each bit-identical to those calls.
        The reference's two directions are not adjoint (its reverse solve runs
        LSQR on M, not Mᵀ), so the two Jacobians differ and there is no mode
        that chooses between them.  stats: dict of (K, B) arrays "istop" and
        "iterations", K = nparam (mode 0) or n (mode 1), always numpy.  J is a
        numpy array, or with ``device`` a torch CUDA tensor written in place by
        the kernels (on torch's current stream)."""
        mode = {"forward": 0, "reverse": 1}.get(mode, mode)
        B, n = self.batch, self.n
        nparam = int(nparam)
        nt, par, kind, idx, coef = self._terms(terms)
        K = n if mode == 1 else nparam
        J = Staged.empty((K, B, nparam if mode == 1 else n), device)
        self._stage([J] if device else [])   # the memory mode (and torch's stream) follow the output
        buf = np.zeros(2 * B * max(K, 1), dtype=np.int32)
        p = Staged.ptr
        rc = self.lib.dopt_conic_params_jacobian(self.h, int(mode), nparam, nt, p(par), p(kind), p(idx), p(coef),
                                                 p(J) if K and B and n else None, buf.ctypes.data)
        _lib.check(rc, self.h)
        buf = buf.reshape(max(K, 1), 2, B)[:K]
        if device:
            J = J.permute(1, 2, 0) if mode == 0 else J.permute(1, 0, 2)
        else:
            J = J.transpose(1, 2, 0) if mode == 0 else J.transpose(1, 0, 2)
        return J, {"istop": buf[:, 0, :], "iterations": buf[:, 1, :]}

    def set_maxiter(self, maxiter):
        """Cap LSQR at ``maxiter`` iterations (0: the reference's default
        max(size(M))) — dopt_conic_set_maxiter."""
        _lib.check(self.lib.dopt_conic_set_maxiter(self.h, int(maxiter)), self.h)

    def lsqr_stats(self):
        """(istop, iterations) of the last run and, after ``forward_reverse``,
        of its forward run: dict of (B,) arrays."""
        buf = np.zeros(4 * self.batch, dtype=np.int32)
        _lib.check(self.lib.dopt_conic_lsqr_stats(self.h, buf.ctypes.data), self.h)
        B = self.batch
        return {"istop": buf[:B], "iterations": buf[B:2 * B], "fwd_istop": buf[2 * B:3 * B],
                "fwd_iterations": buf[3 * B:]}

    def lsqr_norms(self):
        """LSQR's terminal estimates (rnorm, arnorm, xnorm, anorm) of the last
        run and, after ``forward_reverse``, of its forward run: dict of (B, 4)
        arrays under "last" and "fwd"."""
        buf = np.zeros(8 * self.batch, dtype=np.float64)
        _lib.check(self.lib.dopt_conic_lsqr_norms(self.h, buf.ctypes.data), self.h)
        B = self.batch
        return {"last": buf[:4 * B].reshape(B, 4), "fwd": buf[4 * B:].reshape(B, 4)}

    def info(self):
        buf = np.zeros(self.batch, dtype=np.int32)
        _lib.check(self.lib.dopt_get_info(self.h, buf.ctypes.data), self.h)
        return buf

    def iterations(self):
        buf = np.zeros(self.batch, dtype=np.int32)
        _lib.check(self.lib.dopt_get_system_size(self.h, buf.ctypes.data), self.h)
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
        return _lib.phase_times(self.lib, self.h)


class Model:
    """Single-problem ``DiffOpt.ConicProgram.Model`` on the engine."""

    def __init__(self, device=0):
        self.device = device
        self.empty()

    def empty(self):
        self.A = self.b = self.c = None
        self.cones = []
        self.max_sense = False
        self.x = self.s = self.y = None
        self._engine = None
        self.forw_grad_cache = None
        self.back_grad_cache = None
        self.diff_time = float("nan")
        self.input_dx = {}
        self.input_objective = None
        self.input_constraints = {}   # cone index -> (coeffs (dim×n), constants (dim))
        self.param_terms, self.nparam = [], 0
        self.input_dp = {}            # parameter -> ForwardConstraintSet direction
        self.back_param_cache = None

    def set_problem(self, A, b, c, cones, max_sense=False, param_terms=(), nparam=0):
        """``param_terms``: the parametric terms (param, kind, index, coef) of
        the problem's ``nparam`` parameters (``ConicBatch._terms``: kind 0 a
        constraint row in ProductOfSets order, 2 the objective, 3 objective
        parameter×variable)."""
        self.A = np.asarray(A, dtype=np.float64)
        self.b = np.asarray(b, dtype=np.float64)
        self.c = np.asarray(c, dtype=np.float64)
        self.cones = [(int(k), int(d)) for k, d in cones]
        self.max_sense = bool(max_sense)
        self.param_terms = [tuple(t) for t in param_terms]
        self.nparam = int(nparam)
        self.input_dp = {}
        self._engine = None

    def rows(self, ci):
        o = sum(d for _, d in self.cones[:ci])
        return np.arange(o, o + self.cones[ci][1])

    def set_variable_primal_start(self, x):
        self.x = np.asarray(x, dtype=np.float64)
        self._engine = None

    def set_constraint_primal_start(self, s):
        self.s = np.asarray(s, dtype=np.float64)
        self._engine = None

    def set_constraint_dual_start(self, y):
        self.y = np.asarray(y, dtype=np.float64)
        self._engine = None

    def set_reverse_variable_primal(self, i, value):
        self.input_dx[int(i)] = float(value)

    def set_forward_objective_function(self, dc):
        self.input_objective = np.asarray(dc, dtype=np.float64)

    def set_forward_constraint_function(self, ci, coeffs, constants):
        self.input_constraints[int(ci)] = (np.asarray(coeffs, float), np.asarray(constants, float))

    def set_forward_parameter(self, p, value):
        """``ForwardConstraintSet`` of ``ParameterRef(p)``: the direction ``Parameter(value)``."""
        if not 0 <= int(p) < self.nparam:
            raise IndexError(f"parameter {p} of {self.nparam}")
        self.input_dp[int(p)] = float(value)

    def _ensure(self):
        m = self.A.shape[0]
        if self.y is None or np.any(np.isnan(self.y)) or len(self.y) < m:
            raise ValueError("Some constraints are missing a value for the "
                             "`ConstraintDualStart` attribute.")
        if self.s is None or np.any(np.isnan(self.s)) or len(self.s) < m:
            raise ValueError("Some constraints are missing a value for the "
                             "`ConstraintPrimalStart` attribute.")
        if self._engine is None:
            e = ConicBatch(1, self.A.shape[1], self.cones, self.device)
            c = -self.c if self.max_sense else self.c
            e.set(self.A[None], self.b[None], c[None], self.x[None], self.s[None], self.y[None])
            self._engine = e
        return self._engine

    def forward_differentiate(self):
        t0 = time.perf_counter()
        e = self._ensure()
        m, n = self.A.shape
        dA = np.zeros((m, n))
        db = np.zeros(m)
        for ci, (cf, k) in self.input_constraints.items():
            r = self.rows(ci)
            dA[r] = cf
            db[r] = k
        dc = np.zeros(n) if self.input_objective is None else self.input_objective
        if self.input_dp:   # the parameters' tangents on top of the functions' (parameters.jl:120-145, :226-275)
            dp = np.zeros((1, self.nparam))
            for p, v in self.input_dp.items():
                dp[0, p] = v
            pb, pc = e.params_forward(dp, self.param_terms)
            db, dc = db + np.asarray(pb)[0], dc + np.asarray(pc)[0]
        out, dx = e.forward(dA[None], db[None], dc[None])
        self.forw_grad_cache = (np.asarray(out)[0], np.asarray(dx)[0])
        self.diff_time = time.perf_counter() - t0

    def reverse_differentiate(self):
        t0 = time.perf_counter()
        e = self._ensure()
        dx = np.zeros(self.A.shape[1])
        for i, v in self.input_dx.items():
            dx[i] = v
        g, dA, db, dc = e.reverse(dx[None])
        self.back_grad_cache = tuple(np.asarray(a)[0] for a in (g, dA, db, dc))
        self.back_param_cache = (np.asarray(e.params_reverse(g, self.param_terms, self.nparam))[0]
                                 if self.nparam else None)
        self.diff_time = time.perf_counter() - t0

    def forward_variable_primal(self, i):
        return self.forw_grad_cache[1][i]

    def reverse_objective_function(self):
        return self.back_grad_cache[3].copy()

    def reverse_constraint_function(self, ci):
        """(dA rows, db entries) for constraint ``ci`` (``_get_dA``/``_get_db``)."""
        r = self.rows(ci)
        _, dA, db, _ = self.back_grad_cache
        return dA[r], db[r]

    def reverse_parameter(self, p):
        """``ReverseConstraintSet`` of ``ParameterRef(p)`` (parameters.jl:365-388, :463-509)."""
        return float(self.back_param_cache[p])

    def differentiate_time_sec(self):
        return self.diff_time
