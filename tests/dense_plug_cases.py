"""Dense matrices for the arbitrary-matrix entry of the engine — the
``LinearAlgebraSolver`` plug point (dopt_lhs_solve / dopt_lhs_resolve,
``MI355XSolver``) and KKT mode (dopt_nlp_set_kkt / _factor / _kkt_solve).
test_dense_plug_cases_cpu.py pins on the CPU what each case is,
test_dense_plug_gpu.py runs them through the no-pivot LU (qp_nopiv.hip), the
partial-pivoting blocked LU (qp_blocked.hip), the singular-pivot verdict
(nlp.hip) and the multi-RHS sweep (qp_multi.hip).

Here the test, not a problem generator, decides the size, the pivot pattern,
the accept / reject verdict of the no-pivot LU and the exact solution.

Every matrix has **small-integer entries** and every right-hand side is
``b = M·x*`` with integer ``x*`` in [−8, 8]: each product and each partial sum
is an integer far below 2^53, so ``b`` is exact in Float64 in any summation
order and ``x*`` is the exact solution (``exact_rhs`` checks it against the
long-double product).

Families (seeded; ``matrix(family, rows, seed)``):

* ``dom``      entries in [−3, 3], diagonal = Σ|off-diagonal| + 1..3 with a
               random sign: nonsymmetric, strictly row-dominant.  The no-pivot
               LU accepts it.
* ``perm``     a ``dom`` matrix with its rows randomly permuted.
* ``antidiag`` a ``dom`` matrix with its rows reversed: every pivot comes from
               the far end, so every swap crosses blocks and the panel.
* ``gauss``    integers in [−9, 9]: real partial pivoting.
               These three are regular and refused by the no-pivot rule, at
               every size from 2 rows up (a 1 × 1 matrix has no multiplier):
               a draw that is not is passed over (``_draw``).
* ``spike(rows, i, j, c)``  I + c·e_i·e_jᵀ, i > j: its only multiplier is c.
* ``zero_col(family, rows, seed, j)``  column j zeroed: exactly singular, and
               with partial pivoting the zero pivot appears at column j.
* ``tiny_col(family, rows, seed, j)``  column j scaled by 2^-80: no pivot is
               zero, but u_jj falls below the engine's rank-revealing threshold.
* ``saddle(nw, nc, zero_row, seed)``  [[W, Jᵀ], [J, 0]], W symmetric integer
               and strongly dominant, row ``zero_row`` of J all zero: exactly
               singular in any elimination order.

Everything is built once per process (lru_cache) and returned read-only."""

import functools

import numpy as np

EPS = float(np.finfo(np.float64).eps)
NOPIV_LMAX = 10.0        # dopt_internal.h
NOPIV_GROWTH = 1e8       # dopt_internal.h
PIVOT_MAX = 1536         # dopt_internal.h
MKC = 16                 # qp_multi.hip: right-hand sides per workgroup
LHS_PACK_MAX = 1 << 20   # abi.hip: bytes of M and the sides packed into one pinned copy
LD = np.longdouble

FAMILIES = ("dom", "perm", "antidiag", "gauss")

# ---- the cases of test_dense_plug_gpu.py -------------------------------------
BLOCK_ROWS = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 193, 257)
# qp_multi.hip: lds_v = Np·132 bytes (Np = rows rounded up to 32) — 480: below
# the 64 KB default; 481 (Np 512): the opt-in; 1152: 148.5 KB, the last chunk in
# LDS; 1153 (Np 1184): the global workspace.  512 / 1024 / 1536: the
# partial-pivoting panel at 512 threads × 1, 2, 3 rows.
STORAGE_ROWS = (480, 481, 512, 513, 1024, 1025, 1152, 1153, 1536)
STORAGE_FAMILIES = ("dom", "gauss")
PACK_ROWS = (361, 362)   # batch 1, k = 1: (rows² + rows)·8 bytes either side of LHS_PACK_MAX
CHUNK_ROWS = 97
CHUNK_K = (1, 2, 15, 16, 17, 33)
CHUNK_BATCHES = (3, 8)
SPIKE_ROWS = 130         # Np 160: 64-column steps 0 and 64, a 32-wide tail at 128
SPIKE_SITES = ((1, 0), (31, 0), (32, 0), (63, 31), (64, 0), (95, 64), (129, 0), (129, 128), (128, 96))
SPIKE_C = (10.0, -10.0, 10.5, -10.5)
SINGULAR_ROWS = (65, 97)
SADDLE_ROWS = (33, 65, 97)


def singular_columns(rows):
    return tuple(dict.fromkeys((0, 31, 32, 63, 64, rows - 1)))


def _rng(*key):
    return np.random.default_rng([20251021, *[int(k) for k in key]])


def _frozen(a):
    a.setflags(write=False)
    return a


def _dom_draw(rows, seed, attempt=0):
    r = _rng(1, rows, seed, *([attempt] if attempt else []))
    M = r.integers(-3, 4, size=(rows, rows)).astype(np.float64)
    np.fill_diagonal(M, 0.0)
    d = np.abs(M).sum(axis=1) + r.integers(1, 4, size=rows)
    M[np.arange(rows), np.arange(rows)] = d * r.choice([-1.0, 1.0], size=rows)
    return M


def _refused_and_regular(M):
    """What makes a matrix a case of ``perm`` / ``antidiag`` / ``gauss``: the
    no-pivot rule refuses it, and partial pivoting finds no small pivot.  A 1 × 1
    matrix has no multiplier to refuse: there regular is all that can be asked."""
    return first_singular_column(M) == 0 and (M.shape[0] == 1 or not nopiv_accepts(M))


def _draw(make, rows):
    """The first draw ``make(attempt)`` that belongs to its family.  Above 8 rows
    that is attempt 0 unchecked (the CPU test pins those draws); at 2 rows entries
    this small give no multiplier above 10, so only a zero first pivot is refused
    and some draws have to be passed over."""
    for attempt in range(1000):
        M = make(attempt)
        if rows > 8 or _refused_and_regular(M):
            return _frozen(M)
    raise AssertionError("no draw of the family")


@functools.lru_cache(maxsize=None)
def dom(rows, seed=0):
    return _frozen(_dom_draw(rows, seed))


@functools.lru_cache(maxsize=None)
def perm(rows, seed=0):
    def make(attempt):
        p = _rng(2, rows, seed, *([attempt] if attempt else [])).permutation(rows)
        return _dom_draw(rows, seed, attempt)[p]
    return _draw(make, rows)


@functools.lru_cache(maxsize=None)
def antidiag(rows, seed=0):
    return _draw(lambda attempt: _dom_draw(rows, seed, attempt)[::-1].copy(), rows)


@functools.lru_cache(maxsize=None)
def gauss(rows, seed=0):
    return _draw(lambda attempt: _rng(3, rows, seed, attempt).integers(-9, 10, size=(rows, rows)).astype(np.float64),
                 rows)


def matrix(family, rows, seed=0):
    return {"dom": dom, "perm": perm, "antidiag": antidiag, "gauss": gauss}[family](rows, seed)


@functools.lru_cache(maxsize=None)
def spike(rows, i, j, c):
    assert i > j
    M = np.eye(rows)
    M[i, j] = c
    return _frozen(M)


@functools.lru_cache(maxsize=None)
def zero_col(family, rows, seed, j):
    M = matrix(family, rows, seed).copy()
    M[:, j] = 0.0
    return _frozen(M)


@functools.lru_cache(maxsize=None)
def tiny_col(family, rows, seed, j):
    """Column j scaled by 2^-80 (exact): every elimination order, multiplier
    and pivot choice is that of the unscaled matrix, only u_jj is 2^-80 times
    its regular value — not zero, so no LU meets a zero pivot, yet far below
    rows·ε·max|M|: the verdict is the rank-revealing test's alone (nlp.hip)."""
    M = matrix(family, rows, seed).copy()
    M[:, j] *= 2.0 ** -80
    return _frozen(M)


@functools.lru_cache(maxsize=None)
def saddle(nw, nc, zero_row, seed=0):
    r = _rng(4, nw, nc, zero_row, seed)
    W = np.triu(r.integers(-3, 4, size=(nw, nw)).astype(np.float64), 1)
    W = W + W.T
    W[np.arange(nw), np.arange(nw)] = 2.0 * np.abs(W).sum(axis=1) + r.integers(1, 4, size=nw)
    J = r.integers(-3, 4, size=(nc, nw)).astype(np.float64)
    J[zero_row] = 0.0
    M = np.zeros((nw + nc, nw + nc))
    M[:nw, :nw] = W
    M[:nw, nw:] = J.T
    M[nw:, :nw] = J
    return _frozen(M)


def saddle_split(rows):
    """(nw, nc) of the saddle case with `rows` rows: a third are constraints."""
    nc = max(rows // 3, 2)
    return rows - nc, nc


def saddle_corrected(M, nw, nc, corr, st=1e-6):
    """M + corr·st·D, D = +1 except −1 on the constraint rows
    (NonLinearProgram.jl:356-381)."""
    d = np.ones(nw + nc)
    d[nw:] = -1.0
    return M + corr * st * np.diag(d)


@functools.lru_cache(maxsize=None)
def solution(rows, k, seed=0):
    """x* (rows, k): integers in [−8, 8], no column all zero."""
    X = _rng(5, rows, k, seed).integers(-8, 9, size=(rows, k)).astype(np.float64)
    X[0, np.abs(X).sum(axis=0) == 0] = 1.0
    return _frozen(X)


def rhs(M, k, seed=0, trans=False):
    """(B, X*) with B = M·X* (Mᵀ·X* if `trans`), (rows, k) each; B is exact."""
    X = solution(M.shape[0], k, seed)
    return (M.T if trans else M) @ X, X


def exact_rhs(M, k, seed=0, trans=False):
    """True when the Float64 product of ``rhs`` equals the long-double one."""
    B, X = rhs(M, k, seed, trans)
    A = M.T if trans else M
    return bool(np.array_equal(B.astype(LD), A.astype(LD) @ X.astype(LD)))


# ---- reference predicates (plain loops over the columns) --------------------
def nopiv_scan(M, nb=64):
    """Gaussian elimination without pivoting under the documented acceptance
    rule (include/diffopt_mi355x.h, dopt_internal.h): every pivot non-zero,
    every |l_ij| ≤ NOPIV_LMAX, every entry of U within NOPIV_GROWTH·max|M|.
    Column by column inside a panel of `nb` columns, then the panel's rows of
    U and one product for the trailing matrix (nb = 1: the textbook loop; the
    CPU test holds the two to the same verdicts).  Stops at the first panel
    column that breaks the rule.  Returns a dict: ``accept``; ``lmax`` the
    largest |l| formed, the breaking column's included (∞ at a zero pivot);
    ``umax`` the largest |u| over the bound; ``column`` where it stopped."""
    A = np.array(M, dtype=np.float64)
    n = A.shape[0]
    bound = NOPIV_GROWTH * np.abs(A).max()
    lmax = umax = 0.0
    for j0 in range(0, n, nb):
        j1 = min(j0 + nb, n)
        for j in range(j0, j1):
            if A[j, j] == 0.0 or not np.isfinite(A[j, j]):
                return {"accept": False, "lmax": np.inf, "umax": umax, "column": j}
            if j + 1 < n:
                A[j + 1:, j] /= A[j, j]
                lmax = max(lmax, float(np.abs(A[j + 1:, j]).max()))
                if not lmax <= NOPIV_LMAX:
                    return {"accept": False, "lmax": lmax, "umax": umax, "column": j}
                A[j + 1:, j + 1:j1] -= np.outer(A[j + 1:, j], A[j, j + 1:j1])
        for j in range(j0, j1 - 1):   # U12 = L11⁻¹ A12
            A[j + 1:j1, j1:] -= np.outer(A[j + 1:j1, j], A[j, j1:])
        umax = max(umax, float(np.abs(np.triu(A[j0:j1, j0:])).max()) / bound)
        if not umax <= 1.0:
            return {"accept": False, "lmax": lmax, "umax": umax, "column": j0}
        A[j1:, j1:] -= A[j1:, j0:j1] @ A[j0:j1, j1:]
    return {"accept": True, "lmax": lmax, "umax": umax, "column": n}


def nopiv_accepts(M):
    return nopiv_scan(M)["accept"]


@functools.lru_cache(maxsize=None)
def accepts(family, rows, seed=0):
    """nopiv_accepts of a family's matrix (what lu_kind must report)."""
    return nopiv_accepts(matrix(family, rows, seed))


def decisive(scan):
    """The verdict of ``nopiv_scan`` does not hang on a rounding: an accepted
    matrix keeps every |l| below 9.99 (or has exactly-representable multipliers,
    the spikes) and U a decade inside the bound; a refused one has a zero pivot
    or a multiplier above 10.01 — 1e-3 away where an elimination's rounding
    moves a multiplier by 1e-13."""
    if scan["accept"]:
        return scan["lmax"] <= 9.99 and scan["umax"] <= 0.1
    return scan["lmax"] >= 10.01 and scan["umax"] <= 0.1


def pivots(M):
    """|u_ii| of a plain partial-pivoting LU (first largest entry wins ties)."""
    A = np.array(M, dtype=np.float64)
    n = A.shape[0]
    out = np.zeros(n)
    for j in range(n):
        p = j + int(np.argmax(np.abs(A[j:, j])))
        if p != j:
            A[[j, p]] = A[[p, j]]
        out[j] = abs(A[j, j])
        if A[j, j] != 0.0 and j + 1 < n:
            l = A[j + 1:, j] / A[j, j]
            A[j + 1:, j + 1:] -= np.outer(l, A[j, j + 1:])
            A[j + 1:, j] = 0.0
    return out


def first_singular_column(M):
    """1-based index of the first pivot of a plain partial-pivoting LU with
    |u_ii| ≤ rows·ε·max|M| (the engine's rank-revealing test, nlp.hip), or 0."""
    M = np.asarray(M, dtype=np.float64)
    n = M.shape[0]
    tol = n * EPS * np.abs(M).max()
    bad = np.flatnonzero(~(pivots(M) > tol))
    return int(bad[0]) + 1 if bad.size else 0


# ---- measures (long double) ---------------------------------------------------
def eta(M, x, b):
    """Normwise backward error ‖b − M x‖∞ / (‖M‖∞‖x‖∞ + ‖b‖∞)."""
    Ml, xl, bl = np.asarray(M).astype(LD), np.asarray(x).astype(LD), np.asarray(b).astype(LD)
    r = np.abs(bl - Ml @ xl).max()
    den = np.abs(Ml).sum(axis=1).max() * np.abs(xl).max() + np.abs(bl).max()
    return float(r / den)


def forward_error(x, xstar):
    """‖x − x*‖₂ / ‖x*‖₂."""
    xl, sl = np.asarray(x).astype(LD), np.asarray(xstar).astype(LD)
    return float(np.sqrt(((xl - sl) ** 2).sum()) / np.sqrt((sl ** 2).sum()))


def lapack_errors(A, B, X):
    """LAPACK on A·S = B — the yardstick: (η, forward error) per right-hand
    side (two arrays of k); `X` the exact solution, or None (no forward error)."""
    S = np.linalg.solve(A, B)
    k = B.shape[1]
    return (np.array([eta(A, S[:, c], B[:, c]) for c in range(k)]),
            None if X is None else np.array([forward_error(S[:, c], X[:, c]) for c in range(k)]))


@functools.lru_cache(maxsize=None)
def lapack(family, rows, seed, k, trans=False):
    """``lapack_errors`` of a family's system with the case's right-hand sides."""
    M = matrix(family, rows, seed)
    B, X = rhs(M, k, seed, trans)
    return lapack_errors(M.T if trans else M, B, X)
