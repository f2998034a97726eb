"""Inputs on which LSQR leaves its generic path (test_lsqr_edge_cases_cpu.py
proves on the oracle which branch each takes, test_lsqr_edges_gpu.py runs
them through every LSQR kernel).

On random data every step has β > 0 and α > 0 and the run stops with istop 1,
2 or 7.  The inputs here reach the other paths of csrc/lsqr_core.h and of the
kernels that sequence it by hand (conic_lsqr2_kernel, conic_lsqrk_kernel, the
split path):

* ``beta0``  — exact breakdown, β = 0 inside the loop: the Mᵀ product and the
  v update of that step are skipped;
* ``alpha0`` — Mᵀb = 0 for a non-zero b: x = 0, 0 iterations, istop 0 (the
  second early return, after the zero-seed one);
* ``istop3`` — the condition-number stop;
* the 4- and 16-lane instantiations of the sparse products.

Every degenerate block is built from zeros, single entries and powers of two,
so each quantity LSQR forms on it is exact in binary floating point in any
summation order (each sum has one non-zero term, each product or quotient is
a power of two, hypot(x, 0) = |x|): the oracle's branch and the engine's are
the same branch by construction, not merely up to rounding.  Such cases carry
``exact=True`` and are compared bit for bit.

istop 4, 5 and 6 cannot be returned at the default tolerances: each is
overwritten by 1, 2 or 3 in the same step, since 1 + t ≤ 1 implies
t ≤ eps/2 < √eps = atol = btol = ctol (and test1 ≤ rtol follows from
t1r·(1 + ‖A‖‖x‖/‖b‖) = test1 with rtol = √eps·(1 + ‖A‖‖x‖/‖b‖)).  No case
looks for them.  istop 7 needs a cap (test_conic_gpu.test_capped_lsqr_istop7);
the plug point fixes maxiter = N.

Everything is built once per process (lru_cache) and never modified."""

import functools

import numpy as np

from diffopt_amd.synthetic import conic_numpy_wellcond, lp_sparse_numpy
from oracle import conic as ocn
from oracle import lsqr as olsqr
from oracle import qp as oqp

SP_LANE_BOUNDS = (12.0, 48.0)   # dopt_internal.h::sp_lanes


def sp_lanes(entries_per_output):
    """dopt_internal.h::sp_lanes, restated."""
    return 1 if entries_per_output <= SP_LANE_BOUNDS[0] else 4 if entries_per_output <= SP_LANE_BOUNDS[1] else 16


class Counted:
    """matvec / rmatvec of an operator with call counts: an LSQR run of `it`
    iterations makes `it` matvec calls and 1 + it rmatvec calls, less one
    rmatvec per step with β = 0; a run that stops at α = 0 after the first
    rmatvec makes that one call and no matvec."""

    def __init__(self, matvec, rmatvec):
        self._mv, self._rmv = matvec, rmatvec
        self.nmv = self.nrmv = 0

    def matvec(self, v):
        self.nmv += 1
        return self._mv(v)

    def rmatvec(self, u):
        self.nrmv += 1
        return self._rmv(u)


def counted_lsqr(matvec, rmatvec, b, n, **kw):
    """(x, it, istop, matvec calls, rmatvec calls, stats dict)."""
    op = Counted(matvec, rmatvec)
    stats = {}
    x, it, istop = olsqr.lsqr(op.matvec, op.rmatvec, b, n, return_info=True, stats=stats, **kw)
    return x, it, istop, op.nmv, op.nrmv, stats


def branch_of(it, istop, nmv, nrmv):
    """The branch the call counts prove: "zero" (no product at all: b = 0),
    "alpha0" (one rmatvec, no matvec), "beta0" (a step skipped its rmatvec) or
    "generic" (every step made both products)."""
    if nmv == 0 and nrmv == 0:
        return "zero"
    if it == 0:
        assert (nmv, nrmv) == (0, 1)
        return "alpha0"
    assert nmv == it and nrmv <= it + 1
    return "generic" if nrmv == it + 1 else "beta0"


# ---------------------------------------------------------------------------
# plug point: dense M through solve_system(M, b, iterative=True) — qp_lsqr_kernel
# ---------------------------------------------------------------------------
def _e(n, *pairs):
    v = np.zeros(n)
    for i, a in pairs:
        v[i] = a
    return v


# diag(2^p)·x = 2^q from a seeded random search over exponents in [−40, 0],
# N ≤ 8 (about one draw in 2000 stops with istop 3), kept for: (3, 3) also under
# 1e-6 relative perturbations of b, a 1-ulp envelope of the oracle's x at
# rounding level (1.1e-15), and an x that moves by ≈ 1 when cut at 2 iterations
ISTOP3_P = [-31, -29, -5, -4, -11]
ISTOP3_Q = [0, -36, -39, -40, -39]


@functools.lru_cache(maxsize=None)
def plug_cases():
    """dict name → case: M (N × N), b, the oracle's (it, istop), the branch,
    `exact` (bitwise comparable) and the closed-form x where there is one."""
    D8 = np.diag([0.0, 0, 1, 1, 1, 1, 0, 0])
    T6 = np.triu(np.ones((6, 6)))
    T6[-1] = 0.0
    cases = [
        dict(name="single entry", M=D8, b=_e(8, (3, 2.0)), info=(1, 1), branch="beta0", exact=True,
             x=_e(8, (3, 2.0))),
        dict(name="single entry, inconsistent", M=D8, b=_e(8, (3, 2.0), (0, 1.0)), info=(1, 2), branch=None,
             exact=False, x=_e(8, (3, 2.0))),
        dict(name="Mtb = 0", M=D8, b=_e(8, (0, 1.0)), info=(0, 0), branch="alpha0", exact=True, x=np.zeros(8)),
        dict(name="2x2 zero row", M=np.array([[1.0, 0], [0, 0]]), b=np.array([1.0, 1]), info=(1, 2), branch=None,
             exact=False, x=np.array([1.0, 0])),
        dict(name="two-dimensional Krylov space", M=np.diag([3.0, 3, 3, 4, 4, 4, 0, 0]),
             b=_e(8, (0, 3.0), (3, 4.0)), info=(2, 1), branch=None, exact=False, x=_e(8, (0, 1.0), (3, 1.0))),
        dict(name="triangular, zero last row", M=T6, b=np.arange(1.0, 7.0), info=(5, 2), branch="generic",
             exact=False, x=np.linalg.lstsq(T6, np.arange(1.0, 7.0), rcond=None)[0]),
        dict(name="istop 3", M=np.diag(2.0 ** np.array(ISTOP3_P)), b=2.0 ** np.array(ISTOP3_Q), info=(3, 3),
             branch="generic", exact=False, x=None),
    ]
    return {c["name"]: c for c in cases}


# mixed cases of equal size in one launch: a workgroup that leaves at once, one
# that breaks down and one that iterates, in both orders
PLUG_BATCHES = [("single entry", "Mtb = 0", "two-dimensional Krylov space"),
                ("two-dimensional Krylov space", "single entry, inconsistent", "single entry")]


def ulp_envelope(solve, args, ref, trials=3):
    """test_conic_gpu.envelope's idea: the largest relative change of the
    oracle's output under a 1-ulp (relative 2⁻⁵², seeded) perturbation of its
    right-hand-side data; also the (it, istop) of every perturbed run."""
    rng = np.random.default_rng(7)
    worst, infos = 0.0, []
    nr = np.linalg.norm(ref)
    for _ in range(trials):
        pert = [np.asarray(a, float) * (1.0 + 2.0 ** -52 * rng.standard_normal(np.shape(a))) for a in args]
        x, it, istop = solve(*pert)
        worst = max(worst, np.linalg.norm(x - ref) / nr if nr > 0 else np.linalg.norm(x))
        infos.append((it, istop))
    return worst, infos


# ---------------------------------------------------------------------------
# sparse LP route: QPBatch(sparse=True) + set_csc — sp_lsqr_kernel<lanes>
# ---------------------------------------------------------------------------
LP_N0, LP_P0, LP_EXTRA, LP_K, LP_SEED, LP_B = 40, 4, 30, 3, 9114, 3


def _extend_lp(d0):
    """Every problem of an lp_sparse_numpy batch with (a) variable n0: empty
    column in G and A; (b) variable n0 + 1: the single coefficient 0.5 in the
    new equality row p0; (c) inequality row m0: all zeros, λ = 0, h = 2 (so
    s = −2).  New z, ν entries 0.  The KKT LHS is block diagonal: the original
    LHS, the 2 × 2 block [[0, 0.5], [0.5, 0]] on (z_b, ν_new), the 1 × 1 block
    −2 on λ_c and the zero row / column of z_a."""
    import scipy.sparse as sp
    B, n0 = d0["z"].shape
    m0, p0 = d0["lam"].shape[1], d0["nu"].shape[1]
    n, m, p = n0 + 2, m0 + 1, p0 + 1
    pad = lambda a, k, v=0.0: np.concatenate([a, np.full((B, k), v)], axis=1)
    out = dict(G=[], A=[], h=pad(d0["h"], 1, 2.0), z=pad(d0["z"], 2), lam=pad(d0["lam"], 1), nu=pad(d0["nu"], 1),
               dl_dz=pad(d0["dl_dz"], 2), dq=pad(d0["dq"], 2), dh=pad(d0["dh"], 1), db=pad(d0["db"], 1))
    for b in range(B):
        G = sp.lil_matrix((m, n))
        G[:m0, :n0] = d0["G"][b]
        A = sp.lil_matrix((p, n))
        A[:p0, :n0] = d0["A"][b]
        A[p0, n0 + 1] = 0.5
        out["G"].append(sp.csc_matrix(G))
        out["A"].append(sp.csc_matrix(A))
    return out


@functools.lru_cache(maxsize=None)
def lp_case():
    """The extended LP batch and its calls.  A call is a dict of (B, ·)
    arrays dl_dz, dq, dh, db plus `rev` / `fwd`: per problem the kind of that
    direction's run — "beta0", "alpha0", "zero" (exact; the CPU test proves
    the branch and the closed form) or "generic" (with or without a breakdown
    component; the CPU test records what the oracle gives)."""
    d0 = lp_sparse_numpy(LP_B, LP_N0, LP_P0, LP_EXTRA, LP_K, LP_SEED)
    d = _extend_lp(d0)
    B, n = d["z"].shape
    m, p = d["lam"].shape[1], d["nu"].shape[1]
    va, vb, rc, re = n - 2, n - 1, m - 1, p - 1
    gen_r = d["dl_dz"]                      # the generator's seeds, zero on the new entries
    gen_q, gen_h, gen_b = d["dq"], d["dh"], d["db"]
    zn, zm, zp = np.zeros(n), np.zeros(m), np.zeros(p)

    def call(name, rev, fwd):
        c = dict(name=name, dl_dz=np.stack([r[1] for r in rev]), dq=np.stack([f[1] for f in fwd]),
                 dh=np.stack([f[2] for f in fwd]), db=np.stack([f[3] for f in fwd]),
                 rev=[r[0] for r in rev], fwd=[f[0] for f in fwd])
        return c

    r_b0 = ("beta0", _e(n, (vb, 4.0)))                      # −8 at the new ν
    r_a0 = ("alpha0", _e(n, (va, 4.0)))
    f_b0 = ("beta0", zn, zm, _e(p, (re, 2.0)))              # db on the new equality row: 4 at z_b
    f_zero = ("zero", zn, _e(m, (rc, 3.0)), zp)             # dh on row (c): −λ·dh = 0
    f_a0 = ("alpha0", _e(n, (va, 4.0)), zm, zp)             # dq on the unused variable: LHSᵀ·e_a = 0
    calls = [
        call("degenerate | generic | never live",
             [r_b0, ("generic", gen_r[1]), r_a0],
             [f_b0, ("generic", gen_q[1], gen_h[1], gen_b[1]), f_zero]),
        call("generic + breakdown component | never live | degenerate",
             [("generic", gen_r[0] + r_b0[1]), r_a0, r_b0],
             [("generic", gen_q[0], gen_h[0], gen_b[0] + f_b0[3]), f_a0, f_b0]),
    ]
    return d, calls


def lp_oracle_run(d, b, dl_dz, dq, dh, db):
    """oracle.qp.lp_sparse_differentiate on problem b with call counts:
    ((out, it, istop, nmv, nrmv), …) for reverse and forward."""
    n = d["z"].shape[1]
    m, p = d["lam"].shape[1], d["nu"].shape[1]
    L = oqp.create_LHS_sparse(d["z"][b], d["lam"][b], d["G"][b], d["h"][b], d["A"][b], n)
    N = n + m + p
    r_rev = np.concatenate([dl_dz, np.zeros(m + p)])
    r_fwd = np.concatenate([dq, -d["lam"][b] * dh, -db])
    res = []
    for mat, rhs in ((L, r_rev), (L.T.tocsc(), r_fwd)):
        x, it, istop, nmv, nrmv, _ = counted_lsqr(lambda v: mat @ v, lambda u: mat.T @ u, rhs, N)
        res.append((-x, it, istop, nmv, nrmv))
    return res


ENV_TRIALS = 8   # perturbed oracle runs per measured envelope / iteration spread


def _perturbed(args, rng):
    return [np.asarray(a, float) * (1.0 + 2.0 ** -52 * rng.standard_normal(np.shape(a))) for a in args]


_LP_ENV = {}


def lp_envelope(ci, b):
    """Problem b of lp_case()'s call ci: {"rev" | "fwd": (envelope, spread)} —
    the largest relative change of the oracle's output, and the largest change
    of its iteration count, over ENV_TRIALS runs with the seeds / tangents
    perturbed by one ulp (relative 2⁻⁵², seeded); (inf, ·) if a perturbed run
    stops with another code.  Computed once, shared."""
    if (ci, b) not in _LP_ENV:
        d, calls = lp_case()
        c = calls[ci]
        args = [c[k][b] for k in ("dl_dz", "dq", "dh", "db")]
        ref = lp_oracle_run(d, b, *args)
        rng = np.random.default_rng(7)
        env, spread = [0.0, 0.0], [0, 0]
        for _ in range(ENV_TRIALS):
            for q, r in enumerate(lp_oracle_run(d, b, *_perturbed(args, rng))):
                nr = np.linalg.norm(ref[q][0])
                e = np.linalg.norm(r[0] - ref[q][0]) / nr if nr > 0 else np.linalg.norm(r[0])
                env[q] = max(env[q], e if r[2] == ref[q][2] else np.inf)
                spread[q] = max(spread[q], abs(r[1] - ref[q][1]))
        _LP_ENV[(ci, b)] = dict(rev=(env[0], spread[0]), fwd=(env[1], spread[1]))
    return _LP_ENV[(ci, b)]


def lp_entries_per_output(d):
    """sparse.hip's lane formula: 2·(nnz G + nnz A)/(B·N)."""
    B, n = d["z"].shape
    N = n + d["lam"].shape[1] + d["nu"].shape[1]
    nnz = sum(g.nnz for g in d["G"]) + sum(a.nnz for a in d["A"])
    return 2.0 * nnz / (B * N)


# one converging LP per lane width: (B, n, p, m_extra, k, seed) → lanes.  The
# two routes compared at 1e-7 on them differ by LSQR's stopping noise, which on
# this family is often ≈ 1e-7 itself; the seeds are the first of s, s + 10, …
# whose oracle outputs move by ≤ 1e-8 under 1-ulp perturbations (lp_lanes_envelope)
LP_LANES = {1: (2, 60, 6, 60, 3, 9511), 4: (2, 60, 6, 66, 12, 9222), 16: (2, 100, 10, 110, 60, 9253)}


@functools.lru_cache(maxsize=None)
def lp_lanes(lanes):
    return lp_sparse_numpy(*LP_LANES[lanes])


@functools.lru_cache(maxsize=None)
def lp_lanes_envelope(lanes):
    """The largest 1-ulp envelope over lp_lanes(lanes)' problems and directions."""
    d = lp_lanes(lanes)
    worst = 0.0
    for b in range(d["z"].shape[0]):
        args = [d[k][b] for k in ("dl_dz", "dq", "dh", "db")]
        ref = lp_oracle_run(d, b, *args)
        rng = np.random.default_rng(7)
        for _ in range(ENV_TRIALS):
            for q, r in enumerate(lp_oracle_run(d, b, *_perturbed(args, rng))):
                worst = max(worst, np.linalg.norm(r[0] - ref[q][0]) / np.linalg.norm(ref[q][0]))
    return worst


# ---------------------------------------------------------------------------
# conic
# ---------------------------------------------------------------------------
CONIC_CONES0 = [(0, 2), (1, 6), (3, 4), (4, 6)]
CONIC_N0, CONIC_SEED, CONIC_B = 20, 9310, 3
EXT_CONES = [(0, 1), (1, 2)]    # (b)'s one-row Zeros cone, (c)'s two-row Nonnegatives cone
PSD62 = (4, 62 * 63 // 2)       # the widest side on the persistent kernel: two-wide conic_lsqrk groups


def _extend_conic(d0, cones0):
    """Every problem of a conic batch with (a) variable n0: empty column of A,
    c = 0, x = 0; (b) variable n0 + 1 coupled by the single 0.5 to a new
    one-row Zeros cone with b = 0 (Dπ = 1); (c) a new Nonnegatives cone of two
    rows whose A rows are zero, b = 0, s = 1, y = 0 (v = −1, Dπ = 0).  Dense
    tangents / seeds padded with zeros."""
    B, m0, n0 = d0["A"].shape
    n, m = n0 + 2, m0 + 3
    A = np.zeros((B, m, n))
    A[:, :m0, :n0] = d0["A"]
    A[:, m0, n0 + 1] = 0.5
    dA = np.zeros((B, m, n))
    dA[:, :m0, :n0] = d0["dA"]
    pad = lambda a, tail: np.concatenate([a, np.tile(np.asarray(tail, float), (B, 1))], axis=1)
    return dict(A=A, b=pad(d0["b"], [0, 0, 0]), c=pad(d0["c"], [0, 0]), x=pad(d0["x"], [0, 0]),
                s=pad(d0["s"], [0, 1, 1]), y=pad(d0["y"], [0, 0, 0]), dx=pad(d0["dx"], [0, 0]), dA=dA,
                db=pad(d0["db"], [0, 0, 0]), dc=pad(d0["dc"], [0, 0]))


@functools.lru_cache(maxsize=None)
def conic_case(psd=False, B=CONIC_B):
    """(cones, data, seeds): the extended conic batch — with `psd` the side-62
    PSD cone among the original cones, one problem — and its five seeds per
    direction, in the order generic, exact breakdown at iteration 1, never
    live (Mᵀb = 0), generic + breakdown component, all zero.  seeds["rev"]:
    dx (5, B, n); seeds["fwd"]: (dA (5, B, m, n), db (5, B, m), dc (5, B, n));
    seeds["kind"]: the five names."""
    cones0 = CONIC_CONES0 + ([PSD62] if psd else [])
    if psd:
        B = 1
    d0 = conic_numpy_wellcond(B, CONIC_N0, cones0, CONIC_SEED + int(psd), pair_norm=1.0)
    d = _extend_conic(d0, cones0)
    cones = cones0 + EXT_CONES
    n, m = d["x"].shape[1], d["b"].shape[1]
    va, vb, rc = n - 2, n - 1, m - 2
    Z = lambda *s: np.zeros((B,) + s)
    brk_dx, nev_dx = Z(n), Z(n)
    brk_dx[:, vb] = 4.0
    nev_dx[:, va] = 4.0
    brk_db = Z(m)
    brk_db[:, rc] = 2.0        # forward right-hand side exactly 2·e on a row of (c)
    rev = np.stack([d["dx"], brk_dx, nev_dx, d["dx"] + brk_dx, Z(n)])
    fwd = (np.stack([d["dA"], Z(m, n), Z(m, n), d["dA"], Z(m, n)]),
           np.stack([d["db"], brk_db, Z(m), d["db"] + brk_db, Z(m)]),
           np.stack([d["dc"], Z(n), nev_dx, d["dc"], Z(n)]))   # dc = 4·e_a: right-hand side 4·e_a, Mᵀ·e_a = 0
    return cones, d, dict(rev=rev, fwd=fwd, kind=["generic", "beta0", "alpha0", "mixed", "zero"])


EXACT_KINDS = ("beta0", "alpha0", "zero")
GEN, BRK, NEV, MIX, ZERO = range(5)
CONIC_BATCH_SEEDS = (BRK, GEN, ZERO)   # problem b of the mixed batch runs seed CONIC_BATCH_SEEDS[b]


def conic_cache(cones, d, b):
    return ocn.Cache(d["A"][b], d["b"][b], d["c"][b], d["x"][b], d["s"][b], d["y"][b], cones)


_CONIC_REF = {}


def conic_oracle_run(psd, b, direction, j):
    """The oracle's solve of seed j (conic_case(psd)'s order) on problem b,
    `direction` "fwd" or "rev", with call counts (computed once, shared):
    dict x (the LSQR solution), info (it, istop), nmv, nrmv, stats
    (lsqr_norms' fields) and the derived outputs — forward: fwd, dx; reverse:
    g, dA, db, dc."""
    key = (bool(psd), b, direction, j)
    if key in _CONIC_REF:
        return _CONIC_REF[key]
    cones, d, seeds = conic_case(psd)
    seed = seeds["rev"][j][b] if direction == "rev" else tuple(t[j][b] for t in seeds["fwd"])
    cache = conic_cache(cones, d, b)
    op = Counted(cache.matvec, cache.rmatvec)
    cache.matvec, cache.rmatvec = op.matvec, op.rmatvec
    stats = {}
    if direction == "fwd":
        (odx, du, dv, dw), info = ocn.forward_differentiate(cache, *seed, return_info=True, stats=stats)
        x = np.concatenate([du, dv, [dw]])
        res = dict(x=x, fwd=x, dx=odx)
    else:
        (g, _), info = ocn.reverse_differentiate(cache, seed, return_info=True, stats=stats)
        dA, db, dc = ocn.reverse_outputs(cache, g)
        res = dict(x=g, g=g, dA=dA, db=db, dc=dc)
    if not stats:
        stats = dict(rnorm=0.0, arnorm=0.0, xnorm=0.0, anorm=0.0)
    res.update(info=info, nmv=op.nmv, nrmv=op.nrmv, stats=stats, cache=cache)
    _CONIC_REF[key] = res
    return res


_CONIC_ENV = {}


def conic_envelope(psd, b, direction, j, trials=ENV_TRIALS):
    """(envelope, spread) of conic_oracle_run(psd, b, direction, j)'s LSQR
    solution, as lp_envelope measures them."""
    key = (bool(psd), b, direction, j)
    if key not in _CONIC_ENV:
        cones, d, seeds = conic_case(psd)
        ref = conic_oracle_run(psd, b, direction, j)
        args = [seeds["rev"][j][b]] if direction == "rev" else [t[j][b] for t in seeds["fwd"]]
        cache = conic_cache(cones, d, b)
        rng = np.random.default_rng(7)
        env, spread, nr = 0.0, 0, np.linalg.norm(ref["x"])
        for _ in range(trials):
            pert = _perturbed(args, rng)
            if direction == "fwd":
                (_, du, dv, dw), info = ocn.forward_differentiate(cache, *pert, return_info=True)
                x = np.concatenate([du, dv, [dw]])
            else:
                (x, _), info = ocn.reverse_differentiate(cache, pert[0], return_info=True)
            e = np.linalg.norm(x - ref["x"]) / nr if nr > 0 else np.linalg.norm(x)
            env = max(env, e if info[1] == ref["info"][1] else np.inf)
            spread = max(spread, abs(info[0] - ref["info"][0]))
        _CONIC_ENV[key] = (env, spread)
    return _CONIC_ENV[key]


def conic_entries_per_output(A):
    """conic.hip's lane formula: 2·nnz/(B·(m + n)) for A of shape (B, m, n)."""
    B, m, n = A.shape
    return 2.0 * np.count_nonzero(A) / (B * (m + n))


# the sparse conic route at 4 lanes: (B, n, cones, seed, sparse_k)
CONIC_LANES4 = (2, 40, [(0, 4), (1, 16), (2, 6), (3, 8), (4, 6)], 9400, 16)


@functools.lru_cache(maxsize=None)
def conic_lanes4():
    B, n, cones, seed, k = CONIC_LANES4
    return cones, conic_numpy_wellcond(B, n, cones, seed, pair_norm=1.0, sparse_k=k)
