"""Inputs on which the cone code leaves its generic path
(test_cone_edge_cases_cpu.py proves on the oracle which branch each takes and
measures the bars, test_cone_edges_gpu.py runs them through every conic route).

Only v = y − s matters to conic_cone_kernel and to dpi_apply, so every problem
here is built from a chosen v per cone: y = max(v, 0), s = max(−v, 0) entry by
entry (one of the two is zero, so y − s = v exactly), s = 0 and y = v on the
exact cones, y = s ≠ 0 where v = 0 is meant.  A, b, c, x, the tangents and the
seed are random: neither the oracle nor the engine checks optimality.

A cone carries ``exact=True`` when its branch selection and its π are the same
in any summation order: zeros, small integers, powers of two (Σ 3² + 4² = 25,
64 × 0.5² = 16, an already diagonal PSD input).  Everything else stays inside a
guard band in which no correct implementation can take another branch:
min|λ| ≥ 1e-3·max|λ| (PSD), |‖x‖ − |t|| ≥ 0.1·‖x‖ (SOC), |v| ≥ 0.5
(elementwise).

LSQR is capped at k = 1, 2, 3 iterations (test_conic_gpu.test_capped_lsqr_istop7's
device): engine and oracle do the same k steps, so the comparison carries no
stopping noise and the bar comes from the oracle alone — bar() below.

Everything is built once per process and never modified."""

import copy
import functools

import numpy as np

from oracle import cones as C
from oracle import conic as ocn

N_VARS = 7
CAPS = (1, 2, 3)
SPREAD_TRIALS = 3
BAR_FLOOR = 1e-12     # exact cases have spread 0: four chained products of ≤ 257 terms and Jacobi's
                      # orthogonality loss d·eps ≈ 6e-14, three LSQR steps on top, a margin of ≈ 15
SPREAD_LIMIT = 1e-10  # asserted on the CPU for every case: no bar exceeds 1e-9
EPS = 2.0 ** -52


# ---------------------------------------------------------------------------
# v per cone: (v, y, s, exact, branch); `branch` is what the CPU test proves
# ---------------------------------------------------------------------------
def _split(v):
    return np.maximum(v, 0.0), np.maximum(-v, 0.0)


def _exact(v):
    """s = 0, y = v; y = s = 1 where v = 0."""
    v = np.asarray(v, float)
    z = v == 0.0
    return v, np.where(z, 1.0, v), np.where(z, 1.0, 0.0)


INTS = [0.0, 1.0, -2.0, 0.0, 3.0, -1.0, 0.5, -0.5]


def _elementwise(dim, kind, rng):
    if kind == "rand":     # both signs from dim 2 on, |v| in [0.5, 2]
        v = rng.uniform(0.5, 2.0, dim) * np.where(rng.random(dim) < 0.5, -1.0, 1.0)
        if dim > 1:
            v[0], v[-1] = abs(v[0]), -abs(v[-1])
        return (v,) + _split(v) + (False, "rand")
    if kind == "ints":     # exact, every third entry or so v = 0 with y = s = 1
        v = np.array([INTS[i % len(INTS)] for i in range(dim)])
        return _exact(v) + (True, "ints")
    raise ValueError(kind)


def _unit(dim, rng):
    x = rng.standard_normal(dim)
    return x / np.linalg.norm(x)


# SOC kind → (t for ‖x‖ ≈ 1, case index of oracle.cones.dproj / conic_cone_kernel)
SOC_GENERIC = {"interior": (1.5, 0), "dual": (-1.5, 1), "gen+": (0.5, 2), "gen-": (-0.5, 2), "gen0": (0.0, 2)}
# exact SOC inputs: kind → (v, case index, closed-form π)
SOC_EXACT = {
    "t+": ([2.0], 0, [2.0]), "t-": ([-2.0], 1, [0.0]), "t0": ([0.0], 0, [0.0]),
    "bd2+": ([1.0, 1.0], 0, [1.0, 1.0]), "bd2-": ([-1.0, -1.0], 1, [0.0, 0.0]),
    "gen2": ([0.25, -1.0], 2, [0.625, -0.625]),
    "345+": ([5.0, 3.0, 4.0], 0, [5.0, 3.0, 4.0]), "345-": ([-5.0, 3.0, 4.0], 1, [0.0, 0.0, 0.0]),
    "3450": ([0.0, 3.0, 4.0], 2, [2.5, 2.5 * (3.0 / 5.0), 2.5 * (4.0 / 5.0)]),
    "v0": ([0.0, 0.0, 0.0], 0, [0.0, 0.0, 0.0]),
    "x0t-": ([-2.0, 0.0, 0.0, 0.0], 1, [0.0] * 4), "x0t+": ([2.0, 0.0, 0.0, 0.0], 0, [2.0, 0.0, 0.0, 0.0]),
    # 64 entries of 0.5: Σ = 16 in any order, ‖x‖ = 4
    "bd65+": ([4.0] + [0.5] * 64, 0, [4.0] + [0.5] * 64), "bd65-": ([-4.0] + [0.5] * 64, 1, [0.0] * 65),
    "bd650": ([0.0] + [0.5] * 64, 2, [2.0] + [0.25] * 64),
}


def _soc(dim, kind, rng):
    if kind in SOC_EXACT:
        v, cs, vp = SOC_EXACT[kind]
        assert len(v) == dim, (kind, dim)
        return _exact(v) + (True, ("soc", cs, tuple(vp)))
    t, cs = SOC_GENERIC[kind]
    v = np.concatenate([[t], _unit(dim - 1, rng) * rng.uniform(0.9, 1.1)])
    return (v,) + _split(v) + (False, ("soc", cs, None))


DIAG_MIXED = [-2.0, 0.0, 4.0, 0.0, 2.0, -3.0, 1.0, 0.5, 4.0]   # a negative and a zero from side 2 on, ties from 4 on
DIAG_NONNEG = [4.0, 0.0, 2.0, 0.0, 1.0, 0.5, 4.0, 2.0, 2.0]    # Dπ = I with exact zero eigenvalues


def psd_spectrum(d, kind, rng):
    """Eigenvalues of smat(v) for `kind`."""
    if kind == "mixed":
        lam = rng.uniform(0.5, 2.0, d) * np.where(np.arange(d) % 2 == 0, -1.0, 1.0)
        return lam if d > 1 else np.abs(lam)
    if kind == "neg":
        return -rng.uniform(0.5, 2.0, d)
    if kind == "pos":
        return rng.uniform(0.5, 2.0, d)
    if kind == "clustered":      # −1 (3 of 7), 2 (4 of 7)
        k = max(1, (3 * d) // 7)
        return np.concatenate([-np.ones(k), 2.0 * np.ones(d - k)])
    if kind == "near":           # ±(1 + 1e-9·i)
        i = np.arange(d)
        return np.where(i % 2 == 0, -1.0, 1.0) * (1.0 + 1e-9 * i)
    if kind == "graded":         # |λ| from 1 down to 1.8e-3 (inside the 1e-3 band after the rotation's rounding)
        i = np.arange(d)
        return np.where(i % 2 == 0, -1.0, 1.0) * 10.0 ** (-2.75 * i / max(d - 1, 1))
    if kind in ("diag", "diagpos"):
        src = DIAG_MIXED if kind == "diag" else DIAG_NONNEG
        return np.array([src[i % len(src)] for i in range(d)])
    if kind in ("pos1", "neg1", "zero1"):
        assert d == 1
        return np.array([{"pos1": 2.0, "neg1": -2.0, "zero1": 0.0}[kind]])
    raise ValueError(kind)


PSD_EXACT = ("diag", "diagpos", "pos1", "neg1", "zero1")


def _psd(dim, kind, rng):
    d = C.psd_side(dim)
    lam = psd_spectrum(d, kind, rng)
    if kind in PSD_EXACT:
        return _exact(C.tri(np.diag(lam))) + (True, ("psd", kind, tuple(lam)))
    Q = np.linalg.qr(rng.standard_normal((d, d)))[0]
    X = (Q * lam) @ Q.T
    v = C.tri((X + X.T) / 2.0)
    return (v,) + _split(v) + (False, ("psd", kind, tuple(lam)))


def make_cone(code, dim, kind, rng):
    if dim == 0:
        z = np.zeros(0)
        return z, z, z, True, "empty"
    if code in (C.ZEROS, C.NONNEG, C.NONPOS):
        return _elementwise(dim, kind, rng)
    return _soc(dim, kind, rng) if code == C.SOC else _psd(dim, kind, rng)


# ---------------------------------------------------------------------------
# families: lists of tables; a table is a list of slots (code, dim, kinds).
# Problem p of a batch gives slot i the kind kinds[(p + i) % len(kinds)], so a
# slot sees several branches over the batch and two neighbouring slots never
# rotate in step; a tuple of kinds is taken as listed, kinds[p].
# ---------------------------------------------------------------------------
EW = ["rand", "ints", "rand"]
SOC5 = ["interior", "dual", "gen+", "gen-", "gen0"]
SPECTRA = ["mixed", "neg", "pos", "clustered", "near", "graded", "diag"]
T = lambda d: d * (d + 1) // 2


def _tables():
    fam = {}
    fam["elementwise"] = [[(0, 1, EW)] + [(code, dim, EW) for dim in (1, 255, 256, 257) for code in (1, 2)]
                          + [(1, 5, ["ints"]), (2, 5, ["ints"])]]
    soc = [(3, 1, ["t+", "t-", "t0"]), (3, 2, ["bd2+", "bd2-", "gen2"]), (3, 3, ["345+", "345-", "3450"]),
           (3, 3, ["v0", "gen+", "345-"]), (3, 4, ["x0t-", "x0t+", "gen-"])]
    soc += [(3, dim, SOC5) for dim in (64, 65, 66, 257, 300)] + [(3, 65, ["bd65+", "bd65-", "bd650"])]
    fam["soc"] = [soc]
    psd = [(4, 1, ["pos1", "neg1", "zero1"])] + [(4, T(d), SPECTRA) for d in (2, 3, 4, 5, 7, 8, 9)]
    psd += [(4, T(7), ["clustered", "diag", "near"]), (4, T(8), ["diag", "diagpos", "neg"])]
    fam["psd_small"] = [psd]
    edge = ("mixed", "clustered", "neg")    # problem 0, 1, 2
    fam["psd_lds_edge"] = [[(4, T(63), edge), (3, 3, ["345+", "gen+", "3450"]), (1, 2, EW), (4, T(3), SPECTRA)],
                           [(1, 2, EW), (4, T(64), edge), (3, 3, ["gen-", "345-", "v0"]), (4, T(2), SPECTRA)]]
    fam["psd_big"] = [[(4, T(65), edge), (3, 3, ["345+", "gen+", "3450"]), (4, T(66), ("pos", "mixed", "near")),
                       (1, 2, EW)]]
    fam["psd_table"] = [[(4, T(d), [k])] for d in (256, 257) for k in ("mixed", "clustered")]
    cyc = [(3, 3, ["345+", "345-", "3450", "v0", "interior", "dual", "gen+", "gen-", "gen0"]), (1, 1, EW),
           (4, T(3), SPECTRA), (0, 1, EW)]
    fam["many_cones"] = [[cyc[i % 4] for i in range(nc)] for nc in (128, 129, 300)]
    base = [soc[2], soc[4], (3, 5, SOC5), psd[2], psd[3], (1, 4, EW)]
    empties = [(0, 0, ["-"]), (1, 0, ["-"]), (2, 0, ["-"]), (4, 0, ["-"])]
    fam["empty_cones"] = [[empties[j % 4]] + base[:3] + [empties[(j + 1) % 4], empties[(j + 2) % 4]] + base[3:]
                          + [empties[(j + 3) % 4]] for j in range(4)]
    fam["empty_cones"] += [[(4, T(3), SPECTRA)], [(0, 4, EW), (0, 1, EW), (0, 3, EW)]]
    return fam


TABLES = _tables()
FAMILIES = list(TABLES)
BATCH_OF = {"psd_table": 1}     # B per table; 3 elsewhere
SPLIT_ONLY = ("psd_big", "psd_table")   # PSD sides above 64: the split path only, never the sparse route
SEED0 = 7300


def _kind(slot, p, kinds):
    return kinds[p] if isinstance(kinds, tuple) else kinds[(p + slot) % len(kinds)]


@functools.lru_cache(maxsize=None)
def batch(family, ti):
    """Table ti of `family` as a batch: dict cones, B, n, m, the problem data
    A, b, c, x, s, y, the tangents dA, db, dc, the seed dx (leading axis B),
    A_sparse (about half of A's entries zeroed: the sparse route's input),
    seeds_k (4 reverse seeds and tangents, the first the ones above) and
    info[p][i] = (kind, exact, branch) of cone i in problem p."""
    table = TABLES[family][ti]
    B = BATCH_OF.get(family, 3)
    rng = np.random.default_rng(SEED0 + 100 * FAMILIES.index(family) + ti)
    cones = [(code, dim) for code, dim, _ in table]
    m, n = sum(dim for _, dim in cones), N_VARS
    ys, ss, info = [], [], []
    for p in range(B):
        parts = [make_cone(code, dim, _kind(i, p, kinds), rng) for i, (code, dim, kinds) in enumerate(table)]
        ys.append(np.concatenate([q[1] for q in parts]))
        ss.append(np.concatenate([q[2] for q in parts]))
        info.append([(_kind(i, p, table[i][2]), q[3], q[4]) for i, q in enumerate(parts)])
    A = rng.standard_normal((B, m, n)) / np.sqrt(n)
    d = dict(cones=cones, B=B, n=n, m=m, info=info, A=A, A_sparse=A * (rng.random((B, m, n)) < 0.5),
             y=np.stack(ys), s=np.stack(ss))
    for k, shape in (("b", (B, m)), ("c", (B, n)), ("x", (B, n)), ("dA", (B, m, n)), ("db", (B, m)), ("dc", (B, n)),
                     ("dx", (B, n))):
        d[k] = rng.standard_normal(shape)
    extra = {k: rng.standard_normal((3,) + d[k].shape) for k in ("dA", "db", "dc", "dx")}
    d["seeds_k"] = {k: np.concatenate([d[k][None], extra[k]]) for k in extra}
    return d


def batches(family):
    return [batch(family, ti) for ti in range(len(TABLES[family]))]


def cases():
    """Every (family, table, problem)."""
    return [(f, ti, p) for f in FAMILIES for ti in range(len(TABLES[f])) for p in range(batch(f, ti)["B"])]


def exact_rows(d, p):
    """Mask over the m rows: the rows of exact cones (never perturbed: one ulp
    on a boundary or on v = 0 changes the branch by design)."""
    return np.concatenate([np.full(dim, e) for (_, dim), (_, e, _) in zip(d["cones"], d["info"][p])] + [np.zeros(0, bool)])


def cone_label(d, p, i):
    code, dim = d["cones"][i]
    return f"cone {i}: {C.NAMES[code]}({dim}) {d['info'][p][i][0]}"


# ---------------------------------------------------------------------------
# a second eigensolver
# ---------------------------------------------------------------------------
def jacobi_eigh(X, max_sweeps=60):
    """Textbook cyclic Jacobi (Golub & Van Loan, Algorithm 8.4.3, with the
    symmetric Schur rotation 8.4.1) in a tournament ordering, ⌊d/2⌋ disjoint
    rotations per numpy operation.  A rotation is skipped where the pivot
    cannot change the matrix any more (|a_pq| below the last bit of the
    Frobenius norm by a factor 2⁻⁸).  The loop stops when a sweep rotated
    nothing, or when the off-diagonal norm, already at rounding level
    (≤ 64·eps·‖X‖), no longer halves: inside a cluster of eigenvalues every
    rotation angle is arbitrary and regenerates that much noise per sweep.
    Returns ascending eigenvalues and the eigenvectors as columns."""
    X = np.array(X, dtype=float)
    d = X.shape[0]
    W = np.eye(d)
    if d == 1:
        return X[0].copy(), W
    nrm = np.linalg.norm(X)
    tiny = EPS * 2.0 ** -8 * nrm
    off_before = np.inf
    de = d + (d & 1)
    players = list(range(de))
    for _ in range(max_sweeps):
        rotated = False
        for _round in range(de - 1):
            a = np.array(players[:de // 2])
            c = np.array(players[de // 2:][::-1])
            keep = (a < d) & (c < d)
            p, q = np.minimum(a, c)[keep], np.maximum(a, c)[keep]
            players = [players[0], players[-1]] + players[1:-1]
            apq = X[p, q]
            act = np.abs(apq) > tiny
            if not act.any():
                continue
            rotated = True
            p, q, apq = p[act], q[act], apq[act]
            tau = (X[q, q] - X[p, p]) / (2.0 * apq)
            t = np.where(tau >= 0, 1.0, -1.0) / (np.abs(tau) + np.hypot(1.0, tau))
            cs = 1.0 / np.hypot(1.0, t)
            sn = t * cs
            # X ← JᵀXJ as two row updates (X stays symmetric to rounding: XJ = (JᵀXᵀ)ᵀ); W = Vᵀ ← JᵀW
            c2, s2 = cs[:, None], sn[:, None]
            for M in (X, W):
                rp, rq = M[p], M[q]
                M[p], M[q] = c2 * rp - s2 * rq, s2 * rp + c2 * rq
            X = np.ascontiguousarray(X.T)
            rp, rq = X[p], X[q]
            X[p], X[q] = c2 * rp - s2 * rq, s2 * rp + c2 * rq
        off = np.linalg.norm(X - np.diag(np.diag(X)))
        if not rotated or (off <= 64 * EPS * nrm and off > 0.5 * off_before):
            break
        off_before = off
    else:
        raise RuntimeError("jacobi_eigh: no convergence")
    lam = np.diag(X).copy()
    order = np.argsort(lam, kind="stable")
    return lam[order], W.T[:, order]


class _JacobiPSD(C.PSDStructured):
    """oracle.cones.PSDStructured on jacobi_eigh's eigenpairs."""

    def __init__(self, v):
        v = np.asarray(v, dtype=float)
        self.k = v.shape[0]
        self.shape = (self.k, self.k)
        self.d = d = C.psd_side(self.k)
        lam, self.U = jacobi_eigh(C.smat(v, d))
        self.lam = lam
        self.ident = bool(np.all(lam >= 0))
        lp = np.maximum(lam, 0.0)
        B = np.empty((d, d))
        for i in range(d):
            for j in range(d):
                B[i, j] = (1.0 if lam[i] > 0 else 0.0) if lam[i] == lam[j] else (lp[i] - lp[j]) / (lam[i] - lam[j])
        self.B = B
        s = C.psd_scale(d)
        self.s2 = s * s


def jacobi_dpi(v, dense_below=C.STRUCTURED_MIN):
    """(π(v), Dπ(v)) of a PSD-triangle cone from jacobi_eigh: π = tri(U Λ⁺ Uᵀ)
    and the dense S²JS⁻² block (from side `dense_below` on: the same operator
    applied through U and B, as the oracle itself does there)."""
    op = _JacobiPSD(v)
    pi = C.tri((op.U * np.maximum(op.lam, 0.0)) @ op.U.T)
    if op.d >= dense_below:
        return pi, op
    return pi, np.stack([op @ e for e in np.eye(op.k)], axis=1)


# ---------------------------------------------------------------------------
# oracle runs
# ---------------------------------------------------------------------------
FWD_KEYS, REV_KEYS = ("fwd", "dx"), ("g", "dA", "db", "dc")
KEYS = FWD_KEYS + REV_KEYS


def make_cache(d, p, y=None, s=None, sparse=False, jacobi=False):
    A = d["A_sparse" if sparse else "A"][p]
    cache = ocn.Cache(A, d["b"][p], d["c"][p], d["x"][p], d["s"][p] if s is None else s,
                      d["y"][p] if y is None else y, d["cones"])
    if jacobi:
        off = C.cone_offsets(d["cones"])
        cache.vp = cache.vp.copy()
        for i, (code, dim) in enumerate(d["cones"]):
            if code == C.PSD and dim > 0:
                cache.vp[off[i]:off[i + 1]], cache.blocks[i] = jacobi_dpi(cache.v[off[i]:off[i + 1]])
    return cache


def with_A(cache, A_moi):
    c2 = copy.copy(cache)
    c2.A = -np.asarray(A_moi, dtype=float)
    return c2


def run_capped(cache, dA, db, dc, dx, k):
    """Both directions at cap k: dict of the six outputs and info = ((it,
    istop) forward, (it, istop) reverse)."""
    (odx, du, dv, dw), fi = ocn.forward_differentiate(cache, dA, db, dc, return_info=True, maxiter=k)
    (g, _), ri = ocn.reverse_differentiate(cache, dx, return_info=True, maxiter=k)
    odA, odb, odc = ocn.reverse_outputs(cache, g)
    return dict(fwd=np.concatenate([du, dv, [dw]]), dx=odx, g=g, dA=odA, db=odb, dc=odc, info=(fi, ri))


def errors(got, ref, cache):
    """test_conic_gpu._errors: relfro for the two LSQR solutions, relcomb for
    the outputs derived from them."""
    from test_conic_gpu import _errors
    return _errors(got, ref, cache)


_REF, _SPREAD = {}, {}


def seeds_of(d, p, j=0):
    sk = d["seeds_k"]
    return [sk[k][j][p] for k in ("dA", "db", "dc", "dx")]


def reference(family, ti, p, k, sparse=False, j=0):
    """The oracle at cap k on problem p of table ti, seed j of seeds_k
    (computed once, shared): run_capped's dict plus `cache`."""
    key = (family, ti, p, k, bool(sparse), j)
    if key not in _REF:
        d = batch(family, ti)
        ck = (family, ti, p, "cache")
        if ck not in _REF:
            _REF[ck] = make_cache(d, p)
        cache = with_A(_REF[ck], d["A_sparse"][p]) if sparse else _REF[ck]
        _REF[key] = dict(run_capped(cache, *seeds_of(d, p, j), k), cache=cache)
    return _REF[key]


def spread(family, ti, p):
    """The case's measured spread — the largest, over the caps, the six
    outputs and the dense / half-zeroed A (dense alone on SPLIT_ONLY), of (1) the oracle's change under
    SPREAD_TRIALS seeded 1-ulp perturbations (of the seeds and of y and s on
    the rows of non-exact cones) and (2) the difference between the oracle and the same
    oracle with every PSD block and π from jacobi_dpi — as dict ulp, jacobi."""
    key = (family, ti, p)
    if key in _SPREAD:
        return _SPREAD[key]
    d = batch(family, ti)
    ex = exact_rows(d, p)
    rng = np.random.default_rng(7)
    pert = lambda a: np.asarray(a, float) * (1.0 + EPS * rng.standard_normal(np.shape(a)))
    out = dict(ulp=0.0, jacobi=0.0)
    variants = []
    for _ in range(SPREAD_TRIALS):
        cache = reference(family, ti, p, 1)["cache"] if ex.all() else make_cache(
            d, p, y=np.where(ex, d["y"][p], pert(d["y"][p])), s=np.where(ex, d["s"][p], pert(d["s"][p])))
        variants.append(("ulp", cache, [pert(a) for a in seeds_of(d, p)]))
    if any(code == C.PSD and dim > 0 for code, dim in d["cones"]):
        variants.append(("jacobi", make_cache(d, p, jacobi=True), seeds_of(d, p)))
    for what, cache, seeds in variants:
        for sparse in ((False,) if family in SPLIT_ONLY else (False, True)):
            c = with_A(cache, d["A_sparse"][p]) if sparse else cache
            for k in CAPS:
                ref = reference(family, ti, p, k, sparse)
                got = run_capped(c, *seeds, k)
                err = errors(got, ref, ref["cache"])
                out[what] = max(out[what], max(err.values()))
    _SPREAD[key] = out
    return out


def bar(family, ti, p):
    """max(10 × the measured spread, BAR_FLOOR): the factor 10 because the
    engine differs from both references in summation order as well as in
    eigensolver."""
    sp = spread(family, ti, p)
    return max(10.0 * max(sp["ulp"], sp["jacobi"]), BAR_FLOOR)


# ---------------------------------------------------------------------------
# π probe: n = 1, A = 0, b = 0, c = [1], x = [0], reverse seed dx = [4] on the
# same cones and v.  M = [[0, 0, 1], [0, I − Dπ, 0], [−1, 0, 0]] and the
# right-hand side is 4·e_1: one exact LSQR step, g = (0, …, 0, 4), and
# db = g_v − g_end·π(v) = −4·π(v) — the cone kernel's π read straight out.
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def probe(family, ti):
    d = batch(family, ti)
    B, m = d["B"], d["m"]
    return dict(cones=d["cones"], B=B, n=1, m=m, info=d["info"], A=np.zeros((B, m, 1)), A_sparse=np.zeros((B, m, 1)),
                b=np.zeros((B, m)), c=np.ones((B, 1)), x=np.zeros((B, 1)), s=d["s"], y=d["y"],
                dx=np.full((B, 1), 4.0))


def probe_reference(family, ti, p):
    """(g, db, (it, istop), π(v)) of the oracle on the probe."""
    key = (family, ti, p, "probe")
    if key not in _REF:
        d = probe(family, ti)
        full = reference(family, ti, p, 1)["cache"]      # the same v: its blocks and π serve the probe
        cache = ocn.Cache.__new__(ocn.Cache)
        cache.__dict__.update(full.__dict__)
        cache.A, cache.b, cache.c, cache.x = -d["A"][p], d["b"][p], d["c"][p], d["x"][p]
        cache.n = 1
        (g, _), info = ocn.reverse_differentiate(cache, d["dx"][p], return_info=True)
        _, db, _ = ocn.reverse_outputs(cache, g)
        _REF[key] = (g, db, info, cache.vp)
    return _REF[key]
