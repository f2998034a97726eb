"""The ParametricOptInterface maps of a cone program, restated in numpy (test
infrastructure only), and the term tables the conic parameter tests share.

A term is (param, kind, index, coef) as include/diffopt_mi355x.h lists them
for dopt_conic_params_*: kind 0 a parameter term of constraint row `index` in
ProductOfSets order (ParametricVectorAffineFunction), kind 2 a parameter term
of the objective, kind 3 a parameter×variable term of the objective.

forward: reference src/parameters.jl:120-145 and :226-275 put Σ c·Δp into the
constants of ForwardConstraintFunction and into the objective's coefficient of
v; ConicProgram.jl:270-287 reads them with `_fill(S -> false, …)`, so db keeps
its sign (the QP back-end negates: oracle/poi.py).
reverse: parameters.jl:365-388 and :463-509 sum c · (the constant of
ReverseConstraintFunction's row: `_get_db`, ConicProgram.jl:414-428), c · (the
coefficient of v in ReverseObjectiveFunction: :396-401) and c · (its constant,
0.0: :400), with the dictionary accumulation `get!(…, p, 0.0) + c·s` in the
caller's term order.
"""
import numpy as np

M69 = [(0, 2), (1, 30), (2, 20), (3, 8), (4, 6), (4, 3)]   # test_sparse_gpu.CONIC_ALL5[0]: n = 60, every cone code
RHS_CONES = [(0, 1), (3, 3)]                                # test/parameters.jl:103-152


def forward(terms, dp, n, m):
    """(db, dc) of one problem from its parameter tangents dp."""
    db, dc = np.zeros(m), np.zeros(n)
    for (par, kind, idx, coef) in terms:
        if kind == 0:
            db[idx] += dp[par] * coef
        elif kind == 3:
            dc[idx] += dp[par] * coef
        elif kind != 2:
            raise ValueError(kind)
    return db, dc


def reverse(terms, nparam, g, x, vp):
    """ReverseConstraintSet of every parameter of one problem from a reverse
    solve's g = [g_x | g_v | g_end]."""
    n, m = len(x), len(vp)
    ge = g[n + m]
    out = {}
    for (par, kind, idx, coef) in terms:
        if kind == 0:
            s = g[n + idx] - ge * vp[idx]
        elif kind == 3:
            s = g[idx] - ge * x[idx]
        elif kind == 2:
            s = 0.0
        else:
            raise ValueError(kind)
        out[par] = out.get(par, 0.0) + coef * s
    res = np.zeros(nparam)
    for par, v in out.items():
        res[par] = v
    return res


def edge_terms(n, m, nparam, seed):
    """A table on the accumulation kernels' edges: parameter 0 repeats one
    (parameter, row) pair three times and touches the first and last row of m
    and variables 0 and n − 1; the last parameter shares those rows and
    variables (several parameters on one row: summation order); one parameter
    in the middle (nparam ≥ 4) has no term at all and one has a kind-2 term
    only; the rest draw random rows, variables and kinds.  Coefficients of
    mixed magnitude, so a different summation order shows at 1e-13."""
    rng = np.random.default_rng(seed)
    coef = lambda: float(rng.standard_normal() * 10.0 ** rng.integers(-3, 4))
    last = nparam - 1
    terms = [(0, 0, 0, coef()), (0, 0, 0, coef()), (0, 0, 0, coef()), (0, 0, m - 1, coef()),
             (0, 3, 0, coef()), (0, 3, n - 1, coef()), (0, 2, 0, coef())]
    terms += [(last, 0, 0, coef()), (last, 0, m - 1, coef()), (last, 3, n - 1, coef()), (last, 3, 0, coef())]
    empty, k2only = (1, 2) if nparam >= 4 else (-1, -1)
    if k2only >= 0:
        terms.append((k2only, 2, 0, coef()))
    free = [p for p in range(nparam) if p not in (empty, k2only)]
    for _ in range(3 * nparam + 20):
        p = int(free[rng.integers(len(free))])
        kind = int(rng.choice([0, 0, 3, 2]))
        lim = m if kind == 0 else n
        terms.append((p, kind, int(rng.integers(lim)), coef()))
    order = rng.permutation(len(terms))
    return [terms[i] for i in order]


def e2e_terms(n, m, seed=5):
    """The end-to-end table: 7 parameters, 40 row terms, 15 objective
    parameter×variable terms and one kind-2 term (parameter 6's only term: it
    enters nothing)."""
    rng = np.random.default_rng(seed)
    terms = [(int(rng.integers(6)), 0, int(rng.integers(m)), float(rng.standard_normal())) for _ in range(40)]
    terms += [(int(rng.integers(6)), 3, int(rng.integers(n)), float(rng.standard_normal())) for _ in range(15)]
    terms.append((6, 2, 0, 1.5))
    for p in range(6):   # every one of the six has at least one entering term
        assert any(t[0] == p for t in terms)
    return terms, 7
