"""QP reverse mode with seeds on the duals on the GPU (dopt_qp_reverse_duals_k /
dopt_qp_params_reverse_duals_k; csrc/params.hip, qp.hip, sparse.hip):
[dz; dλ; dν] = −LHS⁻¹·[dl/dz; dl/dλ; dl/dν] against the numpy restatement of
tests/qp_dual_seed_cases.py (pinned on the CPU by test_qp_dual_seeds_cpu.py) at
the project's 1e-6 relative Frobenius, on every factorisation route, and the
bit-identity statements of DESIGN.md §2.1: zero dual seeds give reverse_k's
outputs, a seed's block does not depend on how the seeds are grouped, a seed
on eliminated rows alone reaches nothing but those rows."""

import functools

import numpy as np
import pytest

import qp_dual_seed_cases as dc
import qp_param_cases as qc
from oracle import poi
from oracle import qp as oqp

pytestmark = pytest.mark.gpu
RTOL, ADJ_BAR = 1e-6, 1e-9
LSQR, NOPIV, PIVOT, SMALL = 0, 1, 2, 3
KEYS = ("Q", "G", "h", "A", "z", "lam", "nu")


@pytest.fixture(scope="module")
def QPBatch():
    from diffopt_amd.qp import QPBatch
    return QPBatch


@pytest.fixture(params=["nopiv", "pivot"])
def lu_mode(request, monkeypatch):
    if request.param == "pivot":
        monkeypatch.setenv("DOPT_LU", "0")
    else:
        monkeypatch.delenv("DOPT_LU", raising=False)
    return request.param


def _data(B, n, m, p, seed):
    from diffopt_amd.synthetic import qp_numpy
    return qp_numpy(B, n, m, p, 0.4, seed)


def _seeds(k, d, seed):
    """Standard-normal seeds on all three blocks, (k, B, ·)."""
    B, n = d["z"].shape
    m, p = d["lam"].shape[1], d["nu"].shape[1]
    rng = np.random.default_rng(seed)
    return rng.standard_normal((k, B, n)), rng.standard_normal((k, B, m)), rng.standard_normal((k, B, p))


def _engine(QPBatch, d):
    B, n = d["z"].shape
    m, p = d["lam"].shape[1], d["nu"].shape[1]
    e = QPBatch(B, n, m, p)
    e.set(d["Q"], d["G"], d["h"], d["A"], d["z"], d["lam"], d["nu"])
    return e


def _check(out, d, gz, gl, gn):
    """Every (seed, problem) pair against the restatement."""
    out = np.asarray(out)
    k, B = gz.shape[:2]
    assert out.shape == (k, B, d["z"].shape[1] + d["lam"].shape[1] + d["nu"].shape[1])
    worst = 0.0
    for j in range(k):
        for b in range(B):
            worst = max(worst, dc.relfro(out[j, b], dc.reverse_duals_flat(d, b, gz[j, b], gl[j, b], gn[j, b])))
    print(f"worst relative Frobenius error {worst:.3e}")
    assert worst <= RTOL, worst


# ---------------------------------------------------------------------------
# 1. against the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape,k", [((3, 20, 30, 4), 7),       # general
                                     ((2, 12, 0, 5), 3),        # no λ block
                                     # m > 256: the recovery's row loop wraps; a second seed chunk of one.
                                     # (n = 140, not 70: qp_numpy's ⌊0.4·300⌋ = 120 active rows on 70 variables
                                     # make LHS rank 320 of 370, cond 1.5e18 — no solution to compare)
                                     ((2, 140, 300, 0), 17),
                                     ((2, 384, 40, 3), 2),      # x_z staged in LDS (n·16·8 = 48 KB)
                                     ((2, 385, 40, 3), 2)])     # x_z unstaged
def test_against_restatement(QPBatch, lu_mode, shape, k):
    B, n, m, p = shape
    d = _data(B, n, m, p, 3100 + n)
    gz, gl, gn = _seeds(k, d, 3200 + n)
    e = _engine(QPBatch, d)
    _check(e.reverse_duals_k(gz, gl, gn), d, gz, gl, gn)
    want = NOPIV if lu_mode == "nopiv" else PIVOT
    assert (e.lu_kind() == want).all()


@pytest.mark.parametrize("target", [64, 65])
def test_lu_block_edge(QPBatch, lu_mode, target):
    """n + kept + p = 64 and 65: one full 64-column block of the LU, and one column past it."""
    m, p, n = 30, 3, 49
    for _ in range(4):   # the kept count depends on the data: step n to the target size
        d = _data(1, n, m, p, 3300)
        e = _engine(QPBatch, d)
        e.factor()
        size = int(e.system_size()[0])
        if size == target:
            break
        n += target - size
    assert size == target
    gz, gl, gn = _seeds(3, d, 3301)
    _check(e.reverse_duals_k(gz, gl, gn), d, gz, gl, gn)


def test_each_seed_block_alone(QPBatch, lu_mode):
    """Seed 0 has only dl_dz, seed 1 only dl_dlam, seed 2 only dl_dnu.  Seed 1
    moves dz: the assertion that fails on a build that ignores the dual seeds."""
    d = _data(3, 20, 30, 4, 3400)
    gz, gl, gn = _seeds(3, d, 3401)
    gz[1:] = 0.0
    gl[0] = gl[2] = 0.0
    gn[:2] = 0.0
    e = _engine(QPBatch, d)
    out = np.asarray(e.reverse_duals_k(gz, gl, gn))
    _check(out, d, gz, gl, gn)
    for b in range(3):
        assert np.linalg.norm(out[1, b, :20]) > 1e-3 and np.linalg.norm(out[2, b, :20]) > 1e-3


def test_seed_on_eliminated_rows_alone(QPBatch, lu_mode):
    """Column n+i of LHS is zero in the z rows for an eliminated row, so the
    reduced right-hand side is all zero: dz, dν and the kept rows' dλ are
    exactly zero (0.0 == −0.0: the outputs are negations), and the row itself
    gives dλ_i = −g_i/s_i (the engine's G_i·x_z is an FMA chain on zeros: one
    division and one negation away from exact; the bar is 4 ulp)."""
    d = _data(3, 20, 30, 4, 3500)
    B, n, m, p = 3, 20, 30, 4
    e = _engine(QPBatch, d)
    e.factor()
    kept = e.kept()
    el = (d["lam"] == 0.0) & ~kept
    assert el.any(axis=1).all()
    gl = np.where(el, np.random.default_rng(3501).standard_normal((B, m)), 0.0)
    out = np.asarray(e.reverse_duals(None, gl, None))
    dz, dlam, dnu = out[:, :n], out[:, n:n + m], out[:, n + m:]
    assert np.all(dz == 0.0) and np.all(dnu == 0.0) and np.all(dlam[~el] == 0.0)
    for b in range(B):
        s = oqp.gz_minus_h(d["G"][b], d["z"][b], d["h"][b])
        want = -gl[b][el[b]] / s[el[b]]
        assert np.all(np.abs(dlam[b][el[b]] - want) <= 4 * np.spacing(np.abs(want)))


# ---------------------------------------------------------------------------
# 2. bit identities
# ---------------------------------------------------------------------------
def test_zero_dual_seeds_are_reverse_k_bit_for_bit(QPBatch, lu_mode):
    case = qc.synthetic_case(3, 20, 30, 4, 16, seed=3600)
    d, terms, nparam = case["d"], case["terms"], case["nparam"]
    assert {4, 5} <= {t[1] for t in terms}
    dl = np.random.default_rng(3601).standard_normal((7, 3, 20))
    e = _engine(QPBatch, d)
    base = np.array(e.reverse_k(dl))
    assert np.array_equal(np.asarray(e.reverse_duals_k(dl)), base)
    zl, zn = np.zeros((7, 3, 30)), np.zeros((7, 3, 4))
    assert np.array_equal(np.asarray(e.reverse_duals_k(dl, zl, zn)), base)
    dp0, rev0 = (np.array(a) for a in e.params_reverse_k(dl, terms, nparam, want_rev=True))
    for seeds in ((dl, None, None), (dl, zl, zn)):
        dp1, rev1 = e.params_reverse_duals_k(*seeds, terms, nparam, want_rev=True)
        assert np.array_equal(np.asarray(dp1), dp0) and np.array_equal(np.asarray(rev1), rev0)
        assert np.array_equal(np.asarray(e.params_reverse_duals_k(*seeds, terms, nparam)), dp0)


def _mixed():
    """test_qp_params_k_gpu.py's mixed batch: (4, 20, 30, 4), problem 1 with
    Q = 0 (LSQR), problem 2 with an indefinite Q the no-pivot LU rejects, the
    others no-pivot."""
    case = qc.synthetic_case(4, 20, 30, 4, 17, seed=8101, phi=0.54)
    d = {k: v.copy() for k, v in case["d"].items()}
    d["Q"][1] = 0.0
    S = np.random.default_rng(5).standard_normal((20, 20))
    Qi = (S + S.T) / 2
    Qi[np.diag_indices(20)] = 1e-4
    d["Q"][2] = Qi
    return d


def test_a_seed_does_not_depend_on_its_group(QPBatch):
    """One seed at positions 0 and k − 1 of calls on k ∈ {1, 15, 16, 17, 33}
    seeds: always the same bits, on the no-pivot, partial-pivoting and LSQR
    problems of one batch."""
    d = _mixed()
    e = _engine(QPBatch, d)
    gz, gl, gn = _seeds(33, d, 3700)
    one = np.array(e.reverse_duals_k(gz[:1], gl[:1], gn[:1]))[0]
    assert list(e.lu_kind()) == [NOPIV, LSQR, PIVOT, NOPIV]
    for k in (15, 16, 17, 33):
        for pos in (0, k - 1):
            sz, sl, sn = (np.roll(a[:k], pos, axis=0) for a in (gz, gl, gn))   # seed 0 moves to `pos`
            out = np.asarray(e.reverse_duals_k(sz, sl, sn))
            assert np.array_equal(out[pos], one), (k, pos)


@pytest.mark.parametrize("chunk", [1, 5, 16, 17])
def test_chunk_edges_are_bit_identical(QPBatch, chunk, monkeypatch):
    d = _mixed()
    case = qc.synthetic_case(4, 20, 30, 4, 17, seed=8101, phi=0.54)
    gz, gl, gn = _seeds(33, d, 3701)

    def run():
        e = _engine(QPBatch, d)
        res = [e.reverse_duals_k(gz, gl, gn),
               *e.params_reverse_duals_k(gz, gl, gn, case["terms"], case["nparam"], want_rev=True)]
        return [np.array(a) for a in res]

    monkeypatch.delenv("DOPT_QP_JAC_CHUNK", raising=False)
    base = run()
    assert np.array_equal(base[0], base[2])
    monkeypatch.setenv("DOPT_QP_JAC_CHUNK", str(chunk))
    for a, b in zip(run(), base):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------
# 3. the other routes
# ---------------------------------------------------------------------------
def test_pivot_fallback(QPBatch, lu_mode):
    """test_qp_gpu.py's _indefinite construction: problems 1 and 4 fail the
    no-pivot threshold test and are factorised with partial pivoting."""
    d = _data(6, 60, 80, 5, 41)
    rng = np.random.default_rng(5)
    for b in (1, 4):
        S = rng.standard_normal((60, 60))
        Q = (S + S.T) / 2
        Q[np.diag_indices(60)] = 1e-4
        d["Q"][b] = Q
    gz, gl, gn = _seeds(3, d, 3800)
    e = _engine(QPBatch, d)
    _check(e.reverse_duals_k(gz, gl, gn), d, gz, gl, gn)
    want = [NOPIV, PIVOT, NOPIV, NOPIV, PIVOT, NOPIV] if lu_mode == "nopiv" else [PIVOT] * 6
    np.testing.assert_array_equal(e.lu_kind(), want)


@functools.lru_cache(maxsize=None)
def _lp():
    """The sparse LPs, three seeds per problem and −lsqr(LHS, g) of oracle/lsqr.py
    on the reference's sparse LHS, with its stop code."""
    from diffopt_amd.synthetic import lp_sparse_numpy
    from oracle.lsqr import lsqr
    d = lp_sparse_numpy(3, 300, 20, 200, 4, 101)
    gz, gl, gn = _seeds(3, d, 3900)
    n, m, p = 300, d["lam"].shape[1], 20
    ref = np.zeros((3, 3, n + m + p))
    istop = np.zeros((3, 3), dtype=int)
    for b in range(3):
        L = oqp.create_LHS_sparse(d["z"][b], d["lam"][b], d["G"][b], d["h"][b], d["A"][b], n)
        for j in range(3):
            g = np.concatenate([gz[j, b], gl[j, b], gn[j, b]])
            x, _, istop[j, b] = lsqr(lambda v: L @ v, lambda u: L.T @ u, g, n + m + p, return_info=True)
            ref[j, b] = -x
    return d, (gz, gl, gn), ref, istop


def _lp_batch(QPBatch, d, sparse):
    import scipy.sparse as sp
    B, n = d["z"].shape
    m, p = d["lam"].shape[1], d["nu"].shape[1]
    e = QPBatch(B, n, m, p, sparse=sparse)
    e.set_csc([sp.csc_matrix((n, n))] * B, d["G"], d["h"], d["A"], d["z"], d["lam"], d["nu"])
    return e


def test_lsqr_on_the_dense_route(QPBatch):
    d, (gz, gl, gn), ref, _ = _lp()
    e = _lp_batch(QPBatch, d, False)
    out = np.asarray(e.reverse_duals_k(gz, gl, gn))
    assert list(e.lu_kind()) == [LSQR] * 3
    worst = max(dc.relfro(out[j, b], ref[j, b]) for j in range(3) for b in range(3))
    print(f"worst relative Frobenius error {worst:.3e}")
    assert worst <= RTOL, worst


def test_lsqr_on_the_sparse_route(QPBatch):
    d, (gz, gl, gn), ref, istop = _lp()
    e = _lp_batch(QPBatch, d, True)
    out = np.asarray(e.reverse_duals(gz[0], gl[0], gn[0]))
    worst = max(dc.relfro(out[b], ref[0, b]) for b in range(3))
    print(f"worst relative Frobenius error {worst:.3e}")
    assert worst <= RTOL, worst
    assert list(e.lsqr_stats()[:, 0, 0]) == list(istop[0])


def test_adjoint_identity_with_the_device_forward(QPBatch, lu_mode):
    """⟨g, forward(dq, dh, db)⟩ = ⟨reverse_duals(g), forward_rhs⟩."""
    d = _data(3, 20, 30, 4, 4000)
    gz, gl, gn = _seeds(1, d, 4001)
    e = _engine(QPBatch, d)
    fwd = np.asarray(e.forward(dq=d["dq"], dh=d["dh"], db=d["db"]))
    rev = np.asarray(e.reverse_duals(gz[0], gl[0], gn[0]))
    for b in range(3):
        g = np.concatenate([gz[0, b], gl[0, b], gn[0, b]])
        r = oqp.forward_rhs(*[d[k][b] for k in KEYS], dq=d["dq"][b], dh=d["dh"][b], db=d["db"][b])
        lhs, rhs = g @ fwd[b], rev[b] @ r
        assert abs(lhs - rhs) <= ADJ_BAR * max(1.0, abs(lhs)), (lhs, rhs)


# ---------------------------------------------------------------------------
# 4. parameters
# ---------------------------------------------------------------------------
def test_parameter_gradients(QPBatch, lu_mode):
    """out_dp from the call's own out_rev: kinds 0-3 by oracle/poi.py (the
    bar of test_params_gpu.py), every kind by qp_param_cases' restatement — the
    same sum of ≤ T ≈ 100 products in the caller's order, so a relative
    Frobenius error of T·2⁻⁵³ times the sums' cancellation, held to 1e-12 —
    and the adjoint identity with params_forward_k over all three blocks."""
    case = qc.synthetic_case(3, 20, 30, 4, 16, seed=4100)
    d, terms, nparam = case["d"], case["terms"], case["nparam"]
    B, n, m, p = case["shape"]
    gz, gl, gn = _seeds(3, d, 4101)
    e = _engine(QPBatch, d)
    dp, rev = (np.asarray(a) for a in e.params_reverse_duals_k(gz, gl, gn, terms, nparam, want_rev=True))
    _check(rev, d, gz, gl, gn)
    t03 = [t for t in terms if t[1] <= 3]
    dp03 = np.asarray(e.params_reverse_duals_k(gz, gl, gn, t03, nparam))
    for j in range(3):
        for b in range(B):
            np.testing.assert_allclose(dp03[j, b], poi.reverse(t03, nparam, d["lam"][b], rev[j, b], n, m, p),
                                       rtol=1e-13, atol=1e-14)
            want = qc.poi_reverse_full(terms, nparam, d["z"][b], d["lam"][b], d["nu"][b], rev[j, b])
            assert qc.relfro(dp[j, b], want) <= 1e-12
    dpt = np.random.default_rng(4102).standard_normal((3, B, nparam))
    fwd = np.asarray(e.params_forward_k(dpt, terms))
    for j in range(3):
        for b in range(B):
            lhs = np.concatenate([gz[j, b], gl[j, b], gn[j, b]]) @ fwd[j, b]
            rhs = dp[j, b] @ dpt[j, b]
            assert abs(lhs - rhs) <= ADJ_BAR * max(1.0, abs(lhs)), (lhs, rhs)


# ---------------------------------------------------------------------------
# 5. interface
# ---------------------------------------------------------------------------
def test_device_memory_mode(QPBatch):
    import torch
    d = _data(3, 20, 30, 4, 4200)
    gz, gl, gn = _seeds(5, d, 4201)
    dev = lambda a: torch.as_tensor(a, device="cuda")
    e = QPBatch(3, 20, 30, 4)
    e.set(*[dev(d[k]) for k in KEYS])
    out = e.reverse_duals_k(dev(gz), dev(gl), dev(gn))
    assert torch.is_tensor(out) and out.is_cuda
    _check(out.cpu().numpy(), d, gz, gl, gn)


def test_model_reverse_constraint_dual():
    """MOI-sign seeds through Model: stored negated, as the dual starts are."""
    from diffopt_amd.qp import EQ, LE, Model
    d = _data(1, 12, 9, 3, 4300)
    a = {k: v[0] for k, v in d.items()}
    mod = Model()
    mod.set_problem(a["Q"], a["q"], a["G"], a["h"], a["A"], a["b"])
    mod.set_variable_primal_start(a["z"])
    mod.set_constraint_dual_start(LE, -a["lam"])
    mod.set_constraint_dual_start(EQ, -a["nu"])
    gz, gl, gn = np.zeros(12), np.zeros(9), np.zeros(3)
    gz[2], gl[1], gl[7], gn[0] = 0.7, -1.3, 0.4, 2.1
    mod.set_reverse_variable_primal(2, 0.7)
    mod.set_reverse_constraint_dual(LE, 1, 1.3)
    mod.set_reverse_constraint_dual(LE, 7, -0.4)
    mod.set_reverse_constraint_dual(EQ, 0, -2.1)
    mod.reverse_differentiate()
    want = dc.reverse_duals_flat(d, 0, gz, gl, gn)
    assert dc.relfro(np.concatenate(mod.back_grad_cache), want) <= RTOL
    # cleared with the other inputs: the unseeded path again
    mod.empty_input_sensitivities()
    mod.set_reverse_variable_primal(2, 0.7)
    mod.reverse_differentiate()
    want0 = np.concatenate(oqp.reverse_differentiate(*[a[k] for k in KEYS], gz))
    assert dc.relfro(np.concatenate(mod.back_grad_cache), want0) <= RTOL
    # ForwardConstraintDual: the forward tangents of the MOI duals
    mod.set_forward_objective_function(dq=a["dq"])
    mod.forward_differentiate()
    f = oqp.forward_differentiate(*[a[k] for k in KEYS], dq=a["dq"])
    assert abs(mod.forward_constraint_dual(LE, 1) + f[1][1]) <= RTOL * np.linalg.norm(f[1])
    assert abs(mod.forward_constraint_dual(EQ, 0) + f[2][0]) <= RTOL * np.linalg.norm(f[2])


def test_after_the_small_path(QPBatch):
    """Batch 1 at the config-1 shape: `reverse` runs the one-launch small
    path and leaves no batched factors; the new call factorises, and a
    following `forward` uses those factors."""
    from diffopt_amd.synthetic import qp_numpy
    d = qp_numpy(1, 50, 80, 30, 0.2, 20250307 + 1)
    e = _engine(QPBatch, d)
    e.reverse(d["dl_dz"])
    assert (e.lu_kind() == SMALL).all()
    gz, gl, gn = _seeds(2, d, 4400)
    _check(e.reverse_duals_k(gz, gl, gn), d, gz, gl, gn)
    assert (e.lu_kind() != SMALL).all()
    fwd = np.asarray(e.forward(dq=d["dq"], dh=d["dh"], db=d["db"]))
    ref = np.concatenate(oqp.forward_differentiate(*[d[k][0] for k in KEYS], dq=d["dq"][0], dh=d["dh"][0],
                                                   db=d["db"][0]))
    assert dc.relfro(fwd[0], ref) <= RTOL


def test_singular_problem_raises(QPBatch, lu_mode):
    """test_qp_gpu.py's test_singular_kkt_raises: λ_i == 0 and s_i == 0, a zero row of LHS."""
    from diffopt_amd import SingularException
    e = QPBatch(1, 2, 1, 0)
    e.set(np.eye(2)[None], np.array([[[1.0, 0.0]]]), np.array([[1.0]]), np.zeros((1, 0, 2)), np.array([[1.0, 2.0]]),
          np.zeros((1, 1)), np.zeros((1, 0)))
    with pytest.raises(SingularException) as want:
        e.reverse(np.ones((1, 2)))
    with pytest.raises(SingularException) as got:
        e.reverse_duals(np.ones((1, 2)), np.ones((1, 1)))
    assert got.value.info == want.value.info > 0
    assert e.info()[0] > 0


def test_refusals(QPBatch):
    from diffopt_amd import _lib
    from diffopt_amd.conic import ConicBatch
    d = _data(2, 9, 7, 2, 4500)
    B, n, m, p = 2, 9, 7, 2
    e = _engine(QPBatch, d)
    gz, gl, gn = _seeds(2, d, 4501)
    out = np.full((2, B, n + m + p), 7.0)
    ptr = lambda a: None if a is None else a.ctypes.data
    err = lambda h=e: h.lib.dopt_last_error(h.h).decode()
    call = lambda h, k, a, b, c, o: h.lib.dopt_qp_reverse_duals_k(h.h, k, ptr(a), ptr(b), ptr(c), ptr(o))
    assert call(e, 0, gz, gl, gn, out) == -1 and "k must be positive" in err()
    assert call(e, 2, None, None, None, out) == -1 and "at least one seed block" in err()
    assert call(e, 2, gz, gl, gn, None) == -1 and "out is required" in err()
    nt, par, kind, idx, var, coef = QPBatch._terms([(0, 3, 0, 1.0)], True)
    odp = np.full((2, B, 1), 7.0)
    pcall = lambda h, k, a, b, c: h.lib.dopt_qp_params_reverse_duals_k(
        h.h, k, ptr(a), ptr(b), ptr(c), 1, nt, ptr(par), ptr(kind), ptr(idx), None, ptr(coef), None, ptr(odp))
    assert pcall(e, 0, gz, gl, gn) == -1 and "k must be positive" in err()
    assert pcall(e, 2, None, None, None) == -1 and "at least one seed block" in err()
    assert (out == 7.0).all() and (odp == 7.0).all()
    ec = ConicBatch(1, 2, [(1, 2)])
    assert call(ec, 2, gz, gl, gn, out) == -1 and "non-QP handle" in err(ec)
    assert pcall(ec, 2, gz, gl, gn) == -1 and "non-QP handle" in err(ec)
    es = QPBatch(B, n, m, p, sparse=True)
    with pytest.raises(_lib.EngineError, match="multi-RHS calls need factors: not on the sparse"):
        es.reverse_duals_k(gz, gl, gn)
    with pytest.raises(_lib.EngineError, match="multi-RHS calls need factors: not on the sparse"):
        es.params_reverse_duals_k(gz[:1], gl[:1], gn[:1], [(0, 3, 0, 1.0)], 1)
