"""Parametric QPs on the GPU through the `_k` parameter calls:
dopt_qp_params_forward_k / dopt_qp_params_reverse_k (csrc/params.hip;
QPBatch.params_forward_k / params_reverse_k / params_jacobian and qp.Model's
parameter surface) against the reference's own known answers
(tests/golden/qp_param_fixtures.json), the CPU oracle's solves on the numpy
restatement's dense tangents (tests/qp_param_cases.py) and the engine's own
dense-tangent and multi-RHS calls.

Bars: 1e-6 relative Frobenius per problem against the oracle (the project's
bar); engine against engine 1e-10 on LU-route problems (the bar between the
small and the batched route) and 1e-7 on a Q = 0 problem (the
"same LSQR" bar, §2.4); forward against reverse Jacobian 1e-9 (the adjoint
test's bar, test_params_gpu.py); chunks of seeds bit-identical."""

import functools
import gc

import numpy as np
import pytest

import qp_param_cases as qc
from oracle import qp as oqp

pytestmark = pytest.mark.gpu
RTOL, LU_BAR, LSQR_BAR, ADJ_BAR = 1e-6, 1e-10, 1e-7, 1e-9
FX = qc.fixtures()
LSQR, NOPIV, PIVOT = 0, 1, 2


@functools.lru_cache(maxsize=None)
def _case(shape, nparam, phi=0.4):
    B, n, m, p = shape
    return qc.synthetic_case(B, n, m, p, nparam, seed=7000 + 10 * n + nparam, phi=phi)


@functools.lru_cache(maxsize=None)
def _oracle_rev(shape, nparam, b):
    # (the data depends on the seed, hence on nparam; the reverse outputs on no term)
    return qc.oracle_reverse_outputs(_case(shape, nparam)["d"], b)


def _engine(d, shape):
    from diffopt_amd.qp import QPBatch
    B, n, m, p = shape
    e = QPBatch(B, n, m, p)
    e.set(d["Q"], d["G"], d["h"], d["A"], d["z"], d["lam"], d["nu"])
    return e


def _unit_dp(case, j):
    return np.tile(qc.unit(case["nparam"], j), (case["shape"][0], 1))


def _check_forward_vs_engine(e, case, J0, bars, singular_ok=False, skip=()):
    """Mode 0 against the engine's own forward on the dense tangents, seed by seed."""
    B = case["shape"][0]
    for j in range(case["nparam"]):
        f = np.asarray(e.forward(singular_ok=singular_ok, **qc.dense_tangents(case, _unit_dp(case, j))))
        for b in range(B):
            if b not in skip:
                assert qc.relfro(J0[b, :, j], f[b]) <= bars[b], (j, b)


def _check_reverse_vs_engine(e, case, J1, bars, singular_ok=False, skip=()):
    """Mode 1 against reverse_k on the unit seeds + the restatement's accumulation."""
    B, n, m, p = case["shape"]
    d = case["d"]
    rev = np.asarray(e.reverse_k(np.tile(np.eye(n)[:, None, :], (1, B, 1)), singular_ok=singular_ok))
    for b in range(B):
        if b in skip:
            continue
        want = np.stack([qc.poi_reverse_full(case["terms"], case["nparam"], d["z"][b], d["lam"][b], d["nu"][b],
                                             rev[i, b]) for i in range(n)])
        assert qc.relfro(J1[b], want) <= bars[b], b


# ---------------------------------------------------------------------------
# 1. the reference's own tests (test/parameters.jl:32-101, :259-315, :570-610)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fx", FX, ids=[f["name"] for f in FX])
def test_fixture_batch_calls(fx):
    Q, G, h, A, z, lam, nu = qc.fixture_arrays(fx)
    shape = (1, fx["n"], fx["m"], fx["p"])
    n, nparam, terms = fx["n"], fx["nparam"], fx["terms"]
    e = _engine(dict(Q=Q[None], G=G[None], h=h[None], A=A[None], z=z[None], lam=lam[None], nu=nu[None]), shape)
    ok = lambda got, want: qc.isapprox(got, want, fx["rtol"], fx["atol"])
    J0 = np.asarray(e.params_jacobian(terms, nparam, "forward"))
    J1 = np.asarray(e.params_jacobian(terms, nparam, "reverse"))
    assert J0.shape == (1, sum(shape[1:]), nparam) and J1.shape == (1, n, nparam)
    for sw in fx["fwd"]:
        dp = np.array(sw["dp"])
        out = np.asarray(e.params_forward_k(dp[None, None], terms))[0, 0]
        assert all(ok(out[i], sw["dx"][i]) for i in range(n)), (sw, out)
        if sorted(dp) == [0.0] * (nparam - 1) + [1.0]:   # a unit direction: the Jacobian's column
            j = int(np.argmax(dp))
            assert all(ok(J0[0, i, j], sw["dx"][i]) for i in range(n)), (sw, J0)
    for sw in fx["rev"]:
        got = np.asarray(e.params_reverse_k(np.array(sw["dx"])[None, None], terms, nparam))[0, 0]
        assert all(ok(got[j], sw["dp"][j]) for j in range(nparam)), (sw, got)
        if sw["dx"] == [1.0]:
            assert all(ok(J1[0, 0, j], sw["dp"][j]) for j in range(nparam)), (sw, J1)


@pytest.mark.parametrize("fx", FX, ids=[f["name"] for f in FX])
def test_fixture_model_surface(fx):
    from diffopt_amd.qp import LE, Model
    Q, G, h, A, z, lam, nu = qc.fixture_arrays(fx)
    mdl = Model()
    mdl.set_problem(Q, fx["q"], G, h, param_terms=[tuple(t) for t in fx["terms"]], nparam=fx["nparam"])
    mdl.set_variable_primal_start(z)
    mdl.set_constraint_dual_start(LE, -lam)   # MOI's dual; stored with the OptNet sign flip
    ok = lambda got, want: qc.isapprox(got, want, fx["rtol"], fx["atol"])
    for sw in fx["fwd"]:
        mdl.empty_input_sensitivities()
        for j, v in enumerate(sw["dp"]):
            mdl.set_forward_parameter(j, v)
        mdl.forward_differentiate()
        assert ok(mdl.forward_variable_primal(0), sw["dx"][0]), sw
    for sw in fx["rev"]:
        mdl.empty_input_sensitivities()
        mdl.set_reverse_variable_primal(0, sw["dx"][0])
        mdl.reverse_differentiate()
        for j, want in enumerate(sw["dp"]):
            assert ok(mdl.reverse_parameter(j), want), sw
    with pytest.raises(IndexError):
        mdl.set_forward_parameter(fx["nparam"], 1.0)


def test_model_parameters_add_to_function_tangents():
    """forward_differentiate: the parameters' tangents on top of the functions'."""
    from diffopt_amd.qp import EQ, LE, Model
    case = _case(qc.SHAPES[0], 16)
    d, (B, n, m, p) = case["d"], case["shape"]
    mdl = Model()
    mdl.set_problem(d["Q"][0], d["q"][0], d["G"][0], d["h"][0], d["A"][0], d["b"][0], param_terms=case["terms"],
                    nparam=16)
    mdl.set_variable_primal_start(d["z"][0])
    mdl.set_constraint_dual_start(LE, -d["lam"][0])
    mdl.set_constraint_dual_start(EQ, -d["nu"][0])
    rng = np.random.default_rng(11)
    dp, dq, cf = rng.standard_normal(16), rng.standard_normal(n), rng.standard_normal(n)
    mdl.set_forward_objective_function(None, dq)
    mdl.set_forward_constraint_function(LE, 2, cf, 0.7)
    for j, v in enumerate(dp):
        mdl.set_forward_parameter(j, v)
    mdl.forward_differentiate()
    tq, th, tb, tG, tA = qc.poi_forward_full(case["terms"], dp, n, m, p)
    tG[2] += cf
    th[2] += -0.7
    want = np.concatenate(oqp.forward_differentiate(d["Q"][0], d["G"][0], d["h"][0], d["A"][0], d["z"][0],
                                                    d["lam"][0], d["nu"][0], dq=dq + tq, dG=tG, dh=th, dA=tA, db=tb))
    assert qc.relfro(np.concatenate(mdl.forw_grad_cache), want) <= RTOL
    mdl.set_reverse_variable_primal(1, 1.0)
    mdl.reverse_differentiate()
    rev = np.concatenate(mdl.back_grad_cache)
    wrev = np.concatenate(oqp.reverse_differentiate(d["Q"][0], d["G"][0], d["h"][0], d["A"][0], d["z"][0],
                                                    d["lam"][0], d["nu"][0], qc.unit(n, 1)))
    assert qc.relfro(rev, wrev) <= RTOL
    got = np.array([mdl.reverse_parameter(j) for j in range(16)])
    assert qc.relfro(got, qc.poi_reverse_full(case["terms"], 16, d["z"][0], d["lam"][0], d["nu"][0], wrev)) <= RTOL


# ---------------------------------------------------------------------------
# 2. synthetic shapes: the oracle, the engine's own calls, adjointness, J·dp
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nparam", qc.NPARAMS)
@pytest.mark.parametrize("shape", qc.SHAPES, ids=str)
def test_jacobian_vs_oracle_and_engine(shape, nparam):
    case = _case(shape, nparam)
    d, (B, n, m, p), terms = case["d"], shape, case["terms"]
    e = _engine(d, shape)
    J0 = np.asarray(e.params_jacobian(terms, nparam, 0))
    J1 = np.asarray(e.params_jacobian(terms, nparam, 1))
    assert J0.shape == (B, n + m + p, nparam) and J1.shape == (B, n, nparam)
    assert not e.iterative().any()
    for b in range(B):
        assert qc.relfro(J0[b], qc.oracle_forward_jacobian(case, b)) <= RTOL, b
        orev = _oracle_rev(shape, nparam, b)
        want = np.stack([qc.poi_reverse_full(terms, nparam, d["z"][b], d["lam"][b], d["nu"][b], orev[i])
                         for i in range(n)])
        assert qc.relfro(J1[b], want) <= RTOL, b
        assert qc.relfro(J0[b, :n], J1[b]) <= ADJ_BAR, b          # the z rows of mode 0 = mode 1
    _check_forward_vs_engine(e, case, J0, [LU_BAR] * B)
    _check_reverse_vs_engine(e, case, J1, [LU_BAR] * B)
    rng = np.random.default_rng(nparam)
    # params_reverse_k on k = 3 seeds = reverse_k + the restatement's accumulation
    dl = rng.standard_normal((3, B, n))
    out_dp, rev = (np.asarray(a) for a in e.params_reverse_k(dl, terms, nparam, want_rev=True))
    rk = np.asarray(e.reverse_k(dl))
    only = np.asarray(e.params_reverse_k(dl, terms, nparam))
    assert np.array_equal(only, out_dp)                            # with and without out_rev
    for s in range(3):
        for b in range(B):
            assert qc.relfro(rev[s, b], rk[s, b]) <= LU_BAR
            want = qc.poi_reverse_full(terms, nparam, d["z"][b], d["lam"][b], d["nu"][b], rk[s, b])
            assert qc.relfro(out_dp[s, b], want) <= LU_BAR
    # params_forward_k on a random dp = J·dp
    dp = rng.standard_normal((3, B, nparam))
    out = np.asarray(e.params_forward_k(dp, terms))
    for s in range(3):
        for b in range(B):
            assert qc.relfro(out[s, b], J0[b] @ dp[s, b]) <= LU_BAR
    if nparam >= 3:   # the term-less and the kind-2-only parameter: all-zero blocks
        assert not J0[:, :, nparam - 2:].any() and not J1[:, :, nparam - 2:].any()


# ---------------------------------------------------------------------------
# 3. chunk edges and mixed routes
# ---------------------------------------------------------------------------
def _mixed_case():
    """(4, 20, 30, 4) with k_act + p = n (a square, generically regular Q = 0
    system): problem 1 with Q = 0 (LSQR), problem 2 with an indefinite Q the
    no-pivot LU rejects (test_qp_gpu.py's _indefinite), the others no-pivot."""
    case = qc.synthetic_case(4, 20, 30, 4, 17, seed=8101, phi=0.54)
    d = {k: v.copy() for k, v in case["d"].items()}
    d["Q"][1] = 0.0
    S = np.random.default_rng(5).standard_normal((20, 20))
    Qi = (S + S.T) / 2
    Qi[np.diag_indices(20)] = 1e-4
    d["Q"][2] = Qi
    return dict(case, d=d)


@pytest.mark.parametrize("lu", ["nopiv", "pivot"])
def test_mixed_routes_in_one_batch(lu, monkeypatch):
    if lu == "pivot":
        monkeypatch.setenv("DOPT_LU", "0")
    else:
        monkeypatch.delenv("DOPT_LU", raising=False)
    case = _mixed_case()
    d, shape, terms, nparam = case["d"], case["shape"], case["terms"], case["nparam"]
    B, n, m, p = shape
    e = _engine(d, shape)
    J0 = np.asarray(e.params_jacobian(terms, nparam, 0))
    J1 = np.asarray(e.params_jacobian(terms, nparam, 1))
    want = [NOPIV, LSQR, PIVOT, NOPIV] if lu == "nopiv" else [PIVOT, LSQR, PIVOT, PIVOT]
    assert list(e.lu_kind()) == want
    bars = [LU_BAR, LSQR_BAR, LU_BAR, LU_BAR]
    _check_forward_vs_engine(e, case, J0, bars)
    _check_reverse_vs_engine(e, case, J1, bars)
    for b in (0, 2, 3):
        assert qc.relfro(J0[b], qc.oracle_forward_jacobian(case, b)) <= RTOL, b


@pytest.mark.parametrize("chunk", [1, 5, 16, 17])
def test_chunk_edges_are_bit_identical(chunk, monkeypatch):
    """A seed's block does not depend on how the seeds are grouped: every
    seed is a column of the multi-RHS kernel's MFMA products (and a launch of
    its own on the generic / LSQR routes).  33 forward seeds, 20 reverse
    seeds, a k = 19 call; LU, partial-pivoting and LSQR problems."""
    case = _mixed_case()
    terms = case["terms"] + [(17 + j, 3, j % 20, 1.0 + j) for j in range(16)]   # 33 parameters
    nparam = 33
    dp = np.random.default_rng(1).standard_normal((19, 4, nparam))
    dl = np.random.default_rng(2).standard_normal((19, 4, 20))

    def run():
        e = _engine(case["d"], case["shape"])
        res = [e.params_jacobian(terms, nparam, 0), e.params_jacobian(terms, nparam, 1),
               e.params_forward_k(dp, terms), *e.params_reverse_k(dl, terms, nparam, want_rev=True)]
        return [np.array(a) for a in res]

    monkeypatch.delenv("DOPT_QP_JAC_CHUNK", raising=False)
    base = run()
    monkeypatch.setenv("DOPT_QP_JAC_CHUNK", str(chunk))
    for a, b in zip(run(), base):
        assert np.array_equal(a, b)


def test_singular_problem_raises_and_spares_the_others():
    from diffopt_amd import SingularException
    case = _case(qc.SHAPES[0], 16)
    d = {k: v.copy() for k, v in case["d"].items()}
    B, n, m, p = case["shape"]
    i = int(np.flatnonzero(d["lam"][1] != 0.0)[0])          # λ_i = 0 and s_i = 0 exactly: a zero row of the LHS
    d["lam"][1, i] = 0.0
    d["h"][1, i] = oqp.gz_minus_h(d["G"][1], d["z"][1], np.zeros(m))[i]
    case = dict(case, d=d)
    e = _engine(d, case["shape"])
    for mode in (0, 1):
        with pytest.raises(SingularException):
            e.params_jacobian(case["terms"], 16, mode)
    with pytest.raises(SingularException):
        e.forward_k(dq=np.ones((2, B, n)))
    assert e.info()[1] > 0 and e.info()[0] == 0 and e.info()[2] == 0
    J0 = np.asarray(e.params_jacobian(case["terms"], 16, 0, singular_ok=True))
    J1 = np.asarray(e.params_jacobian(case["terms"], 16, 1, singular_ok=True))
    _check_forward_vs_engine(e, case, J0, [LU_BAR] * B, singular_ok=True, skip=(1,))
    _check_reverse_vs_engine(e, case, J1, [LU_BAR] * B, singular_ok=True, skip=(1,))
    for b in (0, 2):
        assert qc.relfro(J0[b], qc.oracle_forward_jacobian(case, b)) <= RTOL


# ---------------------------------------------------------------------------
# 4. memory modes, reused handles, device memory
# ---------------------------------------------------------------------------
def test_host_arrays_and_device_tensors_give_the_same_bits():
    import torch
    from diffopt_amd.qp import QPBatch
    case = _case(qc.SHAPES[0], 17)
    d, shape, terms = case["d"], case["shape"], case["terms"]
    B, n, m, p = shape
    rng = np.random.default_rng(4)
    dp, dl = rng.standard_normal((3, B, 17)), rng.standard_normal((3, B, n))
    e = _engine(d, shape)
    host = [e.params_jacobian(terms, 17, 0), e.params_jacobian(terms, 17, 1), e.params_forward_k(dp, terms),
            *e.params_reverse_k(dl, terms, 17, want_rev=True)]
    t = {k: torch.tensor(v, device="cuda") for k, v in d.items()}
    e2 = QPBatch(B, n, m, p)
    e2.set(t["Q"], t["G"], t["h"], t["A"], t["z"], t["lam"], t["nu"])
    dev = [e2.params_jacobian(terms, 17, 0, device=True), e2.params_jacobian(terms, 17, 1, device=True),
           e2.params_forward_k(torch.tensor(dp, device="cuda"), terms),
           *e2.params_reverse_k(torch.tensor(dl, device="cuda"), terms, 17, want_rev=True)]
    for a, b in zip(host, dev):
        assert b.is_cuda
        assert np.array_equal(np.asarray(a), b.cpu().numpy())


def test_reused_handle_equals_a_fresh_one():
    """Call, re-set with other data, call with a larger term table and nparam."""
    small, big = _case(qc.SHAPES[0], 16), _case(qc.SHAPES[0], 33)
    shape = qc.SHAPES[0]
    n = shape[1]
    dl = np.random.default_rng(6).standard_normal((2, shape[0], n))

    def calls(e, case):
        t, k = case["terms"], case["nparam"]
        return [np.array(a) for a in (e.params_jacobian(t, k, 0), e.params_jacobian(t, k, 1),
                                      e.params_reverse_k(dl, t, k))]

    e = _engine(small["d"], shape)
    calls(e, small)
    d = big["d"]
    e.set(d["Q"], d["G"], d["h"], d["A"], d["z"], d["lam"], d["nu"])
    again = calls(e, big)
    for a, b in zip(again, calls(_engine(d, shape), big)):
        assert np.array_equal(a, b)


def test_destroy_gives_back_every_byte(monkeypatch):
    """dopt_live_device_bytes after every new entry and the destroy equals its
    value before the create (tests/test_device_memory_gpu.py's pattern)."""
    from diffopt_amd import _lib
    gc.collect()
    live = _lib.load().dopt_live_device_bytes
    case = _case(qc.SHAPES[0], 33)
    terms, shape = case["terms"], case["shape"]
    B, n, m, p = shape
    rng = np.random.default_rng(8)
    monkeypatch.setenv("DOPT_QP_JAC_CHUNK", "16")
    before = live()
    e = _engine(case["d"], shape)
    e.params_jacobian(terms, 33, 0)
    e.params_jacobian(terms, 33, 1)
    e.params_forward_k(rng.standard_normal((18, B, 33)), terms)
    e.params_reverse_k(rng.standard_normal((18, B, n)), terms, 33)
    e.params_reverse_k(rng.standard_normal((2, B, n)), terms, 33, want_rev=True)
    held = live()
    e.params_jacobian(terms, 33, 1)
    assert live() == held > before        # repeated calls do not accumulate
    e.close()
    assert live() == before


# ---------------------------------------------------------------------------
# 5. refusals and empty calls
# ---------------------------------------------------------------------------
def _raw(e, fn, k, seeds, nparam, terms, *outs):
    nt, par, kind, idx, var, coef = e._terms(terms, True)
    ptr = lambda a: None if a is None else a.ctypes.data
    return getattr(e.lib, fn)(e.h, k, ptr(seeds), nparam, nt, ptr(par), ptr(kind), ptr(idx), ptr(var), ptr(coef),
                              *[ptr(o) for o in outs])


def test_refusals():
    from diffopt_amd import _lib
    from diffopt_amd.conic import ConicBatch
    from diffopt_amd.qp import QPBatch
    case = _case(qc.SHAPES[2], 16)          # (2, 9, 7, 0): no EqualTo rows
    B, n, m, p = case["shape"]
    e = _engine(case["d"], case["shape"])
    err = lambda: e.lib.dopt_last_error(e.h).decode()
    with pytest.raises(_lib.EngineError, match="term 1 of kind 4 needs t_var"):
        e.params_jacobian([(0, 0, 0, 1.0), (0, 4, 0, 1.0)], 1, 0)       # kind 4, t_var NULL
    with pytest.raises(_lib.EngineError, match="parameter accumulation: term 0 out of range"):
        e.params_jacobian([(0, 4, 0, 1.0, n)], 1, 0)                    # var ≥ n
    with pytest.raises(_lib.EngineError, match="parameter accumulation: term 0 out of range"):
        e.params_jacobian([(0, 5, 0, 1.0, 0)], 1, 1)                    # kind 5 with p = 0
    with pytest.raises(_lib.EngineError, match="parameter accumulation: term 0 out of range"):
        e.params_jacobian([(0, 6, 0, 1.0, 0)], 1, 0)
    with pytest.raises(_lib.EngineError, match="parameter accumulation: term 0 out of range"):
        e.params_forward(np.ones((B, 1)), [(0, 4, 0, 1.0)])            # the single calls keep refusing kind 4
    out = np.full((3, B, n + m + p), 7.0)
    assert _raw(e, "dopt_qp_params_forward_k", 3, None, 2, [(0, 0, 0, 1.0)], out) == -1
    assert "need k == nparam" in err()
    odp = np.full((3, B, 2), 7.0)
    assert _raw(e, "dopt_qp_params_reverse_k", 3, None, 2, [(0, 0, 0, 1.0)], None, odp) == -1
    assert "need k == n" in err()
    assert _raw(e, "dopt_qp_params_forward_k", -1, None, 2, [(0, 0, 0, 1.0)], out) == -1
    assert _raw(e, "dopt_qp_params_reverse_k", -1, None, 2, [(0, 0, 0, 1.0)], None, odp) == -1
    # nothing to do: nothing written, 0 returned
    assert _raw(e, "dopt_qp_params_forward_k", 0, None, 0, [], out) == 0
    assert _raw(e, "dopt_qp_params_forward_k", 0, np.ones((1, B, 2)), 2, [(0, 0, 0, 1.0)], out) == 0
    assert _raw(e, "dopt_qp_params_forward_k", 3, np.ones((3, B, 1)), 0, [], out) == 0
    assert _raw(e, "dopt_qp_params_reverse_k", 0, np.ones((1, B, n)), 2, [(0, 0, 0, 1.0)], None, odp) == 0
    assert (out == 7.0).all() and (odp == 7.0).all()
    es = QPBatch(B, n, m, p, sparse=True)
    with pytest.raises(_lib.EngineError, match="multi-RHS calls need factors"):
        es.params_jacobian([(0, 0, 0, 1.0)], 1, 0)
    with pytest.raises(_lib.EngineError, match="multi-RHS calls need factors"):
        es.params_reverse_k(np.ones((1, B, n)), [(0, 0, 0, 1.0)], 1)
    ec = ConicBatch(1, 2, [(1, 2)])
    out1 = np.zeros((1, 1, 4))
    for fn, outs in (("dopt_qp_params_forward_k", (out1,)), ("dopt_qp_params_reverse_k", (None, out1))):
        nt, par, kind, idx, var, coef = QPBatch._terms([(0, 3, 0, 1.0)], True)
        rc = getattr(ec.lib, fn)(ec.h, 1, None, 1, nt, par.ctypes.data, kind.ctypes.data, idx.ctypes.data, None,
                                 coef.ctypes.data, *[None if o is None else o.ctypes.data for o in outs])
        assert rc == -1 and "non-QP handle" in ec.lib.dopt_last_error(ec.h).decode()
