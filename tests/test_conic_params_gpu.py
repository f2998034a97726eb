"""Parametric cone programs on the GPU: dopt_conic_params_forward / _reverse /
_jacobian (csrc/params.hip; ConicBatch.params_forward / params_reverse /
params_jacobian, conic.Model's parameter surface) against the numpy
restatement of the reference's POI maps (tests/conic_poi_cases.py) and the CPU
oracle's conic solves (oracle/conic.py).

There is deliberately no adjoint-identity test here (the QP's
test_params_gpu.py has one): the reference's reverse_differentiate! runs lsqr
on M, not Mᵀ (ConicProgram.jl:372, TODO :381-384), and M is singular at every
exact primal-dual point, so its forward and reverse parameter sensitivities
are not adjoint — ⟨dx_seed, dx(dp)⟩ = 3.016 against ⟨dp_out, dp⟩ = 1.465 on the
CPU oracle for a converging n = 20 problem.

End-to-end count (test_end_to_end_vs_oracle, m69, B = 4, 16 judged outputs):
see the test's docstring."""

import json
import os

import numpy as np
import pytest

import conic_poi_cases as poi
from oracle import conic as ocn

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FX = json.load(open(os.path.join(HERE, "golden", "conic_param_fixtures.json")))
RTOL = 1e-6
M69_N = 60
SHAPES = {"rhs": (1, poi.RHS_CONES), "m69": (M69_N, poi.M69)}


def _rows(cones):
    return sum(d for _, d in cones)


def _data(B, n, cones, seed):
    from diffopt_amd.synthetic import conic_numpy_wellcond
    return conic_numpy_wellcond(B, n, cones, seed, pair_norm=1.0)


def _handle(d, B, n, cones, route="persistent", monkeypatch=None):
    """A set handle on one route: the dense persistent kernels
    (DOPT_CONIC_SPLIT=0), the split path (=1), or the sparse route (set_csc on
    a dopt_set_sparse handle).  The split switch is read when the handle is
    created."""
    from diffopt_amd.conic import ConicBatch
    if route == "sparse":
        import scipy.sparse as sp
        e = ConicBatch(B, n, cones, sparse=True)
        e.set_csc([sp.csc_matrix(a) for a in d["A"]], d["b"], d["c"], d["x"], d["s"], d["y"])
        return e
    monkeypatch.setenv("DOPT_CONIC_SPLIT", "1" if route == "split" else "0")
    e = ConicBatch(B, n, cones)
    e.set(d["A"], d["b"], d["c"], d["x"], d["s"], d["y"])
    return e


def _caches(d, B, cones):
    return [ocn.Cache(d["A"][b], d["b"][b], d["c"][b], d["x"][b], d["s"][b], d["y"][b], cones) for b in range(B)]


# ---------------------------------------------------------------------------
# 1. the reference's own test (test/parameters.jl:103-152)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fx", FX, ids=[f["name"] for f in FX])
def test_fixture_model_and_batch(fx):
    from diffopt_amd.conic import ConicBatch, Model
    cones = [tuple(c) for c in fx["cones"]]
    terms = [tuple(t) for t in fx["terms"]]
    A, n = np.array(fx["A"], dtype=float), fx["n"]
    mdl = Model()
    mdl.set_problem(A, fx["b"], fx["c"], cones, fx["max_sense"], param_terms=terms, nparam=fx["nparam"])
    mdl.set_variable_primal_start(fx["x"])
    mdl.set_constraint_primal_start(fx["s"])
    mdl.set_constraint_dual_start(fx["y"])
    e = ConicBatch(1, n, cones)
    e.set(A[None], np.array(fx["b"])[None], np.array(fx["c"])[None], np.array(fx["x"])[None],
          np.array(fx["s"])[None], np.array(fx["y"])[None])
    for sw in fx["sweeps"]:
        d = sw["direction"]
        mdl.set_forward_parameter(0, d)
        mdl.forward_differentiate()
        assert abs(mdl.forward_variable_primal(0) - sw["dx"]) <= fx["atol"], (fx["p"], d)
        mdl.set_reverse_variable_primal(0, d)
        mdl.reverse_differentiate()
        assert abs(mdl.reverse_parameter(0) - sw["dp"]) <= fx["atol"], (fx["p"], d)
        db, dc = e.params_forward(np.array([[d]]), terms)
        assert db[0, 0] == -3.0 * d and not db[0, 1:].any() and not dc.any()
        _, dx = e.forward(None, db, dc)
        assert abs(dx[0, 0] - sw["dx"]) <= fx["atol"], (fx["p"], d, dx)
        g = e.reverse(np.array([[d]]), want_dA=False)[0]
        dp = e.params_reverse(g, terms, 1)
        assert abs(dp[0, 0] - sw["dp"]) <= fx["atol"], (fx["p"], d, dp)
    J0, st0 = e.params_jacobian(terms, 1, 0)
    J1, st1 = e.params_jacobian(terms, 1, 1)
    assert J0.shape == J1.shape == (1, 1, 1)
    assert abs(J0[0, 0, 0] - 3.0) <= fx["atol"] and abs(J1[0, 0, 0] - 3.0) <= fx["atol"], (J0, J1)
    e.close()


# ---------------------------------------------------------------------------
# 2. accumulation against the numpy restatement
# ---------------------------------------------------------------------------
def _check_accumulation(e, d, B, n, cones, terms, nparam, seed):
    m = _rows(cones)
    rng = np.random.default_rng(seed)
    dp = rng.standard_normal((B, nparam))
    g = rng.standard_normal((B, n + m + 1))
    db, dc = e.params_forward(dp, terms)
    out = e.params_reverse(g, terms, nparam)
    assert db.shape == (B, m) and dc.shape == (B, n) and out.shape == (B, nparam)
    for b, cache in enumerate(_caches(d, B, cones)):
        rdb, rdc = poi.forward(terms, dp[b], n, m)
        np.testing.assert_allclose(db[b], rdb, rtol=1e-13, atol=1e-14)
        np.testing.assert_allclose(dc[b], rdc, rtol=1e-13, atol=1e-14)
        ref = poi.reverse(terms, nparam, g[b], cache.x, cache.vp)
        np.testing.assert_allclose(out[b], ref, rtol=1e-13, atol=1e-14)
    return db, dc, out


@pytest.mark.parametrize("nparam", [1, 257])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", ["rhs", "m69"])
def test_accumulation_vs_restatement(monkeypatch, shape, B, nparam):
    """nparam = 257 passes one 256-thread block of the reverse kernel; m69's
    m + n = 129 rows and rhs's 5 rows are below one of the forward kernel's.
    The table (conic_poi_cases.edge_terms) repeats a (parameter, row) pair,
    puts several parameters on one row, touches the first and last row and
    variable, and has a parameter with no term and one with a kind-2 term only."""
    n, cones = SHAPES[shape]
    d = _data(B, n, cones, 42)
    e = _handle(d, B, n, cones, "persistent", monkeypatch)
    terms = poi.edge_terms(n, _rows(cones), nparam, 100 + nparam)
    db, dc, out = _check_accumulation(e, d, B, n, cones, terms, nparam, 7)
    if nparam >= 4:
        assert not out[:, 1].any() and not out[:, 2].any()   # no term; kind 2 only
    e.close()


@pytest.mark.parametrize("shape", ["rhs", "m69"])
def test_accumulation_no_terms_and_kind2_only(monkeypatch, shape):
    n, cones = SHAPES[shape]
    B = 3
    d = _data(B, n, cones, 42)
    e = _handle(d, B, n, cones, "persistent", monkeypatch)
    for terms in ([], [(0, 2, 0, 2.5), (2, 2, 5, -1.0)]):   # (kind 2 ignores its index)
        db, dc, out = _check_accumulation(e, d, B, n, cones, terms, 3, 9)
        assert not db.any() and not dc.any() and not out.any()
    e.close()


# ---------------------------------------------------------------------------
# 3. end to end at 1e-6
# ---------------------------------------------------------------------------
def test_end_to_end_vs_oracle(monkeypatch):
    """params_forward → forward and reverse → params_reverse on m69 (B = 4,
    seed 42) against the restatement on oracle.conic, per problem four judged
    outputs: the forward solution and dx, the reverse solution g and dp.
    Metrics as test_conic_gpu._errors: relative Frobenius for the two LSQR
    solutions; dx and dp normalised by what a 1e-6-relative error of the
    solution propagates to (dp = T·[db; dc] with ‖T‖₂ ≤ ‖coefficients‖₂, on top
    of db's and dc's gains 1 + ‖vp‖, 1 + ‖x‖).  Stop codes equal the oracle's.
    An output above 1e-6 falls back to the exact min-norm bar
    (test_conic_gpu._minnorm_judge); at most a quarter of the 16 may.
    Fallbacks used on the MI355X: 0 of 16 (worst error printed by the test)."""
    from test_conic_gpu import _minnorm_judge, relcomb, relfro
    n, cones, B = M69_N, poi.M69, 4
    m = _rows(cones)
    d = _data(B, n, cones, 42)
    terms, nparam = poi.e2e_terms(n, m)
    assert nparam == 7 and sum(t[1] == 0 for t in terms) == 40 and sum(t[1] == 3 for t in terms) == 15
    dp = np.random.default_rng(3).standard_normal((B, nparam))
    e = _handle(d, B, n, cones, "persistent", monkeypatch)
    db, dc = e.params_forward(dp, terms)
    out, dx = e.forward(None, db, dc)
    f_istop = e.lsqr_stats()["istop"].copy()
    g = e.reverse(d["dx"], want_dA=False)[0]
    r_istop = e.lsqr_stats()["istop"].copy()
    dpo = e.params_reverse(g, terms, nparam)
    e.close()
    cnorm = np.linalg.norm([t[3] for t in terms])
    odb, odc = zip(*[poi.forward(terms, dp[b], n, m) for b in range(B)])
    dd = dict(dA=np.zeros((B, m, n)), db=np.stack(odb), dc=np.stack(odc), dx=d["dx"])
    judged = fallback = 0
    worst = 0.0
    for b, cache in enumerate(_caches(d, B, cones)):
        (rdx, du, dv, dw), fi = ocn.forward_differentiate(cache, None, odb[b], odc[b], return_info=True)
        (og, _), ri = ocn.reverse_differentiate(cache, d["dx"][b], return_info=True)
        assert fi[1] in (1, 2) and ri[1] in (1, 2), (b, fi, ri)
        assert (f_istop[b], r_istop[b]) == (fi[1], ri[1]), (b, f_istop[b], r_istop[b], fi, ri)
        ref = dict(fwd=np.concatenate([du, dv, [dw]]), g=og)
        rdp = poi.reverse(terms, nparam, og, cache.x, cache.vp)
        nx, nvp = np.linalg.norm(cache.x), np.linalg.norm(cache.vp)
        err = dict(fwd=relfro(out[b], ref["fwd"]),
                   dx=relcomb(dx[b], rdx, np.linalg.norm(ref["fwd"]) * (1 + nx)),
                   g=relfro(g[b], og),
                   dp=relcomb(dpo[b], rdp, np.linalg.norm(og) * (1 + max(nx, nvp)) * cnorm))
        print(f"[conic params e2e] problem {b}: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
        mn = None
        for k, v in err.items():
            judged += 1
            worst = max(worst, v)
            if v <= RTOL:
                continue
            if mn is None:
                mn = _minnorm_judge(cache, dd, b, out[b], g[b], ref)
            assert mn["fwd" if k in ("fwd", "dx") else "rev"], (b, k, v)
            fallback += 1
    print(f"[conic params e2e] {judged} outputs, {fallback} on the exact min-norm bar, worst error {worst:.2e}")
    assert judged == 16 and 4 * fallback <= judged, (judged, fallback)


# ---------------------------------------------------------------------------
# 4. the Jacobian: bit-identical to the single calls, on every route
# ---------------------------------------------------------------------------
def _terms_nparam5(n, m):
    """Five parameters (a group of four seeds plus one); parameter 3 has
    kind-2 terms only."""
    rng = np.random.default_rng(17)
    terms = []
    for p in (0, 1, 2, 4):
        terms += [(p, 0, int(rng.integers(m)), float(rng.standard_normal())) for _ in range(4)]
        terms += [(p, 3, int(rng.integers(n)), float(rng.standard_normal())) for _ in range(2)]
    terms += [(3, 2, 0, 1.0), (3, 2, 7, -2.0)]
    return [terms[i] for i in rng.permutation(len(terms))], 5, 3


JAC = {"nparam1": (lambda n, m: ([(0, 0, m - 1, 2.0), (0, 3, 0, -1.5), (0, 0, 0, 0.5)], 1, None), None),
       "nparam5": (_terms_nparam5, None),
       "nparam7_chunk3": (lambda n, m: poi.e2e_terms(n, m) + (6,), "3")}


def _forward_singles(e, terms, nparam):
    B = e.batch
    ref = []
    for j in range(nparam):
        unit = np.zeros((B, nparam))
        unit[:, j] = 1.0
        dx = np.array(e.forward(None, *e.params_forward(unit, terms))[1])
        st = e.lsqr_stats()
        ref.append((dx, st["istop"].copy(), st["iterations"].copy()))
    return ref


def _reverse_singles(e, terms, nparam):
    B, n = e.batch, e.n
    ref = []
    for i in range(n):
        unit = np.zeros((B, n))
        unit[:, i] = 1.0
        g = e.reverse(unit, want_dA=False)[0]
        st = e.lsqr_stats()
        istop, its = st["istop"].copy(), st["iterations"].copy()
        ref.append((np.array(e.params_reverse(g, terms, nparam)), istop, its))
    return ref


def _assert_blocks(J, st, ref, mode):
    for k, (blk, istop, its) in enumerate(ref):
        got = J[:, :, k] if mode == 0 else J[:, k, :]
        np.testing.assert_array_equal(got, blk, err_msg=f"mode {mode} block {k}")
        np.testing.assert_array_equal(st["istop"][k], istop, err_msg=f"mode {mode} block {k}: istop")
        np.testing.assert_array_equal(st["iterations"][k], its, err_msg=f"mode {mode} block {k}: iterations")


@pytest.mark.parametrize("cfg", list(JAC))
@pytest.mark.parametrize("route", ["persistent", "split", "sparse"])
def test_jacobian_forward_bitwise(monkeypatch, route, cfg):
    n, cones, B = M69_N, poi.M69, 2
    make, chunk = JAC[cfg]
    terms, nparam, dead = make(n, _rows(cones))
    d = _data(B, n, cones, 42)
    e = _handle(d, B, n, cones, route, monkeypatch)
    ref = _forward_singles(e, terms, nparam)
    if chunk:
        monkeypatch.setenv("DOPT_CONIC_JAC_CHUNK", chunk)
    else:
        monkeypatch.delenv("DOPT_CONIC_JAC_CHUNK", raising=False)
    J, st = e.params_jacobian(terms, nparam, 0)
    assert J.shape == (B, n, nparam) and st["istop"].shape == (nparam, B)
    _assert_blocks(J, st, ref, 0)
    for k in range(nparam):
        if k == dead:   # an exactly zero right-hand side: 0 with istop 0, no iteration
            assert not J[:, :, k].any() and not st["istop"][k].any() and not st["iterations"][k].any()
        else:
            assert J[:, :, k].any() and st["iterations"][k].all()
    from diffopt_amd import EngineError
    with pytest.raises(EngineError):   # the chunks' _k calls are not the caller's
        e.lsqr_stats_k(nparam)
    e.close()


@pytest.mark.parametrize("route", ["persistent", "split", "sparse"])
def test_jacobian_reverse_bitwise(monkeypatch, route):
    """Mode 1: n = 60 unit seeds in chunks of 16, 16, 16, 12 under the override."""
    n, cones, B = M69_N, poi.M69, 2
    terms, nparam = poi.e2e_terms(n, _rows(cones))
    d = _data(B, n, cones, 42)
    e = _handle(d, B, n, cones, route, monkeypatch)
    ref = _reverse_singles(e, terms, nparam)
    monkeypatch.setenv("DOPT_CONIC_JAC_CHUNK", "16")
    J, st = e.params_jacobian(terms, nparam, 1)
    assert J.shape == (B, n, nparam) and st["istop"].shape == (n, B)
    _assert_blocks(J, st, ref, 1)
    assert not J[:, :, 6].any()   # the kind-2-only parameter
    assert J[:, :, :6].any(axis=(0, 1)).all()
    e.close()


def test_jacobian_chunk_size_does_not_matter(monkeypatch):
    """The same Jacobian for chunks of 1, 2, 4 and the workspace bound's own choice."""
    n, cones, B = M69_N, poi.M69, 2
    terms, nparam = poi.e2e_terms(n, _rows(cones))
    d = _data(B, n, cones, 42)
    e = _handle(d, B, n, cones, "persistent", monkeypatch)
    monkeypatch.delenv("DOPT_CONIC_JAC_CHUNK", raising=False)
    J0, st0 = e.params_jacobian(terms, nparam, 0)
    for chunk in ("1", "2", "4"):
        monkeypatch.setenv("DOPT_CONIC_JAC_CHUNK", chunk)
        J, st = e.params_jacobian(terms, nparam, 0)
        np.testing.assert_array_equal(J, J0)
        np.testing.assert_array_equal(st["iterations"], st0["iterations"])
    e.close()


def test_device_arrays_equal_host_arrays(monkeypatch):
    """torch CUDA inputs and outputs (DOPT_MEM_DEVICE: the kernels read and
    write the caller's buffers) give the host-array calls' bits."""
    import torch
    n, cones, B = M69_N, poi.M69, 3
    m = _rows(cones)
    terms, nparam = poi.e2e_terms(n, m)
    d = _data(B, n, cones, 42)
    e = _handle(d, B, n, cones, "persistent", monkeypatch)
    monkeypatch.setenv("DOPT_CONIC_JAC_CHUNK", "3")
    rng = np.random.default_rng(1)
    dp, g = rng.standard_normal((B, nparam)), rng.standard_normal((B, n + m + 1))
    hdb, hdc = e.params_forward(dp, terms)
    hout = e.params_reverse(g, terms, nparam)
    hJ = [e.params_jacobian(terms, nparam, mode) for mode in (0, 1)]
    ddb, ddc = e.params_forward(torch.from_numpy(dp).cuda(), terms)
    dout = e.params_reverse(torch.from_numpy(g).cuda(), terms, nparam)
    assert ddb.is_cuda and ddc.is_cuda and dout.is_cuda
    np.testing.assert_array_equal(ddb.cpu().numpy(), hdb)
    np.testing.assert_array_equal(ddc.cpu().numpy(), hdc)
    np.testing.assert_array_equal(dout.cpu().numpy(), hout)
    for mode in (0, 1):
        J, st = e.params_jacobian(terms, nparam, mode, device=True)
        assert J.is_cuda and tuple(J.shape) == (B, n, nparam)
        np.testing.assert_array_equal(J.cpu().numpy(), hJ[mode][0])
        np.testing.assert_array_equal(st["iterations"], hJ[mode][1]["iterations"])
    e.close()


def test_jacobian_empty_sizes(monkeypatch):
    n, cones = SHAPES["rhs"]
    d = _data(2, n, cones, 42)
    e = _handle(d, 2, n, cones, "persistent", monkeypatch)
    for mode in (0, 1):
        J, st = e.params_jacobian([], 0, mode)
        assert J.shape == (2, n, 0)
    J, st = e.params_jacobian([], 2, 0)   # parameters without terms: zero blocks, istop 0
    assert J.shape == (2, n, 2) and not J.any() and not st["istop"].any()
    e.close()


# ---------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------
def test_refusals(monkeypatch):
    from diffopt_amd import EngineError
    from diffopt_amd.conic import ConicBatch
    n, cones = SHAPES["rhs"]
    m = _rows(cones)
    d = _data(1, n, cones, 42)
    e = _handle(d, 1, n, cones, "persistent", monkeypatch)
    g = np.zeros((1, n + m + 1))
    dp = np.zeros((1, 2))
    bad = {"kind 1": [(0, 1, 0, 1.0)], "kind 4": [(0, 4, 0, 1.0)], "row m": [(0, 0, m, 1.0)],
           "variable n": [(0, 3, n, 1.0)], "negative row": [(0, 0, -1, 1.0)], "parameter nparam": [(2, 0, 0, 1.0)]}
    for what, terms in bad.items():
        with pytest.raises(EngineError, match="out of range"):
            e.params_forward(dp, terms)
        with pytest.raises(EngineError, match="out of range"):
            e.params_reverse(g, terms, 2)
        for mode in (0, 1):
            with pytest.raises(EngineError, match="out of range"):
                e.params_jacobian(terms, 2, mode)
    with pytest.raises(EngineError, match="term 1 out of range"):   # the offending term is named
        e.params_forward(dp, [(0, 0, 0, 1.0), (0, 1, 0, 1.0)])
    with pytest.raises(EngineError, match="mode"):
        e.params_jacobian([(0, 0, 0, 1.0)], 2, 2)
    e.close()
    fresh = ConicBatch(1, n, cones)   # no model yet
    with pytest.raises(EngineError, match="dopt_conic_set"):
        fresh.params_reverse(g, [(0, 0, 0, 1.0)], 1)
    with pytest.raises(EngineError, match="dopt_conic_set"):
        fresh.params_jacobian([(0, 0, 0, 1.0)], 1, 0)
    fresh.close()


def test_refusals_across_back_ends(monkeypatch):
    """The conic calls on a QP handle and the QP calls on a conic handle."""
    import ctypes
    from diffopt_amd import EngineError, _lib
    from diffopt_amd.qp import QPBatch
    from diffopt_amd.synthetic import qp_numpy
    n, cones = SHAPES["rhs"]
    m = _rows(cones)
    d = _data(1, n, cones, 42)
    ce = _handle(d, 1, n, cones, "persistent", monkeypatch)
    q = qp_numpy(1, 5, 6, 2, 0.4, 3)
    qe = QPBatch(1, 5, 6, 2)
    qe.set(q["Q"], q["G"], q["h"], q["A"], q["z"], q["lam"], q["nu"])
    lib = _lib.load()
    par, kind, idx = (np.zeros(1, dtype=np.int32) for _ in range(3))
    coef, buf = np.ones(1), np.zeros(64)
    p = lambda a: a.ctypes.data
    ibuf = np.zeros(64, dtype=np.int32)
    calls = {
        "dopt_conic_params_forward": lambda h: lib.dopt_conic_params_forward(h, p(buf), 1, 1, p(par), p(kind), p(idx),
                                                                             p(coef), p(buf), p(buf)),
        "dopt_conic_params_reverse": lambda h: lib.dopt_conic_params_reverse(h, p(buf), 1, 1, p(par), p(kind), p(idx),
                                                                             p(coef), p(buf)),
        "dopt_conic_params_jacobian": lambda h: lib.dopt_conic_params_jacobian(h, 0, 1, 1, p(par), p(kind), p(idx),
                                                                               p(coef), p(buf), p(ibuf)),
    }
    for name, call in calls.items():
        with pytest.raises(EngineError, match="non-conic handle"):
            _lib.check(call(qe.h), qe.h)
    with pytest.raises(EngineError, match="non-QP handle"):
        _lib.check(lib.dopt_qp_params_reverse(ce.h, p(buf), 1, 1, p(par), p(kind), p(idx), p(coef), p(buf)), ce.h)
    with pytest.raises(EngineError, match="non-QP handle"):
        _lib.check(lib.dopt_qp_params_forward(ce.h, p(buf), 1, 1, p(par), p(kind), p(idx), p(coef), p(buf), p(buf),
                                              p(buf)), ce.h)
    assert isinstance(ce.h, ctypes.c_void_p)
    qe.close()
    ce.close()


# ---------------------------------------------------------------------------
# 6. handle reuse
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["persistent", "sparse"])
def test_jacobian_after_reset_equals_fresh_handle(monkeypatch, route):
    n, cones, B = M69_N, poi.M69, 2
    terms, nparam = poi.e2e_terms(n, _rows(cones))
    d1, d2 = _data(B, n, cones, 42), _data(B, n, cones, 43)
    monkeypatch.setenv("DOPT_CONIC_JAC_CHUNK", "5")
    e = _handle(d1, B, n, cones, route, monkeypatch)
    first = [e.params_jacobian(terms, nparam, mode) for mode in (0, 1)]
    if route == "sparse":
        import scipy.sparse as sp
        e.set_csc([sp.csc_matrix(a) for a in d2["A"]], d2["b"], d2["c"], d2["x"], d2["s"], d2["y"])
    else:
        e.set(d2["A"], d2["b"], d2["c"], d2["x"], d2["s"], d2["y"])
    again = [e.params_jacobian(terms, nparam, mode) for mode in (0, 1)]
    e.close()
    f = _handle(d2, B, n, cones, route, monkeypatch)
    fresh = [f.params_jacobian(terms, nparam, mode) for mode in (0, 1)]
    f.close()
    for mode in (0, 1):
        assert not np.array_equal(first[mode][0], again[mode][0])   # the point did change
        np.testing.assert_array_equal(again[mode][0], fresh[mode][0], err_msg=f"mode {mode}")
        for key in ("istop", "iterations"):
            np.testing.assert_array_equal(again[mode][1][key], fresh[mode][1][key], err_msg=f"mode {mode} {key}")
