"""One long-lived handle, model after model (the Julia QPModel / ConicModel's
pattern, an NLP model re-solved with a new active set, bench.py's, the sharded driver's): after every `set` of every
sequence of reuse_cases.py the handle must behave exactly as a fresh handle of
the same shape and environment given the same model —

* every output bit-equal to the fresh handle's (same kernels, same inputs,
  same launch geometry give the same bits), and every introspection getter of
  the wrapper equal;
* every output at the oracle bar (1e-6 relative Frobenius; QP problems on the
  LSQR branch on reverse only, as test_small_path_fallbacks; conic only on the
  steps test_reuse_cases_cpu.py proves oracle-comparable, no relaxed output).

The sequences cross the state a handle carries from its previous model
(DESIGN.md §"Per-handle state and the reused-handle tests")."""

import numpy as np
import pytest

import reuse_cases as rc
from reuse_cases import LSQR, NOPIV, PIVOT, SMALL, QP_KEYS

pytestmark = pytest.mark.gpu
RTOL = 1e-6   # relative Frobenius, north_star


def relfro(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb > 0 else 1.0)


def _np(a):
    return a if isinstance(a, np.ndarray) else a.detach().cpu().numpy()


def _same(got, want, where):
    """Bit-equality of two runs' outputs and getters."""
    assert list(got) == list(want), (where, list(got), list(want))
    for k in got:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{where}: {k}")


@pytest.fixture(scope="module")
def QPBatch():
    from diffopt_amd.qp import QPBatch
    return QPBatch


@pytest.fixture(scope="module")
def ConicBatch():
    from diffopt_amd.conic import ConicBatch
    return ConicBatch


@pytest.fixture(scope="module")
def NLPBatch():
    from diffopt_amd.nlp import NLPBatch
    return NLPBatch


@pytest.fixture(params=["nopiv", "pivot"])
def lu_mode(request, monkeypatch):
    """The factorisation (read by dopt_create): default, or partial pivoting
    for every problem (DOPT_LU=0)."""
    if request.param == "pivot":
        monkeypatch.setenv("DOPT_LU", "0")
    else:
        monkeypatch.delenv("DOPT_LU", raising=False)
    return request.param


@pytest.fixture(params=["sym", "general"])
def sym_mode(request, monkeypatch):
    """The no-pivot LU's route for P-symmetric problems (read by
    dopt_create): default, or the general one for every problem (DOPT_SYM=0)."""
    if request.param == "general":
        monkeypatch.setenv("DOPT_SYM", "0")
    else:
        monkeypatch.delenv("DOPT_SYM", raising=False)
    return request.param


@pytest.fixture
def default_env(monkeypatch):
    for v in ("DOPT_LU", "DOPT_SYM", "DOPT_LEFT", "DOPT_CONIC_SPLIT"):
        monkeypatch.delenv(v, raising=False)


# ---------------------------------------------------------------------------
# QP
# ---------------------------------------------------------------------------
def _qp_set(e, st, how=None):
    """The step's model through the step's setter.  Returns what has to stay
    alive while the model is in use (device mode borrows its inputs)."""
    d, how = st["data"], how or st["how"]
    if how == "set":
        e.set(*[d[k] for k in QP_KEYS])
        return None
    if how == "csc":
        import scipy.sparse as sp
        e.set_csc([sp.csc_matrix(q) for q in d["Q"]], [sp.csc_matrix(g) for g in d["G"]], d["h"],
                  [sp.csc_matrix(a) for a in d["A"]], d["z"], d["lam"], d["nu"])
        return None
    import torch
    t = {k: torch.as_tensor(d[k], device="cuda") for k in QP_KEYS}
    e.set(*[t[k] for k in QP_KEYS])
    return t


def _qp_getters(e, tag, out):
    out[tag + ".lu_kind"] = e.lu_kind()
    out[tag + ".sym_route"] = e.sym_route()
    out[tag + ".kept"] = e.kept()
    out[tag + ".system_size"] = e.system_size()
    out[tag + ".iterative"] = e.iterative()
    out[tag + ".info"] = e.info()


def _qp_calls(e, st, k, single_first=False, refactor=True):
    """Every solve entry point on the model just set: (single_first: reverse
    then forward on the unfactorised model, the Julia QPModel's order — the
    one-workgroup small path when the model fits it;) the fused
    forward_reverse; factor (unless `refactor` is off: the fused call's
    factors then serve) + reverse + forward; reverse_k / forward_k with k
    seeds (seed 0 is the step's own).  Outputs and getter snapshots by name."""
    d = st["data"]
    dev = st["how"] == "device"
    if dev:
        import torch
        x = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    else:
        x = np.ascontiguousarray
    seed = x(d["dl_dz"])
    fkw = dict(dq=x(d["dq"]), dh=x(d["dh"]), db=x(d["db"]))
    out = {}
    if single_first:
        out["rev_single"] = _np(e.reverse(seed))
        out["single.lu_kind_after_reverse"] = e.lu_kind()
        out["fwd_single"] = _np(e.forward(**fkw))
        _qp_getters(e, "single", out)
    rev, fwd = e.forward_reverse(seed, **fkw)
    out["rev_fused"], out["fwd_fused"] = _np(rev), _np(fwd)
    _qp_getters(e, "fused", out)
    if refactor:
        e.factor()
    out["rev_split"] = _np(e.reverse(seed))
    out["fwd_split"] = _np(e.forward(**fkw))
    _qp_getters(e, "split", out)
    roll = lambda a: np.stack([np.roll(a, j, axis=1) for j in range(k)])
    out["rev_k"] = _np(e.reverse_k(x(roll(d["dl_dz"]))))
    out["fwd_k"] = _np(e.forward_k(dq=x(roll(d["dq"])), dh=x(roll(d["dh"])), db=x(roll(d["db"]))))
    _qp_getters(e, "k", out)
    return out


def _qp_oracle_check(st, out, problems=None):
    B = st["data"]["z"].shape[0]
    for b in (range(B) if problems is None else problems):
        ref_r, ref_f = rc.qp_oracle(st, b)
        for key in ("rev_single", "rev_fused", "rev_split"):
            if key in out:
                assert relfro(out[key][b], ref_r) <= RTOL, (st["name"], b, key)
        assert relfro(out["rev_k"][0, b], ref_r) <= RTOL, (st["name"], b, "rev_k[0]")
        if ref_f is None:   # the LSQR branch: reverse only
            continue
        for key in ("fwd_single", "fwd_fused", "fwd_split"):
            if key in out:
                assert relfro(out[key][b], ref_f) <= RTOL, (st["name"], b, key)
        assert relfro(out["fwd_k"][0, b], ref_f) <= RTOL, (st["name"], b, "fwd_k[0]")


def _expected_kinds(st, lu="nopiv", final=True):
    """lu_kind per problem: the step's under the default mode; with DOPT_LU=0
    partial pivoting for every factorised problem.  `final`: after the batched
    calls that follow the small path's (they refactorise: no-pivot)."""
    k = [PIVOT if (lu == "pivot" and v != LSQR) else v for v in st["lu_kind"]]
    return [NOPIV if (final and v == SMALL) else v for v in k]


def _qp_sequence(QPBatch, shape, steps, ks=(3, 1, 5, 1, 5, 3), lu="nopiv", sym="sym", single_first=False, how=None,
                 oracle_problems=None, refactor=lambda st: True):
    """Every step on the long-lived handle `e` and on a fresh handle `f`:
    bit-equal, the step's stated properties, the oracle.  Returns the
    per-step outputs of `e`."""
    e = QPBatch(*shape)
    outs, keep = [], None
    for i, st in enumerate(steps):
        if how is not None:
            st = dict(st, how=how)
        k = ks[i % len(ks)]
        keep = _qp_set(e, st)   # (a device-mode model's tensors stay alive until the next set has returned)
        out = _qp_calls(e, st, k, single_first, refactor(st))
        f = QPBatch(*shape)
        keep_f = _qp_set(f, st)
        want = _qp_calls(f, st, k, single_first, refactor(st))
        f.close()
        del keep_f
        where = f"step {i} ({st['name']})"
        _same(out, want, where)
        np.testing.assert_array_equal(out["k.system_size"], st["nsys"], err_msg=where)
        np.testing.assert_array_equal(out["k.iterative"], st["iterative"], err_msg=where)
        np.testing.assert_array_equal(out["k.lu_kind"], _expected_kinds(st, lu), err_msg=where)
        np.testing.assert_array_equal(out["k.info"], 0, err_msg=where)
        want_sym = [int(s and lu == "nopiv" and sym == "sym") for s in st["sym"]]
        if single_first:   # after the batched calls every accepted problem is on the batched no-pivot route
            want_sym = [int(kk == NOPIV and lu == "nopiv" and sym == "sym") for kk in _expected_kinds(st, lu)]
            np.testing.assert_array_equal(out["single.lu_kind_after_reverse"], _expected_kinds(st, lu, final=False),
                                          err_msg=where)
        np.testing.assert_array_equal(out["k.sym_route"], want_sym, err_msg=where)
        for b in range(shape[0]):
            np.testing.assert_array_equal(out["k.kept"][b], rc.oracle_kept(st["data"], b), err_msg=where)
        _qp_oracle_check(st, out, oracle_problems)
        outs.append(out)
    e.close()
    del keep
    return outs


def test_batched_route_grow_shrink(QPBatch, lu_mode, sym_mode):
    """a. sizes on the batched route: N' 220 → 340 (grown) → 170 (shrunk
    below the first) → mixed within the batch → 360 (nothing eliminated) →
    the first model again, whose every output equals the first step's bit for
    bit; k of the multi-RHS calls cycles through 3, 1, 5 (their buffers resize)."""
    steps = rc.qp_sizes()
    outs = _qp_sequence(QPBatch, rc.SIZES_SHAPE, steps, lu=lu_mode, sym=sym_mode)
    _same(outs[-1], outs[0], "the first model again")   # (k = 3 at both steps)


def test_batched_route_kind_transitions(QPBatch, default_env):
    """b. one size (N' = 129), the kinds of single problems changing: accepted
    ↔ rejected (partial pivoting; n_pivot back to 0), a problem on and off the
    LSQR branch, a problem off and on the P-symmetric route (a general-route
    factorisation in K, then only-L factors over it), every problem rejected,
    all accepted.  lu_kind / iterative / sym_route as stated at every step."""
    _qp_sequence(QPBatch, rc.KINDS_SHAPE, rc.qp_kinds())


def test_tall_route_transitions(QPBatch, default_env):
    """c. reduced sizes across PIVOT_MAX = 1536 (entry-chunked solves above
    it), a rejected problem above it (generic LU) and below it (partial-
    pivoting panel), then a clean batch (n_generic back to 0, info_clear true
    again).  Oracle on problem 0.  The generic LU of a 1620-row system takes
    1.7 s: the step that runs it factorises once per handle (the fused call;
    the single solves and the multi-RHS calls use its factors), every other
    step also through dopt_qp_factor."""
    generic = lambda st: any(k == PIVOT and s > rc.PIVOT_MAX for k, s in zip(st["lu_kind"], st["nsys"]))
    _qp_sequence(QPBatch, rc.TALL_SHAPE, rc.qp_tall(), ks=(2, 1, 3), oracle_problems=[0],
                 refactor=lambda st: not generic(st))


@pytest.mark.parametrize("how,B", [("set", 2), ("csc", 1)], ids=["set_B2", "set_csc_B1"])
def test_small_batched_transitions(QPBatch, default_env, how, B):
    """d. the one-workgroup small path (N' = 96) and the batched route
    (N' = 152) by turns on one handle: the last three small steps run the
    pinned-I/O route with small_ready coming back from a batched
    factorisation.  Each step: reverse, forward (the Julia QPModel's order),
    then the batched calls."""
    _qp_sequence(QPBatch, (B,) + rc.SMALL_SHAPE, rc.qp_small_batched(B), single_first=True, how=how)


def test_staging_and_memory_mode_transitions(QPBatch, default_env):
    """e. dopt_qp_set (host) → dopt_qp_set_csc with a 30 %-dense G → device
    tensors (borrowed) → host → CSC, a new model each time."""
    _qp_sequence(QPBatch, rc.STAGING_SHAPE, rc.qp_staging())


def _set_sparse(e, on):
    from diffopt_amd import _lib
    _lib.check(e.lib.dopt_set_sparse(e.h, int(on)), e.h)


def _sym_is_cleared(e):
    """dopt_qp_get_sym on a sparse-route handle: zeros or a clear error, never
    an earlier dense factorisation's flags."""
    from diffopt_amd import EngineError
    try:
        flags = e.sym_route()
    except EngineError:
        return
    np.testing.assert_array_equal(flags, 0)


def test_sparse_toggle_on_one_handle(QPBatch, default_env):
    """f. one handle: a QP solved densely, dopt_set_sparse(1) and an LP in the
    MOI form (against a fresh sparse handle bit for bit, and the oracle at
    test_sparse_gpu.py's bar), a QP the sparse route refuses, then
    dopt_set_sparse(0) and the first QP again, bit-equal to the first step."""
    import scipy.sparse as sp
    from diffopt_amd import EngineError
    from oracle import qp as oqp
    qp, lp, refused = rc.qp_sparse_toggle()
    B, n, m, p = rc.TOGGLE_SHAPE
    e = QPBatch(B, n, m, p)
    _qp_set(e, qp)
    out0 = _qp_calls(e, qp, 3)
    assert out0["k.sym_route"].all()   # the flags the sparse route must not report
    f = QPBatch(B, n, m, p)
    _qp_set(f, qp)
    _same(out0, _qp_calls(f, qp, 3), "dense QP")
    f.close()
    _qp_oracle_check(qp, out0)

    _set_sparse(e, 1)
    _sym_is_cleared(e)
    Q0 = [sp.csc_matrix((n, n))] * B

    def lp_run(h):
        h.set_csc(Q0, lp["G"], lp["h"], lp["A"], lp["z"], lp["lam"], lp["nu"])
        rev, fwd = h.forward_reverse(lp["dl_dz"], dq=lp["dq"], dh=lp["dh"], db=lp["db"])
        out = dict(rev=rev, fwd=fwd, stats=h.lsqr_stats(), rev1=h.reverse(lp["dl_dz"]),
                   fwd1=h.forward(dq=lp["dq"], dh=lp["dh"], db=lp["db"]), stats1=h.lsqr_stats(),
                   lu_kind=h.lu_kind(), iterative=h.iterative(), system_size=h.system_size(), info=h.info(),
                   sym=h.sym_route())
        return out
    got = lp_run(e)
    f = QPBatch(B, n, m, p, sparse=True)
    _same(got, lp_run(f), "sparse LP")
    f.close()
    np.testing.assert_array_equal(got["sym"], 0)
    np.testing.assert_array_equal(got["lu_kind"], LSQR)
    np.testing.assert_array_equal(got["system_size"], n + m + p)
    assert got["iterative"].all()
    for b in range(B):
        orv, ofw, (_, isr), (_, isf) = oqp.lp_sparse_differentiate(
            lp["G"][b], lp["h"][b], lp["A"][b], lp["z"][b], lp["lam"][b], lp["nu"][b], lp["dl_dz"][b],
            lp["dq"][b], lp["dh"][b], lp["db"][b])
        assert isr in (1, 2) and isf in (1, 2)
        assert got["stats"][b, 0, 0] in (1, 2) and got["stats"][b, 1, 0] in (1, 2), got["stats"][b]
        assert relfro(got["rev"][b], orv) <= RTOL and relfro(got["fwd"][b], ofw) <= RTOL

    # Q ≠ 0 on the sparse route: the documented refusal, and no stale flags
    e.set_csc([sp.csc_matrix(q) for q in refused["Q"]], [sp.csc_matrix(g) for g in refused["G"]], refused["h"],
              [sp.csc_matrix(a) for a in refused["A"]], refused["z"], refused["lam"], refused["nu"])
    assert not e.iterative().any()
    with pytest.raises(EngineError, match="sparse direct LU"):
        e.factor()
    with pytest.raises(EngineError):
        e.forward_reverse(refused["dl_dz"], dq=refused["dq"], dh=refused["dh"], db=refused["db"])
    _sym_is_cleared(e)

    _set_sparse(e, 0)
    with pytest.raises(EngineError):   # the route change left no model
        e.reverse(qp["data"]["dl_dz"])
    _qp_set(e, qp)
    _same(_qp_calls(e, qp, 3), out0, "the first QP again, dense")
    e.close()


# ---------------------------------------------------------------------------
# conic
# ---------------------------------------------------------------------------
@pytest.fixture(params=["persistent", "split", "sparse"])
def conic_route(request, monkeypatch):
    """The conic LSQR route: the persistent kernel (DOPT_CONIC_SPLIT=0), the
    split path (=1), or A_moi kept sparse (dopt_set_sparse + set_csc)."""
    if request.param == "sparse":
        monkeypatch.delenv("DOPT_CONIC_SPLIT", raising=False)
    else:
        monkeypatch.setenv("DOPT_CONIC_SPLIT", "1" if request.param == "split" else "0")
    return request.param


@pytest.fixture(params=["persistent", "split"])
def dense_conic_route(request, monkeypatch):
    monkeypatch.setenv("DOPT_CONIC_SPLIT", "1" if request.param == "split" else "0")
    return request.param


def _conic_set(e, st, sparse):
    """The step's model under the step's cone table (assigned first, as the
    Julia shim passes a new table with every set)."""
    d = st["data"]
    e.cones = [(int(c), int(k)) for c, k in st["cones"]]
    if sparse:
        import scipy.sparse as sp
        e.set_csc([sp.csc_matrix(a) for a in d["A"]], d["b"], d["c"], d["x"], d["s"], d["y"])
    else:
        e.set(d["A"], d["b"], d["c"], d["x"], d["s"], d["y"])


def _conic_getters(e, tag, out):
    for name, val in (("lsqr_stats", e.lsqr_stats()), ("lsqr_norms", e.lsqr_norms())):
        for k, v in val.items():
            out[f"{tag}.{name}.{k}"] = v
    out[tag + ".info"] = e.info()
    out[tag + ".iterations"] = e.iterations()


def _conic_fr(e, d, tag, out):
    (o, fdx), (g, dA, db, dc) = e.forward_reverse(d["dx"], d["dA"], d["db"], d["dc"])
    out.update({f"{tag}.fwd": o, f"{tag}.dx": fdx, f"{tag}.g": g, f"{tag}.dA": dA, f"{tag}.db": db, f"{tag}.dc": dc})
    _conic_getters(e, tag, out)


def _conic_calls(e, st, k=5, light=False):
    """forward_reverse; factor + forward + reverse; reverse_k with k seeds;
    an LSQR cap set (one capped run) and lifted; forward_reverse again."""
    d = st["data"]
    out = {}
    _conic_fr(e, d, "fr", out)
    e.factor()
    o, fdx = e.forward(d["dA"], d["db"], d["dc"])
    out["split.fwd"], out["split.dx"] = o, fdx
    _conic_getters(e, "split_fwd", out)
    g, dA, db, dc = e.reverse(d["dx"])
    out.update({"split.g": g, "split.dA": dA, "split.db": db, "split.dc": dc})
    _conic_getters(e, "split_rev", out)
    if light:
        return out
    seeds = np.stack([np.roll(d["dx"], j, axis=1) for j in range(k)])
    gk, dAk, dbk, dck = e.reverse_k(seeds)
    out.update({"k.g": gk, "k.dA": dAk, "k.db": dbk, "k.dc": dck})
    for kk, v in e.lsqr_stats_k(k).items():
        out["k.stats." + kk] = v
    e.set_maxiter(50)
    _conic_fr(e, d, "capped", out)
    e.set_maxiter(0)
    _conic_fr(e, d, "again", out)
    return out


def _conic_oracle_check(st, out, name):
    from test_conic_gpu import Tally, _errors
    tally = Tally(name)
    for b in range(st["data"]["x"].shape[0]):
        ref = rc.conic_oracle(st, b)
        fi, ri = ref["info"]
        assert fi[1] in (1, 2) and ri[1] in (1, 2), (b, fi, ri)
        assert out["fr.lsqr_stats.fwd_istop"][b] in (1, 2) and out["fr.lsqr_stats.istop"][b] in (1, 2)
        for tag in ("fr", "split", "again"):
            got = {k: out[f"{tag}.{k}"][b] for k in ("fwd", "dx", "g", "dA", "db", "dc")}
            for k, v in _errors(got, ref, ref["cache"]).items():
                tally.check(v, lambda: 0.0, (st["name"], tag, b, k))   # envelope 0: no relaxed bar
        got = {k: (out[f"k.{k}"][0, b] if k in ("g", "dA", "db", "dc") else ref[k])
               for k in ("fwd", "dx", "g", "dA", "db", "dc")}
        for k, v in _errors(got, ref, ref["cache"]).items():
            tally.check(v, lambda: 0.0, (st["name"], "k[0]", b, k))
    tally.report(0)


def _conic_sequence(ConicBatch, B, n, steps, sparse, light=False, name="", maxiter=0):
    e = ConicBatch(B, n, steps[0]["cones"], sparse=sparse)
    e.set_maxiter(maxiter)
    outs = []
    for i, st in enumerate(steps):
        _conic_set(e, st, sparse)
        out = _conic_calls(e, st, light=light)
        f = ConicBatch(B, n, st["cones"], sparse=sparse)
        f.set_maxiter(maxiter)
        _conic_set(f, st, sparse)
        want = _conic_calls(f, st, light=light)
        f.close()
        where = f"step {i} ({st['name']})"
        _same(out, want, where)
        if not light:   # the cap lifted: the first call of the step again
            for k in ("fwd", "dx", "g", "dA", "db", "dc"):
                np.testing.assert_array_equal(out["again." + k], out["fr." + k], err_msg=f"{where}: again.{k}")
        if st["comparable"]:
            _conic_oracle_check(st, out, f"{name} {where}")
        outs.append(out)
    e.close()
    return outs


def test_conic_second_model(ConicBatch, conic_route):
    """g. three models under one cone table on one handle (SOC pairs changing
    between interior, dual-interior and boundary, PSD ranks changing; the
    middle model LSQR to maxiter)."""
    _conic_sequence(ConicBatch, rc.CONIC_B, rc.CONIC_N, rc.conic_second_model(), conic_route == "sparse",
                    name=f"second model ({conic_route})")


def test_conic_cone_table_changes(ConicBatch, conic_route):
    """h. the cone table changes under a fixed (n, m): a longer packed Dπ
    (one side-10 PSD block), another split of the rows, and the first table
    and model again — bit-equal to the first step."""
    outs = _conic_sequence(ConicBatch, rc.CONIC_B, rc.CONIC_N, rc.conic_tables(), conic_route == "sparse",
                           name=f"cone tables ({conic_route})")
    _same(outs[-1], outs[0], "the first table again")


def test_conic_big_psd_scratch_reuse(ConicBatch, dense_conic_route):
    """i. a PSD side of 66 (global scratch for the eigensolver and the Dπ
    apply, split path), then a table without any PSD cone (no scratch; the
    persistent kernel when that route is selected), then the first table and
    model again.  Fresh-handle comparison only.  LSQR capped at 300
    iterations on both handles: the side-66 model converges before it (236 and
    258 iterations), the SOC model would run to maxiter = 2292."""
    outs = _conic_sequence(ConicBatch, 1, rc.BIG_PSD_N, rc.conic_big_psd(), False, light=True, maxiter=300)
    assert (outs[0]["fr.lsqr_stats.iterations"] < 300).all() and (outs[0]["fr.lsqr_stats.fwd_iterations"] < 300).all()
    assert (outs[1]["fr.lsqr_stats.iterations"] == 300).all()
    _same(outs[-1], outs[0], "the side-66 table again")


def test_conic_failed_set_leaves_no_model(ConicBatch, conic_route):
    """j. a conic set that fails — a non-monotone colptr, an out-of-range
    rowval, a cone table that does not add up to m — leaves no model: the
    setters touch A (dense copy, densification, or the sparse store) before
    the verdict, so reverse / forward / factor must raise until a good set,
    which then reproduces the first outputs bit for bit."""
    import scipy.sparse as sp
    from diffopt_amd import EngineError
    sparse = conic_route == "sparse"
    st = rc.conic_second_model()[0]
    other = rc.conic_second_model()[2]["data"]   # the rejected sets carry another model's data
    d = st["data"]
    B, n, m = rc.CONIC_B, rc.CONIC_N, 69
    e = ConicBatch(B, n, st["cones"], sparse=sparse)

    def good():
        _conic_set(e, st, sparse)
        e.factor()
        out = {}
        _conic_fr(e, d, "fr", out)
        return out

    def nothing_set():
        with pytest.raises(EngineError):
            e.reverse(d["dx"])
        with pytest.raises(EngineError):
            e.forward(d["dA"], d["db"], d["dc"])
        with pytest.raises(EngineError):
            e.factor()
        with pytest.raises(EngineError):
            e.forward_reverse(d["dx"], d["dA"], d["db"], d["dc"])

    first = good()
    vecs = [other[k] for k in ("b", "c", "x", "s", "y")]

    def broken(kind):
        mats = [sp.csc_matrix(a) for a in other["A"]]
        M = mats[1].copy()
        if kind == "colptr":
            M.indptr = M.indptr.copy()
            M.indptr[3], M.indptr[4] = M.indptr[4] + 2, M.indptr[3]   # not monotone
        else:
            M.indices = M.indices.copy()
            M.indices[7] = m + 5                                        # row out of range
        mats[1] = M
        return mats

    for kind, msg in (("colptr", "colptr"), ("rowval", "rowval")):
        with pytest.raises(EngineError, match=msg):
            _raw_conic_set_csc(e, broken(kind), *vecs)
        nothing_set()
        _same(good(), first, f"good set after a bad {kind}")
    # a cone table that does not add up to m (the dense setter stages A first)
    e.cones = list(st["cones"][:-1]) + [(1, 1)]
    with pytest.raises(EngineError, match="add up"):
        if sparse:
            e.set_csc([sp.csc_matrix(a) for a in other["A"]], *vecs)
        else:
            e.set(other["A"], *vecs)
    nothing_set()
    _same(good(), first, "good set after a bad cone table")
    e.close()


# ---------------------------------------------------------------------------
# NLP
# ---------------------------------------------------------------------------
def _nlp_set(e, st):
    if st["restructure"]:
        s = st["st"]
        e.set_structure(s["con_kind"], s["has_low"], s["has_up"], s["sense"])
    e.set(*[st["data"]["pt"][k] for k in rc.NLP_KEYS])


def _nlp_getters(e, tag, out):
    out[tag + ".corrections"] = e.corrections()
    out[tag + ".system_size"] = e.system_size()
    out[tag + ".lu_kind"] = e.lu_kind()


def _nlp_calls(e, st):
    """forward_reverse on the unfactorised point; then factor + one call, four
    times (in the deferred form each call finishes its own pending
    factorisation); the getters straight after a factor()."""
    d = st["data"]
    out = {}
    out["fr.dx"], out["fr.dd"], out["fr.dp"] = e.forward_reverse(d["dp"], d["dx"], d["dd"])
    _nlp_getters(e, "fr", out)
    e.factor()
    _nlp_getters(e, "factor", out)
    e.factor()
    out["fwd.dx"], out["fwd.dd"] = e.forward(d["dp"])
    e.factor()
    out["rev.dp"] = e.reverse(d["dx"], d["dd"])
    e.factor()
    out["jac"] = e.jacobian()
    _nlp_getters(e, "last", out)
    out["rows"] = np.asarray(e.layout()["rows"])
    return out


def _nlp_oracle_check(st, out):
    from oracle import nlp as onlp
    d = st["data"]
    for b in range(rc.NLP_SHAPE[0]):
        ds, L, corr = rc.nlp_oracle(st, b)
        assert out["last.corrections"][b] == corr, (st["name"], b)
        ox, od = onlp.forward(ds, L, d["dp"][b])
        op = onlp.reverse(ds, L, d["dx"][b], d["dd"][b])
        for tag in ("fr", "fwd"):
            got = np.concatenate([out[tag + ".dx"][b], out[tag + ".dd"][b]])
            assert relfro(got, np.concatenate([ox, od])) <= RTOL, (st["name"], b, tag)
        for key in ("fr.dp", "rev.dp"):
            assert relfro(out[key][b], op) <= RTOL, (st["name"], b, key)
        assert relfro(out["jac"][b], ds) <= RTOL, (st["name"], b, "jac")


@pytest.mark.parametrize("deferred", [False, True], ids=["sync", "deferred"])
def test_nlp_structure_and_route_transitions(NLPBatch, default_env, deferred):
    """k. one NLP handle through reuse_cases.nlp_structures: dopt_nlp_set_structure
    changing num_w / nlo / nup and the rows of M on the live handle, a
    corrected problem (shift, corrections, the full M) followed by a regular
    point, an asymmetric problem (the speculative launch off) followed by a
    new structure.  In the deferred form every step also leaves a
    factorisation pending, which the next step's set drops
    (nlp_drop_pending)."""
    steps = rc.nlp_structures()
    B, n, c, P = rc.NLP_SHAPE
    e = NLPBatch(B, n, c, P, deferred=deferred)
    outs = []
    for i, st in enumerate(steps):
        _nlp_set(e, st)
        out = _nlp_calls(e, st)
        if deferred:
            e.factor()   # left pending
        f = NLPBatch(B, n, c, P, deferred=deferred)
        _nlp_set(f, dict(st, restructure=True))
        want = _nlp_calls(f, st)
        f.close()
        where = f"step {i} ({st['name']})"
        _same(out, want, where)
        for tag in ("fr", "factor", "last"):
            np.testing.assert_array_equal(out[tag + ".system_size"], st["nsys"], err_msg=where)
            np.testing.assert_array_equal(out[tag + ".corrections"] != 0, [b in st["corrected"] for b in range(B)],
                                          err_msg=where)
        _nlp_oracle_check(st, out)
        outs.append(out)
    e.close()
    _same(outs[-1], outs[0], "the first structure and point again")


def _raw_conic_set_csc(e, mats, b, c, x, s, y):
    """dopt_conic_set_csc on the CSC arrays of `mats` as they are (ConicBatch.set_csc
    converts through scipy, which may canonicalise broken arrays)."""
    from diffopt_amd import _lib
    from diffopt_amd._arrays import vector
    B, n, m = e.batch, e.n, e.m
    cps, rvs, nzs, off = [], [], [], 0
    for M in mats:
        cps.append(np.asarray(M.indptr, dtype=np.int64) + off + 1)
        rvs.append(np.asarray(M.indices, dtype=np.int64) + 1)
        nzs.append(np.asarray(M.data, dtype=np.float64))
        off += len(M.data)
    cp, rv, nz = (np.ascontiguousarray(np.concatenate(v)) for v in (cps, rvs, nzs))
    st = e._stage([b, c, x, s, y])
    vecs = [vector(b, (B, m)), vector(c, (B, n)), vector(x, (B, n)), vector(s, (B, m)), vector(y, (B, m))]
    desc = np.array([v for cd in e.cones for v in cd], dtype=np.int32)
    rc_ = e.lib.dopt_conic_set_csc(e.h, cp.ctypes.data, rv.ctypes.data, nz.ctypes.data, off,
                                   *[st.ptr(v) for v in vecs], desc.ctypes.data, len(e.cones))
    _lib.check(rc_, e.h)
