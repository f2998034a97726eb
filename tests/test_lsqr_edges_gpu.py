"""LSQR's breakdown branches, stop codes and lane widths in every LSQR kernel
(inputs: lsqr_edge_cases.py; what each does on the oracle:
test_lsqr_edge_cases_cpu.py).

Kernels and how they are reached —
  qp_lsqr_kernel                     solve_system(..., iterative=True), single and batched; QPBatch with Q = 0
  sp_lsqr_kernel<1 | 4 | 16>         QPBatch(sparse=True): forward_reverse and the separate calls
  conic_lsqr_kernel<false>           DOPT_CONIC_SPLIT=0, forward / reverse
  conic_lsqr2_kernel                 DOPT_CONIC_SPLIT=0, forward_reverse
  conic_lsqrk_kernel<4>, <2>         DOPT_CONIC_SPLIT=0, reverse_k / forward_k (<2>: with the side-62 PSD cone)
  fused split, six-launch split      DOPT_CONIC_SPLIT=1 (and DOPT_SPLIT_FUSE=0); one and four row blocks
  conic_lsqr_kernel<true, 4>         ConicBatch(sparse=True) + set_csc (the edge problem has 16.8 entries per
                                     output; <true, 1> and <true, 16> run in test_sparse_gpu.py)

Bars.  Exact cases (β = 0 at iteration 1, Mᵀb = 0, zero seed): every output,
(istop, iterations) and the LSQR norms equal the oracle's bit for bit — all of
them are single-term sums and powers of two.  Generic and mixed seeds: the
project's RTOL = 1e-6 with no relaxed output (the CPU test shows every
oracle envelope ≤ RTOL/10), the oracle's stop code, and an iteration count
within the spread the oracle itself shows under 1-ulp perturbations
(lsqr_edge_cases.*_envelope; 0 for most seeds).  And the engine's own bitwise
contracts on these inputs: forward_reverse = the separate calls, every _k seed
= its single call, a batch = its problems alone."""

import numpy as np
import pytest

import lsqr_edge_cases as ec
from test_conic_gpu import Tally, _errors, relfro
from test_conic_multi_rhs_gpu import _check_forward_k, _check_reverse_k

pytestmark = pytest.mark.gpu
RTOL = 1e-6


# ---------------------------------------------------------------------------
# plug point: qp_lsqr_kernel
# ---------------------------------------------------------------------------
def _plug_ref(c):
    from oracle import lsqr as olsqr
    x, it, istop = olsqr.lsqr_dense(c["M"], c["b"], return_info=True)
    assert (it, istop) == c["info"]
    return x


def _plug_judge(tally, c, x):
    from oracle import lsqr as olsqr
    ref = _plug_ref(c)
    if c["exact"]:
        np.testing.assert_array_equal(x, ref, err_msg=c["name"])
        return
    err = relfro(x, ref)
    print(f"[lsqr-edge] plug point, {c['name']}: {err:.2e} from the oracle")
    # the Tally rule: RTOL, or 10 × the oracle's 1-ulp envelope where that exceeds RTOL/10 (none here does)
    tally.check(err, lambda: ec.ulp_envelope(lambda bb: olsqr.lsqr_dense(c["M"], bb, return_info=True), [c["b"]], ref,
                                             trials=ec.ENV_TRIALS)[0], c["name"])


@pytest.mark.parametrize("name", list(ec.plug_cases()))
def test_plug_point_single(name):
    """x alone pins the stopping iteration (one iteration less moves it by
    > 1e-3, CPU test): the plug point returns no stop code."""
    from diffopt_amd.qp import solve_system
    c = ec.plug_cases()[name]
    tally = Tally(f"plug point: {name}")
    _plug_judge(tally, c, solve_system(c["M"], c["b"], iterative=True))
    tally.report(0)


@pytest.mark.parametrize("names", ec.PLUG_BATCHES, ids=["leave-break-iterate", "iterate-inconsistent-break"])
def test_plug_point_batched(names):
    """Three systems with three different stopping points in one launch: each
    as alone, bit for bit — one workgroup's early exit leaves its neighbours
    untouched."""
    from diffopt_amd.qp import solve_system
    cs = [ec.plug_cases()[k] for k in names]
    X = solve_system(np.stack([c["M"] for c in cs]), np.stack([c["b"] for c in cs]), iterative=True)
    tally = Tally("plug point, batched")
    for c, x in zip(cs, X):
        _plug_judge(tally, c, x)
        np.testing.assert_array_equal(x, solve_system(c["M"], c["b"], iterative=True), err_msg=c["name"])
    tally.report(0)


# ---------------------------------------------------------------------------
# sparse LP route: sp_lsqr_kernel
# ---------------------------------------------------------------------------
def _lp_batch(d, sparse=True):
    import scipy.sparse as sp
    from diffopt_amd.qp import QPBatch
    B, n = d["z"].shape
    m, p = d["lam"].shape[1], d["nu"].shape[1]
    e = QPBatch(B, n, m, p, sparse=sparse)
    e.set_csc([sp.csc_matrix((n, n))] * B, d["G"], d["h"], d["A"], d["z"], d["lam"], d["nu"])
    return e


def _lp_fused_and_separate(e, c):
    """forward_reverse and the separate calls: bit for bit, statistics
    included.  Returns (reverse, forward, stats (B, 2, 2))."""
    rev, fwd = e.forward_reverse(c["dl_dz"], dq=c["dq"], dh=c["dh"], db=c["db"])
    rev, fwd = np.array(rev), np.array(fwd)
    stats = e.lsqr_stats().copy()
    r1 = np.array(e.reverse(c["dl_dz"]))
    s_r = e.lsqr_stats()[:, 0].copy()
    f1 = np.array(e.forward(dq=c["dq"], dh=c["dh"], db=c["db"]))
    s_f = e.lsqr_stats()[:, 1].copy()
    np.testing.assert_array_equal(r1, rev)
    np.testing.assert_array_equal(f1, fwd)
    np.testing.assert_array_equal(s_r, stats[:, 0])
    np.testing.assert_array_equal(s_f, stats[:, 1])
    return rev, fwd, stats


@pytest.mark.parametrize("ci", [0, 1])
def test_sparse_lp_edge_calls(ci):
    """The extended LPs (an unused variable, a variable in one equality row
    only, an all-zero inequality row), degenerate and generic seeds side by
    side in one batch."""
    d, calls = ec.lp_case()
    c = calls[ci]
    e = _lp_batch(d)
    rev, fwd, stats = _lp_fused_and_separate(e, c)
    e.close()
    for b in range(d["z"].shape[0]):
        ref = ec.lp_oracle_run(d, b, c["dl_dz"][b], c["dq"][b], c["dh"][b], c["db"][b])
        for q, got, (x, it, istop, _, _) in zip((0, 1), (rev[b], fwd[b]), ref):
            kind = c["rev" if q == 0 else "fwd"][b]
            what = f"call {ci} problem {b} {'fwd' if q else 'rev'} ({kind})"
            if kind in ec.EXACT_KINDS:
                np.testing.assert_array_equal(got, x, err_msg=what)
                assert tuple(stats[b, q]) == (istop, it), (what, stats[b, q], (istop, it))
            else:
                err = relfro(got, x)
                spread = ec.lp_envelope(ci, b)["fwd" if q else "rev"][1]
                print(f"[lsqr-edge] sparse LP {what}: {err:.2e}, (istop, iterations) {tuple(stats[b, q])}, "
                      f"oracle {(istop, it)}, spread {spread}")
                assert err <= RTOL, (what, err)
                assert stats[b, q, 0] == istop, (what, stats[b, q], istop)
                assert abs(int(stats[b, q, 1]) - it) <= spread, (what, stats[b, q], it, spread)


@pytest.mark.parametrize("ci", [0, 1])
def test_dense_route_lp_edge_calls(ci):
    """The same LPs and calls on the dense route (Q = 0: the QP path's
    `iterative` branch, qp_lsqr_kernel on the assembled full LHS): the exact
    seeds bit for bit, the generic ones at RTOL; the fused call equal to the
    separate calls."""
    d, calls = ec.lp_case()
    c = calls[ci]
    e = _lp_batch(d, sparse=False)
    rev, fwd = e.forward_reverse(c["dl_dz"], dq=c["dq"], dh=c["dh"], db=c["db"])
    rev, fwd = np.array(rev), np.array(fwd)
    assert list(e.iterative()) == [True] * d["z"].shape[0] and list(e.lu_kind()) == [0] * d["z"].shape[0]   # LSQR
    np.testing.assert_array_equal(np.array(e.reverse(c["dl_dz"])), rev)
    np.testing.assert_array_equal(np.array(e.forward(dq=c["dq"], dh=c["dh"], db=c["db"])), fwd)
    e.close()
    for b in range(d["z"].shape[0]):
        ref = ec.lp_oracle_run(d, b, c["dl_dz"][b], c["dq"][b], c["dh"][b], c["db"][b])
        for q, got, (x, it, istop, _, _) in zip((0, 1), (rev[b], fwd[b]), ref):
            kind = c["rev" if q == 0 else "fwd"][b]
            what = f"dense route, call {ci} problem {b} {'fwd' if q else 'rev'} ({kind})"
            if kind in ec.EXACT_KINDS:
                np.testing.assert_array_equal(got, x, err_msg=what)
            else:
                err = relfro(got, x)
                print(f"[lsqr-edge] {what}: {err:.2e}")
                assert err <= RTOL, (what, err)


@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_sparse_lp_lane_widths(lanes):
    """One converging LP per instantiation of sp_lsqr_kernel (the lane count
    each input selects: CPU test): RTOL against the oracle with its stop
    codes, and the dense route's LSQR kernel on the same LPs to 1e-7."""
    d = ec.lp_lanes(lanes)
    assert ec.sp_lanes(ec.lp_entries_per_output(d)) == lanes
    c = {k: d[k] for k in ("dl_dz", "dq", "dh", "db")}
    e = _lp_batch(d)
    rev, fwd, stats = _lp_fused_and_separate(e, c)
    e.close()
    ed = _lp_batch(d, sparse=False)
    rd, fd = ed.forward_reverse(c["dl_dz"], dq=c["dq"], dh=c["dh"], db=c["db"])
    ed.close()
    for b in range(d["z"].shape[0]):
        ref = ec.lp_oracle_run(d, b, *[c[k][b] for k in ("dl_dz", "dq", "dh", "db")])
        for q, got, dense, (x, it, istop, _, _) in zip((0, 1), (rev[b], fwd[b]), (rd[b], fd[b]), ref):
            err, vs_dense = relfro(got, x), relfro(got, dense)
            print(f"[lsqr-edge] {lanes} lane(s) problem {b} {'fwd' if q else 'rev'}: {err:.2e} from the oracle, "
                  f"{vs_dense:.2e} from the dense route, (istop, iterations) {tuple(stats[b, q])}, oracle {(istop, it)}")
            assert err <= RTOL, (lanes, b, q, err)
            assert stats[b, q, 0] == istop, (lanes, b, q, stats[b, q], istop)
            assert vs_dense <= 1e-7, (lanes, b, q, vs_dense)


# ---------------------------------------------------------------------------
# conic
# ---------------------------------------------------------------------------
ROUTES = {"persistent": dict(DOPT_CONIC_SPLIT="0"),
          "split-fused": dict(DOPT_CONIC_SPLIT="1"),
          "split-six-launch": dict(DOPT_CONIC_SPLIT="1", DOPT_SPLIT_FUSE="0"),
          "sparse": dict(sparse=True)}
FWD_KEYS, REV_KEYS = ("fwd", "dx"), ("g", "dA", "db", "dc")


def _conic_handle(monkeypatch, route, cones, d, problems=None):
    """A handle on `route` holding the problems `problems` (default: all)."""
    import scipy.sparse as sp
    from diffopt_amd.conic import ConicBatch
    opts = dict(ROUTES[route])
    sparse = opts.pop("sparse", False)
    monkeypatch.delenv("DOPT_CONIC_SPLIT", raising=False)
    monkeypatch.delenv("DOPT_SPLIT_FUSE", raising=False)
    for k, v in opts.items():
        monkeypatch.setenv(k, v)
    sl = slice(None) if problems is None else problems
    args = [d[k][sl] for k in ("A", "b", "c", "x", "s", "y")]
    e = ConicBatch(args[0].shape[0], args[0].shape[2], cones, sparse=sparse)
    if sparse:
        e.set_csc([sp.csc_matrix(a) for a in args[0]], *args[1:])   # the empty column and the empty rows as CSC
    else:
        e.set(*args)
    return e


def _norms(e, which):
    return e.lsqr_norms()[which].copy()


def _run_forward(e, t):
    out, dx = e.forward(*t)
    st = e.lsqr_stats()
    return dict(fwd=np.array(out), dx=np.array(dx), istop=st["istop"].copy(), it=st["iterations"].copy(),
                norms=_norms(e, "last"))


def _run_reverse(e, dx):
    g, dA, db, dc = e.reverse(dx)
    st = e.lsqr_stats()
    return dict(g=np.array(g), dA=np.array(dA), db=np.array(db), dc=np.array(dc), istop=st["istop"].copy(),
                it=st["iterations"].copy(), norms=_norms(e, "last"))


def _run_both(e, t, dx):
    (out, fdx), (g, dA, db, dc) = e.forward_reverse(dx, *t)
    st, nr = e.lsqr_stats(), e.lsqr_norms()
    f = dict(fwd=np.array(out), dx=np.array(fdx), istop=st["fwd_istop"].copy(), it=st["fwd_iterations"].copy(),
             norms=nr["fwd"].copy())
    r = dict(g=np.array(g), dA=np.array(dA), db=np.array(db), dc=np.array(dc), istop=st["istop"].copy(),
             it=st["iterations"].copy(), norms=nr["last"].copy())
    return f, r


def _same(a, b, what, rows=slice(None), rows_b=slice(None)):
    """Two engine results bit for bit: outputs, statistics, norms."""
    for k in a:
        np.testing.assert_array_equal(a[k][rows], b[k][rows_b], err_msg=f"{what}: {k}")


NORM_KEYS = ("rnorm", "arnorm", "xnorm", "anorm")   # lsqr_norms' column order


def _vs_oracle(got, psd, b, direction, j, kind, what, row=None):
    """Problem b (row `row` of `got`, default b) of an engine result against
    the oracle's solve of seed j."""
    row = b if row is None else row
    ref = ec.conic_oracle_run(psd, b, direction, j)
    it, istop = ref["info"]
    keys = FWD_KEYS if direction == "fwd" else REV_KEYS
    if kind in ec.EXACT_KINDS:
        for k in keys:
            np.testing.assert_array_equal(got[k][row], ref[k], err_msg=f"{what}: {k}")
        assert (got["istop"][row], got["it"][row]) == (istop, it), (what, got["istop"][row], got["it"][row], ref["info"])
        np.testing.assert_array_equal(got["norms"][row], [ref["stats"][k] for k in NORM_KEYS], err_msg=f"{what}: norms")
        return
    other = ec.conic_oracle_run(psd, b, "rev" if direction == "fwd" else "fwd", j)
    full_got = {k: got[k][row] for k in keys}
    full_got.update({k: other[k] for k in (REV_KEYS if direction == "fwd" else FWD_KEYS)})
    full_ref = {**ref, **{k: other[k] for k in (REV_KEYS if direction == "fwd" else FWD_KEYS)}}
    err = {k: v for k, v in _errors(full_got, full_ref, ref["cache"]).items() if k in keys}
    spread = ec.conic_envelope(psd, b, direction, j)[1]
    print(f"[lsqr-edge] {what}: " + " ".join(f"{k}={v:.2e}" for k, v in err.items()) +
          f", (istop, iterations) {(got['istop'][row], got['it'][row])}, oracle {(istop, it)}, spread {spread}")
    assert max(err.values()) <= RTOL, (what, err)
    assert got["istop"][row] == istop, (what, got["istop"][row], istop)
    assert abs(int(got["it"][row]) - it) <= spread, (what, got["it"][row], it, spread)


# forward seed, reverse seed of a co-iterated call: one sequence breaks down at
# iteration 1 / is never live / has a zero seed while the other iterates (the
# mt[0] != mt[1] and live[0] != live[1] branches), the mirror images, both
# degenerate, both mixed
PAIRS = [(ec.BRK, ec.GEN), (ec.GEN, ec.BRK), (ec.NEV, ec.GEN), (ec.GEN, ec.NEV), (ec.ZERO, ec.GEN),
         (ec.GEN, ec.ZERO), (ec.BRK, ec.NEV), (ec.NEV, ec.BRK), (ec.BRK, ec.BRK), (ec.MIX, ec.MIX)]


@pytest.mark.parametrize("route", list(ROUTES))
def test_conic_edge_seeds(monkeypatch, route):
    """Every seed through the separate calls against the oracle; then the
    co-iterated call on the pairs above, equal to the separate calls bit for
    bit (statistics and norms included)."""
    cones, d, seeds = ec.conic_case(False)
    B = d["x"].shape[0]
    e = _conic_handle(monkeypatch, route, cones, d)
    fwd, rev = [], []
    for j, kind in enumerate(seeds["kind"]):
        t = tuple(a[j] for a in seeds["fwd"])
        fwd.append(_run_forward(e, t))
        rev.append(_run_reverse(e, seeds["rev"][j]))
        for b in range(B):
            _vs_oracle(fwd[j], False, b, "fwd", j, kind, f"{route} problem {b} forward seed {j} ({kind})")
            _vs_oracle(rev[j], False, b, "rev", j, kind, f"{route} problem {b} reverse seed {j} ({kind})")
    for jf, jr in PAIRS:
        f, r = _run_both(e, tuple(a[jf] for a in seeds["fwd"]), seeds["rev"][jr])
        _same(f, fwd[jf], f"{route} forward_reverse({seeds['kind'][jf]}, {seeds['kind'][jr]}) forward")
        _same(r, rev[jr], f"{route} forward_reverse({seeds['kind'][jf]}, {seeds['kind'][jr]}) reverse")
    e.close()


@pytest.mark.parametrize("route", list(ROUTES))
def test_conic_edge_mixed_batch(monkeypatch, route):
    """One batch holding a degenerate, a generic and a zero-seed problem:
    each problem as the oracle has it, and as it is alone on a batch-1 handle
    (the split path's batch slices; one workgroup's early exit beside its
    neighbours on the others) — separate calls and the co-iterated call."""
    cones, d, seeds = ec.conic_case(False)
    B = d["x"].shape[0]
    js = ec.CONIC_BATCH_SEEDS
    t = tuple(np.stack([a[j][b] for b, j in enumerate(js)]) for a in seeds["fwd"])
    dx = np.stack([seeds["rev"][j][b] for b, j in enumerate(js)])
    e = _conic_handle(monkeypatch, route, cones, d)
    f, r = _run_forward(e, t), _run_reverse(e, dx)
    f2, r2 = _run_both(e, t, dx)
    e.close()
    _same(f2, f, f"{route} mixed batch forward")
    _same(r2, r, f"{route} mixed batch reverse")
    for b, j in enumerate(js):
        kind = seeds["kind"][j]
        _vs_oracle(f, False, b, "fwd", j, kind, f"{route} mixed batch problem {b} forward ({kind})")
        _vs_oracle(r, False, b, "rev", j, kind, f"{route} mixed batch problem {b} reverse ({kind})")
        e1 = _conic_handle(monkeypatch, route, cones, d, problems=slice(b, b + 1))
        f1, r1 = _run_both(e1, tuple(a[b:b + 1] for a in t), dx[b:b + 1])
        e1.close()
        _same(f, f1, f"{route} problem {b} alone, forward", rows=slice(b, b + 1))
        _same(r, r1, f"{route} problem {b} alone, reverse", rows=slice(b, b + 1))


@pytest.mark.parametrize("route", list(ROUTES))
def test_conic_edge_seeds_k(monkeypatch, route):
    """reverse_k / forward_k with k = 5 — a full group of four and a
    remainder group on the persistent route's conic_lsqrk_kernel<4>: generic,
    breakdown at iteration 1, never live, generic + breakdown, all zero.
    Every seed equals its single call bit for bit, statistics included
    (a sequence dropped from the wrong list of a sweep fails here first), and
    the exact seeds equal the oracle."""
    cones, d, seeds = ec.conic_case(False)
    B = d["x"].shape[0]
    e = _conic_handle(monkeypatch, route, cones, d)
    (g, dA, db, dc), st = _check_reverse_k(e, seeds["rev"])
    (out, fdx), sf = _check_forward_k(e, *seeds["fwd"])
    e.close()
    for j, kind in enumerate(seeds["kind"]):
        if kind not in ec.EXACT_KINDS:
            continue
        for b in range(B):
            ref_r, ref_f = (ec.conic_oracle_run(False, b, q, j) for q in ("rev", "fwd"))
            for a, k in zip((g, dA, db, dc), REV_KEYS):
                np.testing.assert_array_equal(np.asarray(a)[j][b], ref_r[k], err_msg=f"{route} reverse_k seed {j}: {k}")
            for a, k in zip((out, fdx), FWD_KEYS):
                np.testing.assert_array_equal(np.asarray(a)[j][b], ref_f[k], err_msg=f"{route} forward_k seed {j}: {k}")
            assert (st["iterations"][j][b], st["istop"][j][b]) == ref_r["info"], (route, j, b)
            assert (sf["iterations"][j][b], sf["istop"][j][b]) == ref_f["info"], (route, j, b)


def test_conic_edge_seeds_k_two_wide_groups(monkeypatch):
    """The same five seeds with a side-62 PSD cone among the cones, on the
    persistent kernel (forced: m = 1974 would take the split route): the Dπ
    images leave LDS for two sequences only, so conic_lsqrk_kernel<2> runs
    groups (generic, breakdown), (never live, mixed), (zero).  (A side above
    64 — the issue's 66 — always takes the split path, conic.hip::use_split;
    62 is the side test_bitwise_two_wide_groups_large_psd uses.)"""
    cones, d, seeds = ec.conic_case(True)
    assert ec.PSD62 in cones and d["x"].shape[0] == 1
    e = _conic_handle(monkeypatch, "persistent", cones, d)
    (g, dA, db, dc), st = _check_reverse_k(e, seeds["rev"])
    (out, fdx), sf = _check_forward_k(e, *seeds["fwd"])
    e.close()
    assert np.all(st["istop"][[ec.GEN, ec.MIX]] > 0) and np.all(st["iterations"][[ec.GEN, ec.MIX]] > 10)
    for j, kind in enumerate(seeds["kind"]):
        if kind not in ec.EXACT_KINDS:
            continue
        ref_r, ref_f = (ec.conic_oracle_run(True, 0, q, j) for q in ("rev", "fwd"))
        for a, k in zip((g, dA, db, dc), REV_KEYS):
            np.testing.assert_array_equal(np.asarray(a)[j][0], ref_r[k], err_msg=f"reverse_k seed {j}: {k}")
        for a, k in zip((out, fdx), FWD_KEYS):
            np.testing.assert_array_equal(np.asarray(a)[j][0], ref_f[k], err_msg=f"forward_k seed {j}: {k}")
        assert (st["iterations"][j][0], st["istop"][j][0]) == ref_r["info"], j
        assert (sf["iterations"][j][0], sf["istop"][j][0]) == ref_f["info"], j


@pytest.mark.parametrize("route", ["split-fused", "split-six-launch"])
def test_conic_edge_seeds_split_row_blocks(monkeypatch, route):
    """The PSD(62) problem on the split path: m = 1974 is four row blocks, the
    degenerate rows sit in the last one, so a skipped Mᵀ pass (skipT) and a
    never-live sequence meet the partial-sum reduction over row blocks.  The
    exact seeds against the oracle; co-iterated with a generic sequence on
    either side, equal to the separate calls bit for bit."""
    cones, d, seeds = ec.conic_case(True)
    e = _conic_handle(monkeypatch, route, cones, d)
    fwd, rev = {}, {}
    for j, kind in enumerate(seeds["kind"]):
        if kind == "mixed":
            continue
        fwd[j] = _run_forward(e, tuple(a[j] for a in seeds["fwd"]))
        rev[j] = _run_reverse(e, seeds["rev"][j])
        if kind in ec.EXACT_KINDS:
            _vs_oracle(fwd[j], True, 0, "fwd", j, kind, f"{route}, four row blocks, forward seed {j} ({kind})")
            _vs_oracle(rev[j], True, 0, "rev", j, kind, f"{route}, four row blocks, reverse seed {j} ({kind})")
    assert fwd[ec.GEN]["istop"][0] > 0 and fwd[ec.GEN]["it"][0] > 10 and rev[ec.GEN]["it"][0] > 10
    for jf, jr in [(ec.BRK, ec.GEN), (ec.GEN, ec.BRK), (ec.NEV, ec.GEN), (ec.GEN, ec.NEV), (ec.BRK, ec.NEV)]:
        f, r = _run_both(e, tuple(a[jf] for a in seeds["fwd"]), seeds["rev"][jr])
        _same(f, fwd[jf], f"{route} forward_reverse({seeds['kind'][jf]}, {seeds['kind'][jr]}) forward")
        _same(r, rev[jr], f"{route} forward_reverse({seeds['kind'][jf]}, {seeds['kind'][jr]}) reverse")
    e.close()


def test_sparse_conic_four_lanes(monkeypatch):
    """conic_lsqr_kernel<true, 4> on a generic converging problem (16 entries
    per row of A: 13.9 per output): every output at RTOL of the oracle with
    its stop codes, and the dense persistent route to 1e-7."""
    from oracle import conic as ocn
    from test_conic_gpu import _oracle_outputs
    cones, d = ec.conic_lanes4()
    B = d["x"].shape[0]
    assert ec.sp_lanes(ec.conic_entries_per_output(d["A"])) == 4
    t = (d["dA"], d["db"], d["dc"])
    res = {}
    for route in ("sparse", "persistent"):
        e = _conic_handle(monkeypatch, route, cones, d)
        res[route] = _run_both(e, t, d["dx"])
        e.close()
    f, r = res["sparse"]
    for b in range(B):
        cache = ocn.Cache(d["A"][b], d["b"][b], d["c"][b], d["x"][b], d["s"][b], d["y"][b], cones)
        ref = _oracle_outputs(cache, d["dA"][b], d["db"][b], d["dc"][b], d["dx"][b])
        fi, ri = ref["info"]
        err = _errors({**{k: f[k][b] for k in FWD_KEYS}, **{k: r[k][b] for k in REV_KEYS}}, ref, cache)
        print(f"[lsqr-edge] sparse conic, 4 lanes, problem {b}: " + " ".join(f"{k}={v:.2e}" for k, v in err.items()))
        assert max(err.values()) <= RTOL, (b, err)
        assert (f["istop"][b], r["istop"][b]) == (fi[1], ri[1]), (b, f["istop"][b], r["istop"][b], fi, ri)
    for got, dense in zip(res["sparse"], res["persistent"]):
        for k in got:
            if k not in ("istop", "it", "norms"):
                assert relfro(got[k], dense[k]) <= 1e-7, k
