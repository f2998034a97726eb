"""The LSQR edge cases (lsqr_edge_cases.py) take the branches they claim —
on the oracle alone, no GPU.  Per case: the stated (iterations, istop); by the
matvec / rmatvec call counts which branch ran (a step with β = 0 makes no
rmatvec, a start with Mᵀb = 0 makes one rmatvec and no matvec); the closed
form, bit for bit where the case is exact; for the others the oracle's own
1-ulp envelope and the spread of its iteration count, which are the bars
test_lsqr_edges_gpu.py holds the engine to; and the lane widths the sparse
inputs select, from the formulas of sparse.hip and conic.hip restated here.
Every case prints one line (pytest -s)."""

import numpy as np
import pytest

import lsqr_edge_cases as ec
from oracle import lsqr as olsqr

RTOL = 1e-6   # the project's parity bar (tests/test_conic_gpu.py)


def _report(what, info, branch, env=None, spread=None, extra=""):
    e = "" if env is None else f", 1-ulp envelope {env:.2e}"
    s = "" if spread is None else f", iteration spread {spread}"
    print(f"[lsqr-edge] {what}: (iterations, istop) = {info}, branch {branch}{e}{s}{extra}")


# ---------------------------------------------------------------------------
# plug point
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.plug_cases()))
def test_plug_case(name):
    c = ec.plug_cases()[name]
    M, b = c["M"], c["b"]
    N = M.shape[0]
    x, it, istop, nmv, nrmv, _ = ec.counted_lsqr(lambda v: M @ v, lambda u: M.T @ u, b, N)
    branch = ec.branch_of(it, istop, nmv, nrmv)
    assert (it, istop) == c["info"], (name, it, istop)
    if c["branch"] is not None:
        assert branch == c["branch"], (name, branch, nmv, nrmv)
    env, infos = ec.ulp_envelope(lambda bb: olsqr.lsqr_dense(M, bb, return_info=True), [b], x, trials=ec.ENV_TRIALS)
    assert all(i == c["info"] for i in infos), (name, infos)
    if c["exact"]:
        np.testing.assert_array_equal(x, c["x"])
    else:
        # held to the oracle at RTOL with no relaxed bar: its own noise must sit a decade below
        assert env <= RTOL / 10, f"{name}: 1-ulp envelope {env:.3e}"
        if c["x"] is not None:
            err = np.linalg.norm(x - c["x"]) / np.linalg.norm(c["x"])
            assert err <= RTOL / 10, f"{name}: {err:.3e} from the closed form (envelope {env:.3e})"
    cut = None
    if it > 0:
        # the plug point returns no stop code: x alone pins the stopping iteration
        xc = olsqr.lsqr_dense(M, b, maxiter=it - 1)
        cut = np.linalg.norm(xc - x) / np.linalg.norm(x)
        assert cut > 1e-3, f"{name}: stopping at {it - 1} moves x by {cut:.3e} only (envelope {env:.3e})"
    _report(f"plug point, {name}", (it, istop), branch, env,
            extra="" if cut is None else f", one iteration less moves x by {cut:.2e}")


def test_plug_batches_mix_equal_sizes():
    for names in ec.PLUG_BATCHES:
        cs = [ec.plug_cases()[k] for k in names]
        assert len({c["M"].shape for c in cs}) == 1 and len(cs) == 3
        assert len({c["info"] for c in cs}) == 3   # three different stopping points in one launch


# ---------------------------------------------------------------------------
# sparse LP route
# ---------------------------------------------------------------------------
LP_EXPECT = {"beta0": (1, 1), "alpha0": (0, 0), "zero": (0, 0)}


def test_lp_calls():
    d, calls = ec.lp_case()
    B, n = d["z"].shape
    m, p = d["lam"].shape[1], d["nu"].shape[1]
    per = ec.lp_entries_per_output(d)
    assert ec.sp_lanes(per) == 1, per
    for G, A in zip(d["G"], d["A"]):
        assert G[:, n - 2].nnz == 0 and A[:, n - 2].nnz == 0              # (a) an empty column
        assert G[:, n - 1].nnz == 0 and A[:, n - 1].nnz == 1 and A[p - 1, n - 1] == 0.5   # (b)
        assert A[p - 1].nnz == 1 and G[m - 1].nnz == 0                    # (b)'s row, (c) an empty row
    assert np.all(d["lam"][:, m - 1] == 0) and np.all(d["h"][:, m - 1] == 2)
    for ci, c in enumerate(calls):
        kinds = set()
        for b in range(B):
            res = ec.lp_oracle_run(d, b, c["dl_dz"][b], c["dq"][b], c["dh"][b], c["db"][b])
            for q, (x, it, istop, nmv, nrmv) in zip(("rev", "fwd"), res):
                kind = c[q][b]
                kinds.add(kind)
                branch = ec.branch_of(it, istop, nmv, nrmv)
                what = f"sparse LP call {ci} problem {b} {q} ({kind})"
                if kind in LP_EXPECT:
                    assert (it, istop) == LP_EXPECT[kind] and branch == kind, (what, it, istop, branch)
                    want = np.zeros(n + m + p)
                    if kind == "beta0":   # −8 at the new ν (reverse), 4 at z_b (forward)
                        want[n + m + p - 1 if q == "rev" else n - 1] = -8.0 if q == "rev" else 4.0
                    np.testing.assert_array_equal(x, want, err_msg=what)
                    _report(what, (it, istop), branch)
                else:
                    env, spread = ec.lp_envelope(ci, b)[q]
                    assert istop in (1, 2) and branch == "generic", (what, it, istop, branch)
                    assert env <= RTOL / 10, f"{what}: 1-ulp envelope {env:.3e}"
                    _report(what, (it, istop), branch, env, spread)
        assert {"beta0", "alpha0", "generic"} <= kinds    # one workgroup leaves early beside one that iterates
    assert any("zero" in c["fwd"] for c in calls)


@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_lp_lane_widths(lanes):
    d = ec.lp_lanes(lanes)
    B, n = d["z"].shape
    N = n + d["lam"].shape[1] + d["nu"].shape[1]
    # sparse.hip::sp_lsqr: per = 2·(nnz G + nnz A)/(B·N); dopt_internal.h::sp_lanes: ≤ 12 → 1, ≤ 48 → 4, else 16
    per = 2.0 * (sum(g.nnz for g in d["G"]) + sum(a.nnz for a in d["A"])) / (B * N)
    got = 1 if per <= 12.0 else 4 if per <= 48.0 else 16
    assert got == lanes == ec.sp_lanes(ec.lp_entries_per_output(d)), (per, got)
    infos = []
    for b in range(B):
        res = ec.lp_oracle_run(d, b, d["dl_dz"][b], d["dq"][b], d["dh"][b], d["db"][b])
        for x, it, istop, nmv, nrmv in res:
            assert istop in (1, 2) and ec.branch_of(it, istop, nmv, nrmv) == "generic", (lanes, b, it, istop)
            infos.append((it, istop))
    # the GPU file holds the sparse route to the dense route at 1e-7 on these: the oracle's own noise a decade below
    env = ec.lp_lanes_envelope(lanes)
    assert env <= 1e-8, f"{lanes} lanes: 1-ulp envelope {env:.3e}"
    print(f"[lsqr-edge] sparse LP at {lanes} lane(s): {per:.2f} entries per output (N = {N}), "
          f"(iterations, istop) per problem and direction {infos}, 1-ulp envelope {env:.2e}")


def test_existing_sparse_inputs_use_one_lane_only():
    """What the issue states about the suite before this file: every
    lp_sparse_numpy input of test_sparse_gpu.py / the smoke run / the reuse
    sequences selects 1 lane; the sparse conic inputs 16 (dense A as CSC) and
    1 (sparse_k = 5)."""
    from diffopt_amd.synthetic import conic_numpy_wellcond, lp_sparse_numpy
    for args in ((3, 300, 20, 200, 4, 101), (2, 120, 10, 80, 3, 102), (1, 60, 5, 30, 3, 104), (2, 60, 5, 30, 3, 7),
                 (2, 40, 10, 30, 3, 8601)):
        assert ec.sp_lanes(ec.lp_entries_per_output(lp_sparse_numpy(*args))) == 1, args
    m69 = [(0, 2), (1, 30), (2, 20), (3, 8), (4, 6), (4, 3)]
    assert ec.sp_lanes(ec.conic_entries_per_output(conic_numpy_wellcond(4, 60, m69, 42, pair_norm=1.0)["A"])) == 16
    cones = [(0, 10), (3, 20)] * 2 + [(1, 20)]
    d = conic_numpy_wellcond(1, 90, cones, 77, pair_norm=1.0, sparse_k=5)
    assert ec.sp_lanes(ec.conic_entries_per_output(d["A"])) == 1


# ---------------------------------------------------------------------------
# conic
# ---------------------------------------------------------------------------
CONIC_EXPECT = {"beta0": ((1, 1), (1, 1)), "alpha0": ((0, 0), (0, 1)), "zero": ((0, 0), (0, 0))}


@pytest.mark.parametrize("psd", [False, True], ids=["small", "psd62"])
def test_conic_seeds(psd):
    cones, d, seeds = ec.conic_case(psd)
    B, m, n = d["A"].shape
    va, vb, rz, rc = n - 2, n - 1, m - 3, m - 2
    assert cones[-2:] == ec.EXT_CONES and sum(dim for _, dim in cones) == m
    assert (ec.PSD62 in cones) == psd
    assert not np.any(d["A"][:, :, va]) and not np.any(d["A"][:, rc:, :])           # (a), (c)
    assert np.all(d["A"][:, rz, vb] == 0.5) and np.all(np.count_nonzero(d["A"][:, :, vb], axis=1) == 1)
    assert np.all(np.count_nonzero(d["A"][:, rz, :], axis=1) == 1)
    for b in range(B):
        cache = ec.conic_cache(cones, d, b)
        assert np.all(cache.v[rc:] == -1) and not np.any(cache.D[rc:, rc:]) and cache.D[rz, rz] == 1
        for direction in ("fwd", "rev"):
            for j, kind in enumerate(seeds["kind"]):
                r = ec.conic_oracle_run(psd, b, direction, j)
                it, istop = r["info"]
                branch = ec.branch_of(it, istop, r["nmv"], r["nrmv"])
                what = f"conic{' + PSD(62)' if psd else ''} problem {b} {direction} seed {j} ({kind})"
                if kind in CONIC_EXPECT:
                    info, calls = CONIC_EXPECT[kind]
                    assert (it, istop) == info and (r["nmv"], r["nrmv"]) == calls and branch == kind, (what, r["info"])
                    want = np.zeros(n + m + 1)
                    if kind == "beta0":   # dv = 2·e on (c)'s row (forward); g = −8 on (b)'s row (reverse)
                        want[n + (rc if direction == "fwd" else rz)] = 2.0 if direction == "fwd" else -8.0
                    np.testing.assert_array_equal(r["x"], want, err_msg=what)
                    # every derived output is a single-term sum too
                    if direction == "fwd":
                        np.testing.assert_array_equal(r["dx"], np.zeros(n))
                    else:
                        np.testing.assert_array_equal(r["dc"], np.zeros(n))
                        np.testing.assert_array_equal(r["db"], want[n:n + m])
                    st = r["stats"]
                    assert (st["rnorm"], st["arnorm"], st["anorm"]) == (0.0, 0.0, 0.0)
                    assert st["xnorm"] == np.abs(want).sum()
                    _report(what, r["info"], f"{branch} (matvec {r['nmv']}, rmatvec {r['nrmv']})")
                else:
                    assert istop in (1, 2) and branch == "generic" and r["nrmv"] == it + 1, (what, r["info"])
                    env, spread = ec.conic_envelope(psd, b, direction, j, trials=2 if psd else ec.ENV_TRIALS)
                    if not psd:   # (the PSD problem's generic seeds are held to the bitwise contracts only)
                        assert env <= RTOL / 10, f"{what}: 1-ulp envelope {env:.3e}"
                    _report(what, r["info"], branch, env, spread)
        # the degenerate component rides on the generic block: the same stop code, its own entry exact to rounding
        for direction, at, val in (("fwd", n + rc, 2.0), ("rev", n + rz, -8.0)):
            g, mx = (ec.conic_oracle_run(psd, b, direction, j) for j in (ec.GEN, ec.MIX))
            assert g["x"][at] == 0.0 and abs(mx["x"][at] - val) <= 1e-6 * abs(val), (b, direction, mx["x"][at])


def test_conic_batch_mixes_stopping_points():
    """One batch of three problems with a degenerate, a generic and a zero
    seed: three different (iterations, istop) side by side."""
    for direction in ("fwd", "rev"):
        infos = [ec.conic_oracle_run(False, b, direction, j)["info"] for b, j in enumerate(ec.CONIC_BATCH_SEEDS)]
        assert infos[0] == (1, 1) and infos[2] == (0, 0) and infos[1][0] > 10 and infos[1][1] in (1, 2), infos


def test_conic_lanes4():
    cones, d = ec.conic_lanes4()
    B, m, n = d["A"].shape
    per = 2.0 * np.count_nonzero(d["A"]) / (B * (m + n))   # conic.hip::conic_lsqr_sparse
    assert 12.0 < per <= 48.0 and ec.sp_lanes(per) == 4, per
    from oracle import conic as ocn
    infos = []
    for b in range(B):
        cache = ec.conic_cache(cones, d, b)
        _, fi = ocn.forward_differentiate(cache, d["dA"][b], d["db"][b], d["dc"][b], return_info=True)
        _, ri = ocn.reverse_differentiate(cache, d["dx"][b], return_info=True)
        assert fi[1] in (1, 2) and ri[1] in (1, 2), (b, fi, ri)
        infos.append((fi, ri))
    print(f"[lsqr-edge] sparse conic at 4 lanes: {per:.2f} entries per output, (forward, reverse) infos {infos}")


def test_two_step_breakdown_is_not_exact():
    """Two decoupled pairs with coefficients 3 and 4 and seed entries 3 and 4:
    ‖b‖ = 5 is exact but u = b/5 is not, and the oracle's β of iteration 2 is
    rounding noise, not 0 — every step makes its rmatvec.  So no case claims a
    breakdown after a normal step; the GPU file does not assert that branch."""
    c = ec.plug_cases()["two-dimensional Krylov space"]
    M = c["M"]
    _, it, istop, nmv, nrmv, _ = ec.counted_lsqr(lambda v: M @ v, lambda u: M.T @ u, c["b"], 8)
    assert (it, istop, nmv, nrmv) == (2, 1, 2, 3)
