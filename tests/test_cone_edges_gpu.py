"""Cone projections and Dπ at their edges on every conic route (inputs and
bars: cone_edge_cases.py; what each case is on the oracle, and the measured
spreads the bars come from: test_cone_edge_cases_cpu.py).

Routes and the kernels that call dpi_apply —
  R1  DOPT_CONIC_SPLIT=0, forward / reverse                 conic_lsqr_kernel<false>
  R2  DOPT_CONIC_SPLIT=0, forward_reverse                   conic_lsqr2_kernel
  R3  DOPT_CONIC_SPLIT=0, reverse_k / forward_k, k = 4      conic_lsqrk_kernel<4> (<2> with a side-63 / 64 cone)
  R4  DOPT_CONIC_SPLIT=1, DOPT_SPLIT_FUSE=0                 conic_split_dpi_kernel
  R5  DOPT_CONIC_SPLIT=1                                    conic_fsplit_dpiU_kernel / dpiV_kernel
  R6  ConicBatch(sparse=True) + set_csc, half of A zero     conic_lsqr_kernel<true, 1>
psd_big and psd_table (sides above 64) run on R4 and R5 only: conic.hip's
use_split sends such a table to the split path whatever the environment says,
and the sparse route is persistent.

LSQR is capped at k = 1, 2, 3: the engine does the oracle's k steps and stops
as it does, (k, 7); every output is held to bar(case) = max(10 × the oracle's
own measured spread, 1e-12) — about six orders below the project's 1e-6,
which an eigensolver converged to 1e-9, a lost orthogonality of U or one wrong
weight on a tie would pass.  A failure names the cone slice with the largest
error.  The π probe reads conic_cone_kernel's π out of db with no LSQR noise:
bit for bit on the exact cones."""

import json
import os

import numpy as np
import pytest

import cone_edge_cases as ec
from oracle import cones as C
from test_conic_multi_rhs_gpu import _check_forward_k, _check_reverse_k
from test_lsqr_edges_gpu import _conic_handle, _run_both, _run_forward, _run_reverse, _same

pytestmark = pytest.mark.gpu

# route → (test_lsqr_edges_gpu.ROUTES' name, how the calls are made)
ROUTES = {"R1": ("persistent", "separate"), "R2": ("persistent", "both"), "R3": ("persistent", "k"),
          "R4": ("split-six-launch", "both"), "R5": ("split-fused", "both"), "R6": ("sparse", "both")}
SPLIT_ONLY = ec.SPLIT_ONLY
# one test per family and route; psd_table one per table (a side-256 / 257 Jacobi each)
GROUPS = [(f, [ti]) for f in ec.FAMILIES for ti in range(len(ec.TABLES[f])) if f == "psd_table"] + \
         [(f, list(range(len(ec.TABLES[f])))) for f in ec.FAMILIES if f != "psd_table"]
GROUPS.sort(key=lambda g: ec.FAMILIES.index(g[0]))
COMBOS = [(f, tis, r) for f, tis in GROUPS for r in ROUTES if f not in SPLIT_ONLY or r in ("R4", "R5")]


def _id(c):
    f, tis, r = c
    return f"{f}{tis[0] if f == 'psd_table' else ''}-{r}"


def _data(d, sparse):
    return dict(d, A=d["A_sparse"]) if sparse else d


def _worst_cone(d, p, got, ref):
    """The cone slice of the m part of fwd and g with the largest error
    (relative to the whole vector), named."""
    n, off = d["n"], C.cone_offsets(d["cones"])
    worst = (0.0, "no cone slice differs: the n part or the end")
    for key in ("fwd", "g"):
        diff, nr = got[key][n:n + d["m"]] - ref[key][n:n + d["m"]], np.linalg.norm(ref[key])
        for i in range(len(d["cones"])):
            e = np.linalg.norm(diff[off[i]:off[i + 1]]) / nr
            if e > worst[0]:
                worst = (e, f"{key}, {ec.cone_label(d, p, i)}: {e:.2e}")
    return worst[1]


def _judge(family, ti, d, route, k, p, got, sparse):
    """Problem p at cap k against the oracle: the stop, then every output
    within the bar.  Returns the worst error."""
    ref = ec.reference(family, ti, p, k, sparse)
    what = f"{family} table {ti} {route} cap {k} problem {p}"
    assert ((got["fwd_it"], got["fwd_istop"]), (got["it"], got["istop"])) == ref["info"], (what, got["fwd_it"],
                                                                                         got["fwd_istop"], ref["info"])
    err = ec.errors(got, ref, ref["cache"])
    bar = ec.bar(family, ti, p)
    print(f"[cone-edge] {what}: " + " ".join(f"{key}={v:.2e}" for key, v in err.items()) + f", bar {bar:.1e}")
    assert max(err.values()) <= bar, (what, err, bar, _worst_cone(d, p, got, ref))
    return max(err.values())


def _rows(f, r, p):
    out = {key: f[key][p] for key in ec.FWD_KEYS}
    out.update({key: r[key][p] for key in ec.REV_KEYS})
    out.update(fwd_it=f["it"][p], fwd_istop=f["istop"][p], it=r["it"][p], istop=r["istop"][p])
    return out


def _log(family, route, k, worst, bar):
    log = os.environ.get("DOPT_PARITY_LOG")
    if log:
        with open(log, "a") as fh:
            fh.write(json.dumps(dict(test=f"cone edges: {family} {route}", cap=k, worst=worst, bar=bar)) + "\n")


@pytest.mark.parametrize("family,tables,route", COMBOS, ids=[_id(c) for c in COMBOS])
def test_cone_edges(monkeypatch, family, tables, route):
    name, how = ROUTES[route]
    sparse = name == "sparse"
    for ti in tables:
        d = _data(ec.batch(family, ti), sparse)
        B = d["B"]
        e = _conic_handle(monkeypatch, name, d["cones"], d)
        t = (d["dA"], d["db"], d["dc"])
        for k in ec.CAPS:
            e.set_maxiter(k)
            if how == "k":      # every seed bit for bit its single call (the helpers assert it); seed 0 is t, dx
                sk = d["seeds_k"]
                (g, dA, db, dc), st = _check_reverse_k(e, sk["dx"])
                (out, fdx), sf = _check_forward_k(e, sk["dA"], sk["db"], sk["dc"])
                f = dict(fwd=np.asarray(out)[0], dx=np.asarray(fdx)[0], it=sf["iterations"][0], istop=sf["istop"][0])
                r = dict(g=np.asarray(g)[0], dA=np.asarray(dA)[0], db=np.asarray(db)[0], dc=np.asarray(dc)[0],
                         it=st["iterations"][0], istop=st["istop"][0])
            elif how == "separate":
                f, r = _run_forward(e, t), _run_reverse(e, d["dx"])
            else:
                f, r = _run_both(e, t, d["dx"])
                if route == "R2":   # the co-iterated kernel: bit for bit the separate calls
                    _same(f, _run_forward(e, t), f"{family} table {ti} cap {k}: R2 forward against R1")
                    _same(r, _run_reverse(e, d["dx"]), f"{family} table {ti} cap {k}: R2 reverse against R1")
            worst = max(_judge(family, ti, d, route, k, p, _rows(f, r, p), sparse) for p in range(B))
            _log(f"{family} table {ti}", route, k, worst, max(ec.bar(family, ti, p) for p in range(B)))
        e.close()


def test_fused_split_batch_equals_problems_alone(monkeypatch):
    """R5 on psd_small: the batch of 3 (slices of 2 and 1 problems) bit for
    bit each problem alone — a parameter offset taken from the wrong problem
    shows here as well as against the oracle."""
    d = ec.batch("psd_small", 0)
    t = (d["dA"], d["db"], d["dc"])
    for k in ec.CAPS:
        e = _conic_handle(monkeypatch, "split-fused", d["cones"], d)
        e.set_maxiter(k)
        f, r = _run_both(e, t, d["dx"])
        e.close()
        for p in range(d["B"]):
            e1 = _conic_handle(monkeypatch, "split-fused", d["cones"], d, problems=slice(p, p + 1))
            e1.set_maxiter(k)
            f1, r1 = _run_both(e1, tuple(a[p:p + 1] for a in t), d["dx"][p:p + 1])
            e1.close()
            _same(f, f1, f"cap {k} problem {p} alone, forward", rows=slice(p, p + 1))
            _same(r, r1, f"cap {k} problem {p} alone, reverse", rows=slice(p, p + 1))


PROBE_ROUTES = ("R1", "R4", "R6")
PROBES = [(f, tis, r) for f, tis in GROUPS for r in PROBE_ROUTES if f not in SPLIT_ONLY or r == "R4"]


@pytest.mark.parametrize("family,tables,route", PROBES, ids=[_id(c) for c in PROBES])
def test_pi_probe(monkeypatch, family, tables, route):
    """n = 1, A = 0, b = 0, c = [1], x = [0], dx = [4]: one exact LSQR step,
    g = (0, …, 0, 4) and db = −4·π(v).  Exact cones: π bit for bit the
    oracle's.  The others: ‖π − oracle‖ ≤ bar·‖v‖ per cone (π is
    1-Lipschitz, so ‖v‖ is its scale; a π that is 0 but for rounding has no
    scale of its own)."""
    name = ROUTES[route][0]
    for ti in tables:
        d = ec.probe(family, ti)
        off = C.cone_offsets(d["cones"])
        e = _conic_handle(monkeypatch, name, d["cones"], d)
        r = _run_reverse(e, d["dx"])
        e.close()
        worst = 0.0
        for p in range(d["B"]):
            g, _, info, vp = ec.probe_reference(family, ti, p)
            what = f"{family} table {ti} {route} probe, problem {p}"
            assert (r["it"][p], r["istop"][p]) == info == (1, 1), (what, r["it"][p], r["istop"][p])
            np.testing.assert_array_equal(r["g"][p], g, err_msg=what)
            pi = r["db"][p] / -4.0
            v = d["y"][p] - d["s"][p]
            bar = ec.bar(family, ti, p)
            for i, (_, exact, _) in enumerate(d["info"][p]):
                sl = slice(off[i], off[i + 1])
                if exact:
                    np.testing.assert_array_equal(pi[sl], vp[sl], err_msg=f"{what}, {ec.cone_label(d, p, i)}")
                else:
                    err = np.linalg.norm(pi[sl] - vp[sl]) / np.linalg.norm(v[sl])
                    worst = max(worst, err)
                    assert err <= bar, (what, ec.cone_label(d, p, i), err, bar)
        print(f"[cone-edge] {family} table {ti} {route} probe: worst π error {worst:.2e}")
        _log(f"{family} table {ti} probe", route, 0, worst, max(ec.bar(family, ti, p) for p in range(d["B"])))


def test_negative_and_unknown_cones_rejected():
    """dim == 0 is accepted for Zeros, Nonnegatives, Nonpositives and the PSD
    triangle (the empty_cones family runs them); an empty SecondOrderCone and
    a negative dimension are refused when the table is set."""
    from diffopt_amd import EngineError
    from diffopt_amd.conic import ConicBatch
    for cones in ([(3, 0), (1, 2)], [(1, -1), (1, 3)]):
        e = ConicBatch(1, 2, cones)
        with pytest.raises(EngineError):
            e.set(np.zeros((1, 2, 2)), np.zeros((1, 2)), np.zeros((1, 2)), np.zeros((1, 2)), np.zeros((1, 2)),
                  np.zeros((1, 2)))
        e.close()
