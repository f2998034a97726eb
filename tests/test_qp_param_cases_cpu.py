"""The parametric-QP case module (tests/qp_param_cases.py) against the CPU
oracle: the extended POI restatement agrees with oracle/poi.py where both are
defined, the golden fixtures' known answers (the reference's own tests,
transcribed by tests/golden/make_qp_param_golden.py) are met by the oracle's
solves on the restatement's tangents, and the synthetic builder puts terms
where the engine can go wrong."""

import numpy as np
import pytest

import qp_param_cases as qc
from oracle import poi
from oracle import qp as oqp

FX = qc.fixtures()


def test_restatement_equals_poi_oracle_on_kinds_0_to_3():
    rng = np.random.default_rng(3)
    n, m, p, nparam = 7, 5, 3, 6
    terms = []
    for _ in range(60):
        kind = int(rng.integers(4))
        lim = {0: m, 1: p, 2: 1, 3: n}[kind]
        terms.append((int(rng.integers(nparam)), kind, int(rng.integers(lim)), float(rng.standard_normal())))
    dp = rng.standard_normal(nparam)
    dq, dh, db, dG, dA = qc.poi_forward_full(terms, dp, n, m, p)
    rq, rh, rb = poi.forward(terms, dp, n, m, p)
    assert np.array_equal(dq, rq) and np.array_equal(dh, rh) and np.array_equal(db, rb)
    assert not dG.any() and not dA.any()
    z, lam, nu = rng.standard_normal(n), rng.uniform(0, 1, m), rng.standard_normal(p)
    rev = rng.standard_normal(n + m + p)
    assert np.array_equal(qc.poi_reverse_full(terms, nparam, z, lam, nu, rev),
                          poi.reverse(terms, nparam, lam, rev, n, m, p))


def test_fixture_file_is_what_the_generator_writes(tmp_path, monkeypatch):
    import importlib.util
    import json
    import os
    spec = importlib.util.spec_from_file_location("make_qp_param_golden",
                                                  os.path.join(qc.HERE, "golden", "make_qp_param_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(mod, "OUT", str(tmp_path))
    mod.main()
    assert json.load(open(tmp_path / "qp_param_fixtures.json")) == FX
    names = [f["name"] for f in FX]
    assert "diff_rhs_p3" in names and "quadratic_objective_qp_p3" in names
    assert sum(nm.startswith("affine_changes_compact") for nm in names) == 9


@pytest.mark.parametrize("fx", FX, ids=[f["name"] for f in FX])
def test_fixture_known_answers_on_the_oracle(fx):
    Q, G, h, A, z, lam, nu = qc.fixture_arrays(fx)
    n, m, p, nparam, terms = fx["n"], fx["m"], fx["p"], fx["nparam"], fx["terms"]
    # the point is a KKT point of the problem as written
    assert np.allclose(Q @ z + np.array(fx["q"]) + G.T @ lam, 0.0, atol=1e-15)
    assert np.all(G @ z - h <= 1e-15) and np.all(lam >= 0)
    for sw in fx["fwd"]:
        dq, dh, db, dG, dA = qc.poi_forward_full(terms, np.array(sw["dp"]), n, m, p)
        dz, _, _ = oqp.forward_differentiate(Q, G, h, A, z, lam, nu, dq=dq, dG=dG, dh=dh, dA=dA, db=db)
        for got, want in zip(dz, sw["dx"]):
            assert qc.isapprox(got, want, fx["rtol"], fx["atol"]), (sw, got)
    for sw in fx["rev"]:
        rev = np.concatenate(oqp.reverse_differentiate(Q, G, h, A, z, lam, nu, np.array(sw["dx"])))
        got = qc.poi_reverse_full(terms, nparam, z, lam, nu, rev)
        for g, want in zip(got, sw["dp"]):
            assert qc.isapprox(g, want, fx["rtol"], fx["atol"]), (sw, got)


@pytest.mark.parametrize("shape", qc.SHAPES, ids=str)
@pytest.mark.parametrize("nparam", [16, 17, 33])
def test_synthetic_cases_cover_the_edges(shape, nparam):
    B, n, m, p = shape
    case = qc.synthetic_case(B, n, m, p, nparam, seed=100 + nparam)
    terms = [qc.term5(t) for t in case["terms"]]
    d = case["d"]
    by_param = {}
    for t in terms:
        by_param.setdefault(t[0], []).append(t)
        lim = {0: m, 1: p, 2: 1, 3: n, 4: m, 5: p}[t[1]]
        assert 0 <= t[0] < nparam and 0 <= t[2] < lim and 0 <= t[4] < n
    assert nparam - 1 not in by_param                                  # a parameter with no terms
    assert {t[1] for t in by_param[nparam - 2]} == {2}                 # ... and one with kind-2 terms only
    keys = [(t[0], t[1], t[2], t[4]) for t in terms if t[1] in (4, 5)]
    assert len(keys) > len(set(keys))                                  # two terms on one (parameter, row, variable)
    assert {t[1] for t in terms} == {2, 3} | ({0, 4} if m else set()) | ({1, 5} if p else set())
    if not m:
        return
    rows = {k: {t[2] for t in terms if t[1] == k} for k in (0, 4)}
    for b in range(B):
        s = oqp.gz_minus_h(d["G"][b], d["z"][b], d["h"][b])
        elim = {i for i in range(m) if d["lam"][b, i] == 0.0 and s[i] != 0.0}
        kept = set(range(m)) - elim
        for k in (0, 4):   # every problem: a kind-0 and a kind-4 term on an eliminated row and on a kept one
            assert rows[k] & elim and rows[k] & kept


def test_small_nparam_case_is_all_active():
    case = qc.synthetic_case(3, 20, 30, 4, 1, seed=101)
    assert case["active"] == 1 and {qc.term5(t)[0] for t in case["terms"]} == {0}
