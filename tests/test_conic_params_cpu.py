"""The parametric cone-program fixture (tests/golden/conic_param_fixtures.json,
the reference's test/parameters.jl:103-152) through the numpy restatement of
the POI maps (tests/conic_poi_cases.py) and the CPU oracle's conic solves
(oracle/conic.py): forward dx = 3·direction, reverse dp = 3·direction at the
reference's atol.  No GPU."""

import json
import os

import numpy as np
import pytest

import conic_poi_cases as poi
from oracle import conic as ocn

HERE = os.path.dirname(os.path.abspath(__file__))
FX = json.load(open(os.path.join(HERE, "golden", "conic_param_fixtures.json")))


def test_fixture_is_what_the_maker_writes(tmp_path, monkeypatch):
    import importlib.util
    spec = importlib.util.spec_from_file_location("mk", os.path.join(HERE, "golden", "make_conic_param_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    monkeypatch.setattr(mk, "OUT", str(tmp_path))
    mk.main()
    assert json.load(open(tmp_path / "conic_param_fixtures.json")) == FX


@pytest.mark.parametrize("fx", FX, ids=[f["name"] for f in FX])
def test_fixture_on_the_oracle(fx):
    cones = [tuple(c) for c in fx["cones"]]
    assert cones == poi.RHS_CONES
    terms = [tuple(t) for t in fx["terms"]]
    cache = ocn.Cache(fx["A"], fx["b"], fx["c"], fx["x"], fx["s"], fx["y"], cones, fx["max_sense"])
    n, m = cache.n, cache.m
    for sw in fx["sweeps"]:
        d = sw["direction"]
        db, dc = poi.forward(terms, np.array([d]), n, m)
        assert db[0] == -3.0 * d and not db[1:].any() and not dc.any()   # the sign: no `_fill` negation
        dx = ocn.forward_differentiate(cache, None, db, dc)[0]
        assert abs(dx[0] - sw["dx"]) <= fx["atol"], (fx["p"], d, dx)
        g, _ = ocn.reverse_differentiate(cache, np.array([d]))
        dp = poi.reverse(terms, fx["nparam"], g, cache.x, cache.vp)
        assert abs(dp[0] - sw["dp"]) <= fx["atol"], (fx["p"], d, dp)


def test_restatement_edges():
    """The restatement itself: summation in term order, kind 2 dropped /
    zero, kind 1 refused, the reverse entries equal to reverse_outputs'."""
    rng = np.random.default_rng(0)
    n, m = 5, 4
    terms = [(0, 0, 3, 2.0), (1, 3, 4, -1.0), (0, 0, 3, 0.5), (2, 2, 0, 7.0), (1, 0, 0, 3.0)]
    dp = rng.standard_normal(3)
    db, dc = poi.forward(terms, dp, n, m)
    np.testing.assert_array_equal(db, [dp[1] * 3.0, 0, 0, dp[0] * 2.0 + dp[0] * 0.5])
    np.testing.assert_array_equal(dc, [0, 0, 0, 0, -dp[1]])
    g, x, vp = rng.standard_normal(n + m + 1), rng.standard_normal(n), rng.standard_normal(m)

    class C:
        pass
    c = C()
    c.n, c.m, c.x, c.vp = n, m, x, vp
    _, odb, odc = ocn.reverse_outputs(c, g)
    out = poi.reverse(terms, 3, g, x, vp)
    np.testing.assert_array_equal(out, [2.0 * odb[3] + 0.5 * odb[3], -odc[4] + 3.0 * odb[0], 0.0])
    with pytest.raises(ValueError):
        poi.forward([(0, 1, 0, 1.0)], dp, n, m)
    with pytest.raises(ValueError):
        poi.reverse([(0, 1, 0, 1.0)], 3, g, x, vp)
