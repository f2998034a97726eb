"""Device memory of the engine's handles (dopt_live_device_bytes, the
process-wide count of the bytes its device buffers hold): dopt_destroy gives
back everything a handle of any kind and route allocated, whichever entry
points ran, and repeated calls on one handle do not accumulate.  The counter
is read only as differences, with no other handle created in between, so the
device-wide free-memory figure (which other tenants of a shared card move)
plays no part."""

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

B, N, M, P = 2, 5, 3, 2
QP_TERMS = [(0, 0, 0, 1.0), (0, 0, 2, -0.5), (1, 1, 1, 2.0), (1, 2, 0, 3.0), (2, 3, 4, 1.5), (2, 3, 0, -1.0)]
CONES = [(1, 3), (3, 3)]   # Nonneg(3), SOC(3)
CN, CM = 4, 6
CONIC_TERMS = [(0, 0, 0, 1.0), (0, 0, 4, -2.0), (1, 3, 1, 0.5), (1, 2, 0, 1.0), (2, 3, 3, 1.0)]


def live():
    from diffopt_amd import _lib
    return _lib.load().dopt_live_device_bytes()


def _qp_data(batch=B):
    from diffopt_amd.synthetic import qp_numpy
    return qp_numpy(batch, N, M, P, 0.5, 4242, dense_tangents=True)


def _qp_dense():
    from diffopt_amd.qp import QPBatch
    d = _qp_data()
    e = QPBatch(B, N, M, P)
    e.set(d["Q"], d["G"], d["h"], d["A"], d["z"], d["lam"], d["nu"])
    rev = np.array(e.reverse(d["dl_dz"]))
    e.forward(dq=d["dq"], dh=d["dh"], db=d["db"])
    e.forward(dQ=d["dQ"], dq=d["dq"], dG=d["dG"], dh=d["dh"], dA=d["dA"], db=d["db"])
    e.forward_reverse(d["dl_dz"], dq=d["dq"], dh=d["dh"], db=d["db"])
    e.reverse_k(np.stack([d["dl_dz"], 2.0 * d["dl_dz"]]))
    e.forward_k(dq=np.stack([d["dq"], -d["dq"]]), dh=np.stack([d["dh"], d["dh"]]))
    e.reverse_grads(rev)
    e.params_reverse(rev, QP_TERMS, 3)
    e.params_forward(np.ones((B, 3)), QP_TERMS)
    return e


def _qp_sparse():
    from diffopt_amd.qp import QPBatch
    d = _qp_data()
    e = QPBatch(B, N, M, P, sparse=True)
    G = [sp.csc_matrix(g) for g in d["G"]]
    e.set_csc([sp.csc_matrix((N, N))] * B, G, d["h"], [sp.csc_matrix(a) for a in d["A"]], d["z"], d["lam"], d["nu"])
    rev, _ = e.forward_reverse(d["dl_dz"], dq=d["dq"], dh=d["dh"], db=d["db"])
    rev = np.array(rev)
    e.forward_reverse(d["dl_dz"], dq=d["dq"], dG=[0.5 * g for g in G], dh=d["dh"], db=d["db"])
    e.reverse_grads_at(rev)
    return e


def _conic_data(batch=B):
    from diffopt_amd.synthetic import conic_numpy
    return conic_numpy(batch, CN, CONES, 777)


def _conic(sparse):
    from diffopt_amd.conic import ConicBatch
    d = _conic_data()
    rng = np.random.default_rng(3)
    db, dc = rng.standard_normal((B, CM)), rng.standard_normal((B, CN))
    e = ConicBatch(B, CN, CONES, sparse=sparse)
    A = [sp.csc_matrix(a) for a in d["A"]]
    if sparse:
        e.set_csc(A, d["b"], d["c"], d["x"], d["s"], d["y"])
        (_, _), (g, _, _, _) = e.forward_reverse(d["dx"], dA=[0.5 * a for a in A], db=db, dc=dc)
        e.reverse_grads_at(np.array(g))
    else:
        e.set(d["A"], d["b"], d["c"], d["x"], d["s"], d["y"])
        e.forward(rng.standard_normal((B, CM, CN)), db, dc)
        g = e.reverse(d["dx"])[0]
        e.forward_reverse(d["dx"], db=db, dc=dc)
        e.reverse_k(np.stack([d["dx"], -d["dx"]]))
        e.forward_k(db=np.stack([db, db]), dc=np.stack([dc, -dc]))
        e.params_forward(np.ones((B, 3)), CONIC_TERMS)
        e.params_reverse(np.array(g), CONIC_TERMS, 3)
        e.params_jacobian(CONIC_TERMS, 3, 0)
        e.params_jacobian(CONIC_TERMS, 3, 1)
    return e


def _nlp():
    from diffopt_amd.nlp import NLPBatch
    from diffopt_amd.synthetic import nlp_numpy
    st, pt, dp, dx, dd = nlp_numpy(B, 6, 4, 2, 31)
    e = NLPBatch(B, 6, 4, 2)
    e.set_structure(st["con_kind"], st["has_low"], st["has_up"], st["sense"])
    e.set(*[pt[k] for k in ["Hxx", "Hxp", "Jx", "Jp", "x", "cval", "crhs", "y", "xl", "xu", "yl", "yu"]])
    e.factor()
    e.forward(dp)
    e.reverse(dx, dd)
    e.forward_reverse(dp, dx, dd)
    e.jacobian()
    return e


def _plug_point():
    from diffopt_amd.qp import MI355XSolver
    rng = np.random.default_rng(5)
    L = rng.standard_normal((7, 7)) + 7.0 * np.eye(7)
    s = MI355XSolver()
    s.solve_system(L, rng.standard_normal(7))
    s.solve_system(L + np.eye(7), rng.standard_normal(7))
    s.resolve(rng.standard_normal(7))
    return s


@pytest.mark.parametrize("make", [_qp_dense, _qp_sparse, lambda: _conic(False), lambda: _conic(True), _nlp,
                                  _plug_point],
                         ids=["qp_dense", "qp_sparse", "conic_dense", "conic_sparse", "nlp", "plug_point"])
def test_destroy_frees_everything(make):
    before = live()
    e = make()
    assert live() > before
    e.close()
    assert live() == before


def _rounds(step, n=20):
    """live after round 2 and after round n of `step`"""
    at2 = None
    for r in range(1, n + 1):
        step()
        if r == 2:
            at2 = live()
    return at2, live()


def test_params_calls_do_not_accumulate():
    from diffopt_amd.conic import ConicBatch
    from diffopt_amd.qp import QPBatch
    d = _qp_data()
    e = QPBatch(B, N, M, P)
    e.set(d["Q"], d["G"], d["h"], d["A"], d["z"], d["lam"], d["nu"])
    rev = np.array(e.reverse(d["dl_dz"]))

    def qp_step():
        e.params_reverse(rev, QP_TERMS, 3)
        e.params_forward(np.ones((B, 3)), QP_TERMS)

    at2, at20 = _rounds(qp_step)
    e.close()
    assert at20 == at2

    c = _conic_data()
    ce = ConicBatch(B, CN, CONES)
    ce.set(c["A"], c["b"], c["c"], c["x"], c["s"], c["y"])
    g = np.array(ce.reverse(c["dx"])[0])

    def conic_step():
        ce.params_forward(np.ones((B, 3)), CONIC_TERMS)
        ce.params_reverse(g, CONIC_TERMS, 3)
        ce.params_jacobian(CONIC_TERMS, 3, 0)
        ce.params_jacobian(CONIC_TERMS, 3, 1)

    at2, at20 = _rounds(conic_step)
    ce.close()
    assert at20 == at2


def test_model_loop_does_not_accumulate():
    """set_csc + reverse + forward on a batch-1 handle (the QPModel pattern),
    across the switch from pageable to pinned staging at the third call."""
    from diffopt_amd.qp import QPBatch
    d = _qp_data(1)
    e = QPBatch(1, N, M, P)
    Q, G, A = sp.csc_matrix(d["Q"][0]), sp.csc_matrix(d["G"][0]), sp.csc_matrix(d["A"][0])

    def step():
        e.set_csc(Q, G, d["h"], A, d["z"], d["lam"], d["nu"])
        e.reverse(d["dl_dz"])
        e.forward(dq=d["dq"], dh=d["dh"], db=d["db"])

    at2, at20 = _rounds(step)
    e.close()
    assert at20 == at2
