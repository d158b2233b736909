"""tests/stlsq_path_symreg_model.py -- the numpy restatement of symode_stlsq_path_symreg the GPU test compares the kernel with
-- against a dense fp64 solve per step, on the deck of tests/stlsq_path_symreg_cases.py; the conditions the GPU test's bounds
and its demand for equal decisions rest on, asserted for every case and step from the model alone (cond(A) <= 1e6, every
elimination and every comparison behind ``best`` decided by at least 100 bounds -- the tie and the zero right-hand side are
the stated exceptions, decided by index); and the host twin ``sindy.stlsq_path_symreg_from_gram`` against the model."""
import warnings

import numpy as np
import pytest

from tests import stlsq_constrained_model as Q
from tests import stlsq_path_symreg_cases as P
from tests import stlsq_path_symreg_model as M


def test_the_models_solve_is_the_shared_statement_to_the_bit():
    """M.solve writes the rank-one update of tests.stlsq_constrained_model.solve as one array statement: the same bits."""
    for name, gamma, w_sym in (("osc_o3", 0.1, 1.0), ("osc_o2_exp", 0.0, 10.0), ("n2", 0.0, 1.0)):
        for active, A, b, sel in P.chained(name, gamma, w_sym)[1][::3]:
            assert M.solve(A, b, M.PIVOT_FLOOR).tobytes() == Q.solve(A, b, M.PIVOT_FLOOR).tobytes()
    assert M.solve(np.zeros((3, 3)), np.zeros(3), M.PIVOT_FLOOR) is None and Q.solve(np.zeros((3, 3)), np.zeros(3), M.PIVOT_FLOOR) is None
    A = np.array([[1.0, 0.0], [0.0, 1e-15]])
    assert M.solve(A, np.ones(2), M.PIVOT_FLOOR) is None and M.solve(A, np.ones(2), 0.0) is not None


@pytest.mark.parametrize("name", P.DECK)
def test_the_model_equals_a_dense_solve_and_the_deck_meets_its_conditions(name):
    G, R, V, d = P.case(name)
    p = G.shape[0] - d
    n0 = d * p
    for gamma, w_sym in P.CONFIGS:
        o, trace = P.chained(name, gamma, w_sym)
        assert o["fell"] == 0 and len(trace) == n0 and sorted(o["order"].tolist()) == list(range(n0))
        assert not o["path_xi"][n0].any() and o["mse_val"][n0] == sum(V[p + j, p + j] for j in range(d))
        for t, (active, A, b, sel) in enumerate(trace):
            n = len(sel)
            assert n == n0 - t == active.sum() and np.array_equal(A, A.T)
            cond = np.linalg.cond(A)
            assert cond <= P.COND_BOUND, (name, gamma, w_sym, t, cond)
            v = o["path_xi"][t][active].astype(np.float64)
            assert (np.abs(v - np.linalg.solve(A, b)) <= M.xi_bound(v, cond, n)).all(), (name, gamma, w_sym, t)
            assert not o["path_xi"][t][~active].any()
            assert active.reshape(-1)[o["order"][t]] and (t == 0 or not active.reshape(-1)[o["order"][t - 1]])
        for t in range(n0 + 1):
            xi = o["path_xi"][t]
            assert abs(o["mse_train"][t] - P.quad(G, d, p, xi)) <= P.mse_bound(G, d, p, xi)
            assert abs(o["mse_val"][t] - P.quad(V, d, p, xi)) <= P.mse_bound(V, d, p, xi)
            vl = xi.reshape(-1).astype(np.longdouble)
            assert abs(o["reg_train"][t] - vl @ R.astype(np.longdouble) @ vl) <= P.reg_bound(R, xi)
        cond, gap, ties, margins = P.conditions(name, gamma, w_sym)
        assert gap >= P.DECIDED_BY, (name, gamma, w_sym, gap)
        assert (ties > 0) == (name in P.INDEX_DECIDED), (name, ties)
        for tol in P.TOLS:
            assert margins[tol] >= P.DECIDED_BY, (name, gamma, w_sym, tol, margins[tol])
            m = P.modelled(name, gamma, w_sym, tol)
            best = m["best"]
            assert m["Xi"].tobytes() == o["path_xi"][best].tobytes()             # the chosen step solved again: the same bits
            assert np.array_equal(np.sort(o["order"][best:]), np.nonzero(m["mask"].reshape(-1))[0])


def test_what_the_deck_covers():
    shapes = {name: (P.case(name)[3], P.case(name)[0].shape[0] - P.case(name)[3]) for name in P.DECK}
    assert shapes == {"osc_o2": (2, 6), "osc_o3": (2, 10), "osc_o5": (2, 21), "osc_o2_exp": (2, 8), "osc3_o3": (3, 20),
                      "spd_d4_p16": (4, 16), "spd_d1_p64": (1, 64), "n1": (1, 1), "n2": (2, 1), "tie": (1, 3), "zero_rhs": (2, 6)}
    # the tie: bit-equal |v| of columns 0 and 1 at step 0, column 0 leaves first
    o = P.chained("tie", 0.0, 0.0)[0]
    assert o["path_xi"][0, 0, 0].tobytes() == o["path_xi"][0, 0, 1].tobytes() == np.float32(0.5).tobytes()
    assert o["order"].tolist() == [0, 1, 2] and o["near"] == 1
    # the zero right-hand side: every solution 0, eliminated by index, the empty model kept
    o = P.chained("zero_rhs", 0.1, 1.0)[0]
    assert not o["path_xi"].any() and o["order"].tolist() == list(range(12)) and len(set(o["mse_val"].tolist())) == 1
    assert P.modelled("zero_rhs", 0.1, 1.0, 0.0)["best"] == 12 and not P.modelled("zero_rhs", 0.1, 1.0, 0.0)["mask"].any()
    # the singular pair is flagged at its first pivot
    G, R, V, d = P.case("singular")
    assert M.path(G, R, V, d, 0.0, 1.0, 0.0, P.FLOOR_REL, P.BAND)["fell"] == 1
    # the regulariser and the tolerance decide
    bests = {(w, tol): P.modelled("osc_o5", 0.0, w, tol)["best"] for w in P.W_SYMS for tol in P.TOLS}
    assert len(set(bests.values())) >= 4
    assert not np.array_equal(P.chained("osc_o5", 0.0, 0.0)[0]["order"], P.chained("osc_o5", 0.0, 10.0)[0]["order"])
    # w_sym = 0 uncouples the rows: the regulariser's score is still taken, the system is block diagonal
    assert P.chained("osc_o3", 0.0, 0.0)[0]["reg_train"][0] > 0.0


def test_gamma_and_w_sym_are_held_in_fp32():
    G, R, V, d = P.case("osc_o2")
    a = M.chain(G, R, V, d, 0.1, 0.3, P.BAND)
    b = M.chain(G, R, V, d, float(np.float32(0.1)), float(np.float32(0.3)), P.BAND)
    assert a["path_xi"].tobytes() == b["path_xi"].tobytes() and a["mse_val"].tobytes() == b["mse_val"].tobytes()


@pytest.mark.parametrize("name", ("osc_o2", "osc_o3", "osc_o2_exp", "n1", "n2", "tie", "zero_rhs"))
def test_the_host_twin_follows_the_model(name):
    """sindy.stlsq_path_symreg_from_gram solves each step with LAPACK where the model restates the kernel: equal decisions
    (the deck's conditions), coefficients within the two solves' bounds, scores within theirs."""
    from symode_amd.sindy import stlsq_path_symreg_from_gram, stlsq_path_symreg_select
    G, R, V, d = P.case(name)
    p = G.shape[0] - d
    n0 = d * p
    for gamma, w_sym in P.CONFIGS:
        o, trace = P.chained(name, gamma, w_sym)
        for tol in P.TOLS:
            m = P.modelled(name, gamma, w_sym, tol)
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                xi, mask, rec = stlsq_path_symreg_from_gram(G, R, V, M.f32(gamma), M.f32(w_sym), tol, P.FLOOR_REL, P.BAND, d, P.N_POINTS)
            assert np.array_equal(rec["order"], o["order"]) and rec["best"] == m["best"] and rec["near"] == o["near"], (name, gamma, w_sym, tol)
            assert np.array_equal(mask, m["mask"]) and rec["path_xi"].shape == (n0 + 1, d, p) and rec["mse_val"].shape == (n0 + 1,)
            assert xi.tobytes() == rec["path_xi"][rec["best"]].tobytes()
            assert stlsq_path_symreg_select(rec["mse_val"], V, d, tol, P.FLOOR_REL) == rec["best"]
            for t, (active, A, b, sel) in enumerate(trace):
                bound = 2 * M.xi_bound(o["path_xi"][t][active], np.linalg.cond(A), len(sel))
                assert (np.abs(rec["path_xi"][t][active].astype(np.float64) - o["path_xi"][t][active]) <= bound).all()
            for t in range(n0 + 1):
                xi_t = rec["path_xi"][t]
                assert abs(rec["mse_train"][t] - P.quad(G, d, p, xi_t)) <= P.mse_bound(G, d, p, xi_t)
                assert abs(rec["mse_val"][t] - P.quad(V, d, p, xi_t)) <= P.mse_bound(V, d, p, xi_t)
                vl = xi_t.reshape(-1).astype(np.longdouble)
                assert abs(rec["reg_train"][t] - vl @ R.astype(np.longdouble) @ vl) <= P.reg_bound(R, xi_t)


def test_the_host_twin_warns_on_a_singular_support(monkeypatch):
    from symode_amd import lstsq
    from symode_amd.sindy import stlsq_path_symreg_from_gram
    monkeypatch.setattr(lstsq, "_warned_singular", False)                      # (the fallback warns once per process)
    G, R, V, d = P.case("singular")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        xi, mask, record = stlsq_path_symreg_from_gram(G, R, V, 0.0, 1.0, 0.02, P.FLOOR_REL, P.BAND, d, P.N_POINTS)
    assert any(w.category is RuntimeWarning and "minimum-norm solution" in str(w.message) for w in rec)
    assert not xi.any() and record["order"].tolist() == list(range(12))       # nothing to fit: zeros, eliminated by index
    assert record["best"] == 12 and not mask.any()
