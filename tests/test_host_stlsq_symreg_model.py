"""tests/stlsq_symreg_model.py -- the numpy restatement of symode_stlsq_sweep_symreg the GPU test compares the kernel with --
against a dense solve of the same system per pass, on the deck of tests/stlsq_symreg_cases.py; the conditions the GPU test's
bound rests on (cond(A) of every pass, no coefficient of a deciding pass near the threshold); and the host twin
``sindy.stlsq_symreg_from_gram`` / ``SeedSweepSTLSQ.solve(rev=...)`` against the model."""
import numpy as np
import pytest
import torch

from tests import stlsq_symreg_cases as C
from tests import stlsq_symreg_model as M

CONFIGS = [(g, w, it) for g in C.GAMMAS for w in C.W_SYMS for it in C.MAX_ITERS]


def _dense_sweep(G, R, d, gamma, threshold, w_sym, max_iter):
    """The loop with np.linalg.solve on the model's own A, b per pass: (Xi, mask, passes)."""
    gamma, threshold, w_sym = M.f32(gamma), M.f32(threshold), M.f32(w_sym)
    p = G.shape[0] - d
    mask = np.ones((d, p), dtype=bool)
    xi, passes = np.zeros((d, p)), 0
    for it in range(max_iter):
        passes = it + 1
        sel = M.support(mask)
        A, b = M.build_system(G, R, d, gamma, w_sym, sel)
        xi = np.zeros((d, p))
        if sel:
            xi[mask] = np.linalg.solve(A, b)
        new = mask & (np.abs(xi.astype(np.float32)) > np.float32(threshold))
        same = np.array_equal(new, mask)
        mask = new
        if same:
            break
    return xi, mask, passes


@pytest.mark.parametrize("name", C.DECK)
def test_the_model_equals_a_dense_solve_and_the_deck_meets_its_conditions(name):
    G, R, d = C.pair(name)
    n_max = 0
    for gamma, w_sym, max_iter in CONFIGS:
        out, trace = C.modelled(name, gamma, w_sym, max_iter)
        assert out["fell"] == 0 and out["passes"] == len(trace) <= max_iter
        xi, mask, passes = _dense_sweep(G, R, d, gamma, C.THRESHOLD, w_sym, max_iter)
        assert passes == out["passes"] and np.array_equal(mask, out["mask"]), (name, gamma, w_sym, max_iter)
        for before, xi_t, A, b, sel in trace:
            n = len(sel)
            n_max = max(n_max, n)
            assert np.array_equal(A, A.T) and n == before.sum()
            cond = np.linalg.cond(A)
            assert cond <= C.COND_BOUND, (name, gamma, w_sym, cond)
            v = xi_t[before].astype(np.float64)
            bound = M.xi_bound(v, cond, n)
            gap = np.abs(np.abs(v) - M.f32(C.THRESHOLD))
            assert (gap > C.GAP * bound).all(), (name, gamma, w_sym, (gap / bound).min())
            assert (np.abs(v - np.linalg.solve(A, b)) <= bound).all()
        last = trace[-1]
        err = np.abs(out["xi"].astype(np.float64) - xi)
        assert (err[last[0]] <= M.xi_bound(out["xi"][last[0]], np.linalg.cond(last[2]), len(last[4]))).all()
        assert not out["xi"][~last[0]].any()                                  # zeros off the support of the last solve
    assert n_max == {"osc_o2": 12, "osc_o3": 20, "osc_o5": 42, "osc_o2_exp": 16, "osc3_o3": 60}.get(name, 64)


def test_what_the_deck_covers():
    shapes = {name: (C.pair(name)[2], C.pair(name)[0].shape[0] - C.pair(name)[2]) for name in C.DECK}
    assert shapes == {"osc_o2": (2, 6), "osc_o3": (2, 10), "osc_o5": (2, 21), "osc_o2_exp": (2, 8), "osc3_o3": (3, 20),
                      "spd_d4_p16": (4, 16), "spd_d1_p64": (1, 64)}
    assert max(C.modelled(n, g, w, 10)[0]["passes"] for n in C.DECK for g in C.GAMMAS for w in C.W_SYMS) >= 4
    # the regulariser decides: at order 5 the plain fit ends on a wrong support, w_sym = 10 on the true one
    assert not np.array_equal(C.modelled("osc_o5", 0.0, 0.0, 10)[0]["mask"], C.truth("osc_o5"))
    assert np.array_equal(C.modelled("osc_o5", 0.0, 10.0, 10)[0]["mask"], C.truth("osc_o5"))
    for name in ("osc_o2", "osc_o3"):
        assert np.array_equal(C.modelled(name, 0.0, 1.0, 10)[0]["mask"], C.truth(name))
    # max_iter cuts the loop: one pass thresholds once
    one = C.modelled("osc_o3", 0.0, 1.0, 1)[0]
    assert one["passes"] == 1 and one["mask"].sum() == len(C.modelled("osc_o3", 0.0, 1.0, 10)[1][1][4])


def test_w_sym_zero_is_the_block_diagonal_system_to_the_bit():
    """With w_sym = 0 and a finite R the product is a zero: A is blockdiag(Gtt + gamma^2 I)[M, M] exactly, cross-row entries
    exact zeros -- what the GPU test's comparison with symode_stlsq_sweep rests on."""
    G, R, d = C.pair("osc_o3")
    p = G.shape[0] - d
    mask = np.ones((d, p), dtype=bool)
    mask[0, 3], mask[1, 7] = False, False
    sel = M.support(mask)
    A, b = M.build_system(G, R, d, 0.1, 0.0, sel)
    want = np.zeros((d * p, d * p))
    for j in range(d):
        want[j * p:(j + 1) * p, j * p:(j + 1) * p] = G[:p, :p] + 0.1 * 0.1 * np.eye(p)
    flat = mask.reshape(-1)
    assert A.tobytes() == np.ascontiguousarray(want[flat][:, flat]).tobytes()
    assert np.array_equal(b, G[:p, p:].T.reshape(-1)[flat])


def test_an_exactly_singular_pair_is_flagged_and_an_empty_support_ends_the_problem():
    G, R = np.zeros((8, 8)), np.zeros((12, 12))
    out = M.sweep(G, R, 2, 0.0, C.THRESHOLD, 1.0, 10)
    assert out["fell"] == 1 and out["passes"] == 1
    G, R, d = C.pair("osc_o2")
    out = M.sweep(G, R, d, 0.0, 50.0, 1.0, 10)                       # a threshold above every coefficient: pass 2 has n = 0
    assert out["fell"] == 0 and out["passes"] == 2 and not out["mask"].any() and not out["xi"].any()


# ---- the host twin ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["osc_o3", "osc_o2_exp", "osc3_o3"])
def test_the_host_pass_solves_the_models_system(name):
    from symode_amd.sindy import stlsq_symreg_from_gram, stlsq_symreg_system
    G, R, d = C.pair(name)
    for gamma, w_sym in ((0.0, 0.0), (M.f32(0.1), M.f32(0.1)), (0.0, 10.0)):
        out, trace = C.modelled(name, gamma, w_sym, 10)
        for before, xi_t, A, b, sel in trace:
            A_h, b_h = stlsq_symreg_system(G, R, before, gamma, w_sym, d)
            assert A_h.tobytes() == A.tobytes() and b_h.tobytes() == b.tobytes()
            for driver in ("gels", "min_norm"):
                xi, w = stlsq_symreg_from_gram(G, R, C.N_POINTS, before, gamma, w_sym, d, driver)
                assert xi.dtype == np.float32 and xi.shape == before.shape and not xi[~before].any()
                bound = 2 * M.xi_bound(xi_t[before], np.linalg.cond(A), len(sel))            # two fp64 solves of one system
                assert (np.abs(xi[before].astype(np.float64) - xi_t[before]) <= bound).all(), (name, driver)
    xi, w = stlsq_symreg_from_gram(G, R, C.N_POINTS, np.zeros_like(trace[0][0]), 0.0, 1.0, d, "gels")
    assert not xi.any() and len(w) == 0


def _sweep_on(G, d, order, exp, n_points, engine):
    from symode_amd.sweep import SeedSweepSTLSQ
    S = G.shape[0]
    sw = SeedSweepSTLSQ(torch.zeros(8, d), torch.zeros(8, d), order, include_exp=exp, n_seeds=S, engine=engine,
                        idx=torch.zeros(S, 4, dtype=torch.int32))
    sw._gram, sw.n_points = np.ascontiguousarray(G), n_points
    return sw


def test_solve_on_the_host_route_is_the_models_loop():
    from tests.oracle_engine import OracleEngine
    names = ("osc_o2", "osc_o2")
    G = np.stack([C.pair(n)[0] for n in names])
    R = np.stack([C.pair(n)[1] for n in names])
    R[1] *= 0.5                                                    # a second problem with another regulariser
    sw = _sweep_on(G, 2, 2, False, C.N_POINTS, OracleEngine())
    w_sym = 1.0
    Xi, mask, passes = sw.solve(0.0, M.f32(C.THRESHOLD), max_iter=10, rev=(R, w_sym))
    for R_in in (torch.from_numpy(R),):                             # R as a tensor gives the same answer
        again = _sweep_on(G, 2, 2, False, C.N_POINTS, OracleEngine()).solve(0.0, M.f32(C.THRESHOLD), max_iter=10, rev=(R_in, w_sym))
        assert torch.equal(again[0], Xi) and torch.equal(again[1], mask)
    for s in range(2):
        out = M.sweep(G[s], R[s], 2, 0.0, C.THRESHOLD, w_sym, 10, band=C.BAND)
        assert np.array_equal(mask[s].numpy() > 0, out["mask"]) and passes[s] == out["passes"]
        assert np.allclose(Xi[s].numpy(), out["xi"], rtol=1e-6, atol=1e-7)
    assert Xi.dtype == torch.float32 and tuple(Xi.shape) == (2, 2, 6)
