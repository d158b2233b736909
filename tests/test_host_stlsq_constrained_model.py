"""tests/stlsq_constrained_model.py -- the per-pass algorithm of symode_stlsq_sweep_constrained in numpy -- checked without a
GPU: (i) against ``solve_SINDy_one_step`` driven pass by pass on the oracle engine for the four solve_* cases of
tests/golden/f5_constraint.npz (masks and conv equal to the fixture's, Xi within the tolerance tests/test_oracle_golden.py
uses for these arrays); (ii) against an np.longdouble solve of the same Gq on every pass of every deck case, within the
derived bound (``M.xi_bound``: 4 n^2 cond(Gq) 2^-53 max|beta| through |q_xi|, plus (r' + 2) 2^-24 |q_xi| |beta| for the fp32
steps), with cond(Gq) <= 1e6 asserted; and the conditions on the deck itself (tests/stlsq_constrained_cases.py)."""
import numpy as np
import pytest
import torch

from symode_amd import lstsq
from symode_amd.sindy import SINDyRegression, solve_SINDy_one_step, stlsq_constrained_from_gram
from tests import stlsq_constrained_cases as C
from tests import stlsq_constrained_model as M
from tests.oracle_engine import OracleEngine


def test_the_pivot_floor_is_the_sweeps():
    assert M.PIVOT_FLOOR == lstsq.SINGULAR_RCOND ** 2


# ---- (i) solve_SINDy_one_step, pass by pass ----------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", C.SOLVE_TAGS)
def test_the_model_is_solve_sindy_one_step(tag):
    g = C.golden()
    d, order, cc = [int(v) for v in g[f"{tag}_cfg"]]
    gamma, thr = [float(v) for v in g[f"{tag}_hp"]]
    x, dx = torch.from_numpy(g[f"{tag}_x"]), torch.from_numpy(g[f"{tag}_dx"])
    eng = OracleEngine()
    reg = SINDyRegression(d, order, False, False, L_list=[torch.from_numpy(g[f"{tag}_L"])], threshold=thr, device="cpu",
                          constrain_constant=bool(cc), engine=eng, lstsq_driver="gels")
    reg.Q = torch.from_numpy(g[f"{tag}_Q"])
    coef = C.fixture_coef(tag)
    qs, qx = C.matrices(coef)
    G = eng.aug_gram(x, dx, order).numpy()
    mask = np.ones((d, coef.p), dtype=bool)
    conv = []
    for it, (want_mask, want_xi) in enumerate(zip(g[f"{tag}_masks"], g[f"{tag}_xis"])):
        out = M.one_pass(G, d, gamma, qs, qx, coef.allow_constant, mask)
        assert out is not None
        xi, var, Gq, _, cols = out
        assert np.linalg.cond(Gq) <= C.COND_BOUND
        _, done = solve_SINDy_one_step(reg, x, dx, gamma, thr)
        host_xi = reg.get_Xi().detach().numpy()
        new = mask & (np.abs(xi) > np.float32(thr))
        conv.append(bool(np.array_equal(new, mask)))
        assert conv[-1] == done
        mask = new
        assert np.array_equal(mask, reg.mask.numpy() > 0) and np.array_equal(mask, want_mask > 0), (tag, it)
        assert np.allclose(xi, want_xi, rtol=1e-5, atol=1e-6), (tag, it)                 # the fixture tolerance
        bound = 2 * M.xi_bound(qx, var, np.linalg.cond(Gq), len(cols), d, coef.p, coef.allow_constant)
        assert (np.abs(xi.astype(np.float64) - host_xi) <= bound).all(), (tag, it)        # two fp64 solves, two fp32 products
        # the restatement from a Gram matrix that the sweep's host loop uses is the same pass
        again = stlsq_constrained_from_gram(G, x.shape[0], trace_mask(want_mask, g[f"{tag}_masks"], it), gamma, d, coef, "gels")[0]
        assert (np.abs(again.astype(np.float64) - host_xi) <= bound).all(), (tag, it)
    assert conv == g[f"{tag}_conv"].tolist()


def trace_mask(_, masks, it):
    """The mask pass ``it`` was solved on: full before the first pass, then the fixture's mask after the pass before."""
    return np.ones(masks[0].shape, dtype=bool) if it == 0 else masks[it - 1] > 0


# ---- (ii) an extended-precision solve of the same system ---------------------------------------------------------------------
def _longdouble_xi(Gq, cq, cols, q_solve, q_xi, d, p, allow_constant):
    r = q_xi.shape[1]
    full = np.zeros(q_solve.shape[1], dtype=np.longdouble)
    if len(cols):
        A, c = Gq.astype(np.longdouble), cq.astype(np.longdouble)
        n = len(cols)
        for k in range(n):                                   # Gaussian elimination with partial pivoting in extended precision
            piv = k + int(np.argmax(np.abs(A[k:, k])))
            A[[k, piv]], c[[k, piv]] = A[[piv, k]], c[[piv, k]]
            for i in range(k + 1, n):
                f = A[i, k] / A[k, k]
                A[i, k:] -= f * A[k, k:]
                c[i] -= f * c[k]
        w = np.zeros(n, dtype=np.longdouble)
        for i in range(n - 1, -1, -1):
            w[i] = (c[i] - A[i, i + 1:] @ w[i + 1:]) / A[i, i]
        full[cols] = w
    xi = (q_xi.astype(np.longdouble) @ full[:r]).reshape(d, p)
    if allow_constant:
        xi[:, 0] += full[r:r + d]
    return xi, full


@pytest.mark.parametrize("name", C.SOLVED)
def test_every_pass_of_the_deck_against_extended_precision(name):
    coef = C.coef_map(name)
    qs, qx = C.matrices(coef)
    G, _ = C.gram(name)
    for gamma in C.GAMMAS:
        trace = []
        out = M.sweep(G, coef.d, gamma, C.THRESHOLD, 10, qs, qx, coef.allow_constant, band=C.BAND, trace=trace)
        assert out["fell"] == 0 and out["near"] == 0 and len(trace) == out["passes"]
        for mask, xi, Gq, cq, cols in trace:
            cond = np.linalg.cond(Gq) if len(cols) else 1.0
            assert cond <= C.COND_BOUND, (name, gamma, cond)
            assert np.array_equal(Gq, Gq.T)                                              # exactly symmetric
            want, full = _longdouble_xi(Gq, cq, cols, qs, qx, coef.d, coef.p, coef.allow_constant)
            var32 = full.astype(np.float64).astype(np.float32)
            bound = M.xi_bound(qx, var32, cond, len(cols), coef.d, coef.p, coef.allow_constant)
            err = np.abs(xi.astype(np.longdouble) - want).astype(np.float64)
            assert (err <= bound).all(), (name, gamma, err.max(), bound.min())


# ---- the deck ----------------------------------------------------------------------------------------------------------------
def test_the_deck_is_what_it_is_meant_to_be():
    assert len(C.DECK) == 24 and set(C.FLAGGED) < set(C.DECK)
    assert {C.coef_map(k).use_kron for k in C.SOLVED} == {True, False}
    assert {C.coef_map(k).allow_constant for k in C.SOLVED} == {True, False}
    assert {C.coef_map(k).d for k in C.DECK} == {2, 3}
    outs = {(k, g): M.sweep(C.gram(k)[0], C.coef_map(k).d, g, C.THRESHOLD, 10, *C.matrices(C.coef_map(k)),
                            C.coef_map(k).allow_constant, band=C.BAND) for k in C.SOLVED for g in C.GAMMAS}
    assert not any(o["fell"] for o in outs.values()) and not any(o["near"] for o in outs.values())
    assert max(o["passes"] for o in outs.values()) >= 3 and all(o["passes"] < 10 for o in outs.values())
    dropped = [k for k in C.SOLVED if not outs[k, 0.0]["mask"].all()]
    assert 2 * len(dropped) >= len(C.DECK)
    # a pass limit cuts the loop where it would run on
    k = max(C.SOLVED, key=lambda k: outs[k, 0.0]["passes"])
    capped = M.sweep(C.gram(k)[0], C.coef_map(k).d, 0.0, C.THRESHOLD, 2, *C.matrices(C.coef_map(k)), C.coef_map(k).allow_constant)
    assert capped["passes"] == 2 and not np.array_equal(capped["mask"], outs[k, 0.0]["mask"])


@pytest.mark.parametrize("name", C.FLAGGED)
def test_the_cases_moved_to_the_flagged_set_are_flagged(name):
    coef = C.coef_map(name)
    assert not coef.use_kron                               # the reference's indexing quirk: tests/stlsq_constrained_cases.py
    for gamma in C.GAMMAS:
        out = M.sweep(C.gram(name)[0], coef.d, gamma, C.THRESHOLD, 10, *C.matrices(coef), coef.allow_constant, band=C.BAND)
        assert out["fell"] == 1 and out["passes"] == 2
        first = M.sweep(C.gram(name)[0], coef.d, gamma, C.THRESHOLD, 1, *C.matrices(coef), coef.allow_constant, band=C.BAND)
        assert first["fell"] == 0 and first["passes"] == 1


def test_the_rank_deficient_situation_is_flagged():
    """so(2), order 3, support = the linear terms: Q's four columns span two directions there, the last pivots are round-off
    of either sign -- an exact > 0 test would let two correct implementations disagree, the floor flags both."""
    G, coef, mask = C.rankdef()
    qs, qx = C.matrices(coef)
    assert M.one_pass(G, 2, 0.0, qs, qx, coef.allow_constant, mask) is None
    cols = M.effective_columns(qs, mask)
    Gq, _ = M.build_system(G, 2, 0.0, qs, mask, cols)
    s = np.linalg.svd(Gq, compute_uv=False)
    assert len(cols) == 4 and s[2] < 1e-10 * s[0] and s[1] > 1e-3 * s[0]                # rank 2 of 4
    assert M.one_pass(G, 2, 0.0, qs, qx, coef.allow_constant, np.ones((2, 10), dtype=bool)) is not None
    out = M.sweep(G, 2, 0.0, C.THRESHOLD, 10, qs, qx, coef.allow_constant)
    assert out["fell"] == 1 and out["passes"] == 2                                      # the first thresholding leads there
    # the fixture's rankdef system (the same situation, recorded from the reference's run) is flagged as well
    g = C.golden()
    assert M.solve(g["rankdef_G"], g["rankdef_C"], M.PIVOT_FLOOR) is None
    # ... and the host loop's minimum-norm rule solves it
    xi = stlsq_constrained_from_gram(G, C.N_POINTS, mask, 0.0, 2, coef, "min_norm")[0]
    assert np.isfinite(xi).all() and np.abs(xi[0, 1] - 0.9) < 0.05 and np.abs(xi[0, 2] + 1.2) < 0.05


@pytest.mark.parametrize("kw", [dict(), dict(d=3, p=10, r=8, allow_constant=True, seed=6)], ids=["r64", "ortho_d3"])
def test_the_synthetic_cases_of_the_gpu_test_meet_the_decks_conditions(kw):
    """The lane limit (r' = 64 at p = 41, d = 2) and the d = 3 case with an orthonormal Q: solved to the end, well conditioned."""
    G, coef = C.orthonormal_case(**kw)
    qs, qx = C.matrices(coef)
    assert qs.shape[1] == (64 if not kw else 11)
    for gamma in C.GAMMAS:
        trace = []
        out = M.sweep(G, coef.d, gamma, C.THRESHOLD, 10, qs, qx, coef.allow_constant, band=C.BAND, trace=trace)
        assert out["fell"] == 0 and out["near"] == 0 and out["passes"] == 2 and not out["mask"].all()
        assert max(np.linalg.cond(t[2]) for t in trace) <= C.COND_BOUND
