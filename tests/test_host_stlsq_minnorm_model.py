"""tests/stlsq_minnorm_model.py -- the rank-revealing mode of the constrained device sweep in numpy -- checked without a GPU
on the cases of tests/stlsq_minnorm_cases.py: (i) its per-pass solve against the native host routine the sweep's replay calls
(``lstsq_normal(Gq, cq, m, 'gelsy', 1e-7)`` on the model's own Gq, cq: equal ranks, the solution within the derived bound) and
against an np.longdouble restatement of the truncated solve; (ii) on the full-rank cases, byte for byte the model of the
existing entry; (iii) its sweep against the host loop ``_replay(..., 'min_norm')`` (masks and passes equal, Xi within twice
the bound: two summation orders); (iv) the conditions on the inputs -- margins of the rank decision on both sides of the cut
and the condition number -- on every truncated pass.  They are properties of the inputs, not tuned to any kernel."""
import functools

import numpy as np
import pytest

from symode_amd import lstsq
from tests import stlsq_constrained_cases as C
from tests import stlsq_constrained_model as M0
from tests import stlsq_minnorm_cases as K
from tests import stlsq_minnorm_model as M


@functools.lru_cache(maxsize=None)
def swept(key, gamma, max_iter=10):
    G, coef = K.inputs(key)
    qs, qx = C.matrices(coef)
    trace = []
    out = M.sweep(G, coef.d, gamma, K.THRESHOLD, max_iter, qs, qx, coef.allow_constant, band=K.BAND, trace=trace)
    return out, trace


def test_the_cut_is_the_sweeps():
    assert M.RCOND == lstsq.SINGULAR_RCOND == 1e-7


def test_the_cases_are_what_they_are_meant_to_be():
    assert set(K.FULL) - {"r64"} <= set(C.SOLVED) and len(K.FULL) == 4 and K.FLAGGED == C.FLAGGED
    G, coef = K.inputs("dup64")
    qs = C.matrices(coef)[0]
    assert qs.shape == (82, 64) and coef.d == 2 and coef.p == 41 and np.array_equal(qs[:, 40:], qs[:, :24])
    assert (qs.shape[1], K.inputs("rankdef")[1].p, K.inputs("so3a_o2")[1].d) == (64, 10, 3)
    for key, want in K.RANKS.items():
        out, trace = swept(key, 0.0)
        got = [(t[5]["n"], t[5]["rank"]) for t in trace]
        assert got == want and out["fell"] == 0 and out["near"] == 0, (key, got)
        assert out["trunc"] == sum(r < n for n, r in want) and out["rank"] == want[-1][1]
    zero, _ = swept("zero", 0.0)
    assert not zero["mask"].any() and not zero["xi"].any() and zero["trunc"] == 1 and zero["passes"] == 2


# ---- (i) the per-pass solve ---------------------------------------------------------------------------------------------------
def _longdouble_min_norm(Gq, cq, orig, rank):
    """The truncated solve restated in extended precision from Gq itself: the first ``rank`` rows of the Cholesky factor in the
    model's pivot order, q = R11^-T c1, Y = Wm^T (Wm Wm^T)^-1 q by Gaussian elimination with partial pivoting."""
    n = len(cq)
    S = Gq.astype(np.longdouble)[np.ix_(orig, orig)]
    c = cq.astype(np.longdouble)[orig]
    R = np.zeros((rank, n), dtype=np.longdouble)
    q = np.zeros(rank, dtype=np.longdouble)
    for k in range(rank):
        R[k, k] = np.sqrt(S[k, k])
        R[k, k + 1:] = S[k, k + 1:] / R[k, k]
        S[k + 1:, k + 1:] -= np.outer(R[k, k + 1:], R[k, k + 1:])
        q[k] = (c[k] - R[:k, k] @ q[:k]) / R[k, k]
    A, z = R @ R.T, q.copy()
    for k in range(rank):
        piv = k + int(np.argmax(np.abs(A[k:, k])))
        A[[k, piv]], z[[k, piv]] = A[[piv, k]], z[[piv, k]]
        for i in range(k + 1, rank):
            f = A[i, k] / A[k, k]
            A[i, k:] -= f * A[k, k:]
            z[i] -= f * z[k]
    for i in range(rank - 1, -1, -1):
        z[i] = (z[i] - A[i, i + 1:] @ z[i + 1:]) / A[i, i]
    w = np.zeros(n, dtype=np.longdouble)
    w[orig] = R.T @ z
    return w


@pytest.mark.parametrize("key", K.ALL)
def test_every_pass_against_the_native_host_routine_and_extended_precision(key):
    G, coef = K.inputs(key)
    for gamma in K.GAMMAS:
        out, trace = swept(key, gamma)
        assert out["fell"] == 0 and len(trace) == out["passes"]
        for _, xi, Gq, cq, cols, info in trace:
            n, rank = info["n"], info["rank"]
            if n == 0:
                continue
            assert np.array_equal(Gq, Gq.T)                                              # exactly symmetric
            mine, _ = M.solve(Gq, cq)
            host, host_rank = lstsq.lstsq_normal(Gq, cq, coef.d * (K.N_POINTS + coef.p), "gelsy", M.RCOND)
            assert host_rank == rank, (key, gamma, host_rank, rank)
            cond = M.pass_cond(info, Gq)
            bound = (M.var_bound if rank < n else M0.var_bound)(mine.astype(np.float32), cond, n)
            err = np.abs(mine - host)
            print(key, gamma, "n", n, "rank", rank, "cond %.3g" % cond, "max err / bound %.3g" % (err / bound).max(),
                  "bit-equal", mine.tobytes() == np.asarray(host).tobytes())
            assert (err <= bound).all(), (key, gamma, err.max())
            if 0 < rank < n:
                want = _longdouble_min_norm(Gq, cq, info["orig"], rank)
                err = np.abs(mine.astype(np.longdouble) - want).astype(np.float64)
                bound = M.var_bound(want.astype(np.float64).astype(np.float32), cond, n)
                print("   against extended precision: max err / bound %.3g" % (err / bound).max())
                assert (err <= bound).all(), (key, gamma, err.max())


# ---- (ii) full rank: the existing entry's model ----------------------------------------------------------------------------------
@pytest.mark.parametrize("key", K.FULL)
def test_a_full_rank_sweep_is_the_existing_models_byte_for_byte(key):
    G, coef = K.inputs(key)
    qs, qx = C.matrices(coef)
    for gamma in K.GAMMAS:
        for max_iter in K.MAX_ITERS:
            new, _ = swept(key, gamma, max_iter)
            old = M0.sweep(G, coef.d, gamma, K.THRESHOLD, max_iter, qs, qx, coef.allow_constant, band=K.BAND)
            assert old["fell"] == 0 and new["trunc"] == 0 and new["fell"] == 0
            for name in ("xi", "var", "mask"):
                assert new[name].tobytes() == old[name].tobytes(), (key, gamma, max_iter, name)
            assert (new["passes"], new["near"]) == (old["passes"], old["near"])


# ---- (iii) the host loop ---------------------------------------------------------------------------------------------------------
def _replayed(G, coef, gamma, order):
    """``_DeviceSTLSQ._replay(..., 'min_norm')`` on one matrix: what solve(device=True, coef=) returns for a flagged problem."""
    from symode_amd.sweep import _DeviceSTLSQ
    sw = _DeviceSTLSQ()
    sw.n_points, sw.d, sw.near_threshold = K.N_POINTS, coef.d, []
    Xi = np.zeros((1, coef.d, coef.p), dtype=np.float32)
    mask, passes = np.ones((1, coef.d, coef.p), dtype=bool), np.zeros(1, dtype=np.int64)
    sw._replay(0, G, gamma, K.THRESHOLD, 10, "min_norm", Xi, mask, passes, coef)
    return Xi[0], mask[0], int(passes[0])


@pytest.mark.parametrize("key", K.ALL)
def test_the_models_sweep_against_the_host_loop(key):
    G, coef = K.inputs(key)
    qx = coef.xi_matrix()
    for gamma in K.GAMMAS:
        out, trace = swept(key, gamma)
        xi, mask, passes = _replayed(G, coef, gamma, None)
        assert np.array_equal(out["mask"], mask) and out["passes"] == passes, (key, gamma, out["passes"], passes)
        info, Gq = trace[-1][5], trace[-1][2]
        cond = M.pass_cond(info, Gq)
        assert cond <= K.COND_BOUND
        bound = 2 * (M.xi_bound if info["rank"] < info["n"] else M0.xi_bound)(qx, out["var"], cond, info["n"], coef.d, coef.p,
                                                                             coef.allow_constant)
        err = np.abs(out["xi"].astype(np.float64) - xi)
        print(key, gamma, "passes", passes, "max |dXi| / bound %.3g" % (err / bound).max())
        assert (err <= bound).all(), (key, gamma, err.max())


# ---- (iv) the conditions on the inputs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", K.TRUNCATED)
def test_every_truncated_pass_decides_its_rank_with_a_margin(key):
    seen = 0
    for gamma in K.GAMMAS:
        out, trace = swept(key, gamma)
        for _, _, Gq, _, _, info in trace:
            n, rank, fact, R = info["n"], info["rank"], info["fact"], info["R"]
            if not 0 < rank < n:
                continue
            seen += 1
            first = abs(R[0, 0])
            kept = abs(R[rank - 1, rank - 1])
            dropped = abs(R[rank, rank]) if rank < fact else 0.0                         # (a pivot that is not > 0: no row of R)
            cond = M.truncated_cond(info)
            print(key, gamma, "n", n, "rank", rank, "dropped / cut %.3g" % (dropped / (M.RCOND * first)), "kept / R00 %.3g" % (kept / first),
                  "cond %.3g" % cond)
            assert kept >= 100 * M.RCOND * first, (key, gamma, kept / first)
            assert dropped <= M.RCOND * first / 2, (key, gamma, dropped / first)
            assert cond <= K.COND_BOUND, (key, gamma, cond)
    assert seen >= 2
