"""``SeedSweepSTLSQ.solve(..., min_norm=True)`` and ``main_sweep --min_norm_stlsq`` without a GPU: the three refusals of the
keyword by name, the flag's parsing and refusal text, and the routing of ``_solve_device`` on an engine whose launch is
tests/stlsq_minnorm_model.py -- which problems still reach the host loop, with which rule, and the one warning."""
import warnings

import numpy as np
import pytest
import torch

from tests import stlsq_constrained_cases as C
from tests import stlsq_minnorm_cases as K
from tests import stlsq_minnorm_model as M
from tests.test_host_sweep_plan import ENGINE, TEXT, _args, _untouchable

WORDS = "singular normal equations under the full-rank (gels) driver: minimum-norm solution returned instead"
REFUSAL = ("--min_norm_stlsq needs --equiv_stlsq: it is the rank-revealing mode of the constrained device fit (collinear "
           "columns of Q on the support are solved by the minimum-norm rule inside the launch), so it needs --method stlsq "
           "--device_stlsq --equiv_stlsq --eq_constraint; the unconstrained sweep meets no such systems")


# ---- solve's refusals ----------------------------------------------------------------------------------------------------------
def _bare_sweep():
    from symode_amd.sweep import SeedSweepSTLSQ
    sw = SeedSweepSTLSQ.__new__(SeedSweepSTLSQ)
    sw.x = torch.zeros(4, 2)
    sw._solve_device = _untouchable("_solve_device")
    sw.grams = _untouchable("grams")
    return sw


def test_solve_refuses_min_norm_by_name():
    from symode_amd.coef_map import CoefMap
    coef = C.coef_map("so2_o3_cc1")
    plain = CoefMap(2, 10, None, True, True)
    sw = _bare_sweep()
    with pytest.raises(ValueError, match="min_norm=True needs device=True"):
        sw.solve(0.0, 0.1, coef=coef, min_norm=True)
    with pytest.raises(ValueError, match="min_norm=True needs device=True"):
        sw.solve(0.0, 0.1, coef=coef, min_norm=True, lstsq_driver="gelsy")
    with pytest.raises(ValueError, match="min_norm=True needs coef=<a CoefMap that holds Q>"):
        sw.solve(0.0, 0.1, device=True, min_norm=True)
    with pytest.raises(ValueError, match="min_norm=True needs coef=<a CoefMap that holds Q>"):
        sw.solve(0.0, 0.1, device=True, coef=plain, min_norm=True)
    with pytest.raises(ValueError, match="min_norm=True does not go with lstsq_driver='gelsy'"):
        sw.solve(0.0, 0.1, device=True, coef=coef, min_norm=True, lstsq_driver="gelsy")


# ---- the routing of _solve_device ------------------------------------------------------------------------------------------------
class ModelEngine:
    """An engine whose rank-revealing launch is the numpy model (and which has no other launch)."""

    def __init__(self, near=None):
        self.calls, self.near = 0, near

    def stlsq_sweep_minnorm(self, G, n_points, gamma, threshold, max_iter, q_solve, q_xi, allow_constant, hyper=None, n_problems=None,
                            *, d, rcond, near_band, to_host, tail):
        assert to_host and tail is None and rcond == 1e-7 and hyper is None
        self.calls += 1
        outs = [M.sweep(g.numpy(), d, gamma, threshold, max_iter, q_solve.numpy(), q_xi.numpy(), allow_constant, band=near_band)
                for g in G]
        i32 = lambda k: np.array([o[k] for o in outs], dtype=np.int32)                    # noqa: E731
        near = i32("near") if self.near is None else np.array(self.near, dtype=np.int32)
        return (np.stack([o["xi"] for o in outs]), np.stack([o["mask"] for o in outs]).astype(np.uint8), i32("passes"), near,
                i32("fell"), np.stack([o["var"] for o in outs]), i32("trunc"), i32("rank"))


def _sweep_on(engine, keys):
    from symode_amd.sweep import SeedSweepSTLSQ
    G = np.stack([K.inputs(k)[0] for k in keys])
    sw = SeedSweepSTLSQ.__new__(SeedSweepSTLSQ)
    sw.engine, sw.x, sw.S, sw.d, sw.p, sw.n_points = engine, torch.zeros(4, 2), len(keys), 2, 10, K.N_POINTS
    sw._gram, sw._gram_dev = G, torch.from_numpy(G)
    replays = []
    inner = sw._replay
    sw._replay = lambda s, G_s, w, t, it, driver, *a: (replays.append((s, driver)), inner(s, G_s, w, t, it, driver, *a))[1]
    return sw, replays


def _solve(sw, **kw):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        Xi, mask, passes = sw.solve(0.0, K.THRESHOLD, max_iter=10, device=True, lstsq_driver="gels", **kw)
    return Xi.numpy(), mask.numpy() > 0, np.asarray(passes), [str(w.message) for w in rec if w.category is RuntimeWarning]


def test_a_truncated_problem_costs_no_host_work_and_one_warning():
    coef = C.coef_map("so2_o3_cc1")
    eng = ModelEngine()
    sw, replays = _sweep_on(eng, ["rankdef", "so2_o3_cc1"])
    Xi, mask, passes, said = _solve(sw, coef=coef, min_norm=True)
    assert eng.calls == 1 and replays == [] and said == [WORDS]
    assert sw.rank_truncated.tolist() == [True, False] and sw.near_threshold == []
    # ... and the answer is the host loop's minimum-norm answer for the problem the old route hands over
    want, replays = _sweep_on(None, ["rankdef"])
    x1, m1, p1 = np.zeros((1, 2, 10), dtype=np.float32), np.ones((1, 2, 10), dtype=bool), np.zeros(1, dtype=np.int64)
    want.near_threshold = []
    want._replay(0, K.inputs("rankdef")[0], 0.0, K.THRESHOLD, 10, "min_norm", x1, m1, p1, coef)
    assert np.array_equal(mask[0], m1[0]) and passes[0] == p1[0] and mask[0].sum() > 0
    info_trace = []
    out = M.sweep(K.inputs("rankdef")[0], 2, 0.0, K.THRESHOLD, 10, *C.matrices(coef), coef.allow_constant, band=K.BAND, trace=info_trace)
    info = info_trace[-1][5]
    bound = 2 * M.xi_bound(coef.xi_matrix(), out["var"], M.truncated_cond(info), info["n"], 2, 10, coef.allow_constant)
    assert (np.abs(Xi[0].astype(np.float64) - x1[0]) <= bound).all()


def test_no_truncation_no_warning():
    eng = ModelEngine()
    sw, replays = _sweep_on(eng, ["so2_o3_cc1"])
    _, _, _, said = _solve(sw, coef=C.coef_map("so2_o3_cc1"), min_norm=True)
    assert replays == [] and said == [] and sw.rank_truncated.tolist() == [False]


def test_a_near_threshold_problem_is_replayed_with_the_rule_the_launch_applied():
    eng = ModelEngine(near=[1, 2])
    sw, replays = _sweep_on(eng, ["rankdef", "so2_o3_cc1"])
    _, _, _, said = _solve(sw, coef=C.coef_map("so2_o3_cc1"), min_norm=True)
    assert replays == [(0, "min_norm"), (1, "gels")] and said == [WORDS]


# ---- the flag ------------------------------------------------------------------------------------------------------------------
EQ = dict(eq_constraint=True)


def test_the_flag_is_refused_by_name_without_equiv_stlsq():
    from symode_amd.main_sweep import _refusal
    for method, over, device in (("stlsq", EQ, True), ("stlsq", {}, False), ("lbfgs", EQ, False), ("lbfgs", {}, True)):
        assert _refusal(_args("lbfgs", "cuda:0", **over), method, device_stlsq=device, min_norm_stlsq=True) == REFUSAL
    assert _refusal(_args("lbfgs", "cuda:0", **EQ), "stlsq", wsindy=True, min_norm_stlsq=True) == REFUSAL
    # with --equiv_stlsq the flag adds no rule: the answers are that flag's
    ok = dict(device_stlsq=True, equiv_stlsq=True)
    for over in (EQ, dict(EQ, constrain_constant=True), dict(EQ, lstsq_driver="gels")):
        assert _refusal(_args("lbfgs", "cuda:0", **over), "stlsq", min_norm_stlsq=True, **ok) is None
    assert _refusal(_args("lbfgs", "cuda:0", **EQ), "stlsq", stlsq_grid=["threshold=0.05,0.1"], n_seeds=4, min_norm_stlsq=True, **ok) is None
    for over, flags in ((dict(EQ, lstsq_driver="gelsy"), ok), ({}, ok), (EQ, dict(equiv_stlsq=True))):
        assert _refusal(_args("lbfgs", "cuda:0", **over), "stlsq", min_norm_stlsq=True, **flags) == \
            _refusal(_args("lbfgs", "cuda:0", **over), "stlsq", **flags) != None                  # noqa: E711
    # and without it nothing changes
    assert _refusal(_args("lbfgs", "cuda:0", **EQ), "stlsq", device_stlsq=True) == TEXT["stlsq_eq"]
    assert _refusal(_args("lbfgs", "cuda:0", **EQ), "stlsq", min_norm_stlsq=False, **ok) is None


STLSQ = ["--task", "dosc", "--sindy_optimizer", "lbfgs", "--method", "stlsq", "--n_seeds", "2"]


@pytest.mark.parametrize("extra", [["--min_norm_stlsq"], ["--min_norm_stlsq", "--device_stlsq", "--eq_constraint"],
                                   ["--device_stlsq", "--min_norm_stlsq"]])
def test_the_flag_is_popped_and_its_refusal_comes_before_data_set_and_process_group(extra, monkeypatch):
    import torch.distributed as dist
    from symode_amd import main_sweep
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(main_sweep, "get_dataset", _untouchable("get_dataset"))
    monkeypatch.setattr(main_sweep, "init_ranks", _untouchable("init_ranks"))
    monkeypatch.setattr(dist, "init_process_group", _untouchable("init_process_group"))
    with pytest.raises(SystemExit) as e:
        main_sweep.main(STLSQ + extra, engine=ENGINE)
    assert str(e.value.code) == REFUSAL


def test_an_accepted_run_reaches_the_data_set_with_the_flag_gone_from_argv(monkeypatch):
    from symode_amd import main_sweep

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()

    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(main_sweep, "init_ranks", lambda *a, **k: None)
    monkeypatch.setattr(main_sweep, "get_dataset", stop)
    with pytest.raises(Reached):
        main_sweep.main(STLSQ + ["--device_stlsq", "--equiv_stlsq", "--eq_constraint", "--min_norm_stlsq"], engine=ENGINE)


def test_the_summary_line_counts_the_truncated_problems():
    import types

    from symode_amd import main_sweep
    sw = types.SimpleNamespace(rank_truncated=np.array([True, False, True, False, False]))
    assert main_sweep._min_norm_lines(sw, dict(coef=None)) == []
    assert main_sweep._min_norm_lines(sw, dict(coef=None, min_norm=True)) == [
        "rank-truncated passes (minimum-norm solution inside the launch): 2 of 5 problems"]
