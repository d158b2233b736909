"""What the six engine.stlsq_* wrappers share -- the packed result, its one copy to the host, the tail, path_xi -- on the
synthetic operands of tests/stlsq_wrapper_cases.py (no model flags one of them: tests/test_host_stlsq_wrapper_cases.py).  The
fits themselves are checked against the numpy models by the tests of each launch."""
import numpy as np
import pytest
import torch

from tests import stlsq_wrapper_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


def _calls(eng, d, p, allow_constant):
    """{wrapper: [call(**kw) for the scalar launch, ... for the grid of 6 problems]}"""
    o = {k: torch.from_numpy(v).to(DEV) for k, v in W.operands(d, p, allow_constant).items()}
    G, V, R, qs, qx = o["G"], o["V"], o["R"], o["q_solve"], o["q_xi"]
    table = lambda *cols: torch.tensor(np.stack(cols, axis=1), dtype=torch.float32, device=DEV)     # noqa: E731
    t2, t3, tp = table(W.GAMMAS, W.THRESHOLDS), table(W.GAMMAS, W.THRESHOLDS, W.W_SYMS), table(W.GAMMAS, W.W_SYMS)
    fit = (W.N_POINTS, W.GAMMA, W.THRESHOLD, W.MAX_ITER)
    q = (qs, qx, allow_constant)
    return {
        "stlsq_sweep": [lambda **kw: eng.stlsq_sweep(G, *fit, d=d, near_band=W.BAND, **kw),
                        lambda **kw: eng.stlsq_sweep(G, *fit, hyper=t2, d=d, near_band=W.BAND, **kw)],
        "stlsq_sweep_constrained": [
            lambda **kw: eng.stlsq_sweep_constrained(G, *fit, *q, d=d, pivot_floor=W.PIVOT_FLOOR, near_band=W.BAND, **kw),
            lambda **kw: eng.stlsq_sweep_constrained(G, *fit, *q, hyper=t2, d=d, pivot_floor=W.PIVOT_FLOOR, near_band=W.BAND, **kw)],
        "stlsq_sweep_minnorm": [
            lambda **kw: eng.stlsq_sweep_minnorm(G, *fit, *q, d=d, rcond=W.RCOND, near_band=W.BAND, **kw),
            lambda **kw: eng.stlsq_sweep_minnorm(G, *fit, *q, hyper=t2, d=d, rcond=W.RCOND, near_band=W.BAND, **kw)],
        "stlsq_sweep_symreg": [
            lambda **kw: eng.stlsq_sweep_symreg(G, R, W.N_POINTS, W.GAMMA, W.THRESHOLD, W.W_SYM, W.MAX_ITER, d=d, pivot_floor=W.PIVOT_FLOOR,
                                                near_band=W.BAND, **kw),
            lambda **kw: eng.stlsq_sweep_symreg(G, R, W.N_POINTS, W.GAMMA, W.THRESHOLD, W.W_SYM, W.MAX_ITER, hyper=t3, d=d,
                                                pivot_floor=W.PIVOT_FLOOR, near_band=W.BAND, **kw)],
        "stlsq_path": [lambda **kw: eng.stlsq_path(G, V, W.N_POINTS, W.GAMMA, W.TOL, W.FLOOR_REL, d=d, near_band=W.BAND, **kw),
                       lambda **kw: eng.stlsq_path(G, V, W.N_POINTS, W.GAMMA, W.TOL, W.FLOOR_REL, W.GRID, d=d, near_band=W.BAND, **kw)],
        "stlsq_path_symreg": [
            lambda **kw: eng.stlsq_path_symreg(G, R, V, W.N_POINTS, W.GAMMA, W.W_SYM, W.TOL, W.FLOOR_REL, d=d, pivot_floor=W.PIVOT_FLOOR,
                                               near_band=W.BAND, **kw),
            lambda **kw: eng.stlsq_path_symreg(G, R, V, W.N_POINTS, W.GAMMA, W.W_SYM, W.TOL, W.FLOOR_REL, hyper=tp, d=d,
                                               pivot_floor=W.PIVOT_FLOOR, near_band=W.BAND, **kw)],
    }


def _same(host, device):
    assert isinstance(host, np.ndarray) and isinstance(device, torch.Tensor) and device.is_cuda
    back = device.cpu().numpy()
    assert host.dtype == back.dtype and host.shape == back.shape and host.tobytes() == back.tobytes()


@pytest.mark.parametrize("allow_constant", (False, True))
@pytest.mark.parametrize("d,p", W.SHAPES)
def test_the_sweeps_return_the_same_bytes_on_either_side_and_carry_the_tail(eng, d, p, allow_constant):
    calls = _calls(eng, d, p, allow_constant)
    tail = torch.tensor([7, -1, 2 ** 30], dtype=torch.int32, device=DEV)
    r1 = W.R_FREE + (d if allow_constant else 0)
    for name, n_out in (("stlsq_sweep", 5), ("stlsq_sweep_constrained", 6), ("stlsq_sweep_minnorm", 8), ("stlsq_sweep_symreg", 5)):
        for call, n in zip(calls[name], (W.S, W.GRID)):
            on_device, on_host = call(), call(to_host=True)
            assert isinstance(on_device, tuple) and isinstance(on_host, tuple) and len(on_device) == len(on_host) == n_out, name
            for h, t in zip(on_host, on_device):
                _same(h, t)
            xi, mask, passes, near, fell = on_device[:5]
            assert xi.shape == mask.shape == (n, d, p) and xi.dtype == torch.float32 and mask.dtype == torch.uint8, name
            assert all(t.shape == (n,) and t.dtype == torch.int32 for t in (passes, near, fell) + tuple(on_device[6:])), name
            assert n_out == 5 or (on_device[5].shape == (n, r1) and on_device[5].dtype == torch.float32), name
            assert not fell.any().item() and passes.min().item() >= 1, (name, fell.tolist())      # real fits
            assert len({t.untyped_storage().data_ptr() for t in on_device}) == 1, name             # one allocation
            with_tail, with_tail_host = call(tail=tail), call(tail=tail, to_host=True)
            assert len(with_tail) == len(with_tail_host) == n_out + 1, name
            assert torch.equal(with_tail[-1], tail) and with_tail_host[-1].tolist() == tail.tolist(), name
            assert with_tail[-1].data_ptr() % 4 == 0 and with_tail[-1].untyped_storage().data_ptr() == with_tail[0].untyped_storage().data_ptr()
            for h, t, plain in zip(with_tail_host, with_tail, on_device):
                _same(h, t)
                assert torch.equal(t, plain), name                                                 # the tail changes no result


@pytest.mark.parametrize("d,p", W.SHAPES)
def test_the_paths_return_the_same_bytes_on_either_side_and_path_xi_only_when_kept(eng, d, p):
    calls = _calls(eng, d, p, False)
    n0 = d * p
    for name, small, shape in (("stlsq_path", ("Xi", "mask", "order", "rss_train", "rss_val", "best", "near", "fell"), (d, p + 1, p)),
                               ("stlsq_path_symreg", ("Xi", "mask", "order", "mse_train", "reg_train", "mse_val", "best", "near", "fell"),
                                (n0 + 1, d, p))):
        for call, n in zip(calls[name], (W.S, W.GRID)):
            on_device, on_host, kept = call(), call(to_host=True), call(to_host=True, keep_path=True)
            assert list(on_device) == list(small) + ["path_xi"] == list(kept) and list(on_host) == list(small), name
            assert call(keep_path=True).keys() == on_device.keys()                                 # on the device it is always there
            for k in small:
                _same(on_host[k], on_device[k])
                _same(kept[k], on_device[k])
            _same(kept["path_xi"], on_device["path_xi"])
            assert on_device["path_xi"].shape == (n,) + shape and on_device["path_xi"].dtype == torch.float32, name
            assert on_device["Xi"].shape == on_device["mask"].shape == (n, d, p) and on_device["fell"].shape == (n,), name
            assert not on_device["fell"].any().item(), (name, on_device["fell"].tolist())          # real fits
            assert len({on_device[k].untyped_storage().data_ptr() for k in small}) == 1, name     # one allocation
