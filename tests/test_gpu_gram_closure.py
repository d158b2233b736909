"""The Gram-form closure on the GPU: symode_symreg_reversed_gram against an fp64 restatement, symode_quad_closure against the
data (fp64 restatement, the oracle along the recorded L-BFGS trajectories, the regulariser in the configs[2] setting), the
device trainer in Gram mode on the reference's recorded runs, and statistics accumulated in chunks."""
import numpy as np
import pytest
import torch

from oracle import sindy_oracle as O
from tests.helpers import f11_case, t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def S():
    import symode_amd
    assert torch.cuda.is_available()
    return symode_amd


# ---------------------------------------------------------------------------------------------------------------------
# fp64 restatement: G = A^T A with A = [Theta | dx]; R = sum_g sum_n B^T B with B[i, (j, a)] = J[i, j] theta_a(x) - d_ij theta_a(gx)
# ---------------------------------------------------------------------------------------------------------------------
def _rows_b(x, gx, jgx, order, sine, exp):
    """B (n_g, N, d, d p) in fp64 from the fp32 library (J theta exact in fp64, minus theta(g x))."""
    d = x.shape[-1]
    th = O.theta(x, order, sine, exp).double()
    out = []
    for g in range(gx.shape[0]):
        thg = O.theta(gx[g], order, sine, exp).double()
        J = jgx[g].double()
        B = torch.einsum("nij,na->nija", J, th) - torch.einsum("ij,na->nija", torch.eye(d, dtype=torch.float64), thg)
        out.append(B.reshape(x.shape[0], d, -1))
    return torch.stack(out)


def _rev_gram_ref(x, gx, jgx, order, sine=False, exp=False):
    B = _rows_b(x, gx, jgx, order, sine, exp)
    R = torch.einsum("gnir,gnis->rs", B, B)
    Rabs = torch.einsum("gnir,gnis->rs", B.abs(), B.abs())
    return R, Rabs


def _group_data(N, d, n_g, seed):
    """Points, a rotation-like group action with a little distortion, and Jacobians near the rotation."""
    gen = torch.Generator().manual_seed(seed)
    x = (torch.rand(N, d, generator=gen) * 3.0 - 1.5)
    gx, jgx = [], []
    for g in range(n_g):
        A = torch.eye(d) + 0.2 * torch.randn(d, d, generator=gen)
        gx.append(x @ A.T + 0.01 * torch.randn(N, d, generator=gen))
        jgx.append(A.expand(N, d, d) + 0.01 * torch.randn(N, d, d, generator=gen))
    return x, torch.stack(gx).contiguous(), torch.stack(jgx).contiguous()


@pytest.mark.parametrize("d,order,flags", [(2, 3, 0), (2, 5, 0), (2, 2, 2), (3, 2, 0)],
                         ids=["d2_o3", "d2_o5", "d2_o2_exp", "d3_o2"])
@pytest.mark.parametrize("n_g", [1, 3])
@pytest.mark.parametrize("n_problems", [1, 4])
def test_reversed_gram_matches_fp64_restatement(S, d, order, flags, n_g, n_problems):
    """R of every problem within 1e-12 of sum |B| |B| (polynomial libraries: exact fp64 products, only the order of the fp64
    sums differs) or 1e-6 of it (exp library: the device expf and the CPU's differ by ulps); N = 1237 is no multiple of any
    block or stage size."""
    eng = S.get_engine()
    sine, exp = bool(flags & 1), bool(flags & 2)
    N = 1237
    xs, gxs, jgxs = zip(*[_group_data(N, d, n_g, seed=10 * s + n_g) for s in range(n_problems)])
    X, GX, JGX = torch.stack(xs), torch.stack(gxs), torch.stack(jgxs)
    R = eng.symreg_reversed_gram(X.to(DEV), GX.to(DEV), JGX.to(DEV), order, flags).cpu()
    p = eng.lib_size(d, order, flags)
    assert R.shape == (n_problems, d * p, d * p) and R.dtype == torch.float64
    tol = 1e-12 if flags == 0 else 1e-6
    for s in range(n_problems):
        want, yard = _rev_gram_ref(xs[s], gxs[s], jgxs[s], order, sine, exp)
        err = ((R[s] - want).abs() / yard.clamp_min(1e-300)).max().item()
        assert err <= tol, (s, err)
        assert torch.equal(R[s], R[s].T)
    if n_problems == 1:                                          # the unbatched form
        R1 = eng.symreg_reversed_gram(xs[0].to(DEV), gxs[0].to(DEV), jgxs[0].to(DEV), order, flags).cpu()
        assert torch.equal(R1, R[0])


def test_reversed_gram_unsupported_library_raises(S):
    eng = S.get_engine()
    x, gx, jgx = _group_data(100, 3, 1, seed=0)
    with pytest.raises(S.engine.SymodeError):
        eng.symreg_reversed_gram(x.to(DEV), gx.to(DEV), jgx.to(DEV), 4, 0)        # d = 3 order 4: d p = 105


# ---------------------------------------------------------------------------------------------------------------------
# the quadratic closure
# ---------------------------------------------------------------------------------------------------------------------
def _closure_ref(x, dx, gx, jgx, Xi, M, order, w_sym, sine=False, exp=False):
    """fp64 closure from the data: (mse, reg, grad of mse + w reg, operand yardsticks of loss and gradient)."""
    N, d = x.shape
    inv = 1.0 / (N * d)
    th = O.theta(x, order, sine, exp).double()
    W = (Xi * M).double()
    r = th @ W.T - dx.double()
    mse = inv * (r ** 2).sum()
    grad = 2 * inv * (r.T @ th)
    operands = th.abs() @ W.abs().T + dx.double().abs()
    yard_g = 2 * inv * (operands.T @ th.abs())
    yard_l = inv * (operands ** 2).sum()
    reg = torch.zeros((), dtype=torch.float64)
    if gx is not None:
        B = _rows_b(x, gx, jgx, order, sine, exp)              # (n_g, N, d, d p)
        v = W.reshape(-1)
        u = B @ v
        reg = inv * (u ** 2).sum()
        gr = 2 * inv * torch.einsum("gnir,gni->r", B, u).reshape(d, -1)
        grad = grad + w_sym * gr
        Babs = B.abs()
        ua = Babs @ v.abs()
        yard_g = yard_g + w_sym * 2 * inv * torch.einsum("gnir,gni->r", Babs, ua).reshape(d, -1)
        yard_l = yard_l + w_sym * inv * (ua ** 2).sum()
    return mse, reg, grad * M.double(), yard_l, yard_g


@pytest.mark.parametrize("with_reg", [False, True], ids=["mse", "mse_reg"])
def test_quad_closure_matches_fp64_restatement(S, with_reg):
    """Random (Xi, mask) for four problems at d = 2 order 3: loss and gradient equal the fp64 closure of the data up to one
    fp32 rounding of the output and 1e-9 of the operand yardstick."""
    eng = S.get_engine()
    N, d, order, n_g, w = 3001, 2, 3, 2, 0.1
    gen = torch.Generator().manual_seed(7)
    probs = []
    for s in range(4):
        x, gx, jgx = _group_data(N, d, n_g, seed=100 + s)
        dx = torch.stack([x[:, 1], -x[:, 0] - 0.1 * x[:, 1] ** 3], 1) + 0.05 * torch.randn(N, d, generator=gen)
        Xi = torch.randn(d, 10, generator=gen) * 0.5
        M = (torch.rand(d, 10, generator=gen) > 0.3).float()
        probs.append((x, dx.contiguous(), gx, jgx, Xi, M))
    X, DX, GX, JGX, XI, MS = [torch.stack(c).to(DEV) for c in zip(*probs)]
    G = eng.aug_gram(X, DX, order)
    R = eng.symreg_reversed_gram(X, GX, JGX, order) if with_reg else None
    loss, grad = eng.quad_closure(G, R, XI, MS, 1.0 / (N * d), w)
    loss, grad = loss.cpu().double(), grad.cpu().double()
    for s, (x, dx, gx, jgx, Xi, M) in enumerate(probs):
        mse, reg, gw, yl, yg = _closure_ref(x, dx, gx if with_reg else None, jgx, Xi, M, order, w)
        got_mse = loss[s, 0] if with_reg else loss[s]
        assert abs(got_mse - mse) <= 2 ** -24 * abs(mse) + 1e-9 * yl, (s, got_mse.item(), mse.item())
        if with_reg:
            assert abs(loss[s, 1] - reg) <= 2 ** -24 * abs(reg) + 1e-9 * yl, (s, loss[s, 1].item(), reg.item())
        err = (grad[s] - gw).abs() - 2 ** -24 * gw.abs()
        assert (err <= 1e-9 * yg).all(), (s, (err / yg).max().item())


def _check_trace(eng, x, dx, trace, order, what):
    """The Gram-form closure at every recorded closure point against the oracle's, on the yardsticks of
    test_hip_closure_along_the_recorded_lbfgs_trajectory (gradient 1e-5 of the operand magnitude; loss 1e-5 relative or,
    at the noise-free floor, 1e-8 of the loss's own operand yardstick -- see the docstring of the caller)."""
    n = len(trace)
    Xi = torch.stack([a for a, _ in trace]).to(DEV)
    M = torch.stack([b for _, b in trace]).to(DEV)
    G = eng.aug_gram(x.to(DEV), dx.to(DEV), order)
    loss, grad = eng.quad_closure(G[None].expand(n, -1, -1).contiguous(), None, Xi, M, 1.0 / x.numel())
    loss, grad = loss.cpu().numpy(), grad.cpu().numpy()
    th = O.theta(x, order).double().abs()
    worst_l = worst_g = 0.0
    for k, (a, b) in enumerate(trace):
        wl, wg = O.mse_loss_and_grad(x, dx, a, b, order)
        wl, wg = wl.item(), wg.numpy()
        operands = th @ (a * b).double().abs().T + dx.double().abs()
        yard = (2.0 / operands.numel()) * (operands.T @ th).numpy()
        yard_l = ((operands ** 2).sum() / operands.numel()).item()
        worst_l = max(worst_l, abs(loss[k] - wl) / max(1e-5 * abs(wl), 1e-8 * yard_l) * 1e-5)
        live = b.numpy() > 0
        worst_g = max(worst_g, (np.abs(grad[k] - wg)[live] / yard[live]).max())
    print(f"{what}: {n} closure points, loss err {worst_l:.2e} (1e-5 = limit), grad err vs operand magnitude {worst_g:.2e}")
    assert worst_l <= 1e-5, worst_l
    assert worst_g <= 1e-5, worst_g


@pytest.mark.parametrize("tag", ["dosc_sindy", "dosc_esindy", "selkov_sindy"])
def test_quad_closure_along_the_recorded_lbfgs_trajectory(S, golden, tag):
    """Every closure point of the pinned oracle run (f4), through ONE launch of symode_quad_closure on the batch's Gram
    matrix.  One known difference: at the noise-free floor the Gram form gives the exact loss of the fp32 features, the
    oracle the loss of an fp32-ROUNDED residual (a sum of squared rounding errors there), so the loss is held to 1e-5 of
    itself or 1e-8 of its operand yardstick (1/(N d) sum (|Theta| |w| + |dx|)^2), whichever is larger; the gradient to 1e-5
    of its operand yardstick, as the streaming kernel is."""
    from tests.test_gpu_parity_round2 import _oracle_run
    g = golden("f4_lbfgs")
    reg, hist, x, dx, order = _oracle_run(g, tag)
    assert len(reg.trace) == hist["n_closure"] and len(reg.trace) >= 10
    _check_trace(S.get_engine(), x, dx, reg.trace, order, tag)


F11_CASES = ["dosc_n20_o3", "dosc_n20_o2", "selkov_n20_o3", "dosc_n20_so2", "growth_n05_scaling2", "growth_n05_o2",
             "dosc_n20_o3_edge"]


@pytest.mark.parametrize("tag", F11_CASES)
def test_quad_closure_along_the_noisy_trajectory(S, golden, tag):
    """The same at every closure point of the reference's recorded noisy runs (f11 traces)."""
    c = f11_case(golden("f11_lbfgs_noisy"), tag)
    _check_trace(S.get_engine(), c["x"], c["dx"], list(zip(c["trace_Xi"], c["trace_mask"])), c["order"], "f11 " + tag)


def test_quad_closure_with_the_regulariser_in_the_config2_setting(S):
    """configs[2] shape (lv, order 2 + exp, 20 000 points, tiny frozen autoencoder): mse + 0.1 reg and its gradient from
    G and R equal the oracle's closure with O.symreg_reversed_precomputed, within the tolerances of
    test_config2_lv_exp_library_symreg_reversed_closure."""
    import os
    from tests.helpers import TinyAE
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "f6_symreg.npz"))
    x, dx = S.data.make_dataset("lv", 200, 10000, dt=0.002, noise=0.0, seed=4, device=DEV)
    gsel = torch.Generator().manual_seed(0)
    rows = torch.randperm(x.shape[1], generator=gsel)[:20000].to(DEV)
    xc, dxc = x[0][rows].cpu().contiguous(), dx[0][rows].cpu().contiguous()
    torch.manual_seed(3)
    Xi = torch.randn(2, 8) * 0.3
    tae = TinyAE(g, "tanh_learn", "Tanh")
    gel = [t(e) for e in g["tanh_learn_gelems_r"]]
    gx, Jgx = O.precompute_group_jacobians(xc, tae.encode, tae.decode, tae.z_mean, gel)
    reg = O.OracleRegressor(2, 2, False, True, Xi0=Xi)
    lo = torch.nn.functional.mse_loss(reg(xc), dxc) + 0.1 * O.symreg_reversed_precomputed(xc, gx, Jgx, reg)
    lo.backward()
    from symode_amd.gram_closure import GramStatistics
    st = GramStatistics(1, 2, 2, 2, regulariser=True, device=DEV)
    st.add(xc.to(DEV), dxc.to(DEV), torch.stack(gx).to(DEV), torch.stack(Jgx).to(DEV))
    assert st.count == 20000
    loss, grad, none = st.evaluate(Xi.to(DEV)[None], torch.ones(1, 2, 8, device=DEV), w_sym=0.1)
    assert none is None
    assert np.isclose(loss.item(), lo.item(), rtol=2e-5), (loss.item(), lo.item())
    gw = reg.Xi.grad.numpy()
    assert np.abs(grad[0].cpu().numpy() - gw).max() <= 5e-5 * np.abs(gw).max()


# ---------------------------------------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------------------------------------
def _regressor(S, g, tag, d, order, thr):
    if f"{tag}_init_Xi" in g.files:
        r = S.SINDyRegression(d, order, False, False, threshold=thr, device=DEV)
        r.Xi.data = t(g[f"{tag}_init_Xi"]).to(DEV)
    else:
        r = S.SINDyRegression(d, order, False, False, L_list=[torch.tensor([[0.0, 1.0], [-1.0, 0.0]])], threshold=thr,
                              device=DEV, constrain_constant=False)
        r.Q = t(g[f"{tag}_Q"]).to(DEV)
        r.beta.data, r.const.data = t(g[f"{tag}_init_beta"]).to(DEV), t(g[f"{tag}_init_const"]).to(DEV)
    return r


@pytest.mark.parametrize("tag", ["dosc_sindy", "dosc_esindy", "selkov_sindy"])
def test_gram_closure_trainer_matches_reference_run(S, golden, tag, tmp_path, monkeypatch):
    """train_SIGED_lbfgs(gram_closure=True) on the reference's three recorded runs: the reference's final mask exactly,
    coefficients within the tolerances of the streaming device trainer (test_gpu_train.py)."""
    monkeypatch.chdir(tmp_path)
    g = golden("f4_lbfgs")
    d, order = [int(v) for v in g[f"{tag}_cfg"]]
    lr, st_freq, thr, epochs = g[f"{tag}_hp"]
    x, dx = t(g[f"{tag}_x"]), t(g[f"{tag}_dx"])
    r = _regressor(S, g, tag, d, order, float(thr))
    ident = torch.nn.Identity()
    S.train.train_SIGED_lbfgs(train_loader=[(x, dx)], test_loader=[], num_epochs=int(epochs), device=DEV,
                              log_interval=10 ** 9, save_interval=10 ** 9, save_dir="t", autoencoder=ident, generator=ident,
                              regressor=r, regressor_dst=None, use_latent=False, distill_latent=False, lr_sindy=float(lr),
                              w_sindy_z=0.0, w_sindy_x=1.0, sindy_reg_type="l1", w_sindy_reg=0.0, sym_reg_type="i",
                              w_sym_reg=0.0, st_freq=int(st_freq), threshold=float(thr), int_t=0.1, int_dt=0.01, print_eq=False,
                              gram_closure=True)
    m = g[f"{tag}_mask_final"]
    assert np.array_equal(r.mask.cpu().numpy(), m)
    want = g[f"{tag}_Xi_final"]
    got = r.get_Xi().detach().cpu().numpy()
    atol = 1e-3 if tag == "selkov_sindy" else 1e-4
    assert np.allclose(got * m, want * m, rtol=1e-3, atol=atol), np.abs(got - want).max()


def test_gram_closure_refuses_a_path_without_the_device_trainer(S):
    g = torch.nn.Identity()
    r = S.SINDyRegression(2, 3, False, False, threshold=0.05, device=DEV)
    x = torch.randn(100, 2)
    with pytest.raises(ValueError, match="gram_closure"):
        S.train.train_SIGED_lbfgs(train_loader=[(x, x)], test_loader=[], num_epochs=1, device=DEV, log_interval=10 ** 9,
                                  save_interval=10 ** 9, save_dir="t", autoencoder=g, generator=g, regressor=r, regressor_dst=None,
                                  use_latent=False, distill_latent=False, lr_sindy=0.1, w_sindy_z=0.0, w_sindy_x=1.0,
                                  sindy_reg_type="l1", w_sindy_reg=0.0, sym_reg_type="i", w_sym_reg=0.0, st_freq=10,
                                  threshold=0.05, int_t=0.1, int_dt=0.01, print_eq=False, gram_closure=True, torch_lbfgs=True)


def test_statistics_in_four_chunks_equal_one_pass_and_fit_alike(S, golden):
    """G and R accumulated from four .add() chunks equal one .add() of the whole set to 1e-12; the device trainer fed
    either (prebuilt statistics, no point data) ends on the same mask."""
    from symode_amd.device_lbfgs import DeviceTrainer
    from symode_amd.gram_closure import GramStatistics
    g = golden("f4_lbfgs")
    tag = "dosc_sindy"
    d, order = [int(v) for v in g[f"{tag}_cfg"]]
    lr, st_freq, thr, epochs = [float(v) for v in g[f"{tag}_hp"]]
    x, dx = t(g[f"{tag}_x"]).to(DEV)[None], t(g[f"{tag}_dx"]).to(DEV)[None]
    N = x.shape[1]
    rot = torch.matrix_exp(0.01 * torch.tensor([[0.0, 1.0], [-1.0, 0.0]])).to(DEV)
    gx = (x @ rot.T)[:, None].contiguous()
    jgx = rot.expand(1, 1, N, 2, 2).contiguous()
    whole = GramStatistics(1, d, order, regulariser=True, device=DEV).add(x, dx, gx, jgx)
    parts = GramStatistics(1, d, order, regulariser=True, device=DEV)
    cuts = [0, N // 5, N // 2, N // 2 + 7, N]
    for a, b in zip(cuts[:-1], cuts[1:]):
        parts.add(x[:, a:b].contiguous(), dx[:, a:b].contiguous(), gx[:, :, a:b].contiguous(), jgx[:, :, a:b].contiguous())
    assert parts.count == whole.count == N
    for A, B in ((parts.G, whole.G), (parts.R, whole.R)):
        assert ((A - B).abs().max() / B.abs().max()).item() <= 1e-12
    Xi0 = t(g[f"{tag}_init_Xi"]).reshape(1, -1)
    out = []
    for st in (whole, parts):
        tr = DeviceTrainer(None, None, order, 0, reversed_sym=(None, None, 0.05), lr=lr, threshold=thr, st_freq=int(st_freq),
                           closure="gram", statistics=st)
        assert tr.x is None and tr.dx is None
        out.append(tr.fit(Xi0, int(epochs)))
    assert torch.equal(out[0]["mask"], out[1]["mask"])
    assert torch.allclose(out[0]["Xi"], out[1]["Xi"], rtol=1e-4, atol=1e-5)
