"""Device Adam trainer with the reversed symmetry regulariser (symode_adam_epochs_reversed / DeviceAdam(reversed_sym=...) /
train_SIGED(device_adam=True, sym_reg_type='r')) against the optimiser
the reference uses: the oracle regressor on the CPU under torch.optim.Adam with the loss
w_x * mse + w_sym * O.symreg_reversed_precomputed + w_reg * l1, fed exactly the same batches.  Data: the 300 rows of the
noisy quadratic field of tests/test_gpu_adam.py; two synthetic group elements, g1(x) = R(0.3) x (constant Jacobian) and
g2(x) = R(-0.2) x + 0.1 sin(x) (pointwise, nonlinear, analytic Jacobian); for d = 3 the rotations act on the first two
coordinates."""
import math

import numpy as np
import pytest
import torch

from oracle import sindy_oracle as O
from tests.test_gpu_adam import LIBS, LR, N, ROT, THR, TOL, W_REG, _DATA, _oracle, _orders, _params, _scaled_err, _table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W_SYM = 0.1
KEYS = ("params", "m", "v", "step", "mask", "xi")


@pytest.fixture(scope="module")
def S():
    import symode_amd
    assert torch.cuda.is_available()
    return symode_amd


def _rot(angle, d):
    R = torch.eye(d)
    R[0, 0], R[0, 1], R[1, 0], R[1, 1] = math.cos(angle), -math.sin(angle), math.sin(angle), math.cos(angle)
    return R


def _group(d):
    """gx (2, N, d), jgx (2, N, d, d) in fp64 (the fp32 operands are their roundings)."""
    x = _DATA[d][0].double()
    R1, R2 = _rot(0.3, d).double(), _rot(-0.2, d).double()
    gx = torch.stack([x @ R1.T, x @ R2.T + 0.1 * torch.sin(x)])
    jgx = torch.stack([R1.expand(N, d, d), R2[None] + 0.1 * torch.diag_embed(torch.cos(x))])
    return gx.contiguous(), jgx.contiguous()


_GROUP = {d: _group(d) for d in (2, 3)}


def _operands(d, n_g, dtype=torch.float32):
    gx, jgx = _GROUP[d]
    return gx[:n_g].to(dtype).contiguous(), jgx[:n_g].to(dtype).contiguous()


def _to_double(reg):
    """The oracle regressor with fp64 leaves holding the same (fp32) start."""
    if reg.constraint:
        reg.beta = reg.beta.detach().double().requires_grad_(True)
        reg.const = reg.const.detach().double().requires_grad_(True)
        reg.Q = reg.Q.double() if isinstance(reg.Q, torch.Tensor) else reg.Q
    else:
        reg.Xi = reg.Xi.detach().double().requires_grad_(True)
    reg.mask = reg.mask.double()
    return reg


def _oracle_fit(reg, d, batch, orders, n_g, st_freq=0, threshold=0.0, dtype=torch.float32):
    """The reference's loop (train.py:491-547) with loss_sym_reg = symmreg_r on precomputed operands: per-epoch means
    (mse, l1, regulariser) and, per thresholding event, (|Xi| before, mask after, raw parameters after)."""
    x, dx = (t.to(dtype) for t in _DATA[d])
    gx, jgx = _operands(d, n_g, dtype)
    opt = torch.optim.Adam(reg.parameters(), lr=LR)
    means, events = [], []
    for epoch, order in enumerate(orders):
        rec = []
        for lo in range(0, N, batch):
            rows = order[lo:lo + batch]
            mse = torch.nn.functional.mse_loss(reg(x[rows]), dx[rows])
            sym = O.symreg_reversed_precomputed(x[rows], [g[rows] for g in gx], [j[rows] for j in jgx], reg)
            l1 = sum(torch.norm(q, 1) for q in reg.parameters())
            loss = 1.0 * mse + W_SYM * sym + W_REG * l1
            opt.zero_grad()
            loss.backward()
            opt.step()
            rec.append((mse.item(), l1.item(), sym.item()))
        if st_freq > 0 and (epoch + 1) % st_freq == 0:
            before = reg.get_Xi().detach().abs().clone()
            reg.set_threshold(threshold)
            reg.mask = reg.mask.to(dtype)
            events.append((before, reg.mask.clone(), torch.cat([q.detach().reshape(-1) for q in reg.parameters()])))
        means.append(np.mean(np.array(rec), axis=0))
    return np.array(means), events


def _trainer(reg, d, order, flags, batch, n_g, st_freq=0, threshold=0.0):
    from symode_amd.coef_map import CoefMap
    from symode_amd.device_adam import DeviceAdam
    x, dx = _DATA[d]
    gx, jgx = _operands(d, n_g)
    p = O.term_count(d, order, bool(flags & 1), bool(flags & 2))
    coef = CoefMap(d, p, reg.Q, reg.use_kron_product, reg.allow_constant) if reg.constraint else CoefMap(d, p)
    return DeviceAdam(x.to(DEV), dx.to(DEV), order, bool(flags & 1), bool(flags & 2), coef, LR, 1.0, W_REG, threshold, st_freq,
                      batch, reversed_sym=(gx.to(DEV), jgx.to(DEV), W_SYM))


def _xi_params(reg):
    return reg.get_Xi().detach().double().numpy(), _params(reg)[0].double().numpy()


@pytest.mark.parametrize("n_g", [1, 2])
@pytest.mark.parametrize("batch", [64, 77, 300])
@pytest.mark.parametrize("d, order, flags, constrain_constant", LIBS)
def test_parity_with_torch_adam_on_the_oracle_regressor(S, d, order, flags, constrain_constant, batch, n_g):
    """3 epochs over the 300 rows (77: a short, padded last batch; 300: more rows than threads), one or two group elements,
    the rotation-equivariant library with the constant column free and constrained.  Condition on the inputs, checked on the
    CPU first: the same loop in fp64 agrees with the fp32 oracle to TOL / 4 -- otherwise the case would measure the
    sensitivity of Adam's first steps (g / sqrt(g^2)) to rounding, not the kernel.
    The regulariser means are compared like the MSE means, relative to themselves, above a floor of one fp32 ulp of the MSE
    mean next to which they enter the loss: under the constraint with the constant column constrained h is
    rotation-equivariant, so for g1 alone (a rotation) the exact regulariser is ZERO and every fp32 evaluation returns its own
    rounding noise (1e-15 here, fp32 and fp64 oracle apart by 50 % of it) -- no relative bound holds for such a number."""
    L = [] if constrain_constant is None else [ROT]
    orders = _orders(3)
    reg = _oracle(d, order, flags, L, bool(constrain_constant))
    reg64 = _to_double(_oracle(d, order, flags, L, bool(constrain_constant)))
    tr = _trainer(reg, d, order, flags, batch, n_g)
    p0 = _params(reg)
    means, _ = _oracle_fit(reg, d, batch, orders, n_g)
    means64, _ = _oracle_fit(reg64, d, batch, orders, n_g, dtype=torch.float64)
    (xi, par), (xi64, par64) = _xi_params(reg), _xi_params(reg64)
    floor = np.finfo(np.float32).eps * means[:, 0]
    cond = max(_scaled_err(xi, xi64), _scaled_err(par, par64), (np.abs(means - means64) / np.abs(means64))[:, 0].max(),
               (np.abs(means - means64)[:, 2] / (np.abs(means64[:, 2]) + floor / (TOL / 4))).max())
    print(f"d={d} order={order} flags={flags} cc={constrain_constant} batch={batch} n_g={n_g}: fp32 oracle vs fp64 {cond:.2e}", end="; ")
    assert cond <= TOL / 4, cond
    out = tr.fit(p0, 3, (o[None].to(DEV) for o in orders))
    err = _scaled_err(out["Xi"][0].cpu().numpy(), xi)
    perr = _scaled_err(out["params"][0].cpu().numpy(), par)
    lerr = np.abs(out["log"][:, 0, 0] - means[:, 0]) / np.abs(means[:, 0])
    serr = np.abs(out["log"][:, 0, 7] - means[:, 2]) / (np.abs(means[:, 2]) + floor / TOL)
    rerr = np.abs(out["log"][:, 0, 1] - means[:, 1]) / np.abs(means[:, 1])
    print(f"Xi {err:.2e} params {perr:.2e} mse means {lerr.max():.2e} regulariser means {serr.max():.2e} l1 means {rerr.max():.2e}")
    assert not out["nan"].any() and (out["log"][:, 0, 2] == tr.steps).all() and int(out["step"][0]) == 3 * tr.steps
    assert err <= TOL and perr <= TOL, (err, perr)
    assert lerr.max() <= TOL and serr.max() <= TOL and rerr.max() <= TOL, (lerr, serr, rerr)
    assert torch.equal(out["mask"].cpu(), torch.ones(1, d, tr.coef.p))


# ------------------------------------------------------------------------------------------------ raw launches
def _raw(S, tables, params, mask=None, state=None, lib=(2, 3, 0), st_freq=2, epoch0=0, n_g=2, plain=False):
    """One launch on fresh copies of the state: symode_adam_epochs_reversed, or (``plain``) symode_adam_epochs."""
    d, order, flags = lib
    x, dx = _DATA[d]
    eng = S.get_engine()
    n_s = params.shape[0]
    p = params.to(DEV).clone()
    m, v, step = (torch.zeros_like(p), torch.zeros_like(p), torch.zeros(n_s, dtype=torch.int32, device=DEV)) if state is None \
        else (t.clone() for t in state)
    mk = torch.ones(n_s, d, p.shape[1] // d, device=DEV) if mask is None else mask.clone()
    kw = dict(lr=LR, w_reg=W_REG, threshold=THR, st_freq=st_freq, epoch0=epoch0)
    if plain:
        xi, log = eng.adam_epochs(x.to(DEV), dx.to(DEV), tables.to(DEV).contiguous(), p, m, v, step, mk, order, flags, **kw)
    else:
        gx, jgx = (t.to(DEV) for t in _operands(d, n_g)) if n_g is not None else (None, None)
        xi, log = eng.adam_epochs_reversed(x.to(DEV), dx.to(DEV), gx, jgx, tables.to(DEV).contiguous(), p, m, v, step, mk, order,
                                           flags, w_sym=W_SYM, **kw)
    torch.cuda.synchronize()
    return {"params": p, "m": m, "v": v, "step": step, "mask": mk, "xi": xi, "log": log}


def _same(a, b, keys=KEYS + ("log",)):
    return all(torch.equal(a[k], b[k]) for k in keys)


@pytest.fixture(scope="module")
def three():
    g = torch.Generator().manual_seed(11)
    return torch.randn(3, 20, generator=g) * 0.3


@pytest.mark.parametrize("own_tables", [False, True])
@pytest.mark.parametrize("empty", [None, 0])
def test_without_group_elements_it_is_the_plain_entry_bit_for_bit(S, three, own_tables, empty):
    """n_g = 0 (no arrays at all, or arrays with an empty first axis), a nonzero w_sym notwithstanding: one shared table and
    per-problem tables, batch 77 (padded) with thresholding events at epochs 1 and 3."""
    tabs = torch.cat([_table(_orders(4, seed=20 + s)) for s in range(3)], dim=1) if own_tables else _table(_orders(4))
    plain = _raw(S, tabs, three, plain=True)
    rev = _raw(S, tabs, three, n_g=empty)
    assert _same(plain, rev, KEYS)
    assert torch.equal(plain["log"][:, :, :7], rev["log"][:, :, :7]) and (rev["log"][:, :, 7] == 0).all()
    assert (plain["mask"] == 0).any() and plain["step"].tolist() == [16, 16, 16]


def test_the_regulariser_moves_the_fit(S, three):
    """(guards the tests below against comparing two runs that ignore the operands)"""
    t = _table(_orders(4))
    assert not torch.equal(_raw(S, t, three[:1])["params"], _raw(S, t, three[:1], plain=True)["params"])
    assert not torch.equal(_raw(S, t, three[:1])["params"], _raw(S, t, three[:1], n_g=1)["params"])
    assert (_raw(S, t, three[:1])["log"][:, 0, 7] > 0).all()


def test_two_identical_calls_are_bit_identical(S, three):
    t = _table(_orders(4))
    assert _same(_raw(S, t, three[:1]), _raw(S, t, three[:1]))


def test_four_epochs_equal_two_plus_two(S, three):
    t = _table(_orders(4))
    whole = _raw(S, t, three[:1])
    a = _raw(S, t[:2], three[:1])
    b = _raw(S, t[2:], a["params"], mask=a["mask"], state=(a["m"], a["v"], a["step"]), epoch0=2)
    assert _same(whole, b, KEYS)
    assert torch.equal(whole["log"], torch.cat([a["log"], b["log"]]))
    assert whole["log"][:, 0, 5].tolist() == [0, 1, 0, 1]                      # the events at epochs 1 and 3 took place
    assert int(whole["step"][0]) == 16 and (a["mask"] == 0).any()


def test_per_problem_tables_equal_single_problem_calls(S, three):
    tabs = [_table(_orders(4, seed=20 + s)) for s in range(3)]
    out = _raw(S, torch.cat(tabs, dim=1), three)
    for s in range(3):
        one = _raw(S, tabs[s], three[s:s + 1])
        for k in KEYS:
            assert torch.equal(out[k][s:s + 1], one[k]), (s, k)
        assert torch.equal(out["log"][:, s:s + 1], one["log"]), s
    assert not torch.equal(out["params"][0], out["params"][1])


def test_extra_padding_columns_change_nothing(S, three):
    t = _table(_orders(4))
    wide = torch.cat([t, torch.full((4, 1, 4, 200), -1, dtype=torch.int32)], dim=3)       # 277 columns: a second chunk of pads
    past = wide.clone()
    past[:, :, :, 100:110] = N                                                             # n_src: one past the end
    base = _raw(S, t, three[:1])
    assert _same(base, _raw(S, wide, three[:1])) and _same(base, _raw(S, past, three[:1]))


def test_a_nan_problem_is_frozen_and_isolated(S, three):
    t = _table(_orders(4))
    start = three.clone()
    start[1] = float("inf")
    out = _raw(S, t, start)
    assert out["step"].tolist() == [16, -1, 16]
    assert torch.isinf(out["params"][1]).all() and (out["m"][1] == 0).all() and (out["mask"][1] == 1).all()
    assert (out["log"][:, 1, 4] == 1).all() and (out["log"][:, 1, 2] == 0).all() and (out["log"][:, [0, 2], 4] == 0).all()
    for s in (0, 2):
        one = _raw(S, t, three[s:s + 1])
        for k in KEYS:
            assert torch.equal(out[k][s:s + 1], one[k]), (s, k)
        assert torch.equal(out["log"][:, s:s + 1], one["log"])


# ------------------------------------------------------------------------------------------------ thresholding in the launch
def test_thresholding_inside_the_launch_with_the_regulariser_on(S):
    from symode_amd.sindy import NEAR_THRESHOLD_BAND
    d, order, flags, batch = 2, 3, 0, 77
    reg = _oracle(d, order, flags)
    tr = _trainer(reg, d, order, flags, batch, 2, st_freq=2, threshold=THR)
    p0, orders = _params(reg), _orders(4)
    _, events = _oracle_fit(reg, d, batch, orders, 2, st_freq=2, threshold=THR)
    # the oracle alone: both events are decided away from the threshold, and the first removes some, not all
    assert len(events) == 2
    for before, _, _ in events:
        assert ((before - THR).abs() >= NEAR_THRESHOLD_BAND).all(), (before - THR).abs().min()
    assert 0 < int((events[0][1] == 0).sum()) < events[0][1].numel()
    got = {}
    out = tr.fit(p0, 4, (o[None].to(DEV) for o in orders), epochs_per_launch=2,
                 on_epoch=lambda e, rec: got.update({e: (rec, {k: v.clone() for k, v in rec["state"].items()} if rec["state"] else None)}))
    assert [int(got[e][0]["event"][0]) for e in range(4)] == [0, 1, 0, 1] and all(got[e][0]["loss_sym_reg"][0] > 0 for e in range(4))
    for e, (_, mask, params) in zip((1, 3), events):
        assert torch.equal(got[e][1]["mask"][0].cpu(), mask), e
        assert _scaled_err(got[e][1]["params"][0].cpu().numpy(), params.numpy()) <= TOL
    assert torch.equal(out["mask"][0].cpu(), events[1][1])


# ------------------------------------------------------------------------------------------------ train_SIGED
LALIGAN = ["--latent_dim", "2", "--n_comps", "2", "--hidden_dim", "32", "--n_layers", "3", "--repr", "(2,1,2)", "--ae_arch", "mlp",
           "--ortho_ae", "--batch_norm", "--group_idx", "0"]


def _frozen_laligan(x, task="dosc"):
    """A small random LaLiGAN, batch-norm statistics warmed on the data, frozen as main.py leaves it under --fix_laligan."""
    from symode_amd.autoencoder import AutoEncoder
    from symode_amd.lie import LieGenerator
    from symode_amd.parser_utils import get_args
    args = vars(get_args(argv=["--task", task] + LALIGAN))
    args["input_dim"] = x.shape[1]
    torch.manual_seed(11)
    ae, gen = AutoEncoder(**args).to(DEV), LieGenerator(**args).to(DEV)
    ae.train()
    with torch.no_grad():
        for k in range(4):
            ae(torch.stack([x[k::4], x[k::4] * 1.05], dim=1))
    gen.masks = [m.to(DEV) if m is not None else None for m in gen.masks]
    for module in (ae, gen):
        module.eval()
        for q in module.parameters():
            q.requires_grad = False
    return ae, gen


def _regressor(S):
    torch.manual_seed(123)
    reg = S.SINDyRegression(2, 3, False, False, threshold=THR, device=DEV)
    with torch.no_grad():
        reg.Xi.mul_(0.3)
    return reg


def test_train_SIGED_device_adam_with_the_reversed_regulariser(S, capsys, tmp_path, monkeypatch):
    from symode_amd.dataset import DeviceBatches
    from symode_amd.model_utils import symmreg_r
    monkeypatch.chdir(tmp_path)
    x, dx = (t.to(DEV) for t in _DATA[2])
    ae, gen = _frozen_laligan(x)
    batch, epochs = 77, 4
    # the tensor-op loop of train_SIGED's plain branch with loss_sym_reg = symmreg_r, on the loader's own shuffles
    ref = _regressor(S)
    loader = DeviceBatches([x, dx], N, batch, True, DEV)
    opt = torch.optim.Adam(ref.parameters(), lr=LR)
    ref_sym = []
    for epoch in range(epochs):
        vals = []
        for xb, dxb in loader:
            xb = xb.contiguous()
            sym = symmreg_r(xb, ae, gen, ref, require_grad=True)
            loss = 1.0 * ref.mse_loss(xb, dxb) + W_SYM * sym + W_REG * sum(torch.norm(q, 1) for q in ref.parameters())
            opt.zero_grad()
            loss.backward()
            opt.step()
            vals.append(sym.item())
        if (epoch + 1) % 2 == 0:
            ref.set_threshold(THR)
        ref_sym.append(float(np.mean(vals)))
    ref_rng = torch.rand(1, device=DEV).item()
    got = _regressor(S)
    loader = DeviceBatches([x, dx], N, batch, True, DEV)
    test = DeviceBatches([x[:100], dx[:100]], 100, 64, False, DEV)
    ident = torch.nn.Identity()
    capsys.readouterr()
    S.train.train_SIGED(train_loader=loader, test_loader=test, num_epochs=epochs, device=DEV, log_interval=1, save_interval=10 ** 9,
                        save_dir="t", autoencoder=ae, discriminator=ident, generator=gen, lr_ae=0, lr_d=0, lr_g=0, w_recon=0,
                        w_gan=0, w_reg_norm=0, w_reg_ortho=0, w_reg_closure=0, use_original_x=False, gan_st_freq=0, gan_st_thres=0.0,
                        ae_arch="mlp", regressor=got, use_latent=False, lr_sindy=LR, w_sindy_z=0.0, w_sindy_x=1.0,
                        sindy_reg_type="l1", w_sindy_reg=W_REG, w_sym_reg=W_SYM, sym_reg_type="r", st_freq=2, threshold=THR,
                        int_t=0.1, int_dt=0.01, print_eq=False, device_adam=True)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Epoch") and "loss_sym_reg" in l]
    assert torch.rand(1, device=DEV).item() == ref_rng                       # the generator was advanced alike: the same shuffles
    assert torch.equal(got.mask, ref.mask) and 0 < int((ref.mask == 0).sum()) < ref.mask.numel()
    err = _scaled_err(got.Xi.detach().cpu().numpy(), ref.Xi.detach().cpu().numpy())
    printed = [float(l.split("loss_sym_reg: ")[1].split(",")[0]) for l in lines]
    print(f"train_SIGED device_adam + symmreg_r vs tensor-op loop: coefficient scaled err {err:.2e}; loss_sym_reg {printed} vs {ref_sym}")
    assert err <= TOL, err
    assert len(printed) == epochs and min(ref_sym) > 0
    assert np.abs(np.array(printed) - np.array(ref_sym)).max() <= 1e-4        # four decimals: one unit of the last place
