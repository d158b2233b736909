"""The latent L-BFGS fit on the fused path, above the kernel, on the CPU: the fifth route of _lbfgs_route and what it
refuses, and the algebra of model_utils.latent_operands (QR reduction of the decoder's Jacobian, the d / D factor, the
constant e0) against the reference-shaped closure of train._autograd_closure in fp64."""
import itertools

import pytest
import torch

from symode_amd import train as T
from symode_amd.model_utils import latent_operands
from symode_amd.sindy import SINDyRegression
from symode_amd.train import _lbfgs_route
from tests.latent_cases import closure_from_operands, random_points, seeded_autoencoder
from tests.oracle_engine import OracleEngine
from tests.test_host_lbfgs_route import BASE, GRAM_MSG, GROUP_MSG, SHARDS, _outcome

torch.set_num_threads(4)

LATENT = dict(BASE, use_latent=True, fused_latent=True, w_sindy_z=1.0, has_latent=True)
NEEDS = "fused_latent=True needs "
TABLE = [
    ({}, "latent"),
    (dict(sindy_reg_type="none"), "latent"),
    (dict(w_sindy_x=0.0), "latent"),                       # the x-term is logged whatever its weight
    (dict(w_sym_reg=0.1, sym_reg_type="r"), "latent"),     # the latent closure has no symmetry term (train.py:647-661)
    (dict(is_cuda=False), NEEDS + "a GPU"),
    (dict(host_lbfgs=False), NEEDS + "host_lbfgs=True"),
    (dict(torch_lbfgs=True), NEEDS + "the device optimiser: no torch_lbfgs / numpy_lbfgs / SYMODE_TORCH_OPTIM=1"),
    (dict(numpy_lbfgs=True), NEEDS + "the device optimiser: no torch_lbfgs / numpy_lbfgs / SYMODE_TORCH_OPTIM=1"),
    (dict(torch_optim_env=True), NEEDS + "the device optimiser: no torch_lbfgs / numpy_lbfgs / SYMODE_TORCH_OPTIM=1"),
    (dict(w_sindy_z=0.0), NEEDS + "w_sindy_z > 0"),
    (dict(w_sindy_z=-1.0), NEEDS + "w_sindy_z > 0"),
    (dict(sindy_reg_type="l2"), NEEDS + "sindy_reg_type 'l1' or 'none'"),
    (dict(mask_numel=257), NEEDS + "at most 256 coefficients"),
    (dict(has_latent=False), NEEDS + "symode_loss_grad_latent and the device trainer in the library"),
    (dict(has_trainer=False), NEEDS + "symode_loss_grad_latent and the device trainer in the library"),
    (dict(gram_closure=True), NEEDS + "gram_closure=False: the latent closure has no Gram form"),
    (dict(group=SHARDS), GROUP_MSG),                       # the multi-rank latent fit stays what it was: refused
    (dict(group=SHARDS, gram_closure=True), GROUP_MSG),
    # without use_latent the keyword is ignored: the routes of the observed-space fit
    (dict(use_latent=False), "device"),
    (dict(use_latent=False, torch_lbfgs=True), "shadow"),
    (dict(use_latent=False, is_cuda=False), "plain"),
    (dict(use_latent=False, gram_closure=True, torch_lbfgs=True), GRAM_MSG),
]


@pytest.mark.parametrize("change, want", TABLE, ids=[",".join(f"{k}={v}" for k, v in c.items() if k != "group") +
                                                     (",shards" if "group" in c else "") or "default" for c, _ in TABLE])
def test_fused_latent_route_table(change, want):
    assert _outcome(**dict(LATENT, **change)) == want


def test_without_the_keyword_every_outcome_is_what_it_was():
    axes = dict(is_cuda=(False, True), use_latent=(False, True), w_sym_reg=(0.0, 0.1), sym_reg_type=("i", "f", "r"),
                w_sindy_x=(0.0, 1.0), sindy_reg_type=("l1", "none"), frozen=(False, True), group=(None, SHARDS),
                host_lbfgs=(False, True), torch_lbfgs=(False, True), numpy_lbfgs=(False, True), gram_closure=(False, True),
                torch_optim_env=(False, True), mask_numel=(256, 257), has_trainer=(False, True))
    for values in itertools.product(*axes.values()):
        kw = dict(zip(axes, values))
        want = _outcome(**kw)
        assert want != "latent"
        assert _outcome(fused_latent=False, **kw) == want, kw
        # the facts only the latent route reads change nothing either
        assert _outcome(fused_latent=False, w_sindy_z=0.0, has_latent=False, **kw) == want, kw
        if not kw["use_latent"]:
            assert _outcome(fused_latent=True, w_sindy_z=0.0, has_latent=False, **kw) == want, kw


def test_train_signature_and_flag():
    import inspect
    from symode_amd import parser_utils
    assert inspect.signature(T.train_SIGED_lbfgs).parameters["fused_latent"].default is False
    assert inspect.signature(_lbfgs_route).parameters["fused_latent"].default is False
    assert parser_utils.get_args(argv=[]).fused_latent is False
    assert parser_utils.get_args(argv=["--use_latent", "--fused_latent"]).fused_latent is True


# ------------------------------------------------------------------------ latent_operands
def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("D, d, n_comps", [(2, 2, 1), (2, 2, 2), (6, 2, 1), (6, 2, 2)])
def test_latent_operands_reproduce_the_reference_closure_in_fp64(D, d, n_comps):
    """loss2 from the operands (+ e0 / (n D)) against the terms train._autograd_closure(use_latent=True) logs, and the
    closure's Xi-gradient, for random Xi and a mask with zeros, to 1e-10 relative.  The reference's closure differentiates
    the z-term alone (compute_dx is a functional jvp without create_graph: loss_sindy_x reaches no parameter), so its
    gradient is compared with the w_pair = 0 form; the x-term's own gradient -- the QR reduction and the d / D factor under
    differentiation -- is compared with autograd through the same decoder JVP with the graph kept."""
    order, f64 = 2, torch.float64
    ae = seeded_autoencoder(D, d, n_comps, seed=5 + D + n_comps, dtype=f64)
    x, dx = random_points(37, n_comps, D, seed=D * 10 + n_comps, dtype=f64)
    reg = SINDyRegression(d, order, False, False, threshold=0.1, device="cpu", engine=OracleEngine()).double()
    torch.manual_seed(1)
    reg.Xi.data = 0.5 * torch.randn_like(reg.Xi)
    reg.mask = (torch.rand_like(reg.Xi) > 0.3).double()
    reg.mask[1] = 0.0
    reg.mask[0, 0] = 1.0
    w_z, w_x = 0.7, 0.3

    z, dz, B, y, e0, D_out = latent_operands(x, dx, ae, chunk=16)          # several chunks, a ragged last one
    n = x.shape[0] * n_comps
    assert D_out == D and z.shape == (n, d) and dz.shape == (n, d) and B.shape == (n, d, d) and y.shape == (n, d)
    assert z.dtype == f64 and (e0 == 0.0) == (D == d)
    whole = latent_operands(x, dx, ae)
    for a, b in zip((z, dz, B, y), whole[:4]):
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-14)

    losses = {}
    terms = T._LossTerms(w_z, w_x, "none", 0.0, "i", 0.0, 0.1, 0.01)
    closure = T._autograd_closure(reg, x, dx, ae, None, terms, losses, True, None)
    loss = closure(torch.optim.SGD(reg.parameters(), lr=0.0))
    ref_grad = reg.Xi.grad.clone()

    loss2, g_z = closure_from_operands(z, dz, B, y, reg.Xi, reg.mask, order, 0.0)
    loss_x = loss2[1] * d / D + e0 / (n * D)
    assert _rel(loss2[0], losses["loss_sindy_z"]) < 1e-10
    assert _rel(loss_x, losses["loss_sindy_x"]) < 1e-10
    assert _rel(w_z * loss2[0] + w_x * loss_x, loss.detach()) < 1e-10
    assert _rel(w_z * g_z, ref_grad) < 1e-10
    assert float(ref_grad[1].abs().max()) == 0.0 and float(g_z[1].abs().max()) == 0.0       # the all-zero mask row

    # the x-term under differentiation
    from torch.autograd.functional import jvp
    Xi = reg.Xi.detach().clone().requires_grad_(True)
    zz = ae.encode(x)
    from oracle import sindy_oracle as O
    h = (O.theta(zz.reshape(-1, d), order) @ (Xi * reg.mask).T).reshape(zz.shape)
    dx_pred = jvp(ae.decode, zz, v=h, create_graph=True)[1]
    (want,) = torch.autograd.grad(torch.nn.functional.mse_loss(dx_pred, dx), Xi)
    _, g_both = closure_from_operands(z, dz, B, y, reg.Xi, reg.mask, order, 1.0)
    assert _rel((g_both - g_z) * d / D, want) < 1e-10


def test_latent_operands_refuse_a_training_mode_autoencoder():
    ae = seeded_autoencoder(2, 2, 1, seed=0).train()
    x, dx = random_points(8, 1, 2, seed=0)
    with pytest.raises(ValueError, match="eval mode"):
        latent_operands(x, dx, ae)
