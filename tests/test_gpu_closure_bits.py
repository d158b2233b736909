"""The reversed-closure kernels (symreg_reversed_kernel: fused closure and regulariser alone) against their own recorded bits.

The other closure tests compare the kernel's forms with each other (packed against scalar, compact table against
materialised Jacobian) and with the oracle at 2e-5 ... 3e-5: a change of the order of a sum in every form alike passes all
of them.  tests/golden/closure_bits.npz pins the bits instead.  It is THIS project's own output on an MI355X, recorded at
commit f3b48a3 (the last one before the kernel's per-point arithmetic and group loop were stated once) -- not the
reference's, which sums in another order.  The inputs come from CPU torch.Generator seeds (make_case of
test_gpu_constj.py), so only the outputs are stored: loss and gradient of the fused closure and of the regulariser alone,
one set per input case.  The Jacobian layouts of a case (materialised, compact table with the scalar body, compact table
with the launcher's choice of body) are each held to that one set with np.array_equal; the recorder refuses a case on which
they disagree.  Polynomial libraries only: sine / exp columns would tie the file to one ROCm's inlined sinf / expf.

    python -m tests.test_gpu_closure_bits OUT.npz        records (on the GPU, with the library to be pinned)
"""
import sys

import numpy as np
import pytest
import torch

from tests.test_gpu_closure_packed import pk_env
from tests.test_gpu_constj import expand, make_case

pytestmark = pytest.mark.gpu

W_SYM = 0.37
# layout -> (SYMODE_CLOSURE_PK, Jacobian given as the compact table?)
LAYOUTS = {"materialised": (None, False), "table_scalar": ("0", True), "table": (None, True)}


def case_id(S, n, n_g, d, order, masked, one):
    return f"d{d}o{order}_S{S}{'one' if one else ''}_n{n}_g{n_g}_{'masked' if masked else 'unmasked'}"


# (S, n, n_g, d, order, masked, one problem in the unbatched form, forms, layouts)
BOTH, ALL3, MAT_TABLE = ("fused", "alone"), tuple(LAYOUTS), ("materialised", "table")
CASES = (
    # d = 2, order 3 (Xi in VGPRs) and 5 (Xi in SGPRs; the packed library).  N = 1031 and N = 5: n d is no multiple of 4, so
    # the slabs of problems 1, 2 leave the 16-byte grid and the launch takes the per-point path; 1032: ring turns and a partial turn
    [(3, n, n_g, 2, order, masked, False, BOTH, ALL3)
     for order in (3, 5) for n_g in (1, 2) for n in (1031, 1032, 5) for masked in (True, False)]
    # one aligned problem: the ring and the ragged tail in one launch; N = 5: a ring shorter than one turn (two chunks, one point)
    + [(1, 1031, 1, 2, 5, True, True, BOTH, ALL3)]
    + [(1, 5, 1, 2, order, True, True, BOTH, ALL3) for order in (3, 5)]
    # d = 3: S = 1, N = 1031, n_g = 1 is 257 chunks of four -- four whole-wave tile exchanges, one ragged lane, a three-point
    # tail (with n_g = 2 the second slab starts off the 16-byte grid: per point); S = 3: N = 1032 tiles and a partial wave, 1031 per point
    + [(S, n, n_g, 3, 3, True, S == 1, BOTH, MAT_TABLE) for (S, n) in ((1, 1031), (3, 1032), (3, 1031)) for n_g in (1, 2)]
    # d = 1: four points per chunk without the tile exchange (N = 1032; 1031 with three problems runs per point)
    + [(3, n, n_g, 1, 3, True, False, ("fused",), MAT_TABLE) for n in (1031, 1032) for n_g in (1, 2)])


def expected_body(layout, d, order):
    return "packed" if (layout == "table" and d == 2 and order == 5) else "scalar"


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


def run_case(eng, case, layout):
    """{"fused_loss", "fused_grad", "alone_loss", "alone_grad"} (the forms of the case) as numpy arrays, and the body of every launch"""
    S, n, n_g, d, order, masked, one, forms, _ = case
    x, dx, gx, table, xi, mask = make_case(S, n, n_g, d, order, eng, seed=5 if one else 0)
    if d == 2:
        if masked:
            mask[:, :, 2] = 0.0                              # besides the random zeros: a whole column gone in every problem
        else:
            mask = None
    pk, compact = LAYOUTS[layout]
    jgx = table if compact else expand(table, n)
    if one:
        x, dx, gx, jgx, xi, mask = x[0], dx[0], gx[0], jgx[0], xi[0], None if mask is None else mask[0]
        for t in (x, dx, gx):
            assert t.data_ptr() % 16 == 0 and t.is_contiguous()
    ws = eng.new_workspace(x.device, eng.lib.symode_workspace_bytes(d, order, 0, S, n))
    out, bodies = {}, []
    with pk_env(pk):
        if "fused" in forms:
            loss2, grad = eng.loss_grad_reversed(x, dx, gx, jgx, xi, mask, order, 0, w_sym=W_SYM, ws=ws)
            bodies.append(eng.closure_body(ws))
            out["fused_loss"], out["fused_grad"] = loss2.cpu().numpy(), grad.cpu().numpy()
        if "alone" in forms:
            loss, grad = eng.symreg_reversed(x, gx, jgx, xi, mask, order, 0, ws=ws)
            bodies.append(eng.closure_body(ws))
            out["alone_loss"], out["alone_grad"] = loss.cpu().numpy(), grad.cpu().numpy()
    return out, bodies


@pytest.mark.parametrize("case,layout", [(c, l) for c in CASES for l in c[-1]],
                         ids=[f"{case_id(*c[:7])}-{l}" for c in CASES for l in c[-1]])
def test_closure_returns_the_recorded_bits(eng, golden, case, layout):
    want = golden("closure_bits")
    got, bodies = run_case(eng, case, layout)
    assert bodies == [expected_body(layout, case[3], case[4])] * len(case[7])
    key = case_id(*case[:7])
    for name, arr in got.items():
        w = want[f"{key}/{name}"]
        assert np.isfinite(w).all() and np.abs(w).max() > 0
        assert arr.dtype == w.dtype and np.array_equal(arr, w), f"{key} {layout} {name}"


def test_the_fixture_holds_exactly_these_cases(golden):
    want = {f"{case_id(*c[:7])}/{form}_{what}" for c in CASES for form in c[7] for what in ("loss", "grad")}
    assert set(golden("closure_bits").files) == want


def record(path):
    import symode_amd
    eng_, arrays = symode_amd.get_engine(), {}
    for case in CASES:
        key, first = case_id(*case[:7]), None
        for layout in case[-1]:
            got, bodies = run_case(eng_, case, layout)
            assert bodies == [expected_body(layout, case[3], case[4])] * len(case[7]), (key, layout, bodies)
            if first is None:
                first = got
            for name, arr in got.items():
                assert np.array_equal(arr, first[name]), f"{key}: {layout} differs from {case[-1][0]} in {name}"
        arrays.update({f"{key}/{name}": arr for name, arr in first.items()})
    np.savez_compressed(path, **arrays)
    print(f"{len(arrays)} arrays of {len(CASES)} cases -> {path}")


if __name__ == "__main__":
    record(sys.argv[1])
