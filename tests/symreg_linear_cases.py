"""The cases of the S1 (linear-latent symmetry regulariser) tests, with their tolerances.

``tests/test_gpu_symreg_linear.py`` plays them through ``engine.symreg_linear`` on the device,
``tests/test_host_symreg_linear_model.py`` replays them on the CPU with the float32 model standing where the device stands.
Either is compared with the fp64 model (tests/symreg_linear_model.py) on the same float32 inputs, the deviation taken as a
fraction of the model's yardsticks (``symreg_linear_model.deviation``).

Everything is seeded; the deck of a library does not depend on which other libraries are compiled.
"""
import functools
import math
from collections import namedtuple

import torch

from tests import symreg_linear_model as M
from tests.helpers import only_compiled

# ---------------------------------------------------------------------------------------------------------------------
# Tolerances, per state dimension (the d = 4 libraries are an optional part of the build).  Derived, not chosen:
# tests/test_host_symreg_linear_model.py replays every case below with the model in float32, every sum taken one term after
# the other, against the model in fp64 from the same float32 inputs, takes per field the worst deviation as a fraction of
# the yardstick, and asserts that each constant here is 4 x that figure (rounded up to two digits; x 4 for the reason
# tests/adam_cases.py states: the device adds per-thread partial sums, a wave butterfly and wave partials where the replay
# adds sequentially).  The replay figures and the worst the MI355X run showed are in profiles/symreg_linear_cases.txt.
# ---------------------------------------------------------------------------------------------------------------------
TOL = {1: {"loss": 8.3e-7, "grad": 3.1e-7}, 2: {"loss": 5.8e-7, "grad": 7.1e-7}, 3: {"loss": 1.1e-6, "grad": 1.1e-6}, 4: {"loss": 3.7e-7, "grad": 3.7e-7}}

ORDERS = {1: (1, 2, 3, 4, 5), 2: (1, 2, 3, 4, 5), 3: (1, 2, 3, 4), 4: (1, 2, 3)}
STEADY_N = {1: 6455, 2: 3227, 3: 6455, 4: 1613}          # 256 * 6 + 77 chunks (+ a ragged point where a chunk has several)
STEADY_GRIDS = (1, 3)                                    # SYMODE_REDUCE_GRID: one full ring turn and a ragged drain per lane

Case = namedtuple("Case", "name lib z xi mask L shift env exact_zero")      # shift: floats the base pointer is moved by


def all_libs():
    """Every (d, order) at flags 0; flags 1, 2, 3 at the lowest and highest order of each d."""
    out = []
    for d, orders in ORDERS.items():
        out += [(d, o, 0) for o in orders]
        out += [(d, o, f) for o in (orders[0], orders[-1]) for f in (1, 2, 3)]
    return out


def libs():
    return only_compiled(all_libs())


def sizes(d):
    ppt = M.PPT[d]
    base = (1031 // ppt) * ppt
    s = {1, ppt} | {base + r for r in range(ppt)}
    if ppt > 1:
        s.add(ppt - 1)
    if d == 3:
        s |= {65, 257}                                   # the last wave is partial
    return sorted(s)


def rotation(d):
    """The generator of the rotation in the (0, 1) plane (entries 0, +-1: products with it are exact); d = 1: [[1]]."""
    L = torch.zeros(1, d, d)
    if d == 1:
        L[0, 0, 0] = 1.0
    else:
        L[0, 0, 1], L[0, 1, 0] = 1.0, -1.0
    return L


def _dense(n_gen, d, gen):
    """Dense random generators, |entries| in 0.5 .. 1 with random signs: neither symmetric nor antisymmetric."""
    mag = 0.5 + 0.5 * torch.rand(n_gen, d, d, generator=gen)
    sign = torch.where(torch.rand(n_gen, d, d, generator=gen) < 0.5, -1.0, 1.0)
    return (mag * sign).contiguous()


def _mask(kind, d, p, gen):
    if kind == "none":
        return None
    mk = torch.ones(d, p)
    if kind == "random":
        mk = (torch.rand(d, p, generator=gen) >= 0.3).float()
        mk[0, 1] = 1.0                                   # never all zero
    elif kind == "row_off":
        mk[int(torch.randint(0, d, (1,), generator=gen))] = 0.0
    elif kind == "zero":
        mk.zero_()
    return mk


def _z(n, d, gen):
    """Points ~ 0.5 N(0, 1) clamped to +-1.2.  The ragged tail and the last full chunk lie at 0.9 <= |z_i| <= 1.2: a point
    among thousands that happens to lie near the origin adds less to the sums than float32 rounding, and a launch that
    dropped or repeated it could not be told from a correct one (the decidability gate of the host witness)."""
    z = (0.5 * torch.randn(n, d, generator=gen)).clamp(-1.2, 1.2)
    ppt = M.PPT[d]
    k = min(n, n % ppt + ppt)
    far = 0.9 + 0.3 * torch.rand(k, d, generator=gen)
    z[n - k:] = far * torch.where(torch.rand(k, d, generator=gen) < 0.5, -1.0, 1.0)
    return z.contiguous()


def _deck(values, n, gen):
    reps = (list(range(len(values))) * (n // len(values) + 1))[:n]
    order = torch.randperm(n, generator=gen).tolist()
    return [values[reps[i]] for i in order]


def equivariant_xi(d, p, gen):
    """h = a z (d = 2: a z + b J z): equivariant under ``rotation(d)``, so u = 0 and the fp64 loss and gradient are exactly 0."""
    a, b = (float(v) for v in 0.3 + torch.rand(2, generator=gen))
    xi = torch.zeros(d, p)
    for i in range(d):
        xi[i, 1 + i] = a
    if d == 2:
        xi[0, 2], xi[1, 1] = b, -b
    return xi


@functools.lru_cache(maxsize=None)
def lib_cases(lib):
    d, order, flags = lib
    p = M.terms(d, order, flags)
    gen = torch.Generator().manual_seed(31000 + 1000 * d + 10 * order + flags)
    near = 1031                                          # ragged for every chunk width above 1
    tag = f"d{d}o{order}f{flags}"
    out = []

    def add(name, n, n_gen, mask, shift=0, env=None, L=None, xi=None, exact_zero=False):
        L = _dense(n_gen, d, gen) if L is None else L
        xi = 0.4 * torch.randn(d, p, generator=gen) if xi is None else xi
        out.append(Case(f"{tag}-{name}-n{n}-g{L.shape[0]}-{mask}-s{shift}", lib, _z(n, d, gen), xi, _mask(mask, d, p, gen), L, shift,
                        env or {}, exact_zero))

    ns = sizes(d)
    gens, masks, shifts = _deck([0, 1, 2, 3], len(ns), gen), _deck(["none", "random", "row_off"], len(ns), gen), \
        _deck([0, 0, 0, 1, 2, 3], len(ns), gen)
    for k, n in enumerate(ns):
        add("size", n, gens[k], masks[k], shifts[k])
    for n_gen, mask in zip((0, 1, 2, 3), ("random", "row_off", "none", "random")):
        add("gen", near, n_gen, mask)
    for shift in (1, 2, 3):                              # a flat buffer moved by 1, 2, 3 floats: misaligns every d
        add("shift", near - 1, 2, "none", shift)
    add("maskzero", near, 2, "zero", exact_zero=True)
    add("rotation", near, 1, "random", L=rotation(d))
    add("equivariant", near, 1, "none", L=rotation(d), xi=equivariant_xi(d, p, gen))
    for k, grid in enumerate(STEADY_GRIDS):
        add(f"steady{grid}", STEADY_N[d], 2 + k, ("random", "none")[k], env={"SYMODE_REDUCE_GRID": grid})
    return tuple(out)


def deck(which=None):
    return [c for lib in (libs() if which is None else which) for c in lib_cases(tuple(lib))]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The fp64 model of a case, computed once and shared."""
    c = BY_NAME[name]
    return M.evaluate(c.z, c.xi, c.mask, c.L, c.lib[1], c.lib[2])


class _ByName(dict):
    def __missing__(self, name):
        for lib in all_libs():
            for c in lib_cases(tuple(lib)):
                dict.__setitem__(self, c.name, c)
        return dict.__getitem__(self, name)


BY_NAME = _ByName()


def round_up_2(x):
    """x rounded up to two significant digits."""
    if x <= 0.0:
        return 0.0
    e = math.floor(math.log10(x)) - 1
    return float(f"{math.ceil(x / 10 ** e - 1e-9) * 10 ** e:.1e}")
