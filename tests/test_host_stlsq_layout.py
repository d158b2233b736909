"""``engine.packed_layout`` on a CPU buffer: the one statement of where the small outputs of the six STLSQ launches lie in the
buffer they share.  Torch and numpy forms, with and without a tail."""
import itertools

import numpy as np
import pytest
import torch

from symode_amd import engine

ENTRIES = ("symode_stlsq_sweep", "symode_stlsq_path", "symode_stlsq_sweep_constrained", "symode_stlsq_sweep_minnorm",
           "symode_stlsq_sweep_symreg", "symode_stlsq_path_symreg")
SIZES = ((1, 1, 1), (3, 1, 3), (6, 2, 3), (3, 2, 10))
ITEM = {"f8": 8, "f4": 4, "i4": 4, "u1": 1}
TORCH = {"f8": torch.float64, "f4": torch.float32, "i4": torch.int32, "u1": torch.uint8}
NUMPY = {"f8": np.float64, "f4": np.float32, "i4": np.int32, "u1": np.uint8}


def documented(entry, d, p, r1):
    """name -> (type, per-problem shape) as the wrappers' docstrings give them, in the order of the result"""
    n0 = d * p
    sweep = [("xi", "f4", (d, p)), ("mask", "u1", (d, p)), ("passes", "i4", ()), ("near", "i4", ()), ("fell", "i4", ())]
    if entry == "symode_stlsq_path":
        return [("Xi", "f4", (d, p)), ("mask", "u1", (d, p)), ("order", "i4", (d, p)), ("rss_train", "f8", (d, p + 1)),
                ("rss_val", "f8", (d, p + 1)), ("best", "i4", (d,)), ("near", "i4", ()), ("fell", "i4", ())]
    if entry == "symode_stlsq_path_symreg":
        return [("Xi", "f4", (d, p)), ("mask", "u1", (d, p)), ("order", "i4", (n0,)), ("mse_train", "f8", (n0 + 1,)),
                ("reg_train", "f8", (n0 + 1,)), ("mse_val", "f8", (n0 + 1,)), ("best", "i4", ()), ("near", "i4", ()), ("fell", "i4", ())]
    if entry == "symode_stlsq_sweep_constrained":
        return sweep + [("var", "f4", (r1,))]
    if entry == "symode_stlsq_sweep_minnorm":
        return sweep + [("var", "f4", (r1,)), ("trunc", "i4", ()), ("rank", "i4", ())]
    return sweep


def cases():
    for entry, (S, d, p), n_tail in itertools.product(ENTRIES, SIZES, (None, 3)):
        for r1 in ((1, 3) if "constrained" in entry or "minnorm" in entry else (0,)):
            yield entry, S, d, p, r1, n_tail


def _span(view, base):
    """[lo, hi) of a view in bytes from the buffer's start"""
    if isinstance(view, torch.Tensor):
        return view.data_ptr() - base, view.data_ptr() - base + view.numel() * view.element_size()
    return view.ctypes.data - base, view.ctypes.data - base + view.nbytes


@pytest.mark.parametrize("entry,S,d,p,r1,n_tail", list(cases()))
def test_the_layout_of_every_launch(entry, S, d, p, r1, n_tail):
    fields = engine.stlsq_fields(entry, d, p, r1)
    assert fields == documented(entry, d, p, r1)
    n_bytes, views = engine.packed_layout(fields, S, n_tail)
    want = [(name, kind, (S,) + shape) for name, kind, shape in fields] + ([("tail", "i4", (n_tail,))] if n_tail is not None else [])
    assert n_bytes >= sum(ITEM[kind] * int(np.prod(shape)) for _, kind, shape in want)
    for buf, types in ((torch.zeros(n_bytes, dtype=torch.uint8), TORCH), (np.zeros(n_bytes, dtype=np.uint8), NUMPY)):
        base = buf.data_ptr() if isinstance(buf, torch.Tensor) else buf.ctypes.data
        o = views(buf)
        assert list(o) == [name for name, _, _ in want]                               # the order of the result, the tail last
        spans = []
        for name, kind, shape in want:
            assert o[name].dtype == types[kind] and tuple(o[name].shape) == shape, name
            lo, hi = _span(o[name], base)
            assert hi - lo == ITEM[kind] * int(np.prod(shape)) and lo % ITEM[kind] == 0 and 0 <= lo and hi <= n_bytes, name
            spans.append((lo, hi))
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))                     # pairwise disjoint
        if n_tail is not None:
            lo, hi = _span(o["tail"], base)
            behind = max(_span(o[name], base)[1] for name, _, _ in want[:-1])
            assert lo % 4 == 0 and behind <= lo < behind + 4 and hi == n_bytes         # 4-aligned behind the last field
        # a distinct pattern through each view reads back through the views of a copy of the buffer
        for i, (name, kind, shape) in enumerate(want):
            pattern = (np.arange(int(np.prod(shape))) % 97 + 100 * i + 1).reshape(shape).astype(NUMPY[kind])
            if isinstance(buf, torch.Tensor):
                o[name].copy_(torch.from_numpy(pattern))
            else:
                o[name][...] = pattern
        copy = views(buf.clone() if isinstance(buf, torch.Tensor) else buf.copy())
        for i, (name, kind, shape) in enumerate(want):
            pattern = (np.arange(int(np.prod(shape))) % 97 + 100 * i + 1).reshape(shape).astype(NUMPY[kind])
            assert np.array_equal(np.asarray(copy[name]), pattern), name


def test_nine_mask_bytes_leave_three_of_padding_before_the_tail():
    S, d, p = 3, 1, 3
    n_bytes, views = engine.packed_layout(engine.stlsq_fields("symode_stlsq_sweep", d, p), S, 3)
    buf = np.zeros(n_bytes, dtype=np.uint8)
    o = views(buf)
    mask_end = _span(o["mask"], buf.ctypes.data)[1]
    assert mask_end == 4 * S * (d * p + 3) + 9 and _span(o["tail"], buf.ctypes.data) == (mask_end + 3, mask_end + 3 + 12) == (n_bytes - 12, n_bytes)
    assert engine.packed_layout(engine.stlsq_fields("symode_stlsq_sweep", d, p), S)[0] == mask_end + 3   # the buffer's size as before
