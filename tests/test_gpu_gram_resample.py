"""symode_gram_resample (engine.gram_resample) against the numpy model tests/gram_resample_model.py on the deck of
tests/gram_resample_cases.py: ``out`` and ``counts_out`` byte for byte.  Both sides add count[c] * chunk[k, c, e] for c
ascending from 0.0 in fp64, one multiply and one add per term and nothing contracted, so there is no rounding to bound: the
bytes are equal or the kernel is wrong.  Every case is launched once and modelled once; the tests share both."""
import functools

import numpy as np
import pytest
import torch

from tests import gram_resample_cases as C
from tests import gram_resample_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def eng():
    import symode_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return symode_amd.get_engine()


def _launch(chunk, seeds, B):
    import symode_amd
    out, counts = symode_amd.get_engine().gram_resample(torch.from_numpy(chunk).to(DEV), seeds, B, want_counts=True)
    return out.cpu().numpy(), counts.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _device(case):
    return _launch(C.chunks(case), C.seeds_of(case), case[2])


@functools.lru_cache(maxsize=None)
def _model(case):
    return M.resample(C.chunks(case), C.seeds_of(case), case[2])


def test_the_deck_covers_every_value():
    for axis, values in enumerate(((1, 3, 12, 23, 68), (1, 2, 7, 128, 1024), (1, 3, 33), (1, 3))):
        assert sorted({c[axis] for c in C.DECK}) == list(values)
    spread = [np.log10(np.abs(C.chunks(c)).max() / np.abs(C.chunks(c))[np.abs(C.chunks(c)) > 0].min()) for c in C.DECK[::2]]
    assert max(spread) >= 12.0                                                  # entries spread over 12 decades


@pytest.mark.parametrize("case", C.DECK, ids=C.IDS)
def test_the_launch_is_the_model_byte_for_byte(eng, case):
    n, Cn, B, S = case
    out, counts = _device(case)
    want, want_counts = _model(case)
    assert out.shape == (S * B, n, n) and counts.shape == (S * B, Cn) and counts.dtype == np.int32
    assert counts.tobytes() == want_counts.tobytes()
    assert (counts.sum(axis=1) == Cn).all() and counts.min() >= 0
    assert out.tobytes() == want.tobytes(), np.abs(out - want).max()
    assert np.array_equal(out, out.transpose(0, 2, 1))                          # entries equal their mirrored entries exactly
    if Cn == 1:                                                                 # one chunk: the replica IS the chunk
        chunk = C.chunks(case)
        for k in range(S):
            for b in range(B):
                assert out[k * B + b].tobytes() == chunk[k, 0].tobytes()
    if Cn >= 7 and B > 1:
        assert len({counts[b].tobytes() for b in range(B)}) > 1                 # the replicas of a seed differ


@pytest.mark.parametrize("case", [C.DECK[4], C.DECK[11]], ids=[C.IDS[4], C.IDS[11]])
def test_a_second_launch_gives_equal_bytes(eng, case):
    again = _launch(C.chunks(case), C.seeds_of(case), case[2])
    assert again[0].tobytes() == _device(case)[0].tobytes() and again[1].tobytes() == _device(case)[1].tobytes()


def test_a_replica_does_not_depend_on_its_launch(eng):
    """replica b of a seed: launched with other seeds and B = 33, alone with B = 33, alone with B = 3, and without counts_out"""
    case = C.DECK[4]
    n, Cn, B, S = case
    assert (S, B) == (3, 33)
    chunk, seeds = C.chunks(case), C.seeds_of(case)
    big = _device(case)
    for k in range(S):
        alone = _launch(chunk[k:k + 1], seeds[k:k + 1], B)
        fewer = _launch(chunk[k:k + 1], seeds[k:k + 1], 3)
        for got, rows in ((alone, B), (fewer, 3)):
            assert got[0].tobytes() == big[0][k * B:k * B + rows].tobytes()
            assert got[1].tobytes() == big[1][k * B:k * B + rows].tobytes()
    only = eng.gram_resample(torch.from_numpy(chunk).to(DEV), torch.tensor(seeds, dtype=torch.int64, device=DEV), B)
    assert only.cpu().numpy().tobytes() == big[0].tobytes()


def test_the_twin_of_the_draw_is_the_launch(eng):
    from symode_amd.sweep import resample_counts, resample_grams
    for case in (C.DECK[1], C.DECK[4], C.DECK[6]):
        n, Cn, B, S = case
        counts = _device(case)[1]
        for k, seed in enumerate(C.seeds_of(case)):
            for b in (0, B - 1):
                assert np.array_equal(resample_counts(seed, b, Cn), counts[k * B + b]), (case, k, b)
    case = C.DECK[4]
    out, counts = resample_grams(C.chunks(case), C.seeds_of(case), case[2])
    assert out.tobytes() == _device(case)[0].tobytes() and counts.tobytes() == _device(case)[1].tobytes()


def test_the_wrapper_refuses_what_is_not_a_chunk_table(eng):
    from symode_amd.engine import SymodeError
    chunk = torch.zeros(2, 3, 4, 4, dtype=torch.float64, device=DEV)
    with pytest.raises(SymodeError, match="n_seeds, n_chunks, n, n"):
        eng.gram_resample(chunk[:, :, :, :3], [1, 2], 2)
    with pytest.raises(SymodeError, match="seeds must be"):
        eng.gram_resample(chunk, [1, 2, 3], 2)
    with pytest.raises(SymodeError, match="float64"):
        eng.gram_resample(chunk.float(), [1, 2], 2)
    with pytest.raises(SymodeError, match="symode_gram_resample failed"):
        eng.gram_resample(chunk, [1, 2], 0)
