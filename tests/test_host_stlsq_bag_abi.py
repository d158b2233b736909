"""CPU-side checks of symode_gram_resample and symode_stlsq_bag: the entries are additions (declared, exported, bound with the
header's argument count, the ABI version unchanged, the siblings' signatures kept), and every refusal of the header is an error
code before any device work -- the pointers below are junk and none is dereferenced."""
import os
import re

import pytest

from symode_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "symmetry-ode-discovery_amd", "csrc")
NULL, JUNK = None, 0x1000                      # JUNK: non-null, 256-byte aligned
OK, UNSUPPORTED, NULLPTR, BADSIZE, WORKSPACE, ALIGN = 0, -1, -2, -3, -4, -5


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return engine.load_library()


def _resample(lib, chunk=JUNK, seeds=JUNK, n_seeds=3, n_chunks=8, n=12, n_replicas=5, out=JUNK, counts=JUNK):
    return lib.symode_gram_resample(chunk, seeds, n_seeds, n_chunks, n, n_replicas, out, counts, None)


def _bag(lib, aug=JUNK, n_seeds=3, n_problems=3, d=2, p=10, n_replicas=5, rep_xi=JUNK, rep_mask=JUNK, rep_fell=JUNK, tau_table=NULL,
         tau_milli=500, gamma=0.1, xi=JUNK, mask=JUNK, fell=JUNK, count=JUNK, valid=JUNK, mean=JUNK, std=JUNK):
    return lib.symode_stlsq_bag(aug, n_seeds, n_problems, d, p, n_replicas, rep_xi, rep_mask, rep_fell, tau_table, tau_milli, gamma,
                                xi, mask, fell, count, valid, mean, std, None)


def test_the_entries_are_additions(lib):
    assert lib.symode_abi_version() == engine.ABI_VERSION == 8         # an added entry leaves the version (include/symode.h)
    header = open(os.path.join(ROOT, "include", "symode.h")).read()
    names = {"symode_gram_resample": ["chunk", "seeds", "n_seeds", "n_chunks", "n", "n_replicas", "out", "counts_out", "stream"],
             "symode_stlsq_bag": ["aug_gram", "n_seeds", "n_problems", "d", "p", "n_replicas", "rep_xi", "rep_mask", "rep_fell",
                                  "tau_table", "tau_milli", "gamma", "xi_out", "mask_out", "fell_out", "count_out", "valid_out",
                                  "mean_out", "std_out", "stream"]}
    for name, want in names.items():
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl and hasattr(lib, name)
        args = [a.strip() for a in decl.group(1).split(",")]
        assert len(args) == len(engine._SIGNATURES[name][1]) == len(want)
        assert [a.split()[-1].lstrip("*") for a in args] == want
        comment = header[:decl.start()].rsplit("/*", 1)[1]
        assert "Added to ABI version 8 (nothing existing changed)" in comment and "replaces: nothing in the reference" in comment
    for name, count in (("symode_stlsq_sweep", 17), ("symode_stlsq_sweep_constrained", 23), ("symode_stlsq_sweep_minnorm", 25),
                        ("symode_stlsq_sweep_symreg", 20), ("symode_stlsq_path", 22), ("symode_stlsq_path_symreg", 27),
                        ("symode_aug_gram_gather", 13)):
        sibling = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert len(sibling.group(1).split(",")) == len(engine._SIGNATURES[name][1]) == count, name


def test_the_kernels_share_what_is_stated_once():
    """Only the C ABI's translation unit sees the two kernels; the draw uses the sweeps' two counter hashes and the refit the
    sweep's row solve, neither restated."""
    read = lambda f: open(os.path.join(CSRC, f)).read()                                        # noqa: E731
    sources = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".cpp"))]
    for header in ("gram_resample.hpp", "stlsq_bag.hpp"):
        assert [f for f in sources if '#include "%s"' % header in read(f)] == ["capi.hip"]
    draw, bag = read("gram_resample.hpp"), read("stlsq_bag.hpp")
    assert '#include "adam_order.hpp"' in draw and "0x9E3779B" not in draw and "seed_words(seed_words(seed)" in draw
    assert '#include "stlsq.hpp"' in bag and bag.count("stlsq_row_solve(G, F, p, j, gamma * gamma, n, lane, A, xrow, sel)") == 1
    assert "__shfl" not in bag and "stlsq_lds_bytes(d, p)" in bag and "hipFuncAttributeMaxDynamicSharedMemorySize" in bag


def test_every_refusal_of_the_resample_entry(lib):
    for n_chunks in (0, -1, 1025, 2 ** 20):
        assert _resample(lib, n_chunks=n_chunks) == BADSIZE, n_chunks
    for n in (0, -1, 69, 1000):
        assert _resample(lib, n=n) == BADSIZE, n
    for n_replicas in (0, -4):
        assert _resample(lib, n_replicas=n_replicas) == BADSIZE, n_replicas
    for n_seeds in (0, -1, 2 ** 31):
        assert _resample(lib, n_seeds=n_seeds) == BADSIZE, n_seeds
    # a replica count the sweep entry would refuse as a problem count: n_seeds * n_replicas >= 2^31
    assert _resample(lib, n_seeds=2 ** 16, n_replicas=2 ** 15) == BADSIZE
    assert _resample(lib, n_seeds=2 ** 30, n_replicas=2 ** 30) == BADSIZE
    assert _resample(lib, n_seeds=2 ** 16, n_replicas=2 ** 15 - 1, chunk=NULL) == NULLPTR
    for n_chunks, n in ((1, 1), (1024, 68), (1, 68), (1024, 1)):                       # the corners pass the size rules
        assert _resample(lib, n_chunks=n_chunks, n=n, chunk=NULL) == NULLPTR, (n_chunks, n)
    for name in ("chunk", "seeds", "out"):
        assert _resample(lib, **{name: NULL}) == NULLPTR, name
        assert _resample(lib, **{name: 0x1004}) == ALIGN, name                         # 8 bytes
    assert _resample(lib, counts=0x1002) == ALIGN
    assert _resample(lib, counts=NULL, chunk=0x1004) == ALIGN                          # counts_out is optional: decided further on
    # a size before a pointer, a pointer before an alignment
    assert _resample(lib, n=69, chunk=NULL) == BADSIZE and _resample(lib, chunk=0x1004, out=NULL) == NULLPTR


def test_every_refusal_of_the_bag_entry(lib):
    for d in (0, -2, 5):
        assert _bag(lib, d=d) == BADSIZE, d
    for p in (0, -1, 65, 1000):
        assert _bag(lib, p=p) == BADSIZE, p
    for d, p in ((1, 1), (4, 64), (1, 64), (4, 1)):                                    # the corners pass the size rules
        assert _bag(lib, d=d, p=p, aug=NULL) == NULLPTR, (d, p)
    for n_seeds in (0, -3):
        assert _bag(lib, n_seeds=n_seeds) == BADSIZE, n_seeds
    for n_problems in (2, 0, 2 ** 31, 4, 7):                                           # fewer than the seeds, too many, no multiple
        assert _bag(lib, n_problems=n_problems, tau_table=JUNK) == BADSIZE, n_problems
    for n_problems in (3, 6, 27):
        assert _bag(lib, n_problems=n_problems, tau_table=JUNK, aug=NULL) == NULLPTR, n_problems
        assert _bag(lib, n_problems=n_problems, aug=NULL) == NULLPTR, n_problems        # one level for all: also a grid of one
    for n_replicas in (0, -1):
        assert _bag(lib, n_replicas=n_replicas) == BADSIZE, n_replicas
    assert _bag(lib, n_seeds=2 ** 16, n_problems=2 ** 16, n_replicas=2 ** 15) == BADSIZE
    for tau in (-1, 1001, 2 ** 20):
        assert _bag(lib, tau_milli=tau) == BADSIZE, tau
        assert _bag(lib, tau_milli=tau, tau_table=JUNK, aug=NULL) == NULLPTR, tau       # behind a table the scalar is not read
    for tau in (0, 1, 999, 1000):
        assert _bag(lib, tau_milli=tau, aug=NULL) == NULLPTR, tau
    for bad in (-1e-14, -1.0, float("nan"), float("inf"), float("-inf")):
        assert _bag(lib, gamma=bad) == BADSIZE, bad
    assert _bag(lib, gamma=0.0, aug=NULL) == NULLPTR                                   # zero is a value
    pointers = ("aug", "rep_xi", "rep_mask", "rep_fell", "xi", "mask", "fell", "count", "valid", "mean", "std")
    for name in pointers:
        assert _bag(lib, **{name: NULL}) == NULLPTR, name
    for name in ("aug", "mean", "std"):                                                # fp64: 8 bytes
        assert _bag(lib, **{name: 0x1004}) == ALIGN, name
    for name in ("rep_xi", "rep_fell", "xi", "fell", "count", "valid"):                # fp32 / int: 4 bytes
        assert _bag(lib, **{name: 0x1002}) == ALIGN, name
        assert _bag(lib, aug=NULL, **{name: 0x1004}) == NULLPTR, name
    assert _bag(lib, tau_table=0x1002) == ALIGN
    assert _bag(lib, aug=NULL, rep_mask=0x1001, mask=0x1003) == NULLPTR                # bytes: any address
    # a size before a pointer, a pointer before an alignment, as the other entries decide
    assert _bag(lib, p=65, aug=NULL) == BADSIZE and _bag(lib, tau_milli=-1, xi=NULL) == BADSIZE
    assert _bag(lib, aug=0x1004, std=NULL) == NULLPTR


def test_the_host_checks_a_table_before_upload():
    """engine.stlsq_bag looks at a list of levels before anything is uploaded; the sweep's parser is stricter still"""
    from symode_amd.sweep import inclusion_milli
    assert inclusion_milli(1.0) == [1000] and inclusion_milli([0, 0.5, 0.6, 0.999, 1]) == [0, 500, 600, 999, 1000]
    for bad in (-0.001, 1.001, 0.5005, float("nan"), float("inf"), [0.5, 2], []):
        with pytest.raises(ValueError, match="inclusion"):
            inclusion_milli(bad)
