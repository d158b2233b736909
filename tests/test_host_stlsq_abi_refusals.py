"""The six symode_stlsq_* entries answer every case of tests/stlsq_abi_cases.py as the library did before their checks were
gathered into shared helpers: same code for every argument combination, a size before a pointer before an alignment."""
import json
import os

import pytest

from symode_amd import engine
from tests import stlsq_abi_cases as C


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return engine.load_library()


@pytest.fixture(scope="module")
def before():
    return json.load(open(C.GOLDEN))


def test_the_table_is_the_one_recorded_and_launches_nothing(before):
    assert sorted(before) == sorted(C.ENTRIES)
    for entry in C.ENTRIES:
        assert [case for case, _ in before[entry]] == C.cases(entry), entry          # the generator has not drifted
        assert all(C.refused_by_construction(entry, case) for case, _ in before[entry]), entry
        assert {code for _, code in before[entry]} == {C.NULLPTR, C.BADSIZE, C.ALIGN}, entry
        assert len(engine._SIGNATURES[entry][1]) == len(C.ENTRIES[entry]) + 1, entry   # every argument and the stream
    assert 2000 < sum(len(rows) for rows in before.values()) < 5000


@pytest.mark.parametrize("entry", list(C.ENTRIES))
def test_every_case_is_refused_as_before(lib, before, entry):
    wrong = [(case, code, C.call(lib, entry, case)) for case, code in before[entry] if C.refused_by_construction(entry, case)]
    wrong = [w for w in wrong if w[1] != w[2]]
    assert not wrong, wrong[:10]
