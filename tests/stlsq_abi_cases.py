"""The case table behind tests/golden/stlsq_abi_refusals_before_refactor.json: for each of the six symode_stlsq_* entries the
valid baseline call of its test_host_stlsq_*_abi.py (junk non-null addresses, a None stream) with one and two arguments moved
off it, and one argument moved off the grid of six problems behind a table.  Every case breaks at least one rule of the entry, so none reaches a launch: ``refused_by_construction`` says why, from
the case alone.  ``python -m tests.stlsq_abi_cases`` records the loaded library's answers into the fixture."""
import json
import os

NULL, JUNK = None, 0x1000                      # JUNK: non-null, 256-byte aligned
OK, UNSUPPORTED, NULLPTR, BADSIZE, WORKSPACE, ALIGN = 0, -1, -2, -3, -4, -5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stlsq_abi_refusals_before_refactor.json")

P, B, T, I, F = "pointer", "bytes", "table", "int", "scalar"        # T: the optional hyper table; B: the mask (any address)
_SIZES = [("n_sets", I, 3), ("n_problems", I, 3), ("d", I, 2), ("p", I, 10), ("n_points", I, 200)]
_PATH_SIZES = [("n_sets", I, 3), ("n_val_sets", I, 1), ("n_problems", I, 3), ("d", I, 2), ("p", I, 10), ("n_points", I, 200)]
_Q = [("q_solve", P, JUNK), ("q_xi", P, JUNK), ("r", I, 4), ("allow_constant", I, 1)]
_SWEEP_OUT = [("xi", P, JUNK), ("mask", B, JUNK), ("passes", P, JUNK), ("near", P, JUNK), ("fell", P, JUNK)]
_CON_OUT = [("xi", P, JUNK), ("var", P, JUNK), ("mask", B, JUNK), ("passes", P, JUNK), ("near", P, JUNK), ("fell", P, JUNK)]
_FIT = [("hyper", T, NULL), ("gamma", F, 0.1), ("threshold", F, 0.05)]

# the arguments of every entry in the header's order (the stream, always None, left out) with their baseline values
ENTRIES = {
    "symode_stlsq_sweep": [("aug", P, JUNK)] + _SIZES + _FIT + [("max_iter", I, 10), ("near_band", F, 1e-4)] + _SWEEP_OUT,
    "symode_stlsq_path": [("aug", P, JUNK), ("val", P, JUNK)] + _PATH_SIZES + [
        ("gamma", F, 0.1), ("tol", F, 0.02), ("floor_rel", F, 1e-10), ("near_band", F, 1e-4), ("path", P, JUNK), ("order", P, JUNK),
        ("rss_train", P, JUNK), ("rss_val", P, JUNK), ("best", P, JUNK), ("xi", P, JUNK), ("mask", B, JUNK), ("near", P, JUNK),
        ("fell", P, JUNK)],
    "symode_stlsq_sweep_constrained": [("aug", P, JUNK)] + _SIZES + _Q + _FIT + [
        ("max_iter", I, 10), ("near_band", F, 1e-4), ("pivot_floor", F, 1e-14)] + _CON_OUT,
    "symode_stlsq_sweep_minnorm": [("aug", P, JUNK)] + _SIZES + _Q + _FIT + [
        ("max_iter", I, 10), ("near_band", F, 1e-4), ("rcond", F, 1e-7)] + _CON_OUT + [("trunc", P, JUNK), ("rank", P, JUNK)],
    "symode_stlsq_sweep_symreg": [("aug", P, JUNK), ("rev", P, JUNK)] + _SIZES + _FIT + [
        ("w_sym", F, 1.0), ("max_iter", I, 10), ("near_band", F, 1e-4), ("pivot_floor", F, 1e-14)] + _SWEEP_OUT,
    "symode_stlsq_path_symreg": [("aug", P, JUNK), ("rev", P, JUNK), ("val", P, JUNK)] + _PATH_SIZES + [
        ("hyper", T, NULL), ("gamma", F, 0.1), ("w_sym", F, 1.0), ("tol", F, 0.02), ("floor_rel", F, 1e-10), ("near_band", F, 1e-4),
        ("pivot_floor", F, 1e-14), ("path", P, JUNK), ("order", P, JUNK), ("mse_train", P, JUNK), ("reg_train", P, JUNK),
        ("mse_val", P, JUNK), ("best", P, JUNK), ("xi", P, JUNK), ("mask", B, JUNK), ("near", P, JUNK), ("fell", P, JUNK)],
}

# boundary values of the sizes; the first tuple of each holds the values no entry that has the argument accepts
_INT_VALUES = {
    "d": ((0, -2, 5), (1, 4)),
    "p": ((0, -1, 65), (1, 32, 33, 64)),
    "r": ((0, -3), (1, 16, 17, 19, 21, 62, 63, 65)),
    "allow_constant": ((), (0, 1, 2)),
    "max_iter": ((0, -1), (1,)),
    "n_sets": ((0, -3), (1, 4)),
    "n_problems": ((0, 2, 2 ** 31), (4, 6, 27, 2 ** 31 - 1)),
    "n_val_sets": ((0, -1), (2, 3, 4, 28)),
    "n_points": ((), (0,)),
}
_SCALAR_VALUES = ("nan", "inf", -1.0, 0.0, 1.0, 1e39)                   # 1e39: finite, not in fp32


def _variations(args):
    out = []
    for name, kind, base in args:
        if kind in (P, B):
            out += [(name, NULL), (name, JUNK + 2)]
        elif kind == T:
            out += [(name, JUNK), (name, JUNK + 2)]
        elif kind == I:
            out += [(name, v) for group in _INT_VALUES[name] for v in group]
        else:
            out += [(name, v) for v in _SCALAR_VALUES]
    return out


def _probes(args):
    """The second argument of a pair: one variation of every kind of rule, against which every variation is recorded -- a size,
    the table with a grid behind it, a null and a misaligned pointer at either end of the list, a scalar."""
    pointers = [name for name, kind, _ in args if kind == P]
    scalar = next(name for name, kind, _ in args if kind == F)
    table = [("hyper", JUNK)] if any(kind == T for _, kind, _ in args) else []
    return [("d", 0), ("n_problems", 6)] + table + [(pointers[0], NULL), (pointers[-1], NULL), (pointers[0], JUNK + 2),
                                                    (pointers[-1], JUNK + 2), (scalar, "nan")]


def refused_by_construction(entry, case):
    """True where the case names a rule it breaks without a model of the entry: a null pointer (the table aside), an address
    off by two where the entry checks alignment (the mask aside), or a size no entry takes."""
    kinds = {name: kind for name, kind, _ in ENTRIES[entry]}
    for name, value in case.items():
        if kinds[name] in (P, B) and value is NULL:
            return True
        if kinds[name] in (P, T) and value is not NULL and value % 4:
            return True
        if kinds[name] == I and value in _INT_VALUES[name][0]:
            return True
    return False


def cases(entry):
    """The overrides of the baseline, one dict per case, in a fixed order."""
    args = ENTRIES[entry]
    variations, out, seen = _variations(args), [], set()
    # a grid behind a table is valid as a pair: every variation once more on top of it
    grid = [[("hyper", JUNK), ("n_problems", 6)]] if any(kind == T for _, kind, _ in args) else []
    for first in variations:
        for second in [[]] + [[probe] for probe in _probes(args)] + grid:
            if first[0] in dict(second):
                continue
            case = dict([first] + second)
            key = tuple(sorted((k, repr(v)) for k, v in case.items()))
            if key not in seen and refused_by_construction(entry, case):
                seen.add(key)
                out.append(case)
    return out


def call(lib, entry, case):
    values = [case.get(name, base) for name, _, base in ENTRIES[entry]]
    return getattr(lib, entry)(*[float(v) if isinstance(v, str) else v for v in values], None)


def record(lib):
    return {entry: [[case, call(lib, entry, case)] for case in cases(entry)] for entry in ENTRIES}


if __name__ == "__main__":
    from symode_amd import engine
    table = record(engine.load_library())
    assert all(code in (NULLPTR, BADSIZE, ALIGN) for rows in table.values() for _, code in rows)
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(entry) + ": [\n" + ",\n".join(json.dumps(row) for row in rows) + "\n]"
                                   for entry, rows in table.items()) + "\n}\n")
    print({entry: len(rows) for entry, rows in table.items()})
