"""CPU-side checks of symode_adam_run, the descriptor entry of the device Adam trainer that carries the per-problem
hyper-parameter table: the entry is additive (the ABI version stays the binding's), ``symode_adam_job`` is laid out as the
ctypes mirror ``engine.AdamJob`` says (sizeof and every offset from a C program compiled against include/symode.h), every
refusal of the header is an error code before any device work, pointers of another kind are not looked at, and
``DeviceAdam.fit(hyper=...)`` refuses what it cannot place in the table."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from symode_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, JUNK, ODD = None, 0x1000, 0x1002         # JUNK: non-null, aligned, never dereferenced -- validation fails first
PLAIN, REVERSED, LATENT = engine.ADAM_PLAIN, engine.ADAM_REVERSED, engine.ADAM_LATENT
_STATE = ("params", "m", "v", "step", "mask", "xi_out", "log")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return engine.load_library()


def _job(kind=PLAIN, keyed=True, **over):
    """A complete descriptor of ``kind`` (3 epochs of 300 rows in batches of 77, two problems of the (2, 2, 0) library) with
    a hyper table; ``over`` replaces fields."""
    a = dict(kind=kind, x=JUNK, dx=JUNK, n_src=300, n_epochs=3, batch=77, n_problems=2, d=2, order=2, flags=0, q_eff=NULL, r=0,
             allow_constant=1, n_params=12, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, w_x=1.0, w_obs=0.5, w_reg=1e-3, w_sym=0.25,
             l1=1, threshold=0.1, st_freq=2, epoch0=0, near_band=1e-4, hyper=JUNK, **{k: JUNK for k in _STATE})
    a.update(dict(order_seeds=JUNK, n_order_seeds=1, shuffle=1) if keyed else dict(idx=JUNK, n_idx_problems=1, n_steps=4))
    if kind == REVERSED:
        a.update(gx=JUNK, jgx=JUNK, n_g=2)
    if kind == LATENT:
        a.update(lat_B=JUNK, lat_y=JUNK, lat_e=JUNK, lat_L=JUNK, D_obs=4, n_gen=1)
    a.update(over)
    return engine.AdamJob(**a)


def _run(lib, base=PLAIN, keyed=True, **over):
    job = _job(base, keyed, **{k: v for k, v in over.items() if k != "kind"})
    job.kind = over.get("kind", base)                                # a kind outside the three: the fields of ``base`` stay
    return lib.symode_adam_run(ctypes.byref(job), None)


def test_the_entry_is_additive(lib):
    assert lib.symode_abi_version() == engine.ABI_VERSION            # (the number itself: tests/test_abi.py)
    assert hasattr(lib, "symode_adam_run") and engine._SIGNATURES["symode_adam_run"] == (ctypes.c_int, [ctypes.c_void_p] * 2)
    header = open(os.path.join(ROOT, "include", "symode.h")).read()
    assert re.search(r"\bint symode_adam_run\(const symode_adam_job\* J, void\* stream\);", header)
    for name, value in (("PLAIN", 0), ("REVERSED", 1), ("LATENT", 2), ("HYPER", 4)):
        assert re.search(r"#define SYMODE_ADAM_%s %d\b" % (name, value), header), name
        assert getattr(engine, "ADAM_" + name) == value
    # the six entries it gathers are not widened: the argument counts of the header are the binding's
    for name in ("symode_adam_epochs", "symode_adam_epochs_reversed", "symode_adam_epochs_latent"):
        for entry in (name, name + "_keyed"):
            decl = re.search(r"\bint %s\(([^;]*)\);" % entry, header)
            assert decl and "hyper" not in decl.group(1), entry
            assert len(decl.group(1).split(",")) == len(engine._SIGNATURES[entry][1]), entry


def test_the_struct_is_laid_out_as_the_ctypes_mirror_says():
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    names = [n for n, _ in engine.AdamJob._fields_]
    src = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"symode_adam_job_layout_{os.getpid()}.c")
    exe = src[:-2]
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "symode.h"\n'
                'int main(void) { printf("%zu' + ' %zu' * len(names) + '\\n", sizeof(symode_adam_job), '
                + ', '.join(f'offsetof(symode_adam_job, {n})' for n in names) + '); return 0; }\n')
    try:
        r = subprocess.run([cc, "-std=c99", f"-I{os.path.join(ROOT, 'include')}", src, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]                    # a field the header does not have fails here
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    finally:
        for p in (src, exe):
            if os.path.exists(p):
                os.remove(p)
    D = engine.AdamJob
    assert got == [ctypes.sizeof(D)] + [getattr(D, n).offset for n in names]
    # ... and the header has no field the mirror lacks: the struct's declarators, in order
    header = open(os.path.join(ROOT, "include", "symode.h")).read()
    body = re.search(r"typedef struct symode_adam_job \{(.*?)\} symode_adam_job;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"\*?\s*([A-Za-z_][A-Za-z0-9_]*)\s*(?:,|$)", decl.strip())]
    assert declared == names


@pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "table"])
@pytest.mark.parametrize("kind", [PLAIN, REVERSED, LATENT], ids=["plain", "reversed", "latent"])
def test_the_entry_refuses_before_any_launch(lib, kind, keyed):
    run = lambda **over: _run(lib, kind, keyed, **over)  # noqa: E731
    assert lib.symode_adam_run(None, None) == -2                                       # J == NULL
    assert run(kind=-1) == -3 and run(kind=3) == -3 and run(kind=4) == -3              # the three kinds
    assert run(idx=JUNK, order_seeds=JUNK) == -3 and run(idx=NULL, order_seeds=NULL) == -3     # the table or the seeds
    assert run(idx=NULL, order_seeds=NULL, n_epochs=0) == -3                            # ... before the nothing-to-do cases
    assert run(hyper=ODD) == -5
    assert run(hyper=NULL, log=NULL) == -2                                              # the scalar form: same checks
    # everything the entry of that kind and order refuses
    assert run(d=7) == -1 and run(order=6) == -1 and run(flags=4) == -1
    assert run(n_epochs=-1) == -3 and run(n_problems=-1) == -3 and run(epoch0=-1) == -3 and run(batch=0) == -3
    assert run(n_src=0) == -3 and run(n_src=2 ** 31) == -3
    assert run(n_params=11) == -3 and run(q_eff=JUNK, r=3, n_params=12) == -3
    if keyed:
        assert run(order_seeds=ODD) == -5 and run(n_order_seeds=3) == -3 and run(n_order_seeds=2, log=NULL) == -2
    else:
        assert run(idx=ODD) == -5 and run(n_idx_problems=3) == -3 and run(n_steps=0) == -3
    for name in ("x", "dx") + _STATE:
        assert run(**{name: NULL}) == -2, name
        assert run(**{name: ODD}) == -5, name
    empty = dict(x=NULL, dx=NULL, hyper=NULL, **{k: NULL for k in _STATE})
    assert run(n_epochs=0, **empty) == 0 and run(n_problems=0, **empty) == 0           # nothing to do: no pointer is looked at
    assert run(d=7, n_epochs=0, **empty) == -1


def test_each_kind_keeps_its_own_refusals_and_reads_no_other_kinds_fields(lib):
    assert _run(lib, REVERSED, n_g=-1) == -3 and _run(lib, REVERSED, w_x=0.0) == -3
    assert _run(lib, REVERSED, gx=NULL) == -2 and _run(lib, REVERSED, jgx=ODD) == -5
    assert _run(lib, REVERSED, n_g=0, gx=NULL, jgx=NULL, log=NULL) == -2                # no elements: none read
    assert _run(lib, LATENT, n_gen=-1) == -3 and _run(lib, LATENT, w_x=0.0) == -3 and _run(lib, LATENT, D_obs=1) == -3
    assert _run(lib, LATENT, lat_e=NULL) == -3 and _run(lib, LATENT, lat_L=NULL) == -3  # D_obs > d, n_gen > 0
    assert _run(lib, LATENT, lat_B=NULL) == -2 and _run(lib, LATENT, lat_y=ODD) == -5
    # with everything else in order the call ends at log == NULL (-2): values that would be refused earlier are not looked at
    other = dict(n_g=-1, gx=ODD, jgx=NULL, n_gen=-1, D_obs=0, lat_B=NULL, lat_y=ODD, lat_e=NULL, lat_L=NULL, log=NULL)
    assert _run(lib, PLAIN, **other) == -2 and _run(lib, PLAIN, w_x=0.0, **other) == -2
    assert _run(lib, REVERSED, **dict(other, n_g=2, gx=JUNK, jgx=JUNK)) == -2
    assert _run(lib, LATENT, **dict(other, n_gen=1, D_obs=4, lat_B=JUNK, lat_y=JUNK, lat_e=JUNK, lat_L=JUNK)) == -2
    # the order that was not chosen: its counts are not looked at
    assert _run(lib, PLAIN, True, n_idx_problems=7, n_steps=-3, log=NULL) == -2
    assert _run(lib, PLAIN, False, n_order_seeds=7, log=NULL) == -2


def test_the_binding_and_the_trainer_take_the_keyword():
    import inspect
    from symode_amd.device_adam import HYPER_COLUMNS, DeviceAdam
    assert inspect.signature(engine.HipEngine.adam_epochs).parameters["hyper"].default is None
    assert inspect.signature(DeviceAdam.fit).parameters["hyper"].default is None
    assert HYPER_COLUMNS == ("lr", "w_reg", "threshold", "w_sym") and len(HYPER_COLUMNS) == engine.ADAM_HYPER


def _trainer(**kw):
    from symode_amd.coef_map import CoefMap
    from symode_amd.device_adam import DeviceAdam
    x = torch.zeros(10, 2)
    return DeviceAdam(x, x.clone(), 2, False, False, CoefMap(2, 6), 0.03, 0.6, 0.05, 0.1, 2, 4, **kw)


def test_the_trainer_fills_missing_columns_from_its_scalars():
    tr = _trainer()
    t = tr.hyper_table({"threshold": [0.1, 0.2, 0.3]}, 3)
    assert t.dtype == torch.float32 and t.shape == (3, 4) and t.is_contiguous()
    assert torch.equal(t, torch.tensor([[0.03, 0.05, 0.1, 0.0], [0.03, 0.05, 0.2, 0.0], [0.03, 0.05, 0.3, 0.0]]))
    gx, jgx = torch.zeros(1, 10, 2), torch.zeros(1, 10, 2, 2)
    t = _trainer(reversed_sym=(gx, jgx, 0.25)).hyper_table({"lr": torch.tensor([1.0, 2.0]), "w_sym": (0.5, 0.0)}, 2)
    assert torch.equal(t, torch.tensor([[1.0, 0.05, 0.1, 0.5], [2.0, 0.05, 0.1, 0.0]]))
    lat = (torch.zeros(10, 2, 2), torch.zeros(10, 2), None, 2, None, 0.37, 2e-3)
    assert torch.equal(_trainer(latent=lat).hyper_table({}, 2)[:, 3], torch.tensor([2e-3, 2e-3]))


def test_the_trainer_refuses_what_it_cannot_place():
    tr, p0 = _trainer(), torch.zeros(3, 12)
    with pytest.raises(ValueError, match="w_sym needs a trainer with reversed_sym or latent"):
        tr.fit(p0, 0, order_seeds=[1], hyper={"w_sym": [0.1, 0.2, 0.3]})
    with pytest.raises(ValueError, match=r"unknown keys \['beta1'\]"):
        tr.fit(p0, 0, order_seeds=[1], hyper={"beta1": [0.1, 0.2, 0.3]})
    with pytest.raises(ValueError, match=r"lr must hold one value per problem \(3\)"):
        tr.fit(p0, 0, order_seeds=[1], hyper={"lr": [0.1, 0.2]})
    with pytest.raises(ValueError, match="one value per problem"):
        tr.fit(p0, 0, order_seeds=[1], hyper={"threshold": 0.1})
    with pytest.raises(ValueError, match="must be a dict"):
        tr.fit(p0, 0, order_seeds=[1], hyper=[0.1, 0.2, 0.3])
    assert tr.fit(p0, 0, order_seeds=[1], hyper={"lr": [0.1, 0.2, 0.3]})["Xi"].shape == (3, 2, 6)
