#!/usr/bin/env python3
"""Which kernels of the built libsymode_hip.so touch scratch memory?

Pulls every gfx950 code object out of the library's clang offload bundles (section .hip_fatbin), disassembles it with
llvm-objdump and counts scratch_* instructions per kernel.  `--fail-on PATTERN` exits 1 if a kernel whose demangled name
matches the regular expression has any (tests/test_abi.py uses it for the D <= 3, order <= 3 libraries).

    python tools/scratch_report.py [path/to/libsymode_hip.so] [--fail-on 'Library<[123], [123], ']

`--compare OTHER [--kernels PATTERN]` prints, for every kernel of the library whose demangled name matches PATTERN, whether
its generated code has the resources of the same kernel in OTHER (a build of another commit): VGPR, AGPR, SGPR counts,
scratch and LDS bytes from the kernel metadata, and the count of every instruction mnemonic from the disassembly.  "same"
means all of them equal (operand order and instruction order are not looked at); otherwise the differing counts, OTHER -> this.
"""
import argparse
import collections
import os
import re
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def code_objects(blob):
    """yield (triple, bytes) of every device code object of every bundle in the file"""
    pos = blob.find(MAGIC)
    while pos >= 0:
        n = struct.unpack_from("<Q", blob, pos + len(MAGIC))[0]
        q = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, q)
            triple = blob[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if "amdgcn" in triple and size > 0:
                yield triple, blob[pos + off:pos + off + size]
        pos = blob.find(MAGIC, pos + 1)


def scratch_by_kernel(lib):
    blob = open(lib, "rb").read()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, (_, co) in enumerate(code_objects(blob)):
            path = os.path.join(tmp, f"{k}.co")
            with open(path, "wb") as f:
                f.write(co)
            asm = subprocess.run([OBJDUMP, "-d", "--demangle", path], capture_output=True, text=True, check=True).stdout
            name = None
            for line in asm.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
                if m:
                    name = m.group(1)
                    out.setdefault(name, 0)
                elif name is not None and re.search(r"\bscratch_(load|store)", line):
                    out[name] += 1
    return out


READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
RESOURCES = {"vgpr_count": "vgpr", "agpr_count": "agpr", "sgpr_count": "sgpr", "private_segment_fixed_size": "scratch",
             "group_segment_fixed_size": "lds"}


def run(*cmd):
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def kernel_table(lib, pattern):
    """{demangled kernel name: {"vgpr", "agpr", "sgpr", "scratch", "lds": int, "ops": Counter of mnemonics}}"""
    blob = open(lib, "rb").read()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, (_, co) in enumerate(code_objects(blob)):
            path = os.path.join(tmp, f"{k}.co")
            with open(path, "wb") as f:
                f.write(co)
            label = re.compile(r"^[0-9a-f]+ <(.*)>:$")
            mangled = [m.group(1) for m in map(label.match, run(OBJDUMP, "-d", path).splitlines()) if m]
            ops, names, name = {}, [], None
            for line in run(OBJDUMP, "-d", "--demangle", path).splitlines():
                m = label.match(line)
                if m:
                    name = m.group(1)
                    names.append(name)
                    ops[name] = collections.Counter()
                elif name is not None:
                    m = re.match(r"^\s+([a-z][a-z0-9_]+)\b", line)
                    if m:
                        ops[name][m.group(1)] += 1
            demangled = dict(zip(mangled, names))
            # the kernels of the metadata note: one "  - .agpr_count:" item each, its own keys at an indent of four
            for item in re.split(r"(?m)^  - (?=\.)", run(READELF, "--notes", path))[1:]:
                keys = dict(re.findall(r"(?m)^(?:    |)\.(\w+):\s+(\S+)", item))
                name = demangled.get(keys.get("name"))
                if name is None or not re.search(pattern, name):
                    continue
                out[name] = {short: int(keys[key]) for key, short in RESOURCES.items()}
                out[name]["ops"] = ops[name]
    return out


def compare(lib, other, pattern):
    mine, theirs = kernel_table(lib, pattern), kernel_table(other, pattern)
    print(f"{len(mine)} kernels matching {pattern!r}; {other} -> {lib}")
    differ = unmatched = 0
    for name in sorted(set(mine) | set(theirs)):
        if name not in mine or name not in theirs:
            what = "only in " + (lib if name in mine else other)
            unmatched += 1
        else:
            a, b = theirs[name], mine[name]
            d = [f"{k} {a[k]} -> {b[k]}" for k in RESOURCES.values() if a[k] != b[k]]
            d += [f"{op} {a['ops'][op]} -> {b['ops'][op]}" for op in sorted(set(a["ops"]) | set(b["ops"])) if a["ops"][op] != b["ops"][op]]
            r = b
            what = "same" if not d else "; ".join(d)
            what += f"   [{r['vgpr']} VGPRs, {r['agpr']} AGPRs, {r['sgpr']} SGPRs, {r['scratch']} B scratch, {r['lds']} B LDS, {sum(r['ops'].values())} instructions]"
        differ += not what.startswith("same")
        print(f"{name}: {what}")
    print(f"{differ} differ")
    return 1 if unmatched else 0                 # a kernel on one side only: the names no longer match, the table proves nothing


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib", nargs="?", default=os.path.join(ROOT, "symmetry-ode-discovery_amd", "libsymode_hip.so"))
    ap.add_argument("--fail-on", default=None, help="regular expression on the demangled kernel name")
    ap.add_argument("--compare", metavar="OTHER", default=None, help="another build of the library: per-kernel resource table against it")
    ap.add_argument("--kernels", default="symreg_reversed_kernel", help="with --compare: regular expression on the demangled kernel name")
    a = ap.parse_args()
    if a.compare:
        return compare(a.lib, a.compare, a.kernels)
    res = scratch_by_kernel(a.lib)
    bad = {k: v for k, v in res.items() if v > 0}
    print(f"{len(res)} kernels, {len(bad)} with scratch instructions")
    for k, v in sorted(bad.items(), key=lambda kv: -kv[1]):
        print(f"{v:6d}  {k[:150]}")
    if a.fail_on:
        hit = [k for k in bad if re.search(a.fail_on, k)]
        if hit:
            print(f"FAIL: {len(hit)} kernels matching {a.fail_on!r} use scratch")
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
