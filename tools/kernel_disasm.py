#!/usr/bin/env python3
"""tools/kernel_disasm.py -- compare the gfx950 code of two builds of a HIP library, kernel by kernel (no GPU needed).

    python tools/kernel_disasm.py [--by-body] OLD.so NEW.so

Splits each library's ``.hip_fatbin`` section at every ``__CLANG_OFFLOAD_BUNDLE__`` magic (one bundle per translation
unit), unbundles the gfx950 code object of each, disassembles it with ``llvm-objdump -d`` and compares the instructions
per symbol.  Prints the symbols of OLD that are missing or different in NEW, the new ones, and a count line; exits 1 if
any symbol of OLD changed or went missing.  What DESIGN.md section 5.7 uses to show that adding the weighted kernels
left every unweighted kernel of ``libdcs_beamformer.so`` instruction for instruction as it was.

``--by-body`` compares across a rename: each symbol of OLD is matched to the symbol of NEW that has its instructions, or,
failing that, its opcode sequence (every instruction reduced to its mnemonic: the same code with other register numbers).
Prints every symbol that is not identical under its own name, with both kernels' register, scratch, spill, LDS and
kernarg figures from the code objects' metadata (old / new); exits 1 if a symbol of OLD has no such match or a figure
changed.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "lib" / "llvm" / "bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


RESOURCES = (".vgpr_count", ".sgpr_count", ".agpr_count", ".private_segment_fixed_size", ".vgpr_spill_count",
             ".group_segment_fixed_size", ".kernarg_segment_size")


def code_objects(lib: str, tmp: str):
    """the gfx950 code object of each translation unit of lib, unbundled into tmp"""
    fb = Path(tmp) / "fatbin"
    subprocess.run([str(LLVM / "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, str(fb)], check=True)
    data = fb.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    for i, s in enumerate(starts):
        part, obj = Path(tmp) / f"b{i}", Path(tmp) / f"b{i}.o"
        part.write_bytes(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
        r = subprocess.run([str(LLVM / "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={part}",
                            f"--output={obj}", f"--targets={TARGET}"], capture_output=True, text=True)
        if r.returncode == 0 and obj.exists() and obj.stat().st_size != 0:
            yield obj


def kernels(lib: str, resources: dict[str, dict[str, int]] | None = None) -> dict[str, list[str]]:
    """symbol -> its instructions (comments, which carry addresses, dropped); with resources, also symbol -> the RESOURCES
    of its kernel, from the code objects' metadata"""
    out: dict[str, list[str]] = {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in code_objects(lib, tmp):
            dis = subprocess.run([str(LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", str(obj)],
                                 check=True, capture_output=True, text=True).stdout
            cur = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line.strip())
                if m:
                    cur = m.group(1)
                    out.setdefault(cur, [])
                elif cur and line.strip() and line.strip() != "...": # (llvm-objdump's mark for the zero padding behind a kernel)
                    out[cur].append(re.sub(r"\s*//.*$", "", line.rstrip()))
            if resources is None:
                continue
            notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(obj)], check=True, capture_output=True, text=True).stdout
            entry: dict[str, str] = {}
            for line in notes.splitlines() + ["  - .end: 0"]: # a kernel's entry: "  - .key: value", then "    .key: value" lines
                m = re.match(r"^(  - |    )(\.\w+):\s*(.*)$", line)
                if not m:
                    continue
                if m.group(1) == "  - ":
                    if ".name" in entry:
                        resources[entry[".name"]] = {k: int(entry[k]) for k in RESOURCES if k in entry}
                    entry = {}
                entry[m.group(2)] = m.group(3)
    return out


def opcodes(body: list[str]) -> list[str]:
    """each instruction reduced to its mnemonic"""
    return [line.split()[0] for line in body if line.split()]


def match_bodies(old: dict[str, list[str]], new: dict[str, list[str]]) -> dict[str, tuple[str, str | None]]:
    """For each symbol of old, (verdict, its symbol in new): "identical" -- same instructions; "renamed-registers" -- same
    opcode sequence, other operands; "different" -- the same symbol with another opcode sequence; "missing" -- neither the
    symbol nor a body like it.  A symbol of new is given to one symbol of old only; the same name goes first, then equal
    bodies, and among equal opcode sequences the one with the fewest differing lines."""
    verdict: dict[str, tuple[str, str | None]] = {}
    free = set(new)
    for k in sorted(old):
        if k in new and old[k] == new[k]:
            verdict[k] = ("identical", k)
            free.discard(k)
    rest = [k for k in sorted(old) if k not in verdict]
    for k in rest:
        twin = next((n for n in ([k] if k in free else []) + sorted(free) if new[n] == old[k]), None)
        if twin is not None:
            verdict[k] = ("identical", twin)
            free.discard(twin)
    for k in [k for k in rest if k not in verdict]:
        ops = opcodes(old[k])
        same = [n for n in sorted(free) if len(new[n]) == len(old[k]) and opcodes(new[n]) == ops]
        if same:
            twin = min(same, key=lambda n: (n != k, sum(x != y for x, y in zip(old[k], new[n]))))
            verdict[k] = ("renamed-registers", twin)
            free.discard(twin)
        else:
            verdict[k] = ("different", k) if k in new else ("missing", None)
    return verdict


def main() -> int:
    args = [x for x in sys.argv[1:] if x != "--by-body"]
    by_body = len(args) != len(sys.argv) - 1
    if len(args) != 2:
        print(__doc__)
        return 2
    if by_body:
        return report_by_body(*args)
    old, new = kernels(args[0]), kernels(args[1])
    changed = [k for k in sorted(old) if k in new and old[k] != new[k]]
    missing = [k for k in sorted(old) if k not in new]
    added = [k for k in sorted(new) if k not in old]
    for k in missing:
        print("MISSING", k)
    for k in changed:
        print("DIFFERENT", k)
    for k in added:
        print("NEW", k)
    print(f"{len(old)} symbols before: {len(old) - len(changed) - len(missing)} identical, {len(changed)} different, "
          f"{len(missing)} missing; {len(added)} new")
    return 1 if changed or missing else 0


def report_by_body(old_lib: str, new_lib: str) -> int:
    res_old: dict[str, dict[str, int]] = {}
    res_new: dict[str, dict[str, int]] = {}
    old, new = kernels(old_lib, res_old), kernels(new_lib, res_new)
    verdict = match_bodies(old, new)
    count = {v: 0 for v in ("identical", "renamed-registers", "different", "missing")}
    bad = False
    for k in sorted(old):
        v, twin = verdict[k]
        count[v] += 1
        ro, rn = res_old.get(k, {}), res_new.get(twin, {}) if twin else {}
        if v == "identical" and twin == k and ro == rn:
            continue # nothing to say
        bad |= v in ("different", "missing") or ro != rn
        print(v.upper(), k, *(["->", twin] if twin and twin != k else []))
        if v == "renamed-registers":
            print("    lines that differ:", sum(x != y for x, y in zip(old[k], new[twin])), "of", len(old[k]))
        for key in RESOURCES:
            if key in ro or key in rn:
                print(f"    {key[1:]}: {ro.get(key)} / {rn.get(key)}" + ("" if ro.get(key) == rn.get(key) else "   <-- not equal"))
    taken = {twin for _, twin in verdict.values()}
    for k in sorted(new):
        if k not in taken:
            print("NEW", k)
    print(f"{len(old)} symbols before: " + ", ".join(f"{n} {v}" for v, n in count.items()) + f"; {len(set(new) - taken)} new")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
