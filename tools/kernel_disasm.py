#!/usr/bin/env python3
"""tools/kernel_disasm.py -- compare the gfx950 code of two builds of a HIP library, kernel by kernel (no GPU needed).

    python tools/kernel_disasm.py OLD.so NEW.so

Splits each library's ``.hip_fatbin`` section at every ``__CLANG_OFFLOAD_BUNDLE__`` magic (one bundle per translation
unit), unbundles the gfx950 code object of each, disassembles it with ``llvm-objdump -d`` and compares the instructions
per symbol.  Prints the symbols of OLD that are missing or different in NEW, the new ones, and a count line; exits 1 if
any symbol of OLD changed or went missing.  What DESIGN.md section 5.7 uses to show that adding the weighted kernels
left every unweighted kernel of ``libdcs_beamformer.so`` instruction for instruction as it was.
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


def kernels(lib: str) -> dict[str, list[str]]:
    """symbol -> its instructions (comments, which carry addresses, dropped)"""
    out: dict[str, list[str]] = {}
    with tempfile.TemporaryDirectory() as tmp:
        fb = Path(tmp) / "fatbin"
        subprocess.run([str(LLVM / "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, str(fb)], check=True)
        data = fb.read_bytes()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
        for i, s in enumerate(starts):
            part, obj = Path(tmp) / f"b{i}", Path(tmp) / f"b{i}.o"
            part.write_bytes(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
            r = subprocess.run([str(LLVM / "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={part}",
                                f"--output={obj}", f"--targets={TARGET}"], capture_output=True, text=True)
            if r.returncode != 0 or not obj.exists() or obj.stat().st_size == 0:
                continue
            dis = subprocess.run([str(LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", str(obj)],
                                 check=True, capture_output=True, text=True).stdout
            cur = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line.strip())
                if m:
                    cur = m.group(1)
                    out.setdefault(cur, [])
                elif cur and line.strip():
                    out[cur].append(re.sub(r"\s*//.*$", "", line.rstrip()))
    return out


def main() -> int:
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
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


if __name__ == "__main__":
    sys.exit(main())
