"""The state the pytest process is in after the suite: one HIP runtime, and no torch ("Which runtime the tests
use").  The file sorts last on purpose, and its two tests mean something only in a whole-suite run (``pytest tests``,
``pytest tests -m gpu``, ``pytest tests -m "not gpu"``): alone they see a process in which nothing else has run.

torch brings a libamdhip64.so of its own.  Imported into this process it either becomes a second runtime beside the one the
product library is linked to, or -- imported first -- takes that one's place, and then the GPU tests hold every kernel to a
runtime the library was not built for, and no record says so.  bench.py, the examples and the sharding workers import torch
in processes of their own; no test may import it here."""
import re
import struct
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def mapped_hip_runtimes():
    """The files with libamdhip64 in their name that this process has mapped."""
    out = set()
    for line in open("/proc/self/maps"):
        f = line.split(None, 5)
        if len(f) == 6 and "libamdhip64" in f[5]:
            out.add(f[5].strip())
    return sorted(out)


def who_imports_torch():
    """The loaded modules of this repository whose text imports torch: where to look."""
    out = []
    for mod in list(sys.modules.values()):
        path = getattr(mod, "__file__", None)
        if path and Path(path).resolve().is_relative_to(ROOT) and path.endswith(".py"):
            if re.search(r"^\s*(import torch|from torch)", Path(path).read_text(), flags=re.M):
                out.append(str(Path(path).resolve().relative_to(ROOT)))
    return sorted(out)


def runpath_of(path):
    """The DT_RUNPATH (or DT_RPATH) directories of a little-endian ELF64 shared object, from its dynamic section."""
    data = Path(path).read_bytes()
    assert data[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64 file"
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    dirs = []
    for _, kind, _, _, offset, size, link, _, _, entsize in sections:
        if kind != 6:  # SHT_DYNAMIC
            continue
        strtab = sections[link][4]
        for at in range(offset, offset + size, entsize or 16):
            tag, val = struct.unpack_from("<qQ", data, at)
            if tag in (15, 29):  # DT_RPATH, DT_RUNPATH
                end = data.index(b"\0", strtab + val)
                dirs += data[strtab + val:end].decode().split(":")
    return dirs


def check_process(dcs_lib):
    assert "torch" not in sys.modules, f"torch was imported into the pytest process; these loaded files import it: {who_imports_torch()}"
    mapped = mapped_hip_runtimes()
    assert len(mapped) <= 1, f"more than one HIP runtime is mapped: {mapped}"
    return mapped


def test_no_torch_and_one_runtime_after_the_cpu_tests(dcs_lib):
    mapped = check_process(dcs_lib)
    print(f"\nHIP runtime mapped: {mapped}")


@pytest.mark.gpu
def test_no_torch_and_the_librarys_own_runtime_after_the_gpu_tests(gpu, dcs_lib):
    """On the GPU the one runtime is there, and it is the file the library's RUNPATH names: what the kernels were built for."""
    from dc_sand_amd import _lib

    mapped = check_process(dcs_lib)
    print(f"\nHIP runtime mapped: {mapped}")
    assert len(mapped) == 1
    dirs = [Path(d).resolve() for d in runpath_of(_lib.LIB_PATH) if d and "$" not in d]
    assert dirs, "the product library has no RUNPATH"
    assert Path(mapped[0]).resolve().parent in dirs, (mapped, dirs)
