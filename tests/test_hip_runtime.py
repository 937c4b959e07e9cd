"""Which HIP runtime the graph helper of the GPU tests binds (tests/helpers/hip_graph.py; DESIGN.md, "Which runtime the
tests use").  No GPU and no HIP call: only symbol lookups, in a child process per order of "load the product library" and
"import torch".  torch brings a libamdhip64.so of its own, with the SONAME of the system's, so the order decides what a
process has mapped:

    library first, then torch    two runtimes: the library's NEEDED entry took the one its RUNPATH names, torch took its own
    torch first, then library    one runtime: torch's copy, which also satisfies the library's NEEDED entry

In both, every entry point the helper calls must lie in the same mapped file as the hipStreamBeginCapture that a lookup on
the library's own handle finds: the runtime that makes the library's streams is the one that captures them.  A helper that
opens "libamdhip64.so" by name fails the first order: the name matches torch's copy, already mapped under that name."""
import json
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HELPER = ROOT / "tests" / "helpers" / "hip_graph.py"

CHILD = r"""
import ctypes, json, sys
root, order, names = sys.argv[1], sys.argv[2], sys.argv[3].split(",")
sys.path[:0] = [root, root + "/tests"]


def load_library():
    from dc_sand_amd import _lib
    return _lib.lib()


def load_torch():
    import torch  # noqa: F401


for step in order.split("-"):
    {"library": load_library, "torch": load_torch}[step]()

from helpers import hip_graph


def maps():
    out = []
    for line in open("/proc/self/maps"):
        f = line.split(None, 5)
        if len(f) == 6 and f[5].strip().startswith("/"):
            lo, hi = (int(x, 16) for x in f[0].split("-"))
            out.append((lo, hi, f[5].strip()))
    return out


def file_of(fn, regions):
    at = ctypes.cast(fn, ctypes.c_void_p).value
    hits = {path for lo, hi, path in regions if lo <= at < hi}
    assert len(hits) == 1, (hex(at), hits)
    return hits.pop()


hip = hip_graph._hip()
regions = maps()
print(json.dumps({
    "handle": file_of(load_library()["hipStreamBeginCapture"], regions),
    "graph": {name: file_of(getattr(hip, name), regions) for name in names},
    "mapped": sorted({path for _, _, path in regions if "libamdhip64" in path}),
    "torch": "torch" in sys.modules,
}))
"""


def entry_points():
    """The HIP functions the helper calls, from its text: ``_hip().hipX(`` and ``hip.hipX(``."""
    return sorted(set(re.findall(r"\b(?:_hip\(\)|hip)\.(hip[A-Z]\w+)\(", HELPER.read_text())))


def test_the_helper_names_every_entry_point_it_calls_and_opens_no_library():
    from helpers import hip_graph

    names = entry_points()
    assert len(names) == 9 and "hipStreamBeginCapture" in names and "hipGraphLaunch" in names
    assert names == sorted(hip_graph.ENTRY_POINTS)
    text = HELPER.read_text()
    assert "CDLL(" not in text and "dlopen" not in text


@pytest.mark.parametrize("order", ["library-torch", "torch-library"])
def test_every_entry_point_is_in_the_librarys_own_runtime(dcs_lib, order):
    res = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), order, ",".join(entry_points())], capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    seen = json.loads(res.stdout.strip().splitlines()[-1])
    print(f"\n{order}: mapped {seen['mapped']}\n  the library's handle binds {seen['handle']}\n  hip_graph binds {sorted(set(seen['graph'].values()))}")
    assert seen["torch"] and "libamdhip64" in seen["handle"] and seen["handle"] in seen["mapped"]
    assert 1 <= len(seen["mapped"]) <= 2
    other = {name: path for name, path in seen["graph"].items() if path != seen["handle"]}
    assert not other, f"the helper binds {other}, the library's own handle {seen['handle']}"
