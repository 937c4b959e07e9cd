#!/usr/bin/env python3
"""tools/stage_overlap.py -- where do the staging copy and gather run?  Reads the CSVs of one
``rocprofv3 --kernel-trace --memory-copy-trace --output-format csv`` run (of ``measure.py stream --table-mode staged-*``)
and reports, for every host-to-device copy and every ``bf_gather_beams_kernel`` dispatch, whether it ran while a
generator kernel (``bf_tiled_kernel``) was running, and on which hardware queue each kind ran.

    python tools/stage_overlap.py <rocprofv3 output directory> [last]   -> one JSON line
        last: the generator figures (duration, gap to the next) over the last `last` generator dispatches only -- the
        tick loop at the end of the run, not the autotune before it
"""
from __future__ import annotations

import csv
import json
import sys
from pathlib import Path

import numpy as np


def _rows(d: Path, suffix: str):
    out = []
    for f in sorted(d.rglob(f"*{suffix}")):
        with open(f, newline="") as fh:
            out += list(csv.DictReader(fh))
    return out


def _span(r):
    return int(r["Start_Timestamp"]), int(r["End_Timestamp"])


def summarise(d: Path, last: int = 0) -> dict:
    kernels = _rows(d, "kernel_trace.csv")
    copies = [_span(r) for r in _rows(d, "memory_copy_trace.csv") if "HOST_TO_DEVICE" in r.get("Direction", "").upper()]
    gens = sorted((_span(r) + (r.get("Queue_Id", "?"),) for r in kernels if "bf_tiled_kernel" in r["Kernel_Name"]))
    gathers = [_span(r) + (r.get("Queue_Id", "?"),) for r in kernels if "bf_gather_beams_kernel" in r["Kernel_Name"]]
    g_start = np.array([g[0] for g in gens], dtype=np.int64)
    g_end = np.array([g[1] for g in gens], dtype=np.int64)

    def overlap(items):
        """items: (start, end, ...) -- how many lie inside / overlap / miss a generator kernel."""
        inside = part = 0
        for s, e, *_ in items:
            i = np.searchsorted(g_start, s, side="right") - 1  # the last generator that started before s
            if i >= 0 and g_end[i] >= e:
                inside += 1
            elif (i >= 0 and g_end[i] > s) or (i + 1 < len(g_start) and g_start[i + 1] < e):
                part += 1
        dur = [e - s for s, e, *_ in items]
        return dict(n=len(items), inside_a_generator=inside, partly=part, outside=len(items) - inside - part,
                    median_us=float(np.median(dur)) / 1e3 if dur else None)

    ls, le = (g_start[-last:], g_end[-last:]) if last else (g_start, g_end)
    gaps = (ls[1:] - le[:-1]) / 1e3 if len(ls) > 1 else np.array([])
    return {
        "generator": dict(n=len(gens), window=len(ls), median_us=float(np.median(le - ls)) / 1e3 if len(ls) else None,
                          median_gap_us=float(np.median(gaps)) if gaps.size else None,
                          median_start_to_start_us=float(np.median(np.diff(ls))) / 1e3 if len(ls) > 1 else None,
                          queues=sorted({g[2] for g in gens})),
        "h2d_copy": overlap(copies),
        "gather": dict(overlap(gathers), queues=sorted({g[2] for g in gathers})),
    }


if __name__ == "__main__":
    print(json.dumps(summarise(Path(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 0)))
