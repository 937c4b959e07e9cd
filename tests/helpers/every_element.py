"""The full-size comparison that tests/test_gpu_parity.py and tests/test_gpu_streaming.py share."""
import os
import time

import numpy as np


def compare_every_element(gpu, oracle, d_buf, op, table, dt, nc_total, n_pairs, readings=(0, 1), slab_bytes=1 << 30, half=False):
    """verify_output at full size (BeamformerCoefficientTest.cu:348-357 compares EVERY element): the device tensor
    [nc_total][n_pairs][2] fp32 of ONE time step comes back in <= 1 GiB slabs through a pinned buffer and each slab
    is compared with the verifier generated on the fly over all host cores (oracle.compare_generated).  Returns
    {reading: dict(hist, max_ulp, first_over_1ulp, seconds)} accumulated over the slabs.  ``half``: the packed binary16
    output, compared as bit patterns with RN-even(verifier's fp32), distances in binary16 ulps."""
    row = n_pairs * (4 if half else 8)
    per = max(1, slab_bytes // row)
    nthreads = max(1, min(64, len(os.sched_getaffinity(0))))
    pinned = gpu.pagelocked_empty(per * n_pairs * 2, np.uint16 if half else np.float32)
    tot = {r: dict(hist=[0, 0, 0, 0], max_ulp=0, first_over_1ulp=-1, seconds=0.0) for r in readings}
    t_copy = 0.0
    for c0 in range(0, nc_total, per):
        nc = min(per, nc_total - c0)
        view = pinned[: nc * n_pairs * 2]
        t0 = time.perf_counter()
        gpu.memcpy_dtoh(view, int(d_buf) + c0 * row)
        t_copy += time.perf_counter() - t0
        for r in readings:
            res = oracle.compare_generated(op, table, [dt], c0, nc, view, nthreads=nthreads, reading=r)
            acc = tot[r]
            acc["hist"] = [a + b for a, b in zip(acc["hist"], res["hist"])]
            acc["max_ulp"] = max(acc["max_ulp"], res["max_ulp"])
            if acc["first_over_1ulp"] < 0 and res["first_over_1ulp"] >= 0:
                acc["first_over_1ulp"] = c0 * n_pairs * 2 + res["first_over_1ulp"]
            acc["seconds"] += res["seconds"]
    tot["copy_seconds"] = t_copy
    tot["threads"] = nthreads
    return tot
