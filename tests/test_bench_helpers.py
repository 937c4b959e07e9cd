"""bench.py pieces that run without a GPU: the cpu_baseline leg (oracle timed on a
bounded slab) and the committed PMC traffic file it reads."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def test_cpu_baseline_leg_small_shape(oracle):
    sys.path.insert(0, str(ROOT))
    import bench
    from dc_sand_amd import BeamformerParameters

    bp = BeamformerParameters(NR_CHANNELS=256, NR_STATIONS=8, NR_BEAMS=16)
    table = oracle.simulate_input(oracle.params_from(bp))
    out = bench.cpu_baseline(bp, table, seconds=0.2)
    assert out["unit"] == "Gcoeff/s" and out["cores"] == 1 and out["kind"] == "port"
    assert out["value"] > 0 and "channels [0," in out["sample"]


def test_committed_pmc_traffic_matches_workload():
    sys.path.insert(0, str(ROOT))
    import bench

    d = json.loads((ROOT / "profiles" / "pmc_write_size.json").read_text())
    algo = 8 * 64 * 1024 * 32768
    assert d["algorithmic_bytes_per_launch"] == algo
    t, src = bench.pmc_traffic(algo)
    assert t is not None and 0.99 < t / algo < 1.05  # measured HBM bytes ~ algorithmic bytes
    assert "pmc_write_size.json" in src and "rocprofv3 --pmc" in src  # the JSON line says where the number comes from
    assert bench.pmc_traffic(algo // 2) == (None, None)  # another workload: no number is invented


def test_gpus_n_without_ranks_is_an_error_not_a_one_gpu_line(dcs_lib):
    """bench.py's launch contract, the part that needs no GPU: ``--gpus 2`` without a launcher starts two rank
    processes; here neither finds a HIP device, so the command exits non-zero and prints NO JSON line (round 2's
    bench.py would have measured one GPU and printed ``n_gpus: 1``).  Also: a launcher environment whose WORLD_SIZE
    disagrees with --gpus is refused."""
    import os
    import subprocess

    import pytest

    from dc_sand_amd import device

    if device.device_count() >= 1:  # the count the `gpu` fixture takes; torch stays out of this process
        pytest.skip("a GPU is present: tests/test_bench_contract.py covers this case there")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"], capture_output=True,
                         text=True, env=env, timeout=600)
    assert res.returncode != 0 and res.stdout.strip() == ""
    assert "no result line" in res.stderr and "rank" in res.stderr
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "8"], capture_output=True, text=True,
                         env=dict(env, RANK="0", LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="29999"), timeout=600)
    assert res.returncode != 0 and res.stdout.strip() == "" and "WORLD_SIZE=2" in res.stderr


class _HostDevice:
    """The two calls bench.dump_outputs makes on dc_sand_amd.device, served from a host array standing for the output."""

    def __init__(self, buf: np.ndarray):
        self.buf, self.base = buf.view(np.uint8).ravel(), 1 << 40

    def stream_synchronize(self, stream):
        pass

    def memcpy_dtoh(self, dst, src):
        off = int(src) - self.base
        assert 0 <= off and off + dst.nbytes <= self.buf.size
        dst.view(np.uint8).ravel()[:] = self.buf[off:off + dst.nbytes]


def test_dump_outputs_is_a_seeded_bounded_sample(tmp_path):
    """--dump-outputs: the same rows for the same shape, the rows' values as the output holds them, at most the budget;
    a channel row wider than the budget is sampled at seeded (antenna, beam) pairs; at N > 1 one file per rank."""
    sys.path.insert(0, str(ROOT))
    import bench
    from dc_sand_amd import BeamformerParameters

    def dump(d, bp, rank=0, n_ranks=1):
        out = np.random.default_rng(rank).standard_normal((bp.NR_CHANNELS, bp.NR_STATIONS, bp.NR_BEAMS, 2)).astype(np.float32)
        dev = _HostDevice(out)
        bench.dump_outputs(str(d), dev.base, bp, rank, n_ranks, dev, None)
        return out

    bp = BeamformerParameters(NR_CHANNELS=4096, NR_STATIONS=64, NR_BEAMS=256)  # 128 KiB per channel row
    out = dump(tmp_path / "a", bp)
    dump(tmp_path / "b", bp)
    c, ch = np.load(tmp_path / "a" / "coefficients.npy"), np.load(tmp_path / "a" / "coefficient_channels.npy")
    assert c.dtype == np.float32 and ch.dtype == np.float64 and c.nbytes == bench.DUMP_BYTES and len(np.unique(ch)) == len(ch)
    assert np.array_equal(c, out[ch.astype(np.int64)])
    assert np.array_equal(ch, np.load(tmp_path / "b" / "coefficient_channels.npy"))
    wide = BeamformerParameters(NR_CHANNELS=2, NR_STATIONS=64, NR_BEAMS=65536)  # 32 MiB per channel row
    out = dump(tmp_path / "w", wide)
    c, ch, pr = (np.load(tmp_path / "w" / f) for f in ("coefficients.npy", "coefficient_channels.npy", "coefficient_pairs.npy"))
    assert c.nbytes == bench.DUMP_BYTES and c.shape == (1, bench.DUMP_BYTES // 8, 2)
    assert np.array_equal(c[0], out[int(ch[0])].reshape(-1, 2)[pr.astype(np.int64)])
    assert sum(f.stat().st_size for f in (tmp_path / "w").iterdir()) < 64e6
    for r in range(2):
        dump(tmp_path / "r", bp, r, 2)
    assert sorted(f.name for f in (tmp_path / "r").iterdir()) == ["coefficient_channels.npy", "coefficients_rank0.npy", "coefficients_rank1.npy"]
    assert np.load(tmp_path / "r" / "coefficients_rank1.npy").nbytes == bench.DUMP_BYTES // 2


def test_named_configs_are_the_baseline_shapes():
    sys.path.insert(0, str(ROOT))
    import bench

    assert bench.CONFIGS["cfg3"]["ant"] * bench.CONFIGS["cfg3"]["beams_per_gpu"] * bench.CONFIGS["cfg3"]["chan"] == 64 * 1024 * 32768
    c4 = bench.CONFIGS["cfg4"]
    assert (c4["ant"], c4["beams_per_gpu"] * 8, c4["chan"]) == (256, 4096, 32768)  # BASELINE configs[3] over 8 GPUs
