"""Turn a profile_out/<tag>_{kt,pmc_w,pmc_f} set + bench JSON (tools/profile_bench.sh) into the committed profiles/ artefacts."""
import csv
import glob
import json
import shutil
import statistics as st
import sys
from pathlib import Path

R = str(Path(__file__).resolve().parent.parent) + "/"
O = R + "profile_out/"  # what tools/profile_bench.sh wrote
tag, bench_json, rnd = sys.argv[1], sys.argv[2], sys.argv[3]  # e.g. prof5 bench5.json r01
f = glob.glob(O + f"{tag}_kt/**/*kernel_trace.csv", recursive=True)[0]
import re

# production symbol of the fp32 generator: bf_tiled_kernel<false, TPB, NT, ALIGNED, NOMATH=false, TAG=0, INL, TERMS, HALF>;
# dcs_bf_autotune's trial launches run as <..., TAG=1, ...>
PROD_RE = re.compile(r"bf_tiled_kernel<false, \d, (true|false), (true|false), false, 0, (true|false), (true|false), false>")


def is_prod(name):
    return PROD_RE.search(name) is not None


rows = [r for r in csv.DictReader(open(f)) if is_prod(r["Kernel_Name"])]
bench_rows = rows[-60:]  # 10 warm-up + 50 timed
d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in bench_rows]
timed = d[10:]
vg = bench_rows[-1]
shutil.copy(glob.glob(O + f"{tag}_kt/**/*kernel_stats.csv", recursive=True)[0], R + f"profiles/{rnd}_bench_kernel_stats.csv")
shutil.copy(O + bench_json, R + f"profiles/{rnd}_bench_n1.json")
prof = None
for l in open(O + f"{tag}_kt.log"):
    if l.startswith('{"metric"'):
        prof = json.loads(l)
        open(R + f"profiles/{rnd}_bench_n1_under_rocprof.json", "w").write(l)
b = json.loads(open(O + bench_json).read())
res = {}
for d_, name in ((f"{tag}_pmc_w", "WRITE_SIZE"), (f"{tag}_pmc_f", "FETCH_SIZE")):
    ff = glob.glob(O + f"{d_}/**/*counter_collection.csv", recursive=True)[0]
    v = [float(r["Counter_Value"]) for r in csv.DictReader(open(ff)) if is_prod(r["Kernel_Name"]) and r["Counter_Name"] == name]
    res[name] = (len(v), st.mean(v))
    shutil.copy(ff, R + f"profiles/{rnd}_pmc_{name.lower()}_counter_collection.csv")
algo = 17179869184
w = res["WRITE_SIZE"][1] * 1024
fr = res["FETCH_SIZE"][1] * 1024 * 2
json.dump(
    {
        "workload": "64ant x 1024beam x 32768chan, fp32, one time step per launch",
        "kernel": vg["Kernel_Name"],
        "round": rnd,
        "launch_geometry": b["config"]["launch_geometry"],
        "algorithmic_bytes_per_launch": algo,
        "hbm_write_bytes_per_launch": w,
        "hbm_read_bytes_per_launch": fr,
        "hbm_bytes_per_launch": w + fr,
        "write_over_algorithmic": w / algo,
        "method": "rocprofv3 --pmc WRITE_SIZE and --pmc FETCH_SIZE in separate passes (bench.py --steps 6 --warmup 2); "
                  "WRITE_SIZE[KiB]*1024 (exact for 16-B-per-lane streaming stores); FETCH_SIZE[KiB]*1024*2 (gfx950 reports half of a "
                  "wide coalesced read stream) -- MI355X_MICROARCH.md section HBM",
        "launches_averaged": res["WRITE_SIZE"][0],
    },
    open(R + "profiles/pmc_write_size.json", "w"),
    indent=1,
)
cb = b.get("cpu_baseline", {})
# whole-run stats for the tiled kernel (includes the ~60 autotune launches at other geometries)
allms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows]
md = f"""# {rnd} — bench.py under rocprofv3 (MI355X, ROCm 7.2; final build of the round)

Commands (`bash tools/profile_bench.sh`; the profiler from /tmp with `TMPDIR=/tmp`, program directly after `--`):

```
python bench.py --full                                                   -> {rnd}_bench_n1.json
rocprofv3 --kernel-trace --stats --output-format csv -- python3 bench.py
                                                                         -> {rnd}_bench_kernel_stats.csv, {rnd}_bench_n1_under_rocprof.json
rocprofv3 --pmc WRITE_SIZE --output-format csv -- python3 bench.py --steps 6 --warmup 2
rocprofv3 --pmc FETCH_SIZE --output-format csv -- python3 bench.py --steps 6 --warmup 2
                                                                         -> {rnd}_pmc_*_counter_collection.csv, pmc_write_size.json
```
(plain runs: without the side measurements of `--full`, so that the last 60 dispatches of the production kernel are the
10 warm-up + 50 timed steps.)

Dominant kernel: `{vg['Kernel_Name'].split('(')[1] if False else vg['Kernel_Name'][:100]}` (fp32, 1 tile per workgroup, nontemporal stores,
terms-table variant: its pre-pass `bf_terms_kernel` is the other kernel of every step, ~3 us; the `<..., 1, ...>` rows of the stats file
are the same code under the tuner's symbol: `dcs_bf_autotune`'s trial launches), launch
geometry {b['config']['launch_geometry']}: {vg['VGPR_Count']} VGPRs, {vg['LDS_Block_Size']} B LDS, scratch {vg['Scratch_Size']}, > 99 % of GPU time.

| quantity | value |
|---|---|
| bench.py (un-profiled): `value`, `ms_per_step` | {b['value']:.1f} Gcoeff/s, {b['ms_per_step']:.3f} ms |
| bench.py `roofline.kernel_ms` (HIP events on the launch stream over the 50 timed steps / 50) | {b['roofline']['kernel_ms']:.3f} ms -> {b['roofline']['achieved'] / 1e3:.2f} TB/s algorithmic = {b['roofline']['frac']:.3f} of 8 TB/s |
| the profiled run (`{rnd}_bench_kernel_stats.csv`): `value`, `ms_per_step`, `kernel_ms` | {prof['value']:.1f} Gcoeff/s, {prof['ms_per_step']:.3f} ms, {prof['roofline']['kernel_ms']:.3f} ms |
| rocprofv3 kernel trace of that run, the 50 timed launches (last 50 dispatches): mean / median / min / max | {st.mean(timed):.3f} / {st.median(timed):.3f} / {min(timed):.3f} / {max(timed):.3f} ms |
| same, 10 warm-up + 50 timed launches | {st.mean(d):.4f} ms |
| rocprofv3 `--stats` AverageNs of the production kernel symbol, all {len(allms)} calls (untimed settle launches + 10 warm-up + 50 timed) | {st.mean(allms):.4f} ms |
| WRITE_SIZE per launch | {res['WRITE_SIZE'][1]:.0f} KiB x 1024 = {w / 1e9:.4f} GB = {w / algo:.5f} x algorithmic ({algo / 1e9:.4f} GB) |
| FETCH_SIZE per launch | {res['FETCH_SIZE'][1]:.0f} KiB x 1024 x 2 (gfx950 correction) = {fr / 1e6:.2f} MB (the pre-pass reads the 1 MiB delay table; the main kernel its 512 KiB terms table) |
| CPU baseline in the same bench run (oracle = restated reference verifier) | {cb.get('value', 0) * 1e3:.1f} Mcoeff/s on 1 thread ({cb.get('sample', '')}); {cb.get('all_cores', {}).get('value', 0):.2f} Gcoeff/s on {cb.get('all_cores', {}).get('cores', 0)} threads |

bench.py first lets the library measure its launch geometry (untimed; separate kernel symbols), then runs 24 plain fills of the output buffer
(`__amd_rocclr_fillBufferAligned`, ~2.8 ms each = 6.1 TB/s) to bring the device out of idle; the first few generator launches are
still 3-10 % slower than steady state and fall in the W = 10 warm-up steps.  The event-based `kernel_ms`, the per-dispatch
trace of the same launches and the `--stats` average agree within 1 % (the event span also holds the 5-us slice gather and the gaps between launches, which grow a little under the profiler).  HBM traffic equals the algorithmic bytes: every store is a whole-line write,
nothing is re-read.  Box-to-box spread of `value`: 894-937 Gcoeff/s over fifteen boxes in round 2 (thirteen of them 915-937); the bench lines of round 3's boxes: 913.1, 918.1, 928.3, 930.0, 930.4, 930.8.
"""
# (a section appended by hand below a "## A minute of back-to-back steps" heading survives regeneration)
try:
    old = open(R + f"profiles/{rnd}_bench_profile.md").read()
    if "\n## A minute" in old:
        md += old[old.index("\n## A minute"):]
except FileNotFoundError:
    pass
open(R + f"profiles/{rnd}_bench_profile.md", "w").write(md)
print(md[md.index("| quantity"):])
