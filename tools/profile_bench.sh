#!/bin/bash
# The bench.py evidence set of profiles/rNN_bench_profile.md (run on the GPU box from the repo root):
#   bash tools/profile_bench.sh TAG        -> profile_out/TAG.json, TAG_kt*, TAG_pmc_w*, TAG_pmc_f*
# then, back in the container:  python tools/make_profile_summary.py TAG TAG.json rNN
# One un-profiled bench run (--full: with the side measurements), one rocprofv3 --kernel-trace --stats run and two --pmc passes (WRITE_SIZE, FETCH_SIZE:
# separate passes, nothing traced beside them).  The profiled runs are plain (no side measurements) so that the
# last 60 dispatches of the production kernel are the 10 warm-up + 50 timed steps.
set -e
TAG=${1:-prof}
R=${GRAFT_REPO_ROOT:-$PWD}
OUT=$R/profile_out
mkdir -p $OUT
python bench.py --full > $OUT/$TAG.json 2> $OUT/$TAG.err
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_kt -o runc -- python3 $R/bench.py > $OUT/${TAG}_kt.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/${TAG}_pmc_w -o runc -- python3 $R/bench.py --steps 6 --warmup 2 > $OUT/${TAG}_pmc_w.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/${TAG}_pmc_f -o runc -- python3 $R/bench.py --steps 6 --warmup 2 > $OUT/${TAG}_pmc_f.log 2>&1
cd $R
tail -c 400 $OUT/$TAG.json
