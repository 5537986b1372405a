#!/bin/bash
# The measurements kept under profiles/ for a round (run on an MI355X from the repository root; outputs under the folder given as the
# first argument, default profile_out/):
# default bench line, B = 64 bench line, rocprofv3 kernel-trace summary of the bench, the conv kernels' launch table and the PMC
# counters of the split-operand convolution (counters in their own passes, no trace domains).
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
O=${1:-profile_out}; mkdir -p "$O"
timeout 300 python tools/conv_split_check.py 64 2>&1 | grep -v amdgpu.ids > $O/conv_split_check.txt
timeout 300 python tools/conv_bench.py 64 2>&1 | grep -v amdgpu.ids > $O/conv_bench_b64.txt
timeout 600 python bench.py --full > $O/bench_default.json 2> $O/bench_default.err
timeout 600 python bench.py --full --batch 64 > $O/bench_b64.json 2> $O/bench_b64.err
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $O/kt -- python bench.py --full --steps 3 --warmup 1 > $O/bench_kt.log 2>&1
python tools/kernel_stats.py $O/kt > $O/kernel_stats.txt 2>&1
rm -rf $O/kt
for c in "MfmaUtil SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_BUSY_CYCLES" "SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_INSTS_VALU SQ_INSTS_MFMA"; do
    timeout 300 rocprofv3 --pmc $c --output-format csv -d $O/pmc_split -- python tools/conv_split_pmc.py 32 3 > $O/pmc_split.log 2>&1
done
python tools/pmc_summary.py $O/pmc_split > $O/pmc_split_summary.txt
rm -rf $O/pmc_split
timeout 300 python tools/phase_times.py > $O/phase_times.txt 2>&1
timeout 300 python tools/infer_bench.py 256 2>&1 | tail -1 > $O/infer_b256.json
