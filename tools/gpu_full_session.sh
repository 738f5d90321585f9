#!/bin/bash
# One GPU session that regenerates everything under profiles/: parity suite, smoke, the bench line, step + embedding-forward
# anatomy, the evaluation kernels' trace, counter passes.   bash tools/gpu_full_session.sh <output folder>
# (the --full bench line and the evaluation trace's log go to <output folder>)
mkdir -p gpurun_out
out=$(realpath -m "${1:?usage: bash tools/gpu_full_session.sh <output folder>}"); mkdir -p "$out"
python -m pytest tests -m gpu -q --maxfail=25 --durations=8 > gpurun_out/full_pytest.log 2>&1
echo "pytest rc $?" >> gpurun_out/full_pytest.log
tail -14 gpurun_out/full_pytest.log
python -c "import __graft_entry__ as g; g.smoke()" > gpurun_out/full_smoke.log 2>&1; tail -2 gpurun_out/full_smoke.log
python bench.py --full > "$out/full_bench.json" 2> "$out/full_bench.err"
echo "bench rc $?"
bash tools/prof_train.sh full > gpurun_out/full_anatomy.md 2>&1
head -24 gpurun_out/full_anatomy.md
cp gpurun_out/prof_full.md gpurun_out/full_train_kernel_stats.md 2>/dev/null
bash tools/prof_embed.sh fulle > gpurun_out/full_embed_anatomy.md 2>&1
tail -75 gpurun_out/full_embed_anatomy.md
# the evaluation half of the metric: kernel trace of the same bench command (eval.roofline.frac is reproducible from it)
repo=$(pwd)
(cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats -d $repo/gpurun_out/prof_fullev -o ev -- \
   python $repo/bench.py --workload eval --steps 5 --warmup 2 --full --no-cpu-baseline > "$out/prof_fullev.log" 2>&1)
python tools/prof_summary.py $(find gpurun_out/prof_fullev -name "*.db" | head -1) gpurun_out/full_eval_kernel_stats.md > /dev/null
head -16 gpurun_out/full_eval_kernel_stats.md
rm -rf gpurun_out/prof_full gpurun_out/prof_fulle gpurun_out/prof_fullev
bash tools/pmc_run.sh > gpurun_out/full_pmc.log 2>&1; tail -8 gpurun_out/full_pmc.log
