#!/bin/bash
# rocprofv3 evidence for K1 on the headline bench workload: the K1 passes of tools/profile_r6.sh under a name without a
# round number.  A kernel trace, then every --pmc group in a run of its own (FETCH_SIZE and WRITE_SIZE do not fit one pass, and
# counters are never collected together with a trace), then the two calibration passes against a kernel with a known byte count
# (tools/calib_counters.py), then tools/summarize_prof.py.  Every step that uses the GPU runs under its own time limit and the
# steps are chained: the first one that fails, faults or runs out of time ends the script, and nothing more is started.
# Usage: bash tools/profile_k1.sh        (TAG=k1 by default; writes <OUT>/${TAG}_* and <OUT>/k1_counters.json = what goes to
# profiles/k1_counters.json, which tests/test_jit_cpu.py holds against the kernel the tree compiles.  OUT: build/profile_k1/ of the tree, which git ignores)
set -o pipefail
export TMPDIR=${TMPDIR:-/tmp}
TAG=${TAG:-k1}
R=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
OUT=${OUT:-$R/build/profile_k1}
P=$(mktemp -d "$TMPDIR/profile_k1.XXXXXX")
LIMIT=${LIMIT:-300}            # seconds per pass
mkdir -p "$OUT"
cd "$TMPDIR"
CMD="python $R/bench.py --steps 30 --warmup 5 --no-cpu-baseline --no-secondary"
# The profiler's libraries pull in the system's code-object manager before PyTorch can load the one it bundles, and
# demi_model_specialize would then compile the table with another compiler than in an untraced run: another K1, another
# demi_model_code_id.  Preloading PyTorch's comgr into the traced process keeps the traced kernel the one bench.py measures.
COMGR=$(python -c "import torch, os; print(os.path.join(os.path.dirname(torch.__file__), 'lib', 'libamd_comgr.so'))")
PRE=""
if [ -f "$COMGR" ] && [ -z "$DEMI_PROFILE_SYSTEM_COMGR" ]; then PRE="--preload $COMGR"; fi
SQ1="SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY"
SQ2="SQ_ACTIVE_INST_ANY SQ_WAIT_ANY SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INST_CYCLES_VMEM GRBM_GUI_ACTIVE SQ_THREAD_CYCLES_VALU"
timeout -k 10 $LIMIT rocprofv3 $PRE --kernel-trace --stats -d $P/prof_stats -o k1 -- $CMD > $OUT/${TAG}_prof_stats.log 2>&1 &&
timeout -k 10 $LIMIT rocprofv3 $PRE --pmc FETCH_SIZE -d $P/prof_fetch -o k1 -- $CMD > $OUT/${TAG}_prof_fetch.log 2>&1 &&
timeout -k 10 $LIMIT rocprofv3 $PRE --pmc WRITE_SIZE -d $P/prof_write -o k1 -- $CMD > $OUT/${TAG}_prof_write.log 2>&1 &&
timeout -k 10 $LIMIT rocprofv3 $PRE --pmc $SQ1 -d $P/prof_sq -o k1 -- $CMD > $OUT/${TAG}_prof_sq.log 2>&1 &&
timeout -k 10 $LIMIT rocprofv3 $PRE --pmc $SQ2 -d $P/prof_sq2 -o k1 -- $CMD > $OUT/${TAG}_prof_sq2.log 2>&1 &&
timeout -k 10 $LIMIT rocprofv3 --pmc FETCH_SIZE -d $P/calib_fetch -o c -- python $R/tools/calib_counters.py > $OUT/${TAG}_calib_fetch.log 2>&1 &&
timeout -k 10 $LIMIT rocprofv3 --pmc WRITE_SIZE -d $P/calib_write -o c -- python $R/tools/calib_counters.py > $OUT/${TAG}_calib_write.log 2>&1 &&
python $R/tools/summarize_prof.py ${TAG} $P $OUT &&
cp $OUT/${TAG}_k1_counters.json $OUT/k1_counters.json
rc=$?
rm -rf "$P"
if [ $rc -ne 0 ]; then echo "profile_k1: a pass ended with status $rc; the logs are in $OUT/${TAG}_*.log" >&2; fi
exit $rc
