#!/bin/bash
# Instruction-issue profile of the search and network kernels at the bench layout (C2, four
# game groups): one kernel trace, then counter passes in runs of their own (instruction
# counts, wave / issue / wait cycles, instruction-cache requests), per-kernel averages.
#   bash tools/search_insts_pmc.sh TAG [LIBRARY]   ->  $PROF_OUT/prof_TAG/summary.txt (PROF_OUT: default tools/_build)
# LIBRARY: another build of libkatacoffee.so (KATACOFFEE_LIB), e.g. the parent's for a before/after pair.
set -u
tag=$1
[ $# -ge 2 ] && export KATACOFFEE_LIB=$2
cd "$(dirname "$0")/.."
out=${PROF_OUT:-tools/_build}/prof_$tag
mkdir -p $out
export TMPDIR=/tmp
BENCH="python bench.py --gpus 1 --steps 2 --warmup 1 --rounds-per-step 300"
timeout -k 10 120 rocprofv3 --list-avail > $out/list_avail.txt 2>&1 || { echo "list-avail failed"; exit 1; }
# the instruction-fetch / instruction-cache counters this device offers
grep -o -E '\b[A-Z0-9_]*(ICACHE|IFETCH)[A-Z0-9_]*\b' $out/list_avail.txt | sort -u > $out/icache_counters.txt
echo "instruction-cache counters offered: $(tr '\n' ' ' < $out/icache_counters.txt)"
timeout -k 10 240 rocprofv3 --kernel-trace --stats -d $out/trace -o trace --output-format csv -- $BENCH > $out/trace.log 2>&1 ||
  { echo "trace failed"; tail -5 $out/trace.log; exit 1; }
ic=$(grep -E '^SQC_ICACHE_(REQ|HITS|MISSES|MISSES_DUPLICATE)$' $out/icache_counters.txt | head -4 | tr '\n' ' ')
i=0
for set in "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVES" "SQ_INSTS_VMEM_RD SQ_WAVE_CYCLES SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU" \
           "SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_BUSY_CYCLES SQ_INSTS_SMEM" "$ic"; do
  i=$((i+1))
  [ -z "$set" ] && continue
  timeout -k 10 240 rocprofv3 --pmc $set -d $out/p$i -o p --output-format csv -- $BENCH > $out/p$i.log 2>&1 ||
    { echo "pass $i ($set) failed"; tail -5 $out/p$i.log; exit 1; }
done
python - $out > $out/summary.txt <<'PY'
import collections, csv, glob, sys
out = sys.argv[1]
TAGS = ("kBackupSelect", "kSelect", "kBackup", "kNNForward", "kCompact", "kCommit", "kRows")
for f in glob.glob(out + "/trace/**/*kernel_stats.csv", recursive=True):
    print("== kernel trace (calls, average ns, share)")
    for r in csv.DictReader(open(f)):
        print("  %-58s %7s %12.0f %7s" % (r["Name"][:58], r["Calls"], float(r["AverageNs"]), r["Percentage"]))
agg = collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob(out + "/p*/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        t = next((t for t in TAGS if t in r["Kernel_Name"]), None)
        if t:
            agg[t][r["Counter_Name"]].append(float(r["Counter_Value"]))
print("== counters, mean per dispatch (dispatches)")
for t in TAGS:
    if t in agg:
        print(t)
        for c, v in sorted(agg[t].items()):
            print("  %-28s %16.1f  (%d)" % (c, sum(v) / len(v), len(v)))
        m = {c: sum(v) / len(v) for c, v in agg[t].items()}
        if "SQ_WAVE_CYCLES" in m and m["SQ_WAVE_CYCLES"] > 0:
            print("  share of wave cycles: issuing %.3f (VALU %.3f), waiting %.3f" % (
                m.get("SQ_ACTIVE_INST_ANY", 0) / m["SQ_WAVE_CYCLES"], m.get("SQ_ACTIVE_INST_VALU", 0) / m["SQ_WAVE_CYCLES"],
                m.get("SQ_WAIT_ANY", 0) / m["SQ_WAVE_CYCLES"]))
        if m.get("SQ_WAVES", 0) > 0:
            print("  instructions per wave: VALU %.0f SALU %.0f LDS %.0f" % (
                m.get("SQ_INSTS_VALU", 0) / m["SQ_WAVES"], m.get("SQ_INSTS_SALU", 0) / m["SQ_WAVES"],
                m.get("SQ_INSTS_LDS", 0) / m["SQ_WAVES"]))
PY
cat $out/summary.txt
# the per-dispatch tables are large: the summary is what is kept
find $out -name '*_kernel_trace.csv' -delete
find $out -name '*_counter_collection.csv' -delete
