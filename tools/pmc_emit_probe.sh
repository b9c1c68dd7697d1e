#!/bin/bash
# Memory-side counters of the cluster search's kernels under tools/emit_probe.py, one profiler run per regime (searches behind
# plan.rebuild_dictionary() / with the dictionary resident), counters only - no tracing in the same run:
#   tools/pmc_emit_probe.sh <tag>        -> pmc_out/pmce_<tag>/summary.json   (PMC_OUT names another directory than pmc_out)
# One pass per counter set: FETCH_SIZE and WRITE_SIZE are derived from three and two TCC counters and a channel has four, so
# asked for together the profiler refuses the set ("exceeds the capabilities of the hardware") and ends the run.  The read
# requests to the fabric are TCC_EA0_RDREQ_sum on gfx950 (TCC_EA_RDREQ_sum is the name of gfx90a and older).
# FETCH_SIZE / WRITE_SIZE are in KB; per kernel and regime the average launch, a run's first launch (the warm-up search) left out.
set -e
tag=${1:-x}
root=$(cd "$(dirname "$0")/.." && pwd)
out=${PMC_OUT:-$root/pmc_out}/pmce_$tag
mkdir -p $out
cd /tmp && export TMPDIR=/tmp
for kind in rebuilt resident; do
  i=0
  for set in "FETCH_SIZE" "WRITE_SIZE" "TCC_HIT_sum TCC_MISS_sum" "TCC_EA0_RDREQ_sum"; do
    i=$((i+1))
    timeout -k 10 120 rocprofv3 --pmc $set --output-format csv -d $out/$kind/s$i -o p -- \
      python3 $root/tools/emit_probe.py 1 --rebuild --only $kind --pairs 4 > $out/$kind.s$i.log 2>&1
  done
done
cd $root
OUT=$out python3 - <<'PY'
import collections, csv, glob, json, os
out = os.environ["OUT"]
names = ("k_cs_emit_rows", "k_cs_count", "k_cs_templates")
res = {}
for kind in ("rebuilt", "resident"):
    acc = collections.defaultdict(lambda: collections.defaultdict(dict))  # kernel -> counter -> dispatch -> value
    for f in glob.glob(f"{out}/{kind}/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            k = r["Kernel_Name"].split("(")[0].split("<")[0].replace("void ", "")
            if k.startswith(names):
                d = acc[k][r["Counter_Name"]]
                d[int(r["Dispatch_Id"])] = d.get(int(r["Dispatch_Id"]), 0.0) + float(r["Counter_Value"])
    res[kind] = {}
    for k, cs in acc.items():
        res[kind][k] = {}
        for c, d in cs.items():
            v = [d[i] for i in sorted(d)][1:]
            res[kind][k][c] = {"avg": sum(v) / max(len(v), 1), "launches": len(v)}
json.dump(res, open(f"{out}/summary.json", "w"), indent=1)
for kind, ks in res.items():
    for k, cs in ks.items():
        print(kind, k, {c: round(x["avg"], 1) for c, x in sorted(cs.items())}, "launches", max(x["launches"] for x in cs.values()))
PY
find $out -name "*counter_collection.csv" -size +5M -delete
