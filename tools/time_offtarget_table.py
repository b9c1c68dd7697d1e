#!/usr/bin/env python3
"""The off-targets table stage - hits -> CFD -> offtargets_*.tsv -> per-guide aggregates - on its two engines, on one index and
one guide set (offtargets.estimate_offtargets_spacers):

  objects   one OffTargetHit / BulgeHit per site, a CRISPRitz line rendered and parsed back into an Offtarget, CFD strings joined
            for compute_cfd_batch, report_line().split(), a Python sort, the joins of offtargets_table
  device    GenomeIndex.offtarget_arrays (the hits stay columns), one lexsort, hawk_offtarget_text (k_ot_text_len, the 64-bit
            scan, k_ot_text_fill), hawk_host_tsv_write, the aggregates from arrays

Shape: the panel of profiles/r05_bulges.json - a synthetic genome of 2^26 nt in rows of 4 Mb, 256 random 20-mers, NGG, max_mm = 4;
legs bdna = brna = 0, 1, 2.  Per leg both engines run in the same process, median of --repeats after --warmup; the two files must
be equal byte for byte and the returned dicts equal.  Recorded: wall of estimate_offtargets_spacers per engine (median, min, max:
the spread), the HIP-event times of the text call's stages (upload, k_ot_text_len, scan, k_ot_text_fill, download), rows and bytes.

Every leg runs in a process of its own under a time limit, and the tool stops at the first leg that fails:

    python tools/time_offtarget_table.py [--out profiles/offtarget_table.json] [--leg-timeout 900]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "crispr-hawk_amd")):
    sys.path.insert(0, p)

LEGS = (0, 1, 2)


def run_leg(args, b: int) -> dict:
    import numpy as np

    from crisprhawk_hip import scoring, synth
    from crisprhawk_hip.coordinate import Coordinate
    from crisprhawk_hip.genome import GenomeIndex
    from crisprhawk_hip.offtargets import estimate_offtargets_spacers
    from crisprhawk_hip.pam import PAM

    G, max_mm = 20, args.mm
    pam = PAM("NGG", False, True)
    pam.encode(0)
    scoring.set_cfd_tables(*synth.cfd_tables())
    rng = np.random.default_rng(2605)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    per = 1 << 22
    contigs = {f"chr{i + 1}": acgt[rng.integers(0, 4, size=per, dtype=np.uint8)] for i in range(args.genome_nt // per)}
    guides = ["".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=G)) for _ in range(args.guides)]
    idx = GenomeIndex(contigs, G, 3, piece=per, max_bulge=b)
    del contigs
    coord = Coordinate("chr1", 100, 900, 100)
    out = {"workload": f"{args.genome_nt} nt synthetic genome in rows of {per} nt (seed 2605), {len(guides)} random {G}-mers, NGG, mm <= {max_mm}",
           "bdna": b, "brna": b, "warmup": args.warmup, "repeats": args.repeats}
    files, results = {}, {}
    with tempfile.TemporaryDirectory() as td:
        for engine in ("objects", "device"):
            d = os.path.join(td, engine)
            os.makedirs(d)
            wall, stages = [], []
            for it in range(args.warmup + args.repeats):
                t0 = time.perf_counter()
                res = estimate_offtargets_spacers(guides, pam, idx, coord, max_mm, b, b, G, False, d, 0, True, engine=engine)
                dt = time.perf_counter() - t0
                if it < args.warmup:
                    continue
                wall.append(dt)
                if engine == "device":
                    stages.append(dict(idx.last_text_timing))
            (name,) = os.listdir(d)
            with open(os.path.join(d, name), "rb") as f:
                files[engine] = f.read()
            results[engine] = res
            out[engine] = {"wall_s": statistics.median(wall), "wall_s_min": min(wall), "wall_s_max": max(wall)}
            if engine == "device":
                for k in ("upload_ms", "len_ms", "scan_ms", "fill_ms", "download_ms"):
                    out[engine][k] = statistics.median(s[k] for s in stages)
                out["rows"], out["text_bytes"] = stages[-1]["n_rows"], stages[-1]["out_bytes"]
    out["file_bytes"] = len(files["device"])
    out["files_equal"] = files["objects"] == files["device"]
    out["results_equal"] = results["objects"] == results["device"]
    out["wall_speedup"] = out["objects"]["wall_s"] / out["device"]["wall_s"]
    out["spread_s"] = max(out[e]["wall_s_max"] - out[e]["wall_s_min"] for e in ("objects", "device"))
    out["device_below_objects_by_more_than_the_spread"] = out["objects"]["wall_s"] - out["device"]["wall_s"] > out["spread_s"]
    assert out["files_equal"], "the two engines' files differ"
    assert out["results_equal"], "the two engines' per-guide results differ"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-nt", type=int, default=1 << 26)
    ap.add_argument("--guides", type=int, default=256)
    ap.add_argument("--mm", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--leg", default=None, help="b: run the leg bdna = brna = b in this process and print its JSON line")
    ap.add_argument("--legs", default=",".join(str(b) for b in LEGS), help="the legs to run, comma-separated")
    ap.add_argument("--leg-timeout", type=int, default=900, help="seconds per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "offtarget_table.json"))
    args = ap.parse_args()
    if args.leg is not None:
        print(json.dumps(run_leg(args, int(args.leg))), flush=True)
        return 0
    lines = []
    for b in (int(x) for x in args.legs.split(",")):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", str(b), "--genome-nt", str(args.genome_nt), "--guides", str(args.guides),
               "--mm", str(args.mm), "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.leg_timeout)
        except subprocess.TimeoutExpired:
            print(f"leg {b}: no result within {args.leg_timeout} s - stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"leg {b}: exit status {r.returncode} - stopping", file=sys.stderr)
            return 1
        line = r.stdout.strip().splitlines()[-1]
        json.loads(line)
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
