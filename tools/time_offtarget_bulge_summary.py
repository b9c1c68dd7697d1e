#!/usr/bin/env python3
"""The guide report's two off-target columns with DNA / RNA bulges on their two routes, on one index and one guide set:

  table     offtargets.estimate_offtargets_spacers(engine="device"): every row listed (hawk_offtarget_scan, one
            hawk_offtarget_bulges per (type, size)), downloaded, uploaded again for hawk_offtarget_text, written as
            offtargets_*.tsv, counted and summed on the host
  summary   offtargets.specificity_by_spacer(bdna, brna): hawk_offtarget_summary plus one hawk_offtarget_bulge_summary per
            (type, size) - every row counted and its CFD summed inside the kernel that finds it, no row listed, no file

Shape: the panel of profiles/r05_bulges.json / offtarget_table.json - a synthetic genome of 2^26 nt in rows of 4 Mb, 256 random
20-mers, NGG, max_mm = 4; legs bdna = brna = 1, 2.  Per leg both routes run in the same process, median of --repeats after --warmup.
The two routes' counts must be equal; the number of `cfd` texts that differ is recorded (the table route sums floats in row order,
the summary integers).  Recorded: wall of either route (median, min, max), the kernel times of the summary's calls (HIP events:
PAM scan, site records, match / bulge kernel) and their sum, the part of the summary's wall that is not kernel time, rows.

Every leg runs in a process of its own under a time limit, and the tool stops at the first leg that fails:

    python tools/time_offtarget_bulge_summary.py [--out profiles/offtarget_bulge_summary.json] [--leg-timeout 900]
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

LEGS = (1, 2)


def run_leg(args, b: int) -> dict:
    import numpy as np

    from crisprhawk_hip import scoring, synth
    from crisprhawk_hip.coordinate import Coordinate
    from crisprhawk_hip.genome import GenomeIndex
    from crisprhawk_hip.offtargets import estimate_offtargets_spacers, specificity_by_spacer
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
    results = {}
    with tempfile.TemporaryDirectory() as td:
        for route in ("table", "summary"):
            wall, kern = [], []
            for it in range(args.warmup + args.repeats):
                t0 = time.perf_counter()
                if route == "table":
                    res = estimate_offtargets_spacers(guides, pam, idx, coord, max_mm, b, b, G, False, td, 0, True, engine="device")
                else:
                    res = specificity_by_spacer(guides, pam, idx, max_mm, G, False, True, b, b)
                dt = time.perf_counter() - t0
                if it < args.warmup:
                    continue
                wall.append(dt)
                calls = [idx.last_timing] + list(idx.last_bulge_timing)
                kern.append({"scan_ms": sum(c["scan_ms"] for c in calls), "sites_ms": sum(c["sites_ms"] for c in calls),
                             "match_ms": sum(c["match_ms"] for c in calls)})
            results[route] = res
            out[route] = {"wall_s": statistics.median(wall), "wall_s_min": min(wall), "wall_s_max": max(wall)}
            if route == "summary":  # the table route's last_timing is its last bulge call's alone
                for k in ("scan_ms", "sites_ms", "match_ms"):
                    out[route][k] = statistics.median(x[k] for x in kern)
                out[route]["kernels_ms"] = sum(out[route][k] for k in ("scan_ms", "sites_ms", "match_ms"))
                out[route]["calls"] = len(calls)
                out[route]["wall_outside_kernels_ms"] = out[route]["wall_s"] * 1e3 - out[route]["kernels_ms"]
    out["rows"] = sum(v[0] for v in results["table"].values())
    out["counts_equal"] = {k: v[0] for k, v in results["table"].items()} == {k: v[0] for k, v in results["summary"].items()}
    out["cfd_texts_differ"] = sum(results["table"][k][1] != results["summary"][k][1] for k in results["table"])
    out["cfd_max_abs_diff"] = max(abs(float(results["table"][k][1]) - float(results["summary"][k][1])) for k in results["table"])
    out["guides"] = len(results["table"])
    out["wall_speedup"] = out["table"]["wall_s"] / out["summary"]["wall_s"]
    print(f"bdna = brna = {b}: {out['rows']} rows, cfd texts that differ: {out['cfd_texts_differ']} of {out['guides']}", file=sys.stderr)
    assert out["counts_equal"], "the two routes' counts differ"
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "offtarget_bulge_summary.json"))
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
