#!/usr/bin/env python3
"""Bulged off-target sites: the device engine (k_ot_bulge picks the placement per (site, guide) pair) against the derived-guide
engine it replaces on the product route, on one index and one guide set.

  derived   GenomeIndex.scan_bulges(engine="derived"): every bulged variant of every guide through hawk_offtarget_scan, the hits
            downloaded, the best placement per (guide, site, strand, type, size) picked with numpy
  device    GenomeIndex.scan_bulges(engine="device"): one hawk_offtarget_bulges per (type, size)

Shape: a synthetic genome of 2^26 nt in rows of 4 Mb, 256 random 20-mers, NGG, max_mm = 4; legs (bdna, brna) = (1, 1) and (2, 2).
Per leg and engine: wall clock of scan_bulges and the HIP-event time of its kernels (hawk_ot_timing.total_ms summed over the
calls; for the device engine also match_ms = k_ot_bulge alone); the rows of the two engines must be equal.  One JSON line per
leg with the pairs/s of k_ot_bulge (PAM sites x guides, summed over the leg's calls, over its match_ms).

Every leg runs in a process of its own under a time limit, and the tool stops at the first leg that fails:

    python tools/time_offtarget_bulges.py [--out profiles/r05_bulges.json] [--leg-timeout 900]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "crispr-hawk_amd")):
    sys.path.insert(0, p)

LEGS = ((1, 1), (2, 2))


def run_leg(args, bdna: int, brna: int) -> dict:
    import numpy as np

    from crisprhawk_hip.genome import GenomeIndex
    from crisprhawk_hip.pam import PAM

    G, max_mm = 20, args.mm
    pam = PAM("NGG", False, True)
    pam.encode(0)
    rng = np.random.default_rng(2605)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    per = 1 << 22
    contigs = {f"chr{i + 1}": acgt[rng.integers(0, 4, size=per, dtype=np.uint8)] for i in range(args.genome_nt // per)}
    guides = ["".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=G)) for _ in range(args.guides)]
    idx = GenomeIndex(contigs, G, 3, piece=per, max_bulge=bdna)
    del contigs
    kernel_ms = []
    inner = idx.scan_arrays

    def scan_arrays(*a, **kw):  # the derived engine's scans: their kernels' time
        h, tm = inner(*a, **kw)
        kernel_ms.append(tm["total_ms"])
        return h, tm

    idx.scan_arrays = scan_arrays
    out = {"workload": f"{args.genome_nt} nt synthetic genome in rows of {per} nt (seed 2605), {len(guides)} random {G}-mers, NGG, mm <= {max_mm}",
           "bdna": bdna, "brna": brna, "warmup": args.warmup, "repeats": args.repeats}
    rows = {}
    for engine in ("derived", "device"):
        wall, kern, match, pairs = [], [], [], 0
        for it in range(args.warmup + args.repeats):
            del kernel_ms[:]
            t0 = time.perf_counter()
            res = idx.scan_bulges(guides, pam, False, max_mm, bdna, brna, engine=engine)
            dt = time.perf_counter() - t0
            if it < args.warmup:
                continue
            wall.append(dt)
            if engine == "device":
                kern.append(sum(t["total_ms"] for t in idx.last_bulge_timing))
                match.append(sum(t["match_ms"] for t in idx.last_bulge_timing))
                pairs = sum(int(t["n_sites"]) * len(guides) for t in idx.last_bulge_timing)
            else:
                kern.append(sum(kernel_ms))
        rows[engine] = res
        out[engine] = {"rows": len(res), "wall_s": statistics.median(wall), "wall_s_min": min(wall), "wall_s_max": max(wall),
                       "kernels_ms": statistics.median(kern)}
        if engine == "device":
            out[engine]["k_ot_bulge_ms"] = statistics.median(match)
            out["pairs"] = pairs
            out["k_ot_bulge_pairs_per_s"] = pairs / (statistics.median(match) * 1e-3)
    out["rows_equal"] = rows["derived"] == rows["device"]
    out["wall_speedup"] = out["derived"]["wall_s"] / out["device"]["wall_s"]
    out["kernels_speedup"] = out["derived"]["kernels_ms"] / out["device"]["kernels_ms"]
    assert out["rows_equal"], "the two engines' rows differ"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-nt", type=int, default=1 << 26)
    ap.add_argument("--guides", type=int, default=256)
    ap.add_argument("--mm", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--leg", default=None, help="bdna,brna: run this leg in this process and print its JSON line")
    ap.add_argument("--leg-timeout", type=int, default=900, help="seconds per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05_bulges.json"))
    args = ap.parse_args()
    if args.leg:
        bdna, brna = (int(x) for x in args.leg.split(","))
        print(json.dumps(run_leg(args, bdna, brna)), flush=True)
        return 0
    lines = []
    for bdna, brna in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", f"{bdna},{brna}", "--genome-nt", str(args.genome_nt), "--guides", str(args.guides),
               "--mm", str(args.mm), "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.leg_timeout)
        except subprocess.TimeoutExpired:
            print(f"leg ({bdna}, {brna}): no result within {args.leg_timeout} s - stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"leg ({bdna}, {brna}): exit status {r.returncode} - stopping", file=sys.stderr)
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
