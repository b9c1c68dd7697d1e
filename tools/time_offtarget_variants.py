#!/usr/bin/env python3
"""The off-target scan over a variant-enriched genome (GenomeIndex.variant_arrays: hawk_offtarget_variant_scan) beside the plain
scan (GenomeIndex.scan_arrays: hawk_offtarget_scan) of the same index, same guides, same commit.

Shape: the panel of tools/time_offtarget_bulges.py - a synthetic genome of 2^26 nt in rows of 4 Mb, 256 random 20-mers, NGG,
max_mm = 4 - with seeded SNVs at one per 1000 nt and at one per 100 nt (legs).  Per leg: wall clock of add_variants (entries made
on the host, k_ov_fill), then of variant_arrays and of scan_arrays, with the kernels' time of each by its own timing block - the
variant pass stamps the device's wall clock at its stage boundaries, the plain scan records HIP events - over `--repeats` runs
after `--warmup`: median, min, max.  pairs/s of k_ov_match = variant sites x guides over its match_ms.  One JSON line per leg.

Every leg runs in a process of its own under a time limit, and the tool stops at the first leg that fails:

    python tools/time_offtarget_variants.py [--out profiles/offtarget_variants.json] [--leg-timeout 600]
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

LEGS = (1000, 100)  # one SNV per this many nt


def run_leg(args, per_nt: int) -> dict:
    import numpy as np

    from crisprhawk_hip.genome import GenomeIndex
    from crisprhawk_hip.pam import PAM

    G, max_mm = 20, args.mm
    pam = PAM("NGG", False, True)
    pam.encode(0)
    rng = np.random.default_rng(2605)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    per = 1 << 22
    codes = {f"chr{i + 1}": rng.integers(0, 4, size=per, dtype=np.uint8) for i in range(args.genome_nt // per)}
    guides = ["".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=G)) for _ in range(args.guides)]
    records = []
    for name, c in codes.items():  # one SNV per `per_nt` bases: a position in every stretch, an ALT that is not REF
        pos = np.arange(0, per - per_nt + 1, per_nt) + rng.integers(0, per_nt, size=per // per_nt)
        alt = (c[pos] + rng.integers(1, 4, size=len(pos), dtype=np.uint8)) & 3
        records += [(name, int(p), "ACGT"[r], "ACGT"[a]) for p, r, a in zip(pos.tolist(), c[pos].tolist(), alt.tolist())]
    idx = GenomeIndex({name: acgt[c] for name, c in codes.items()}, G, 3, piece=per)
    del codes
    t0 = time.perf_counter()
    stats = idx.add_variants(records)
    add_s = time.perf_counter() - t0
    out = {"workload": f"{args.genome_nt} nt synthetic genome in rows of {per} nt (seed 2605), {len(guides)} random {G}-mers, NGG, mm <= {max_mm}, "
                       f"one seeded SNV per {per_nt} nt",
           "snv_per_nt": per_nt, "variants": len(records), "applied": stats["applied"], "add_variants_wall_s": add_s,
           "warmup": args.warmup, "repeats": args.repeats}
    for name, call in (("variant", idx.variant_arrays), ("plain", idx.scan_arrays)):
        wall, tms, rows = [], [], 0
        for it in range(args.warmup + args.repeats):
            t0 = time.perf_counter()
            h, tm = call(guides, pam, False, max_mm)
            dt = time.perf_counter() - t0
            if it >= args.warmup:
                wall.append(dt)
                tms.append(dict(tm))
            rows = len(h["guide"])
        leg = {"rows": rows, "n_sites": int(tms[-1]["n_sites"]), "wall_s": statistics.median(wall), "wall_s_min": min(wall), "wall_s_max": max(wall)}
        for k in ("scan_ms", "sites_ms", "match_ms", "total_ms"):
            v = [t[k] for t in tms]
            leg[k] = statistics.median(v)
            leg[k + "_min"], leg[k + "_max"] = min(v), max(v)
        out[name] = leg
    out["k_ov_match_pairs_per_s"] = out["variant"]["n_sites"] * len(guides) / max(out["variant"]["match_ms"] * 1e-3, 1e-12)
    out["kernels_variant_over_plain"] = out["variant"]["total_ms"] / max(out["plain"]["total_ms"], 1e-12)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-nt", type=int, default=1 << 26)
    ap.add_argument("--guides", type=int, default=256)
    ap.add_argument("--mm", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--leg", default=None, help="nt per SNV: run this leg in this process and print its JSON line")
    ap.add_argument("--leg-timeout", type=int, default=600, help="seconds per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "offtarget_variants.json"))
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(run_leg(args, int(args.leg))), flush=True)
        return 0
    lines = []
    for per_nt in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", str(per_nt), "--genome-nt", str(args.genome_nt), "--guides", str(args.guides),
               "--mm", str(args.mm), "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.leg_timeout)
        except subprocess.TimeoutExpired:
            print(f"leg 1 / {per_nt}: no result within {args.leg_timeout} s - stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"leg 1 / {per_nt}: exit status {r.returncode} - stopping", file=sys.stderr)
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
