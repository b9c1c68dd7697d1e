#!/usr/bin/env python3
"""The off-target summary against the per-site route it replaces, on one index and one guide set (C5 geometry: synthetic
genome of seed 1006, guides cut out of it with seed 1005 - what `bench.py --config c5` builds).

  per-site route   offtargets.search (GenomeIndex.scan + one CRISPRitz line per hit) -> Offtarget objects -> compute_cfd_batch
                   (SpCas9 / xCas9 PAMs) -> offtargets_by_spacer
  summary route    offtargets.specificity_by_spacer (GenomeIndex.summary: the hits are summed inside the match kernel)

Per route: wall clock (median, min, max of `--repeats` runs after `--warmup`), hawk_ot_timing of every run; the match kernel's
time with the list sink (scan) and with the summing sink (summary) side by side.  One process on the card.

    python tools/time_offtarget_summary.py [--full] [--cas9] [--out profiles/offtarget_summary.json]

The default size (10^8 nt, 1000 guides) fits the test machine; --full is bench.py's C5 (3.1 x 10^9 nt, 10^4 guides).  C5 is
TTTV / 23 / right, for which no CFD exists; --cas9 runs NGG / 20 with the synthetic CFD tables so that the per-hit CFD is timed."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "crispr-hawk_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-nt", type=int, default=100_000_000)
    ap.add_argument("--contigs", type=int, default=24)
    ap.add_argument("--guides", type=int, default=1000)
    ap.add_argument("--full", action="store_true", help="3.1e9 nt, 1e4 guides")
    ap.add_argument("--cas9", action="store_true", help="NGG / 20 nt with synth.cfd_tables() instead of TTTV / 23 nt / right")
    ap.add_argument("--mm", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "offtarget_summary.json"))
    args = ap.parse_args()
    if args.full:
        args.genome_nt, args.guides = 3_100_000_000, 10_000
    from crisprhawk_hip import offtargets as ot, scoring, synth
    from crisprhawk_hip.genome import GenomeIndex
    from crisprhawk_hip.pam import PAM, SPCAS9, XCAS9

    pam_s, G, right = ("NGG", 20, False) if args.cas9 else ("TTTV", 23, True)
    pam = PAM(pam_s, right, True)
    pam.encode(0)
    scoring.set_cfd_tables(*synth.cfd_tables())
    rng = np.random.default_rng(1006)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    per = args.genome_nt // args.contigs
    contigs = {f"chr{i + 1}": acgt[rng.integers(0, 4, size=per, dtype=np.uint8)] for i in range(args.contigs)}
    names, grng, guides = list(contigs), np.random.default_rng(1005), []
    while len(guides) < args.guides:
        c = contigs[names[int(grng.integers(0, len(names)))]]
        p = int(grng.integers(0, per - 64))
        guides.append(c[p:p + G].tobytes().decode())
    guides = sorted(set(guides))
    idx = GenomeIndex(contigs, G, len(pam))
    del contigs
    cas9 = pam.cas_system in (SPCAS9, XCAS9)

    def per_site():
        lines = ot.search(idx, guides, pam, right, args.mm, 0, True)
        tm = dict(idx.last_timing)
        ots = ot._read_offtargets(lines, pam, right, True)
        if cas9:
            ots = ot._compute_cfd_score(ots, 0, True)
        return ot.offtargets_by_spacer(ots, guides), tm, len(lines)

    def summary():
        res = ot.specificity_by_spacer(guides, pam, idx, args.mm, G, right, True)
        return res, dict(idx.last_timing), sum(v[0] for v in res.values())

    out = {"workload": f"{args.genome_nt} nt synthetic genome in {args.contigs} contigs (seed 1006), {len(guides)} guides, {pam_s} / {G} nt "
                       f"right={right}, mm <= {args.mm}", "warmup": args.warmup, "repeats": args.repeats}
    results = {}
    for name, fn in (("per_site", per_site), ("summary", summary)):
        for _ in range(args.warmup):
            fn()
        wall, tms, n = [], [], 0
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            res, tm, n = fn()
            wall.append(time.perf_counter() - t0)
            tms.append(tm)
        results[name] = res
        out[name] = {"hits": int(n), "wall_s": spread(wall), "match_ms": spread([t["match_ms"] for t in tms]),
                     "kernels_total_ms": spread([t["total_ms"] for t in tms]), "scan_ms": spread([t["scan_ms"] for t in tms]),
                     "sites_ms": spread([t["sites_ms"] for t in tms]), "pam_sites": int(tms[-1]["n_sites"])}
    a, b = results["per_site"], results["summary"]
    out["counts_equal"] = {k: v[0] for k, v in a.items()} == {k: v[0] for k, v in b.items()}
    out["cfd_texts_differing"] = sum(a[k][1] != b[k][1] for k in a)
    out["cfd_max_abs_diff"] = max(abs(float(a[k][1]) - float(b[k][1])) for k in a)
    out["match_ms_list_sink_vs_sum_sink"] = [out["per_site"]["match_ms"]["median"], out["summary"]["match_ms"]["median"]]
    out["wall_speedup_median"] = out["per_site"]["wall_s"]["median"] / out["summary"]["wall_s"]["median"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
