#!/usr/bin/env python3
"""Time pipeline.search_files on an unphased population VCF, files to TSV, with the report made from Guide objects
(unphased_report="objects": search_guides._guides_from_resolved, scoring.cfdon_score, reports.report_from_guides, pandas) against
the report groups made on the device (unphased_report="groups": hawk_resolve_groups, reports.group_columns, write_report_tsv), and
write profiles/unphased_report.json.

    python tools/time_unphased_report.py [--size 200000] [--runs 3] [--objects-limit 150]

The synthetic region of tools/time_resolve_unphased.py: --size nt, 10 unphased samples, SNVs only, NGG / 20, CFD tables on.  One
warm-up run of the groups route (library, context, first launches), then --runs runs of either route: wall seconds of search_files
(reading the files, building the haplotypes on the host, search, resolution, report, TSV), for the groups route the HIP-event time
of every stage of hawk_resolve_groups, n_kept / n_groups / n_members and search_files' own stage clock of the last run - and whether
the two TSVs are byte-equal.  If the first run of the object route takes longer than --objects-limit seconds it stays the only one;
the number of runs done is recorded.  Prints the README table row."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "crispr-hawk_amd"))
OUT = os.path.join(ROOT, "profiles", "unphased_report.json")


def write_inputs(size: int, d: str):
    from crisprhawk_hip import readers, synth
    reg = synth.make_region(8101, "chrT", size + 2400, 1000, 1000 + size)
    synth.add_phased_variants(reg, 8102, size // 15, 10, frac_snv=1.0, frac_del=0.0, max_indel=1, af_min=0.3, af_max=0.6)
    fa, bed, vcf = os.path.join(d, "g.fa"), os.path.join(d, "r.bed"), os.path.join(d, "v.vcf")
    readers.write_fasta(fa, reg.contig, reg.contig_seq, 80)
    with open(bed, "w") as f:
        f.write(f"{reg.contig}\t{reg.bed_start}\t{reg.bed_stop}\n")
    rows = []
    for v in reg.variants:
        fields = reg.vcf_fields(v)
        fields[9:] = [g.replace("|", "/") for g in fields[9:]]
        rows.append(fields)
    readers.write_vcf(vcf, reg.contig, reg.samples, rows, False)
    return fa, bed, vcf, len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=200_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--objects-limit", type=float, default=150.0)
    args = ap.parse_args()
    from crisprhawk_hip import pipeline, synth
    from crisprhawk_hip.hapset import GuideTable
    tables = synth.cfd_tables()
    stages = []
    real = GuideTable.resolve_unphased_groups

    def spy(tab, *a, **k):
        g = real(tab, *a, **k)
        stages.append(dict(g.timing))
        return g
    GuideTable.resolve_unphased_groups = spy
    with tempfile.TemporaryDirectory() as d:
        fa, bed, vcf, n_rec = write_inputs(args.size, d)
        print(f"inputs written: {n_rec} records", flush=True)

        laps = {}

        def run(route, tag):
            laps.clear()
            t0 = time.perf_counter()
            (path,) = pipeline.search_files(fa, bed, [vcf], "NGG", 20, False, os.path.join(d, tag), cfd_tables=tables, debug=True,
                                            unphased_report=route, timings=laps).values()
            return time.perf_counter() - t0, path
        t, _ = run("groups", "warm")
        print(f"warm-up (groups) {t:.2f} s", flush=True)
        stages.clear()
        obj, grp, obj_path, grp_path = [], [], None, None
        for i in range(args.runs):
            t, obj_path = run("objects", "objects")
            obj.append(t)
            print(f"objects {t:.2f} s", flush=True)
            if i == 0 and t > args.objects_limit:
                break
        for _ in range(args.runs):
            t, grp_path = run("groups", "groups")
            grp.append(t)
            print(f"groups {t:.2f} s  {stages[-1]}  {laps}", flush=True)
        groups_laps = dict(laps)
        a, b = open(obj_path, "rb").read(), open(grp_path, "rb").read()
        equal = a == b
        rows = b.count(b"\n") - 1
    mm = lambda v: {"min": min(v), "max": max(v)}
    keys = ("fill_ms", "keys_ms", "sort_ms", "heads_ms", "emit_ms", "total_ms")
    res = {
        "what": "pipeline.search_files, files to TSV, on one synthetic unphased region: 10 samples, SNVs only, NGG / 20, CFD tables on; wall "
                "seconds per route, HIP-event ms per stage of hawk_resolve_groups",
        "size_nt": args.size, "records": n_rec, "runs_objects": len(obj), "runs_groups": len(grp), "objects_limit_s": args.objects_limit,
        "n_kept": stages[0]["n_kept"], "n_groups": stages[0]["n_groups"], "n_members": stages[0]["n_members"], "fill_batches": stages[0]["n_batches"],
        "report_rows": rows, "objects_wall_s": mm(obj), "groups_wall_s": mm(grp), "stage_ms": {k: mm([s[k] for s in stages]) for k in keys},
        "groups_wall_stages_s_last_run": groups_laps, "tsv_byte_equal": bool(equal), "tsv_bytes": len(b),
    }
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if os.path.exists(OUT):  # the figures of the commit before the builder's site-list mapping stay beside the new ones
        res.update({k: v for k, v in json.load(open(OUT)).items() if k == "parent_commit"})
    json.dump(res, open(OUT, "w"), indent=1)
    sm = res["stage_ms"]
    print(json.dumps(res))
    print(f"| unphased report from groups made on the device (`hawk_resolve_groups`: `k_ug_keys`, sort passes, `k_ug_heads`, `k_ug_emit`; "
          f"`tools/time_unphased_report.py`, `profiles/unphased_report.json`, min-max) | {args.size} nt, 10 unphased samples, NGG / 20, CFD tables: "
          f"{res['n_kept']} kept guides -> {res['n_groups']} groups, {res['n_members']} members.  `search_files` wall, files to TSV: object route "
          f"{min(obj):.2f}-{max(obj):.2f} s ({len(obj)} runs), groups route {min(grp):.2f}-{max(grp):.2f} s ({len(grp)} runs); stages: fill "
          f"{sm['fill_ms']['min']:.3f}-{sm['fill_ms']['max']:.3f} ms, keys {sm['keys_ms']['min']:.3f}-{sm['keys_ms']['max']:.3f}, sort "
          f"{sm['sort_ms']['min']:.3f}-{sm['sort_ms']['max']:.3f}, heads + scans {sm['heads_ms']['min']:.3f}-{sm['heads_ms']['max']:.3f}, emit "
          f"{sm['emit_ms']['min']:.3f}-{sm['emit_ms']['max']:.3f}; TSVs {'byte-equal' if equal else 'DIFFER'} |")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
