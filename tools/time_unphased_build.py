#!/usr/bin/env python3
"""Time pipeline.search_files on an unphased population VCF, files to TSV, with the haplotypes built on the host
(unphased_haplotypes="host": haplotypes.add_variants_unphased, one region-long string per carrier, hawk_hapset_pack_ascii) against
the whole-region rows built on the device (unphased_haplotypes="device": workload.expand_unphased_from_vcf - hawk_gt_parse_unphased,
hawk_ubuild_lists, hawk_ubuild_signatures, hawk_ubuild_fill), and write profiles/unphased_build.json.

    python tools/time_unphased_build.py [--size 200000] [--runs 3] [--panel-samples 256] [--host-limit 120]

Point 1: the region and files of tools/time_unphased_report.py (--size nt, 10 unphased samples, SNVs only, NGG / 20, CFD tables
on): one warm-up run, then --runs runs under each builder in this process - wall seconds of search_files, its stage clock (the
builder's lap is named after the builder), the kernels' HIP-event ms of the device builder, and whether the reports are
byte-equal.  Point 2: the same region with --panel-samples samples, where the host builder's cost (samples x region length) shows:
the host builder once, the device builder --runs times; if the host run takes longer than --host-limit seconds the point is
repeated with half the samples and the file says which.  Prints the README table row."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "crispr-hawk_amd"))
OUT = os.path.join(ROOT, "profiles", "unphased_build.json")


def write_inputs(size: int, n_samples: int, d: str):
    from crisprhawk_hip import readers, synth
    reg = synth.make_region(8101, "chrT", size + 2400, 1000, 1000 + size)
    synth.add_phased_variants(reg, 8102, size // 15, n_samples, frac_snv=1.0, frac_del=0.0, max_indel=1, af_min=0.3, af_max=0.6)
    os.makedirs(d, exist_ok=True)
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
    ap.add_argument("--panel-samples", type=int, default=256)
    ap.add_argument("--host-limit", type=float, default=120.0)
    args = ap.parse_args()
    from crisprhawk_hip import pipeline, synth, workload
    tables = synth.cfd_tables()
    kernel_ms, rows_built = [], []
    real = workload.expand_unphased_from_vcf

    def spy(*a, **k):
        out = real(*a, **k)
        kernel_ms.append(dict(out[4]))
        rows_built.append(int(out[0].n_hap))
        return out
    workload.expand_unphased_from_vcf = spy
    mm = lambda v: {"min": min(v), "max": max(v)}

    def point(d, n_samples, host_runs, device_runs, warm):
        fa, bed, vcf, n_rec = write_inputs(args.size, n_samples, d)
        print(f"inputs written: {n_rec} records, {n_samples} samples", flush=True)

        def run(builder, tag):
            laps = {}
            t0 = time.perf_counter()
            (path,) = pipeline.search_files(fa, bed, [vcf], "NGG", 20, False, os.path.join(d, tag), cfd_tables=tables, debug=True,
                                            unphased_haplotypes=builder, timings=laps).values()
            return time.perf_counter() - t0, path, laps
        if warm:
            t, _, _ = run("device", "warm")
            print(f"warm-up (device) {t:.2f} s", flush=True)
        kernel_ms.clear()
        rows_built.clear()
        res = {"samples": n_samples, "records": n_rec, "size_nt": args.size}
        walls, laps_all, paths = {"host": [], "device": []}, {"host": [], "device": []}, {}
        for builder, n in (("host", host_runs), ("device", device_runs)):
            for _ in range(n):
                t, paths[builder], laps = run(builder, builder)
                walls[builder].append(t)
                laps_all[builder].append(laps)
                print(f"{builder} {t:.2f} s  {laps}", flush=True)
        lap_name = {"host": pipeline.HOST_BUILT_LAP, "device": pipeline.DEVICE_BUILT_LAP}
        for b in ("host", "device"):
            res[f"{b}_runs"] = len(walls[b])
            res[f"{b}_wall_s"] = mm(walls[b])
            res[f"{b}_builder_lap_s"] = mm([l[lap_name[b]] for l in laps_all[b]])
            res[f"{b}_stage_laps_s_last_run"] = laps_all[b][-1]
        res["device_route_taken_every_run"] = len(kernel_ms) == device_runs
        res["device_kernel_ms"] = {k: mm([m[k] for m in kernel_ms]) for k in ("parse", "lists", "signatures", "fill")} if kernel_ms else None
        res["rows_in_the_set"] = rows_built[0] if rows_built else None
        a, b = open(paths["host"], "rb").read(), open(paths["device"], "rb").read()
        res["tsv_byte_equal"] = bool(a == b)
        res["report_rows"] = b.count(b"\n") - 1
        return res
    with tempfile.TemporaryDirectory() as d:
        small = point(os.path.join(d, "p1"), 10, args.runs, args.runs, True)
        n = args.panel_samples
        large = point(os.path.join(d, "p2"), n, 1, args.runs, False)
        reduced = None
        if large["host_wall_s"]["max"] > args.host_limit and n > 32:
            reduced = n // 2
            large = point(os.path.join(d, "p3"), reduced, 1, args.runs, False)
    res = {
        "what": "pipeline.search_files, files to TSV, on one synthetic unphased region (SNVs only, NGG / 20, CFD tables on) under "
                "unphased_haplotypes='host' and 'device', both in one process run on one machine: wall seconds, the builder's lap of "
                "search_files' stage clock, HIP-event ms of the device builder's kernels; min-max",
        "runs": args.runs, "host_limit_s": args.host_limit, "point_10_samples": small, "point_panel": large,
        "panel_samples_asked": args.panel_samples, "panel_samples_reduced_to": reduced,
        "default_builder": "host",
    }
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(res, open(OUT, "w"), indent=1)
    print(json.dumps(res))
    for name, p in (("10 samples", small), (f"{large['samples']} samples", large)):
        k = p["device_kernel_ms"] or {}
        km = ", ".join(f"{s} {k[s]['min']:.3f}-{k[s]['max']:.3f}" for s in k)
        print(f"| unphased haplotypes built on the device ({name}; `tools/time_unphased_build.py`, `profiles/unphased_build.json`, min-max) | "
              f"{p['size_nt']} nt, {p['records']} records, {p['rows_in_the_set']} rows: builder lap host {p['host_builder_lap_s']['min']:.3f}-"
              f"{p['host_builder_lap_s']['max']:.3f} s ({p['host_runs']} runs), device {p['device_builder_lap_s']['min']:.3f}-"
              f"{p['device_builder_lap_s']['max']:.3f} s ({p['device_runs']} runs); `search_files` wall host {p['host_wall_s']['min']:.2f}-"
              f"{p['host_wall_s']['max']:.2f} s, device {p['device_wall_s']['min']:.2f}-{p['device_wall_s']['max']:.2f} s; kernels (ms): {km}; "
              f"TSVs {'byte-equal' if p['tsv_byte_equal'] else 'DIFFER'} |")
    return 0 if small["tsv_byte_equal"] and large["tsv_byte_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
