#!/usr/bin/env python3
"""Time pipeline.search_files(unphased_haplotypes="device") on an unphased population VCF WITH indels, files to TSV, with the indel
windows built on the host (unphased_indel_windows="host": a VariantRecord per line involved, haplotypes.unphased_indel_windows, one
Haplotype and one string per (indel, carrier), hawk_hapset_pack_ascii_rows - the route before the option existed) against the
windows built on the device (unphased_indel_windows="device": hawk_uwin_instances, hawk_uwin_signatures, hawk_uwin_group,
hawk_uwin_fill), and write profiles/unphased_windows.json.

    python tools/time_unphased_windows.py [--size 200000] [--runs 3] [--panel-samples 256]

The region is that of tools/time_unphased_build.py (--size nt, NGG / 20, CFD tables on) generated with indels:
synth.add_phased_variants with frac_snv=0.8, frac_del=0.1 (so a tenth insertions), indels of up to 8 bases.  Two points, 10 and
--panel-samples samples; at each, one warm-up run, then --runs runs under each window mode in this one process: wall seconds of
search_files, the builder's lap of its stage clock, the kernels' milliseconds by the device clock stamps of the hawk_uwin_* calls
(and the HIP-event ms of the SNV-row calls beside them), row and instance counts, and whether the reports are byte-equal.  Prints
the README table row."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "crispr-hawk_amd"))
OUT = os.path.join(ROOT, "profiles", "unphased_windows.json")
MIX = dict(frac_snv=0.8, frac_del=0.1, max_indel=8, af_min=0.3, af_max=0.6)


def write_inputs(size: int, n_samples: int, d: str):
    from crisprhawk_hip import readers, synth
    reg = synth.make_region(8101, "chrT", size + 2400, 1000, 1000 + size)
    synth.add_phased_variants(reg, 8102, size // 15, n_samples, **MIX)
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
    n_ins = sum(len(f[4]) > len(f[3]) for f in rows)
    n_del = sum(len(f[4]) < len(f[3]) for f in rows)
    return fa, bed, vcf, dict(records=len(rows), insertions=n_ins, deletions=n_del, snvs=len(rows) - n_ins - n_del)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=200_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--panel-samples", type=int, default=256)
    ap.add_argument("--out", default=OUT, help="where the JSON goes (written after each point)")
    args = ap.parse_args()
    from crisprhawk_hip import pipeline, synth, workload
    tables = synth.cfd_tables()
    seen = []
    real_build, real_rows = workload.expand_unphased_from_vcf, workload.unphased_window_rows

    def build_spy(*a, **k):
        t0 = time.perf_counter()
        out = real_build(*a, **k)
        seen.append(dict(mode=k.get("indel_windows", "host"), ms=dict(out[4]), rows=int(out[0].n_hap), host_windows=len(out[3]),
                         call_s=time.perf_counter() - t0))
        return out
    counts = {}

    def rows_spy(wt, inst_off, *a, **k):
        out = real_rows(wt, inst_off, *a, **k)
        counts.update(indels=len(wt), instances=int(inst_off[-1]), window_rows=len(out[0]))
        return out
    workload.expand_unphased_from_vcf = build_spy
    workload.unphased_window_rows = rows_spy
    mm = lambda v: {"min": min(v), "max": max(v)}

    def point(d, n_samples):
        fa, bed, vcf, n_rec = write_inputs(args.size, n_samples, d)
        print(f"inputs written: {n_rec}, {n_samples} samples", flush=True)

        def run(mode, tag):
            laps = {}
            t0 = time.perf_counter()
            (path,) = pipeline.search_files(fa, bed, [vcf], "NGG", 20, False, os.path.join(d, tag), cfd_tables=tables, debug=True,
                                            unphased_haplotypes="device", unphased_indel_windows=mode, timings=laps).values()
            return time.perf_counter() - t0, path, laps
        t, _, _ = run("device", "warm")
        print(f"warm-up (device windows) {t:.2f} s", flush=True)
        seen.clear()
        res = {"samples": n_samples, "size_nt": args.size, **n_rec}
        paths = {}
        for mode in ("host", "device"):
            walls, laps_all = [], []
            for _ in range(args.runs):
                t, paths[mode], laps = run(mode, mode)
                walls.append(t)
                laps_all.append(laps)
                print(f"{mode} windows {t:.2f} s  {laps}", flush=True)
            mine = [s for s in seen if s["mode"] == mode]
            res[f"{mode}_windows"] = {
                "runs": len(walls), "wall_s": mm(walls), "builder_lap_s": mm([l[pipeline.DEVICE_BUILT_LAP] for l in laps_all]),
                "builder_call_s": mm([s["call_s"] for s in mine]), "route_taken_every_run": len(mine) == args.runs,
                "rows_in_the_set": mine[0]["rows"] if mine else None,
                "kernel_ms": {k: mm([s["ms"][k] for s in mine]) for k in (mine[0]["ms"] if mine else {})},
                "stage_laps_s_last_run": laps_all[-1]}
            if mode == "host" and mine:
                res["window_rows_host_built"] = mine[0]["host_windows"]
        res.update(counts)
        a, b = open(paths["host"], "rb").read(), open(paths["device"], "rb").read()
        res["tsv_byte_equal"] = bool(a == b)
        res["report_rows"] = b.count(b"\n") - 1
        return res

    def result(small, large):
        return {
            "what": "pipeline.search_files(unphased_haplotypes='device'), files to TSV, on one synthetic unphased region with indels (NGG / 20, CFD "
                    "tables on) under unphased_indel_windows='host' (the route of the parent commit) and 'device', both in one process on one "
                    "machine after a warm-up run: wall seconds, the builder's lap of search_files' stage clock, seconds inside "
                    "expand_unphased_from_vcf, kernel ms (window_*: device clock stamps; the rest: HIP events); min-max",
            "variant_mix": {**MIX, "frac_ins": round(1.0 - MIX["frac_snv"] - MIX["frac_del"], 6), "variants_asked": args.size // 15,
                            "generator": "synth.add_phased_variants, genotypes written unphased"},
            "runs": args.runs, "point_10_samples": small, "point_panel": large, "default_window_builder": "host",
        }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with tempfile.TemporaryDirectory() as d:
        small = point(os.path.join(d, "p1"), 10)
        json.dump(result(small, None), open(args.out, "w"), indent=1)
        large = point(os.path.join(d, "p2"), args.panel_samples)
    res = result(small, large)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))
    for p in (small, large):
        h, dv = p["host_windows"], p["device_windows"]
        k = dv["kernel_ms"]
        km = ", ".join(f"{s[7:]} {k[s]['min']:.3f}-{k[s]['max']:.3f}" for s in k if s.startswith("window_"))
        print(f"| unphased indel windows built on the device ({p['samples']} samples; `tools/time_unphased_windows.py`, `profiles/unphased_windows.json`, "
              f"min-max of {dv['runs']} runs) | {p['size_nt']} nt, {p['records']} records ({p['insertions']} insertions, {p['deletions']} deletions), "
              f"{p.get('instances')} instances, {p.get('window_rows')} window rows of {dv['rows_in_the_set']}: builder lap host windows "
              f"{h['builder_lap_s']['min']:.3f}-{h['builder_lap_s']['max']:.3f} s, device windows {dv['builder_lap_s']['min']:.3f}-"
              f"{dv['builder_lap_s']['max']:.3f} s; `search_files` wall {h['wall_s']['min']:.2f}-{h['wall_s']['max']:.2f} s against "
              f"{dv['wall_s']['min']:.2f}-{dv['wall_s']['max']:.2f} s; window kernels (ms): {km}; TSVs {'byte-equal' if p['tsv_byte_equal'] else 'DIFFER'} |")
    return 0 if small["tsv_byte_equal"] and large["tsv_byte_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
