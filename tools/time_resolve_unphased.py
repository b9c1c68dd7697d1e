#!/usr/bin/env python3
"""Time search() on an unphased population VCF with the IUPAC windows resolved on the host (resolve_guide: the route before the
device kernels existed) against the device (hawk_table_resolve_unphased) and write profiles/resolve_unphased.json.

    python tools/time_resolve_unphased.py [--size 200000] [--runs 3] [--host-limit 60]

One seeded synthetic region of --size nt, 10 unphased samples, SNVs only, a sample heterozygous about every 25 nt (a site every 15
nt, carried by a chromosome copy with probability 0.3-0.6), NGG / 20.  The haplotypes are built once on the host
(haplotypes.add_variants_unphased; not timed).  If one host-route run takes longer than --host-limit seconds the region is halved
until it does not; the size used is recorded.  Then --runs runs of either engine: wall time of search(), for the device route the
HIP-event time of every pass, the table's rows, the resolved and the kept guides - and whether the two guide lists are equal.
Prints the README table row."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "crispr-hawk_amd"))
OUT = os.path.join(ROOT, "profiles", "resolve_unphased.json")


def build(size: int):
    from crisprhawk_hip import haplotypes as H, synth
    from crisprhawk_hip.coordinate import Coordinate
    from crisprhawk_hip.haplotype import Haplotype
    from crisprhawk_hip.region import Region
    from crisprhawk_hip.sequence import Sequence
    from crisprhawk_hip.variant import VariantRecord
    reg = synth.make_region(8101, "chrT", size + 2400, 1000, 1000 + size)
    synth.add_phased_variants(reg, 8102, size // 15, 10, frac_snv=1.0, frac_del=0.0, max_indel=1, af_min=0.3, af_max=0.6)
    region = Region(Sequence(reg.sequence, True), Coordinate(reg.contig, reg.bed_start, reg.bed_stop, synth.PADDING))
    recs = []
    for v in reg.variants:
        f = reg.vcf_fields(v)
        f[9:] = [g.replace("|", "/") for g in f[9:]]
        r = VariantRecord(True)
        r.read_vcf_line(f, reg.samples, False)
        recs.append(r)
    haps = [Haplotype(Sequence(region.sequence.sequence, True), region.coordinates, False, 0, True)]
    haps = H.add_variants_unphased(haps, region, reg.samples, recs, False, True)
    for i, h in enumerate(haps):
        h.id = f"hap_{i:08d}"
    het = sum(c in "rykmswbdhvn" for c in haps[1].sequence.sequence) if len(haps) > 1 else 0
    return region, haps, len(recs), het


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=200_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-limit", type=float, default=60.0)
    args = ap.parse_args()
    from crisprhawk_hip import search_guides as sg
    from crisprhawk_hip.pam import PAM
    pam = PAM("NGG", False, True)
    pam.encode(0)

    def run(engine, region, haps):
        t0 = time.perf_counter()
        guides = sg.search(pam, region, haps, None, 20, False, True, False, 0, True, unphased_engine=engine)
        return time.perf_counter() - t0, guides

    def listed(guides):
        return [(g.start, g.stop, g.strand, g.sequence, g.hapid, g.right, g.samples) for g in guides]

    size, shrunk = args.size, []
    while True:
        t0 = time.perf_counter()
        region, haps, n_rec, het = build(size)
        print(f"size {size}: {len(haps)} haplotypes from {n_rec} records built in {time.perf_counter() - t0:.1f} s; "
              f"{het} ambiguous letters in the first sample's haplotype", flush=True)
        run("device", region, haps)  # warm-up: library, context, first launches
        first, want = run("host", region, haps)
        print(f"size {size}: host route {first:.1f} s, {len(want)} guides", flush=True)
        if first <= args.host_limit or size <= 2000:
            break
        shrunk.append({"size": size, "host_seconds": first})
        size //= 2
    want = listed(want)
    host, dev, passes, equal = [first], [], [], True
    for _ in range(args.runs - 1):
        host.append(run("host", region, haps)[0])
        print(f"host {host[-1]:.2f} s", flush=True)
    for _ in range(args.runs):
        t, g = run("device", region, haps)
        dev.append(t)
        passes.append(dict(sg.last_resolve_timing))
        equal = equal and listed(g) == want
        print(f"device {t:.2f} s  {passes[-1]}", flush=True)
    mm = lambda v: {"min": min(v), "max": max(v)}
    keys = ("upload_ms", "refsort_ms", "count_ms", "scan_ms", "fill_ms", "total_ms")
    res = {
        "what": "search() on one synthetic unphased region: 10 samples, SNVs only, NGG / 20; wall seconds per engine, HIP-event ms per pass",
        "size_nt": size, "size_asked": args.size, "shrunk_from": shrunk, "host_limit_s": args.host_limit, "runs": args.runs,
        "records": n_rec, "haplotypes": len(haps), "ambiguous_letters_first_sample": het,
        "source_rows": passes[0]["n_rows"], "resolved": passes[0]["n_resolved"], "kept": passes[0]["n_kept"], "batches": passes[0]["n_batches"],
        "host_wall_s": mm(host), "device_wall_s": mm(dev), "kernel_ms": {k: mm([p[k] for p in passes]) for k in keys},
        "lists_equal": bool(equal), "guides": len(want),
    }
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(res, open(OUT, "w"), indent=1)
    km = res["kernel_ms"]
    print(json.dumps(res))
    print(f"| unphased IUPAC windows resolved on the table (`hawk_table_resolve_unphased`: `k_ur_count`, `k_ur_fill`; `tools/time_resolve_unphased.py`, "
          f"`profiles/resolve_unphased.json`, {args.runs} runs, min-max) | {size} nt, 10 unphased samples, NGG / 20: {res['source_rows']} rows -> "
          f"{res['resolved']} resolved -> {res['kept']} kept guides.  `search()` wall: host route {min(host):.2f}-{max(host):.2f} s, device route "
          f"{min(dev):.2f}-{max(dev):.2f} s; passes: REF sort {km['refsort_ms']['min']:.3f}-{km['refsort_ms']['max']:.3f} ms, count "
          f"{km['count_ms']['min']:.3f}-{km['count_ms']['max']:.3f}, scan {km['scan_ms']['min']:.3f}-{km['scan_ms']['max']:.3f}, fill + copies "
          f"{km['fill_ms']['min']:.3f}-{km['fill_ms']['max']:.3f}, both calls on the device {km['total_ms']['min']:.3f}-{km['total_ms']['max']:.3f}; lists "
          f"{'equal' if equal else 'DIFFER'} |")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
