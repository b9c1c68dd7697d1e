#!/usr/bin/env python3
"""Time the variant-effect stage on the report groups of an unphased interval and write profiles/unphased_effects.json.

    python tools/time_unphased_effects.py [--size 200000] [--runs 3] [--out profiles/unphased_effects.json]

The panel of tools/time_unphased_report.py: --size nt, 10 unphased samples, SNVs only, NGG / 20, CFD tables on (about 10^5 groups
at 2x10^5 nt).  One warm-up, then --runs runs, min-max:
  search_files   wall seconds, files to TSV, without the stage and with it (unphased_effects=True, graphical_reports=True)
  create         on ONE set of resident groups (GuideTable.resolve_unphased_groups(keep_resident=True)): the new entry
                 (hawk_effects_create_ugroups: hawk_effects_timing, and the wall time of the call) against the columns route - the
                 wall time of hawk_ugroups_download into fresh host arrays, then hawk_effects_create_columns' hawk_effects_timing
                 and wall time - and one hawk_effects_rank on either handle
  host           the host twin (hawk_host_effects) on the downloaded groups, wall seconds of one rank
and whether the three results are equal bit for bit."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "crispr-hawk_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "profiles", "unphased_effects.json")


def mm(v):
    return {"min": min(v), "max": max(v)}


def equal(a, b):
    cut = lambda k, x: np.ascontiguousarray(x).tobytes()[:(56 if k == "counts" else None)]
    return all(cut(k, getattr(a, k)) == cut(k, getattr(b, k)) for k in a.ARRAYS)


def built_inputs(fa, bed, vcf):
    """region, haplotypes and PAM of the one interval, as pipeline._search_host_built builds them"""
    from crisprhawk_hip import haplotypes as hap_mod
    from crisprhawk_hip.haplotype import Haplotype
    from crisprhawk_hip.pam import PAM
    from crisprhawk_hip.pipeline import PADDING
    from crisprhawk_hip.readers import VCF, Bed, Fasta
    from crisprhawk_hip.region import Region
    from crisprhawk_hip.sequence import Sequence
    pam = PAM("NGG", False, True)
    pam.encode(0)
    (coord,) = list(Bed(bed, PADDING, True))
    seq = Fasta(fa, 0, True).fetch(coord).sequence
    v = VCF(vcf, 0, True)
    region = Region(Sequence(seq, True), coord)
    haps = [Haplotype(Sequence(seq, True), region.coordinates, False, 0, True)]
    haps = hap_mod.add_variants_unphased(haps, region, v.samples, v.fetch(coord), False, True)
    for i, h in enumerate(haps):
        h.id = f"hap_{i:08d}"
    return coord, region, haps, pam


def create_routes(fa, bed, vcf, tables, runs):
    from crisprhawk_hip import _lib, graphical_reports as gr, reports
    from crisprhawk_hip.hapset import UnphasedGroups
    from crisprhawk_hip.search_guides import _device_set
    coord, region, haps, pam = built_inputs(fa, bed, vcf)
    ds = _device_set(region, haps, len(pam))
    tab = ds.search(pam.bits, pam.bitsrc, len(pam), 20, False, download=False)
    g = tab.resolve_unphased_groups(haps, pam, tables, (0, 0), "device", keep_resident=True)
    tab.close()
    lab = reports.HapLabels.from_objects(haps)
    is_ref = np.asarray(ds.is_ref, dtype=bool)
    _, order, _ = reports.group_columns(g, lab, pam, coord.contig, str(coord), None, True, is_ref_hap=is_ref)
    L = _lib.lib()
    keys = ("upload_ms", "groups_ms", "samples_ms", "total_ms")
    rows = {"ugroups": [], "columns": [], "host": []}
    last = {}
    for k in range(runs + 1):   # the first run warms allocations and is dropped
        t0 = time.perf_counter()
        st = gr.GroupEffects(g, lab.samples, is_ref, order, "device")
        t1 = time.perf_counter()
        last["ugroups"] = st.rank(gr.SIGNED, None, (), 25)
        t2 = time.perf_counter()
        a = {"create_wall_s": t1 - t0, "rank_wall_s": t2 - t1, **{n: st.timing[n] for n in keys}, "rank_total_ms": st.timing["rank_total_ms"]}
        st.close()
        t0 = time.perf_counter()
        d = UnphasedGroups(g.guidelen, g.pamlen, g.right, g.n_groups, g.n_members, getattr(ds, "device", None))
        _lib.check(L.hawk_ugroups_download(g._ug, *d._args()), "hawk_ugroups_download")
        t1 = time.perf_counter()
        st = gr.GroupEffects(d, lab.samples, is_ref, order, "device")
        t2 = time.perf_counter()
        last["columns"] = st.rank(gr.SIGNED, None, (), 25)
        t3 = time.perf_counter()
        b = {"download_wall_s": t1 - t0, "create_wall_s": t2 - t1, "rank_wall_s": t3 - t2, **{n: st.timing[n] for n in keys},
             "rank_total_ms": st.timing["rank_total_ms"]}
        st.close()
        t0 = time.perf_counter()
        st = gr.GroupEffects(d, lab.samples, is_ref, order, "host")
        last["host"] = st.rank(gr.SIGNED, None, (), 25)
        c = {"rank_wall_s": time.perf_counter() - t0}
        if k:
            rows["ugroups"].append(a); rows["columns"].append(b); rows["host"].append(c)
    res = {route: {n: mm([x[n] for x in v]) for n in v[0]} for route, v in rows.items()}
    res.update(n_groups=int(g.n_groups), n_members=int(g.n_members), n_haplotypes=len(haps),
               results_bit_equal=bool(equal(last["ugroups"], last["host"]) and equal(last["columns"], last["host"])))
    g.close(); ds.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=200_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    from crisprhawk_hip import pipeline, synth
    from time_unphased_report import write_inputs
    tables = synth.cfd_tables()
    with tempfile.TemporaryDirectory() as d:
        fa, bed, vcf, n_rec = write_inputs(args.size, d)
        print(f"inputs written: {n_rec} records", flush=True)
        laps = {}

        def run(tag, **kw):
            laps.clear()
            t0 = time.perf_counter()
            pipeline.search_files(fa, bed, [vcf], "NGG", 20, False, os.path.join(d, tag), cfd_tables=tables, debug=True, timings=laps, **kw)
            return time.perf_counter() - t0
        stage = dict(unphased_effects=True, graphical_reports=True)
        print(f"warm-up {run('warm', **stage):.2f} s", flush=True)
        plain, staged = [], []
        for _ in range(args.runs):
            plain.append(run("plain"))
            staged.append(run("staged", **stage))
            print(f"without {plain[-1]:.2f} s, with {staged[-1]:.2f} s  {laps}", flush=True)
        staged_laps = dict(laps)
        routes = create_routes(fa, bed, vcf, tables, args.runs)
    res = {"what": "the variant-effect stage on the report groups of one synthetic unphased region (10 samples, SNVs only, NGG / 20, CFD tables "
                   "on): search_files wall seconds without and with the stage; hawk_effects_timing (ms) and wall seconds of "
                   "hawk_effects_create_ugroups against hawk_ugroups_download + hawk_effects_create_columns on the same groups; the host twin",
           "size_nt": args.size, "records": n_rec, "runs": args.runs, "search_files_wall_s": {"without": mm(plain), "with": mm(staged)},
           "with_stage_wall_stages_s_last_run": staged_laps, **routes}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))
    return 0 if routes["results_bit_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
