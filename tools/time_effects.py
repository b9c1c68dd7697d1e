#!/usr/bin/env python3
"""Time the variant-effect stage (graphical_reports.GroupEffects) and write profiles/effects_table.json.

    python tools/time_effects.py [--runs 5] [--skip-c4] [--reference /path/to/reference/src]

Workloads:
  c3        the C3 report (workload.py: synth.config_c3 -> plan -> cluster search -> collapse; 2.2x10^5 groups over 2.8x10^7 rows),
            ranked by the row order of its real report (reports.group_columns)
  c4_tile   one full-size C4 tile (synth.contig_panel, 4 Mb x 5009 rows, as tests/test_gpu_fullsize_c4.py builds it); the rank of
            its groups is (start, stop) order - what decides nearly every row of the report's order - not a full report assembly
Per workload, --runs times after a warm-up: the TABLE route (hawk_effects_create on the table in HBM: export kernel + k_fx_groups +
k_fx_samples_*, then hawk_effects_rank: k_fx_positions, the selection, k_fx_alts) with wall time and HIP-event stage times; the
columns route from the exported groups (what tiling's merged groups take; it pays the upload); hawk_host_effects on the same
groups, wall time; and whether the three results are equal bit for bit.  All times in seconds, min / median / max.

--reference (build machine only; no GPU needed, and nothing else runs then): the rate of the reference's own
_compute_delta_table on the report text of g7_report_phased16, with graphical_reports.REPORTCOLS re-pointed as
tests/golden/make_golden_effects.py does, in positions per second; merged into the JSON as `reference`."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "crispr-hawk_amd"))
OUT = os.path.join(ROOT, "profiles", "effects_table.json")


def spread(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v)}


def reference_rate(out):
    import io
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import make_golden_effects as gen  # installs the stand-ins and re-points graphical_reports.REPORTCOLS
    from util import load_golden
    tsv = load_golden("g7_report_phased16.json.gz")["report_tsv"]
    runs, positions = [], 0
    for _ in range(3):
        report = gen.frame(tsv)
        t0 = time.perf_counter()
        gen.R_gr._compute_delta_table(report, [], "score_cfdon")
        runs.append(time.perf_counter() - t0)
    positions = gen.one_table(tsv, [], "score_cfdon")[0]["n_positions"]
    res = json.load(open(out)) if os.path.exists(out) else {}
    res["reference"] = {"what": "_compute_delta_table(score_cfdon) of the reference, REPORTCOLS re-pointed, on g7_report_phased16; one CPU core of the build machine",
                        "positions": positions, "report_rows": tsv.count("\n") - 1, "seconds": spread(runs),
                        "positions_per_second": positions / statistics.median(runs)}
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res["reference"]))


def equal(a, b):
    cut = lambda k, x: np.ascontiguousarray(x).tobytes()[:(56 if k == "counts" else None)]
    return all(cut(k, getattr(a, k)) == cut(k, getattr(b, k)) for k in a.ARRAYS)


def measure(name, tab, groups, hap_samples, is_ref, order, runs):
    from crisprhawk_hip import graphical_reports as gr
    res = {"groups": int(groups.n_groups), "member_rows": int(groups.n_rows), "haplotype_rows": len(hap_samples)}
    last = {}
    for route, src, engine in (("table", tab, "device"), ("columns", groups, "device"), ("host", groups, "host")):
        rows = []
        for k in range(runs + 1):  # the first run warms allocations and is dropped
            t0 = time.perf_counter()
            st = gr.GroupEffects(src, hap_samples, is_ref, order, engine)
            t1 = time.perf_counter()
            r = st.rank(gr.SIGNED, None, (), 25)
            t2 = time.perf_counter()
            row = {"create_wall": t1 - t0, "rank_wall": t2 - t1}
            tm = st.timing
            if engine == "device":
                row.update({"create_upload_or_export": tm["upload_ms"] / 1e3, "k_fx_groups": tm["groups_ms"] / 1e3, "k_fx_samples": tm["samples_ms"] / 1e3,
                            "rank_upload": tm["rank_upload_ms"] / 1e3, "k_fx_positions": tm["rank_positions_ms"] / 1e3,
                            "selection": tm["rank_topk_ms"] / 1e3, "k_fx_alts": tm["rank_alts_ms"] / 1e3})
                res["positions"], res["groups_on_the_wave_path"] = int(tm["n_positions"]), int(tm["n_long"])
            st.close()
            if k:
                rows.append(row)
        last[route] = r
        res[route] = {n: spread([x[n] for x in rows]) for n in rows[0]}
        print(name, route, json.dumps({n: round(v["median"], 6) for n, v in res[route].items()}), flush=True)
    res["results_bit_equal"] = equal(last["table"], last["host"]) and equal(last["columns"], last["host"])
    res["worst_delta_of_rank_1"] = float(last["host"].pos_worst[last["host"].chosen[0]]) if len(last["host"].chosen) else None
    return res


def c3(runs):
    from crisprhawk_hip import reports, synth
    from crisprhawk_hip.pam import PAM
    from crisprhawk_hip.workload import expand_on_device, hap_labels
    reg = synth.config_c3()
    ds, info, _, kept = expand_on_device(reg, 3, keep_plan=True)
    pam = PAM("NGG", False, True)
    pam.encode(0)
    mm, pt = synth.cfd_tables()
    tab = ds.plan.view().search(pam.bits, pam.bitsrc, 3, 20, False, mm, pt, download=False, collapse=True)
    groups = tab.export_groups()
    lab = hap_labels(reg.contig, reg.variants, ds, info, kept)
    is_ref = np.asarray(ds.is_ref, dtype=bool)
    _, order, _ = reports.group_columns(groups, lab, pam, reg.contig, f"{reg.contig}:{reg.bed_start}-{reg.bed_stop}", None, True, is_ref_hap=is_ref)
    res = measure("c3", tab, groups, lab.samples, is_ref, order, runs)
    tab.close(); ds.plan.close(); ds.close()
    return res


def c4_tile(runs):
    from crisprhawk_hip import synth
    from crisprhawk_hip.pam import PAM
    from crisprhawk_hip.tiling import TiledRegionSearch
    tile_nt, n_block, n_samples = 4_000_000, 300_000, 2504
    seq, panel = synth.contig_panel(1004, "chr22", tile_nt + 200, n_block, n_samples)
    pam = PAM("NGG", False, True)
    pam.encode(0)
    trs = TiledRegionSearch(lambda lo, hi: seq[lo - 1:hi], "chr22", 1, tile_nt + 200, panel, pam, 20, False, tile_nt=2 * tile_nt)
    pt = trs.prepare_tile(0, keep_plan=True)
    mm, ptab = synth.cfd_tables()
    tab = pt.plan.view().search(pam.bits, pam.bitsrc, 3, 20, False, mm, ptab, download=False, collapse=True, cfd_na_on_ambiguous=True)
    groups = tab.export_groups()
    ng = groups.n_groups
    order = np.lexsort((np.asarray(groups.stop)[:ng], np.asarray(groups.start)[:ng]))
    hap_samples = ["" if lb is None else lb.samples for lb in pt.labels]
    is_ref = np.array([s == "REF" for s in hap_samples])
    res = measure("c4_tile", tab, groups, hap_samples, is_ref, order, runs)
    res["rank_is"] = "(start, stop) order of the groups, not a full report assembly"
    tab.close(); pt.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--skip-c4", action="store_true")
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.reference:
        return reference_rate(a.out)
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res = {"units": "seconds", "runs": a.runs, **{k: v for k, v in res.items() if k == "reference"}}
    res["c3"] = c3(a.runs)
    json.dump(res, open(a.out, "w"), indent=1)
    if not a.skip_c4:
        res["c4_tile"] = c4_tile(max(2, a.runs // 2))
        json.dump(res, open(a.out, "w"), indent=1)
    ok = all(res[k]["results_bit_equal"] for k in ("c3", "c4_tile") if k in res)
    print(json.dumps({k: (v if not isinstance(v, dict) else {"groups": v.get("groups"), "bit_equal": v.get("results_bit_equal")}) for k, v in res.items()}))
    if not ok:
        sys.exit("device and host results differ")


if __name__ == "__main__":
    main()
