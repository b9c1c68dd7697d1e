#!/usr/bin/env python3
"""Generate tests/golden/g16_effects_unphased.json.gz: the REFERENCE's variant-effect data stage on UNPHASED reports.

    python tests/golden/make_golden_effects_unphased.py

Build container only, like make_golden_effects.py, whose functions do the work here: they are imported, not copied, and with them
comes that module's one re-pointing (graphical_reports' own REPORTCOLS with [14] = "origin" and [15] = "samples"; its docstring
says why).  The reference's stage accepts an unphased report as it accepts a phased one: every table below is computed by
_compute_delta_table, _count_guide_type(_assign_guide_type(_assign_extended_guide_ids(...))) and candidate_guides.subset_reports.

Inputs, two reports:
  unphased        the report text of g7_report_unphased (3.2 kb, 9 haplotypes)
  unphased_dense  make_golden.g7_report(None, reg, "NGG", 20, False, unphased=True) on a 7 kb region of 260 variants in 6 samples
                  (227 SNVs + 33 indels: 7 whole-region haplotypes + 114 indel windows, 1994 report rows, 905 positions with a REF
                  group, 166 of them with two or more alternatives, at most 10).  Its whole fixture dict is stored (`fixture`), so
                  tests can write its FASTA / BED / VCF.

Stored per input what g14 stores per fixture: the added column, the candidate strings, the tables (columns, dtypes, rows; null =
NaN) with each chosen row's worst delta and where the cut at rank 25 falls, the type counts, the sub-report text.  No program text.

Asserted here, each of the reference alone:
  - every input has exactly one haplotype labelled REF (the device resolution declines a set with more: MULTI_REF);
  - at most one of a score's no-candidate tables splits a run of equal worst deltas at rank 25 (the tests exempt the order
    inside such a run and rely on this cap);
  - pick_candidates and synthetic_column find their positions (their own assertions).
"""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_effects as ge  # noqa: E402  (make_golden's stand-ins, the reference on sys.path, the REPORTCOLS re-pointing)

mg, R_gr, R_cg, R_pam, Coordinate = ge.mg, ge.R_gr, ge.R_cg, ge.R_pam, ge.Coordinate

from crisprhawk_hip import synth  # noqa: E402

INPUTS = ["unphased", "unphased_dense"]


def dense_fixture():
    reg = synth.make_region(16001, "chrD", 9000, 1000, 8000)
    synth.add_phased_variants(reg, 16002, 260, 6, frac_snv=0.85, frac_del=0.08, max_indel=3, af_min=0.2, af_max=0.6)
    return mg.g7_report(None, reg, "NGG", 20, False, unphased=True)


def record(fx, seed, splits, name):
    """what make_golden_effects stores for one fixture, by its functions"""
    tsv = fx["report_tsv"]
    rec = {"tables": {}}
    base, worst, report = ge.one_table(tsv, [], "score_cfdon")
    two, none_valid = ge.pick_candidates(fx, worst, report)
    rec["candidates"] = {"two": two, "none_valid": none_valid}
    rec["tables"]["cfdon"] = base
    rec["tables"]["cfdon_two"] = ge.one_table(tsv, two, "score_cfdon")[0]
    rec["tables"]["cfdon_none_valid"] = ge.one_table(tsv, none_valid, "score_cfdon")[0]
    col, where = ge.synthetic_column(tsv, seed)
    rec["score_azimuth"], rec["score_azimuth_nans"] = col, where
    rec["tables"]["azimuth"] = ge.one_table(tsv, [], "score_azimuth", col)[0]
    rec["tables"]["azimuth_two"] = ge.one_table(tsv, two, "score_azimuth", col)[0]
    nans = [f"{fx['contig']}_{where[k]}" for k in ("first_alt_nan", "later_alt_nan", "ref_nan")]
    rec["candidates"]["nans"] = nans
    rec["tables"]["azimuth_nans"] = ge.one_table(tsv, nans, "score_azimuth", col)[0]
    w3 = rec["tables"]["azimuth_nans"]["worst"][:3]
    assert w3[0] is None and w3[1] is not None and w3[2] is None, w3
    for key, tab in rec["tables"].items():
        score = "score_cfdon" if key.startswith("cfdon") else "score_azimuth"
        if not key.endswith(("_two", "_none_valid", "_nans")):
            splits[score] += tab["cut"]["split"]
        print(f"   {name} {key}: {len(tab['rows'])} rows, {tab['n_positions']} positions, max {tab['max_alts']} alts, cut {tab['cut']['last_in']} | "
              f"{tab['cut']['first_out']} split={tab['cut']['split']} ({len(tab['cut']['run_ids'])} ids)")
    typed = R_gr._assign_guide_type(R_gr._assign_extended_guide_ids(ge.frame(tsv)), True)
    rec["type_counts"] = R_gr._count_guide_type(typed["guide_type"].tolist())
    rec["n_distinct_guides"] = int(len(typed))
    print(f"   {name} types: {rec['type_counts']}")
    pam = R_pam.PAM(fx["pam"], fx["right"], True)
    subs = {}
    cstr = [f"{fx['contig']}:{g.split('_')[-2]}:{g.split('_')[-1]}" for g in two + none_valid]
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "report.tsv")
        with open(path, "w") as f:
            f.write(tsv)
        cgs = R_cg.initialize_candidate_guides(cstr, fx["guidelen"], True)
        region = Coordinate(fx["contig"], fx["bed_start"], fx["bed_stop"], 0)
        made = R_cg.subset_reports(cgs, {region: path}, pam, fx["guidelen"], td, True)
        assert len(made) == len(cgs)
        for cg, p in made.items():
            subs[os.path.basename(p)] = open(p).read()
    rec["candidate_strings"] = cstr
    rec["subreports"] = subs
    return rec


if __name__ == "__main__":
    out = {"k": ge.K, "fixtures": {}}
    splits = {"score_cfdon": 0, "score_azimuth": 0}
    for fi, name in enumerate(INPUTS):
        fx = ge.load_golden("g7_report_unphased.json.gz") if name == "unphased" else dense_fixture()
        n_ref = sum(1 for h in fx["haplotypes"] if h["samples"] == "REF")
        assert fx["unphased"] and n_ref == 1, (name, n_ref)
        rec = record(fx, 16000 + fi, splits, name)
        if name == "unphased_dense":
            rec["fixture"] = fx
            nv = sum(1 for v in fx["variants"] if len(v[1]) == len(v[2]))
            print(f"   {name}: {nv} SNVs + {len(fx['variants']) - nv} indels, {len(fx['haplotypes'])} haplotypes, "
                  f"{fx['report_tsv'].count(chr(10)) - 1} report rows")
        out["fixtures"][name] = rec
    assert all(v <= 1 for v in splits.values()), splits
    out["split_tables"] = splits
    mg.dump("g16_effects_unphased.json.gz", out)
