#!/usr/bin/env python3
"""Generate tests/golden/g14_effects.json.gz by running the REFERENCE's variant-effect data stage.

    python tests/golden/make_golden_effects.py

Build container only, like make_golden.py (whose stand-ins are imported).  seaborn is absent and gets an empty stand-in module;
pandas and matplotlib are present, and their module-level imports are all the reference's graphical_reports.py and
candidate_guides.py need of them for the functions run here (no figure is drawn).

ONE THING IS RE-POINTED.  At the reference's current commit graphical_reports.py reads `origin` as REPORTCOLS[14] and `samples`
as REPORTCOLS[15]; since three score columns were added to reports.REPORTCOLS those indices name `score_elevationon` and
`gc_content`, and `_compute_delta_table` ends in "AttributeError: 'float' object has no attribute 'split'" on every report.
This generator gives graphical_reports its OWN copy of the list with [14] = "origin" and [15] = "samples" - the list the module
was written for - in this process only, and changes nothing else: every table below is computed by the reference's functions
(_compute_delta_table and the steps it is made of, _count_guide_type(_assign_guide_type(_assign_extended_guide_ids(...))),
candidate_guides.subset_reports).

Inputs: the report text of g7_report_phased16 / phased4 / indel_dense.  score_cfdon runs without candidates, with two
candidates, and with one candidate whose position has alternatives but none valid.  The absolute family runs on the same
reports with a seeded synthetic `score_azimuth` column of 4-decimal values that holds a position whose FIRST alternative is NaN,
one whose LATER alternative is NaN and a NaN REF; those three positions are also run as candidates (`azimuth_nans`), which puts
their worst deltas - NaN, the maximum of the rest, NaN - into a stored table.

Stored: the fixture name, the added column, the candidate strings; the tables (columns, dtypes, rows; null = NaN), each
chosen row's worst delta, where the cut at rank 25 falls relative to the runs of equal worst delta (and, when it splits a run,
the ids of that run), the type counts, the sub-report text.  No program text.
"""
import io
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (installs the stand-ins, puts the reference and the package on sys.path)

sys.path.insert(0, mg.ROOT)
sys.modules.setdefault("seaborn", types.ModuleType("seaborn"))

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

from util import load_golden  # noqa: E402
from crisprhawk import graphical_reports as R_gr  # noqa: E402
from crisprhawk import candidate_guides as R_cg  # noqa: E402
from crisprhawk import pam as R_pam  # noqa: E402
from crisprhawk.coordinate import Coordinate  # noqa: E402

_cols = list(R_gr.REPORTCOLS)
_cols[14], _cols[15] = "origin", "samples"
R_gr.REPORTCOLS = _cols  # graphical_reports' own name only: reports.REPORTCOLS and candidate_guides.REPORTCOLS stay as they are

FIXTURES = ["phased16", "phased4", "indel_dense"]
K = 25


def frame(tsv):
    return pd.read_csv(io.StringIO(tsv), sep="\t")


def delta_table(report, cgids, score):
    """_compute_delta_table, step by step (graphical_reports.py:875-881), keeping the ranking it selects from"""
    report = R_gr._assign_guide_ids(report)
    report = R_gr._assign_nsamples(report)
    deltas = R_gr._compute_scores_delta(report, score)
    rows = R_gr._build_guide_rows(deltas, score)
    worst = R_gr._rank_guides_by_worst_delta(rows, score)
    final = R_gr._select_top_guides(worst, cgids)
    return R_gr._construct_delta_table(final, rows), worst, final


def same(a, b):
    return (a != a and b != b) or a == b


def table_json(df):
    rows = []
    for rec in df.itertuples(index=False):
        rows.append([None if (isinstance(v, float) and v != v) else (v.item() if hasattr(v, "item") else v) for v in rec])
    return {"columns": list(df.columns), "dtypes": [str(t) for t in df.dtypes], "rows": rows}


def one_table(tsv, cgids, score, extra=None):
    report = frame(tsv)
    if extra is not None:
        report[score] = np.array([np.nan if v is None else v for v in extra], dtype=np.float64)
    table, worst, final = delta_table(report, list(cgids), score)
    again = R_gr._compute_delta_table(frame(tsv).assign(**({score: report[score]} if extra is not None else {})), list(cgids), score)
    assert table.equals(again)
    wd = dict(zip(worst["guide_id"], worst["delta"]))
    others = worst[~worst["guide_id"].isin(cgids)].reset_index(drop=True)
    n_other = K - len(cgids)
    cut = {"split": False, "last_in": None, "first_out": None, "run_ids": []}
    if len(others) > n_other:
        a, b = float(others["delta"][n_other - 1]), float(others["delta"][n_other])
        cut["last_in"], cut["first_out"] = (None if a != a else a), (None if b != b else b)
        cut["split"] = bool(same(a, b))
        if cut["split"]:
            cut["run_ids"] = [g for g, d in zip(others["guide_id"], others["delta"]) if same(float(d), a)]
    out = table_json(table)
    out["worst"] = [None if wd[g] != wd[g] else float(wd[g]) for g in table["guide_id"]]
    out["cut"] = cut
    out["n_positions"] = int(len(worst))
    out["max_alts"] = (len(table.columns) - 6) // 7
    return out, worst, report


def synthetic_column(tsv, seed):
    """score_azimuth per report row: 4-decimal values, then the three NaNs"""
    report = frame(tsv)
    rng = np.random.default_rng(seed)
    col = [round(float(v), 4) for v in rng.integers(0, 10001, len(report)) / 10000.0]
    gid = (report["start"].astype(str) + "_" + report["strand"]).tolist()
    origin = report["origin"].tolist()
    by = {}
    for i, g in enumerate(gid):
        by.setdefault(g, []).append(i)
    pos = [(g, r) for g, r in by.items() if sum(origin[i] == "ref" for i in r) == 1 and sum(origin[i] == "alt" for i in r) >= 2]
    assert len(pos) >= 3
    alts = lambda r: [i for i in r if origin[i] == "alt"]
    first_nan, later_nan, ref_nan = pos[0], pos[1], pos[2]
    col[alts(first_nan[1])[0]] = None
    col[alts(later_nan[1])[1]] = None
    col[[i for i in ref_nan[1] if origin[i] == "ref"][0]] = None
    return col, {"first_alt_nan": first_nan[0], "later_alt_nan": later_nan[0], "ref_nan": ref_nan[0]}


def pick_candidates(fx, worst, report):
    """two positions outside the 25 worst (one with valid alternatives, one without any alternative), and one position that has
    alternatives of which none is valid"""
    contig = fx["contig"]
    chosen = set(worst["guide_id"][:K])
    rest = worst[~worst["guide_id"].isin(chosen)]
    with_valid = rest[rest["delta"] < 0]["guide_id"].tolist()
    gid = (report["chr"] + "_" + report["start"].astype(str) + "_" + report["strand"])
    n_alt = (report["origin"] == "alt").groupby(gid).sum()
    zero = rest[rest["delta"] == 0]["guide_id"].tolist()
    none_valid = [g for g in zero if n_alt[g] > 0]
    no_alt = [g for g in zero if n_alt[g] == 0]
    assert with_valid and none_valid and no_alt, (len(with_valid), len(none_valid), len(no_alt))
    assert all(g.startswith(contig + "_") for g in (with_valid[-1], no_alt[0], none_valid[0]))
    return [no_alt[0], with_valid[-1]], [none_valid[0]]


if __name__ == "__main__":
    out = {"k": K, "fixtures": {}}
    splits = {"score_cfdon": 0, "score_azimuth": 0}
    for fi, name in enumerate(FIXTURES):
        fx = load_golden(f"g7_report_{name}.json.gz")
        tsv = fx["report_tsv"]
        rec = {"tables": {}}
        base, worst, report = one_table(tsv, [], "score_cfdon")
        two, none_valid = pick_candidates(fx, worst, report)
        rec["candidates"] = {"two": two, "none_valid": none_valid}
        rec["tables"]["cfdon"] = base
        rec["tables"]["cfdon_two"] = one_table(tsv, two, "score_cfdon")[0]
        rec["tables"]["cfdon_none_valid"] = one_table(tsv, none_valid, "score_cfdon")[0]
        col, where = synthetic_column(tsv, 14000 + fi)
        rec["score_azimuth"], rec["score_azimuth_nans"] = col, where
        rec["tables"]["azimuth"] = one_table(tsv, [], "score_azimuth", col)[0]
        rec["tables"]["azimuth_two"] = one_table(tsv, two, "score_azimuth", col)[0]
        # the three planted positions forced in as candidates: the reference computes each candidate's own worst delta, so the
        # NaN-first rule of max() is in a stored table (a NaN worst ranks last and would never be chosen otherwise)
        nans = [f"{fx['contig']}_{where[k]}" for k in ("first_alt_nan", "later_alt_nan", "ref_nan")]
        rec["candidates"]["nans"] = nans
        rec["tables"]["azimuth_nans"] = one_table(tsv, nans, "score_azimuth", col)[0]
        w3 = rec["tables"]["azimuth_nans"]["worst"][:3]
        assert w3[0] is None and w3[1] is not None and w3[2] is None, w3
        for key, tab in rec["tables"].items():
            score = "score_cfdon" if key.startswith("cfdon") else "score_azimuth"
            if not key.endswith(("_two", "_none_valid", "_nans")):
                splits[score] += tab["cut"]["split"]
            print(f"   {name} {key}: {len(tab['rows'])} rows, {tab['n_positions']} positions, max {tab['max_alts']} alts, cut {tab['cut']['last_in']} | "
                  f"{tab['cut']['first_out']} split={tab['cut']['split']} ({len(tab['cut']['run_ids'])} ids)")
        rep = frame(tsv)
        typed = R_gr._assign_guide_type(R_gr._assign_extended_guide_ids(rep), True)
        rec["type_counts"] = R_gr._count_guide_type(typed["guide_type"].tolist())
        rec["n_distinct_guides"] = int(len(typed))
        print(f"   {name} types: {rec['type_counts']}")
        # candidate_guides.subset_reports on the written report (as is: no stale index in that module)
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
        out["fixtures"][name] = rec
    # the conditions tests rely on when they exempt the order inside a run of equal worst deltas
    assert all(v <= 1 for v in splits.values()), splits
    out["split_tables"] = splits
    mg.dump("g14_effects.json.gz", out)
