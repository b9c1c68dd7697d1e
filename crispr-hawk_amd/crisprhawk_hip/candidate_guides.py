"""Candidate guides (the reference's --candidate-guides, candidate_guides.py:39-216): the CandidateGuide coordinate class and the
per-candidate sub-report - the report rows whose start is the candidate's position.  The reference reads the report TSV it has
just written back into pandas and filters it; here the rows come from the report's columns, which are still in hand
(reports.group_columns), joined as the report's own text is: byte-identical to filtering the written report, nothing is read back.
The candidate plots stay out of scope."""
import os
from typing import Dict, List

import numpy as np

from .coordinate import Coordinate
from .crisprhawk_error import CrisprHawkCandidateGuideError
from .exception_handlers import exception_handler
from .utils import CANDIDATEGUIDESREPORTPREFIX


class CandidateGuide:
    """'contig:position:strand' (candidate_guides.py:39-80)"""

    def __init__(self, coordinate: str, guidelen: int, debug: bool) -> None:
        self._debug = debug
        self._parse_candidate_coord(coordinate, guidelen, debug)

    def __str__(self) -> str:
        return f"{self.contig}:{self.position}"

    def _parse_candidate_coord(self, coordinate: str, guidelen: int, debug: bool) -> None:
        contig, position, strand = coordinate.split(":")
        try:
            self._coordinate = Coordinate(contig, int(position), int(position) + guidelen, 0)
            self._strand = strand
        except Exception as e:
            exception_handler(CrisprHawkCandidateGuideError, f"Forbidden candidate guide coordinate ({coordinate})", os.EX_DATAERR, debug, e)

    coordinate = property(lambda self: self._coordinate)
    contig = property(lambda self: self._coordinate.contig)
    position = property(lambda self: self._coordinate.start)
    strand = property(lambda self: self._strand)


def initialize_candidate_guides(candidate_guides: List[str], guidelen: int, debug: bool) -> List[CandidateGuide]:
    return [CandidateGuide(g, guidelen, debug) for g in candidate_guides]


def initialize_region_reports(reports_by_region: Dict) -> Dict[Coordinate, object]:
    """{region: report} -> {region's coordinates: report} (candidate_guides.py:102-116); a report here is what
    reports.group_columns returned for the region - (cols, order, plain)"""
    return {(r if isinstance(r, Coordinate) else r.coordinates): rep for r, rep in reports_by_region.items()}


def subset_reports(candidate_guides: List[CandidateGuide], region_reports: Dict[Coordinate, object], pam, guidelen: int, outdir: str,
                   debug: bool) -> Dict[CandidateGuide, str]:
    """{CANDIDATEGUIDESREPORTPREFIX}__{contig}_{position}_{pam}_{guidelen}.tsv per candidate inside a region
    (candidate_guides.py:119-216): the rows of the region's report whose `start` equals the candidate's position, in report order.
    A candidate without a row is a CrisprHawkCandidateGuideError with the reference's message."""
    from . import reports
    cg_reports = {}
    for region, (cols, order, plain) in region_reports.items():
        order = np.asarray(order, dtype=np.int64)
        start = np.asarray(cols["start"].v)[order] if len(order) else np.zeros(0, np.int64)
        for cg in candidate_guides:
            if not region.contains(cg.coordinate):
                continue
            rows = order[start == cg.position]
            if len(rows) == 0:
                exception_handler(CrisprHawkCandidateGuideError, f"Candidate guide {cg} not found. Is the candidate guide correct?", os.EX_DATAERR, debug)
            path = os.path.join(outdir, f"{CANDIDATEGUIDESREPORTPREFIX}__{cg.contig}_{cg.position}_{pam}_{guidelen}.tsv")
            # a few rows: their fields taken column by column and joined as reports.to_tsv joins the whole report
            import pandas as pd
            take = lambda col: (np.full(len(rows), col.text, dtype=object) if isinstance(col, reports.ConstCol)
                                else col.take(rows) if isinstance(col, reports.IntCol) else np.asarray(reports._col_take(col, rows)).astype(object))
            with open(path, "w") as f:
                f.write(reports.to_tsv(pd.DataFrame({c: take(col) for c, col in cols.items()})))
            cg_reports[cg] = path
    return cg_reports
