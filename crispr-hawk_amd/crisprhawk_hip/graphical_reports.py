"""The data stage behind the reference's --graphical-reports (graphical_reports.py): which reference guides lose the most
activity to population variants, in how many samples, and because of which variant - as TABLES.  Plotting stays out of scope
(DESIGN.md §9): nothing here imports matplotlib.

The reference computes these tables with DataFrame.apply / groupby.apply over the report TSV it has just written and read back.
Here they are a few passes over the report GROUPS, which are still in HBM after the collapse (csrc/hawk_effects.hip behind
hawk_effects_*; the rules are stated once in csrc/hawk_effects.h, which `engine="host"` applies on the host through
hawk_host_effects).  Only the strings of the at most 25 chosen positions and their few alternatives are taken from the report
columns on the host.

Pinned against the reference's own functions (tests/golden/g14_effects.json.gz), with ONE order that is ours: inside a run of
equal worst deltas pandas' unstable single-column sort leaves the reference's order undefined, and positions rank here by their
first appearance in report order.
"""
import ctypes as C
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from .crisprhawk_error import CrisprHawkGraphicalReportsError
from .exception_handlers import exception_handler

PADDING = 100  # region_constructor.py:21

GUIDETYPES = {  # graphical_reports.py:37-42
    0: "Reference Guides",
    1: "Spacer+PAM Alternative Guides",
    2: "Spacer Alternative Guides",
    3: "PAM Alternative Guides",
}
SCORES = ["score_azimuth", "score_rs3", "score_deepcpf1", "score_cfdon", "score_elevationon", "score_plmcrispr", "score_crispron",
          "score_sgdesigner"]  # graphical_reports.py:45-54
DELTACOLS = ["delta", "abs_delta"]
TOPK = 25
FX_NONE = 0xFFFFFFFF      # HAWK_FX_NONE (include/hawk.h)
FX_TYPE_UNKNOWN = 255     # HAWK_FX_TYPE_UNKNOWN
SIGNED, ABSOLUTE = 0, 1
_FAMILY = {"score_cfdon": SIGNED, "score_azimuth": ABSOLUTE, "score_rs3": ABSOLUTE, "score_deepcpf1": ABSOLUTE}


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def create_figures_dir(outdir: str) -> str:
    outdir_gr = os.path.join(outdir, "figures")
    os.makedirs(outdir_gr, exist_ok=True)
    return outdir_gr


def format_region_prefix(region) -> str:
    """`region`: anything with contig / start / stop holding the PADDED coordinates (a coordinate.Coordinate, a region.Region)"""
    return f"{region.contig}_{region.start + PADDING}_{region.stop - PADDING}"


def score_family(score: str, debug: bool = True) -> int:
    if score not in _FAMILY:
        exception_handler(CrisprHawkGraphicalReportsError, f"No delta table for score {score}: this package computes {sorted(_FAMILY)}", os.EX_DATAERR, debug)
    return _FAMILY[score]


def sample_csr(hap_samples: Sequence[str]):
    """Haplotype row -> the ids of the samples its label names (the text before ':' of every comma entry; 'REF' and '' name none)
    as a CSR: (hap_off uint64[n_hap + 1], sample_id uint32[], number of distinct names)."""
    ids: Dict[str, int] = {}
    memo: Dict[str, np.ndarray] = {}
    per = []
    for lab in hap_samples:
        a = memo.get(lab)
        if a is None:
            names = [] if lab in ("REF", "") else [e.split(":")[0] for e in lab.split(",")]
            a = memo[lab] = np.array([ids.setdefault(n, len(ids)) for n in names], dtype=np.uint32)
        per.append(a)
    off = np.zeros(len(per) + 1, dtype=np.uint64)
    if per:
        off[1:] = np.cumsum([len(a) for a in per])
    flat = np.ascontiguousarray(np.concatenate(per), dtype=np.uint32) if per and off[-1] else np.zeros(0, np.uint32)
    return off, flat, len(ids)


class EffectsResult:
    """What one rank call leaves: per group score / delta / abs_delta / n_samples / type / dup / position, per position (at its
    head) ref / worst / n_valid / first_rank, the chosen heads with the CSR of their valid alternatives, the counts."""

    def __init__(self, n_groups: int, per_position: bool = True):
        g = n_groups
        self.score, self.delta, self.abs_delta = np.zeros(g), np.zeros(g), np.zeros(g)
        self.n_samples, self.type, self.dup = np.zeros(g, np.uint32), np.zeros(g, np.uint8), np.zeros(g, np.uint8)
        self.position = np.zeros(g, np.uint32)
        self.pos_ref, self.pos_worst = np.zeros(g, np.uint32), np.zeros(g)
        self.pos_nvalid, self.pos_first_rank = np.zeros(g, np.uint32), np.zeros(g, np.uint32)
        self.counts = np.zeros(8, np.uint64)
        self.chosen, self.alt_off, self.alt_group = np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint32)

    def out_struct(self) -> "_lib.EffectsOut":
        return _lib.EffectsOut(*[_p(getattr(self, k)) for k, _ in _lib.EffectsOut._fields_])

    ARRAYS = ("score", "delta", "abs_delta", "n_samples", "type", "dup", "position", "pos_ref", "pos_worst", "pos_nvalid", "pos_first_rank",
              "chosen", "alt_off", "alt_group", "counts")


class GroupEffects:
    """The variant-effect stage over one set of report groups.

    `groups`: a hapset.GuideTable that is collapsed and still on the device (engine "device": hawk_effects_create, nothing is
    downloaded), or group columns - a hapset.GroupTable, reports.ReportGroups, tiling's merged groups - which go through
    hawk_effects_create_columns ("device") or hawk_host_effects ("host").  A hapset.UnphasedGroups that still holds its device
    result (resolve_unphased_groups(..., keep_resident=True)) is ranked where it lies on engine "device"
    (hawk_effects_create_ugroups: no group column is uploaded); without the handle, or on "host", it is group columns like any
    other.  `order` is the row order reports.group_columns returned,
    `hap_samples[h]` the samples label of haplotype row h, `is_ref_hap[h]` whether it is REF."""

    def __init__(self, groups, hap_samples: Sequence[str], is_ref_hap, order, engine: str = "device"):
        if engine not in ("device", "host"):
            raise ValueError(f"engine {engine!r}: 'device' or 'host'")
        self.engine = engine
        self._L = _lib.lib()
        self._fx = None
        self.timing: Dict[str, float] = {}
        ng = int(groups.n_groups)
        self.n_groups = ng
        order = np.asarray(order, dtype=np.int64)
        if len(order) != ng:
            raise ValueError("order: one entry per group")
        rank = np.empty(ng, dtype=np.uint32)
        rank[order] = np.arange(ng, dtype=np.uint32)
        self._hap_off, self._sid, self._n_ids = sample_csr(hap_samples)
        is_ref_hap = np.ascontiguousarray(np.asarray(is_ref_hap, dtype=bool).astype(np.uint8))
        self._table = hasattr(groups, "_t") and hasattr(groups, "export_groups")
        self.perm = None  # group columns are brought into collapse order (start, strand, group) when they are not in it
        if self._table:
            if engine != "device":
                raise ValueError("a device-resident table runs on the device: export its groups for engine='host'")
            if groups._t is None:
                raise RuntimeError("the table has been closed or downloaded: the stage needs it collapsed and still on the device")
            self._rank = rank
            fx, tm = C.c_void_p(), _lib.EffectsTiming()
            _lib.check(self._L.hawk_effects_create(groups._t, _p(rank), _p(self._hap_off), _p(self._sid), C.c_uint32(len(hap_samples)),
                                                   C.c_uint32(self._n_ids), C.byref(fx), C.byref(tm)), "hawk_effects_create")
            self._fx = fx
            self.timing = {k: getattr(tm, k) for k, _ in tm._fields_ if k != "reserved"}
            return
        if engine == "device" and getattr(groups, "_ug", None) is not None:  # resident groups: already in (start, strand, ...) order
            self._rank = rank
            fx, tm = C.c_void_p(), _lib.EffectsTiming()
            _lib.check(self._L.hawk_effects_create_ugroups(groups._ug, _p(rank), _p(self._hap_off), _p(self._sid), C.c_uint32(len(hap_samples)),
                                                           C.c_uint32(self._n_ids), C.byref(fx), C.byref(tm)), "hawk_effects_create_ugroups")
            self._fx = fx
            self.timing = {k: getattr(tm, k) for k, _ in tm._fields_ if k != "reserved"}
            return
        start, strand = np.asarray(groups.start, dtype=np.int64)[:ng], np.asarray(groups.strand, dtype=np.uint8)[:ng]
        perm = np.lexsort((strand, start))  # stable: groups of one position keep their order
        if not np.array_equal(perm, np.arange(ng)):
            self.perm = perm
        take = (lambda a: np.ascontiguousarray(a[perm])) if self.perm is not None else (lambda a: np.ascontiguousarray(a))
        moff = np.asarray(groups.member_off, dtype=np.int64)
        mhap = np.asarray(groups.member_hap, dtype=np.uint32)
        if self.perm is not None:
            cnt = np.diff(moff)[perm]
            new_off = np.zeros(ng + 1, dtype=np.int64)
            new_off[1:] = np.cumsum(cnt)
            idx = np.repeat(moff[:-1][perm] - new_off[:-1], cnt) + np.arange(int(new_off[-1]))
            mhap, moff = mhap[idx], new_off
        self._a = dict(start=take(start), stop=take(np.asarray(groups.stop, dtype=np.int64)[:ng]), strand=take(strand),
                       win=np.ascontiguousarray(np.asarray(groups.win, dtype=np.uint64)[:, :ng][:, perm] if self.perm is not None
                                                else np.asarray(groups.win, dtype=np.uint64)[:, :ng]),
                       cfdon=None if groups.cfdon is None else take(np.asarray(groups.cfdon, dtype=np.float64)[:ng]),
                       member_off=np.ascontiguousarray(moff, dtype=np.uint64), member_hap=np.ascontiguousarray(mhap, dtype=np.uint32),
                       hap_is_ref=is_ref_hap, rank=take(rank))
        a = self._a
        self._cols = _lib.EffectsColumns(ng, ng, _p(a["start"]), _p(a["stop"]), _p(a["strand"]), _p(a["win"]), _p(a["cfdon"]), _p(a["member_off"]),
                                         _p(a["member_hap"]), _p(a["hap_is_ref"]), _p(self._hap_off), _p(self._sid), _p(a["rank"]),
                                         len(hap_samples), self._n_ids, int(groups.guidelen), int(groups.pamlen), int(bool(groups.right)), 0)
        if engine == "device":
            fx, tm = C.c_void_p(), _lib.EffectsTiming()
            _lib.check(self._L.hawk_effects_create_columns(_lib.context(), C.byref(self._cols), C.byref(fx), C.byref(tm)), "hawk_effects_create_columns")
            self._fx = fx
            self.timing = {k: getattr(tm, k) for k, _ in tm._fields_ if k != "reserved"}

    def close(self) -> None:
        if self._fx is not None:
            self._L.hawk_effects_free(self._fx)
            self._fx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rank(self, family: int, score: Optional[np.ndarray] = None, candidates: Sequence = (), K: int = TOPK) -> EffectsResult:
        """One score: `score[g]` per group in the order the groups were given (None: the groups' CFDon), `candidates` (start,
        strand) pairs.  The result's arrays are indexed by the groups as they were given."""
        ng = self.n_groups
        cs = np.ascontiguousarray([c[0] for c in candidates], dtype=np.int64)
        ct = np.ascontiguousarray([c[1] for c in candidates], dtype=np.uint8)
        sc = None
        if score is not None:
            sc = np.asarray(score, dtype=np.float64)
            if len(sc) != ng:
                raise ValueError("score: one value per group")
            sc = np.ascontiguousarray(sc[self.perm] if self.perm is not None else sc)
        res = EffectsResult(ng)
        nc, na = C.c_uint32(0), C.c_uint64(0)
        if self._fx is not None:
            tm = _lib.EffectsTiming()
            _lib.check(self._L.hawk_effects_rank(self._fx, family, _p(sc), _p(cs), _p(ct), C.c_uint32(len(cs)), C.c_uint32(K), C.byref(nc), C.byref(na),
                                                 C.byref(tm)), "hawk_effects_rank")
            self.timing.update({"rank_" + k: getattr(tm, k) for k, _ in tm._fields_ if k.endswith("_ms")})
            res.chosen, res.alt_off, res.alt_group = np.zeros(nc.value, np.uint32), np.zeros(nc.value + 1, np.uint64), np.zeros(na.value, np.uint32)
            out = res.out_struct()
            _lib.check(self._L.hawk_effects_download(self._fx, C.byref(out)), "hawk_effects_download")
        else:
            res.chosen, res.alt_off, res.alt_group = np.zeros(K, np.uint32), np.zeros(K + 1, np.uint64), np.zeros(max(ng, 1), np.uint32)
            out = res.out_struct()
            _lib.check(self._L.hawk_host_effects(C.byref(self._cols), family, _p(sc), _p(cs), _p(ct), C.c_uint32(len(cs)), C.c_uint32(K), C.byref(out),
                                                 C.c_uint64(len(res.alt_group)), C.byref(nc), C.byref(na)), "hawk_host_effects")
            res.chosen, res.alt_off, res.alt_group = res.chosen[:nc.value], res.alt_off[:nc.value + 1], res.alt_group[:na.value]
        if self.perm is not None:  # back to the caller's group numbering
            res = _unpermute(res, self.perm)
        return res


def _unpermute(res: EffectsResult, perm: np.ndarray) -> EffectsResult:
    """arrays indexed by sorted position -> indexed by the caller's groups; group numbers inside them mapped the same way"""
    ng = len(perm)
    out = EffectsResult(ng)
    pm = perm.astype(np.uint32)

    def ids(a):
        a = np.asarray(a)
        r = np.full(a.shape, FX_NONE, dtype=np.uint32)
        ok = a != FX_NONE
        r[ok] = pm[a[ok]]
        return r
    for k in ("score", "delta", "abs_delta", "n_samples", "type", "dup", "pos_worst", "pos_nvalid", "pos_first_rank"):
        getattr(out, k)[perm] = getattr(res, k)
    out.position[perm] = ids(res.position)
    out.pos_ref[perm] = ids(res.pos_ref)
    out.chosen, out.alt_off, out.alt_group, out.counts = ids(res.chosen), res.alt_off, ids(res.alt_group), res.counts
    return out


def parse_candidate_ids(cgids: Sequence[str], debug: bool = True):
    """'chr_start_strand' (graphical_reports.py:434-438) -> (start, strand 0 / 1)"""
    out = []
    for cg in cgids:
        try:
            _, start, strand = cg.rsplit("_", 2)
            out.append((int(start), {"+": 0, "-": 1}[strand]))
        except (ValueError, KeyError) as e:
            exception_handler(CrisprHawkGraphicalReportsError, f"Forbidden candidate guide id ({cg})", os.EX_DATAERR, debug, e)
    return out


def _stage(groups_or_table, labels, order, engine, is_ref_hap=None) -> GroupEffects:
    samples = labels.samples if hasattr(labels, "samples") and not isinstance(labels, (list, tuple)) else [("" if h is None else h.samples) for h in labels]
    if is_ref_hap is None:
        is_ref_hap = labels.is_ref if hasattr(labels, "is_ref") and not isinstance(labels, (list, tuple)) else [s == "REF" for s in samples]
    return GroupEffects(groups_or_table, samples, is_ref_hap, order, engine)


def compute_delta_table(groups_or_table, labels, cgids: Sequence[str], score: str, engine: str = "device", columns=None,
                        scores: Optional[Dict[str, np.ndarray]] = None, is_ref_hap=None, stage: Optional[GroupEffects] = None, debug: bool = True):
    """The reference's _compute_delta_table (graphical_reports.py:857-881) as a pandas.DataFrame with its columns, column order,
    dtypes and NaN fill: guide_id, Rank, ref_sgRNA, pam, ref_score, ref_n_samples, then alt{i}_sgRNA / _pam / _score / _delta /
    _abs_delta / _n_samples / _variant_id up to the widest chosen position.

    `columns`: what reports.group_columns returned for the same groups - (cols, order, ...) - the report this table is about: its
    row order ranks the groups, and the strings of the chosen rows are taken from its columns.  `scores[score]` holds the
    unrounded score per group (score_cfdon defaults to the groups' CFDon).  `stage`: a GroupEffects made earlier for the same
    groups (one handle serves every score)."""
    import pandas as pd
    if columns is None:
        raise ValueError("columns: pass what reports.group_columns returned for these groups")
    family = score_family(score, debug)
    cols, order = columns[0], np.asarray(columns[1], dtype=np.int64)
    if len(cgids) > TOPK:
        exception_handler(CrisprHawkGraphicalReportsError, f"{len(cgids)} candidate guides: the delta table holds {TOPK} positions", os.EX_DATAERR, debug)
    cands = parse_candidate_ids(cgids, debug)
    own = stage is None
    if own:
        stage = _stage(groups_or_table, labels, order, engine, is_ref_hap)
    try:
        vals = None if (score == "score_cfdon" and not (scores and score in scores)) else (scores or {}).get(score)
        if vals is None and score != "score_cfdon":
            exception_handler(CrisprHawkGraphicalReportsError, f"No values for {score}", os.EX_DATAERR, debug)
        res = stage.rank(family, vals, cands, TOPK)
    finally:
        if own:
            stage.close()
    for cg, h in zip(cgids, res.chosen[:len(cgids)].tolist()):
        if h == FX_NONE:
            exception_handler(CrisprHawkGraphicalReportsError, f"Candidate guide {cg} has no reference guide in the report", os.EX_DATAERR, debug)
    chosen = res.chosen.astype(np.int64)
    if len(chosen) == 0:
        return pd.DataFrame({c: [] for c in ("guide_id", "Rank", "ref_sgRNA", "pam", "ref_score", "ref_n_samples")})
    refs = res.pos_ref[chosen].astype(np.int64)
    alts = res.alt_group.astype(np.int64)
    need = np.concatenate([refs, alts])
    from .reports import ConstCol, _col_take
    text = {c: (np.full(len(need), cols[c].text, dtype=object) if isinstance(cols[c], ConstCol) else np.asarray(_col_take(cols[c], need)))
            for c in ("chr", "start", "strand", "sgRNA_sequence", "pam", "variant_id")}
    at = {int(g): i for i, g in enumerate(need.tolist())}
    s = lambda c, g: str(text[c][at[g]])
    off = res.alt_off.astype(np.int64)
    max_alts = int(np.diff(off).max())
    rows = []
    for i, (h, r) in enumerate(zip(chosen.tolist(), refs.tolist())):
        row = {"guide_id": f"{s('chr', r)}_{s('start', r)}_{s('strand', r)}", "Rank": i + 1, "ref_sgRNA": s("sgRNA_sequence", r), "pam": s("pam", r),
               "ref_score": float(res.score[r]), "ref_n_samples": int(res.n_samples[r])}
        mine = alts[off[i]:off[i + 1]].tolist()
        for k in range(max_alts):
            pre = f"alt{k + 1}_"
            if k < len(mine):
                g = mine[k]
                vid = s("variant_id", g)
                row.update({pre + "sgRNA": s("sgRNA_sequence", g), pre + "pam": s("pam", g), pre + "score": float(res.score[g]),
                            pre + "delta": float(res.delta[g]), pre + "abs_delta": float(res.abs_delta[g]), pre + "n_samples": int(res.n_samples[g]),
                            pre + "variant_id": np.nan if vid == "NA" else vid})
            else:
                row.update({pre + k2: np.nan for k2 in ("sgRNA", "pam", "score", "delta", "abs_delta", "n_samples", "variant_id")})
        rows.append(row)
    return pd.DataFrame(rows)


def guide_type_counts(groups_or_table, labels, order, engine: str = "device", is_ref_hap=None, stage: Optional[GroupEffects] = None,
                      debug: bool = True) -> Dict[str, int]:
    """_count_guide_type(_assign_guide_type(_assign_extended_guide_ids(report))) (graphical_reports.py:149-175, 218-293): the
    report's distinct guides by type, keyed by the reference's four labels."""
    own = stage is None
    if own:
        stage = _stage(groups_or_table, labels, order, engine, is_ref_hap)
    try:
        if stage._fx is not None:
            counts = np.zeros(8, np.uint64)
            out = _lib.EffectsOut(**{"counts": _p(counts)})
            _lib.check(stage._L.hawk_effects_download(stage._fx, C.byref(out)), "hawk_effects_download")
        else:
            cf = stage._cols.cfdon
            counts = stage.rank(SIGNED, None if cf else np.zeros(stage.n_groups), (), 1).counts
    finally:
        if own:
            stage.close()
    if int(counts[4]):
        exception_handler(CrisprHawkGraphicalReportsError, f"Unknown guide type for {int(counts[4])} alternative guides without a lower-case base", os.EX_DATAERR, debug)
    return {label: int(counts[t]) for t, label in GUIDETYPES.items()}


def delta_table_tsv(df) -> str:
    return df.to_csv(sep="\t", index=False, na_rep="NA")


def compute_graphical_reports(groups_or_table, labels, columns, region, outdir: str, candidate_guides: Sequence = (), scores=None,
                              engine: str = "device", is_ref_hap=None, debug: bool = True) -> List[str]:
    """For one interval: figures/{contig}_{start}_{stop}_{score}_delta.tsv for every score column the report has a number in, and
    figures/{prefix}_guides_type.tsv - the reference's figures directory and prefix (graphical_reports.py:94-124, 884-900) with
    .tsv in place of .png.  `candidate_guides`: candidate_guides.CandidateGuide objects (those outside the region are skipped, as
    graphical_reports.py:434-438 skips them) or 'chr_start_strand' ids.  Returns the paths written."""
    figdir = create_figures_dir(outdir)
    prefix = format_region_prefix(region)
    cols, order = columns[0], np.asarray(columns[1], dtype=np.int64)
    cgids = []
    for cg in candidate_guides:
        if isinstance(cg, str):
            cgids.append(cg)
        elif cg.contig == region.contig and region.start + PADDING <= cg.position and cg.position + (cg.coordinate.stop - cg.coordinate.start) <= region.stop - PADDING:
            cgids.append(f"{cg.contig}_{cg.position}_{cg.strand}")
    paths = []
    stage = _stage(groups_or_table, labels, order, engine, is_ref_hap)
    try:
        from .reports import ConstCol
        for score in SCORES:
            if score not in _FAMILY or score not in cols or isinstance(cols[score], ConstCol):
                continue  # (a ConstCol score column is all "NA": no number to take a delta of)
            if stage.n_groups == 0:
                continue
            df = compute_delta_table(groups_or_table, labels, cgids, score, engine, columns, scores, is_ref_hap, stage, debug)
            path = os.path.join(figdir, f"{prefix}_{score}_delta.tsv")
            with open(path, "w") as f:
                f.write(delta_table_tsv(df))
            paths.append(path)
        counts = guide_type_counts(groups_or_table, labels, order, engine, is_ref_hap, stage, debug)
        path = os.path.join(figdir, f"{prefix}_guides_type.tsv")
        with open(path, "w") as f:
            f.write("guide_type\tcount\n" + "".join(f"{k}\t{v}\n" for k, v in counts.items()))
        paths.append(path)
    finally:
        stage.close()
    return paths
