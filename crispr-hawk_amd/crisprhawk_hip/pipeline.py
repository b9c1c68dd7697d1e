"""Files in, guide reports out: the path of `crisprhawk_search` (`crisprhawk.py:121-138`) for phased or variant-free
inputs, with every stage on the device path of this package.

    FASTA + BED (+ VCF)  --readers-->  region string, VCF record text
                         --hawk_gt_parse / hawk_gt_lists / hawk_xplan_create_gt-->  expansion plan in HBM
                         --hawk_search (+ CFDon)-->  guide table in HBM
                         --hawk_table_collapse-->  report groups
                         --hawk_annot_query-->  BED / gene annotation columns of the groups (optional)
                         --reports.report_frame-->  crisprhawk_guides__*.tsv
                         --hawk_xplan_text-->  haplotypes_table_*.tsv (optional: the plan's rows as text)

Only what the reference's search sub-command does between reading its inputs and writing the guide report is covered;
the non-CFDon scorers (model files) and the off-target stage have their own entry points (`scoring.py`, `offtargets.py`).
"""
import os
from typing import Dict, List, Optional

import numpy as np

from . import reports
from . import scoring
from .pam import CPF1, PAM, SPCAS9, XCAS9
from .readers import VCF, Bed, Fasta
from .utils import VERBOSITYLVL, print_verbosity
from .expand import HaplotypeBuildError
from .workload import HapInfo, RowLabel, expand_from_vcf, hap_labels

PADDING = 100  # region_constructor.py:21
ANN_STAGE = "BED / gene annotation of the groups (device join)"
HAPTAB_STAGE = "haplotypes table (rows as text from the plan + write)"


def _labels(ds, info: List[HapInfo], kept: List[int], vt) -> List[Optional[RowLabel]]:
    """RowLabel per device row: samples joined as collapse_haplotypes does, variant ids in the reference's order
    (SNVs by position, then indels: haplotype.py:234-242), allele frequencies by id, ids hap_<k> in list order."""
    out: List[Optional[RowLabel]] = [None] * ds.n_hap
    for k, (r, inf) in enumerate(zip(kept, info)):
        idx = [int(i) for i in inf.variant_idx]
        snv = [i for i in idx if len(vt.ref[i]) == len(vt.alt[i])]
        indel = [i for i in idx if len(vt.ref[i]) != len(vt.alt[i])]
        ids = [vt.id[i] for i in snv + indel]
        out[r] = RowLabel(",".join(inf.samples), ",".join(ids) if ids else "NA", {vt.id[i]: float(vt.af[i]) for i in idx},
                          f"hap_{k:08d}", ds.host_meta[r].seg)
    return out


def check_annotation_args(annotations, annotation_colnames, gene_annotations, gene_annotation_colnames) -> None:
    """The reference's checks of --annotation / --gene-annotation and their column names (crisprhawk_argparse.py:252-330), as
    ValueError: names without files, counts that differ, files that are missing or empty."""
    for files, names, what in ((annotations, annotation_colnames, "annotation"), (gene_annotations, gene_annotation_colnames, "gene annotation")):
        files, names = list(files or []), list(names or [])
        missing = [f for f in files if not os.path.isfile(f)]
        if missing:
            raise ValueError(f"Cannot find the specified {what} BED files {', '.join(missing)}")
        empty = [f for f in files if os.stat(f).st_size <= 0]
        if empty:
            raise ValueError(f"{', '.join(empty)} look empty")
        if names and not files:
            raise ValueError(f"{what.capitalize()} column names provided, but no input {what} file")
        if names and len(names) != len(files):
            raise ValueError(f"Mismatching number of {what} files and {what} column names")


class AnnotationSet:
    """The annotation files of one search_files call: opened once, one device table per (file, contig) made on first use and
    reused across BED intervals.  `columns(contig)` is what reports.group_columns / report_frame take as `annotations`."""

    def __init__(self, annotations, annotation_colnames, gene_annotations, gene_annotation_colnames, device, debug: bool,
                 inflate: Optional[str] = None):
        from .bedannot import FUNC, GENE, BedAnnotation
        self.device = device
        self.func = [BedAnnotation(f, 0, debug, inflate) for f in (annotations or [])]
        self.gene = [BedAnnotation(f, 0, debug, inflate) for f in (gene_annotations or [])]
        for b in self.func:
            b.require(FUNC)
        for b in self.gene:
            b.require(GENE)
        self.names = reports.annotation_colnames(len(self.func), annotation_colnames, len(self.gene), gene_annotation_colnames)
        self.func_names = list(annotation_colnames) if annotation_colnames else None  # the off-targets table's own default names
        self._kinds = [(b, FUNC) for b in self.func] + [(b, GENE) for b in self.gene]

    def __bool__(self) -> bool:
        return bool(self._kinds)

    def columns(self, contig: str, lap=None):
        """(starts, stops) -> {column: Ragged}; `lap` (search_files' stage clock) is charged with the join when given"""
        def join(starts, stops):
            if lap is not None:
                lap("host-built route: haplotypes, search, scoring, grouping")
            cols = {name: bed.table(contig, kind, self.device).query(starts, stops) for name, (bed, kind) in zip(self.names, self._kinds)}
            if lap is not None:
                lap(ANN_STAGE)
            return cols
        return join

    def close(self) -> None:
        for b, _ in self._kinds:
            b.close()


def _offtargets(spacers, pam: PAM, ot, coord, guidelen: int, right: bool, outdir: str, debug: bool):
    """--estimate-offtargets for one region: {SPACER: (count, global CFD)} + offtargets_{contig}_{start}_{stop}.tsv."""
    from .offtargets import estimate_offtargets_spacers, specificity_by_spacer
    if not ot.get("table", True):  # the report's two columns alone: summed per guide on the device, no site listed
        return specificity_by_spacer(spacers, pam, ot["genome"], ot["mm"], guidelen, right, debug, ot["bdna"], ot["brna"])
    ann = ot.get("ann")
    return estimate_offtargets_spacers(spacers, pam, ot["genome"], coord, ot["mm"], ot["bdna"], ot["brna"], guidelen, right, outdir, 0, debug,
                                       ann.func if ann else None, ann.func_names if ann else None, ann.device if ann else None,
                                       engine=ot.get("engine", "device"), **({"variants": True} if ot.get("variants") else {}))


def _plan_row_variants(info, vt) -> List[bytes]:
    """the `variants` label of every kept row of an expansion: the ids of what it carries in the reference's order (SNVs by
    position, then indels: haplotype.py:234-242), NA for REF"""
    out = []
    for inf in info:
        idx = [int(i) for i in inf.variant_idx]
        ids = [vt.id[i] for i in idx if len(vt.ref[i]) == len(vt.alt[i])] + [vt.id[i] for i in idx if len(vt.ref[i]) != len(vt.alt[i])]
        out.append((",".join(ids) if ids else "NA").encode("ascii"))
    return out


UNPHASED_REPORTS = (None, "groups", "objects")


def _search_host_built(coord, seq: str, vcf, phased: bool, pam: PAM, guidelen: int, right: bool, outdir: str, mm, pt, debug: bool,
                       ot=None, ann=None, lap=None, tables=None, unphased_engine=None, unphased_report=None, azimuth_model=None,
                       deepcpf1_weights=None, plm_on=False, fx=None, unphased_haplotypes="host", device=None,
                       unphased_indel_windows="host") -> str:
    """One BED interval with the haplotypes built on the host by the mirror of the reference's own construction
    (haplotypes.py:106-368 phased, 370-712 unphased) - the route of unphased VCFs (IUPAC haplotypes + indel windows; their
    windows resolved on the device table, search_guides.search's `unphased_engine`) and the fallback for phased records the device expansion
    declines (a chromosome copy carrying overlapping records, multi-base deletion alts).  The search itself still runs
    on the device.

    An unphased interval with records then takes `unphased_report` (None: HAWK_UNPHASED_REPORT, else "groups"):
      "groups"   the kept guides stay in HBM and become report groups there (GuideTable.resolve_unphased_groups: CFDon against
                 the REF guide, the report's key - widened to the scorers' k-mer when Azimuth or DeepCpf1 is on - one
                 representative and the member haplotypes per group); from the groups on it is the phased route's own code
                 (_group_report_columns: model scorers on the representatives, the annotation join, the off-target callback,
                 reports.group_columns, write_report_tsv).  No Guide object is built, and the report carries the model scores the
                 caller switched on.  Falls back to "objects" - with a line at verbosity level 3 that carries the status - when the
                 resolution declines, when any status other than a HIP failure comes back, or when `unphased_engine` (or
                 HAWK_UNPHASED_ENGINE) asks for the host.
      "objects"  the reference's order of business on Guide objects: annotate -> reverse_guides -> CFDon -> report
                 (reports.report_from_guides; the model-score columns say NA).  The phased fallback always takes it.
    `fx` (search_files' `unphased_effects=True` with `graphical_reports` / `candidate_guides`; unphased intervals with records
    only): the "groups" route keeps its groups in HBM and runs the variant-effect stage on them (_interval_effects, as
    _finish_interval does on a collapsed table).  Nothing else can serve the stage: "objects", the host engine, a resolution
    that declines or refuses are then a ValueError naming `graphical_reports`, raised before any file of the interval is written.
    The phased fallback never receives `fx`: there the stage stays a ValueError (_search_intervals).
    `unphased_haplotypes="device"` (unphased intervals): the whole-region rows are built on the device first (_unphased_device_built);
    where that route does not apply or declines, the interval is built here as if it had not been asked for."""
    if unphased_report not in UNPHASED_REPORTS:
        raise ValueError(f"unphased_report {unphased_report!r}: None, 'groups' or 'objects'")
    mode = unphased_report or os.environ.get("HAWK_UNPHASED_REPORT") or "groups"
    engine = unphased_engine or os.environ.get("HAWK_UNPHASED_ENGINE") or "device"
    if fx is not None and mode not in ("groups", "objects"):
        raise ValueError(f"HAWK_UNPHASED_REPORT={mode!r}: 'groups' or 'objects'")
    if fx is not None and (mode != "groups" or engine == "host"):
        why = f"unphased_report={mode!r} builds Guide objects" if mode != "groups" else "the host engine was asked for (unphased_engine / HAWK_UNPHASED_ENGINE)"
        raise ValueError(f"graphical_reports / candidate_guides on an unphased interval rank the report groups in device memory: {why}")
    if unphased_haplotypes == "device" and not phased:
        path = _unphased_device_built(coord, seq, vcf, pam, guidelen, right, outdir, mm, pt, debug, ot, ann, lap, tables, mode, engine,
                                      azimuth_model, deepcpf1_weights, plm_on, fx, device, unphased_indel_windows)
        if path is not None:
            return path
    from . import haplotypes as hap_mod
    from .annotation import reverse_guides
    from .haplotype import Haplotype
    from .region import Region
    from .search_guides import search
    from .sequence import Sequence
    region = Region(Sequence(seq, debug), coord)
    haps = [Haplotype(Sequence(seq, debug), region.coordinates, False, 0, debug)]
    records = vcf.fetch(coord)
    if records:
        build = hap_mod.add_variants_phased if phased else hap_mod.add_variants_unphased
        haps = build(haps, region, vcf.samples, records, phased, debug)
    for i, h in enumerate(haps):
        h.id = f"hap_{i:08d}"
    def write_table():
        if tables is not None:  # the strings are on the host already: the same writer, no kernel
            tables[str(coord)] = hap_mod.haplotypes_table(coord.contig, coord.start, coord.stop, outdir, [h.id for h in haps],
                                                          [h.variants for h in haps], [h.samples for h in haps],
                                                          sequences=[h.sequence.sequence for h in haps])
    if fx is None:  # (with the stage on, the table waits until the resolution has not refused: no file before a ValueError)
        write_table()
    if records and not phased:
        if mode not in ("groups", "objects"):
            raise ValueError(f"HAWK_UNPHASED_REPORT={mode!r}: 'groups' or 'objects'")
        if mode == "groups" and engine == "host":
            print_verbosity("Unphased report from Guide objects: the host engine was asked for", 0, VERBOSITYLVL[3])
        elif mode == "groups":
            path = _unphased_groups_report(coord, region, haps, pam, guidelen, right, outdir, mm, pt, debug, ot, ann, lap, azimuth_model,
                                           deepcpf1_weights, plm_on, fx, write_table)
            if path is not None:
                return path
    if fx is not None:
        raise ValueError("graphical_reports / candidate_guides: this interval's report comes from Guide objects, which leave no report groups "
                         "in device memory for the variant-effect stage")
    guides = search(pam, region, haps, None, guidelen, right, bool(records), phased, 0, debug, unphased_engine=unphased_engine)
    cfd = None
    if mm is not None:
        scoring.set_cfd_tables(mm, pt)
        windows = [g.sequence for g in guides]  # the report wants the + strand windows: keep them across the reversal
        rights = [g.right for g in guides]
        scored = scoring.cfdon_score(reverse_guides(list(guides), 0), 0, debug)
        val = {id(g): g.cfdon_score for g in scored}
        cfd = [float("nan") if val[id(g)] == "NA" else float(val[id(g)]) for g in guides]
        for g, w, r in zip(guides, windows, rights):  # undo the in-place reversal
            if g.strand == 1:
                g.reverse_complement()
            assert g.sequence == w and g.right == r
    bed_start, bed_stop = coord.start + PADDING, coord.stop - PADDING
    otmap = None
    if ot is not None:  # spacers as reverse_guides would leave them (annotation.py:27-51)
        from .utils import _RC_TRANS
        cores = [g.sequence[10:-10][::-1].translate(_RC_TRANS) if g.strand == 1 else g.sequence[10:-10] for g in guides]
        otmap = _offtargets([c[len(pam):] if right else c[:guidelen] for c in cores], pam, ot, coord, guidelen, right, outdir, debug)
    df = reports.report_from_guides(guides, haps, pam, coord.contig, f"{coord.contig}:{bed_start}-{bed_stop}", cfd, otmap,
                                    ann.columns(coord.contig, lap) if ann else None)
    path = os.path.join(outdir, reports.report_filename(coord.contig, bed_start, bed_stop, pam, guidelen))
    with open(path, "w") as f:
        f.write(reports.to_tsv(df))
    return path


UNPHASED_HAPLOTYPES = (None, "host", "device")
UNPHASED_INDEL_WINDOWS = (None, "host", "device")
HOST_BUILT_LAP = "host-built route: unphased haplotypes built on the host"
DEVICE_BUILT_LAP = "host-built route: unphased haplotypes built on the device"


def _unphased_device_built(coord, seq: str, vcf, pam: PAM, guidelen: int, right: bool, outdir: str, mm, pt, debug: bool, ot, ann, lap, tables,
                           mode: str, engine: str, azimuth_model, deepcpf1_weights, plm_on, fx, device, indel_windows: str = "host") -> Optional[str]:
    """An unphased interval with its whole-region rows built on the device (workload.expand_unphased_from_vcf) and the "groups"
    report made from that set, its labels and its allele table: no VariantRecord per line, no string per carrier.  None - with a
    line at verbosity level 3 that says why - where the route does not apply ("objects", the host engine, haplotype_table=True
    whose writer wants the strings), where the builder declines, and where the resolution declines or refuses: the caller then
    builds the interval on the host, which raises or succeeds as it always has.  An interval without records is the caller's too.
    `indel_windows="device"` builds the indel windows on the device too; where only that builder declines (HAWK_UBUILD_WINDOW,
    HAWK_UBUILD_INDEL_BASE, an indel's HAWK_UBUILD_REF) the interval is built once more with the windows on the host."""
    from ._lib import UnphasedBuildDeclined
    from .workload import expand_unphased_from_vcf
    why = None
    if mode != "groups":
        why = f"unphased_report={mode!r} builds Guide objects from Haplotype objects"
    elif engine == "host":
        why = "the host engine was asked for (unphased_engine / HAWK_UNPHASED_ENGINE)"
    elif tables is not None:
        why = "haplotype_table=True writes the table from the host-built strings"
    if why is not None:
        print_verbosity(f"Unphased haplotypes built on the host: {why}", 0, VERBOSITYLVL[3])
        if indel_windows == "device":
            print_verbosity("unphased_indel_windows='device' not used: the interval is built on the host", 0, VERBOSITYLVL[3])
        return None
    blk = vcf.fetch_block(coord)
    if len(blk) == 0:
        return None
    built = None
    if indel_windows == "device":
        try:
            built = expand_unphased_from_vcf(seq, coord.start, coord.stop, blk, vcf.samples, len(pam), device, coord=coord, debug=debug,
                                             indel_windows="device")
        except UnphasedBuildDeclined as e:  # one step down: the SNV rows on the device, the windows on the host
            print_verbosity(f"Unphased indel windows built on the host: the device builder declined: {e}", 0, VERBOSITYLVL[3])
    if built is None:
        try:
            built = expand_unphased_from_vcf(seq, coord.start, coord.stop, blk, vcf.samples, len(pam), device, coord=coord, debug=debug)
        except UnphasedBuildDeclined as e:
            print_verbosity(f"Unphased haplotypes built on the host: the device builder declined: {e}", 0, VERBOSITYLVL[3])
            return None
    return _unphased_groups_report(coord, None, None, pam, guidelen, right, outdir, mm, pt, debug, ot, ann, lap, azimuth_model, deepcpf1_weights,
                                   plm_on, fx, None, built=built)


def _unphased_groups_report(coord, region, haps, pam: PAM, guidelen: int, right: bool, outdir: str, mm, pt, debug: bool, ot, ann, lap,
                            azimuth_model, deepcpf1_weights, plm_on, fx=None, before_files=None, built=None) -> Optional[str]:
    """_search_host_built's "groups" route from the built haplotypes to the report file; None: the device declined or refused
    and the caller takes the object route.  With `fx` the groups stay in HBM for the variant-effect stage, a decline or refusal
    is a ValueError, and `before_files()` runs once the groups are made, ahead of the interval's first file.
    `built` (in place of `region` and `haps`): what workload.expand_unphased_from_vcf returned - the set is searched as it lies,
    the resolution reads its allele table and the report its row labels."""
    from ._lib import HawkStatusError
    from .search_guides import _device_set
    lap = lap or (lambda stage: None)
    if built is not None:
        lap(DEVICE_BUILT_LAP)
        ds, row_labels, haps = built[0], built[1], built[2]  # (`haps`: what resolve_unphased_groups reads, here the allele table)
    else:
        lap(HOST_BUILT_LAP)
        ds, row_labels = _device_set(region, haps, len(pam)), haps
    try:
        tab = ds.search(pam.bits, pam.bitsrc, len(pam), guidelen, right, download=False)
        azimuth_on = pam.cas_system in (SPCAS9, XCAS9) and azimuth_model is not None
        deepcpf1_on = pam.cas_system == CPF1 and deepcpf1_weights is not None
        resident = dict(keep_resident=True) if fx is not None and fx["on"] else {}  # candidates alone need only the columns
        try:
            groups = tab.resolve_unphased_groups(haps, pam, (mm, pt) if mm is not None else None,
                                                 (4, 3) if (azimuth_on or deepcpf1_on) else (0, 0), "device", **resident)
        except HawkStatusError as e:  # a decline (HawkResolveDeclined) or a refusal; a HIP failure is a HawkDeviceError and is raised
            if fx is not None:
                raise ValueError(f"graphical_reports / candidate_guides: the device made no report groups of this unphased interval ({e}), and "
                                 "the route over Guide objects leaves none in device memory for the variant-effect stage") from e
            print_verbosity(f"Unphased report from Guide objects: {e}", 0, VERBOSITYLVL[3])
            return None
        finally:
            tab.close()
        is_ref_hap = np.asarray(ds.is_ref, dtype=bool)
    finally:
        ds.close()
    try:  # (the resident groups own their memory: they outlive the table and the set)
        lap("host-built route: planes, search, resolution and report groups on the device")
        if before_files is not None:
            before_files()
        bed_start, bed_stop = coord.start + PADDING, coord.stop - PADDING
        labels = reports.HapLabels.from_objects(row_labels)
        cols, order, plain, scores = _group_report_columns(coord, groups, labels, is_ref_hap, pam, guidelen, right, outdir, mm is not None, debug, ot,
                                                           ann, azimuth_on, deepcpf1_on, plm_on, bed_start, bed_stop, lap)
        if fx is not None:
            _interval_effects(coord, groups if fx["on"] else None, labels, is_ref_hap, cols, order, plain, scores, pam, guidelen, outdir, debug,
                              bed_start, bed_stop, fx, lap)
    finally:
        groups.close()
    return _write_group_report(coord, cols, order, plain, pam, guidelen, outdir, bed_start, bed_stop, lap)


def _group_report_columns(coord, groups, labels, is_ref_hap, pam, guidelen, right, outdir, score, debug, ot, ann, azimuth_on, deepcpf1_on, plm_on,
                          bed_start, bed_stop, lap):
    """Report groups (hapset.GroupTable of a collapsed table, hapset.UnphasedGroups) -> the report as columns: model scorers on the
    representatives, the annotation join, the off-target callback, reports.group_columns.  -> (cols, order, plain, scores)"""
    # model-based scorers run once per report row, on the group representatives (scoring.py:749-813), when the
    # caller has supplied their parameters
    scores = {}
    if groups.n_groups and (azimuth_on or deepcpf1_on or plm_on):
        kmers = reports.group_kmers(groups)
        if azimuth_on:
            scores["score_azimuth"] = np.asarray(scoring.azimuth(kmers, debug), dtype=np.float64)
        if deepcpf1_on:
            scores["score_deepcpf1"] = np.asarray(scoring.deepcpf1(kmers, debug), dtype=np.float64)
        if plm_on:  # guide + PAM of the 4 + 23 + 3 k-mer (left-PAM systems only reach here)
            scores["score_plmcrispr"] = np.asarray(scoring.plmcrispr([k[4:27] for k in kmers], pam.cas_system, debug), dtype=np.float64)
    anncols = None
    if ann:  # one join per file over the groups' (start, stop), while the table is closed and before the report's own threads start
        anncols = ann.columns(coord.contig)(np.asarray(groups.start, dtype=np.int64), np.asarray(groups.stop, dtype=np.int64))
        lap(ANN_STAGE)
    otcb = None if ot is None else (lambda spacers: _offtargets(spacers, pam, ot, coord, guidelen, right, outdir, debug))
    # the report as columns (no Python string per row: the carriers' columns of a 2504-sample panel are 0.6 GB of text), written
    # by the library's TSV writer
    cols, order, plain = reports.group_columns(groups, labels, pam, coord.contig, f"{coord.contig}:{bed_start}-{bed_stop}", scores, score,
                                               is_ref_hap=is_ref_hap, offtargets=otcb, annotations=anncols)
    lap("report assembly")
    return cols, order, plain, scores


def _write_group_report(coord, cols, order, plain, pam, guidelen, outdir, bed_start, bed_stop, lap) -> str:
    path = os.path.join(outdir, reports.report_filename(coord.contig, bed_start, bed_stop, pam, guidelen))
    reports.write_report_tsv(path, cols, order, plain)
    lap("TSV text + write")
    return path


# Everything behind `outdir` is to be passed by keyword: new options are inserted where they belong (graphical_reports,
# candidate_guides, figures, unphased_report, unphased_engine, unphased_effects, unphased_haplotypes, unphased_indel_windows and offtargets_variants sit before `annotations`), and only the order of the last three parameters is held fixed.
def search_files(fasta: str, bedfile: str, vcfs: List[str], pam_seq: str, guidelen: int, right: bool, outdir: str,
                 cfd_tables=None, azimuth_model=None, deepcpf1_weights=None, plmcrispr_model=None,
                 device: Optional[int] = None, debug: bool = True, estimate_offtargets=None, mm: int = 4, bdna: int = 0, brna: int = 0,
                 timings: Optional[Dict[str, float]] = None, offtargets_table: bool = True, offtargets_summary: bool = False,
                 graphical_reports: bool = False,
                 candidate_guides: Optional[List[str]] = None, figures: Optional[Dict[str, List[str]]] = None,
                 unphased_report: Optional[str] = None, unphased_engine: Optional[str] = None, unphased_effects: bool = False,
                 unphased_haplotypes: Optional[str] = None, unphased_indel_windows: Optional[str] = None, bgzf_inflate: Optional[str] = None,
                 offtargets_variants=None, annotations: Optional[List[str]] = None,
                 annotation_colnames: Optional[List[str]] = None, gene_annotations: Optional[List[str]] = None,
                 gene_annotation_colnames: Optional[List[str]] = None, haplotype_table: bool = False,
                 tables: Optional[Dict[str, str]] = None) -> Dict[str, str]:
    """One report per BED interval; returns {str(coordinate): path}.  `cfd_tables = (mm[20,4,4], pam[16])` adds the
    CFDon column for SpCas9-class PAMs (scoring.py:352-387); `azimuth_model` (a fitted sklearn GBR or the flattened
    dict of scoring.azimuth_model_from_sklearn) and `deepcpf1_weights` (scoring.set_deepcpf1_weights layout) switch
    their score columns on - the reference reads those parameters from files it downloads.  `plmcrispr_model` (keyword only in
    practice, like everything behind `outdir`): a pair (state_dict by name, {cas_system: (L, 1280) embedding}) as
    scoring.set_plmcrispr_model takes them, or True for the model that is already set; for SpCas9 / xCas9-class PAMs it fills
    `score_plmcrispr` for the group representatives (their guide + PAM 23-mers), and guidelen + len(pam) != 23 is a
    CrisprHawkPlmCrisprScoreError before any search - the reference fails on every such run.  `estimate_offtargets` (the
    reference's --estimate-offtargets with its --crispritz-index: a genome.GenomeIndex, a {contig: sequence} dict or a
    FASTA path) runs the off-target stage per region: the `offtargets` / `cfd` columns of the guide report
    (reports.py:292-333, 612-660) and offtargets_{contig}_{start}_{stop}.tsv next to it (offtargets.py:486-558); `mm`,
    `bdna`, `brna` as on the reference's command line (bulges of up to 2 bases).  The per-site CFD needs `cfd_tables`.
    `offtargets_table=False` fills the two columns from the device's per-guide summary (offtargets.specificity_by_spacer)
    and writes no offtargets_*.tsv; it is mismatch-only, so asking for it with `bdna` or `brna` is a ValueError.
    `offtargets_summary=True` takes the same summary route at the given `bdna` / `brna` - the bulged rows are counted and their
    CFD summed inside the bulge kernel (GenomeIndex.summary(bdna=, brna=)) - and writes no offtargets_*.tsv either;
    `offtargets_table` is then not consulted.
    `offtargets_variants` makes the off-target stage variant-aware: True adds the SNVs of `vcfs` to the genome index, a list of
    VCF paths or (contig, pos0, ref, alt) records adds those (GenomeIndex.add_variants: sites only, genotypes and phasing are
    not consulted - every allele is taken to exist, an upper bound), and the sites only an ALT allele makes
    (GenomeIndex.variant_arrays) join the rows of offtargets_*.tsv, which gains the columns `origin` (ref / alt) and
    `variant_id`; the `offtargets` / `cfd` columns of the guide report include them.  The variant pass is mismatch-only and
    listed: with `bdna` / `brna`, `offtargets_table=False`, `offtargets_summary=True` or without `estimate_offtargets` it is a
    ValueError before any file is written.  None / False: nothing changes, no new column, no new call.
    `annotations` / `gene_annotations` (the reference's --annotation / --gene-annotation BED files, plain, gzip or BGZF, no .tbi
    needed) add one column per file to every guide report - the 4th BED column, or feature:gene_name, of the features a guide
    overlaps - named by `annotation_colnames` / `gene_annotation_colnames` or annotation_{i} / gene_annotation_{i}; the
    `annotations` files also annotate the rows of offtargets_*.tsv.  The join runs on the device (bedannot.AnnotTable).
    `haplotype_table=True` (the reference's --haplotype-table, haplotypes.py:818-859) also writes
    haplotypes_table_{contig}_{start}_{stop}.tsv per BED interval (padded coordinates): id, haplotype, variants, samples of every
    haplotype searched, REF first, `id` being the guide report's haplotype_id.  The strings of a device-built plan are fetched
    as text in batches (haplotypes.haplotypes_table; HAWK_HAPTEXT_BATCH_BYTES, default 256 MiB).  The returned dict stays
    {str(coordinate): report path}; pass a dict as `tables` and it is filled in place with {str(coordinate): table path}.
    `graphical_reports=True` (the data behind the reference's --graphical-reports; no plot is drawn) runs the variant-effect stage
    on the collapsed table while it is still in HBM (graphical_reports.py: hawk_effects_*) and writes, per interval,
    figures/{contig}_{start}_{stop}_{score}_delta.tsv for every score column with numbers in it and
    figures/{contig}_{start}_{stop}_guides_type.tsv; `candidate_guides` ('contig:position:strand' strings, the reference's
    --candidate-guides) are forced into the delta tables and each gets its sub-report
    crisprhawk_candidate_guides__{contig}_{position}_{pam}_{guidelen}.tsv (candidate_guides.subset_reports).  Pass a dict as
    `figures` and it is filled with {str(coordinate): [paths]}.  Intervals whose haplotypes are built on the host (unphased
    VCFs, records the device expansion declines) have no device table: asking for the stage there is a ValueError - unless
    `unphased_effects=True`, which runs the stage of an unphased interval on its report groups while they are still in HBM
    (the "groups" route below with the groups kept resident; hawk_effects_create_ugroups) and writes the same files as for a
    phased interval, model-score delta tables included.  The stage then needs that route: `unphased_report="objects"`, the host
    engine, or a resolution the device declines or refuses (the message carries the status) is a ValueError naming
    `graphical_reports`, raised before any file of that interval is written.  An unphased VCF without a record in the interval
    takes the variant-free device route: report and figures of a run without a VCF.  Records of a phased VCF that the device
    expansion declines keep the ValueError.
    `unphased_report` (unphased VCFs; None reads HAWK_UNPHASED_REPORT, else "groups"): "groups" turns the resolved guides into
    report groups on the device and writes the report through the phased route's column writer - no Guide object, and the
    model-score columns (`azimuth_model`, `deepcpf1_weights`, `plmcrispr_model`) are filled as in a phased report; "objects" is
    the route over Guide objects and pandas, whose model-score columns say NA (_search_host_built).  `unphased_engine` as
    search_guides.search takes it; "host" implies the object route.
    `unphased_haplotypes` (unphased VCFs; None reads HAWK_UNPHASED_HAPLOTYPES, else "host"): "host" builds every haplotype of an
    interval in Python (haplotypes.add_variants_unphased); "device" builds the whole-region SNV rows from the genotype text on
    the device (workload.expand_unphased_from_vcf; the indel windows stay on the host builder) for an interval with records on
    the "groups" route with the device engine - `unphased_effects=True` works on top of it - and writes the same files.
    "objects", the host engine and `haplotype_table=True` (whose writer wants the strings) build that interval on the host, as
    does an interval the device builder declines (a malformed or haploid genotype, a multi-base substitution, a base outside
    A/C/G/T, a ref base the sequence does not hold, an SNV outside the region, an alt one sample carries twice at a position):
    the host builder then raises or succeeds exactly as under "host".  A line at verbosity level 3 says why.
    `unphased_indel_windows` (None reads HAWK_UNPHASED_INDEL_WINDOWS, else "host"): under "device" the 201-nt indel
    windows of such an interval are built on the device as well (hawk_uwin_*: no VariantRecord, no Haplotype, no row string).  It
    takes effect only where `unphased_haplotypes="device"` does; elsewhere a line at verbosity level 3 says it was not used.  Where
    the window builder declines (an indel that does not fit its window, an indel base outside A/C/G/T, an indel ref the row does not
    hold) the interval is rebuilt one step down - device SNV rows, host windows - with a level-3 line naming reason and variant;
    if that declines too, the host builder takes over as above.
    `bgzf_inflate` (None reads HAWK_BGZF_INFLATE, else "zlib"): who inflates the members of bgzipped VCF and annotation files -
    "zlib" on this thread, "native" the library's host decoder, "device" its kernel (readers._TextSource); the text, and so every
    output, is the same on all three.  (Everything from `timings` on is meant to be passed by keyword.)"""
    from .readers import inflate_route
    bgzf_inflate = inflate_route(bgzf_inflate)
    if unphased_report not in UNPHASED_REPORTS:
        raise ValueError(f"unphased_report {unphased_report!r}: None, 'groups' or 'objects'")
    if unphased_haplotypes not in UNPHASED_HAPLOTYPES:
        raise ValueError(f"unphased_haplotypes {unphased_haplotypes!r}: None, 'host' or 'device'")
    builder = unphased_haplotypes or os.environ.get("HAWK_UNPHASED_HAPLOTYPES") or "host"
    if builder not in ("host", "device"):
        raise ValueError(f"HAWK_UNPHASED_HAPLOTYPES={builder!r}: 'host' or 'device'")
    if unphased_indel_windows not in UNPHASED_INDEL_WINDOWS:
        raise ValueError(f"unphased_indel_windows {unphased_indel_windows!r}: None, 'host' or 'device'")
    windows = unphased_indel_windows or os.environ.get("HAWK_UNPHASED_INDEL_WINDOWS") or "host"
    if windows not in ("host", "device"):
        raise ValueError(f"HAWK_UNPHASED_INDEL_WINDOWS={windows!r}: 'host' or 'device'")
    if windows == "device" and builder != "device":
        print_verbosity("unphased_indel_windows='device' not used: it builds behind unphased_haplotypes='device'", 0, VERBOSITYLVL[3])
    import time as _time
    check_annotation_args(annotations, annotation_colnames, gene_annotations, gene_annotation_colnames)
    _t = [_time.perf_counter()]

    def lap(stage: str) -> None:  # stage seconds into `timings` (bench.py's files_to_tsv line); no-op without it
        if timings is not None:
            now = _time.perf_counter()
            timings[stage] = timings.get(stage, 0.0) + now - _t[0]
            _t[0] = now
    if not offtargets_summary and not offtargets_table and (bdna or brna):
        raise ValueError("offtargets_table=False is the mismatch-only summary: bulged sites (bdna / brna) need the off-targets table, "
                         "or offtargets_summary=True for the two report columns alone")
    ot_variants = offtargets_variants is not None and offtargets_variants is not False
    if ot_variants:
        if estimate_offtargets is None:
            raise ValueError("offtargets_variants needs the off-target stage: estimate_offtargets is None")
        if bdna or brna:
            raise ValueError("offtargets_variants is mismatch-only: bulges over ALT alleles (bdna / brna) are not enumerated")
        if offtargets_summary or not offtargets_table:
            raise ValueError("offtargets_variants lists its rows: offtargets_table=False / offtargets_summary=True sum the plain scan alone")
        if offtargets_variants is True and not vcfs:
            raise ValueError("offtargets_variants=True takes the SNVs of `vcfs`, and none were given")
    ot = None
    if estimate_offtargets is not None:
        from .genome import GenomeIndex, read_fasta
        genome = estimate_offtargets
        if isinstance(genome, (str, os.PathLike)):
            genome = read_fasta(str(genome))
        if isinstance(genome, dict):
            genome = GenomeIndex(genome, guidelen, len(pam_seq), device=device, max_bulge=bdna)  # once for all regions
        ot = dict(genome=genome, mm=mm, bdna=bdna, brna=brna, table=bool(offtargets_table) and not offtargets_summary)
        if ot_variants:
            genome.add_variants(list(vcfs) if offtargets_variants is True else offtargets_variants)
            ot["variants"] = True
        if cfd_tables is not None:
            scoring.set_cfd_tables(*cfd_tables)
    if azimuth_model is not None:
        scoring.set_azimuth_model(azimuth_model)
    if deepcpf1_weights is not None:
        scoring.set_deepcpf1_weights(deepcpf1_weights)
    pam = PAM(pam_seq, right, debug)
    pam.encode(0)
    plm_on = plmcrispr_model is not None and plmcrispr_model is not False and pam.cas_system in (SPCAS9, XCAS9)
    if plm_on:
        if guidelen + len(pam_seq) != 23:
            from .crisprhawk_error import CrisprHawkPlmCrisprScoreError
            from .exception_handlers import exception_handler
            exception_handler(CrisprHawkPlmCrisprScoreError, f"PLM-CRISPR scores guide + PAM of 23 nt, got {guidelen} + {len(pam_seq)}",
                              os.EX_DATAERR, debug)
        if plmcrispr_model is not True:
            scoring.set_plmcrispr_model(*plmcrispr_model)
    fa = Fasta(fasta, 0, debug)
    fastas = {fa.contig: fa}
    vcf_by_contig = {}
    for f in vcfs or []:
        v = VCF(f, 0, debug, inflate=bgzf_inflate)
        vcf_by_contig[v.contig] = v
    score = cfd_tables is not None and pam.cas_system in (SPCAS9, XCAS9) and not right
    mmt, pt = cfd_tables if score else (None, None)
    os.makedirs(outdir, exist_ok=True)
    paths = {}
    if haplotype_table and tables is None:
        tables = {}
    if not haplotype_table:
        tables = None
    lap("open inputs (FASTA index, VCF header + line index)")
    ann = None
    if annotations or gene_annotations:
        ann = AnnotationSet(annotations, annotation_colnames, gene_annotations, gene_annotation_colnames, device, debug, bgzf_inflate)
        if ot is not None:
            ot["ann"] = ann
        lap("open annotation BED files")
    fx = None
    if graphical_reports or candidate_guides:
        from .candidate_guides import initialize_candidate_guides
        fx = dict(on=bool(graphical_reports), cgs=initialize_candidate_guides(list(candidate_guides or []), guidelen, debug),
                  figures=figures if figures is not None else {})
    try:
        return _search_intervals(Bed(bedfile, PADDING, debug), fastas, vcf_by_contig, pam, guidelen, right, outdir, score, mmt, pt, device, debug, ot,
                                 ann, azimuth_model, deepcpf1_weights, paths, lap, tables, fx, plm_on, unphased_report, unphased_engine,
                                 bool(unphased_effects), builder, windows)
    finally:
        if ann is not None:
            ann.close()


def _search_intervals(bed, fastas, vcf_by_contig, pam, guidelen, right, outdir, score, mmt, pt, device, debug, ot, ann, azimuth_model,
                      deepcpf1_weights, paths, lap, tables=None, fx=None, plm_on=False, unphased_report=None, unphased_engine=None,
                      unphased_effects=False, unphased_haplotypes="host", unphased_indel_windows="host") -> Dict[str, str]:
    """search_files' loop over the BED intervals."""
    stage_on = fx is not None and (fx["on"] or bool(fx["cgs"]))

    def no_table(unphased=False):
        if stage_on:
            raise ValueError("graphical_reports / candidate_guides: this interval's haplotypes are built on the host, so there is no collapsed "
                             "table on the device for the variant-effect stage" +
                             (" (unphased_effects=True runs it on the unphased report groups in device memory)" if unphased else ""))
    for coord in bed:
        seq = fastas[coord.contig].fetch(coord).sequence
        v = vcf_by_contig.get(coord.contig)
        if v is not None and not v.phased and stage_on and unphased_effects and not v.fetch(coord):
            v = None  # no record in the interval: REF alone, the variant-free device route and its collapsed table
        if v is not None and not v.phased:
            if not unphased_effects:
                no_table(True)
            paths[str(coord)] = _search_host_built(coord, seq, v, False, pam, guidelen, right, outdir, mmt if score else None,
                                                   pt if score else None, debug, ot, ann, lap, tables, unphased_engine, unphased_report,
                                                   azimuth_model, deepcpf1_weights, plm_on, fx if stage_on else None, unphased_haplotypes, device,
                                                   unphased_indel_windows)
            continue
        from .readers import VcfBlock
        blk = v.fetch_block(coord) if v is not None else VcfBlock(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint64), [])
        samples = v.samples if v is not None else []
        lap("fetch region + VCF record text")
        try:
            ds, info, _, kept, vt = expand_from_vcf(seq, coord.start, coord.stop, blk, samples, len(pam), True, device, keep_plan=True)
        except HaplotypeBuildError:
            # records the device expansion does not take (overlapping records on one chromosome copy, deletions with a
            # multi-base alt): the host builder mirrors the reference's own construction, the search stays on the device
            no_table()
            paths[str(coord)] = _search_host_built(coord, seq, v, True, pam, guidelen, right, outdir, mmt if score else None,
                                                   pt if score else None, debug, ot, ann, lap, tables)
            continue
        # the search runs from the expansion plan (hawk_xplan_view: once per distinct cluster of neighbouring variants when the
        # panel shares them, per row otherwise; no planes read) - a region without variants has no plan and searches REF's planes
        lap("genotype parse + plan on the device")
        plan = getattr(ds, "plan", None)
        target = plan.view() if plan is not None else ds
        tab = target.search(pam.bits, pam.bitsrc, len(pam), guidelen, right, mmt, pt, download=False)
        labels = hap_labels(coord.contig, vt, ds, info, kept)
        bed_start, bed_stop = coord.start + PADDING, coord.stop - PADDING  # reports.py:1036-1041
        # With a model scorer on, the reference's groupby includes its score column (reports.py:978-1003): rows that
        # differ only in the 4 + 3 flanking bases the scorer reads stay separate, so the device groups on the k-mer.
        azimuth_on = pam.cas_system in (SPCAS9, XCAS9) and azimuth_model is not None
        deepcpf1_on = pam.cas_system == CPF1 and deepcpf1_weights is not None
        tab.collapse((4, 3) if (azimuth_on or deepcpf1_on) else (0, 0), download_perm=False)
        groups = tab.export_groups()
        keep_table = fx is not None and fx["on"]  # the effects stage ranks the table's groups in HBM; candidates alone need only the columns
        if not keep_table:
            tab.close()
        lap("dictionary + search + collapse + export of the groups")
        try:
            _finish_interval(coord, tab if keep_table else None, groups, ds, plan, labels, info, vt, kept, seq, pam, guidelen, right, outdir, score, debug, ot, ann,
                             azimuth_on, deepcpf1_on, bed_start, bed_stop, paths, lap, tables, fx, plm_on)
        finally:
            if keep_table:
                tab.close()
    return paths


def _interval_effects(coord, resident, labels, is_ref_hap, cols, order, plain, scores, pam, guidelen, outdir, debug, bed_start, bed_stop, fx,
                      lap) -> None:
    """The variant-effect stage of one interval, by the report's row order: delta and type tables from `resident` - the collapsed
    table of a phased interval or the resident report groups of an unphased one, still in HBM; None when only candidates were
    asked for - and the candidates' sub-reports from the report's columns.  Fills fx["figures"]."""
    from . import candidate_guides as cg_mod, graphical_reports as gr_mod
    made = []
    if resident is not None:
        made += gr_mod.compute_graphical_reports(resident, labels, (cols, order, plain), coord, outdir, fx["cgs"], scores, is_ref_hap=is_ref_hap,
                                                 debug=debug)
    if fx["cgs"]:
        from .coordinate import Coordinate
        made += list(cg_mod.subset_reports(fx["cgs"], {Coordinate(coord.contig, bed_start, bed_stop, 0): (cols, order, plain)}, pam, guidelen,
                                           outdir, debug).values())
    fx["figures"][str(coord)] = made
    lap("variant effects: delta, type and candidate tables")


def _finish_interval(coord, tab, groups, ds, plan, labels, info, vt, kept, seq, pam, guidelen, right, outdir, score, debug, ot, ann, azimuth_on, deepcpf1_on,
                     bed_start, bed_stop, paths, lap, tables, fx, plm_on=False) -> None:
    """One interval from its exported groups to its files: scorers, annotation join, report, the optional tables.  `tab`: the
    collapsed table, still in HBM, when the variant-effect stage is on (the caller closes it whatever happens here)."""
    if True:
        cols, order, plain, scores = _group_report_columns(coord, groups, labels, np.asarray(ds.is_ref, dtype=bool), pam, guidelen, right, outdir, score,
                                                           debug, ot, ann, azimuth_on, deepcpf1_on, plm_on, bed_start, bed_stop, lap)
        if fx is not None:  # the table is still collapsed in HBM: the effects stage ranks its groups there, by the report's row order
            _interval_effects(coord, tab, labels, np.asarray(ds.is_ref, dtype=bool), cols, order, plain, scores, pam, guidelen, outdir, debug,
                              bed_start, bed_stop, fx, lap)
        if tables is not None:  # the plan's metadata is finished; its rows as text, batch by batch, straight into the file
            from . import haplotypes as hap_mod
            hap_ids, hap_samples = [labels.ids[r] for r in kept], [labels.samples[r] for r in kept]
            if plan is not None:
                tables[str(coord)] = hap_mod.haplotypes_table(coord.contig, coord.start, coord.stop, outdir, hap_ids, _plan_row_variants(info, vt),
                                                              hap_samples, plan=plan, rows=kept)
            else:  # no variants: REF alone, upper case as the reference's REF haplotype (sequence.py:49)
                tables[str(coord)] = hap_mod.haplotypes_table(coord.contig, coord.start, coord.stop, outdir, hap_ids, ["NA"], hap_samples,
                                                              sequences=[seq.upper()])
            lap(HAPTAB_STAGE)
        if plan is not None:
            plan.close()
        ds.close()
        lap("report assembly")
        paths[str(coord)] = _write_group_report(coord, cols, order, plain, pam, guidelen, outdir, bed_start, bed_stop, lap)
