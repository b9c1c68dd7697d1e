"""Off-target estimation — the reference's offtargets.py with the external CRISPRitz search
(offtargets.py:222-293) replaced by the K7 GPU scan over a GenomeIndex, and the per-site CFD
(offtargets.py:328-363) computed in one GPU batch.  The scan's hits are rendered as
CRISPRitz-format report lines so that ``Offtarget`` parsing, the per-guide counts and the global
CFD ``100 / (100 + sum(cfd))`` (offtargets.py:561-627) keep the reference's semantics.
When only the guide report's two columns are wanted (``pipeline.search_files(offtargets_table=False)``, or
``offtargets_summary=True`` at any ``bdna`` / ``brna``), ``specificity_by_spacer`` takes them from ``GenomeIndex.summary``: the
match kernels and the bulge kernel sum, per guide, the rows and their CFD rounded to 4 decimals as integers, and no site is
listed, rendered, parsed or scored on the host.
With `annotations` the off-targets table gets one column per BED file (offtargets.py:407-483), joined on the device
(bedannot.AnnotTable: one handle per file and contig of the table).  Elevation is out of scope.
``estimate_offtargets_spacers`` - the stage as ``pipeline.search_files`` runs it - keeps the hits as columns from the scan to the
file by default (``engine="device"``: ``GenomeIndex.offtarget_arrays`` / ``rows_text``, the rows' CFD and text written by
``hawk_offtarget_text``); the route over one ``Offtarget`` per site is its ``engine="objects"`` and what ``search`` /
``report_offtargets`` / ``estimate_offtargets``, the reference's signatures, run."""
import os
from typing import Dict, List, Set

import numpy as np

from .crisprhawk_error import CrisprHawkOffTargetsError
from .exception_handlers import exception_handler
from .genome import GenomeIndex, OffTargetHit
from .guide import Guide
from .offtarget import Offtarget
from .pam import PAM, SPCAS9, XCAS9
from .region import Region
from .utils import VERBOSITYLVL, print_verbosity

PADDING = 100
OTREPCNAMES = ["chrom", "position", "strand", "grna", "spacer", "pam", "mm", "bulge_size", "bulg_type", "cfd", "elevation"]


def _filter_guides(guides: List[Guide]) -> Set[str]:
    return {g.guide.upper() for g in guides}


def crispritz_report_line(hit: OffTargetHit, guide: str, pamlen: int, right: bool) -> str:
    """One `targets.txt` row: bulge type, crRNA, DNA (mismatches lower-case), chrom, position,
    cluster position, strand, mismatches, bulge size, total (offtarget.py:89-101)."""
    glen = len(guide)
    sp = hit.window[pamlen:] if right else hit.window[:glen]
    pm = hit.window[:pamlen] if right else hit.window[glen:]
    dna_sp = "".join(t if t == g else t.lower() for t, g in zip(sp, guide))
    crrna = ("N" * pamlen + guide) if right else (guide + "N" * pamlen)
    dna = (pm + dna_sp) if right else (dna_sp + pm)
    return f"X\t{crrna}\t{dna}\t{hit.contig}\t{hit.position}\t{hit.position}\t{hit.strand}\t{hit.mm}\t0\t{hit.mm}"


def crispritz_bulge_line(hit, pamlen: int, right: bool) -> str:
    """The `targets.txt` row of a bulged site (genome.BulgeHit): type DNA / RNA, crRNA and DNA with '-' at the bulge positions
    (the field set offtarget.py:77-101 reads; `total` = mismatches + bulge size)."""
    crrna = ("N" * pamlen + hit.crrna) if right else (hit.crrna + "N" * pamlen)
    dna = (hit.pam + hit.dna) if right else (hit.dna + hit.pam)
    return (f"{hit.bulge_type}\t{crrna}\t{dna}\t{hit.contig}\t{hit.position}\t{hit.position}\t{hit.strand}\t{hit.mm}\t{hit.bulge_size}\t"
            f"{hit.mm + hit.bulge_size}")


def search(genome: GenomeIndex, guides_seqs: List[str], pam: PAM, right: bool, mm: int, verbosity: int, debug: bool,
           bdna: int = 0, brna: int = 0) -> List[str]:
    """The CRISPRitz call's replacement (`crispritz.py search ... -mm M -bDNA B -bRNA R`, offtargets.py:264-268): report lines
    for every hit of every unique spacer - the un-bulged sites, then the DNA- / RNA-bulged ones (genome.GenomeIndex.scan_bulges with
    engine="device", the placement chosen per (site, guide) in k_ot_bulge: bulges of up to 2 bases, one row per (guide, site, type, size); CRISPRitz itself is absent, so its output beyond the field
    set the reference parses is unpinned)."""
    if bdna < 0 or brna < 0 or bdna > 2 or brna > 2:
        exception_handler(CrisprHawkOffTargetsError, f"DNA / RNA bulges of 0..2 bases are enumerated (got {bdna} / {brna})", os.EX_DATAERR, debug)
    try:
        hits = genome.scan(guides_seqs, pam, right, mm)
        bulged = genome.scan_bulges(guides_seqs, pam, right, mm, bdna, brna, engine="device") if (bdna or brna) else []
    except ValueError as e:
        exception_handler(CrisprHawkOffTargetsError, f"Off-targets search failed: {e}", os.EX_DATAERR, debug, e)
    return [crispritz_report_line(h, guides_seqs[h.guide], len(pam), right) for h in hits] + \
        [crispritz_bulge_line(h, len(pam), right) for h in bulged]


def _compute_cfd_score(offtargets: List[Offtarget], verbosity: int, debug: bool) -> List[Offtarget]:
    from .scoring import compute_cfd_batch
    print_verbosity(f"Computing CFD score for {len(offtargets)} off-targets", verbosity, VERBOSITYLVL[3])
    if offtargets:
        wt, sg, pm = zip(*(ot.cfd_inputs() for ot in offtargets))
        for ot, s in zip(offtargets, compute_cfd_batch(list(wt), list(sg), list(pm), debug).tolist()):
            ot.set_cfd(float(s))
    return offtargets


def _read_offtargets(crispritz_targets, pam: PAM, right: bool, debug: bool) -> List[Offtarget]:
    """offtargets.py:296-325.  `crispritz_targets`: the path of a CRISPRitz `*.targets.txt` (first line = header,
    skipped) or the scan's report lines themselves."""
    try:
        if isinstance(crispritz_targets, (str, os.PathLike)):
            with open(crispritz_targets) as infile:
                infile.readline()
                return [Offtarget(line, pam.pam, right, debug) for line in infile]
        return [Offtarget(line, pam.pam, right, debug) for line in crispritz_targets]
    except Exception as e:
        exception_handler(CrisprHawkOffTargetsError, f"Failed retrieving CRISPRitz off-targets in {crispritz_targets}", os.EX_DATAERR, debug, e)


def _tsv_float(x: str) -> str:
    """A score as pandas writes it after the reference's read_csv / to_csv round trip (offtargets.py:540-548): the text
    is parsed to float64 and written with repr(), NaN as NA."""
    return "NA" if x == "NA" else repr(float(x))


def _annotate_rows(rows: List[List[str]], annotations, anncolnames, debug: bool, device=None):
    """annotate_offtargets (offtargets.py:447-483) for the sorted table rows: per file one column, row = the 4th BED column of
    the features overlapping (chrom, position, position + len(spacer)) - `spacer` as the table prints it - or NA.  One device
    table per (file, contig present in the rows); the rows are sorted by (chrom, position), the order the join likes."""
    from .bedannot import BedAnnotation
    names = list(anncolnames) if anncolnames else [f"annotation_{i + 1}" for i in range(len(annotations))]
    chrom = np.array([f[0] for f in rows], dtype=object)
    pos = np.array([int(f[1]) for f in rows], dtype=np.int64)
    stop = pos + np.array([len(f[4]) for f in rows], dtype=np.int64)
    out = []
    for fann in annotations:
        bedann = fann if isinstance(fann, BedAnnotation) else BedAnnotation(fann, 0, debug)
        col = np.full(len(rows), "NA", dtype=object)
        try:
            for c in dict.fromkeys(chrom.tolist()):
                idx = np.flatnonzero(chrom == c)
                col[idx] = bedann.table(c, 0, device).query(pos[idx], stop[idx]).strings()
        finally:
            if bedann is not fann:
                bedann.close()
        out.append(col.tolist())
    return names, out


def offtargets_table(offtargets: List[Offtarget], annotations=None, anncolnames=None, debug: bool = True, device=None) -> str:
    """The text of offtargets_*.tsv: header, rows sorted by (chrom, position) - pandas' two-key sort_values is a stable
    lexsort, ties keep file order -, a trailing newline.  A column without a single number (elevation; cfd for PAMs
    outside SpCas9 / xCas9) comes back from read_csv as all-NaN and is written NA throughout.  `annotations` (paths or opened
    BedAnnotation objects): one more column per file behind `elevation`, named anncolnames[i] or annotation_{i + 1}."""
    rows = sorted(offtargets, key=lambda o: (o.chrom, o.position))
    fields = []
    for o in rows:
        f = o.report_line().split("\t")
        f[9], f[10] = _tsv_float(f[9]), _tsv_float(f[10])
        fields.append(f)
    header = list(OTREPCNAMES)
    if annotations:
        names, cols = _annotate_rows(fields, annotations, anncolnames, debug, device)
        header += names
        if any(ch in x for col in cols for x in set(col) for ch in '"\t\n\r') or any(ch in x for x in names for ch in '"\t\n\r'):
            import io
            import pandas as pd  # a label csv quoting reacts to: written as the reference's to_csv writes it
            df = pd.DataFrame({h: [f[k] for f in fields] for k, h in enumerate(OTREPCNAMES)})
            for nm, col in zip(names, cols):
                df[nm] = col
            buf = io.StringIO()
            df.to_csv(buf, sep="\t", index=False, na_rep="NA")
            return buf.getvalue()
        for f, *labels in zip(fields, *cols):
            f.extend(labels)
    return "\n".join(["\t".join(header)] + ["\t".join(f) for f in fields]) + "\n"


def report_offtargets(crispritz_targets_file, region: Region, pam: PAM, guidelen: int, annotations: List[str], anncolnames: List[str],
                      compute_elevation: bool, right: bool, outdir: str, verbosity: int, debug: bool, device=None) -> List[Offtarget]:
    """offtargets.py:486-558, same arguments (+ `device`: whose context holds the annotation tables; default: the process default).  CFD for SpCas9 / xCas9 PAMs in one device batch; `annotations` (BED paths, or
    bedannot.BedAnnotation objects a caller opened once) add their columns to the table by the device join.  Elevation is
    outside the path and refused, not skipped."""
    if compute_elevation and guidelen + len(pam) == 23 and not right:
        from .crisprhawk_error import CrisprHawkElevationScoreError
        exception_handler(CrisprHawkElevationScoreError, "Elevation is not part of the GPU scoring path", os.EX_DATAERR, debug)
    offtargets = _read_offtargets(crispritz_targets_file, pam, right, debug)
    if pam.cas_system in (SPCAS9, XCAS9):
        offtargets = _compute_cfd_score(offtargets, verbosity, debug)
    print_verbosity("Writing off-targets report", verbosity, VERBOSITYLVL[1])
    if outdir:
        fname = os.path.join(outdir, f"offtargets_{region.contig}_{region.start + PADDING}_{region.stop - PADDING}.tsv")
        text = offtargets_table(offtargets, annotations, anncolnames, debug, device)
        try:
            with open(fname, "w") as f:
                f.write(text)
        except OSError as e:
            exception_handler(CrisprHawkOffTargetsError, f"Failed writing off-targets report for region {region}", os.EX_IOERR, debug, e)
    return offtargets


def _calculate_offtargets_map(offtargets: List[Offtarget], guides: List[Guide]) -> Dict[str, List[Offtarget]]:
    otmap: Dict[str, List[Offtarget]] = {g.guide.upper(): [] for g in guides}
    for ot in offtargets:
        otmap[ot.grna_.upper().replace("-", "")].append(ot)
    return otmap


def _calculate_global_cfd(offtargets: List[Offtarget]) -> float:
    cfds = [0 if ot.cfd == "NA" else float(ot.cfd) for ot in offtargets]
    return 100 / (100 + sum(cfds))


def annotate_guides_offtargets(offtargets: List[Offtarget], guides: List[Guide], verbosity: int) -> List[Guide]:
    otmap = _calculate_offtargets_map(offtargets, guides)
    for guide in guides:
        guide.offtargets = len(otmap[guide.guide.upper()])
        guide.cfd = _calculate_global_cfd(otmap[guide.guide.upper()])
    return guides


def _genome_index(crispritz_index, guidelen: int, pamlen: int, max_bulge: int = 0) -> GenomeIndex:
    """What stands where the reference passes a CRISPRitz index directory: a GenomeIndex (built with max_bulge >= the DNA bulges
    asked for), a {contig: sequence} dict or a FASTA path."""
    if isinstance(crispritz_index, GenomeIndex):
        return crispritz_index
    if isinstance(crispritz_index, (str, os.PathLike)):
        from .genome import read_fasta
        crispritz_index = read_fasta(str(crispritz_index))
    return GenomeIndex(crispritz_index, guidelen, pamlen, max_bulge=max_bulge)


def offtargets_by_spacer(offtargets: List[Offtarget], spacers) -> Dict[str, tuple]:
    """{SPACER: (number of rows, global CFD as the report prints it)} - what annotate_guides_offtargets leaves on every
    guide with that spacer (offtargets.py:597-627; Guide.cfd stores str(round(100 / (100 + sum), 4)), guide.py:723-744)."""
    from .utils import round_score
    rows: Dict[str, List[Offtarget]] = {sp.upper(): [] for sp in spacers}
    for ot in offtargets:
        rows[ot.grna_.upper().replace("-", "")].append(ot)
    return {sp: (len(r), str(round_score(_calculate_global_cfd(r)))) for sp, r in rows.items()}


def specificity_by_spacer(spacers, pam: PAM, crispritz_index, mm: int, guidelen: int, right: bool, debug: bool, bdna: int = 0,
                          brna: int = 0) -> Dict[str, tuple]:
    """{SPACER: (count, global CFD text)} - offtargets_by_spacer's result without the per-site route: one
    GenomeIndex.summary over the unique spacers, with the sites of DNA / RNA bulges of up to `bdna` / `brna` bases (0..2) when
    asked for.  `count` is the guide's rows at 0..mm mismatches, the on-target site and the bulged rows included (the
    reference's len(rows)); the global CFD is 100 / (100 + sum of the rows' CFD rounded to 4 decimals), the sum kept as an
    integer number of 1e-4 units on the device.  An index made here is built with max_bulge = bdna; bulge sizes outside 0..2
    are a CrisprHawkOffTargetsError, as on the table route.  PAMs outside SpCas9 / xCas9 get no CFD
    ("1.0", what the table route's NA -> 0 gives).  The CFD tables are scoring.set_cfd_tables'; a hit with a non-ACGT base
    under a lookup raises CrisprHawkCfdScoreError as compute_cfd_batch does."""
    from .crisprhawk_error import CrisprHawkCfdScoreError
    from .utils import round_score
    uniq = sorted({sp.upper() for sp in spacers})
    if not uniq:
        return {}
    tables = None
    if pam.cas_system in (SPCAS9, XCAS9):
        from .scoring import _tables
        tables = _tables(debug)
    if bdna < 0 or brna < 0 or bdna > 2 or brna > 2:
        exception_handler(CrisprHawkOffTargetsError, f"DNA / RNA bulges of 0..2 bases are enumerated (got {bdna} / {brna})", os.EX_DATAERR, debug)
    try:
        res = _genome_index(crispritz_index, guidelen, len(pam), bdna).summary(uniq, pam, right, mm, cfd_tables=tables, bdna=bdna, brna=brna)
    except ValueError as e:
        exception_handler(CrisprHawkOffTargetsError, f"Off-targets search failed: {e}", os.EX_DATAERR, debug, e)
    if res["n_unscorable"] > 0:
        exception_handler(CrisprHawkCfdScoreError, "CFDon score calculation failed", os.EX_DATAERR, debug)
    counts = res["hist"].sum(axis=1, dtype=np.int64)
    if "bulge_hist" in res:
        counts = counts + res["bulge_hist"].sum(axis=(1, 2), dtype=np.int64)
    counts = counts.tolist()
    sums = res["cfd_e4"].tolist() if res["cfd_e4"] is not None else [0] * len(uniq)
    return {sp: (int(c), str(round_score(100 / (100 + e4 / 1e4)))) for sp, c, e4 in zip(uniq, counts, sums)}


def _annotation_columns_device(annotations, anncolnames, chrom_names, chrom_of_row, pos, stop, debug: bool, device=None):
    """annotate_offtargets (offtargets.py:447-483) for rows sorted by (chrom, position), as columns: per file one Ragged, row =
    the labels of the features overlapping (chrom, position, stop) or NA.  The rows of a contig are consecutive, so a file's
    column is its per-contig query results back to back.  (names, columns)."""
    from .bedannot import BedAnnotation
    from .reports import Ragged
    names = list(anncolnames) if anncolnames else [f"annotation_{i + 1}" for i in range(len(annotations))]
    n = len(pos)
    cuts = np.flatnonzero(np.diff(chrom_of_row)) + 1 if n else np.zeros(0, np.int64)
    lo = np.concatenate([[0], cuts]).astype(np.int64) if n else np.zeros(0, np.int64)
    hi = np.concatenate([cuts, [n]]).astype(np.int64) if n else np.zeros(0, np.int64)
    out = []
    for fann in annotations:
        bedann = fann if isinstance(fann, BedAnnotation) else BedAnnotation(fann, 0, debug)
        blobs, offs, base = [], [np.zeros(1, np.uint64)], 0
        try:
            for a, b in zip(lo.tolist(), hi.tolist()):
                col = bedann.table(chrom_names[int(chrom_of_row[a])], 0, device).query(pos[a:b], stop[a:b])
                nb = int(col.off[-1])
                blobs.append(np.asarray(col.blob[:nb]))
                offs.append(col.off[1:] + np.uint64(base))
                base += nb
        finally:
            if bedann is not fann:
                bedann.close()
        out.append(Ragged(np.concatenate(blobs) if blobs else np.zeros(0, np.uint8), np.concatenate(offs)))
    return names, out


def _estimate_device(uniq, pam: PAM, genome: GenomeIndex, region, mm: int, bdna: int, brna: int, right: bool, outdir: str, debug: bool,
                     annotations, anncolnames, device, variants: bool = False):
    """estimate_offtargets_spacers on arrays: the hits stay columns from the scan to the file.  Returns None when a label or a
    column name would need csv quoting (the caller takes the `objects` engine, which writes through pandas)."""
    from .bedannot import plain_labels
    from .crisprhawk_error import CrisprHawkCfdScoreError
    from .reports import write_report_tsv
    from .utils import round_score
    if bdna < 0 or brna < 0 or bdna > 2 or brna > 2:
        exception_handler(CrisprHawkOffTargetsError, f"DNA / RNA bulges of 0..2 bases are enumerated (got {bdna} / {brna})", os.EX_DATAERR, debug)
    tables = None
    if pam.cas_system in (SPCAS9, XCAS9):
        from .scoring import _tables
        tables = _tables(debug)
    try:
        arr = genome.offtarget_arrays(uniq, pam, right, mm, bdna, brna, **({"variants": True} if variants else {}))
    except ValueError as e:
        exception_handler(CrisprHawkOffTargetsError, f"Off-targets search failed: {e}", os.EX_DATAERR, debug, e)
    n = len(arr["guide"])
    rc, roff, _nblob, _noff, names = genome.row_table()
    # the table's order: (chrom as a string, position), ties in the order of the hits (pandas' stable two-key sort)
    srank = np.empty(len(names), dtype=np.int64)
    srank[np.array(sorted(range(len(names)), key=lambda i: names[i]), dtype=np.int64)] = np.arange(len(names))
    chrom = rc[arr["row"]]
    pos = (roff[arr["row"]] + arr["q"].astype(np.uint64)).astype(np.int64)
    order = np.lexsort((pos, srank[chrom]))
    text, cfd_rows, n_uns = genome.rows_text(arr, uniq, pam, right, order, tables)
    if n_uns > 0:  # before any file is written
        exception_handler(CrisprHawkCfdScoreError, "CFDon score calculation failed", os.EX_DATAERR, debug)
    if outdir:
        cols = {"\t".join(OTREPCNAMES): text}
        if annotations:
            glen = genome.guidelen + len(pam)
            stop = pos + glen + np.where(arr["kind"] == 1, arr["size"], 0).astype(np.int64)  # + len(spacer field): '-' counts
            anames, acols = _annotation_columns_device(annotations, anncolnames, names, chrom[order], pos[order], stop[order], debug, device)
            if any(ch in x for x in anames for ch in '"\t\n\r') or not all(plain_labels(c) for c in acols):
                return None
            cols.update(zip(anames, acols))
        if variants:  # behind any annotation column; built on the host, for the alt rows alone
            from .reports import Ragged
            is_alt = arr["alt"][order] != 0
            sel = order[is_alt]
            ids = genome.variant_ids({k: v[sel] for k, v in arr.items()})
            it = iter(ids)
            cols["origin"] = Ragged.from_strings(["alt" if a else "ref" for a in is_alt.tolist()])
            cols["variant_id"] = Ragged.from_strings([next(it) if a else "NA" for a in is_alt.tolist()])
        fname = os.path.join(outdir, f"offtargets_{region.contig}_{region.start + PADDING}_{region.stop - PADDING}.tsv")
        try:
            if n == 0:
                with open(fname, "w") as f:
                    f.write("\t".join(cols) + "\n")
            else:
                write_report_tsv(fname, cols, np.arange(n, dtype=np.uint64))
        except (OSError, RuntimeError) as e:
            exception_handler(CrisprHawkOffTargetsError, f"Failed writing off-targets report for region {region}", os.EX_IOERR, debug, e)
    # per guide: rows, and the CFD sum accumulated one row after the other in the order of the hits - Python's sum over the
    # guide's Offtarget list, which numpy's pairwise sum does not reproduce in the last digit (cumsum is sequential)
    cfd_hit = np.empty(n, dtype=np.int64)
    cfd_hit[order] = cfd_rows
    val = np.where(cfd_hit < 0, 0, cfd_hit) / 1e4
    counts = np.bincount(arr["guide"], minlength=len(uniq))
    by_guide = np.argsort(arr["guide"], kind="stable")
    ends = np.cumsum(counts)
    res = {}
    for gi, sp in enumerate(uniq):
        a, b = int(ends[gi] - counts[gi]), int(ends[gi])
        tot = float(np.cumsum(val[by_guide[a:b]])[-1]) if b > a else 0
        res[sp] = (int(counts[gi]), str(round_score(100 / (100 + tot))))
    return res


def estimate_offtargets_spacers(spacers, pam: PAM, crispritz_index, region, mm: int, bdna: int, brna: int, guidelen: int, right: bool,
                                outdir: str, verbosity: int, debug: bool, annotations=None, anncolnames=None, device=None,
                                engine: str = "device", variants: bool = False) -> Dict[str, tuple]:
    """estimate_offtargets for the columnar report (pipeline.search_files): the same stage - unique spacers -> device scan
    -> CFD -> offtargets_*.tsv -> per-spacer aggregates - without Guide objects.
    `engine`: "device" keeps the hits as columns from the scan to the file - GenomeIndex.offtarget_arrays, the rows' text and
    CFD written by hawk_offtarget_text, the file by hawk_host_tsv_write, the aggregates from arrays; "objects" is the route
    over one Offtarget per site (search -> report_offtargets -> offtargets_by_spacer).  Same file, same result; a label or
    column name csv quoting reacts to sends the device engine's call to "objects".
    `variants`: the index (a GenomeIndex with SNVs added: add_variants) is scanned for the sites only an ALT allele makes as well
    (GenomeIndex.variant_arrays: every allele is taken to exist, an upper bound; mismatch-only).  Their rows go through the same
    sort, text, CFD and annotation join - spacer / pam / mm / cfd are those of the RESOLVED window - and the file gains two columns
    behind any annotation column: `origin` (ref / alt) and `variant_id` (contig-pos1-REF/ALT of the ALT bases the row reads,
    comma-joined in ascending position; NA on ref rows).  Counts and global CFD include them.  With bulges, with the `objects`
    engine or on an index without variants it is a ValueError before any device work or file."""
    if engine not in ("device", "objects"):
        raise ValueError(f"engine {engine!r}: 'device' or 'objects'")
    if variants:
        if engine != "device":
            raise ValueError("variants=True needs the 'device' engine: the object route lists the plain scan alone")
        if bdna or brna:
            raise ValueError("variants=True is mismatch-only: bulges over ALT alleles (bdna / brna) are not enumerated")
        if not isinstance(crispritz_index, GenomeIndex) or not (crispritz_index.has_variants or crispritz_index.ds is None):
            raise ValueError("variants=True needs a GenomeIndex with variants added (GenomeIndex(variants=...) / add_variants)")
    uniq = sorted({sp.upper() for sp in spacers})
    if engine == "device" and uniq:
        crispritz_index = _genome_index(crispritz_index, guidelen, len(pam), bdna)
        res = _estimate_device(uniq, pam, crispritz_index, region, mm, bdna, brna, right, outdir, debug, annotations or [], anncolnames or [], device,
                               **({"variants": True} if variants else {}))
        if res is not None:
            return res
        if variants:
            raise ValueError("variants=True: an annotation label or column name needs csv quoting, which only the 'objects' engine writes")
    lines = search(_genome_index(crispritz_index, guidelen, len(pam), bdna), uniq, pam, right, mm, verbosity, debug, bdna, brna) if uniq else []
    ots = report_offtargets(lines, region, pam, guidelen, annotations or [], anncolnames or [], False, right, outdir, verbosity, debug, device)
    return offtargets_by_spacer(ots, uniq)


def estimate_offtargets(guides: List[Guide], pam: PAM, crispritz_index, region: Region, crispritz_config, mm: int, bdna: int, brna: int,
                        annotations: List[str], anncolnames: List[str], guidelen: int, compute_elevation: bool, right: bool,
                        threads: int, outdir: str, verbosity: int, debug: bool) -> List[Guide]:
    """offtargets.py:630-722 with the reference's seventeen arguments in the reference's order.  `crispritz_index` is the
    genome (see _genome_index); `crispritz_config` (the conda environment of the external tool) and `threads` have no
    meaning on the device path and are ignored."""
    guides_seqs = sorted(_filter_guides(guides))
    print_verbosity("Estimating off-targets for found guides", verbosity, VERBOSITYLVL[3])
    genome = _genome_index(crispritz_index, guidelen, len(pam), bdna)
    lines = search(genome, guides_seqs, pam, right, mm, verbosity, debug, bdna, brna)
    offtargets = report_offtargets(lines, region, pam, guidelen, annotations, anncolnames, compute_elevation, right, outdir, verbosity, debug)
    return annotate_guides_offtargets(offtargets, guides, verbosity)
