"""Genome index for the off-target scan (K7): contigs cut into equal plane rows in HBM.

The reference hands CRISPRitz a pre-built genome index directory (offtargets.py:264-268); here
the "index" is the genome itself as one-hot bit-planes.  Contigs are split into pieces of
``piece`` bases, each extended by ``overlap`` bases of its successor so every window is seen
whole by exactly one piece (the piece that owns its start)."""
import ctypes as C
from dataclasses import dataclass
from math import comb
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .hapset import DeviceHapSet, HostHaplotype, PosSegments, _p

_CODE2BASE = np.frombuffer(b"ACGT", dtype=np.uint8)


def read_fasta(path: str) -> Dict[str, str]:
    """Minimal multi-FASTA reader (plain text).  The reference reads FASTA through pysam
    (sequence.py:183-360), which is out of scope; this is only a convenience feeder."""
    out, name, buf = {}, None, []
    with open(path) as f:
        for line in f:
            if line.startswith(">"):
                if name is not None:
                    out[name] = "".join(buf)
                name, buf = line[1:].split()[0], []
            else:
                buf.append(line.strip())
    if name is not None:
        out[name] = "".join(buf)
    return out


def encode_guides(guides: Sequence[str]) -> np.ndarray:
    """Spacers (5'->3', ACGT only) -> one uint64 each, base i at bits 2i,2i+1 (A0 C1 G2 T3)."""
    n = len(guides)
    out = np.zeros(n, dtype=np.uint64)
    if n == 0:
        return out
    lens = {len(g) for g in guides}
    if len(lens) != 1 or not 0 < next(iter(lens)) <= 32:
        raise ValueError("guides must share one length of 1..32 bases")
    L = next(iter(lens))
    m = np.frombuffer("".join(guides).upper().encode("ascii"), dtype=np.uint8).reshape(n, L)
    lut = np.full(256, 255, dtype=np.uint8)
    lut[[65, 67, 71, 84]] = (0, 1, 2, 3)
    codes = lut[m]
    bad = np.flatnonzero((codes == 255).any(axis=1))
    if len(bad):
        raise ValueError(f"guide {guides[int(bad[0])]!r} holds a non-ACGT base")
    return (codes.astype(np.uint64) << (2 * np.arange(L, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)


def _no_timing() -> dict:
    """The timing block (hawk_ot_timing) of a call that had nothing to run."""
    return dict(scan_ms=0.0, sites_ms=0.0, match_ms=0.0, total_ms=0.0, n_sites=0, scanned_positions=0)


def decode_window(code: int, nmask: int, length: int) -> str:
    return "".join("N" if (nmask >> i) & 1 else "ACGT"[(code >> (2 * i)) & 3] for i in range(length))


@dataclass
class OffTargetHit:
    guide: int      # index into the guide list
    contig: str
    position: int   # 0-based start of the window on the + strand
    strand: str     # "+" / "-"
    mm: int
    window: str     # guidelen+pamlen bases in guide orientation (5'->3'), N for ambiguous bases


@dataclass
class BulgeHit:
    guide: int        # index into the guide list
    contig: str
    position: int     # 0-based start of the window (site spacer + PAM) on the + strand
    strand: str
    mm: int           # mismatches among the paired bases
    bulge_type: str   # "DNA" / "RNA"
    bulge_size: int
    crrna: str        # the guide spacer, '-' where the DNA has a base without partner
    dna: str          # the site spacer, mismatches lower-case, '-' where the guide has a base without partner
    pam: str          # the site's own PAM
    gaps: int         # bit i: position i (of the site spacer for DNA bulges, of the guide for RNA bulges) is bulged out


def _derived_guides(guides: Sequence[str], G: int, b: int, dna: bool):
    """The mismatch-only guides a bulge of b bases turns every guide into - RNA: b interior bases deleted; DNA: b bases (each of
    A, C, G, T) inserted between two bases - with the guide each came from and its bulge positions as a bitmask (of the guide
    for RNA, of the derived guide = the site spacer for DNA).  RNA: identical derived guides of one guide are kept once, under
    their lexicographically smallest positions (the paired bases are the same string either way).  DNA: every (placement,
    inserted bases) is its own derived guide - two placements may spell the same string and still pair the site's bases with
    different guide bases, so the host must see each."""
    from itertools import combinations, combinations_with_replacement, product
    derived, owner, gaps = [], [], []
    for gi, g in enumerate(guides):
        seen = {}
        if dna:
            for slots in combinations_with_replacement(range(1, G), b):          # insert before guide base s, ascending
                pos = tuple(s + k for k, s in enumerate(slots))                    # positions of the inserted bases in the derived guide
                for bases in product("ACGT", repeat=b):
                    chars, ins = list(g), 0
                    for s, x in zip(slots, bases):
                        chars.insert(s + ins, x)
                        ins += 1
                    derived.append("".join(chars))
                    owner.append(gi)
                    gaps.append(sum(1 << q for q in pos))
        else:
            for dele in combinations(range(1, G - 1), b):
                d = "".join(c for i, c in enumerate(g) if i not in dele)
                if d not in seen or dele < seen[d]:
                    seen[d] = dele
        for d, pos in seen.items():
            derived.append(d)
            owner.append(gi)
            gaps.append(sum(1 << p for p in pos))
    return derived, owner, gaps


def derived_per_guide(G: int, b: int, dna: bool) -> int:
    """How many derived guides _derived_guides makes of one guide of G bases at most (exactly, for DNA bulges)."""
    return comb(G - 2 + b, b) * 4 ** b if dna else comb(G - 2, b)


def min_spacer(guidelen: int) -> int:
    """The shortest spacer an index of `guidelen` is asked about: the site of an RNA bulge of 2 (scan_bulges)."""
    return max(1, guidelen - 2)


def row_geometry(lengths: Dict[str, int], guidelen: int, pamlen: int, piece: int, max_bulge: int, spacer: int) -> List[Tuple[str, int, int, int]]:
    """The rows of a genome index and the window starts each owns, without a device: (contig, offset, end, own) per row, in
    contig order.  A row holds contig bases [offset, end): `piece` bases plus an overlap of the longest window (guidelen +
    max_bulge + pamlen) less one, clipped to the contig.  Rows exist wherever the SHORTEST window (min_spacer + pamlen) fits,
    so a tail too short for the full window still has a row for the windows of RNA-bulged sites.  For windows of `spacer` +
    pamlen bases the row owns starts [offset, offset + own): those of its piece whose window lies inside the row.  Every
    start s with s + window <= contig length is then owned by exactly one row, for every spacer of min_spacer ..
    guidelen + max_bulge (tests/test_host_logic.py sweeps the edges)."""
    Lmin = min_spacer(guidelen) + pamlen
    overlap = guidelen + pamlen + max_bulge - 1
    Lw = spacer + pamlen
    out = []
    for name, n in lengths.items():
        for off in range(0, max(n, 1), piece):
            end = min(n, off + piece + overlap)
            if end - off < Lmin:
                continue
            out.append((name, off, end, max(0, min(piece, end - off - Lw + 1))))
    return out


# ---- SNVs added to an index (hawk_genome_variants): the off-target scan over a variant-enriched genome ---------------------------
_BASE_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
# why a record is dropped (counted in variant_stats, never raised): not a single-base substitution; its contig is not in the
# index; its position is outside the contig; the index holds N or another non-ACGT base there; its REF base is not the index's;
# its ALT is its REF; no row of the index holds the position (a contig shorter than the shortest window)
VARIANT_DROPS = ("not_snv", "unknown_contig", "out_of_contig", "ref_n", "ref_mismatch", "alt_is_ref", "no_row")
_STATUS_DROP = {1: "ref_n", 2: "ref_mismatch", 3: "alt_is_ref"}  # include/hawk.h: HAWK_OV_*


def variant_records(src) -> List[Tuple[str, int, str, str]]:
    """`src` - (contig, pos0, ref, alt) tuples, a readers.VCF, a VCF path, or a list mixing them - as a list of (contig, 0-based
    position, REF, ALT), multi-allelic records split per ALT."""
    from .readers import VCF
    if src is None:
        return []
    if isinstance(src, (str, VCF)) or hasattr(src, "__fspath__"):
        src = [src]
    out = []
    for item in src:
        if isinstance(item, VCF):
            recs = item.sites()
        elif isinstance(item, str) or hasattr(item, "__fspath__"):
            recs = VCF(str(item)).sites()
        else:
            recs = [(str(item[0]), int(item[1]), str(item[2]), str(item[3]))]
        for contig, pos, ref, alt in recs:
            for a in alt.split(","):
                out.append((contig, pos, ref.upper(), a.upper()))
    return out


def variant_entries(lengths: Dict[str, int], geo, records, row_lo: int = 0, row_hi: Optional[int] = None):
    """The (row, q, ref, alt) entries hawk_genome_variants takes, from records and the rows of row_geometry (`geo`): a variant
    in the overlap of two rows is entered in both; rows outside [row_lo, row_hi) (another rank's shard) are left out and the
    rows are numbered from row_lo.  Returns (row uint32[], q uint32[], ref uint8[], alt uint8[], var int64[] = the record each
    entry came from, dropped = {reason: count} of the records no entry was made for, kept = [(contig, pos0, ref, alt)] of the
    records with an entry, in `var` numbering)."""
    row_hi = len(geo) if row_hi is None else row_hi
    by_contig: Dict[str, list] = {}
    for k, (name, off, end, _own) in enumerate(geo):
        by_contig.setdefault(name, []).append((off, end, k))
    starts = {name: [r[0] for r in rows] for name, rows in by_contig.items()}
    dropped = {k: 0 for k in VARIANT_DROPS}
    dropped["other_shard"] = 0
    row, q, rb, ab, var, kept = [], [], [], [], [], []
    from bisect import bisect_right
    for contig, pos, ref, alt in records:
        if len(ref) != 1 or len(alt) != 1 or ref not in _BASE_CODE or alt not in _BASE_CODE:
            dropped["not_snv"] += 1
            continue
        name = contig if contig in lengths else (contig[3:] if contig.startswith("chr") and contig[3:] in lengths else
                                                 "chr" + contig if "chr" + contig in lengths else None)
        if name is None:
            dropped["unknown_contig"] += 1
            continue
        if not 0 <= pos < lengths[name]:
            dropped["out_of_contig"] += 1
            continue
        if alt == ref:
            dropped["alt_is_ref"] += 1
            continue
        rows = by_contig.get(name, [])
        k = bisect_right(starts.get(name, []), pos) - 1  # the last row that starts at or before pos; earlier ones may still reach it
        hit, mine = 0, 0
        while k >= 0 and rows[k][1] > pos:
            hit += 1
            if row_lo <= rows[k][2] < row_hi:
                if not mine:
                    kept.append((name, pos, ref, alt))
                mine += 1
                row.append(rows[k][2] - row_lo); q.append(pos - rows[k][0]); rb.append(_BASE_CODE[ref]); ab.append(_BASE_CODE[alt])
                var.append(len(kept) - 1)
            k -= 1
        if not hit:
            dropped["no_row"] += 1
        elif not mine:
            dropped["other_shard"] += 1
    return (np.array(row, np.uint32), np.array(q, np.uint32), np.array(rb, np.uint8), np.array(ab, np.uint8), np.array(var, np.int64),
            dropped, kept)


def variant_outcome(status: np.ndarray, var: np.ndarray, dropped: Dict[str, int], kept) -> Tuple[dict, list]:
    """variant_stats from the entries' statuses (every entry of a variant gets the same one: the rows that share a position
    hold the same base): (dict(applied=..., dropped={reason: count}), the applied (contig, pos0, ref, alt))."""
    first = np.unique(var, return_index=True)[1] if len(var) else np.zeros(0, np.int64)
    st = status[first]
    dropped = dict(dropped)
    for code, reason in _STATUS_DROP.items():
        dropped[reason] += int((st == code).sum())
    applied = [kept[i] for i in np.flatnonzero(st == 0).tolist()]
    return dict(applied=len(applied), dropped=dropped), applied


def _host_rows(contigs: Dict[str, str], geo):
    """(text, seq_off uint64[rows + 1], scan_start int32[rows], scan_stop int32[rows]) of the rows of row_geometry"""
    parts = [contigs[name][off:end] for name, off, end, _own in geo]
    seq_off = np.zeros(len(geo) + 1, np.uint64)
    np.cumsum([len(p) for p in parts], out=seq_off[1:])
    return ("".join(parts).encode("ascii"), seq_off, np.zeros(len(geo), np.int32), np.array([own for *_x, own in geo], np.int32))


OTV_COLUMNS = (("guide", np.uint32), ("row", np.uint32), ("q", np.uint32), ("strand", np.uint8), ("mm", np.uint8), ("code", np.uint64),
               ("nmask", np.uint32), ("alt", np.uint32))


def host_variant_scan(contigs: Dict[str, str], guidelen: int, pamlen: int, piece: int, records, guides: Sequence[str], pam, right: bool,
                      max_mm: int, cap: int = 1 << 16):
    """The variant rows of GenomeIndex(contigs, guidelen, pamlen, piece, variants=records).variant_arrays(guides, pam, right,
    max_mm) made on the host, no device (hawk_host_offtarget_variant_scan: the resolver the kernel runs, in plain loops):
    ({guide, row, q, strand, mm, code, nmask, alt} arrays in (row, q, strand, guide) order, variant_stats).  For tests and for
    machines without a GPU; the product scans on the device."""
    lens = {name: len(seq) for name, seq in contigs.items()}
    geo = row_geometry(lens, guidelen, pamlen, piece, 0, guidelen)
    row, q, rb, ab, var, dropped, kept = variant_entries(lens, geo, variant_records(records))
    text, seq_off, ss, se = _host_rows(contigs, geo)
    status = np.zeros(len(row), np.uint8)
    g2 = encode_guides([g.upper() for g in guides])
    par = _lib.OtParams(pam.bits, pam.bitsrc, len(pam), guidelen, int(bool(right)), max_mm)
    while True:
        o = {k: np.empty(cap, t) for k, t in OTV_COLUMNS}
        n = C.c_uint64(0)
        rc = _lib.lib().hawk_host_offtarget_variant_scan(text, _p(seq_off), C.c_uint32(len(geo)), _p(ss), _p(se), _p(row), _p(q), _p(rb), _p(ab),
                                                          C.c_uint64(len(row)), _p(status), C.byref(par), _p(g2), C.c_uint32(len(g2)),
                                                          *[_p(o[k]) for k, _t in OTV_COLUMNS], C.c_uint64(cap), C.byref(n))
        if rc != _lib.HAWK_E_CAPACITY:
            break
        cap = int(n.value)
    _lib.check(rc, "hawk_host_offtarget_variant_scan")
    stats, _applied = variant_outcome(status, var, dropped, kept)
    return {k: o[k][:int(n.value)].copy() for k, _t in OTV_COLUMNS}, stats


class GenomeIndex:
    """`shard = (rank, world)`: the genome's rows (pieces) are block-partitioned over the ranks of a multi-GPU job
    ("shard the genome by contig/offset across ranks, guides replicated, rows gathered"); every rank keeps the
    descriptors of ALL rows, so a hit's global row index names its contig and offset anywhere."""

    def __init__(self, contigs: Dict[str, object], guidelen: int, pamlen: int, piece: int = 1 << 22, device: Optional[int] = None,
                 shard: Optional[Tuple[int, int]] = None, max_bulge: int = 0, variants=None):
        """`max_bulge`: the largest DNA bulge the index will be asked about - neighbouring rows then overlap by that many bases
        more, so that the longer windows of bulged sites (guidelen + bulge + pamlen) still lie inside one row.  Rows and the
        window starts they own: row_geometry.  `variants`: SNVs to add to the index (add_variants)."""
        self.L = guidelen + pamlen
        self.guidelen, self.pamlen, self.max_bulge = guidelen, pamlen, int(max_bulge)
        if self.max_bulge < 0 or self.L + self.max_bulge > 32:
            raise ValueError(f"windows of {guidelen} + {self.max_bulge} (DNA bulge) + {pamlen} bases: the device encodes windows of up to 32 bases")
        self._lens = {name: len(seq) for name, seq in contigs.items()}
        geo = row_geometry(self._lens, guidelen, pamlen, piece, self.max_bulge, guidelen)
        self.rows: List[Tuple[str, int, int]] = [(name, off, own) for name, off, _end, own in geo]  # (contig, offset, owned window starts), all ranks' rows
        spans = [(name, off, end) for name, off, end, _own in geo]
        self.total = sum(self._lens.values())
        if not self.rows:
            raise ValueError(f"genome shorter than the shortest window the index is asked about ({min_spacer(guidelen)} + {pamlen} bases)")
        self.n_rows_total = len(self.rows)
        self.row_lo, self.row_hi = 0, self.n_rows_total
        if shard is not None and shard[1] > 1:
            from .parallel import shard_range
            self.row_lo, self.row_hi = shard_range(self.n_rows_total, shard[0], shard[1])
        haps: List[HostHaplotype] = []
        for (name, off, end), (_n, _o, own) in zip(spans[self.row_lo:self.row_hi], self.rows[self.row_lo:self.row_hi]):
            seq = contigs[name]
            arr = np.frombuffer(seq.encode("ascii"), dtype=np.uint8) if isinstance(seq, str) else np.frombuffer(seq, dtype=np.uint8)
            haps.append(HostHaplotype(arr[off:end], PosSegments.identity(off, end - off), True, (0, own)))
        self.ds = None
        self._piece = piece
        self._meta_guidelen = guidelen
        if haps:  # a rank may own no row of a tiny genome
            self.ds = DeviceHapSet(haps, device)
            _lib.check(self.ds._L.hawk_genome_finalize(self.ds._h), "hawk_genome_finalize")
        self.last_timing = None
        self._geo = geo
        self.variant_stats = dict(applied=0, dropped={k: 0 for k in VARIANT_DROPS + ("other_shard",)})
        self._var_applied: Dict[Tuple[str, int], str] = {}  # (contig, pos0) -> REF base of the positions that hold an ALT allele
        self.has_variants = False
        if variants is not None:
            self.add_variants(variants)

    # ---- the variant-enriched genome (hawk_genome_variants / hawk_offtarget_variant_scan) ------------------------------------
    def add_variants(self, records) -> dict:
        """Adds SNVs to the index: `records` = (contig, pos0, ref, alt) tuples, a readers.VCF or a VCF path (only the first five
        columns are read: sites, no genotypes), or a list of them; multi-allelic records are split per ALT.  Every allele at a
        position is taken to exist in somebody and every combination of alleles inside a window on one chromosome - genotypes and
        phasing are not consulted (the enriched-genome semantics of CRISPRitz add-variants): what variant_arrays lists is an
        UPPER BOUND on the sites a population carries.  A record that is no single-base substitution, names an unknown contig or
        a position outside it, meets N (or another non-ACGT base) in the index, states a REF base that is not the index's, or an
        ALT equal to its REF is dropped and counted in variant_stats = dict(applied, dropped={reason: count}) - never raised.
        A sharded index adds the variants of its own rows (the others count as dropped['other_shard']).  Calling it again adds to
        the set.  The plain scans (scan_arrays, bulge_arrays, summary) do not see the variants.  Returns this call's stats."""
        recs = variant_records(records)
        row, q, rb, ab, var, dropped, kept = variant_entries(self._lens, self._geo, recs, self.row_lo, self.row_hi)
        status = np.zeros(len(row), np.uint8)
        if self.ds is not None:
            na, nd = C.c_uint64(0), C.c_uint64(0)
            _lib.check(self.ds._L.hawk_genome_variants(self.ds._h, _p(row), _p(q), _p(rb), _p(ab), C.c_uint64(len(row)), _p(status),
                                                       C.byref(na), C.byref(nd)), "hawk_genome_variants")
            self.has_variants = True
        stats, applied = variant_outcome(status, var, dropped, kept)
        for name, pos, ref, _alt in applied:
            self._var_applied[(name, pos)] = ref
        self.variant_stats["applied"] += stats["applied"]
        for k, v in stats["dropped"].items():
            self.variant_stats["dropped"][k] += v
        return stats

    def variant_arrays(self, guides: Sequence[str], pam, right: bool, max_mm: int, cap: int = 1 << 20):
        """One hawk_offtarget_variant_scan over this rank's rows - the sites only an ALT allele makes: ({guide, row (global), q,
        strand, mm, code, nmask, alt} arrays in no particular order, timing).  A window (either strand, guide orientation) is
        resolved against a guide position by position: a PAM position is satisfied iff its allele set ({REF} + its ALTs) meets the
        PAM's IUPAC set and reads REF's base if that is in the set, else the lowest allele that is; a spacer position reads the
        guide's base if the allele set holds it, else REF's (a mismatch; N is a mismatch).  A row is listed when every PAM position
        is satisfied, mm <= max_mm and alt - bit i: window position i reads an ALT base - is not 0; rows with alt == 0 are
        scan_arrays' and are not listed again, so a window may have a REF row there and an ALT row here for one guide: two alleles
        of one locus.  code / nmask are the RESOLVED window.  Mismatch-only."""
        self._set_window(self.guidelen)
        g2 = encode_guides([g.upper() for g in guides])
        if len(g2) and len(guides[0]) != self.guidelen:
            raise ValueError(f"guides of {len(guides[0])} bases on an index built for {self.guidelen}")
        if self.ds is None:
            return {k: np.zeros(0, t) for k, t in OTV_COLUMNS}, _no_timing()
        par = _lib.OtParams(pam.bits, pam.bitsrc, len(pam), self.guidelen, int(bool(right)), max_mm)
        return self._collect("hawk_offtarget_variant_scan", (self.ds._h, C.byref(par), _p(g2), len(g2)), 8, cap, OTV_COLUMNS)

    def variant_ids(self, h) -> List[str]:
        """Per row of variant_arrays' columns the variants its window reads, as the guide report spells them - contig-pos1-REF/ALT,
        joined by commas in ascending position."""
        out = []
        comp = (3, 2, 1, 0)
        for i in range(len(h["guide"])):
            name, off, _ = self.rows[int(h["row"][i])]
            q, minus, code, alt = off + int(h["q"][i]), bool(h["strand"][i]), int(h["code"][i]), int(h["alt"][i])
            ids = []
            for k in range(self.L):
                if (alt >> k) & 1:
                    pos = q + (self.L - 1 - k if minus else k)
                    b = (code >> (2 * k)) & 3
                    ids.append((pos, f"{name}-{pos + 1}-{self._var_applied[(name, pos)]}/{'ACGT'[comp[b] if minus else b]}"))
            out.append(",".join(s for _pos, s in sorted(ids)))
        return out

    def _set_window(self, guidelen: int) -> None:
        """Which window starts every row owns depends on the window length (a window must fit its row): scans with another
        spacer length - the sites of bulged alignments - get their own scan ranges (hawk_hapset_set_meta; planes untouched)."""
        if guidelen == self._meta_guidelen or self.ds is None:
            return
        if not (min_spacer(self.guidelen) <= guidelen <= self.guidelen + self.max_bulge):
            raise ValueError(f"window of {guidelen} + {self.pamlen} bases: the index was built for spacers of "
                             f"{min_spacer(self.guidelen)} to {self.guidelen + self.max_bulge}")
        geo = row_geometry(self._lens, self.guidelen, self.pamlen, self._piece, self.max_bulge, guidelen)[self.row_lo:self.row_hi]
        self.ds.set_meta([HostHaplotype(b"", PosSegments.identity(off, end - off), True, (0, own)) for _name, off, end, own in geo])
        self._meta_guidelen = guidelen

    def scan_arrays(self, guides: Sequence[str], pam, right: bool, max_mm: int, cap: int = 1 << 20, guidelen: Optional[int] = None):
        """One hawk_offtarget_scan over this rank's rows: ({guide, row (global), q, strand, mm, code, nmask} arrays, timing).
        `guidelen` (default: the index's): the spacer length of this scan's guides - bulged alignments are searched as
        mismatch-only scans of derived guides that are shorter or longer than the guides themselves (scan_bulges)."""
        guidelen = self.guidelen if guidelen is None else int(guidelen)
        self._set_window(guidelen)
        if self.ds is None:
            return {k: np.zeros(0, t) for k, t in self.OT_COLUMNS[:7]}, _no_timing()
        g2 = encode_guides(guides)
        par = _lib.OtParams(pam.bits, pam.bitsrc, len(pam), guidelen, int(bool(right)), max_mm)
        return self._collect("hawk_offtarget_scan", (self.ds._h, C.byref(par), _p(g2), len(g2)), 7, cap)

    OT_COLUMNS = (("guide", np.uint32), ("row", np.uint32), ("q", np.uint32), ("strand", np.uint8), ("mm", np.uint8), ("code", np.uint64),
                  ("nmask", np.uint32), ("gaps", np.uint64), ("kind", np.uint8), ("size", np.uint8))

    def _collect(self, fn: str, head: tuple, n_cols: int, cap: int, columns=None):
        """One listing call `fn`(*head, the first n_cols OT_COLUMNS as outputs of `cap` rows, cap, &n, &timing), again with room for
        n + 1024 rows for as long as it answers HAWK_E_CAPACITY: (the columns trimmed to the n rows, row made global; timing)."""
        cols = (columns or self.OT_COLUMNS)[:n_cols]
        while True:
            o = {k: np.empty(cap, t) for k, t in cols}
            n, tm = C.c_uint64(0), _lib.OtTiming()
            rc = getattr(self.ds._L, fn)(*head, *[_p(o[k]) for k, _t in cols], C.c_uint64(cap), C.byref(n), C.byref(tm))
            if rc != _lib.HAWK_E_CAPACITY:
                break
            cap = int(n.value) + 1024
        _lib.check(rc, fn)
        self.last_timing = {k: getattr(tm, k) for k, _ in tm._fields_}
        hits = {k: o[k][:int(n.value)].copy() for k, _t in cols}
        hits["row"] = hits["row"] + np.uint32(self.row_lo)
        return hits, self.last_timing

    def _check_bulges(self, bdna: int, brna: int) -> None:
        if not (0 <= bdna <= 2 and 0 <= brna <= 2):
            raise ValueError("bulges of 0..2 bases are enumerated")
        if bdna > self.max_bulge:
            raise ValueError(f"the index was built for DNA bulges of up to {self.max_bulge} bases (GenomeIndex(max_bulge=...))")

    BULGE_KINDS = ((True, 1), (True, 2), (False, 1), (False, 2))  # the order of `bulge_hist`: DNA 1, DNA 2, RNA 1, RNA 2

    def _each_bulge(self, bdna: int, brna: int, run) -> list:
        """`run(b, dna)` -> (result, timing) for every (type, size) asked for, in BULGE_KINDS order: [(slot in BULGE_KINDS, dna, b,
        result)], the timing blocks in last_bulge_timing.  The index's own window is put back, also when a call raises."""
        self.last_bulge_timing, out = [], []
        try:
            for k, (dna, b) in enumerate(self.BULGE_KINDS):
                if b <= (bdna if dna else brna):
                    res, tm = run(b, dna)
                    self.last_bulge_timing.append(dict(tm, bulge_type="DNA" if dna else "RNA", bulge_size=b))
                    out.append((k, dna, b, res))
        finally:
            self._set_window(self.guidelen)
        return out

    # ---- bulged sites (the -bDNA / -bRNA arguments of the reference's CRISPRitz call, offtargets.py:264-268) -------------
    def scan_bulges(self, guides: Sequence[str], pam, right: bool, max_mm: int, bdna: int, brna: int, cap: int = 1 << 20,
                    max_derived: int = 1 << 20, engine: str = "derived") -> List["BulgeHit"]:
        """Sites that pair with a guide once `b` bases are bulged out - of the DNA (the site's spacer is b bases longer, b <= bdna)
        or of the RNA (b bases shorter, b <= brna) - with at most `max_mm` mismatches among the paired bases.  A bulged alignment
        is a mismatch-only alignment of a DERIVED guide: the guide with b interior bases deleted (RNA bulge), or with b bases
        inserted between its bases, every base tried (DNA bulge); each family of derived guides goes through hawk_offtarget_scan
        with its own spacer length, and the host keeps, per (guide, site, type, size), the placement with the fewest mismatches
        (ties: the lexicographically smallest bulge positions) - the definitions of oracle/hawk_oracle.c: ora_offtargets_bulges.
        Bulges of up to 2 bases are enumerated (CRISPRitz's own limit).  A family is derived and scanned for consecutive slices
        of the guides, at most `max_derived` derived guides per scan (a DNA bulge of 2 turns a 20-mer into 3040 of them); rows
        never depend on other guides, so the slicing does not change them.
        `engine`: "derived" is the route above; "device" selects the placement where the site is (hawk_offtarget_bulges, k_ot_bulge:
        one call per (type, size) over the guides as they are - no derived guides, no duplicates, no host selection) and returns
        the same rows in the same order."""
        if engine not in ("derived", "device"):
            raise ValueError(f"engine {engine!r}: 'derived' or 'device'")
        self._check_bulges(bdna, brna)
        G = self.guidelen
        guides = [g.upper() for g in guides]
        order = lambda r: (r.guide, r.bulge_type, r.bulge_size, self._contig_rank(r.contig), r.position, r.strand == "-")
        if engine == "device":  # last_bulge_timing: the timing block of every (type, size) call
            parts = self._each_bulge(bdna, brna, lambda b, dna: self.bulge_arrays(guides, pam, right, max_mm, b, dna, cap))
            return sorted((r for _k, dna, b, h in parts for r in self._bulge_rows_device(h, guides, right, b, dna)), key=order)
        out: List[BulgeHit] = []
        self.last_bulge_timing = []
        for dna, bmax in ((True, bdna), (False, brna)):
            for b in range(1, bmax + 1):
                step = max(1, int(max_derived) // max(1, derived_per_guide(G, b, dna)))
                Gs = G + b if dna else G - b
                for g0 in range(0, len(guides), step):
                    derived, owner, gaps = _derived_guides(guides[g0:g0 + step], G, b, dna)
                    if not derived:
                        continue
                    h, _tm = self.scan_arrays(derived, pam, right, max_mm, cap, guidelen=Gs)
                    out += self._bulge_rows(h, guides, np.asarray(owner) + g0, np.asarray(gaps, dtype=np.uint64), Gs, b, dna, right, max_mm)
        self._set_window(self.guidelen)
        out.sort(key=order)
        return out

    def _contig_rank(self, name: str) -> int:
        m = getattr(self, "_crank", None)
        if m is None:
            m = self._crank = {n: i for i, n in enumerate(dict.fromkeys(r[0] for r in self.rows))}
        return m[name]

    def _bulge_rows(self, h, guides, owner, gaps, Gs: int, b: int, dna: bool, right: bool, max_mm: int) -> List["BulgeHit"]:
        n = len(h["guide"])
        if n == 0:
            return []
        G, P = self.guidelen, self.pamlen
        L = Gs + P
        # the windows as bytes [n, L] (guide orientation, N for ambiguous bases) and their spacers
        win = self._windows(h, L)
        site = win[:, P:] if right else win[:, :Gs]
        g_of = owner[h["guide"]]
        gp = gaps[h["guide"]]
        gmat = np.frombuffer("".join(guides).encode("ascii"), dtype=np.uint8).reshape(len(guides), G)[g_of]  # [n, G]
        # paired positions: site position i <-> guide position j, skipping the bulged ones
        span = Gs if dna else G
        gapbits = ((gp[:, None] >> np.arange(span, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)   # [n, span]
        keep = ~gapbits
        idx = np.argsort(~keep, axis=1, kind="stable")[:, : span - b]  # the span - b unbulged positions, ascending
        if dna:
            s_al, g_al = np.take_along_axis(site, idx, axis=1), gmat
        else:
            s_al, g_al = site, np.take_along_axis(gmat, idx, axis=1)
        mism = (s_al != g_al) | (s_al == ord("N"))
        mm = mism.sum(axis=1)
        ok = mm <= max_mm
        if dna:  # a bulged base is a definite base
            ok &= ~((site == ord("N")) & gapbits).any(axis=1)
        # placement order: the tuple of bulge positions, ascending
        pos_sorted = np.sort(np.where(gapbits, np.arange(span)[None, :], 1 << 20), axis=1)[:, :b]
        rank = np.zeros(n, dtype=np.int64)
        for k in range(b):
            rank = rank * 64 + pos_sorted[:, k]
        sel = np.flatnonzero(ok)
        if len(sel) == 0:
            return []
        order = sel[np.lexsort((rank[sel], mm[sel], h["strand"][sel], h["q"][sel], h["row"][sel], g_of[sel]))]
        key = np.stack([g_of[order].astype(np.int64), h["row"][order].astype(np.int64), h["q"][order].astype(np.int64), h["strand"][order].astype(np.int64)], axis=1)
        first = np.ones(len(order), dtype=bool)
        first[1:] = (key[1:] != key[:-1]).any(axis=1)
        return [self._bulge_hit(h, i, win, guides, int(g_of[i]), int(mm[i]), int(gp[i]), Gs, b, dna, right) for i in order[first].tolist()]

    def _bulge_hit(self, h, i: int, win, guides, g: int, mm: int, gbits: int, Gs: int, b: int, dna: bool, right: bool) -> "BulgeHit":
        """Row i of the scan columns `h` (win[i]: its window's bytes in guide orientation, N for ambiguous bases) as the BulgeHit
        of guide g with the bulges at `gbits`: the crRNA / DNA strings with '-' where the other has no partner, mismatches of the
        DNA in lower case, the site's own PAM."""
        G, P = self.guidelen, self.pamlen
        name, off, _ = self.rows[int(h["row"][i])]
        sp_site = (win[i, P:] if right else win[i, :Gs]).tobytes().decode("ascii")
        pam_site = (win[i, :P] if right else win[i, Gs:]).tobytes().decode("ascii")
        cr, dn = [], []
        si = gi = 0
        while si < Gs or gi < G:
            if dna and si < Gs and (gbits >> si) & 1:
                cr.append("-"); dn.append(sp_site[si]); si += 1
            elif (not dna) and gi < G and (gbits >> gi) & 1:
                cr.append(guides[g][gi]); dn.append("-"); gi += 1
            else:
                t, q = sp_site[si], guides[g][gi]
                cr.append(q); dn.append(t if t == q else t.lower())
                si += 1; gi += 1
        return BulgeHit(g, name, off + int(h["q"][i]), "-" if h["strand"][i] else "+", mm, "DNA" if dna else "RNA", b,
                        "".join(cr), "".join(dn), pam_site, gbits)

    def _windows(self, h, L: int):
        """the windows of scan columns as bytes [n, L]: guide orientation, N for ambiguous bases"""
        sh = (2 * np.arange(L, dtype=np.uint64))[None, :]
        codes = ((h["code"][:, None] >> sh) & np.uint64(3)).astype(np.uint8)
        amb = ((h["nmask"][:, None].astype(np.uint64) >> np.arange(L, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
        win = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
        win[amb] = ord("N")
        return win

    def bulge_arrays(self, guides: Sequence[str], pam, right: bool, max_mm: int, b: int, dna: bool, cap: int = 1 << 20):
        """One hawk_offtarget_bulges over this rank's rows - the bulged sites of one (type, size), the placement chosen on the
        device: ({guide, row (global), q, strand, mm, code, nmask, gaps} arrays in no particular order, timing).  The windows
        (code / nmask) have guidelen + b (DNA bulge) or guidelen - b (RNA bulge) + pamlen bases; the scan ranges are left set
        for them (scan_bulges puts the index's own back)."""
        G = self.guidelen
        if not 1 <= b <= 2:
            raise ValueError("bulges of 1..2 bases are enumerated")
        if G - b < 3:
            raise ValueError(f"guides of {G} bases leave no interior base to pair beside a bulge of {b}")
        if dna and b > self.max_bulge:
            raise ValueError(f"the index was built for DNA bulges of up to {self.max_bulge} bases (GenomeIndex(max_bulge=...))")
        Gs = G + b if dna else G - b
        self._set_window(Gs)
        g2 = encode_guides(guides)
        if len(g2) and len(guides[0]) != G:
            raise ValueError(f"guides of {len(guides[0])} bases on an index built for {G}")
        if self.ds is None or len(g2) == 0:
            return {k: np.zeros(0, t) for k, t in self.OT_COLUMNS[:8]}, _no_timing()
        par = _lib.OtParams(pam.bits, pam.bitsrc, len(pam), G, int(bool(right)), max_mm)
        return self._collect("hawk_offtarget_bulges", (self.ds._h, C.byref(par), _p(g2), len(g2), 1 if dna else 2, int(b)), 8, cap)

    def _bulge_rows_device(self, h, guides, right: bool, b: int, dna: bool) -> List["BulgeHit"]:
        """The columns of one bulge_arrays as BulgeHits, in their order."""
        if len(h["guide"]) == 0:
            return []
        Gs = self.guidelen + b if dna else self.guidelen - b
        win = self._windows(h, Gs + self.pamlen)
        return [self._bulge_hit(h, i, win, guides, int(h["guide"][i]), int(h["mm"][i]), int(h["gaps"][i]), Gs, b, dna, right)
                for i in range(len(h["guide"]))]

    # ---- the off-targets table without an object per site (hawk_offtarget_text) ------------------------------------------
    def _check_variants(self, bdna: int = 0, brna: int = 0) -> None:
        if bdna or brna:
            raise ValueError("the variant pass is mismatch-only: bulges over ALT alleles are not enumerated (bdna = brna = 0 with variants)")
        if not self.has_variants and self.ds is not None:
            raise ValueError("no variants were added to the index (GenomeIndex(variants=...) / add_variants)")

    def offtarget_arrays(self, guides: Sequence[str], pam, right: bool, max_mm: int, bdna: int = 0, brna: int = 0, cap: int = 1 << 20,
                         variants: bool = False):
        """Every hit of `guides` as columns - one scan_arrays, one bulge_arrays per (type, size), concatenated with `kind`
        (0 = X, 1 = DNA, 2 = RNA) and `size` columns (gaps = 0 for un-bulged hits) - in the order the product's file has: the
        un-bulged hits in scan()'s order, then the bulged ones in scan_bulges()' order (guide, type, size, contig, position,
        strand), by one lexsort of integer keys.  No OffTargetHit / BulgeHit is built.  The index's own window is put back.
        `variants`: the rows of variant_arrays are appended as un-bulged hits (kind = size = gaps = 0) and the columns gain `alt`
        (uint32, 0 on every other row); a window's ALT row sorts behind its REF row.  Bulges with variants are a ValueError."""
        self._check_bulges(bdna, brna)
        if variants:
            self._check_variants(bdna, brna)
        guides = [g.upper() for g in guides]
        h, _tm = self.scan_arrays(guides, pam, right, max_mm, cap)
        n0 = len(h["guide"])
        parts = [dict(h, gaps=np.zeros(n0, np.uint64), kind=np.zeros(n0, np.uint8), size=np.zeros(n0, np.uint8))]
        for _k, dna, b, hb in self._each_bulge(bdna, brna, lambda b, dna: self.bulge_arrays(guides, pam, right, max_mm, b, dna, cap)):
            nb = len(hb["guide"])
            parts.append(dict(hb, kind=np.full(nb, 1 if dna else 2, np.uint8), size=np.full(nb, b, np.uint8)))
        if variants:
            hv, self.last_variant_timing = self.variant_arrays(guides, pam, right, max_mm, cap)
            nv = len(hv["guide"])
            parts[0]["alt"] = np.zeros(n0, np.uint32)
            parts.append(dict(hv, gaps=np.zeros(nv, np.uint64), kind=np.zeros(nv, np.uint8), size=np.zeros(nv, np.uint8)))
        names = self.OT_COLUMNS + ((("alt", np.uint32),) if variants else ())
        cols = {k: np.concatenate([pt[k] for pt in parts]).astype(t, copy=False) for k, t in names}
        # rows of a contig ascend with their offsets and own disjoint starts: (row, q) orders as (contig, position) does
        keys = (cols["strand"], cols["q"], cols["row"], cols["size"], cols["kind"], cols["guide"], cols["kind"] != 0)
        order = np.lexsort(((cols["alt"] != 0,) if variants else ()) + keys)
        return {k: np.ascontiguousarray(v[order]) for k, v in cols.items()}

    def row_table(self):
        """(contig id uint32[rows], offset uint64[rows], names blob uint8[], name offsets uint64[contigs + 1], names) of ALL rows"""
        t = getattr(self, "_row_table", None)
        if t is None:
            names = list(dict.fromkeys(r[0] for r in self.rows))
            cid = {n: i for i, n in enumerate(names)}
            enc = [n.encode("ascii") for n in names]
            noff = np.zeros(len(enc) + 1, dtype=np.uint64)
            np.cumsum([len(b) for b in enc], out=noff[1:])
            blob = np.frombuffer(b"".join(enc), dtype=np.uint8) if noff[-1] else np.zeros(1, np.uint8)
            t = self._row_table = (np.array([cid[r[0]] for r in self.rows], dtype=np.uint32), np.array([r[1] for r in self.rows], dtype=np.uint64),
                                   blob, noff, names)
        return t

    def rows_text(self, arrays, guides: Sequence[str], pam, right: bool, order=None, cfd_tables=None):
        """The hits of offtarget_arrays as rows of offtargets_*.tsv, written on the device (hawk_offtarget_text: k_ot_text_len,
        the 64-bit scan, k_ot_text_fill): (reports.Ragged - row i = the eleven tab-joined fields of hit order[i], or of hit i -,
        cfd_e4 int64[n] = the rows' CFD in units of 1e-4 or -1, n_unscorable).  `cfd_tables` = (mm[20,4,4], pam[16]) or None
        (the cfd column is NA).  The rows come down into page-locked blocks (_lib.pinned_empty)."""
        from .reports import Ragged
        n = len(arrays["guide"])
        cols = [np.ascontiguousarray(arrays[k], dtype=t) for k, t in self.OT_COLUMNS]
        if any(len(c) != n for c in cols):
            raise ValueError("rows_text: the hit columns disagree on their length")
        g2 = encode_guides([g.upper() for g in guides])
        rc, roff, nblob, noff, names = self.row_table()
        od = None if order is None else np.ascontiguousarray(order, dtype=np.uint64)
        if od is not None and len(od) != n:
            raise ValueError("rows_text: `order` must name every row once")
        mm, pt = self._cfd_tables(cfd_tables)
        device = self.ds.device if self.ds is not None else None
        L, ctx = _lib.lib(), _lib.context(device)
        par = _lib.OtParams(0, 0, len(pam), self.guidelen, int(bool(right)), 0)
        nbytes, nuns, tm, dl = C.c_uint64(0), C.c_uint64(0), _lib.OtTextTiming(), C.c_float(0)
        byname = dict(zip((k for k, _t in self.OT_COLUMNS), cols))
        _lib.check(L.hawk_offtarget_text(ctx, C.c_uint64(n), *[_p(byname[k]) for k in ("guide", "row", "q", "strand", "mm", "code", "nmask", "gaps", "kind", "size")],
                                         _p(g2), C.c_uint32(len(g2)), C.byref(par), _p(rc), _p(roff), C.c_uint32(len(rc)), _p(nblob), _p(noff),
                                         C.c_uint32(len(names)), pam.pam.encode("ascii"),
                                         _p(od), _p(mm), _p(pt), C.byref(nbytes), C.byref(nuns), C.byref(tm)), "hawk_offtarget_text")
        off = _lib.pinned_empty(n + 1, np.uint64, device)
        blob = _lib.pinned_empty(int(nbytes.value), np.uint8, device)
        cfd = _lib.pinned_empty(n, np.int64, device)
        _lib.check(L.hawk_offtarget_text_download(ctx, _p(blob), _p(off), _p(cfd), C.byref(dl)), "hawk_offtarget_text_download")
        self.last_text_timing = {k: float(getattr(tm, k)) for k in ("upload_ms", "len_ms", "scan_ms", "fill_ms", "total_ms")}
        self.last_text_timing.update(download_ms=float(dl.value), out_bytes=int(nbytes.value), n_rows=n)
        return Ragged(blob, off), cfd, int(nuns.value)

    def hits_from_arrays(self, h) -> List["OffTargetHit"]:
        """Arrays of scan_arrays (of this rank, or gathered from every rank) -> sorted OffTargetHit list."""
        order = np.lexsort((h["strand"], h["q"], h["row"], h["guide"]))
        out = []
        for i in order:
            name, off, _ = self.rows[int(h["row"][i])]
            out.append(OffTargetHit(int(h["guide"][i]), name, off + int(h["q"][i]), "-" if h["strand"][i] else "+", int(h["mm"][i]),
                                    decode_window(int(h["code"][i]), int(h["nmask"][i]), self.L)))
        return out

    def summary(self, guides: Sequence[str], pam, right: bool, max_mm: int, cfd_tables=None, comm=None, bdna: int = 0, brna: int = 0) -> dict:
        """The scan's per-guide aggregates without its hits (hawk_offtarget_summary, and with `bdna` / `brna` above zero one
        hawk_offtarget_bulge_summary per (type, size)): dict(hist = uint32[n_guides, max_mm + 1] un-bulged hits per guide and
        mismatch count - the on-target site included -, cfd_e4 = int64[n_guides] the sum of round(CFD, 4) over the guide's rows
        in units of 1e-4 (None without `cfd_tables` = (mm[20,4,4], pam[16])), n_hits, n_unscorable = rows with a non-ACGT
        base under a CFD lookup, which count in the histograms and add nothing to cfd_e4).  With bulges the dict also holds
        bulge_hist = uint32[n_guides, 4, max_mm + 1], the bulged rows per guide, (type, size) in the order DNA 1, DNA 2, RNA 1,
        RNA 2 (what was not asked for stays zero) and mismatch count; cfd_e4, n_hits and n_unscorable then cover ALL rows, a
        bulged row's CFD being the one the off-targets table prints for it (rows_text).  `hist` stays the un-bulged histogram;
        with both zero the dict is the mismatch-only one, key for key.  last_bulge_timing: the timing block of every (type,
        size) call, as offtarget_arrays fills it.  Every row is consumed inside the kernel that finds it: no capacity, no
        retry, nothing sized by the rows.  Duplicate guides get equal rows; an index without rows on this rank returns zeros.
        The arrays are integers, so shards add up exactly: with a communicator every rank's arrays are gathered to rank 0,
        which returns their sum (other ranks return their own shard's)."""
        self._check_bulges(bdna, brna)
        bulged = bool(bdna or brna)
        n, stride = len(guides), int(max_mm) + 1
        g2 = encode_guides(guides)
        self._set_window(self.guidelen)
        mm, pt = self._cfd_tables(cfd_tables)
        out, self.last_timing = self._summary_call("hawk_offtarget_summary", g2, pam, right, int(max_mm), mm, pt)
        hist, cfd = out["hist"], out["cfd_e4"]
        if bulged:
            out["bulge_hist"] = np.zeros((n, 4, stride), dtype=np.uint32)
            for k, _dna, _b, part in self._each_bulge(bdna, brna, lambda b, dna: self._bulge_summary(g2, pam, right, int(max_mm), b, dna, mm, pt)):
                out["bulge_hist"][:, k, :] = part["hist"]
                if cfd is not None:
                    out["cfd_e4"] += part["cfd_e4"]
                out["n_hits"] += part["n_hits"]
                out["n_unscorable"] += part["n_unscorable"]
        if comm is not None and comm.world > 1:
            tail = np.array([out["n_hits"], out["n_unscorable"]], dtype=np.int64)
            bh = out["bulge_hist"].reshape(-1).astype(np.int64) if bulged else np.zeros(0, np.int64)
            flat = np.concatenate([hist.reshape(-1).astype(np.int64), cfd if cfd is not None else np.zeros(0, np.int64), bh, tail])
            parts = comm.gatherv_bytes(flat, 0)
            if comm.rank == 0:
                tot = np.sum(np.stack(parts), axis=0, dtype=np.int64)
                o1 = n * stride + (n if cfd is not None else 0)
                out = dict(hist=tot[:n * stride].astype(np.uint32).reshape(n, stride),
                           cfd_e4=tot[n * stride:n * stride + n].copy() if cfd is not None else None,
                           n_hits=int(tot[-2]), n_unscorable=int(tot[-1]))
                if bulged:
                    out["bulge_hist"] = tot[o1:o1 + 4 * n * stride].astype(np.uint32).reshape(n, 4, stride)
        return out

    def _bulge_summary(self, g2, pam, right: bool, max_mm: int, b: int, dna: bool, mm, pt):
        """One hawk_offtarget_bulge_summary over this rank's rows: (dict(hist uint32[n, max_mm + 1], cfd_e4 int64[n] or None,
        n_hits, n_unscorable) of the bulged rows of one (type, size), timing).  The scan ranges are left set for the windows of
        that (type, size), as bulge_arrays leaves them."""
        G, n = self.guidelen, len(g2)
        if G - b < 3:
            raise ValueError(f"guides of {G} bases leave no interior base to pair beside a bulge of {b}")
        self._set_window(G + b if dna else G - b)
        return self._summary_call("hawk_offtarget_bulge_summary", g2, pam, right, max_mm, mm, pt, 1 if dna else 2, int(b), run=n > 0)

    @staticmethod
    def _cfd_tables(cfd_tables):
        """(mm[20,4,4], pam[16]) as the contiguous float64 arrays the library reads, or (None, None)"""
        if cfd_tables is None:
            return None, None
        return (np.ascontiguousarray(cfd_tables[0], dtype=np.float64).reshape(20, 4, 4),
                np.ascontiguousarray(cfd_tables[1], dtype=np.float64).reshape(16))

    def _summary_call(self, fn: str, g2, pam, right: bool, max_mm: int, mm, pt, *kind, run: bool = True):
        """One summary call `fn` over this rank's rows, `kind` = (bulge type, size) for the bulged one: (dict(hist uint32[n,
        max_mm + 1], cfd_e4 int64[n] or None without tables, n_hits, n_unscorable), timing) - zeros without rows or with `run` false."""
        n = len(g2)
        hist = np.zeros((n, max_mm + 1), dtype=np.uint32)
        cfd = np.zeros(n, dtype=np.int64) if mm is not None else None
        nh, nu = C.c_uint64(0), C.c_uint64(0)
        timing = _no_timing()
        if self.ds is not None and run:
            par = _lib.OtParams(pam.bits, pam.bitsrc, len(pam), self.guidelen, int(bool(right)), max_mm)
            tm = _lib.OtTiming()
            rc = getattr(self.ds._L, fn)(self.ds._h, C.byref(par), _p(g2), n, *kind, _p(mm), _p(pt), _p(hist), _p(cfd),
                                         C.byref(nh), C.byref(nu), C.byref(tm))
            _lib.check(rc, fn)
            timing = {k: getattr(tm, k) for k, _ in tm._fields_}
        return dict(hist=hist, cfd_e4=cfd, n_hits=int(nh.value), n_unscorable=int(nu.value)), timing

    def scan(self, guides: Sequence[str], pam, right: bool, max_mm: int, cap: int = 1 << 20, comm=None, variants: bool = False) -> List[OffTargetHit]:
        """All windows within ``max_mm`` mismatches of any guide, both strands, sorted by
        (guide, contig order, position, strand).  With a communicator (parallel.RcclComm / TcpComm) the hits of every
        rank's genome shard are gathered to rank 0, which returns the whole list (other ranks return []).
        `variants`: the sites only an ALT allele of the added SNVs makes (variant_arrays) are listed too, with their resolved
        windows; a window's ALT hit follows its REF hit."""
        hits, _tm = self.scan_arrays(guides, pam, right, max_mm, cap)
        if variants:
            self._check_variants()
            hv, self.last_variant_timing = self.variant_arrays(guides, pam, right, max_mm, cap)
            hits = {k: np.concatenate([v, hv[k]]) for k, v in hits.items()}
        if comm is not None and comm.world > 1:
            parts = {k: comm.gatherv_bytes(v, 0) for k, v in hits.items()}
            if comm.rank != 0:
                return []
            hits = {k: np.concatenate(v) for k, v in parts.items()}
        return self.hits_from_arrays(hits)
