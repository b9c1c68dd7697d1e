"""Haplotype reconstruction from in-memory variant records (what `reconstruct_haplotypes` does between reading the VCF
and handing haplotypes to the search, reference haplotypes.py:106-368 phased, 370-712 unphased).

Only the public behaviour is the reference's: which haplotypes exist for a region, their cased sequences, labels,
position maps and (unphased) per-position allele tables.  The construction is organised around one idea instead of the
reference's chain of helpers: every haplotype is "a region string + one list of variant records applied by
`Haplotype.add_variants_*`"; what differs between the modes is only how records are dealt to carriers (`_deal`) and
which stretch of the region a haplotype covers (`_Stretch`).  Identical cased sequences are then merged (`_merge_equal`,
collapse_haplotypes in the reference, 274-294).

`haplotypes_table` (818-859) writes the haplotypes of a region as a TSV; the strings of a device-built expansion plan come
from the plan as text (hawk_xplan_text), a batch of whole rows at a time.
"""
import os
import random
import string
from typing import Callable, Dict, Iterable, List, Optional, Sequence as Seq, Tuple

from .coordinate import Coordinate
from .haplotype import Haplotype
from .region import Region
from .sequence import Sequence
from .variant import VTYPES, VariantRecord

INDEL_WINDOW = 100  # bases kept either side of an unphased indel (haplotypes.py:465-484)


class _Stretch:
    """The part of a region a haplotype is built over: its bases and its coordinates."""

    __slots__ = ("bases", "coords")

    def __init__(self, bases: str, coords: Coordinate):
        self.bases, self.coords = bases, coords

    @classmethod
    def whole(cls, region: Region) -> "_Stretch":
        return cls(region.sequence.sequence, region.coordinates)

    @classmethod
    def around(cls, region: Region, record: VariantRecord) -> Tuple["_Stretch", int, int]:
        """The region cut to INDEL_WINDOW bases either side of `record` (clamped to the region)."""
        grow = len(record.alt[0]) - len(record.ref) if record.alt else 0
        lo = max(region.start, record.position - INDEL_WINDOW)
        hi = min(region.stop, record.position - grow + INDEL_WINDOW)
        a = lo - region.start
        return cls(region.sequence.sequence[a:hi - region.start + 1], Coordinate(region.contig, lo, hi, 0)), lo, hi

    def fresh(self, phased: bool, copy: int, debug: bool) -> Haplotype:
        return Haplotype(Sequence(self.bases, debug), self.coords, phased, copy, debug)


def _split_alleles(records: Iterable[VariantRecord]) -> List[VariantRecord]:
    out: List[VariantRecord] = []
    for r in records:
        out.extend(r.split())
    return out


def _deal(records: Seq[VariantRecord], carriers: Seq[str], copies: Tuple[int, ...]) -> Dict[str, Tuple[List[VariantRecord], ...]]:
    """Records dealt to their carriers, per chromosome copy in `copies`, in record order; carriers without any record
    are dropped, carriers not listed are ignored.  (A record here is biallelic: `samples[0]` holds its carrier sets.)"""
    hands = {name: tuple([] for _ in copies) for name in carriers}
    for rec in records:
        sets = rec.samples[0]
        for slot, c in enumerate(copies):
            for name in sets[c]:
                hand = hands.get(name)
                if hand is not None:
                    hand[slot].append(rec)
    return {name: hand for name, hand in hands.items() if any(hand)}


def _merge_equal(haps: Seq[Haplotype], debug: bool) -> List[Haplotype]:
    """One haplotype per distinct cased sequence (first-seen order).  The merged haplotype takes the first member's
    coordinates, phase, position map, allele frequencies and allele table; labels are unions - sorted here, where the
    reference joins Python sets in hash order; an all-upper-case sequence is REF whatever its members were called."""
    order: List[str] = []
    members: Dict[str, List[Haplotype]] = {}
    for h in haps:
        key = h.sequence.sequence
        if key not in members:
            members[key] = []
            order.append(key)
        members[key].append(h)
    merged = []
    for key in order:
        group = members[key]
        head = group[0]
        m = Haplotype(Sequence(key, debug, allow_lower_case=True), head.coordinates, head.phased, 0, debug)
        is_ref = key.isupper()
        m.samples = "REF" if is_ref else ",".join(sorted({g.samples for g in group}))
        m.variants = "NA" if is_ref else ",".join(sorted({g.variants for g in group}))
        m.set_afs(head.afs)
        m.set_posmap(head.segments)
        m.set_variant_alleles(head.variant_alleles)
        merged.append(m)
    return merged


def collapse_haplotypes(haplotypes: List[Haplotype], debug: bool) -> List[Haplotype]:
    return _merge_equal(haplotypes, debug)


def initialize_haplotypes(regions, debug: bool) -> Dict[Region, List[Haplotype]]:
    """The REF haplotype of every region (haplotypes.py:106-129)."""
    return {r: [_Stretch.whole(r).fresh(False, 0, debug)] for r in regions}


# ---------------------------------------------------------------------------------------------- phased
def add_variants_phased(haplotypes: List[Haplotype], region: Region, samples: List[str], variants: List[VariantRecord], phased: bool,
                        debug: bool) -> List[Haplotype]:
    """Two chromosome copies per carrier sample (one when both come out identical, labelled 1|1), appended to
    `haplotypes`, then merged by sequence (haplotypes.py:297-368, 714-745; the VCF object replaced by its sample list)."""
    stretch = _Stretch.whole(region)
    for sample, (first, second) in _deal(_split_alleles(variants), samples, (0, 1)).items():
        pair = []
        for copy, records in ((0, first), (1, second)):
            h = stretch.fresh(phased, copy, debug)
            h.add_variants_phased(records, sample)
            pair.append(h)
        if pair[0].sequence.sequence == pair[1].sequence.sequence:
            pair[0].homozygous_samples()
            pair.pop()
        haplotypes += pair
    return _merge_equal(haplotypes, debug)


# ---------------------------------------------------------------------------------------------- unphased
def _unphased_set(stretch: _Stretch, hands: Dict[str, Tuple[List[VariantRecord], ...]], phased: bool, debug: bool) -> List[Haplotype]:
    """One IUPAC-encoded haplotype per carrier (all of its records at once: the reference's combination generator
    keys by variant id and therefore yields exactly this one combination, haplotypes.py:384-405), merged by sequence."""
    built = []
    for sample, (records,) in hands.items():
        h = stretch.fresh(phased, 0, debug)
        h.add_variants_unphased(records, sample)
        built.append(h)
    return _merge_equal(built, debug)


def add_variants_unphased(haplotypes: List[Haplotype], region: Region, samples: List[str], variants: List[VariantRecord],
                          phased: bool, debug: bool) -> List[Haplotype]:
    """Unphased VCFs (haplotypes.py:370-712): SNVs become IUPAC letters on one whole-region haplotype per carrier
    (carriers read from the first genotype slot); every indel inside the region gets its own set of short haplotypes
    - the region cut to 100 nt around it - built for the indel's carriers from the indel and the SNVs inside that
    window, and labelled with the carriers only."""
    alleles = _split_alleles(variants)
    snvs = [v for v in alleles if v.vtype[0] == VTYPES[0]]
    if snvs:
        haplotypes.extend(_unphased_set(_Stretch.whole(region), _deal(snvs, samples, (0,)), phased, debug))
    haplotypes.extend(unphased_indel_windows(region, [v for v in alleles if v.vtype[0] != VTYPES[0]], snvs, phased, debug))
    return haplotypes


def indel_in_region(region: Region, indel: VariantRecord) -> bool:
    c = region.coordinates
    return c.startp <= indel.position < c.stopp


def unphased_indel_windows(region: Region, indels: Seq[VariantRecord], snvs: Seq[VariantRecord], phased: bool, debug: bool) -> List[Haplotype]:
    """The short haplotypes of add_variants_unphased: per indel allele inside the region (in the order given) the region cut to
    100 nt around it, built for the indel's carriers from the indel and those of `snvs` (biallelic SNV records, in file order)
    that lie inside the window.  SNVs outside every window change nothing: the device builder of the whole-region rows
    (workload.expand_unphased_from_vcf) hands over the ones inside alone."""
    haplotypes: List[Haplotype] = []
    for indel in indels:
        if not indel_in_region(region, indel):
            continue
        carriers = set(indel.samples[0][0]) if len(indel.samples) else set()
        if not carriers:
            continue
        stretch, lo, hi = _Stretch.around(region, indel)
        nearby = [indel] + [s for s in snvs if lo <= s.position <= hi]
        # the reference walks the carrier set in hash order; sorted here so that runs are reproducible
        for h in _unphased_set(stretch, _deal(nearby, sorted(carriers), (0,)), phased, debug):
            if h.samples != "REF":
                kept = set(h.samples.split(",")) & carriers if h.samples else set()
                if kept:
                    h.samples = ",".join(sorted(kept))
            haplotypes.append(h)
    return haplotypes


def generate_haplotype_ids(haplotypes: Dict[Region, List[Haplotype]]) -> Dict[Region, List[Haplotype]]:
    """`hap_` + 8 random alphanumerics, unique within a region (haplotypes.py:807-814; unseeded in the reference too)."""
    alphabet = string.ascii_letters + string.digits
    for haps in haplotypes.values():
        seen: Dict[str, None] = {}
        while len(seen) < len(haps):
            seen.setdefault("hap_" + "".join(random.choices(alphabet, k=8)))
        for h, hid in zip(haps, seen):
            h.id = hid
    return haplotypes


# ---------------------------------------------------------------------------------------------- haplotypes table
HAPTABCNAMES = ["id", "haplotype", "variants", "samples"]  # the reference's column names
TEXT_BATCH_BYTES = 256 << 20  # text fetched from a plan per call, unless HAWK_HAPTEXT_BATCH_BYTES or the caller says otherwise


def haplotypes_table_filename(contig: str, start: int, stop: int) -> str:
    """haplotypes.py:839-841; start / stop are the padded region's coordinates"""
    return f"haplotypes_table_{contig}_{start}_{stop}.tsv"


def text_batch_bytes(batch_bytes: Optional[int] = None) -> int:
    """the byte budget of one text batch: the argument, else HAWK_HAPTEXT_BATCH_BYTES (read per call), else 256 MiB"""
    if batch_bytes is not None:
        return int(batch_bytes)
    return int(os.environ.get("HAWK_HAPTEXT_BATCH_BYTES", TEXT_BATCH_BYTES))


def text_batches(lengths: Seq[int], budget: int) -> List[Tuple[int, int]]:
    """Rows of the given lengths, in order, cut into batches [a, b) of whole rows whose bytes stay within `budget`; a row that
    alone exceeds the budget is a batch of its own, so every batch holds at least one row."""
    out: List[Tuple[int, int]] = []
    a, used = 0, 0
    for i, n in enumerate(lengths):
        n = int(n)
        if i > a and used + n > budget:
            out.append((a, i))
            a, used = i, 0
        used += n
    if len(lengths) > a:
        out.append((a, len(lengths)))
    return out


def _label_bytes(x) -> bytes:
    return x if isinstance(x, (bytes, bytearray)) else str(x).encode("ascii")


def write_haplotypes_table(path: str, ids: Seq, variants: Seq, samples: Seq, chunks: Iterable) -> str:
    """The table itself: the header, then `id haplotype variants samples` per row.  `chunks` yields (buffer, offsets) for
    consecutive runs of rows - row j of a chunk is buffer[offsets[j]:offsets[j + 1]], any bytes-like buffer (the page-locked
    array of ExpansionPlan.text, or an encoded string) - and its bytes go to the file as they are: no str per haplotype."""
    k = 0
    with open(path, "wb") as f:
        f.write(("\t".join(HAPTABCNAMES) + "\n").encode("ascii"))
        for buf, off in chunks:
            mv = memoryview(buf)
            for j in range(len(off) - 1):
                f.write(_label_bytes(ids[k]) + b"\t")
                f.write(mv[int(off[j]):int(off[j + 1])])
                f.write(b"\t" + _label_bytes(variants[k]) + b"\t" + _label_bytes(samples[k]) + b"\n")
                k += 1
    if k != len(ids):
        raise ValueError(f"haplotypes table: {k} sequences for {len(ids)} rows")
    return path


def haplotypes_table(contig: str, start: int, stop: int, outdir: str, ids: Seq, variants: Seq, samples: Seq, plan=None,
                     rows: Optional[Seq[int]] = None, sequences: Optional[Seq] = None, batch_bytes: Optional[int] = None) -> str:
    """haplotypes_table (haplotypes.py:818-859) for one region: haplotypes_table_{contig}_{start}_{stop}.tsv in `outdir`, one
    line per haplotype in the order given (REF first), labels as given - `ids` are what the guide report's haplotype_id
    column holds, so the two files join (the reference draws random ids, generate_haplotype_ids).  The sequences come either
    from an expansion plan (`plan` = hapset.ExpansionPlan, `rows` = the plan's kept rows the labels belong to: their text is
    fetched with hawk_xplan_text in batches of whole rows under text_batch_bytes(batch_bytes), so neither the device nor the
    host ever holds more than a batch - or one row, if that is longer) or from the host (`sequences`: str / bytes per row).
    Returns the path."""
    path = os.path.join(outdir, haplotypes_table_filename(contig, start, stop))
    if (plan is None) == (sequences is None):
        raise ValueError("haplotypes_table takes the rows of a plan or host sequences")
    if plan is not None:
        import numpy as np
        rows = np.arange(plan.n_hap, dtype=np.uint32) if rows is None else np.asarray(rows, dtype=np.uint32)
        budget = text_batch_bytes(batch_bytes)
        chunks = (plan.text(rows[a:b]) for a, b in text_batches(plan.hap_len[rows].tolist(), budget))
    else:
        chunks = ((_label_bytes(s), (0, len(s))) for s in sequences)
    return write_haplotypes_table(path, ids, variants, samples, chunks)
