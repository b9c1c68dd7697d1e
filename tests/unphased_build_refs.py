"""Inputs and plain statements for the tests of the unphased row builder (workload.expand_unphased_from_vcf, hawk_ubuild_*,
hawk_host_unphased_rows): the unphased genotype rule in Python, a small case builder that yields the same records as a VcfBlock
(what the device builder reads) and as VariantRecord objects (what haplotypes.add_variants_unphased reads), the seam panel, and
the comparisons against the host-built haplotypes.  No device work here."""
import math

import numpy as np

from crisprhawk_hip import haplotypes as hap_mod, search_guides as sg
from crisprhawk_hip.coordinate import Coordinate
from crisprhawk_hip.haplotype import Haplotype
from crisprhawk_hip.readers import VcfBlock
from crisprhawk_hip.region import Region
from crisprhawk_hip.sequence import Sequence
from crisprhawk_hip.variant import VariantRecord

CONTIG = "chrU"
FLAGGED = ["1", "0/1/1", "0|1", "0/1|2", "", "a/1", "/1"]   # genotypes the rule flags
PLAIN = ["0/0", "0/1", "1/0", "1/1", "./1", "1/.", "./.", "1/2", "0/10", "10/2", "0/1:35", "./.:0", "3/254", "0/255", "0/300:7:x"]


def gt_rule(field: str):
    """(flags, code0, code1) of one sample column under the unphased rule (include/hawk.h, hawk_gt_parse_unphased)"""
    g = field.split(":")[0]
    parts = g.split("/")
    flags = 0 if (len(parts) == 2 and "|" not in g) else 1
    codes = [255, 255]
    for c, p in enumerate(parts[:2]):
        if p == ".":
            continue
        if p != "" and all(ch in "0123456789" for ch in p):
            codes[c] = min(int(p), 254)
        else:
            flags |= 4
    return flags, codes[0], codes[1]


def record_codes(rows, n_samples: int):
    """codes[n_lines][2 * n_samples] and the flag byte per record, by gt_rule"""
    codes = np.full((len(rows), 2 * n_samples), 255, np.uint8)
    flags = np.zeros(len(rows), np.uint8)
    for i, f in enumerate(rows):
        cols = f[9:]
        if len(cols) != n_samples:
            flags[i] |= 2
        for s, g in enumerate(cols[:n_samples]):
            fl, a, b = gt_rule(g)
            flags[i] |= fl
            codes[i, 2 * s], codes[i, 2 * s + 1] = a, b
    return codes, flags


def block_of(rows) -> VcfBlock:
    """tab-split records -> the block readers.VCF.fetch_block would hand out"""
    text, line_off, gt_off = bytearray(), [0], []
    for f in rows:
        fixed = "\t".join(f[:9]).encode()
        gt_off.append(len(text) + len(fixed) + 1)
        text += fixed + b"\t" + "\t".join(f[9:]).encode() + b"\n"
        line_off.append(len(text))
    return VcfBlock(np.frombuffer(bytes(text), np.uint8), np.array(line_off, np.uint64), np.array(gt_off, np.uint64), [f[:9] for f in rows])


class Case:
    """One region and its unphased records.  Offsets are 0-based in the region; genotypes are given per sample index, the rest
    is 0/0."""

    def __init__(self, name: str, length: int, n_samples: int, seed: int = 1, startp: int = 5000):
        rng = np.random.default_rng(seed)
        self.name, self.startp = name, startp
        self.seq = "".join("ACGT"[i] for i in rng.integers(0, 4, length))
        self.samples = [f"S{i:03d}" for i in range(n_samples)]
        self.rows = []
        self.fmt = "GT"
        self._region = None   # a region given from outside (g4_case) instead of the one made of startp and seq

    def _row(self, off: int, ref: str, alts: str, gts, fmt=None):
        cols = ["0/0"] * len(self.samples)
        for s, g in gts.items():
            cols[s] = g
        n_alt = alts.count(",") + 1
        af = ",".join(f"{0.05 + 0.01 * ((off + k) % 40):.4g}" for k in range(n_alt))
        self.rows.append([CONTIG, str(self.startp + off), ".", ref, alts, ".", "PASS", f"AF={af}", fmt or self.fmt] + cols)
        return self

    def other(self, off: int, k: int = 1) -> str:
        """the k-th base after REF's at `off` in ACGT order: an alt that is not the ref"""
        return "ACGT"[("ACGT".index(self.seq[off]) + k) % 4]

    def snv(self, off: int, gts, k: int = 1, fmt=None):
        return self._row(off, self.seq[off], self.other(off, k), gts, fmt)

    def multi(self, off: int, ks, gts):
        return self._row(off, self.seq[off], ",".join(self.other(off, k) for k in ks), gts)

    def raw(self, off: int, ref: str, alts: str, gts, fmt=None):
        return self._row(off, ref, alts, gts, fmt)

    def deletion(self, off: int, n: int, gts):
        return self._row(off, self.seq[off:off + n + 1], self.seq[off], gts)

    def insertion(self, off: int, ins: str, gts):
        return self._row(off, self.seq[off], self.seq[off] + ins, gts)

    def sort(self):
        self.rows.sort(key=lambda f: int(f[1]))   # stable: records at one position keep the order they were given in
        return self

    # ---- what the two builders read
    @property
    def coord(self) -> Coordinate:
        return self._region.coordinates if self._region is not None else Coordinate(CONTIG, self.startp, self.startp + len(self.seq) - 1, 0)

    def region(self) -> Region:
        return self._region if self._region is not None else Region(Sequence(self.seq, True), self.coord)

    def block(self) -> VcfBlock:
        return block_of(self.rows)

    def records(self):
        out = []
        for f in self.rows:
            v = VariantRecord(True)
            v.read_vcf_line(list(f), self.samples, False)
            out.append(v)
        return out

    def host(self):
        """(region, haplotypes) as pipeline._search_host_built builds them, ids included"""
        region = self.region()
        haps = [Haplotype(Sequence(self.seq, True), region.coordinates, False, 0, True)]
        haps = hap_mod.add_variants_unphased(haps, region, self.samples, self.records(), False, True)
        for i, h in enumerate(haps):
            h.id = f"hap_{i:08d}"
        return region, haps


def _random_gts(rng, n_samples: int, p: float):
    return {s: ("0/1", "1/0", "1/1", "./1", "1/.")[int(rng.integers(0, 5))] for s in np.flatnonzero(rng.random(n_samples) < p).tolist()}


def panel():
    """The seam panel: the smallest shapes at which each piece of the builder can go wrong (name -> Case)."""
    cases = {}

    def add(c):
        cases[c.name] = c.sort()
    # word seams of the row fill: offsets 0, 31, 32, 33, L - 1, the last word's first bit; L = 32k - 1, 32k, 32k + 1, and L = 960 =
    # 32 * 30, where the row's 30 words and the two guard words fill the stride of 32 (a thread's last vector holds both)
    for length in (1023, 1024, 1025, 960):
        c = Case(f"seams_L{length}", length, 3, seed=length)
        last_word = 32 * ((length + 31) // 32 - 1)
        for k, off in enumerate(sorted({0, 31, 32, 33, 127, 128, last_word, length - 1})):
            c.snv(off, {0: "0/1", 1: "1/1"} if k % 2 == 0 else {0: "1/0"})
        add(c)
    # several alts at one position: 1/2 of one record; separate records; three alts from a 1/2 and a separate record
    c = Case("multi_alts", 700, 4, seed=11)
    c.multi(150, (1, 2), {0: "1/2", 1: "0/2", 2: "1/0"})
    c.snv(200, {0: "0/1", 3: "1/1"}, k=1).snv(200, {0: "1/1"}, k=2)
    c.multi(300, (1, 2), {1: "1/2", 3: "2/2"}).snv(300, {1: "./1", 2: "0/1"}, k=3)
    add(c)
    # a duplicated record, its copies carried by different samples: equal rows, merged, labels joined
    c = Case("duplicate_record", 600, 3, seed=12)
    c.snv(222, {0: "0/1"}).snv(222, {2: "1/1"}).snv(400, {0: "0/1", 2: "0/1"})
    add(c)
    # genotype forms, allele number 10 (the tenth alt is the SNV; the insertions before it have no carrier) and FORMAT fields
    c = Case("genotype_forms", 600, 8, seed=13)
    c.snv(130, {0: "1/1", 1: "./1", 2: "1/.", 3: "0/0", 4: "./.", 5: "0/1", 6: "1/0"})
    ref = c.seq[260]
    c.raw(260, ref, ",".join([ref + "T" * k for k in range(1, 10)] + [c.other(260)]), {1: "0/10:35", 7: "10/10:9"}, fmt="GT:DP")
    c.snv(401, {4: "0/1:3:x", 0: "./.:0"}, fmt="GT:DP:XX")
    add(c)
    # lane = sample: 1, 63, 64, 65, 129 samples
    for ns in (1, 63, 64, 65, 129):
        c = Case(f"samples_{ns}", 500, ns, seed=100 + ns)
        rng = np.random.default_rng(ns)
        for off in (120, 121, 250, 333, 480):
            gts = _random_gts(rng, ns, 0.35)
            gts[ns - 1] = "0/1"   # the last lane carries
            c.snv(off, gts)
        add(c)
    # ballot chunks: 63, 64, 65, 256, 257 variants; sample 0 carries all of them
    for nv in (63, 64, 65, 256, 257):
        c = Case(f"variants_{nv}", 1300, 3, seed=200 + nv)
        rng = np.random.default_rng(nv)
        for off in range(101, 101 + 4 * nv, 4):
            gts = _random_gts(rng, 3, 0.4)
            gts[0] = "0/1"
            c.snv(off, gts)
        add(c)
    # samples without an SNV between carriers; two and five samples with equal rows, not adjacent
    c = Case("interleaved_and_equal", 800, 12, seed=14)
    c.snv(140, {1: "0/1", 4: "1/1", 6: "0/1", 8: "1/0", 9: "0/1", 11: "1/1"})
    c.snv(300, {1: "0/1", 4: "1/0", 6: "0/1", 8: "1/1", 9: "0/1", 11: "0/1", 2: "0/1"})
    c.snv(500, {2: "1/1", 7: "0/1"}).snv(640, {7: "0/1"})   # rows: {1,4,6,8,9,11}... the five of 1,4,6,8,9 + 11; 2; 7
    c.snv(641, {11: "0/1"})                                  # 11 leaves the group: five equal rows (1,4,6,8,9); 2 and 7 and 11 alone
    c.snv(700, {3: "0/1", 10: "0/1"})                        # two equal rows, not adjacent
    add(c)
    c = Case("all_equal", 500, 6, seed=15)
    c.snv(111, {s: "0/1" for s in range(6)}).snv(345, {s: ("1/1" if s % 2 else "./1") for s in range(6)})
    add(c)
    # a sample that carries only an indel; indels in the region's first and last window with SNVs inside their windows
    c = Case("indels_at_the_ends", 900, 5, seed=16)
    c.deletion(40, 2, {0: "0/1", 3: "0/1"}).snv(20, {0: "0/1", 1: "0/1"}).snv(95, {3: "1/1"}).snv(139, {1: "0/1"})
    c.insertion(860, "GG", {2: "0/1", 4: "1/1"}).snv(800, {2: "0/1"}).snv(890, {4: "0/1", 1: "1/0"})
    c.deletion(450, 1, {3: "0/1"})   # an indel in the middle, carried by a sample that also has SNVs
    add(c)
    c = Case("indel_only_sample", 700, 4, seed=17)
    c.insertion(300, "T", {2: "0/1"}).snv(280, {0: "0/1"}).snv(350, {1: "1/1", 0: "0/1"})
    add(c)
    c = Case("indels_without_snvs", 700, 3, seed=18)
    c.deletion(200, 3, {0: "0/1"}).insertion(480, "ACG", {1: "1/1", 2: "0/1"})
    add(c)
    c = Case("snvs_only", 640, 3, seed=19)
    c.snv(100, {0: "0/1"}).snv(320, {1: "0/1", 0: "1/1"}).snv(539, {2: "1/1"})
    add(c)
    return cases


def declines():
    """name -> (Case, the reason expand_unphased_from_vcf declines with) - one per reason the builder can meet in records"""
    out = {}
    c = Case("haploid_genotype", 500, 3, seed=31).snv(200, {0: "0/1", 1: "1"})
    out[c.name] = (c, 1)
    c = Case("phased_genotype", 500, 3, seed=32).snv(200, {0: "0/1", 1: "0|1"})
    out[c.name] = (c, 1)
    c = Case("malformed_genotype", 500, 3, seed=33).snv(200, {0: "0/1", 1: "a/1"})
    out[c.name] = (c, 1)
    c = Case("missing_column", 500, 3, seed=34).snv(200, {0: "0/1"})
    c.rows[0] = c.rows[0][:-1]
    out[c.name] = (c, 1)
    c = Case("multi_base_substitution", 500, 3, seed=35)
    c.raw(200, c.seq[200:202], c.other(200) + c.seq[201], {0: "0/1"})
    out[c.name] = (c, 2)
    c = Case("alt_outside_acgt", 500, 3, seed=36)
    c.raw(200, c.seq[200], "N", {0: "0/1"})
    out[c.name] = (c, 3)
    c = Case("ref_mismatch", 500, 3, seed=37)
    c.raw(200, c.other(200, 1), c.other(200, 2), {0: "0/1"}).snv(300, {1: "0/1"})
    out[c.name] = (c, 4)
    c = Case("ref_mismatch_in_a_later_member", 500, 3, seed=38)   # sample 1's row equals sample 0's; its record names another ref
    c.snv(200, {0: "0/1"}, k=1).raw(200, c.other(200, 1), c.seq[200], {1: "0/1"})
    out[c.name] = (c, 4)
    c = Case("snv_outside_the_region", 500, 3, seed=39)
    c.raw(500, "A", "C", {0: "0/1"}).snv(100, {1: "0/1"})
    out[c.name] = (c, 5)
    c = Case("alt_carried_twice", 500, 3, seed=40).snv(200, {0: "0/1"}).snv(200, {0: "0/1", 1: "0/1"})
    out[c.name] = (c, 7)
    for c, _ in out.values():
        c.sort()
    return out


def g4_case(fx) -> "Case":
    """a g4_unphased* fixture's region and records (test_host_objects._unphased_inputs), as a Case"""
    from test_host_objects import _unphased_inputs
    reg, region, recs = _unphased_inputs(fx)
    c = Case.__new__(Case)
    c.name, c.startp, c.seq, c.samples, c.fmt = "g4", region.start, reg.sequence, list(reg.samples), "GT"
    c.rows = []
    for v in reg.variants:
        f = reg.vcf_fields(v)
        f[9:] = [g.replace("|", "/") for g in f[9:]]
        c.rows.append(f)
    c._region = region
    return c


# ---- comparisons
def _same_afs(a, b) -> bool:
    return list(a) == list(b) and all((x == y) or (isinstance(x, float) and isinstance(y, float) and math.isnan(x) and math.isnan(y))
                                      for x, y in zip(a.values(), b.values()))


def assert_labels_equal(labels, haps):
    assert len(labels) == len(haps)
    for r, (l, h) in enumerate(zip(labels, haps)):
        assert (l.samples, l.variants, l.id) == (h.samples, h.variants, h.id), r
        assert _same_afs(l.afs, h.afs), r
        assert np.array_equal(l.segments.rel, h.segments.rel) and np.array_equal(l.segments.gen, h.segments.gen) and l.segments.length == h.segments.length, r


def assert_alleles_equal(table, haps):
    key, off, ref = sg.flatten_variant_alleles(haps)
    assert np.array_equal(np.asarray(table[0], np.uint64), key) and np.array_equal(np.asarray(table[1], np.uint32), off)
    assert np.array_equal(np.asarray(table[2], np.uint8), ref)


def whole_region_rows(haps):
    """the SNV rows of a host-built list: everything behind REF that spans the region"""
    return [h for h in haps[1:] if h.coordinates.start == haps[0].coordinates.start and h.coordinates.stop == haps[0].coordinates.stop
            and len(h.sequence) == len(haps[0].sequence)]
