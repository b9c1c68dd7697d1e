"""Deterministic synthetic inputs for the guide-search hot path.

The recipes follow SURVEY.md §8(d) / BASELINE.md §3: iid uniform ACGT contigs, a BED
interval padded by 100 nt on each side, and a phased variant panel (SNV / deletion /
insertion sites with log-uniform allele frequencies, every haplotype column carrying the
alt allele independently).  Everything is driven by ``numpy.random.default_rng(seed)`` so
the golden-fixture generator (tests/golden/make_golden.py, which feeds the *reference*),
the parity tests and bench.py all see the same bytes.

Coordinates follow the reference: a BED line ``chrom start stop`` gives a region whose
string index 0 is the 1-based genomic position ``max(0, start-100)`` and whose sequence is
``contig[startp-1 : stop+100]`` (reference: coordinate.py:21-43, sequence.py:340-343,
region_constructor.py:21).
"""

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

PADDING = 100  # reference: region_constructor.py:21

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_IUPAC_EXTRA = np.frombuffer(b"NRYSWKMBDHV", dtype=np.uint8)


def random_sequence(rng: np.random.Generator, n: int, iupac_frac: float = 0.0) -> str:
    """iid uniform ACGT string; with ``iupac_frac`` > 0 sprinkle N/IUPAC codes."""
    seq = _ACGT[rng.integers(0, 4, size=n)]
    if iupac_frac > 0.0 and n > 0:
        mask = rng.random(n) < iupac_frac
        seq = seq.copy()
        seq[mask] = _IUPAC_EXTRA[rng.integers(0, len(_IUPAC_EXTRA), size=int(mask.sum()))]
    return seq.tobytes().decode("ascii")


@dataclass
class VariantSite:
    """One biallelic VCF row (left-anchored indels, VCF conventions)."""

    pos: int  # 1-based genomic position of the first REF base
    ref: str
    alt: str
    af: float
    gt: np.ndarray  # uint8 [n_samples, 2]; 1 = alt on that chromosome copy

    @property
    def chain(self) -> int:
        return len(self.alt) - len(self.ref)

    @property
    def is_snv(self) -> bool:
        return len(self.ref) == len(self.alt)


@dataclass
class SynthRegion:
    contig: str
    contig_seq: str
    bed_start: int
    bed_stop: int
    samples: List[str] = field(default_factory=list)
    variants: List[VariantSite] = field(default_factory=list)
    gt_matrix: Optional[np.ndarray] = None  # uint8 [len(variants), 2 * n_samples]: the records' genotypes as one matrix

    def variant_columns(self):
        """The records as columns - positions, REF / ALT alleles as one byte blob each with offsets - next to the genotype
        matrix: the in-memory form the device path ingests (built once per variant list, like `gt_matrix`)."""
        key = (id(self.variants), len(self.variants))
        c = getattr(self, "_vcols", None)
        if c is None or c[0] != key:
            pos = np.array([v.pos for v in self.variants], dtype=np.int64)
            reflen = np.array([len(v.ref) for v in self.variants], dtype=np.int64)
            altlen = np.array([len(v.alt) for v in self.variants], dtype=np.int64)
            ref_blob = np.frombuffer("".join(v.ref for v in self.variants).encode("ascii"), dtype=np.uint8)
            alt_blob = np.frombuffer("".join(v.alt for v in self.variants).encode("ascii"), dtype=np.uint8)
            off = lambda ln: np.concatenate(([0], np.cumsum(ln)))
            c = (key, dict(pos=pos, ref_blob=ref_blob, ref_off=off(reflen), alt_blob=alt_blob, alt_off=off(altlen)))
            self._vcols = c
        return c[1]

    @property
    def startp(self) -> int:  # padded start (reference Coordinate.start)
        return max(0, self.bed_start - PADDING)

    @property
    def stopp(self) -> int:  # padded stop (reference Coordinate.stop)
        return self.bed_stop + PADDING

    @property
    def sequence(self) -> str:
        return self.contig_seq[self.startp - 1 : self.stopp]

    def vcf_fields(self, v: VariantSite) -> List[str]:
        """The tab-split VCF row the reference's VariantRecord.read_vcf_line consumes."""
        gts = [f"{int(a)}|{int(b)}" for a, b in v.gt]
        return [self.contig, str(v.pos), ".", v.ref, v.alt, ".", "PASS", f"AF={v.af:.6g}", "GT"] + gts


def make_region(
    seed: int,
    contig: str,
    contig_len: int,
    bed_start: int,
    bed_stop: int,
    iupac_frac: float = 0.0,
) -> SynthRegion:
    rng = np.random.default_rng(seed)
    return SynthRegion(contig, random_sequence(rng, contig_len, iupac_frac), bed_start, bed_stop)


def add_phased_variants(
    reg: SynthRegion,
    seed: int,
    n_sites: int,
    n_samples: int,
    frac_snv: float = 0.90,
    frac_del: float = 0.05,
    max_indel: int = 8,
    af_min: Optional[float] = None,
    af_max: float = 0.5,
    edge_margin: int = 1,
    panel: str = "independent",
    n_founders: int = 128,
    block_sites: int = 3000,
) -> SynthRegion:
    """Place ``n_sites`` non-overlapping variant sites inside the padded region.

    SNV / deletion / insertion mix 90/5/5 %, indel length 1+Geometric(0.5) capped at
    ``max_indel``; AF log-uniform on [af_min, af_max]; every one of the 2*n_samples
    haplotype columns carries the alt independently with probability AF
    (``panel="independent"``: no linkage, the worst case for haplotype uniqueness - SURVEY 8(d)'s C3).
    ``panel="linked"``: the columns are mosaics of ``n_founders`` founder haplotypes (drawn as above), switching founder after
    Geometric(1 / block_sites) sites (~100 kb at C3's density) - linkage blocks as in a real phased panel: neighbouring
    variants travel together, so variant clusters are shared by more chromosome copies.
    """
    rng = np.random.default_rng(seed)
    n_hap = 2 * n_samples
    if af_min is None:
        af_min = 1.0 / n_hap
    lo = reg.startp + edge_margin  # first allowed 1-based position
    hi = reg.stopp - edge_margin - max_indel - 1  # last allowed start so REF allele fits
    span = max_indel + 2  # footprint reserved per site: keeps sites non-overlapping
    n_slots = (hi - lo + 1) // span
    if n_sites > n_slots:
        raise ValueError(f"too many variant sites ({n_sites}) for region ({n_slots} slots)")
    slots = np.sort(rng.choice(n_slots, size=n_sites, replace=False))
    jitter = rng.integers(0, 2, size=n_sites)  # 0/1 nt jitter inside the slot
    kinds = rng.random(n_sites)
    lens = np.minimum(rng.geometric(0.5, size=n_sites), max_indel)
    afs = np.exp(rng.uniform(np.log(af_min), np.log(af_max), size=n_sites))
    alt_pick = rng.integers(1, 4, size=n_sites)
    ins_bases = rng.integers(0, 4, size=(n_sites, max_indel))
    seq = reg.contig_seq
    reg.samples = [f"S{i:04d}" for i in range(n_samples)]
    out: List[VariantSite] = []
    ks: List[int] = []  # row of gt_all behind every record of `out`
    gt_all = np.empty((n_sites, n_hap), dtype=np.uint8)
    if panel == "linked":
        founders = (rng.random((n_sites, n_founders)) < afs[:, None]).astype(np.uint8)
        lrng = np.random.default_rng(seed ^ 0x5EED1)
        for c in range(n_hap):
            k = 0
            while k < n_sites:
                k1 = min(n_sites, k + int(lrng.geometric(1.0 / block_sites)))
                gt_all[k:k1, c] = founders[k:k1, int(lrng.integers(0, n_founders))]
                k = k1
    elif panel == "independent":
        for k0 in range(0, n_sites, 4096):  # chunked: 31k x 5008 float64 would be 1.2 GB at once
            k1 = min(n_sites, k0 + 4096)
            gt_all[k0:k1] = rng.random((k1 - k0, n_hap)) < afs[k0:k1, None]
    else:
        raise ValueError(f"unknown panel kind {panel!r}")
    empty = np.flatnonzero(~gt_all.any(axis=1))  # keep every site carried by at least one haplotype
    gt_all[empty, rng.integers(0, n_hap, size=len(empty))] = 1
    for k in range(n_sites):
        pos = int(lo + slots[k] * span + jitter[k])
        refb = seq[pos - 1]
        if refb not in "ACGT":
            continue  # no variant on an ambiguous reference base
        gt = gt_all[k].reshape(n_samples, 2)
        ks.append(k)
        if kinds[k] < frac_snv:
            altb = "ACGT"[("ACGT".index(refb) + int(alt_pick[k])) % 4]
            out.append(VariantSite(pos, refb, altb, float(afs[k]), gt))
        elif kinds[k] < frac_snv + frac_del:
            ln = int(lens[k])
            out.append(VariantSite(pos, seq[pos - 1 : pos + ln], refb, float(afs[k]), gt))
        else:
            ln = int(lens[k])
            ins = "".join("ACGT"[b] for b in ins_bases[k, :ln])
            out.append(VariantSite(pos, refb, refb + ins, float(afs[k]), gt))
    # The reference clamps a variant's REF span with the *original* region length
    # (haplotype.py:199-201: ``if posrel_stop > self._size``), so a site whose haplotype
    # offset has been pushed past the region end by upstream insertions makes it raise
    # "Mismatching reference alleles".  Keep sites out of that tail: the guard is the
    # largest total inserted length any one haplotype carries.
    if out:
        ins_len = np.array([max(0, v.chain) for v in out], dtype=np.int64)
        ins_rows = np.flatnonzero(ins_len > 0)
        ins_gt = gt_all[np.asarray(ks, dtype=np.int64)[ins_rows]]  # [kept insertion, hap] (sites on ambiguous REF bases were skipped)
        guard = int((ins_len[ins_rows, None] * ins_gt.astype(np.int64)).sum(axis=0).max()) if len(ins_rows) else 0
        keep = [i for i, v in enumerate(out) if v.pos + len(v.ref) + guard <= reg.stopp]
        out, ks = [out[i] for i in keep], [ks[i] for i in keep]
    reg.variants = out
    reg.gt_matrix = gt_all[np.asarray(ks, dtype=np.int64)] if ks else None
    reg.variant_columns()
    return reg


# --- named configurations (BASELINE.json configs / SURVEY.md §8d) -----------------

def config_c1() -> SynthRegion:
    """C1/C2: 12 kb contig, BED chrS 1000 11000 -> 10 201-nt region, no VCF."""
    return make_region(1001, "chrS", 12_000, 1_000, 11_000)


def config_c3(n_samples: int = 2504, n_sites: int = 31_000, region_len: int = 1_000_000) -> SynthRegion:
    """C3: 1.2 Mb synthetic chr22, BED 100000..1100000, 2504 phased samples, 31k sites."""
    reg = make_region(1003, "chr22", region_len + 200_000, 100_000, 100_000 + region_len)
    return add_phased_variants(reg, 1003_1, n_sites, n_samples)


def cfd_tables(seed: int = 2001) -> Tuple[np.ndarray, np.ndarray]:
    """Seeded synthetic CFD tables (the real Doench-2016 pickles are fetched from Zenodo by
    the reference at run time and are not available offline).

    Returns ``mm[20, 4, 4]`` indexed [position, wildtype-RNA base (A,C,G,U), sgRNA base
    (A,C,G,T)] and ``pam[16]`` indexed by the dinucleotide 4*b0+b1 over (A,C,G,T).
    """
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, size=(20, 4, 4)), rng.uniform(0.0, 1.0, size=16)


def cfd_tables_as_dicts(mm: np.ndarray, pam: np.ndarray):
    """The two dicts in the key format reference compute_cfd expects
    (scores/cfdscore/cfdscore.py:88-94): ``r{wt}:d{RC(sg)},{i+1}`` and ``{pam[-2:]}``."""
    rna, dna = "ACGU", "ACGT"
    rc = {"A": "T", "C": "G", "G": "C", "T": "A"}
    mmd = {}
    for i in range(20):
        for a in range(4):
            for b in range(4):
                mmd[f"r{rna[a]}:d{rc[dna[b]]},{i + 1}"] = float(mm[i, a, b])
    pamd = {dna[a] + dna[b]: float(pam[4 * a + b]) for a in range(4) for b in range(4)}
    return mmd, pamd


def deepcpf1_weights(seed: int = 2002) -> dict:
    """Seeded N(0, 0.1) fp32 parameters in the torch layout of the reference's SeqDeepCpf1
    (scores/deepCpf1/seqdeepcpf1.py:43-56): conv (80,4,5), fc 1200-80-40-40-1."""
    rng = np.random.default_rng(seed)

    def n(*shape):
        return rng.normal(0.0, 0.1, size=shape).astype(np.float32)

    return dict(
        conv_w=n(80, 4, 5), conv_b=n(80),
        w1=n(80, 1200), b1=n(80), w2=n(40, 80), b2=n(40),
        w3=n(40, 40), b3=n(40), w4=n(1, 40), b4=n(1),
    )


# sgrna_net().state_dict() of the reference's PLM-CRISPR (scores/plm_crispr/train_general.py:12-51), in its order
PLMCRISPR_SHAPES = (
    ("conv1.weight", (64, 5, 5)), ("conv1.bias", (64,)), ("conv2.weight", (64, 64, 5)), ("conv2.bias", (64,)),
    ("conv3.weight", (64, 64, 5)), ("conv3.bias", (64,)), ("conv4.weight", (64, 5, 5)), ("conv4.bias", (64,)),
    ("text_cnn.convs.0.weight", (128, 1280, 5)), ("text_cnn.convs.0.bias", (128,)),
    ("text_cnn.convs.1.weight", (128, 1280, 9)), ("text_cnn.convs.1.bias", (128,)),
    ("text_cnn.convs.2.weight", (128, 1280, 13)), ("text_cnn.convs.2.bias", (128,)),
    ("lin1.weight", (2048, 7552)), ("lin1.bias", (2048,)), ("lin3.weight", (256, 2048)), ("lin3.bias", (256,)),
    ("lin4.weight", (256, 384)), ("lin4.bias", (256,)), ("lin5.weight", (128, 256)), ("lin5.bias", (128,)),
    ("lin6.weight", (1, 128)), ("lin6.bias", (1,)),
    ("weight_net.0.weight", (128, 512)), ("weight_net.0.bias", (128,)),
    ("weight_net.2.weight", (2, 128)), ("weight_net.2.bias", (2,)),
)


def plmcrispr_weights(seed: int = 2003) -> dict:
    """Seeded fp32 parameters of PLM-CRISPR in torch layout, keyed by state_dict name (PLMCRISPR_SHAPES): weights are
    N(0, 1) x 3 / sqrt(fan_in) with fan_in the product of all but the first dimension, biases N(0, 0.1^2).  torch's default
    initialisation squeezes every score into 0.461-0.469, where a structural mistake hides; this family spreads them."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in PLMCRISPR_SHAPES:
        if name.endswith(".bias"):
            out[name] = rng.normal(0.0, 0.1, size=shape).astype(np.float32)
        else:
            fan_in = int(np.prod(shape[1:]))
            out[name] = (rng.standard_normal(size=shape, dtype=np.float32) * np.float32(3.0 / np.sqrt(fan_in))).astype(np.float32)
    return out


def plmcrispr_protein(seed: int, L: int) -> np.ndarray:
    """A stand-in for a per-residue ESM embedding: (L, 1280) N(0, 1), rounded through fp16 as the reference's loader does."""
    rng = np.random.default_rng([seed, L])
    return rng.standard_normal(size=(L, 1280), dtype=np.float32).astype(np.float16).astype(np.float32)


# --- C4: a whole contig with a phased panel too large to hold as a dense matrix ------------------
class BlockGenotypes:
    """The SURVEY §8(d) genotype recipe (every chromosome copy carries the alt independently with probability AF) as a
    function of (variant, column) that is generated on demand: the matrix is cut into fixed blocks of `vblock` variants
    x `cblock` columns, each block drawn from its own `default_rng([seed, variant block, column block])`, so any
    rectangle - a tile's variants x a rank's columns - is reproducible whatever the tiling or the number of ranks.
    Interface of tiling.DenseGenotypes: carried(var_lo, var_hi, col_lo, col_hi)."""

    def __init__(self, seed: int, af: np.ndarray, n_cols: int, vblock: int = 4096, cblock: int = 626):
        self.seed, self.af, self.n_cols, self.vblock, self.cblock = seed, np.asarray(af, dtype=np.float32), n_cols, vblock, cblock

    def block(self, vb: int, cb: int) -> np.ndarray:
        v0, v1 = vb * self.vblock, min(len(self.af), (vb + 1) * self.vblock)
        c0, c1 = cb * self.cblock, min(self.n_cols, (cb + 1) * self.cblock)
        rng = np.random.default_rng([self.seed, vb, cb])
        return rng.random((v1 - v0, c1 - c0), dtype=np.float32) < self.af[v0:v1, None]

    def dense(self, var_lo: int, var_hi: int, col_lo: int, col_hi: int) -> np.ndarray:
        out = np.zeros((var_hi - var_lo, col_hi - col_lo), dtype=bool)
        for vb in range(var_lo // self.vblock, (max(var_hi, var_lo + 1) - 1) // self.vblock + 1):
            v0 = vb * self.vblock
            a, b = max(var_lo, v0), min(var_hi, v0 + self.vblock)
            if b <= a:
                continue
            for cb in range(col_lo // self.cblock, (max(col_hi, col_lo + 1) - 1) // self.cblock + 1):
                c0 = cb * self.cblock
                c, d = max(col_lo, c0), min(col_hi, c0 + self.cblock)
                if d <= c:
                    continue
                out[a - var_lo:b - var_lo, c - col_lo:d - col_lo] = self.block(vb, cb)[a - v0:b - v0, c - c0:d - c0]
        return out

    def carried(self, var_lo: int, var_hi: int, col_lo: int, col_hi: int):
        counts = np.zeros(col_hi - col_lo, dtype=np.int64)
        parts = []
        step = self.cblock
        for c in range(col_lo, col_hi, step):  # column slabs: the transpose scan stays cache-sized
            d = min(col_hi, c + step)
            sub = self.dense(var_lo, var_hi, c, d)
            sites, cols = np.nonzero(sub)  # variant-major scan, then a stable (radix) sort by column: (column, variant) order
            order = np.argsort(cols.astype(np.uint16), kind="stable")
            counts[c - col_lo:d - col_lo] = np.bincount(cols, minlength=d - c)
            parts.append(sites[order].astype(np.uint32))
        return counts, (np.concatenate(parts) if parts else np.zeros(0, np.uint32))


def contig_panel(seed: int, contig: str, contig_len: int, n_block: int, n_samples: int, sites_per_mb: float = 31_000.0,
                 frac_snv: float = 0.90, frac_del: float = 0.05, max_indel: int = 8):
    """C4: an iid ACGT contig with one leading N block and a phased panel at 1000G density over the
    non-N part, fully vectorised (1.25 M sites for chr22).  Returns (contig bases as a uint8 array, tiling.VariantPanel
    with BlockGenotypes).  Sites are non-overlapping (one per slot of max_indel + 2 bases) and never touch N."""
    from .tiling import VariantPanel
    rng = np.random.default_rng(seed)
    seq = np.empty(contig_len, dtype=np.uint8)
    seq[:n_block] = ord("N")
    seq[n_block:] = _ACGT[rng.integers(0, 4, size=contig_len - n_block)]
    span = max_indel + 2
    lo = n_block + 201            # 1-based first allowed position: clear of the N block and of the region pad
    hi = contig_len - 200 - span  # keep the tail free: inserted bases push later variants towards the region end
    n_slots = max(0, (hi - lo) // span)
    n_sites = min(n_slots, int(round(sites_per_mb * (contig_len - n_block) / 1e6)))
    slots = np.sort(rng.choice(n_slots, size=n_sites, replace=False))
    pos = lo + slots * span + rng.integers(0, 2, size=n_sites)
    kinds = rng.random(n_sites)
    lens = np.minimum(rng.geometric(0.5, size=n_sites), max_indel)
    n_cols = 2 * n_samples
    af = np.exp(rng.uniform(np.log(1.0 / n_cols), np.log(0.5), size=n_sites))
    alt_pick = rng.integers(1, 4, size=n_sites)
    ins = rng.integers(0, 4, size=(n_sites, max_indel))
    code = np.zeros(256, dtype=np.int64)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = i
    refb = seq[pos - 1]
    is_snv = kinds < frac_snv
    is_del = ~is_snv & (kinds < frac_snv + frac_del)
    ref: List[str] = [None] * n_sites
    alt: List[str] = [None] * n_sites
    refc = [chr(c) for c in refb.tolist()]
    snv_alt = _ACGT[(code[refb] + alt_pick) % 4]
    sa = [chr(c) for c in snv_alt.tolist()]
    blob = seq.tobytes()
    for k in np.flatnonzero(is_snv).tolist():
        ref[k], alt[k] = refc[k], sa[k]
    for k in np.flatnonzero(is_del).tolist():
        p = int(pos[k])
        ref[k], alt[k] = blob[p - 1:p + int(lens[k])].decode(), refc[k]
    for k in np.flatnonzero(~is_snv & ~is_del).tolist():
        ref[k], alt[k] = refc[k], refc[k] + "".join("ACGT"[b] for b in ins[k, :int(lens[k])])
    vid = [f"{contig}-{p}-{r}/{a}" for p, r, a in zip(pos.tolist(), ref, alt)]
    samples = [f"S{i:04d}" for i in range(n_samples)]
    return seq, VariantPanel(pos.astype(np.int64), ref, alt, vid, af.astype(np.float64), samples,
                             BlockGenotypes(seed + 1, af, n_cols))


def write_region_files(reg: SynthRegion, directory: str, stem: str = "region"):
    """The region as the FILES the reference's `crisprhawk search` takes - FASTA (60 columns), BED, phased VCF text (one `a|b`
    per sample and record, `AF=` in INFO) - for the files -> TSV measurements and tests.  Returns (fasta, bed, vcf) paths."""
    import os
    fa, bed, vcf = (os.path.join(directory, f"{stem}.{ext}") for ext in ("fa", "bed", "vcf"))
    with open(fa, "w") as f:
        f.write(f">{reg.contig}\n")
        s = reg.contig_seq
        f.write("\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n")
    with open(bed, "w") as f:
        f.write(f"{reg.contig}\t{reg.bed_start}\t{reg.bed_stop}\n")
    ns = len(reg.samples)
    with open(vcf, "wb") as f:
        f.write(b"##fileformat=VCFv4.2\n##contig=<ID=" + reg.contig.encode() + b">\n")
        f.write(("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(reg.samples) + "\n").encode())
        for v in reg.variants:
            head = f"{reg.contig}\t{v.pos}\t.\t{v.ref}\t{v.alt}\t.\tPASS\tAF={v.af:.6g}\tGT\t".encode()
            g = np.empty((ns, 4), np.uint8)
            g[:, 0] = v.gt[:, 0] + 48
            g[:, 1] = ord("|")
            g[:, 2] = v.gt[:, 1] + 48
            g[:, 3] = 9
            f.write(head + g.reshape(-1).tobytes()[:-1] + b"\n")
    return fa, bed, vcf



# ---------------------------------------------------------------------------------------------- gnomAD sites records
GNOMAD_POPS = ["afr", "ami", "amr", "asj", "eas", "fin", "nfe", "mid", "sas", "remaining"]
_GN_COUNTS = ["0", "00", "5", "0,0,5", "-3", "2147483647", "3,.", "0", "0", "12", "1", "0,0", "7,0"]
_GN_FILTERS = ["PASS", "PASS", "PASS", ".", "AC0", "AC0;PASS", "PASSED", "NOPASS", "AS_VQSR;AC0"]
_GN_QUALS = [".", "1234", "0.1", "57.25", "1e3", "100000", "3.4e-05", "0"]


def gnomad_sites_header(joint: bool) -> List[str]:
    """The header lines of a sites VCF as gnomad_sites_lines fills it (no FORMAT, no samples)."""
    af = "AF_joint" if joint else "AF"
    return ["##fileformat=VCFv4.2", '##FILTER=<ID=AC0,Description="Allele count is zero">',
            f'##INFO=<ID={af},Number=A,Type=Float,Description="Alternate allele frequency">',
            '##INFO=<ID=AC_afr,Number=A,Type=Integer,Description="Alternate allele count, African">', "##contig=<ID=chr21,length=46709983>",
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]


def gnomad_sites_lines(seed: int, n_records: int, joint: bool, info_keys: int = 150) -> List[str]:
    """Data lines of a gnomAD-like sites VCF, every one convertible: the ten allele-count keys of the file's kind with counts
    of every accepted form, and around them the keys that must NOT be taken for them - `AC_afr_XX`, `XAC_afr`, `nhomalt_afr`,
    the other kind's `AC_joint_afr` / `AC_afr`, an `AC_afr=5` inside another entry's value, flags without '=' - each with a count
    opposite to the real key's, up to about `info_keys` entries in shuffled order.  FILTER, QUAL, AF (absent, '.', lists; a
    joint file has `AF_joint` and no `AF`) and the number of ALT alleles vary; positions ascend on chr21."""
    rng = np.random.default_rng(seed)
    real = [f"AC_joint_{p}" if joint else f"AC_{p}" for p in GNOMAD_POPS]
    other = [f"AC_{p}" if joint else f"AC_joint_{p}" for p in GNOMAD_POPS]
    lines, pos = [], 5_000_000
    for r in range(n_records):
        pos += int(rng.integers(1, 400))
        n_alt = int(rng.choice([1, 1, 1, 1, 2, 3]))
        ref = random_sequence(rng, int(rng.choice([1, 1, 1, 2, 5])))
        alts = []
        while len(alts) < n_alt:
            a = random_sequence(rng, int(rng.choice([1, 1, 1, 3, 9])))
            if a != ref and a not in alts:
                alts.append(a)
        entries = []
        for k, (key, okey, p) in enumerate(zip(real, other, GNOMAD_POPS)):
            val = _GN_COUNTS[int(rng.integers(0, len(_GN_COUNTS)))]
            seen = any(int(e) > 0 for e in val.split(",") if e != ".") if val != "3,." else True
            decoy = "0" if seen else "9"
            entries.append(f"{key}={val}")
            entries += [f"{key}_XX={decoy}", f"X{key}={decoy}", f"{okey}={decoy}", f"nhomalt_{p}={decoy}", f"AN_{p}={int(rng.integers(2, 90000))}",
                        f"note{k}={key}={decoy}"]
        af_kind = int(rng.integers(0, 6))
        af_key = "AF_joint" if joint else "AF"
        if af_kind == 1:
            entries.append(f"{af_key}=.")
        elif af_kind == 2:
            entries.append(f"{af_key}=0.5,.")
        elif af_kind >= 3:
            entries.append(f"{af_key}=" + ",".join(f"{float(rng.random()) * 10 ** -int(rng.integers(0, 7)):.5e}" for _ in range(n_alt)))
        k = 0
        while len(entries) < info_keys:
            kind = int(rng.integers(0, 4))
            if kind == 0:
                entries.append(f"flag{k}")
            elif kind == 1:
                entries.append(f"faf95_{k}={float(rng.random()):.6e}")
            elif kind == 2:
                entries.append(f"vep{k}=" + "|".join(random_sequence(rng, int(rng.integers(1, 12))) for _ in range(int(rng.integers(1, 9)))))
            else:
                entries.append(f"AN_grp{k}={int(rng.integers(0, 200000))}")
            k += 1
        order = rng.permutation(len(entries))
        info = ";".join(entries[int(i)] for i in order)
        vid = f"rs{int(rng.integers(1, 10 ** 9))}" if rng.random() < 0.5 else "."
        lines.append("\t".join(["chr21", str(pos), vid, ref, ",".join(alts), _GN_QUALS[int(rng.integers(0, len(_GN_QUALS)))],
                                _GN_FILTERS[int(rng.integers(0, len(_GN_FILTERS)))], info]))
    return lines
