"""Inputs for the tests of the unphased indel-window builder (workload.expand_unphased_from_vcf(indel_windows="device"),
hawk_uwin_*, hawk_host_unphased_windows): a seam panel on unphased_build_refs.Case - the smallest shapes at which the window
geometry, the carrier walk, the survival rule, the grouping and the row fill can go wrong - the declines, and the comparison of a
twin's or the device's window rows with haplotypes.unphased_indel_windows'.  No device work here."""
import numpy as np

import unphased_build_refs as ub
from crisprhawk_hip import haplotypes as hap_mod

Case = ub.Case


def wcase(name: str, length: int, n_samples: int, seed: int) -> Case:
    """a Case whose sample names do NOT sort in column order: the carrier walk goes by name, the genotype columns do not"""
    c = Case(name, length, n_samples, seed=seed)
    perm = np.random.default_rng(1000 + seed).permutation(n_samples)
    if n_samples > 1 and np.array_equal(perm, np.arange(n_samples)):
        perm = perm[::-1]
    c.samples = [f"P{int(p):03d}" for p in perm]
    return c


def ins(c: Case, off: int, n: int, gts, seed: int = 0):
    rng = np.random.default_rng(7 * off + n + seed)
    return c.insertion(off, "".join("ACGT"[i] for i in rng.integers(0, 4, n)), gts)


def panel():
    """name -> Case; every case builds under the host builder without raising"""
    cases = {}

    def add(c):
        cases[c.name] = c.sort()
    het = {0: "0/1", 1: "1/1"}
    # window start alignment: a mod 32 = 0, 31, 0, 1 (indels at 100, 131, 132, 133) and windows clamped at the region's start
    c = wcase("starts_unclamped", 500, 3, 1)
    for k, off in enumerate((100, 131, 132, 133)):
        (ins(c, off, 2 + k, het) if k % 2 else c.deletion(off, 2 + k, het))
    c.snv(40, {0: "0/1"}).snv(99, {1: "0/1"}).snv(180, {0: "0/1", 1: "0/1"}).snv(232, {1: "1/0"})
    add(c)
    c = wcase("starts_clamped", 400, 3, 2)
    # (a window must reach the region's 100th base, where the scan of a region without padding starts: an insertion at o grows by o
    # at the most)
    for k, off in enumerate((0, 1, 31, 32, 33, 99)):
        (ins(c, off, min(1 + k, off), {k % 3: "0/1"}) if k % 2 else c.deletion(off, 1 + k, {k % 3: "0/1", 2: "1/1"}))
    c.snv(5, {0: "0/1", 2: "0/1"}).snv(64, {1: "0/1"}).snv(130, {2: "0/1"})
    add(c)
    # right clamp: indels within 100 of the region's end, a deletion whose ref ends on the last base, an insertion on the last
    # base (outside indel_in_region: no row)
    c = wcase("right_clamp", 600, 4, 3)
    ins(c, 599, 3, {0: "0/1"})
    c.deletion(594, 5, {1: "0/1", 2: "0/1"})
    ins(c, 550, 7, {0: "0/1", 3: "1/1"})
    c.deletion(500, 4, {2: "0/1"})
    ins(c, 499, 2, {3: "0/1"})
    c.snv(470, {2: "0/1", 3: "0/1"}).snv(560, {0: "0/1", 1: "0/1"}).snv(598, {1: "0/1", 3: "0/1"})
    add(c)
    # indel sizes: insertions of 1, 31, 32, 33, 64, 100 and deletions of 1, 31, 32, 33, 64 bases; an SNV in every window, some in the
    # tail a deletion's position map does not reach
    c = wcase("sizes_insertions", 1300, 3, 4)
    for k, n in enumerate((1, 31, 32, 33, 64, 100)):
        off = 120 + 190 * k
        ins(c, off, n, {k % 3: "0/1", (k + 1) % 3: "1/0"})
        c.snv(off - 37, {k % 3: "0/1"}).snv(off + 64, {(k + 1) % 3: "0/1"})
    add(c)
    c = wcase("sizes_deletions", 1300, 3, 5)
    for k, n in enumerate((1, 31, 32, 33, 64)):
        off = 120 + 230 * k
        c.deletion(off, n, {k % 3: "0/1", (k + 1) % 3: "1/0"})
        c.snv(off - 37, {k % 3: "0/1"}).snv(off + n + 99, {(k + 1) % 3: "0/1"}).snv(off + n + 100, {k % 3: "0/1", (k + 1) % 3: "0/1"})
    add(c)
    # finished rows of 32k - 1, 32k, 32k + 1 bases through clamping: a one-base insertion at o < 100 gives o + 101 bases
    c = wcase("row_lengths", 400, 3, 6)
    for k, off in enumerate((26, 27, 28, 58, 59, 60)):
        ins(c, off, 1, {k % 3: "0/1"})
    c.deletion(300, 3, {0: "0/1"})   # 400 - 200 - 3 = 197 bases ... and the right clamp's own: L - a + grow
    c.snv(3, {0: "0/1", 1: "0/1", 2: "0/1"}).snv(126, {0: "0/1"}).snv(127, {1: "0/1"}).snv(128, {2: "0/1"})
    add(c)
    # SNV placement around a deletion and an insertion
    c = wcase("snvs_around_a_deletion", 700, 6, 7)
    c.deletion(300, 5, {s: "0/1" for s in range(6)})
    c.snv(300, {0: "0/1"})                       # at the anchor: written, overwritten, kept in the allele table
    c.snv(303, {1: "0/1"})                       # strictly inside the deleted span
    c.snv(306, {2: "0/1"})                       # the first base behind it
    c.snv(200, {3: "0/1"}).snv(405, {3: "1/1"})  # the window's first and last base (the last one: in the tail, listed only)
    c.snv(401, {4: "0/1"}).snv(400, {5: "0/1"})  # the tail's first base (skipped) and the last base that is written
    add(c)
    c = wcase("snvs_around_an_insertion", 700, 5, 8)
    ins(c, 300, 4, {s: "0/1" for s in range(5)})
    c.snv(300, {0: "0/1"}).snv(301, {1: "0/1"}).snv(200, {2: "0/1"}).snv(396, {2: "1/1", 3: "0/1"}).snv(299, {4: "0/1"})
    add(c)
    # two carriers that differ only by a skipped or an overwritten SNV: one row, both variants strings
    c = wcase("merged_over_unwritten_snvs", 700, 4, 9)
    c.deletion(300, 6, {s: "0/1" for s in range(4)})
    c.snv(250, {s: "0/1" for s in range(4)}).snv(300, {1: "0/1"}).snv(304, {2: "0/1"}).snv(404, {3: "0/1"})
    add(c)
    # carriers: 1, 63, 64, 65, 129 of one indel, names out of column order; some without an SNV in the window
    for n in (1, 63, 64, 65, 129):
        c = wcase(f"carriers_{n}", 500, max(n, 2) + (1 if n < 129 else 0), 20 + n)
        ns = len(c.samples)
        rng = np.random.default_rng(n)
        carriers = sorted(rng.permutation(ns)[:n].tolist())
        c.deletion(250, 2, {s: ("0/1", "1/0", "1/1", "./1")[s % 4] for s in carriers})
        for off in (170, 249, 290, 349):
            gts = ub._random_gts(rng, ns, 0.3)
            c.snv(off, gts or {carriers[0]: "0/1"})
        add(c)
    # equal rows that are not adjacent in name order; all carriers equal; a carrier with no SNV in the window
    c = wcase("equal_rows_apart", 600, 8, 10)
    ins(c, 300, 3, {s: "0/1" for s in range(7)})
    c.snv(260, {0: "0/1", 2: "0/1", 4: "0/1", 6: "1/1"}).snv(340, {1: "0/1", 3: "0/1"}).snv(341, {3: "0/1"})   # {0,2,4,6}, {1}, {3}, {5}
    add(c)
    c = wcase("all_carriers_equal", 600, 5, 11)
    c.deletion(300, 2, {s: "0/1" for s in range(5)}).snv(280, {s: "1/1" for s in range(5)})
    add(c)
    # a multi-allelic record, 1/2: a deletion at the record's position and an insertion that normalises two bases further
    c = wcase("multi_allelic", 600, 4, 12)
    r3 = c.seq[300:303]
    c.raw(300, r3, r3[0] + "," + r3 + "AC", {0: "1/2", 1: "0/2", 2: "1/0"})
    c.snv(290, {0: "0/1", 2: "0/1"}).snv(302, {1: "0/1"}).snv(310, {0: "0/1", 1: "0/1"})
    add(c)
    # two indels of one sample inside each other's windows; an indel nobody carries; SNVs of a sample that carries no indel
    c = wcase("overlapping_windows", 700, 4, 13)
    c.deletion(300, 3, {0: "0/1", 1: "0/1"})
    ins(c, 320, 2, {0: "0/1", 2: "0/1"})
    ins(c, 340, 5, {})
    c.deletion(360, 40, {})
    c.snv(310, {0: "0/1", 3: "0/1"}).snv(330, {1: "0/1", 2: "0/1", 3: "1/1"})
    add(c)
    c = wcase("indels_alone", 300, 2, 14)
    c.deletion(120, 1, {1: "0/1"})
    ins(c, 10, 2, {0: "1/1", 1: "0/1"})
    add(c)
    return cases


def declines():
    """name -> (Case, the reason expand_unphased_from_vcf(indel_windows="device") declines with): one per new reason and an indel
    ref that REF does not hold"""
    out = {}
    c = wcase("insertion_longer_than_the_flank", 500, 3, 41)
    ins(c, 250, 101, {0: "0/1"})
    c.snv(200, {1: "0/1"})
    out[c.name] = (c, 8)
    c = wcase("indel_base_outside_acgt", 500, 3, 42)
    c.insertion(250, "NN", {0: "0/1"}).snv(200, {1: "0/1"})
    out[c.name] = (c, 9)
    c = wcase("indel_ref_mismatch", 500, 3, 43)
    c.raw(250, c.seq[250] + c.other(251) + c.seq[252], c.seq[250], {0: "0/1"}).snv(200, {1: "0/1"})
    out[c.name] = (c, 4)
    for c, _ in out.values():
        c.sort()
    return out


def host_windows(c: Case):
    """(region, every host-built haplotype, the window haplotypes among them)"""
    region, haps = c.host()
    return region, haps, haps[1 + len(ub.whole_region_rows(haps)):]


def spy_on_the_host_window_builder(monkeypatch):
    """counts calls of what the device window route must never touch"""
    from crisprhawk_hip.haplotype import Haplotype
    from crisprhawk_hip.variant import VariantRecord
    calls = {"windows": 0, "add": 0, "read": 0}

    def counted(owner, name, key):
        real = getattr(owner, name)

        def f(*a, **k):
            calls[key] += 1
            return real(*a, **k)
        monkeypatch.setattr(owner, name, f)
    counted(hap_mod, "unphased_indel_windows", "windows")
    counted(hap_mod, "add_variants_unphased", "add")
    counted(Haplotype, "add_variants_unphased", "add")
    counted(VariantRecord, "read_vcf_line", "read")
    return calls
