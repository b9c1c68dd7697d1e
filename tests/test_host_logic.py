"""Host-side logic of the product package against reference-generated vectors (no GPU):
PAM class, haplotype construction on segments, scan bounds."""
import numpy as np
import pytest

from crisprhawk_hip.pam import PAM
from crisprhawk_hip.workload import build_phased_haplotypes
from crisprhawk_hip.expand import expand_haplotype, HaplotypeBuildError
from util import G3_CASES, load_golden, posmap_from_breaks, synth_region_from_fixture


def test_pam_class_matches_reference():
    g1 = load_golden("g1_tables.json.gz")
    for p in g1["pams"]:
        pm = PAM(p["pam"], p["right"], True)
        pm.encode(0)
        assert (pm.pam, pm.pamrc, pm.bits, pm.bitsrc, pm.bits_list, pm.cas_system, len(pm)) == (
            p["seq"], p["rc"], p["bits"], p["bitsrc"], p["bits_list"], p["cas_system"], p["length"])
    with pytest.raises(ValueError):
        PAM("NGX", False, True)
    assert str(PAM("ngg", False, True)) == "NGG"


@pytest.mark.parametrize("case", G3_CASES)
def test_haplotype_construction_on_segments(case):
    fx = load_golden(f"g3_search_{case}.json.gz")
    reg = synth_region_from_fixture(fx)
    haps, info = build_phased_haplotypes(reg, len(fx["pam"]))
    assert len(haps) == len(fx["haplotypes"])
    for h, i, gold, sc in zip(haps, info, fx["haplotypes"], fx["scan"]):
        assert bytes(h.seq).decode() == gold["seq"]
        assert sorted(i.samples) == gold["samples"]
        assert np.array_equal(h.seg.full(), posmap_from_breaks(gold["posmap_breaks"], gold["posmap_len"]))
        for g, rel in gold["posmap_rev_probe"]:
            assert h.seg.rev(g) == rel
        assert list(h.scan) == sc
        assert h.is_ref == (gold["samples"] == ["REF"])


def test_expand_errors():
    ref = np.frombuffer(b"ACGTACGTACGTACGTACGT", dtype=np.uint8)
    with pytest.raises(HaplotypeBuildError):  # reference ValueError: mismatching REF allele
        expand_haplotype(ref, 100, [(103, b"A", b"G")])
    with pytest.raises(HaplotypeBuildError):  # second variant sits on a deleted position
        expand_haplotype(ref, 100, [(103, b"TACG", b"T"), (105, b"C", b"CA")])
    out, seg = expand_haplotype(ref, 100, [(105, b"CGT", b"C")])  # SURVEY.md §7 probe
    assert out.tobytes() == b"ACGTAcACGTACGTACGT" and seg.full().tolist()[4:8] == [104, 105, 108, 109]
    out, seg = expand_haplotype(ref, 100, [(105, b"C", b"CAA")])
    assert out.tobytes() == b"ACGTAcaaGTACGTACGTACGT" and seg.full().tolist()[4:9] == [104, 105, 105, 105, 106]
    assert seg.rev(105) == 7


def test_variant_table_checks_ref_alleles():
    """workload._variant_table: the REF allele of every record must match the region (haplotype.py:203-208), first base
    and the whole span of a deletion, case-insensitively."""
    from crisprhawk_hip.workload import _variant_table
    seq = "ACGTacgtNNACGTACGT"
    ok = _variant_table(np.array([101, 105, 113]), ["A", "acg", "G"], ["C", "a", "GTT"], seq, 101)
    assert ok[0].tolist() == [0, 4, 12] and ok[1].tolist() == [1, 3, 1] and ok[2].tolist() == [0, -2, 2]
    with pytest.raises(HaplotypeBuildError):
        _variant_table(np.array([102]), ["A"], ["C"], seq, 101)            # region has C there
    with pytest.raises(HaplotypeBuildError):
        _variant_table(np.array([105]), ["ACT"], ["A"], seq, 101)          # deletion: third base differs
    with pytest.raises(HaplotypeBuildError):
        _variant_table(np.array([105]), [""], ["A"], seq, 101)                 # no REF allele at all


def _old_row_own(n, off, end, piece, L):
    """the owned starts of a row as the index computed them for mismatch-only windows before the tail rows existed"""
    return min(piece, n - off, end - off - L + 1) if end - off >= L else None


@pytest.mark.parametrize("guidelen,pamlen", [(20, 3), (23, 4), (29, 3)])
@pytest.mark.parametrize("piece", [64, 512, 1000, 4096])
def test_genome_row_geometry_owns_every_window_once(guidelen, pamlen, piece):
    """GenomeIndex's rows (genome.row_geometry) at the edges of the piece geometry: every window start of every window length
    the index can be asked about - RNA-bulged sites (spacer guidelen - 1, - 2: no extra overlap needed) up to DNA-bulged ones
    (guidelen + max_bulge) - is owned by exactly one row, and its window lies inside that row.  Mismatch-only windows keep the
    rows they had."""
    for max_bulge in range(0, min(2, 32 - guidelen - pamlen) + 1):  # windows of up to the 32 bases the device encodes
        _check_row_geometry(guidelen, pamlen, piece, max_bulge)


def _check_row_geometry(guidelen, pamlen, piece, max_bulge):
    from crisprhawk_hip.genome import min_spacer, row_geometry
    L = guidelen + pamlen
    overlap = L + max_bulge - 1
    lens = sorted({0, 1, *range(L - 3, L + 4), *range(piece - 1, piece + 2), *range(piece + L - 4, piece + L + 3),
                   2 * piece + overlap - 1, 2 * piece + overlap, 2 * piece + overlap + 1, 3 * piece, 3 * piece + 1})
    lengths = {f"c{n}": n for n in lens}
    spans = None
    for spacer in range(min_spacer(guidelen), guidelen + max_bulge + 1):
        Lw = spacer + pamlen
        geo = row_geometry(lengths, guidelen, pamlen, piece, max_bulge, spacer)
        if spans is None:
            spans = [r[:3] for r in geo]
        assert [r[:3] for r in geo] == spans  # the rows themselves do not depend on the window
        owned = {name: np.zeros(n + 1, dtype=np.int64) for name, n in lengths.items()}
        for name, off, end, own in geo:
            n = lengths[name]
            assert 0 <= off < end <= n and own >= 0
            if own:
                assert off + own - 1 + Lw <= end  # the last owned window lies inside the row
            owned[name][off:off + own] += 1
        for name, n in lengths.items():
            m = max(0, n - Lw + 1)  # starts s with s + Lw <= n
            bad = np.flatnonzero(owned[name][:m] != 1)
            assert len(bad) == 0, f"{name}, window {Lw}: starts {bad[:8].tolist()} owned {owned[name][bad[:8]].tolist()} times"
            assert not owned[name][m:].any(), f"{name}, window {Lw}: a start past the last window is owned"
        assert [r[0] for r in geo] == sorted((r[0] for r in geo), key=list(lengths).index)  # contig order
    # mismatch-only windows: the rows that existed before own what they owned; the tail rows added for shorter windows own nothing
    for name, off, end, own in row_geometry(lengths, guidelen, pamlen, piece, max_bulge, guidelen):
        old = _old_row_own(lengths[name], off, end, piece, L)
        assert own == (0 if old is None else old)


def test_genome_index_refuses_before_device_work():
    """Windows the device cannot encode (more than 32 bases with the largest DNA bulge) and genomes without a single window are
    refused at construction, before any device is touched; the message names the shortest window."""
    from crisprhawk_hip.genome import GenomeIndex
    with pytest.raises(ValueError, match="32 bases"):
        GenomeIndex({"c": "ACGT" * 100}, 28, 3, max_bulge=2)
    with pytest.raises(ValueError, match="32 bases"):
        GenomeIndex({"c": "ACGT" * 100}, 30, 3)
    with pytest.raises(ValueError, match=r"18 \+ 3 bases"):
        GenomeIndex({"a": "ACGTACGTACGTACGTACGT", "b": ""}, 20, 3)


@pytest.mark.parametrize("G", [17, 20, 23])
def test_derived_guide_count_bounds_a_chunk(G):
    """scan_bulges sizes its guide slices by derived_per_guide: exact for DNA bulges, an upper bound for RNA bulges (identical
    deletions are kept once)."""
    from crisprhawk_hip.genome import _derived_guides, derived_per_guide
    rng = np.random.default_rng(G)
    for g in ("".join("ACGT"[i] for i in rng.integers(0, 4, G)), "A" * G, "AC" * (G // 2) + "A" * (G % 2)):
        for b in (1, 2):
            assert len(_derived_guides([g], G, b, True)[0]) == derived_per_guide(G, b, True)
            assert 0 < len(_derived_guides([g], G, b, False)[0]) <= derived_per_guide(G, b, False)
    assert derived_per_guide(20, 2, True) == 3040
