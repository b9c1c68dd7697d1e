"""Shared by tests/test_unphased_effects_host.py and tests/test_gpu_unphased_effects.py: the two unphased reports of
tests/golden/g16_effects_unphased.json.gz (made by tests/golden/make_golden_effects_unphased.py from the reference's own stage),
their haplotypes rebuilt by the project's host builder, their report groups through the host chain (rows derived from the
strings as resolve_refs derives them -> hawk_host_resolve_unphased -> hawk_host_unphased_groups), and their input files."""
import functools
import io

import numpy as np

import resolve_refs as rr
import ugroups_refs as ug
from crisprhawk_hip import haplotypes as H, readers, reports, synth
from crisprhawk_hip.coordinate import Coordinate
from crisprhawk_hip.haplotype import Haplotype
from crisprhawk_hip.pam import PAM
from crisprhawk_hip.region import Region
from crisprhawk_hip.search_guides import compute_scan_start_stop
from crisprhawk_hip.sequence import Sequence
from crisprhawk_hip.variant import VariantRecord
from util import load_golden

INPUTS = ["unphased", "unphased_dense"]
TABLES = ["cfdon", "cfdon_two", "cfdon_none_valid", "azimuth", "azimuth_two", "azimuth_nans"]
FLANKS = [(0, 0), (4, 3)]
CFD = synth.cfd_tables()


@functools.lru_cache(maxsize=None)
def g16():
    return load_golden("g16_effects_unphased.json.gz")


@functools.lru_cache(maxsize=None)
def fixture(name):
    """the g7-style fixture dict of an input: the stored file, or the dict g16 carries"""
    return load_golden("g7_report_unphased.json.gz") if name == "unphased" else g16()["fixtures"][name]["fixture"]


def vcf_rows(fx):
    return [[fx["contig"], str(p), ".", r, a, ".", "PASS", f"AF={af:.6g}", "GT"] + [f"{g[0]}/{g[1]}" for g in gts] for p, r, a, af, gts in fx["variants"]]


def write_files(fx, tmp_path, with_records=True):
    """FASTA, BED and unphased VCF of a fixture (with_records=False: the header alone) -> (fa, bed, vcf)"""
    tmp_path.mkdir(parents=True, exist_ok=True)
    contig_seq = "N" * (fx["startp"] - 1) + fx["region_seq"] + "ACGT" * 10
    fa, bed, vcf = str(tmp_path / "g.fa"), str(tmp_path / "r.bed"), str(tmp_path / ("v.vcf" if with_records else "empty.vcf"))
    readers.write_fasta(fa, fx["contig"], contig_seq, 80)
    with open(bed, "w") as f:
        f.write(f"{fx['contig']}\t{fx['bed_start']}\t{fx['bed_stop']}\n")
    readers.write_vcf(vcf, fx["contig"], fx["samples"], vcf_rows(fx) if with_records else [], False)
    return fa, bed, vcf


def fixture_pam(fx):
    pam = PAM(fx["pam"], fx["right"], True)
    pam.encode(0)
    return pam


@functools.lru_cache(maxsize=None)
def built(name):
    """(fixture, region, haplotypes, pam): the haplotypes by haplotypes.add_variants_unphased on the fixture's records"""
    fx = fixture(name)
    region = Region(Sequence(fx["region_seq"], True), Coordinate(fx["contig"], fx["bed_start"], fx["bed_stop"], synth.PADDING))
    recs = []
    for f in vcf_rows(fx):
        r = VariantRecord(True)
        r.read_vcf_line(f, fx["samples"], False)
        recs.append(r)
    haps = [Haplotype(Sequence(region.sequence.sequence, True), region.coordinates, False, 0, True)]
    haps = H.add_variants_unphased(haps, region, fx["samples"], recs, False, True)
    for i, h in enumerate(haps):
        h.id = f"hap_{i:08d}"
    assert sum(h.samples == "REF" for h in haps) == 1 and len(haps) == len(fx["haplotypes"])
    return fx, region, haps, fixture_pam(fx)


@functools.lru_cache(maxsize=None)
def host_report(name, flank=(0, 0)):
    """(fixture, UnphasedGroups of the host chain, HapLabels, (cols, order, plain)) - computed once, never written to"""
    fx, region, haps, pam = built(name)
    hits = []
    for h in haps:
        a, b = compute_scan_start_stop(h, region.start, region.stop, len(pam))
        hits.append(rr.py_pam_hits(h.sequence.sequence, pam, a, b))
    t = rr.derive_rows(haps, hits, len(pam), fx["guidelen"], fx["right"])
    res = rr.twin(haps, t, pam, fx["guidelen"], fx["right"])
    g = ug.host_groups(haps, t, res, pam, fx["guidelen"], fx["right"], flank, CFD)
    lab = reports.HapLabels.from_objects(haps)
    is_ref = np.array([h.samples == "REF" for h in haps], dtype=bool)
    columns = reports.group_columns(g, lab, pam, fx["contig"], fx["target"], with_cfdon=True, is_ref_hap=is_ref)
    return fx, g, lab, columns


def assert_report_equals_reference(text, fx, want_text=None):
    """column-equal to the reference's TSV (or to `want_text`); haplotype ids by their count: the reference numbers the indel
    window haplotypes in the order it walks a set of carriers, so the ids of those rows are its own"""
    import pandas as pd
    got = pd.read_csv(io.StringIO(text), sep="\t", dtype=str, keep_default_na=False)
    want = pd.read_csv(io.StringIO(fx["report_tsv"] if want_text is None else want_text), sep="\t", dtype=str, keep_default_na=False)
    assert list(got.columns) == list(want.columns) and len(got) == len(want)
    for c in got.columns:
        if c != "haplotype_id":
            assert (got[c] == want[c]).all(), (c, got[c][got[c] != want[c]].head(), want[c][got[c] != want[c]].head())
    assert (got["haplotype_id"].str.count(",") == want["haplotype_id"].str.count(",")).all()


def table_args(name, key):
    """(candidate ids, score column name) of one stored table"""
    rec = g16()["fixtures"][name]
    return (rec["candidates"][key.split("_", 1)[1]] if "_" in key else []), ("score_cfdon" if key.startswith("cfdon") else "score_azimuth")


def type_table_text(counts):
    return "guide_type\tcount\n" + "".join(f"{k}\t{v}\n" for k, v in counts.items())


def assert_subreport_equals_reference(text, want_text, report_text, fx):
    """a candidate's sub-report: the reference's under the report's own rule (every column as text, haplotype ids by count), and
    byte for byte the header and the rows of OUR written report that start at the candidate's position"""
    assert_report_equals_reference(text, fx, want_text)
    lines = report_text.splitlines(keepends=True)
    start = text.splitlines()[1].split("\t")[1]
    assert text == lines[0] + "".join(ln for ln in lines[1:] if ln.split("\t")[1] == start)
