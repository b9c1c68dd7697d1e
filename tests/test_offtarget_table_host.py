"""The off-targets table from hit records, host side: hawk_host_offtarget_text runs the emitter the device kernels run
(csrc/hawk_ottext.h: ot_text_row) without a device, so the statement of a row is held to the package's own host chain
(tests/ottable_refs.py) and to fixture g10 on a machine without a GPU."""
import os
import re

import numpy as np
import pytest

import ottable_refs as R
from crisprhawk_hip import _lib, synth
from util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table_order(rows):
    """offtargets_table's order: stable by (chrom as a string, position)"""
    keys = [(r.split("\t")[0], int(r.split("\t")[1])) for r in rows]
    return sorted(range(len(rows)), key=lambda i: keys[i])


@pytest.mark.parametrize("name", ["ngg", "cpf1"])
def test_fixture_targets_become_the_fixture_table(name):
    """Every line of g10's targets.txt - the hand-made DNA / RNA rows included - as a record: the host emitter's rows equal the
    package's chain byte for byte, and in the table's order they are the fixture's offtargets_tsv.
    One byte per hand-made DNA row is compared in upper case: the fixture's generator wrote the bulged base of those rows in
    lower case (make_golden.py: `site.lower()`), a record carries the window as 2-bit codes and prints a bulged base as it is
    (GenomeIndex._bulge_hit does the same).  That byte is located through the '-' of the row's grna field; every other byte of
    the file is compared as it stands."""
    fx = load_golden("g10_offtargets.json.gz")[name]
    tables = synth.cfd_tables() if fx["cfdon"] else None
    cols, guides, names = R.records_from_targets(fx["targets_txt"], fx["pam"], fx["right"])
    assert {int(k) for k in cols["kind"]} == {0, 1, 2}
    rows_of = np.arange(len(names), dtype=np.uint32)
    offs = np.zeros(len(names), dtype=np.uint64)
    want, want_units, want_uns = R.expected(cols, guides, fx["pam"], fx["right"], names, offs, tables)
    rc, got, off, units, n_uns = R.host_text(cols, guides, fx["guidelen"], fx["pam"], fx["right"], rows_of, offs, names, None, tables)
    assert rc == _lib.HAWK_OK
    assert got == want
    assert np.array_equal(units, want_units) and n_uns == want_uns == 0
    assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(r) for r in want])]).astype(np.uint64))
    # the table's order through `order`: the file
    order = np.array(_table_order(want), dtype=np.uint64)
    rc, got_sorted, _off, units_sorted, _ = R.host_text(cols, guides, fx["guidelen"], fx["pam"], fx["right"], rows_of, offs, names, order, tables)
    assert rc == _lib.HAWK_OK and got_sorted == [want[int(i)] for i in order] and np.array_equal(units_sorted, want_units[order])
    fixture = fx["offtargets_tsv"].split("\n")
    assert fixture[0] == "\t".join(R.OTREPCNAMES) and fixture[-1] == ""
    n_fixed = 0
    for k, row in enumerate(fixture[1:-1], 1):
        f = row.split("\t")
        if f[8] == "DNA":
            sp = list(f[4])
            for m in re.finditer("-", f[3]):
                assert sp[m.start()].islower()
                sp[m.start()] = sp[m.start()].upper()
                n_fixed += 1
            f[4] = "".join(sp)
            fixture[k] = "\t".join(f)
    assert n_fixed == 3
    assert "\n".join([fixture[0]] + got_sorted) + "\n" == "\n".join(fixture)


def test_cfd_text_is_pythons_repr_for_every_unit():
    """cfd text == repr(float(str(round(k / 1e4, 4)))) and cfd units == k for every k in 0..20000, and for values above 1
    (2.5, 12.3456) reached with table entries above 1: records with ONE mismatch each read the value from their own cell of the
    mismatch table (60 cells per call: 20 columns x the three other bases), the PAM's entry is 1."""
    guide = "ACGTTGCAAGCTTAGGCTCA"
    recs, cells = [], []
    for c in range(20):
        a = "ACGT".index(guide[c])
        for d in range(1, 4):
            site = guide[:c] + "ACGT"[(a + d) % 4] + guide[c + 1:]
            recs.append(R.make_record(0, guide, site, "AGG", False, q=len(recs)))
            cells.append((c, a, (a + d) % 4))
    cols = R.columns(recs)
    values = list(range(20001)) + [25000, 123456]
    pt = np.ones(16)
    rows_of, offs = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
    for lo in range(0, len(values), len(cells)):
        ks = values[lo:lo + len(cells)]
        mm = np.ones((20, 4, 4))
        for k, (c, a, b) in zip(ks, cells):
            mm[c, a, b] = k / 1e4
        rc, rows, _off, units, n_uns = R.host_text(cols, [guide], 20, "NGG", False, rows_of, offs, ["chr1"], None, (mm, pt))
        assert rc == _lib.HAWK_OK and n_uns == 0
        for k, row, u in zip(ks, rows, units.tolist()):
            assert u == k
            assert row.split("\t")[9] == repr(float(str(round(k / 1e4, 4)))), k
    assert repr(float(str(round(25000 / 1e4, 4)))) == "2.5" and repr(float(str(round(123456 / 1e4, 4)))) == "12.3456"


@pytest.mark.parametrize("pam_text,G,right,with_tables", [("NGG", 20, False, True), ("NGG", 20, False, False), ("TTTV", 23, True, False),
                                                          ("NGG", 20, True, True), ("NGG", 27, False, True), ("TTTV", 26, True, True)])
def test_random_records_of_every_kind(pam_text, G, right, with_tables):
    """X / DNA / RNA records of sizes 0..2 with random interior gaps, ambiguous bases anywhere, several contigs and row offsets
    past 2^32, with and without tables: rows, offsets, CFD units and the unscorable count equal the chain's"""
    rng = np.random.default_rng(G * 7 + right)
    guides = ["".join(rng.choice(list("ACGT"), size=G)) for _ in range(5)]
    names = ["c", "chr2", "chromosome_seventeen", "x" * 300]
    row_contig = np.array([0, 1, 1, 2, 3, 0], dtype=np.uint32)
    row_off = np.array([0, 0, 1 << 22, 999_999_999, 5, (1 << 32) + 12345], dtype=np.uint64)
    recs = R.random_records(rng, 400, guides, len(pam_text), right, len(row_contig))
    cols = R.columns(recs)
    tables = synth.cfd_tables() if with_tables else None
    row_names = [names[int(c)] for c in row_contig]
    want, want_units, want_uns = R.expected(cols, guides, pam_text, right, row_names, row_off, tables)
    rc, got, _off, units, n_uns = R.host_text(cols, guides, G, pam_text, right, row_contig, row_off, names, None, tables)
    assert rc == _lib.HAWK_OK
    assert got == want and np.array_equal(units, want_units) and n_uns == want_uns
    assert (want_uns > 0) == with_tables  # with p(N) = 0.02 per base some row has an N under a lookup
    assert {int(k) for k in cols["kind"]} == {0, 1, 2}


def test_malformed_records_are_refused_with_nothing_written():
    guide = "ACGTTGCAAGCTTAGGCTCA"
    good = R.valid_dna_record(guide)
    rows_of, offs = np.zeros(2, np.uint32), np.array([0, 100], dtype=np.uint64)

    def run(recs, order=None):
        return R.host_text(R.columns(recs), [guide], 20, "NGG", False, rows_of, offs, ["chr1"], order, synth.cfd_tables())
    rc, rows, off, cfd, _ = run([good, good])
    assert rc == _lib.HAWK_OK and len(rows) == 2
    for what, change in R.malformed_cases():
        rc, rows, off, cfd, _ = run([good, dict(good, **change)])
        assert rc == _lib.HAWK_E_INVALID, what
        assert rows is None and (off == 0xFFFFFFFFFFFFFFFF).all() and (cfd == -7).all(), what
    rc, rows, off, cfd, _ = run([good, good], order=np.array([1, 2], dtype=np.uint64))
    assert rc == _lib.HAWK_E_INVALID and (off == 0xFFFFFFFFFFFFFFFF).all()
    # n = 0 is fine
    rc, rows, off, cfd, _ = R.host_text(R.columns([]), [guide], 20, "NGG", False, rows_of, offs, ["chr1"], None, None)
    assert rc == _lib.HAWK_OK and rows == [] and off.tolist() == [0]


def test_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "hawk.h")).read()
    for sym in ("hawk_offtarget_text", "hawk_offtarget_text_download", "hawk_host_offtarget_text"):
        assert sym in _lib.EXPORTS
        assert re.search(r"^int " + sym + r"\(", header, re.M), sym
    assert hasattr(_lib.lib(), "hawk_host_offtarget_text")
