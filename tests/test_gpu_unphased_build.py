"""The whole-region rows of an unphased VCF built on the device (workload.expand_unphased_from_vcf: hawk_gt_parse_unphased,
hawk_ubuild_lists, hawk_ubuild_signatures, hawk_ubuild_fill, hawk_hapset_pack_ascii_rows) against the host-built set: the set
search_guides._device_set makes of haplotypes.add_variants_unphased's haplotypes.  Equality is bit for bit over the whole plane
array, lengths, REF flags, the scan ranges (read back through a search's table), labels and the allele table; every case that
must not decline asserts that the host builder was not called for the whole-region set.  Then the declines, and
pipeline.search_files(unphased_haplotypes="device") against "host", every written file byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import unphased_build_refs as ub
from crisprhawk_hip import _lib, haplotypes as hap_mod, pipeline, readers, search_guides as sg, synth, workload
from crisprhawk_hip.hapset import _p
from crisprhawk_hip.pam import PAM
from resolve_refs import G4_FIXTURES
from test_gpu_unphased_groups import _g4_files, _g7_files
from util import load_golden

pytestmark = pytest.mark.gpu
PANEL = ub.panel()
DECLINES = ub.declines()
TABLES = synth.cfd_tables()
PAMLEN, GUIDELEN = 3, 20


class _Spy:
    """calls of the host builder's whole-region set (add_variants_unphased) and the lines search_files prints at level 3"""

    def __init__(self, monkeypatch):
        self.whole, self.lines = 0, []
        real = hap_mod.add_variants_unphased

        def add(*a, **k):
            self.whole += 1
            return real(*a, **k)
        monkeypatch.setattr(hap_mod, "add_variants_unphased", add)
        monkeypatch.setattr(pipeline, "print_verbosity", lambda msg, *a: self.lines.append(msg))


def _build(c):
    return workload.expand_unphased_from_vcf(c.seq, c.coord.start, c.coord.stop, c.block(), c.samples, PAMLEN, coord=c.coord)


def _table(ds):
    pam = PAM("NGG", False, True)
    pam.encode(0)
    t = ds.search(pam.bits, pam.bitsrc, PAMLEN, GUIDELEN, False)
    o = np.lexsort((t.strand, t.pos, t.hap))
    return t.n_rows, t.hap[o], t.pos[o], t.strand[o], t.start[o], t.stop[o], t.win[:, o]


def _assert_same_set(c, built, region, haps):
    ds, labels, alleles, windows, ms = built
    want = sg._device_set(region, haps, PAMLEN)
    try:
        assert ds.n_hap == want.n_hap and ds.stride == want.stride
        assert np.array_equal(ds.hap_len, want.hap_len) and np.array_equal(ds.is_ref, want.is_ref) and ds.ref_index == want.ref_index == 0
        assert np.array_equal(ds.planes(), want.planes())   # the whole array: guard words and padding bits too
        ub.assert_labels_equal(labels, haps)
        ub.assert_alleles_equal(alleles, haps)
        a, b = _table(ds), _table(want)   # the scan ranges decide which PAM positions are in the table
        assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
        n_whole = len(ub.whole_region_rows(haps))
        assert [w.sequence.sequence for w in windows] == [h.sequence.sequence for h in haps[1 + n_whole:]]
    finally:
        want.close()
        ds.close()


@pytest.mark.parametrize("name", sorted(PANEL))
def test_device_built_set_equals_the_host_built_set(name, monkeypatch):
    c = PANEL[name]
    region, haps = c.host()
    spy = _Spy(monkeypatch)
    built = _build(c)
    assert spy.whole == 0   # nothing fell back
    _assert_same_set(c, built, region, haps)


@pytest.mark.parametrize("fixture", G4_FIXTURES)
def test_device_built_set_on_the_reference_fixtures(fixture, monkeypatch):
    c = ub.g4_case(load_golden(f"{fixture}.json.gz"))
    region, haps = c.host()
    spy = _Spy(monkeypatch)
    built = _build(c)
    assert spy.whole == 0 and built[0].n_hap > 2
    _assert_same_set(c, built, region, haps)


def _parse(rows, n_samples):
    L, ctx = _lib.lib(), _lib.context(None)
    blk = ub.block_of(rows)
    g, ms = C.c_void_p(), C.c_float(0)
    text = np.ascontiguousarray(blk.text)
    _lib.check(L.hawk_gt_parse_unphased(ctx, _p(text), C.c_uint64(len(text)), _p(blk.line_off), _p(blk.gt_off), C.c_uint64(len(blk)), n_samples,
                                        C.byref(g), C.byref(ms)), "hawk_gt_parse_unphased")
    codes, flags = np.zeros((len(rows), 2 * n_samples), np.uint8), np.zeros(len(rows), np.uint8)
    _lib.check(L.hawk_gt_codes(g, _p(codes), _p(flags)), "hawk_gt_codes")
    return g, codes, flags


def test_unphased_parse_equals_the_rule_on_every_form():
    """every plain and every flagged form in every column of short records, a record with a missing column, one with a column too
    many, and records of 1100 columns (4096-byte sweeps of the workgroup) with a flagged form at the sweep's seam"""
    L = _lib.lib()
    forms = ub.PLAIN + ub.FLAGGED
    rows = []
    for k in range(len(forms)):
        rows.append(["chrU", str(100 + k), ".", "A", "C", ".", "PASS", "AF=0.1", "GT:DP"] + [forms[(k + s) % len(forms)] for s in range(5)])
    rows.append(rows[0][:-1])
    rows.append(rows[1] + ["0/1"])
    g, codes, flags = _parse(rows, 5)
    L.hawk_gt_destroy(g)
    want_c, want_f = ub.record_codes(rows, 5)
    assert np.array_equal(codes, want_c) and np.array_equal(flags, want_f) and want_f[-2] & 2 and want_f[-1] & 2
    wide = []
    for k in range(6):
        cols = [ub.PLAIN[(s * 7 + k) % len(ub.PLAIN)] for s in range(1100)]
        if k % 2:
            cols[1020 + k] = ub.FLAGGED[k]
        wide.append(["chrU", str(200 + k), ".", "A", "C", ".", "PASS", "AF=0.1", "GT"] + cols)
    g, codes, flags = _parse(wide, 1100)
    L.hawk_gt_destroy(g)
    want_c, want_f = ub.record_codes(wide, 1100)
    assert np.array_equal(codes, want_c) and np.array_equal(flags, want_f) and want_f.tolist().count(0) == 3
    assert max(len("\t".join(r)) for r in wide) > 4096


@pytest.mark.parametrize("name", sorted(PANEL))
def test_lists_and_signatures_equal_the_twins(name):
    c = PANEL[name]
    L = _lib.lib()
    g, codes, flags = _parse(c.rows, len(c.samples))
    u = C.c_void_p()
    try:
        want_c, want_f = ub.record_codes(c.rows, len(c.samples))
        assert np.array_equal(codes, want_c) and not flags.any()
        rows, labels, alleles, (w_off, w_idx), w_sig, groups = workload.unphased_rows_host(c.seq, c.coord.start, c.block(), c.samples, codes)
        vt = workload.VcfVariants(c.block())
        sel, v_line, v_allele, v_off, v_mask, v_ref = workload.unphased_snv_table(c.block(), vt, len(c.seq), c.coord.start)
        off, ms = np.zeros(len(c.samples) + 1, np.uint64), C.c_float(0)
        _lib.check(L.hawk_ubuild_lists(g, _p(v_line), _p(v_allele), _p(v_off), _p(v_mask), _p(v_ref), len(sel), _p(off), C.byref(u), C.byref(ms)),
                   "hawk_ubuild_lists")
        assert np.array_equal(off, w_off)
        idx, sig, dec = np.zeros(int(off[-1]), np.uint32), np.zeros((len(c.samples), 2), np.uint64), C.c_int64(-1)
        _lib.check(L.hawk_ubuild_lists_download(u, _p(idx)), "hawk_ubuild_lists_download")
        _lib.check(L.hawk_ubuild_signatures(u, _p(sig), C.byref(dec), C.byref(ms)), "hawk_ubuild_signatures")
        assert np.array_equal(idx, w_idx) and np.array_equal(sig, w_sig) and dec.value == -1
        assert workload.group_unphased_rows(off, idx, sig, v_off, v_mask, v_ref) == groups
    finally:
        if u:
            L.hawk_ubuild_free(u)
        L.hawk_gt_destroy(g)


def test_grouping_compares_the_lists_when_signatures_collide():
    """a hash may group rows, the comparison decides: with every signature forced equal the groups stay what the sites say"""
    c = PANEL["interleaved_and_equal"]
    codes, _ = ub.record_codes(c.rows, len(c.samples))
    rows, labels, alleles, (off, idx), sig, groups = workload.unphased_rows_host(c.seq, c.coord.start, c.block(), c.samples, codes)
    vt = workload.VcfVariants(c.block())
    sel, v_line, v_allele, v_off, v_mask, v_ref = workload.unphased_snv_table(c.block(), vt, len(c.seq), c.coord.start)
    assert workload.group_unphased_rows(off, idx, np.zeros_like(sig), v_off, v_mask, v_ref) == groups and len(groups) == 5


def test_fill_refuses_what_it_cannot_write():
    """rows outside the set, a target of another length, REF among the targets, a sample the lists do not have: HAWK_E_INVALID
    before any launch; a REF row that does not hold the variant's ref base: the decline word, and nothing faults"""
    from crisprhawk_hip.hapset import DeviceHapSet
    c = PANEL["snvs_only"]
    L = _lib.lib()
    g, codes, flags = _parse(c.rows, len(c.samples))
    u = C.c_void_p()
    vt = workload.VcfVariants(c.block())
    sel, v_line, v_allele, v_off, v_mask, v_ref = workload.unphased_snv_table(c.block(), vt, len(c.seq), c.coord.start)
    wrong_ref = ((v_ref + 1) % 4).astype(np.uint8)
    off, ms, dec = np.zeros(len(c.samples) + 1, np.uint64), C.c_float(0), C.c_int64(-1)
    n = len(c.seq)
    ds = DeviceHapSet.allocate(np.array([n, n, n, 50], np.uint32))
    try:
        ds.pack_rows(0, [c.seq])
        _lib.check(L.hawk_ubuild_lists(g, _p(v_line), _p(v_allele), _p(v_off), _p(v_mask), _p(wrong_ref), len(sel), _p(off), C.byref(u), C.byref(ms)),
                   "hawk_ubuild_lists")
        rs = np.array([0, 1], np.uint32)
        fill = lambda ref_row, first, nrows, rows: L.hawk_ubuild_fill(u, ds._h, ref_row, first, nrows, _p(rows), C.byref(dec), C.byref(ms))
        assert fill(0, 3, 2, rs) == _lib.HAWK_E_INVALID and fill(0, 2, 2, rs) == _lib.HAWK_E_INVALID   # past the set; a 50-nt row
        assert fill(1, 1, 2, rs) == _lib.HAWK_E_INVALID and fill(0, 1, 2, np.array([0, 3], np.uint32)) == _lib.HAWK_E_INVALID
        assert fill(3, 1, 2, rs) == _lib.HAWK_E_INVALID   # a REF row shorter than the sites
        assert fill(0, 1, 2, rs) == _lib.HAWK_E_UNSUPPORTED and dec.value == 0   # the first variant sample 0 carries
    finally:
        ds.close()
        if u:
            L.hawk_ubuild_free(u)
        L.hawk_gt_destroy(g)


def test_ranged_pack_leaves_the_other_rows_alone():
    from crisprhawk_hip.hapset import DeviceHapSet, HostHaplotype, PosSegments
    seqs = ["ACGTNNacgtRYKM" * 5, "TTTT" * 40 + "a", "GGcc" * 9]
    whole = DeviceHapSet([HostHaplotype(s, PosSegments.identity(0, len(s)), i == 0, (0, 0)) for i, s in enumerate(seqs)])
    ds = DeviceHapSet.allocate(np.array([len(s) for s in seqs], np.uint32))
    try:
        ds.pack_rows(1, seqs[1:2])
        got = ds.planes()
        assert np.array_equal(got[:, 1], whole.planes()[:, 1]) and not got[:, 0].any() and not got[:, 2].any()
        ds.pack_rows(0, seqs[0:1])
        ds.pack_rows(2, seqs[2:3])
        assert np.array_equal(ds.planes(), whole.planes())
        with pytest.raises(_lib.HawkStatusError):
            ds.pack_rows(2, ["GGcc" * 8])   # not the row's length
        with pytest.raises(_lib.HawkStatusError):
            ds.pack_rows(2, seqs[2:3] * 2)  # past the set
        with pytest.raises(_lib.HawkStatusError) as e:
            ds.pack_rows(2, ["GGc!" * 9])
        assert e.value.status == _lib.HAWK_E_IUPAC
    finally:
        ds.close()
        whole.close()


@pytest.mark.parametrize("name", sorted(DECLINES))
def test_builder_declines(name):
    c, reason = DECLINES[name]
    with pytest.raises(_lib.UnphasedBuildDeclined) as e:
        _build(c)
    assert e.value.reason == reason


# ---------------------------------------------------------------------------- files to TSV
def _written(outdir):
    out = {}
    for root, _, files in os.walk(outdir):
        for f in files:
            p = os.path.join(root, f)
            out[os.path.relpath(p, outdir)] = open(p, "rb").read()
    return out


def _both_builders(spy, tmp_path, fa, bed, vcf, pam, guidelen, right, device_taken=True, **kw):
    """the files "host" and "device" write, asserted equal; the route asserted by the spy and by the lap names"""
    spy.whole, spy.lines = 0, []
    th, td = {}, {}
    pipeline.search_files(fa, bed, [vcf], pam, guidelen, right, str(tmp_path / "host"), timings=th, unphased_haplotypes="host", **kw)
    assert spy.whole == 1 and pipeline.DEVICE_BUILT_LAP not in th
    assert pipeline.HOST_BUILT_LAP in th or kw.get("unphased_report") == "objects" or kw.get("unphased_engine") == "host"   # (the object route has no such lap)
    spy.whole = 0
    pipeline.search_files(fa, bed, [vcf], pam, guidelen, right, str(tmp_path / "device"), timings=td, unphased_haplotypes="device", **kw)
    if device_taken:
        assert spy.whole == 0 and pipeline.DEVICE_BUILT_LAP in td and pipeline.HOST_BUILT_LAP not in td and not any("built on the host" in m for m in spy.lines)
    else:
        assert spy.whole == 1 and pipeline.DEVICE_BUILT_LAP not in td
    a, b = _written(tmp_path / "host"), _written(tmp_path / "device")
    assert sorted(a) == sorted(b) and len(a) > 0
    for k in a:
        assert a[k] == b[k], k
    return a


def _azimuth_model():
    g9 = load_golden("g9_azimuth.json.gz")
    return {k: (np.array(v) if isinstance(v, list) else v) for k, v in g9["model"].items()}


@pytest.mark.parametrize("fixture", G4_FIXTURES)
def test_search_files_writes_the_same_files_under_both_builders(tmp_path, monkeypatch, fixture):
    fx, reg, fa, bed, vcf = _g4_files(tmp_path, fixture)
    spy = _Spy(monkeypatch)
    args = (fa, bed, vcf, fx["pam"], fx["guidelen"], fx["right"])
    files = _both_builders(spy, tmp_path / "cfd", *args, cfd_tables=TABLES)
    assert any(v.count(b"\n") > 1 for v in files.values())
    if not fx["right"] and fx["pam"] == "NGG":
        _both_builders(spy, tmp_path / "azimuth", *args, cfd_tables=TABLES, azimuth_model=_azimuth_model())
    fig = _both_builders(spy, tmp_path / "effects", *args, cfd_tables=TABLES, unphased_effects=True, graphical_reports=True)
    assert any(k.startswith("figures") for k in fig)


def test_g7_report_under_both_builders(tmp_path, monkeypatch):
    """g7 is NGG with the PAM on the right of the guide: the set on which Azimuth runs whatever the g4 sets' PAMs are"""
    fx, fa, bed, vcf = _g7_files(tmp_path)
    assert fx["pam"] == "NGG" and not fx["right"] and fx["guidelen"] == 20
    spy = _Spy(monkeypatch)
    args = (fa, bed, vcf, fx["pam"], fx["guidelen"], fx["right"])
    _both_builders(spy, tmp_path / "cfd", *args, cfd_tables=TABLES)
    az = _both_builders(spy, tmp_path / "azimuth", *args, cfd_tables=TABLES, azimuth_model=_azimuth_model())
    (report,) = [v for k, v in az.items() if "figures" not in k]
    head = report.split(b"\n")[0].split(b"\t")
    col = head.index(b"score_azimuth")
    assert any(line.split(b"\t")[col] != b"NA" for line in report.split(b"\n")[1:] if line)   # the scorer ran
    fig = _both_builders(spy, tmp_path / "effects", *args, cfd_tables=TABLES, azimuth_model=_azimuth_model(), unphased_effects=True,
                         graphical_reports=True)
    assert any(k.startswith("figures") for k in fig)


def test_routes_that_build_on_the_host_say_why(tmp_path, monkeypatch):
    fx, reg, fa, bed, vcf = _g4_files(tmp_path, "g4_unphased")
    spy = _Spy(monkeypatch)
    args = (fa, bed, vcf, fx["pam"], fx["guidelen"], fx["right"])
    files = _both_builders(spy, tmp_path / "table", *args, device_taken=False, cfd_tables=TABLES, haplotype_table=True)
    assert any(k.startswith("haplotypes_table") for k in files) and any("haplotype_table=True" in m for m in spy.lines)
    _both_builders(spy, tmp_path / "objects", *args, device_taken=False, unphased_report="objects")
    assert any("objects" in m and "built on the host" in m for m in spy.lines)
    _both_builders(spy, tmp_path / "engine", *args, device_taken=False, unphased_engine="host")
    assert any("host engine" in m and "built on the host" in m for m in spy.lines)
    monkeypatch.setenv("HAWK_UNPHASED_HAPLOTYPES", "device")   # the environment asks, the parameter still decides
    td = {}
    pipeline.search_files(*args[:2], [vcf], *args[3:], str(tmp_path / "env"), timings=td)
    assert pipeline.DEVICE_BUILT_LAP in td
    monkeypatch.setenv("HAWK_UNPHASED_HAPLOTYPES", "gpu")
    with pytest.raises(ValueError, match="HAWK_UNPHASED_HAPLOTYPES"):
        pipeline.search_files(*args[:2], [vcf], *args[3:], str(tmp_path / "env2"))


def _edited_vcf(tmp_path, reg, edit):
    rows = []
    for v in reg.variants:
        f = reg.vcf_fields(v)
        f[9:] = [g.replace("|", "/") for g in f[9:]]
        rows.append(f)
    rows = edit(rows)
    path = str(tmp_path / "edited.vcf")
    readers.write_vcf(path, reg.contig, reg.samples, rows, False)
    return path


@pytest.mark.parametrize("kind", ["haploid", "multi_base", "outside_acgt_never_carried"])
def test_a_declined_interval_is_the_host_builders(tmp_path, monkeypatch, kind):
    """declines the host builder accepts: the same files as under "host", the host builder called, the reason printed"""
    fx, reg, fa, bed, vcf = _g4_files(tmp_path, "g4_unphased")

    def edit(rows):
        if kind == "haploid":
            k = next(i for i, f in enumerate(rows) if "0/1" in f[9:] or "1/0" in f[9:] or "1/1" in f[9:])
            s = next(j for j in range(9, len(rows[k])) if rows[k][j] != "0/0")
            rows[k][s] = "1"
            return rows
        p = reg.bed_start + 57   # 1-based position inside the interval
        two = reg.contig_seq[p - 1:p + 1]
        first = "ACGT"[("ACGT".index(two[0]) + 1) % 4]
        new = ([reg.contig, str(p), ".", two, first + two[1], ".", "PASS", "AF=0.25", "GT"] + ["0/1"] + ["0/0"] * (len(reg.samples) - 1)
               if kind == "multi_base" else
               [reg.contig, str(p), ".", two[0], "N", ".", "PASS", "AF=0.25", "GT"] + ["0/0"] * len(reg.samples))
        rows = [f for f in rows if int(f[1]) != p] + [new]
        return sorted(rows, key=lambda f: int(f[1]))
    vcf2 = _edited_vcf(tmp_path, reg, edit)
    spy = _Spy(monkeypatch)
    _both_builders(spy, tmp_path / "out", fa, bed, vcf2, fx["pam"], fx["guidelen"], fx["right"], device_taken=False, cfd_tables=TABLES)
    want = {"haploid": _lib.UBUILD_REASONS[1], "multi_base": _lib.UBUILD_REASONS[2], "outside_acgt_never_carried": _lib.UBUILD_REASONS[3]}[kind]
    assert any("declined" in m and want in m for m in spy.lines)


RAISING = {"ref_mismatch": (4, ValueError), "alt_carried_twice": (7, None), "malformed_genotype": (1, ValueError), "phased_genotype": (1, ValueError)}


@pytest.mark.parametrize("kind", sorted(RAISING) + ["missing_column"])
def test_a_declined_interval_ends_as_under_the_host_builder(tmp_path, monkeypatch, kind):
    """The declines the host builder answers with an exception - a ref base the sequence does not hold, an alt one sample carries
    twice, a genotype that is no number, a phased genotype among unphased ones - and a record with a column missing: under "device"
    the reason is printed, the host builder is called, and the call ends as under "host" - the same exception type and text, the
    same files left (none where it raised).  Two reasons have no test of this kind: an SNV outside the region cannot come out of
    VCF.fetch_block, which hands out the records with start < POS <= stop only (the builder-level case gives it a block of its
    own), and more than 2^32 - 1 list entries need more memory than a test may take (nothing exercises HAWK_UBUILD_ENTRIES)."""
    from crisprhawk_hip.crisprhawk_error import CrisprHawkIupacTableError
    fx, reg, fa, bed, vcf = _g4_files(tmp_path, "g4_unphased")
    reason, exc = RAISING.get(kind, (1, None))
    if kind == "alt_carried_twice":
        exc = CrisprHawkIupacTableError

    def edit(rows):
        if kind in ("malformed_genotype", "phased_genotype", "missing_column"):
            k = max(i for i, f in enumerate(rows) if any(g != "0/0" for g in f[9:]))   # (not the first record: it decides `phased`)
            if kind == "missing_column":
                rows[k] = rows[k][:-1]
            else:
                col = max(j for j in range(9, len(rows[k])) if rows[k][j] != "0/0")
                rows[k][col] = "a/1" if kind == "malformed_genotype" else "0|1"
            return rows
        p = reg.bed_start + 57
        base = reg.contig_seq[p - 1]
        o1, o2 = ("ACGT"[("ACGT".index(base) + k) % 4] for k in (1, 2))
        gts = ["0/1"] + ["0/0"] * (len(reg.samples) - 1)
        head = [reg.contig, str(p), "."]
        new = ([head + [o1, o2, ".", "PASS", "AF=0.25", "GT"] + gts] if kind == "ref_mismatch" else
               [head + [base, o1, ".", "PASS", "AF=0.25", "GT"] + gts] * 2)
        return sorted([f for f in rows if int(f[1]) != p] + [list(f) for f in new], key=lambda f: int(f[1]))
    vcf2 = _edited_vcf(tmp_path, reg, edit)
    spy = _Spy(monkeypatch)

    def run(builder):
        out = tmp_path / builder
        try:
            pipeline.search_files(fa, bed, [vcf2], fx["pam"], fx["guidelen"], fx["right"], str(out), cfd_tables=TABLES, unphased_haplotypes=builder)
        except Exception as e:
            return "raised", type(e), str(e), _written(out)
        return "files", None, None, _written(out)
    host = run("host")
    host_calls = spy.whole   # (a genotype that is no number stops the host route in VariantRecord.read_vcf_line, before its builder)
    assert host_calls == (0 if kind in ("malformed_genotype", "phased_genotype") else 1) and spy.lines == []
    spy.whole = 0
    dev = run("device")
    assert dev == host
    assert spy.whole == host_calls and any("declined" in m and _lib.UBUILD_REASONS[reason] in m for m in spy.lines)
    if exc is not None:
        assert host[0] == "raised" and issubclass(host[1], exc) and host[3] == {}
    else:
        assert host[0] == "files" and len(host[3]) > 0
