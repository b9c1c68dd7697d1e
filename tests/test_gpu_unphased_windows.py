"""The indel-window rows of an unphased VCF built on the device (workload.expand_unphased_from_vcf(indel_windows="device"):
hawk_uwin_instances, hawk_uwin_signatures, hawk_uwin_group, hawk_uwin_fill) against the host-built set - the set
search_guides._device_set makes of haplotypes.add_variants_unphased's haplotypes.  Equality is bit for bit over the whole plane
array, lengths, REF flags, the stride, labels, the allele table and the NGG/20 search table; every case asserts that neither
unphased_indel_windows nor add_variants_unphased nor VariantRecord.read_vcf_line was called.  Then instances, signatures and heads
against the host twin, the grouping under forged signatures, the refusals, the declines, and
pipeline.search_files(unphased_indel_windows="device") against "host", every written file byte for byte."""
import ctypes as C

import numpy as np
import pytest

import unphased_build_refs as ub
import unphased_window_refs as uw
from crisprhawk_hip import _lib, pipeline, search_guides as sg, synth, workload
from crisprhawk_hip.hapset import DeviceHapSet, _p
from resolve_refs import G4_FIXTURES
from test_gpu_unphased_build import _Spy, _azimuth_model, _edited_vcf, _parse, _table, _written
from test_gpu_unphased_groups import _g4_files, _g7_files
from util import load_golden

pytestmark = pytest.mark.gpu
PANEL = uw.panel()
DECLINES = uw.declines()
TABLES = synth.cfd_tables()
PAMLEN = 3


def _build(c, windows="device"):
    return workload.expand_unphased_from_vcf(c.seq, c.coord.start, c.coord.stop, c.block(), c.samples, PAMLEN, coord=c.coord, indel_windows=windows)


def _assert_device_windows_equal_host(c, monkeypatch):
    region, haps = c.host()
    calls = uw.spy_on_the_host_window_builder(monkeypatch)
    ds, labels, alleles, windows, ms = _build(c)
    assert calls == {"windows": 0, "add": 0, "read": 0} and windows == []   # no record object, no Haplotype, no host window
    want = sg._device_set(region, haps, PAMLEN)
    try:
        assert ds.n_hap == want.n_hap and ds.stride == want.stride
        assert np.array_equal(ds.hap_len, want.hap_len) and np.array_equal(ds.is_ref, want.is_ref) and ds.ref_index == want.ref_index == 0
        assert np.array_equal(ds.planes(), want.planes())   # the whole array: guard words and the bits past every row's end too
        ub.assert_labels_equal(labels, haps)
        ub.assert_alleles_equal(alleles, haps)
        a, b = _table(ds), _table(want)
        assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
    finally:
        want.close()
        ds.close()
    return ms, len(haps)


@pytest.mark.parametrize("name", sorted(PANEL))
def test_device_windows_equal_the_host_built_set(name, monkeypatch):
    ms, n = _assert_device_windows_equal_host(PANEL[name], monkeypatch)
    assert {"window_instances", "window_signatures", "window_groups", "window_fill"} <= set(ms) and n > 1


@pytest.mark.parametrize("fixture", G4_FIXTURES)
def test_device_windows_on_the_reference_fixtures(fixture, monkeypatch):
    ms, n = _assert_device_windows_equal_host(ub.g4_case(load_golden(f"{fixture}.json.gz")), monkeypatch)
    assert n > 2 and "window_fill" in ms


def test_host_windows_stay_the_default():
    c = PANEL["indels_alone"]
    ds, labels, alleles, windows, ms = workload.expand_unphased_from_vcf(c.seq, c.coord.start, c.coord.stop, c.block(), c.samples, PAMLEN, coord=c.coord)
    ds.close()
    assert len(windows) == 2 and not any(k.startswith("window") for k in ms)


class _Device:
    """the device objects of a case up to the instances: (g, u, w) and the arrays around them"""

    def __init__(self, c, rank=None):
        L = _lib.lib()
        self.L, self.c = L, c
        self.g, self.codes, flags = _parse(c.rows, len(c.samples))
        self.u, self.w = C.c_void_p(), C.c_void_p()
        assert not flags.any()
        vt = workload.VcfVariants(c.block())
        self.snv = workload.unphased_snv_table(c.block(), vt, len(c.seq), c.coord.start)
        sel, v_line, v_allele, v_off, v_mask, v_ref = self.snv
        is_snv = np.zeros(len(vt), bool)
        is_snv[sel] = True
        self.table = workload.IndelTable(vt, is_snv, len(c.seq), c.coord.start, c.coord)
        self.sample_off, ms = np.zeros(len(c.samples) + 1, np.uint64), C.c_float(0)
        _lib.check(L.hawk_ubuild_lists(self.g, _p(v_line), _p(v_allele), _p(v_off), _p(v_mask), _p(v_ref), len(sel), _p(self.sample_off),
                                       C.byref(self.u), C.byref(ms)), "hawk_ubuild_lists")
        self.ref = np.frombuffer(c.seq.encode(), np.uint8)
        self.rank = workload._name_ranks(c.samples) if rank is None else rank
        self.inp, self.keep = self.table.c_input(self.rank, self.ref)
        self.inst_off = np.zeros(len(self.table) + 1, np.uint64)
        self.dec = _lib.UbuildDecline()

    def instances(self):
        ms = C.c_float(0)
        return self.L.hawk_uwin_instances(self.g, self.u, C.byref(self.inp), _p(self.inst_off), C.byref(self.w), C.byref(self.dec), C.byref(ms))

    def close(self):
        if self.w:
            self.L.hawk_uwin_free(self.w)
        if self.u:
            self.L.hawk_ubuild_free(self.u)
        self.L.hawk_gt_destroy(self.g)


@pytest.mark.parametrize("name", sorted(PANEL))
def test_instances_signatures_and_heads_equal_the_twins(name):
    c = PANEL[name]
    d = _Device(c)
    try:
        t = workload.unphased_windows_host(c.seq, c.coord.start, c.block(), c.samples, d.codes, c.coord, PAMLEN)
        _lib.check(d.instances(), "hawk_uwin_instances")
        assert np.array_equal(d.inst_off, t["inst_off"])
        n = int(d.inst_off[-1])
        smp, lo, hi = np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        sig, head, ms = np.zeros((n, 2), np.uint64), np.zeros(n, np.uint32), C.c_float(0)
        _lib.check(d.L.hawk_uwin_download(d.w, _p(smp), _p(lo), _p(hi)), "hawk_uwin_download")
        assert np.array_equal(smp, t["inst_sample"]) and np.array_equal(lo, t["inst_lo"]) and np.array_equal(hi, t["inst_hi"])
        _lib.check(d.L.hawk_uwin_signatures(d.w, _p(sig), C.byref(d.dec), C.byref(ms)), "hawk_uwin_signatures")
        assert np.array_equal(sig, t["sig"]) and d.dec.reason == 0
        _lib.check(d.L.hawk_uwin_group(d.w, _p(sig), _p(head), C.byref(ms)), "hawk_uwin_group")
        assert np.array_equal(head, t["head"])
        # a signature may propose a row, the comparison decides: every signature forced equal, the heads stay what the sites say
        forged = np.zeros_like(sig)
        head2 = np.zeros(n, np.uint32)
        _lib.check(d.L.hawk_uwin_group(d.w, _p(forged), _p(head2), C.byref(ms)), "hawk_uwin_group")
        assert np.array_equal(head2, t["head"])
    finally:
        d.close()


def test_calls_refuse_what_they_cannot_index():
    """a rank that is no sample or comes twice, a record the block does not have, a pool range past the pool: HAWK_E_INVALID before
    any launch; rows outside the set, REF among them, a row of another length, an instance that does not exist: HAWK_E_INVALID
    before any write"""
    c = PANEL["indels_alone"]
    ns = len(c.samples)
    for rank in (np.array([0, ns], np.uint32), np.zeros(ns, np.uint32)):
        d = _Device(c, rank=rank)
        try:
            assert d.instances() == _lib.HAWK_E_INVALID and not d.w
        finally:
            d.close()
    d = _Device(c)
    try:
        d.table.line[0] = len(c.rows)
        assert d.instances() == _lib.HAWK_E_INVALID
        d.table.line[0] = 0
        d.inp.pool_len -= 1
        assert d.instances() == _lib.HAWK_E_INVALID
        d.inp.pool_len += 1
        _lib.check(d.instances(), "hawk_uwin_instances")
        n = int(d.inst_off[-1])
        lens = d.table.rowlen[np.repeat(np.arange(len(d.table)), np.diff(d.inst_off.astype(np.int64)))]
        L = len(c.seq)
        ds = DeviceHapSet.allocate(np.concatenate(([L], lens, [50])).astype(np.uint32))
        try:
            ds.pack_rows(0, [c.seq])
            ms = C.c_float(0)
            rows = np.arange(n, dtype=np.uint32)
            fill = lambda ref_row, first, nrows, ri: d.L.hawk_uwin_fill(d.w, ds._h, ref_row, first, nrows, _p(ri), C.byref(ms))
            assert fill(0, 2, n + 1, np.concatenate((rows, [0])).astype(np.uint32)) == _lib.HAWK_E_INVALID   # past the set
            assert fill(0, 0, n, rows) == _lib.HAWK_E_INVALID and fill(1, 1, n, rows) == _lib.HAWK_E_INVALID    # REF among the rows
            assert fill(0, 2, n, rows) == _lib.HAWK_E_INVALID                                                  # rows of other lengths
            assert fill(n + 1, 1, n, rows) == _lib.HAWK_E_INVALID                                              # a REF row of 50 bases
            assert fill(0, 1, n, np.full(n, n, np.uint32)) == _lib.HAWK_E_INVALID                              # no such instance
            before = ds.planes()
            assert not before[:, 1:].any()
            assert fill(0, 1, n, rows) == _lib.HAWK_OK
            assert np.array_equal(ds.planes()[:, 0], before[:, 0]) and not ds.planes()[:, n + 1].any()
        finally:
            ds.close()
    finally:
        d.close()


@pytest.mark.parametrize("name", sorted(DECLINES))
def test_builder_declines(name):
    c, reason = DECLINES[name]
    with pytest.raises(_lib.UnphasedBuildDeclined) as e:
        _build(c)
    assert e.value.reason == reason and "chrU-" in str(e.value)


# ---------------------------------------------------------------------------- files to TSV
def _both_windows(spy, monkeypatch, tmp_path, fa, bed, vcf, pam, guidelen, right, **kw):
    """the files unphased_indel_windows "host" and "device" write behind unphased_haplotypes="device", asserted equal; under
    "device" the host window builder is never called"""
    th, td = {}, {}
    pipeline.search_files(fa, bed, [vcf], pam, guidelen, right, str(tmp_path / "host"), timings=th, unphased_haplotypes="device",
                          unphased_indel_windows="host", **kw)
    assert pipeline.DEVICE_BUILT_LAP in th
    with monkeypatch.context() as m:
        calls = uw.spy_on_the_host_window_builder(m)
        spy.lines.clear()
        pipeline.search_files(fa, bed, [vcf], pam, guidelen, right, str(tmp_path / "device"), timings=td, unphased_haplotypes="device",
                              unphased_indel_windows="device", **kw)
        # (with the variant-effect stage on, search_files itself asks the VCF whether the interval has records: VCF.fetch reads lines)
        assert calls["windows"] == 0 and calls["add"] == 0 and (calls["read"] == 0 or kw.get("unphased_effects")) and pipeline.DEVICE_BUILT_LAP in td
        assert not any("built on the host" in m_ or "not used" in m_ for m_ in spy.lines)
    a, b = _written(tmp_path / "host"), _written(tmp_path / "device")
    assert sorted(a) == sorted(b) and len(a) > 0
    for k in a:
        assert a[k] == b[k], k
    return a


@pytest.mark.parametrize("fixture", G4_FIXTURES)
def test_search_files_writes_the_same_files_under_both_window_builders(tmp_path, monkeypatch, fixture):
    fx, reg, fa, bed, vcf = _g4_files(tmp_path, fixture)
    spy = _Spy(monkeypatch)
    args = (fa, bed, vcf, fx["pam"], fx["guidelen"], fx["right"])
    files = _both_windows(spy, monkeypatch, tmp_path / "cfd", *args, cfd_tables=TABLES)
    assert any(v.count(b"\n") > 1 for v in files.values())
    fig = _both_windows(spy, monkeypatch, tmp_path / "effects", *args, cfd_tables=TABLES, unphased_effects=True, graphical_reports=True)
    assert any(k.startswith("figures") for k in fig)


def test_g7_report_under_both_window_builders(tmp_path, monkeypatch):
    fx, fa, bed, vcf = _g7_files(tmp_path)
    spy = _Spy(monkeypatch)
    args = (fa, bed, vcf, fx["pam"], fx["guidelen"], fx["right"])
    _both_windows(spy, monkeypatch, tmp_path / "cfd", *args, cfd_tables=TABLES, azimuth_model=_azimuth_model())
    fig = _both_windows(spy, monkeypatch, tmp_path / "effects", *args, cfd_tables=TABLES, unphased_effects=True, graphical_reports=True)
    assert any(k.startswith("figures") for k in fig)


def test_the_option_says_when_it_is_not_used(tmp_path, monkeypatch):
    fx, reg, fa, bed, vcf = _g4_files(tmp_path, "g4_unphased")
    spy = _Spy(monkeypatch)
    args = (fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"])
    pipeline.search_files(*args, str(tmp_path / "a"), unphased_indel_windows="device")   # the SNV rows are built on the host
    assert any("unphased_indel_windows='device' not used" in m for m in spy.lines) and spy.whole == 1
    spy.lines.clear()
    pipeline.search_files(*args, str(tmp_path / "b"), unphased_haplotypes="device", unphased_indel_windows="device", unphased_report="objects")
    assert any("unphased_indel_windows='device' not used" in m for m in spy.lines)
    monkeypatch.setenv("HAWK_UNPHASED_INDEL_WINDOWS", "device")   # the environment asks where the parameter does not
    with monkeypatch.context() as m:
        calls = uw.spy_on_the_host_window_builder(m)
        pipeline.search_files(*args, str(tmp_path / "c"), unphased_haplotypes="device")
        assert calls["windows"] == 0
        pipeline.search_files(*args, str(tmp_path / "d"), unphased_haplotypes="device", unphased_indel_windows="host")
        assert calls["windows"] == 1
    assert _written(tmp_path / "c") == _written(tmp_path / "d")


# (the host builder accepts an inserted N; the route behind it does not: a KeyError, under either window builder)
WINDOW_DECLINES = {"insertion_longer_than_the_flank": (8, ValueError), "indel_base_outside_acgt": (9, KeyError), "indel_ref_mismatch": (4, ValueError),
                   "indel_bases_in_lower_case": (9, None)}   # (lower case is outside A/C/G/T to the device; the host builder lowers the alt anyway)


@pytest.mark.parametrize("kind", sorted(WINDOW_DECLINES))
def test_a_declined_window_degrades_one_step(tmp_path, monkeypatch, kind):
    """Under unphased_indel_windows="device" an indel the window builder declines sends the interval to the route one step down -
    device SNV rows, host windows - with a level-3 line naming the reason and the variant: the same files as that route writes, or,
    where the host builder raises on the record, the same exception type and text and no file."""
    fx, reg, fa, bed, vcf = _g4_files(tmp_path, "g4_unphased")
    reason, exc = WINDOW_DECLINES[kind]
    p = reg.bed_start + 57   # 1-based position inside the interval
    here = reg.contig_seq[p - 1:p + 2]
    other = "ACGT"[("ACGT".index(here[1]) + 1) % 4]
    ref, alt = {"insertion_longer_than_the_flank": (here[0], here[0] + "ACGTT" * 20 + "A"), "indel_base_outside_acgt": (here[0], here[0] + "NN"),
                "indel_bases_in_lower_case": (here[0], here[0] + "ac"),
                "indel_ref_mismatch": (here[0] + other + here[2], here[0])}[kind]

    def edit(rows):
        new = [reg.contig, str(p), ".", ref, alt, ".", "PASS", "AF=0.25", "GT"] + ["0/1"] + ["0/0"] * (len(reg.samples) - 1)
        return sorted([f for f in rows if int(f[1]) != p] + [new], key=lambda f: int(f[1]))
    vcf2 = _edited_vcf(tmp_path, reg, edit)
    spy = _Spy(monkeypatch)

    def run(windows):
        out = tmp_path / windows
        try:
            pipeline.search_files(fa, bed, [vcf2], fx["pam"], fx["guidelen"], fx["right"], str(out), cfd_tables=TABLES, unphased_haplotypes="device",
                                  unphased_indel_windows=windows)
        except Exception as e:
            return "raised", type(e), str(e), _written(out)
        return "files", None, None, _written(out)
    host = run("host")
    assert not any("indel windows" in m for m in spy.lines)
    spy.lines.clear()
    dev = run("device")
    assert dev == host
    said = [m for m in spy.lines if "Unphased indel windows built on the host" in m]
    assert len(said) == 1 and _lib.UBUILD_REASONS[reason] in said[0] and f"{reg.contig}-{p}-{ref}/{alt}" in said[0]
    if exc is not None:
        assert host[0] == "raised" and issubclass(host[1], exc) and host[3] == {}
    else:
        assert host[0] == "files" and len(host[3]) > 0, host[:3]
