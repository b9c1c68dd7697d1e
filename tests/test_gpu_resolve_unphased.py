"""Unphased IUPAC windows resolved on the device table (hawk_table_resolve_unphased: k_ur_count / k_ur_fill) against the
reference's own g4 lists, the host twin on the same table, and the Python restatement on the seam panel of
tests/resolve_refs.py; launch, scan and batch seams; both table layouts; the declines as the host route's own exceptions."""
import numpy as np
import pytest

import resolve_refs as rr
from crisprhawk_hip import _lib, search_guides as sg
from crisprhawk_hip.hapset import GuideTable
from util import load_golden

pytestmark = pytest.mark.gpu
PANEL = rr.panel()
EMPTY_ALLELES = (np.zeros(0, np.uint64), np.zeros(1, np.uint32), np.zeros(0, np.uint8))


def _listed(guides, haps):
    hidx = {h.id: i for i, h in enumerate(haps)}
    return [[g.start, g.stop, g.strand, g.sequence, hidx[g.hapid], g.right, g.samples] for g in guides]


def _table(s):
    region, haps, pam = s.build()
    tab = sg._device_set(region, haps, len(pam)).search(pam.bits, pam.bitsrc, len(pam), s.guidelen, s.right, download=False)
    return region, haps, pam, tab


def _same_columns(a, b):
    assert np.array_equal(a.n_resolved, b.n_resolved) and np.array_equal(a.n_kept, b.n_kept)
    assert np.array_equal(a.src_row, b.src_row) and np.array_equal(a.win, b.win)


@pytest.mark.parametrize("fixture", rr.G4_FIXTURES)
def test_search_gives_the_references_lists_on_both_engines(fixture, monkeypatch):
    fx = load_golden(f"{fixture}.json.gz")
    region, haps, pam = rr.haplotypes_from_fixture(fx)
    calls = []
    real = GuideTable.resolve_unphased
    monkeypatch.setattr(GuideTable, "resolve_unphased", lambda self, *a, **k: calls.append(a[-1]) or real(self, *a, **k))
    host_route = sg._resolve_unphased
    monkeypatch.setattr(sg, "_resolve_unphased", lambda *a, **k: calls.append("host route") or host_route(*a, **k))
    dev = sg.search(pam, region, haps, None, fx["guidelen"], fx["right"], True, False, 0, True, unphased_engine="device")
    assert calls == ["device"]   # resolved on the device, nothing declined
    assert _listed(dev, haps) == fx["guides"]
    host = sg.search(pam, region, haps, None, fx["guidelen"], fx["right"], True, False, 0, True, unphased_engine="host")
    assert calls == ["device", "host route"]
    assert _listed(host, haps) == fx["guides"]
    monkeypatch.setenv("HAWK_UNPHASED_ENGINE", "host")   # None: the environment decides, else the device
    sg.search(pam, region, haps, None, fx["guidelen"], fx["right"], True, False, 0, True)
    monkeypatch.delenv("HAWK_UNPHASED_ENGINE")
    sg.search(pam, region, haps, None, fx["guidelen"], fx["right"], True, False, 0, True)
    assert calls == ["device", "host route", "host route", "device"]


@pytest.mark.parametrize("name", sorted(PANEL))
def test_panel_device_against_twin_and_restatement(name):
    s = PANEL[name]
    region, haps, pam, tab = _table(s)
    dev = tab.resolve_unphased(haps, pam, "device")
    host = tab.resolve_unphased(haps, pam, "host")
    _same_columns(dev, host)
    tab.download()
    _, _, _, t = s.rows()
    assert tab.n_rows == t.n_rows   # the device table holds the rows the strings give
    assert rr.guides_of(dev, haps, tab, s.right) == rr.expected_guides(haps, t, pam, s.guidelen, s.right)
    if "n_kept" in s.claims:
        assert sorted(dev.n_kept.tolist()) == sorted(s.claims["n_kept"])


@pytest.mark.parametrize("n_rows", [63, 64, 65, 1025])
def test_source_row_counts_around_a_wave_and_past_a_block(n_rows):
    n_guides = (n_rows + 1) // 2
    s = rr.many_rows_scene(n_guides, f"rows_{n_rows}", n_amb=2)
    if n_rows % 2:   # one guide of the copy left as REF's: its row is not in the table
        p = 150 + 50 * (n_guides - 1)
        for q in (p - 1, p - 2):
            del s.haps[0][2][q]
    region, haps, pam, tab = _table(s)
    assert tab.n_rows == n_rows
    dev = tab.resolve_unphased(haps, pam, "device")
    _same_columns(dev, tab.resolve_unphased(haps, pam, "host"))
    tab.download()
    _, _, _, t = s.rows()
    assert rr.guides_of(dev, haps, tab, s.right) == rr.expected_guides(haps, t, pam, s.guidelen, s.right)
    assert int(dev.n_kept.sum()) == n_guides + 3 * (n_rows - n_guides)


def test_one_row_of_1024_kept_guides_spans_fill_blocks():
    s = rr.wide_row_scene(10, "wide_1024", partner=False)
    region, haps, pam, tab = _table(s)
    dev = tab.resolve_unphased(haps, pam, "device")
    assert dev.n_kept.tolist() == [1024] and dev.n_resolved.tolist() == [1024]
    _same_columns(dev, tab.resolve_unphased(haps, pam, "host"))
    seqs = dev.windows()
    assert len(set(seqs)) == 1024
    tab.download()
    _, _, _, t = s.rows()
    assert rr.guides_of(dev, haps, tab, s.right) == rr.expected_guides(haps, t, pam, s.guidelen, s.right)
    # with the partner: the one combination that is REF's core goes, the order of the others stays
    s = rr.wide_row_scene(10, "wide_1023")
    region, haps, pam, tab = _table(s)
    dev2 = tab.resolve_unphased(haps, pam, "device")
    assert sorted(dev2.n_kept.tolist()) == [1, 1023]
    _same_columns(dev2, tab.resolve_unphased(haps, pam, "host"))


def test_more_than_65536_outputs():
    s = rr.many_rows_scene(40, "many_outputs", n_amb=11)
    region, haps, pam, tab = _table(s)
    dev = tab.resolve_unphased(haps, pam, "device")
    assert dev.timing["n_kept"] == len(dev.src_row) == 40 + 40 * 2047 > 65536 and dev.timing["n_resolved"] == 40 + 40 * 2048
    _same_columns(dev, tab.resolve_unphased(haps, pam, "host"))
    seqs = dev.windows()
    assert len(set(zip(dev.src_row.tolist(), seqs))) == len(seqs)


def test_batches_of_whole_rows(monkeypatch):
    """a budget of 10 outputs: REF's one-guide rows go ten to a batch, the copy's three-guide rows three to a batch - a
    multi-output row first and last in every one of those"""
    s = rr.many_rows_scene(12, "batches", n_amb=2)
    region, haps, pam, tab = _table(s)
    whole = tab.resolve_unphased(haps, pam, "device")
    assert whole.timing["n_batches"] == 1 and whole.n_kept.tolist() == [1] * 12 + [3] * 12
    monkeypatch.setenv("HAWK_RESOLVE_BATCH_BYTES", str(44 * 10))
    cut = tab.resolve_unphased(haps, pam, "device")
    assert cut.timing["n_batches"] == 2 + 4
    _same_columns(cut, whole)
    monkeypatch.setenv("HAWK_RESOLVE_BATCH_BYTES", str(44 * 3))   # every batch one three-guide row, or three of REF's
    one = tab.resolve_unphased(haps, pam, "device")
    assert one.timing["n_batches"] == 4 + 12
    _same_columns(one, whole)
    monkeypatch.setenv("HAWK_RESOLVE_BATCH_BYTES", str(44 * 3 - 1))   # a row that does not fit declines
    with pytest.raises(_lib.HawkResolveDeclined) as e:
        tab.resolve_unphased(haps, pam, "device")
    assert (e.value.status, e.value.reason, e.value.row) == (_lib.HAWK_E_CAPACITY, 5, 12)


def _greedy_batches(n_kept, cap):
    """whole rows while they fit, a batch without outputs not counted (hawk_table_resolve_unphased)"""
    n, r0, batches = len(n_kept), 0, 0
    while r0 < n:
        r1, m = r0 + 1, int(n_kept[r0])
        while r1 < n and m + int(n_kept[r1]) <= cap:
            m += int(n_kept[r1]); r1 += 1
        batches += m > 0
        r0 = r1
    return batches


@pytest.mark.parametrize("name", sorted(PANEL))
def test_panel_in_batches(name, monkeypatch):
    """every panel scene under the smallest budget it fits - its largest row alone fills a batch, so rows whose combinations are
    partly dropped against REF start, end and fill batches - equal to the one-batch result"""
    s = PANEL[name]
    region, haps, pam, tab = _table(s)
    whole = tab.resolve_unphased(haps, pam, "device")
    cap = int(whole.n_kept.max())
    monkeypatch.setenv("HAWK_RESOLVE_BATCH_BYTES", str(44 * cap))
    cut = tab.resolve_unphased(haps, pam, "device")
    assert cut.timing["n_batches"] == _greedy_batches(whole.n_kept, cap)
    if name in ("options", "positions", "strands_right", "ref_last"):
        assert cut.timing["n_batches"] >= 3
    _same_columns(cut, whole)


def test_a_refusal_of_the_device_route_takes_the_host_route_too(monkeypatch):
    """any status of the device call but a HIP failure - a geometry the kernels do not take, say - leaves search() where it was
    before the kernels existed: on the host route"""
    fx = load_golden("g4_unphased.json.gz")
    region, haps, pam = rr.haplotypes_from_fixture(fx)

    def refuse(self, *a, **k):
        raise _lib.HawkStatusError(_lib.HAWK_E_INVALID, "hawk_table_resolve_unphased")
    monkeypatch.setattr(GuideTable, "resolve_unphased", refuse)
    got = sg.search(pam, region, haps, None, fx["guidelen"], fx["right"], True, False, 0, True, unphased_engine="device")
    assert _listed(got, haps) == fx["guides"]


def test_packed_rows_of_a_plan_view(monkeypatch):
    """The cluster search's 64-byte rows through the same kernels: a phased table has no ambiguous letter, so every valid row
    resolves to itself - on both layouts of the same region."""
    from crisprhawk_hip import synth
    from crisprhawk_hip.workload import expand_on_device
    from oracle import oracle as ora
    reg = synth.make_region(11, "chrS", 9000, 1000, 8000)
    synth.add_phased_variants(reg, 12, 150, 3, frac_snv=0.7, frac_del=0.15, af_min=0.2, af_max=0.6)
    bits, bitsrc, _, _ = ora.pam_encode("NGG")
    monkeypatch.setenv("HAWK_CLUSTER_MIN_SHARE", "0")
    ds, _info, _ms, _kept = expand_on_device(reg, 3, device=0, keep_plan=True)
    try:
        got = {}
        for layout, target in (("rows", ds.plan.view()), ("columns", ds)):
            tab = target.search(bits, bitsrc, 3, 20, False, download=False)
            assert tab.layout() == layout
            dev = tab.resolve_unphased(EMPTY_ALLELES, (bits, bitsrc), "device")
            _same_columns(dev, tab.resolve_unphased(EMPTY_ALLELES, (bits, bitsrc), "host"))
            tab.download()
            valid = np.where(tab.right_as_stored(), tab.pos.astype(np.int64) + 33 < target.hap_len[tab.hap], tab.pos.astype(np.int64) - 30 >= 0)
            assert np.array_equal(dev.n_resolved, valid.astype(np.uint32)) and np.array_equal(dev.n_kept, dev.n_resolved) and valid.sum() > 100
            assert np.array_equal(dev.src_row, np.flatnonzero(valid)) and np.array_equal(dev.win, tab.win[:, dev.src_row])
            got[layout] = sorted(zip(tab.start[dev.src_row].tolist(), tab.strand[dev.src_row].tolist(), dev.windows()))
        assert got["rows"] == got["columns"]
    finally:
        ds.plan.close()
        ds.close()


def test_declines_reach_python_as_the_host_routes_exception(monkeypatch):
    s, reason, exc = rr.decline_scenes()["no_entry"]
    region, haps, pam, tab = _table(s)
    with pytest.raises(_lib.HawkResolveDeclined) as e:
        tab.resolve_unphased(haps, pam, "device")
    assert (e.value.status, e.value.reason) == (_lib.HAWK_E_UNSUPPORTED, 1)
    tab.download()
    assert "N" in tab.windows()[e.value.row]
    with pytest.raises(exc):   # search() then takes the host route, which raises the reference's KeyError
        sg.search(pam, region, haps, None, s.guidelen, s.right, True, False, 0, True, unphased_engine="device")
    s, reason, _ = rr.decline_scenes()["multi_ref"]
    region, haps, pam, tab = _table(s)
    with pytest.raises(_lib.HawkResolveDeclined) as e:
        tab.resolve_unphased(haps, pam, "device")
    assert (e.value.status, e.value.reason, e.value.row) == (_lib.HAWK_E_UNSUPPORTED, 2, -1)
    calls = []
    host_route = sg._resolve_unphased
    monkeypatch.setattr(sg, "_resolve_unphased", lambda *a, **k: calls.append(1) or host_route(*a, **k))
    from crisprhawk_hip.crisprhawk_error import CrisprHawkCfdScoreError
    for engine in ("host", "device"):   # the reference's "Duplicate REF guide", from the host route either way
        with pytest.raises(CrisprHawkCfdScoreError):
            sg.search(pam, region, haps, None, s.guidelen, s.right, True, False, 0, True, unphased_engine=engine)
    assert len(calls) == 2
    # REF itself with two combinations at one key: declined, and the host route raises the reference's "Duplicate REF guide"
    s, reason, exc = rr.decline_scenes()["ref_ambig"]
    region, haps, pam, tab = _table(s)
    with pytest.raises(_lib.HawkResolveDeclined) as e:
        tab.resolve_unphased(haps, pam, "device")
    assert (e.value.status, e.value.reason, e.value.row) == (_lib.HAWK_E_UNSUPPORTED, 3, 0)
    for engine in ("host", "device"):
        with pytest.raises(exc, match="Duplicate REF guide"):
            sg.search(pam, region, haps, None, s.guidelen, s.right, True, False, 0, True, unphased_engine=engine)
    # a row above 2^32 - 1 combinations (as a status only: the host route would walk 2^33 of them)
    s = rr.wide_row_scene(29, "wide33")
    for p in (200, 205, 207, 209):
        s.haps[0][2][p] = ("w", [(s.ref[p], "T" if s.ref[p] == "A" else "A")])
    region, haps, pam, tab = _table(s)
    with pytest.raises(_lib.HawkResolveDeclined) as e:
        tab.resolve_unphased(haps, pam, "device")
    assert (e.value.status, e.value.reason) == (_lib.HAWK_E_CAPACITY, 4)
