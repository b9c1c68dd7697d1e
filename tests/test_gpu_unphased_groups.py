"""Report groups of an unphased table on the device (hawk_resolve_groups: k_ug_keys, the sort passes, k_ug_heads, k_ug_emit)
against the host twin on the same table - the twin is held to a plain Python restatement in tests/test_ugroups_host.py - at the
launch, scan, sort and fill-batch seams; the statuses; and pipeline.search_files' "groups" route against the object route, byte
for byte, with the model scores the object route never had.  All comparisons are bit-equal."""
import ctypes as C
import io

import numpy as np
import pytest

import resolve_refs as rr
import ugroups_refs as ug
from crisprhawk_hip import _lib, guide as guide_mod, pipeline, readers, reports, scoring, search_guides as sg, synth
from crisprhawk_hip.hapset import GuideTable, _p
from crisprhawk_hip.pam import SPCAS9
from util import load_golden

pytestmark = pytest.mark.gpu
SCENES = ug.scenes(with_region=True)
TABLES = synth.cfd_tables()
_RC = str.maketrans("ACGT", "TGCA")


def _table(region, haps, pam, guidelen, right):
    ds = sg._device_set(region, haps, len(pam))
    return ds, ds.search(pam.bits, pam.bitsrc, len(pam), guidelen, right, download=False)


def _both(tab, haps, pam, tables=None, flank=(0, 0)):
    dev = tab.resolve_unphased_groups(haps, pam, tables, flank, "device")
    host = tab.resolve_unphased_groups(haps, pam, tables, flank, "host")
    assert (dev.engine, host.engine) == ("device", "host") and dev.n_kept == host.n_kept == dev.timing["n_kept"]
    assert (dev.timing["n_groups"], dev.timing["n_members"]) == (dev.n_groups, dev.n_members)
    ug.assert_groups_equal(dev, host)
    return dev


def test_exports_exist():
    L = _lib.lib()
    for name in ("hawk_resolve_groups", "hawk_ugroups_download", "hawk_ugroups_free", "hawk_host_unphased_groups"):
        assert name in _lib.EXPORTS and hasattr(L, name)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_device_equals_twin_on_every_scene(name):
    region, haps, pam, t, guidelen, right = SCENES[name]
    ds, tab = _table(region, haps, pam, guidelen, right)
    assert tab.n_rows == t.n_rows   # the device table holds the rows the strings give
    for flank in ug.FLANKS:
        for tables in (None, TABLES):
            dev = _both(tab, haps, pam, tables, flank)
            assert dev.n_groups > 0
            if tables is None:
                assert np.all(np.isnan(dev.cfdon))
    tab.close()


def _many(n_kept, name):
    """many_rows_scene with n_kept kept guides: one per REF row, one per row of the copy (the other combination is REF's core)"""
    n_guides = (n_kept + 1) // 2
    s = rr.many_rows_scene(n_guides, name, n_amb=1)
    if n_kept % 2:   # one guide of the copy left as REF's: its row is not in the table
        del s.haps[0][2][150 + 50 * (n_guides - 1) - 1]
    return s


@pytest.mark.parametrize("n_kept", [63, 64, 65, 1025])
def test_kept_guide_counts_around_a_wave_and_past_a_block(n_kept):
    s = _many(n_kept, f"kept_{n_kept}")
    region, haps, pam = s.build()
    ds, tab = _table(region, haps, pam, s.guidelen, s.right)
    dev = _both(tab, haps, pam, TABLES, (4, 3))
    assert dev.n_kept == n_kept and dev.n_groups == n_kept and dev.n_members == n_kept
    assert not np.any(np.isnan(dev.cfdon))
    tab.close()


def test_more_than_65536_indices_through_the_sort():
    s = rr.many_rows_scene(40, "many_sorted", n_amb=11)
    region, haps, pam = s.build()
    ds, tab = _table(region, haps, pam, s.guidelen, s.right)
    dev = _both(tab, haps, pam, TABLES)
    assert dev.n_kept == 40 + 40 * 2047 > 65536 and dev.n_groups == dev.n_kept   # every combination a core of its own
    assert np.all(np.diff(np.asarray(dev.start)) >= 0)   # groups ascend by start first
    tab.close()


def test_fill_batches_leave_the_groups_as_they_are(monkeypatch):
    """a budget of 10 kept guides: the fill into device memory runs in many batches, and the two members of every group of the
    copies come from different batches"""
    s = rr.many_rows_scene(12, "group_batches", n_amb=2)
    s.copy("S2", dict(s.haps[0][2]))
    region, haps, pam = s.build()
    ds, tab = _table(region, haps, pam, s.guidelen, s.right)
    whole = _both(tab, haps, pam, TABLES)
    assert whole.timing["n_batches"] == 1 and whole.n_kept == 12 + 2 * 36 and whole.n_groups == 12 + 36 and whole.n_members == 12 + 2 * 36
    off = np.asarray(whole.member_off).astype(np.int64)
    assert sorted(np.diff(off).tolist()) == [1] * 12 + [2] * 36
    monkeypatch.setenv("HAWK_RESOLVE_BATCH_BYTES", str(44 * 10))
    cut = tab.resolve_unphased_groups(haps, pam, TABLES, (0, 0), "device")
    assert cut.timing["n_batches"] >= 9
    ug.assert_groups_equal(cut, whole)
    tab.close()


def _handle(tab, haps, pam):
    key, off, ref = sg.flatten_variant_alleles(haps)
    key = np.ascontiguousarray(key, np.uint64); off = np.ascontiguousarray(off, np.uint32); ref = np.ascontiguousarray(ref, np.uint8)
    al = _lib.ResolveAlleles(len(key), key.ctypes.data, off.ctypes.data, ref.ctypes.data if len(ref) else None)
    h, nk, nr, dec, tm = C.c_void_p(), C.c_uint64(), C.c_uint64(), _lib.ResolveDecline(), _lib.ResolveTiming()
    _lib.check(_lib.lib().hawk_table_resolve_unphased(tab._t, C.byref(al), C.c_uint64(pam.bits), C.c_uint64(pam.bitsrc), C.byref(h), C.byref(nk),
                                                      C.byref(nr), C.byref(dec), C.byref(tm)), "hawk_table_resolve_unphased")
    return h, nk.value, (key, off, ref)


def _groups_call(h, up=0, down=0):
    gh, ng, nm, tm = C.c_void_p(), C.c_uint64(), C.c_uint64(), _lib.UgroupsTiming()
    rc = _lib.lib().hawk_resolve_groups(h, None, None, C.c_uint32(up), C.c_uint32(down), C.byref(gh), C.byref(ng), C.byref(nm), C.byref(tm))
    return rc, gh, ng.value, nm.value


def test_statuses_of_the_handle():
    L = _lib.lib()
    region, haps, pam, t, guidelen, right = SCENES["options"]
    ds, tab = _table(region, haps, pam, guidelen, right)
    h, nk, keep = _handle(tab, haps, pam)
    for up, down in [(11, 0), (0, 11)]:   # refused before the handle is touched
        rc, gh, _, _ = _groups_call(h, up, down)
        assert rc == _lib.HAWK_E_UNSUPPORTED and not gh.value
    rc, gh, ng, nm = _groups_call(h)
    assert rc == _lib.HAWK_OK and gh.value and ng > 0 and nm >= ng
    rc2, gh2, _, _ = _groups_call(h)   # a second call on one handle
    assert rc2 == _lib.HAWK_E_INVALID and not gh2.value
    off = np.zeros(ng + 1, np.uint64)   # any pointer of the download may be NULL
    _lib.check(L.hawk_ugroups_download(gh, *([None] * 11), _p(off), None), "hawk_ugroups_download")
    assert off[0] == 0 and off[-1] == nm
    L.hawk_ugroups_free(gh)
    L.hawk_resolve_free(h)
    h, nk, keep = _handle(tab, haps, pam)   # downloaded already
    src, win = np.zeros(nk, np.uint32), np.zeros((5, nk), np.uint64)
    _lib.check(L.hawk_resolve_download(h, _p(src), _p(win), None, None, None), "hawk_resolve_download")
    rc, gh, _, _ = _groups_call(h)
    assert rc == _lib.HAWK_E_INVALID and not gh.value
    L.hawk_resolve_free(h)
    h, nk, keep = _handle(tab, haps, pam)   # stale: a later search on the set has overwritten the rows
    tab.close()
    tab2 = ds.search(pam.bits, pam.bitsrc, len(pam), guidelen, right, download=False)
    rc, gh, _, _ = _groups_call(h)
    assert rc == _lib.HAWK_E_INVALID and not gh.value
    L.hawk_resolve_free(h)
    with pytest.raises(_lib.HawkStatusError) as e:
        tab2.resolve_unphased_groups(haps, pam, None, (11, 0))
    assert e.value.status == _lib.HAWK_E_UNSUPPORTED
    tab2.close()


def test_zero_kept_guides_give_a_valid_empty_result():
    """REF alone, its one row not valid (the window ends with the haplotype): a table of one row that keeps nothing"""
    region, haps, pam, t, guidelen, right = SCENES["short_ref"]
    ds, tab = _table(region, haps[:1], pam, guidelen, right)
    assert tab.n_rows == 1
    dev = _both(tab, haps[:1], pam, TABLES, (4, 3))
    assert (dev.n_kept, dev.n_groups, dev.n_members) == (0, 0, 0) and dev.member_off.tolist() == [0] and dev.windows() == []
    tab.close()


def test_three_forms_of_cfdon_agree():
    """the HAWK_HD restatement in k_ug_keys and in the twin, and k_cfd (scoring.compute_cfd_batch) on the decoded strings: the
    same fp64 product; the search kernels' cfdon_from_slices is held to k_cfd by the parity tests of the search"""
    scoring.set_cfd_tables(*TABLES)
    checked = 0
    for name in sorted(SCENES):
        region, haps, pam, t, guidelen, right = SCENES[name]
        if guidelen != 20 or right:
            continue
        ds, tab = _table(region, haps, pam, guidelen, right)
        dev = _both(tab, haps, pam, TABLES)
        tab.close()
        wins = dev.windows()

        def guide(i):
            core = wins[i][10:-10].upper()
            return core[::-1].translate(_RC) if dev.strand[i] else core
        refs = {(int(dev.start[i]), int(dev.strand[i])): guide(i) for i in range(dev.n_groups) if dev.is_ref[i]}
        rows = [i for i in range(dev.n_groups) if (int(dev.start[i]), int(dev.strand[i])) in refs]
        assert np.array_equal(~np.isnan(dev.cfdon), np.isin(np.arange(dev.n_groups), rows))
        if not rows:
            continue
        gs = [guide(i) for i in rows]
        want = scoring.compute_cfd_batch([refs[(int(dev.start[i]), int(dev.strand[i]))][:20] for i in rows], [g[:20] for g in gs], [g[-2:] for g in gs], True)
        assert np.asarray(dev.cfdon)[rows].tobytes() == np.asarray(want, np.float64).tobytes()
        checked += len(rows)
    assert checked > 1000


# ---------------------------------------------------------------------------- files to TSV
def _g4_files(tmp_path, fixture):
    from test_host_objects import _unphased_inputs
    fx = load_golden(f"{fixture}.json.gz")
    reg, _, _ = _unphased_inputs(fx)
    fa, bed, vcf = str(tmp_path / "g.fa"), str(tmp_path / "r.bed"), str(tmp_path / "v.vcf")
    readers.write_fasta(fa, reg.contig, reg.contig_seq, 80)
    with open(bed, "w") as f:
        f.write(f"{reg.contig}\t{reg.bed_start}\t{reg.bed_stop}\n")
    rows = []
    for v in reg.variants:
        fields = reg.vcf_fields(v)
        fields[9:] = [g.replace("|", "/") for g in fields[9:]]
        rows.append(fields)
    readers.write_vcf(vcf, reg.contig, reg.samples, rows, False)
    return fx, reg, fa, bed, vcf


def _g7_files(tmp_path):
    fx = load_golden("g7_report_unphased.json.gz")
    contig_seq = "N" * (fx["startp"] - 1) + fx["region_seq"] + "ACGT" * 10
    fa, bed, vcf = str(tmp_path / "g.fa"), str(tmp_path / "r.bed"), str(tmp_path / "v.vcf")
    readers.write_fasta(fa, fx["contig"], contig_seq, 80)
    with open(bed, "w") as f:
        f.write(f"{fx['contig']}\t{fx['bed_start']}\t{fx['bed_stop']}\n")
    rows = [[fx["contig"], str(p), ".", r, a, ".", "PASS", f"AF={af:.6g}", "GT"] + [f"{g[0]}/{g[1]}" for g in gts] for p, r, a, af, gts in fx["variants"]]
    readers.write_vcf(vcf, fx["contig"], fx["samples"], rows, False)
    return fx, fa, bed, vcf


class _Spy:
    """what the route did: calls of resolve_unphased_groups (and what they returned), of _guides_from_resolved, Guide objects built"""

    def __init__(self, monkeypatch, fail=None):
        self.groups, self.from_resolved, self.guides = [], 0, 0
        real_groups, real_from, real_init = GuideTable.resolve_unphased_groups, sg._guides_from_resolved, guide_mod.Guide.__init__

        def groups(tab, *a, **k):
            if fail is not None:
                self.groups.append(None)
                raise fail
            self.groups.append(real_groups(tab, *a, **k))
            return self.groups[-1]

        def from_resolved(*a, **k):
            self.from_resolved += 1
            return real_from(*a, **k)

        def init(obj, *a, **k):
            self.guides += 1
            real_init(obj, *a, **k)
        monkeypatch.setattr(GuideTable, "resolve_unphased_groups", groups)
        monkeypatch.setattr(sg, "_guides_from_resolved", from_resolved)
        monkeypatch.setattr(guide_mod.Guide, "__init__", init)

    def took_the_device_route(self, n=1):
        return len(self.groups) == n and all(g is not None for g in self.groups) and self.from_resolved == 0 and self.guides == 0

    def reset(self):
        self.groups, self.from_resolved, self.guides = [], 0, 0


def _two_routes(spy, tmp_path, fa, bed, vcf, pam, guidelen, right, **kw):
    """-> (bytes of the "groups" report, bytes of the "objects" report), the routes asserted"""
    spy.reset()
    (a,) = pipeline.search_files(fa, bed, [vcf], pam, guidelen, right, str(tmp_path / "groups"), unphased_report="groups", **kw).values()
    assert spy.took_the_device_route()
    spy.reset()
    (b,) = pipeline.search_files(fa, bed, [vcf], pam, guidelen, right, str(tmp_path / "objects"), unphased_report="objects", **kw).values()
    assert spy.groups == [] and spy.from_resolved == 1 and spy.guides > 0
    return open(a, "rb").read(), open(b, "rb").read()


@pytest.mark.parametrize("fixture", rr.G4_FIXTURES)
def test_groups_and_objects_write_the_same_report(tmp_path, monkeypatch, fixture):
    fx, reg, fa, bed, vcf = _g4_files(tmp_path, fixture)
    spy = _Spy(monkeypatch)
    plain = _two_routes(spy, tmp_path / "plain", fa, bed, vcf, fx["pam"], fx["guidelen"], fx["right"])
    assert plain[0] == plain[1] and plain[0].count(b"\n") > 1
    cfd = _two_routes(spy, tmp_path / "cfd", fa, bed, vcf, fx["pam"], fx["guidelen"], fx["right"], cfd_tables=TABLES)
    assert cfd[0] == cfd[1]
    ann = str(tmp_path / "features.bed")
    span = reg.bed_stop - reg.bed_start
    with open(ann, "w") as f:
        for k, (a, b) in enumerate([(0, span // 3), (span // 4, span // 2), (span // 2 + 7, span // 2 + 40), (span - 50, span)]):
            f.write(f"{reg.contig}\t{reg.bed_start + a}\t{reg.bed_start + b}\tfeature{k}\n")
    both = _two_routes(spy, tmp_path / "ann", fa, bed, vcf, fx["pam"], fx["guidelen"], fx["right"], cfd_tables=TABLES, annotations=[ann])
    assert both[0] == both[1] and b"feature1" in both[0]


def test_g7_groups_report_matches_the_reference_tsv(tmp_path, monkeypatch):
    import pandas as pd
    fx, fa, bed, vcf = _g7_files(tmp_path)
    spy = _Spy(monkeypatch)
    a, b = _two_routes(spy, tmp_path, fa, bed, vcf, fx["pam"], fx["guidelen"], fx["right"], cfd_tables=TABLES)
    assert a == b
    got = pd.read_csv(io.BytesIO(a), sep="\t", dtype=str, keep_default_na=False)
    want = pd.read_csv(io.StringIO(fx["report_tsv"]), sep="\t", dtype=str, keep_default_na=False)
    assert list(got.columns) == list(want.columns) and len(got) == len(want)
    for c in got.columns:
        if c != "haplotype_id":
            assert (got[c] == want[c]).all(), (c, got[c][got[c] != want[c]].head(), want[c][got[c] != want[c]].head())
    assert (got["haplotype_id"].str.count(",") == want["haplotype_id"].str.count(",")).all()


def test_default_is_the_groups_route_and_the_environment_can_change_it(tmp_path, monkeypatch):
    fx, reg, fa, bed, vcf = _g4_files(tmp_path, "g4_unphased")
    spy = _Spy(monkeypatch)
    pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "a"))
    assert spy.took_the_device_route()
    spy.reset()
    monkeypatch.setenv("HAWK_UNPHASED_REPORT", "objects")
    pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "b"))
    assert spy.groups == [] and spy.guides > 0
    monkeypatch.delenv("HAWK_UNPHASED_REPORT")
    spy.reset()
    pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "c"), unphased_report="groups", unphased_engine="host")
    assert spy.groups == [] and spy.guides > 0   # the host engine implies the object route
    with pytest.raises(ValueError, match="unphased_report"):
        pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "d"), unphased_report="frames")
    with pytest.raises(ValueError, match="graphical_reports"):
        pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "e"), unphased_report="groups", graphical_reports=True)


def test_forced_fallback_writes_the_object_routes_file(tmp_path, monkeypatch):
    fx, reg, fa, bed, vcf = _g4_files(tmp_path, "g4_unphased")
    (want,) = pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "objects"), cfd_tables=TABLES,
                                    unphased_report="objects").values()
    spy = _Spy(monkeypatch, fail=_lib.HawkStatusError(_lib.HAWK_E_UNSUPPORTED, "hawk_resolve_groups"))
    (got,) = pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "groups"), cfd_tables=TABLES,
                                   unphased_report="groups").values()
    assert spy.groups == [None] and spy.from_resolved == 1 and spy.guides > 0
    assert open(got, "rb").read() == open(want, "rb").read()


def test_unphased_cpf1_report_carries_deepcpf1_scores(tmp_path, monkeypatch):
    """the object route never received the weights: its column said NA.  Every field is str(round(score, 4)) of scoring.deepcpf1
    on the row's 34-mer."""
    import pandas as pd
    fx, reg, fa, bed, vcf = _g4_files(tmp_path, "g4_unphased_cpf1")
    spy = _Spy(monkeypatch)
    (path,) = pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "out"),
                                    deepcpf1_weights=synth.deepcpf1_weights(), unphased_report="groups").values()
    assert spy.took_the_device_route()
    got = pd.read_csv(path, sep="\t", dtype=str, keep_default_na=False)
    assert len(got) > 0 and (got["score_deepcpf1"] != "NA").all() and np.isfinite(got["score_deepcpf1"].astype(float)).all()
    groups = spy.groups[0]
    kmers = reports.group_kmers(groups)
    assert all(len(k) == 34 for k in kmers) and len(kmers) == len(got)
    scores = scoring.deepcpf1(kmers, True)
    want = sorted((int(s), "-" if st else "+", str(round(float(x), 4))) for s, st, x in zip(groups.start, groups.strand, scores))
    assert sorted(zip(got["start"].astype(int), got["strand"], got["score_deepcpf1"])) == want


def test_unphased_ngg_report_carries_plmcrispr_scores(tmp_path, monkeypatch):
    import pandas as pd
    g15 = load_golden("g15_plmcrispr.json.gz")
    model = (synth.plmcrispr_weights(g15["seed"]), {SPCAS9: synth.plmcrispr_protein(g15["seed"], g15["L"])})
    fx, reg, fa, bed, vcf = _g4_files(tmp_path, "g4_unphased")
    assert fx["guidelen"] + len(fx["pam"]) == 23
    spy = _Spy(monkeypatch)
    (path,) = pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "out"), cfd_tables=TABLES,
                                    plmcrispr_model=model, unphased_report="groups").values()
    assert spy.took_the_device_route()
    got = pd.read_csv(path, sep="\t", dtype=str, keep_default_na=False)
    assert len(got) > 0 and (got["score_plmcrispr"] != "NA").all()
    want = scoring.plmcrispr([(s + p).upper() for s, p in zip(got["sgRNA_sequence"], got["pam"])], SPCAS9)
    assert got["score_plmcrispr"].tolist() == [str(round(x, 4)) for x in want]
