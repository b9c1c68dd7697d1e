"""The off-target summary with DNA / RNA bulges (hawk_offtarget_bulge_summary -> GenomeIndex.summary(bdna=, brna=) ->
offtargets.specificity_by_spacer -> pipeline.search_files(offtargets_summary=True)) against the table route it stands in for.
The reference is always GenomeIndex.offtarget_arrays - the listed rows of hawk_offtarget_scan / hawk_offtarget_bulges - with the
cfd_e4 of rows_text (hawk_offtarget_text), both pinned by their own tests: bincount over (guide, kind, size, mm) and per-guide
integer sums must equal hist, bulge_hist, cfd_e4, n_hits and n_unscorable exactly."""
import ctypes as C

import numpy as np
import pytest

import bulge_refs as B
from crisprhawk_hip import _lib, scoring, synth
from crisprhawk_hip.crisprhawk_error import CrisprHawkCfdScoreError
from crisprhawk_hip.genome import GenomeIndex, encode_guides
from crisprhawk_hip.hapset import _p
from test_gpu_offtarget_summary import _pam, _planted_case

pytestmark = pytest.mark.gpu

KINDS = ((True, 1), (True, 2), (False, 1), (False, 2))  # the order of bulge_hist


def _reference(idx, guides, pam, right, max_mm, bdna, brna, tables):
    """what the listed rows give: dict(hist, bulge_hist, cfd_e4, n_hits, n_unscorable)"""
    n, stride = len(guides), max_mm + 1
    arr = idx.offtarget_arrays(guides, pam, right, max_mm, bdna, brna)
    g, mm, kind, size = (arr[k].astype(np.int64) for k in ("guide", "mm", "kind", "size"))
    x = kind == 0
    hist = np.bincount(g[x] * stride + mm[x], minlength=n * stride).reshape(n, stride)
    k = (kind[~x] - 1) * 2 + size[~x] - 1
    bh = np.bincount((g[~x] * 4 + k) * stride + mm[~x], minlength=n * 4 * stride).reshape(n, 4, stride)
    cfd, n_uns, cfd_b, n_uns_b = None, 0, None, 0
    if tables is not None:
        _text, units, n_uns = idx.rows_text(arr, guides, pam, right, None, tables)
        units = np.asarray(units)
        cfd, cfd_b = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        np.add.at(cfd, g[units >= 0], units[units >= 0])
        np.add.at(cfd_b, g[(units >= 0) & ~x], units[(units >= 0) & ~x])
        assert int((units < 0).sum()) == n_uns
        n_uns_b = int(((units < 0) & ~x).sum())
    return dict(hist=hist, bulge_hist=bh, cfd_e4=cfd, n_hits=len(g), n_unscorable=n_uns, bulged_cfd_e4=cfd_b, bulged_unscorable=n_uns_b)


def _assert_equal(got, want):
    assert got["hist"].dtype == np.uint32 and got["bulge_hist"].dtype == np.uint32
    assert np.array_equal(got["hist"], want["hist"])
    assert np.array_equal(got["bulge_hist"], want["bulge_hist"])
    if want["cfd_e4"] is None:
        assert got["cfd_e4"] is None
    else:
        assert got["cfd_e4"].dtype == np.int64 and np.array_equal(got["cfd_e4"], want["cfd_e4"])
    assert (got["n_hits"], got["n_unscorable"]) == (want["n_hits"], want["n_unscorable"])


def _check(idx, guides, pam, right, max_mm, bdna, brna, tables):
    """With the PAM in front (`right`) and tables - a combination the product never makes: only SpCas9-class PAMs, which stand
    behind, get tables - the CFD of the UN-bulged rows is not compared: hawk_offtarget_summary keys the PAM table by PAM[-2:], the
    table's row by the last two characters of its spacer field, and the two are the same characters only with the PAM behind.
    The bulged rows' sums (the summary with bulges less the summary without) must still equal the table's bulged rows'."""
    want = _reference(idx, guides, pam, right, max_mm, bdna, brna, tables)
    got = idx.summary(guides, pam, right, max_mm, cfd_tables=tables, bdna=bdna, brna=brna)
    if right and tables is not None:
        flat = idx.summary(guides, pam, right, max_mm, cfd_tables=tables)
        assert np.array_equal(got["cfd_e4"] - flat["cfd_e4"], want["bulged_cfd_e4"])
        assert got["n_unscorable"] - flat["n_unscorable"] == want["bulged_unscorable"]
        want = dict(want, cfd_e4=got["cfd_e4"], n_unscorable=got["n_unscorable"])
    _assert_equal(got, want)
    asked = [(dna, b) for dna, b in KINDS if b <= (bdna if dna else brna)]
    assert [(t["bulge_type"] == "DNA", t["bulge_size"]) for t in idx.last_bulge_timing] == asked
    for k, kb in enumerate(KINDS):
        if kb not in asked:
            assert not got["bulge_hist"][:, k].any()
    assert idx._meta_guidelen == idx.guidelen  # the index's own window is back
    return got, want


def _plant_bulged(rng, contigs, guides, pam_s, right, per_kind):
    """bulged near-copies of the first guides, every type and size, both strands, written over the contigs' first one; a few with an
    ambiguous base inside the spacer"""
    name = next(iter(contigs))
    g = list(contigs[name])
    pos = 500
    for kind, b in (("DNA", 1), ("DNA", 2), ("RNA", 1), ("RNA", 2)):
        for k in range(per_kind):
            sp = list(B.mutate(rng, guides[k % 6], kind, b, int(rng.integers(0, 5))))
            if k % 7 == 3:
                sp[int(rng.integers(0, len(sp)))] = "N" if k % 2 else "R"
            B.place(g, pos, "".join(sp), B.CONCRETE[pam_s], right, bool(rng.random() < 0.5))
            pos += 97
    return dict(contigs, **{name: "".join(g)})


_SWEEP = {}


def _sweep_case(pam_s, G, right):
    """(contigs, guides) of a geometry, made once: host data only - every test builds and closes its own index"""
    if (pam_s, G) not in _SWEEP:
        contigs, guides = _planted_case(pam_s, G, right, 4, 70)
        _SWEEP[(pam_s, G)] = (_plant_bulged(np.random.default_rng(5), contigs, guides, pam_s, right, 40), guides)
    return _SWEEP[(pam_s, G)]


@pytest.mark.parametrize("bdna,brna", [(1, 0), (0, 1), (2, 2)])
@pytest.mark.parametrize("max_mm", [0, 2, 4])
@pytest.mark.parametrize("pam_s,G,right", [("NGG", 20, False), ("TTTV", 23, True)])
def test_summary_equals_the_table_route(pam_s, G, right, max_mm, bdna, brna):
    contigs, guides = _sweep_case(pam_s, G, right)
    idx = GenomeIndex(contigs, G, len(pam_s), max_bulge=2)
    pam = _pam(pam_s, right)
    tables = synth.cfd_tables()
    got, want = _check(idx, guides, pam, right, max_mm, bdna, brna, tables)
    assert int(want["bulge_hist"].sum()) >= 3
    if max_mm >= 2:
        assert want["n_unscorable"] >= 1 and int(want["bulged_cfd_e4"].sum()) > 0
    # counts only: the same histograms, no CFD
    plain = idx.summary(guides, pam, right, max_mm, bdna=bdna, brna=brna)
    assert plain["cfd_e4"] is None and plain["n_unscorable"] == 0
    assert np.array_equal(plain["hist"], want["hist"]) and np.array_equal(plain["bulge_hist"], want["bulge_hist"])
    # without bulges the dict is the mismatch-only one, key for key
    flat = idx.summary(guides, pam, right, max_mm, cfd_tables=tables)
    assert sorted(flat) == ["cfd_e4", "hist", "n_hits", "n_unscorable"] and np.array_equal(flat["hist"], want["hist"])
    idx.ds.close()


def test_wave_queue_and_chunk_seam():
    guides, contigs, _fa, _fb = B.dense_panel()
    B.assert_queue_is_exercised(B.queue_figures(contigs, guides, "NGG", False, 2, 2, 2))  # on the host's arithmetic, before any device call
    idx = GenomeIndex(contigs, 20, 3, max_bulge=2)
    got, want = _check(idx, guides, _pam("NGG", False), False, 2, 2, 2, synth.cfd_tables())
    assert int(want["bulge_hist"].sum()) > 1000
    for a, b in ((1023, 1024), (0, 1099)):  # one guide on either side of the chunk seam; duplicates far apart
        assert np.array_equal(got["bulge_hist"][a], got["bulge_hist"][b]) and got["bulge_hist"][a].any()
        assert got["cfd_e4"][a] == got["cfd_e4"][b] and np.array_equal(got["hist"][a], got["hist"][b])


def test_every_pair_is_a_row():
    guides, contigs = B.every_pair_panel()
    idx = GenomeIndex(contigs, 20, 3, max_bulge=2)
    got, want = _check(idx, guides, _pam("NGG", False), False, 20, 2, 2, synth.cfd_tables())
    for k, (dna, b) in enumerate(KINDS):  # no pair is pruned: every (site, guide) of every kind that has a placement
        n_sites = idx.last_bulge_timing[k]["n_sites"]
        assert n_sites > 80 and int(got["bulge_hist"][:, k].sum()) >= (n_sites - 6) * len(guides)
    assert want["n_unscorable"] > 0


def _small_genome(rng, guides, n=20_000):
    g = list(synth.random_sequence(rng, n, iupac_frac=0.001))
    pos = 300
    for k in range(60):
        kind, b = (("DNA", 1), ("RNA", 1), ("DNA", 2), ("RNA", 2))[k % 4]
        B.place(g, pos, B.mutate(rng, guides[k % len(guides)], kind, b, k % 4), "TGG", False, bool(k & 4))
        pos += 211
    return {"s": "".join(g)}


@pytest.mark.parametrize("n_guides", [1, 63, 64, 1024, 1025])
def test_guide_counts(n_guides):
    rng = np.random.default_rng(40 + n_guides)
    guides = [synth.random_sequence(rng, 20) for _ in range(n_guides)]
    idx = GenomeIndex(_small_genome(rng, guides), 20, 3, max_bulge=1)
    _got, want = _check(idx, guides, _pam("NGG", False), False, 3, 1, 1, synth.cfd_tables())
    assert int(want["bulge_hist"].sum()) >= 20


@pytest.mark.parametrize("n_sites", [1, 257])
def test_site_counts(n_sites):
    """a genome of A / T with exactly n_sites PAMs, each behind a bulged copy of a guide that no edit can turn into a PAM"""
    guide = "ATCAATCTTACAATCTAACT"  # no G, no two C within three bases: a deletion or an A / T edit makes neither GG nor CC
    rng = np.random.default_rng(n_sites)
    fill = lambda k: "".join("AT"[int(c)] for c in rng.integers(0, 2, size=k))
    parts = [fill(40)]
    for u in range(n_sites):
        sp = list(guide)
        if u % 3 == 1:
            sp[int(rng.integers(0, 20))] = "AT"[u % 2]
        if u % 2:
            sp.insert(int(rng.integers(1, 20)), "A")
        else:
            del sp[int(rng.integers(1, 19))]
        parts += ["".join(sp), "TGG", fill(17 + u % 5)]
    idx = GenomeIndex({"a": "".join(parts)}, 20, 3, max_bulge=1)
    guides = [guide, guide[:9] + "T" + guide[10:], synth.random_sequence(rng, 20)]
    got, want = _check(idx, guides, _pam("NGG", False), False, 2, 1, 1, synth.cfd_tables())
    assert [t["n_sites"] for t in idx.last_bulge_timing] == [n_sites, n_sites]
    assert int(got["bulge_hist"][0].sum()) >= n_sites


@pytest.mark.parametrize("G,bdna,brna", [(27, 2, 0), (29, 0, 2), (29, 0, 1)])
def test_windows_of_32_bases(G, bdna, brna):
    rng = np.random.default_rng(G)
    guides = [synth.random_sequence(rng, G) for _ in range(9)]
    g = list(synth.random_sequence(rng, 12_000, iupac_frac=0.001))
    for k in range(40):
        kind, b = ("DNA", 2 - k % 2) if bdna else ("RNA", 1 + k % 2)
        B.place(g, 200 + 250 * k, B.mutate(rng, guides[k % 9], kind, b, k % 4), "TGG", False, bool(k & 2))
    idx = GenomeIndex({"w": "".join(g)}, G, 3, max_bulge=bdna)
    _got, want = _check(idx, guides, _pam("NGG", False), False, 3, bdna, brna, synth.cfd_tables())
    assert int(want["bulge_hist"].sum()) >= 20


@pytest.mark.parametrize("G,b", [(4, 1), (5, 2)])
def test_shortest_guides(G, b):
    rng = np.random.default_rng(G)
    guides = [synth.random_sequence(rng, G) for _ in range(5)]
    idx = GenomeIndex({"s": synth.random_sequence(rng, 3000, iupac_frac=0.002)}, G, 3, max_bulge=b)
    _got, want = _check(idx, guides, _pam("NGG", False), False, 1, b, b, synth.cfd_tables())
    assert all(want["bulge_hist"][:, k].any() for k, kb in enumerate(KINDS) if kb[1] <= b)


def test_defined_zeros():
    rng = np.random.default_rng(9)
    seq = synth.random_sequence(rng, 5000)
    guides = [seq[100:120], seq[300:320]]
    pam, tables = _pam("NGG", False), synth.cfd_tables()
    idx = GenomeIndex({"a": seq}, 20, 3, max_bulge=2)
    z = idx.summary([], pam, False, 2, cfd_tables=tables, bdna=2, brna=2)
    assert z["hist"].shape == (0, 3) and z["bulge_hist"].shape == (0, 4, 3) and z["cfd_e4"].shape == (0,) and z["n_hits"] == 0
    bare = GenomeIndex({"b": "ACT" * 400}, 20, 3, max_bulge=2)
    z = bare.summary(guides, pam, False, 2, cfd_tables=tables, bdna=2, brna=2)
    assert not z["hist"].any() and not z["bulge_hist"].any() and not z["cfd_e4"].any() and (z["n_hits"], z["n_unscorable"]) == (0, 0)
    assert [t["n_sites"] for t in bare.last_bulge_timing] == [0, 0, 0, 0]
    empty = GenomeIndex({"a": seq}, 20, 3, shard=(1, 2), max_bulge=2)
    assert empty.ds is None
    z = empty.summary(guides, pam, False, 2, cfd_tables=tables, bdna=1, brna=2)
    assert not z["bulge_hist"].any() and z["bulge_hist"].shape == (2, 4, 3) and z["cfd_e4"].tolist() == [0, 0] and z["n_hits"] == 0
    with pytest.raises(ValueError, match="max_bulge"):
        GenomeIndex({"a": seq}, 20, 3, max_bulge=1).summary(guides, pam, False, 2, bdna=2)
    for kw in (dict(bdna=3), dict(brna=-1)):
        with pytest.raises(ValueError, match="bulges of 0..2"):
            idx.summary(guides, pam, False, 2, **kw)


def test_shards_add_up():
    rng = np.random.default_rng(78)
    contigs = {f"c{i}": synth.random_sequence(rng, 60_000 + 7000 * i, iupac_frac=0.0005) for i in range(4)}
    guides = [seq[p:p + 20] for seq in contigs.values() for p in range(100, 50_000, 2500)]
    guides = [g for g in guides if set(g) <= set("ACGT")]
    for name in contigs:  # bulged copies of the guides in every contig
        g = list(contigs[name])
        for k in range(40):
            kind, b = (("DNA", 1), ("RNA", 1), ("DNA", 2), ("RNA", 2))[k % 4]
            B.place(g, 1000 + 1400 * k, B.mutate(rng, guides[k % len(guides)], kind, b, k % 3), "TGG", False, bool(k & 4))
        contigs[name] = "".join(g)
    pam, tables = _pam("NGG", False), synth.cfd_tables()
    whole = GenomeIndex(contigs, 20, 3, piece=20_000, max_bulge=2).summary(guides, pam, False, 3, cfd_tables=tables, bdna=2, brna=2)
    assert int(whole["bulge_hist"].sum()) >= 100 and whole["cfd_e4"].sum() > 0
    for world in (2, 3):
        parts = [GenomeIndex(contigs, 20, 3, piece=20_000, shard=(r, world), max_bulge=2).summary(guides, pam, False, 3, cfd_tables=tables, bdna=2, brna=2)
                 for r in range(world)]
        assert all(p["bulge_hist"].any() for p in parts)
        for key in ("hist", "bulge_hist", "cfd_e4"):
            assert np.array_equal(sum(p[key].astype(np.int64) for p in parts), whole[key]), key
        assert sum(p["n_hits"] for p in parts) == whole["n_hits"] and sum(p["n_unscorable"] for p in parts) == whole["n_unscorable"]


def test_more_rows_than_a_hit_list_holds():
    """A tandem of 2.66 x 10^5 RNA-1 near-copies of one guide, each followed by TGG, against four guides of its family: more than
    2^20 rows of one (type, size) in one call, no capacity and no retry.  (3 x 10^5 units made the reference - the listed rows,
    which need a retry, and their text - the slow part; 2.66 x 10^5 is the smallest round count whose rows still pass 2^20.)"""
    rng = np.random.default_rng(2025)
    base = B.family_base(rng)
    guides = [base] + [B.mutate(rng, base, "", 0, 1) for _ in range(3)]
    n = 266_000
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    units = np.tile(np.frombuffer(base.encode(), dtype=np.uint8), (n, 1))
    sub = rng.random(n) < 0.5
    col = rng.integers(0, 20, size=n)
    cur = units[np.arange(n), col]
    units[np.arange(n), col] = np.where(sub, letters[(np.searchsorted(letters, cur) + rng.integers(1, 4, size=n)) % 4], cur)
    keep = np.ones((n, 20), dtype=bool)
    keep[np.arange(n), rng.integers(1, 19, size=n)] = False
    units = np.concatenate([units[keep].reshape(n, 19), np.tile(np.frombuffer(b"TGG", dtype=np.uint8), (n, 1))], axis=1)
    genome = "ATTATA" + units.tobytes().decode() + "ATATTA"
    pam, tables = _pam("NGG", False), synth.cfd_tables()
    idx = GenomeIndex({"t": genome}, 20, 3)
    got = idx.summary(guides, pam, False, 3, cfd_tables=tables, brna=1)
    h, _tm = idx.bulge_arrays(guides, pam, False, 3, 1, False)  # the list: its first call runs out of capacity and is repeated
    idx._set_window(20)
    rows = len(h["guide"])
    assert rows > 1 << 20
    want = np.bincount(h["guide"].astype(np.int64) * 4 + h["mm"], minlength=16).reshape(4, 4)
    assert np.array_equal(got["bulge_hist"][:, 2], want) and not got["bulge_hist"][:, [0, 1, 3]].any()
    flat = idx.summary(guides, pam, False, 3, cfd_tables=tables)
    assert got["n_hits"] == rows + flat["n_hits"]
    arr = dict(h, kind=np.full(rows, 2, np.uint8), size=np.full(rows, 1, np.uint8))
    _text, units_e4, n_uns = idx.rows_text(arr, guides, pam, False, None, tables)
    units_e4 = np.asarray(units_e4)
    cfd = np.zeros(4, dtype=np.int64)
    np.add.at(cfd, h["guide"][units_e4 >= 0].astype(np.int64), units_e4[units_e4 >= 0])
    assert np.array_equal(got["cfd_e4"] - flat["cfd_e4"], cfd) and (cfd > 0).all()
    assert got["n_unscorable"] - flat["n_unscorable"] == n_uns


def test_abi_refusals_leave_the_outputs_untouched():
    L = _lib.lib()
    rng = np.random.default_rng(9)
    seq = synth.random_sequence(rng, 5000)
    pam = _pam("NGG", False)
    tables = synth.cfd_tables()
    mm = np.ascontiguousarray(tables[0], dtype=np.float64).reshape(20, 4, 4)
    pt = np.ascontiguousarray(tables[1], dtype=np.float64).reshape(16)
    idx = GenomeIndex({"a": seq}, 20, 3, max_bulge=2)

    def raw(handle, G, guides, btype=1, bsize=1, pamlen=3, max_mm=2, tab=(mm, pt)):
        g2 = encode_guides(guides) if guides else np.zeros(0, np.uint64)
        par = _lib.OtParams(pam.bits, pam.bitsrc, pamlen, G, 0, max_mm)
        hist = np.full((max(len(guides), 1), max_mm + 1), 0xABCD, np.uint32)
        cfd = np.full(max(len(guides), 1), -7, np.int64)
        nh, nu = C.c_uint64(7), C.c_uint64(7)
        rc = L.hawk_offtarget_bulge_summary(handle, C.byref(par), _p(g2), len(g2), btype, bsize, None if tab[0] is None else _p(tab[0]),
                                            None if tab[1] is None else _p(tab[1]), _p(hist), _p(cfd), C.byref(nh), C.byref(nu), None)
        if rc != _lib.HAWK_OK:
            assert (hist == 0xABCD).all() and (cfd == -7).all() and (nh.value, nu.value) == (7, 7)
        return rc, nh.value

    guides = [seq[100:120], seq[300:320]]
    idx._set_window(21)
    assert raw(idx.ds._h, 20, guides)[0] == _lib.HAWK_OK
    for btype, bsize in ((0, 1), (3, 1), (1, 0), (1, 3)):
        assert raw(idx.ds._h, 20, guides, btype, bsize)[0] == _lib.HAWK_E_INVALID
    assert raw(idx.ds._h, 20, guides, tab=(mm, None))[0] == _lib.HAWK_E_INVALID          # one table without the other
    assert raw(idx.ds._h, 20, guides, pamlen=1)[0] == _lib.HAWK_E_UNSUPPORTED           # the PAM table is keyed by PAM[-2:]
    assert raw(idx.ds._h, 20, guides, max_mm=33)[0] == _lib.HAWK_E_UNSUPPORTED
    assert raw(idx.ds._h, 4, ["ACGT"], 1, 2)[0] == _lib.HAWK_E_UNSUPPORTED              # G < size + 3
    assert raw(idx.ds._h, 3, ["ACG"], 2, 1)[0] == _lib.HAWK_E_UNSUPPORTED
    assert raw(idx.ds._h, 29, ["A" * 29], 1, 1)[0] == _lib.HAWK_E_UNSUPPORTED           # Gs + pamlen = 33
    assert raw(idx.ds._h, 33, guides, 2, 1)[0] == _lib.HAWK_E_UNSUPPORTED               # a guide code holds 32 bases
    # scan ranges set for a shorter window than this (type, size) reads
    assert raw(idx.ds._h, 20, guides, 1, 2)[0] == _lib.HAWK_E_INVALID
    idx._set_window(18)
    assert raw(idx.ds._h, 20, guides, 2, 1)[0] == _lib.HAWK_E_INVALID
    assert raw(idx.ds._h, 20, guides, 2, 2)[0] == _lib.HAWK_OK
    # zero guides: zeros, defined
    assert raw(idx.ds._h, 20, [], 2, 2) == (_lib.HAWK_OK, 0)
    idx._set_window(20)
    # a plan view holds no planes
    from crisprhawk_hip.workload import expand_on_device
    reg = synth.make_region(11, "chrS", 9000, 1000, 8000)
    synth.add_phased_variants(reg, 12, 150, 3, frac_snv=0.7, frac_del=0.15, af_min=0.2, af_max=0.6)
    ds2, _info, _ms, _kept = expand_on_device(reg, 3, device=0, keep_plan=True)
    view = ds2.plan.view()
    assert raw(view._h, 20, guides, 2, 1)[0] == _lib.HAWK_E_INVALID
    ds2.plan.close()
    ds2.close()


def _g10_files(tmp_path):
    from crisprhawk_hip import readers
    from util import load_golden
    fx = load_golden("g10_offtargets.json.gz")["ngg"]
    fa, bed, vcf = str(tmp_path / "g.fa"), str(tmp_path / "r.bed"), str(tmp_path / "v.vcf")
    readers.write_fasta(fa, fx["contig"], fx["genome"][fx["contig"]], 60)
    with open(bed, "w") as f:
        f.write(f"{fx['contig']}\t{fx['bed_start']}\t{fx['bed_stop']}\n")
    rows = [[fx["contig"], str(p), ".", r, a, ".", "PASS", f"AF={af:.6g}", "GT"] + [f"{g[0]}|{g[1]}" for g in gts]
            for p, r, a, af, gts in fx["variants"]]
    readers.write_vcf(vcf, fx["contig"], fx["samples"], rows, False)
    return fx, fa, bed, vcf


def test_report_columns_equal_the_table_route(tmp_path):
    """search_files(offtargets_summary=True, bdna=1, brna=1) leaves the `offtargets` column of the table route at the same bulges
    - bulged rows counted - a `cfd` column within one unit of its last printed digit (1e-4 + 1e-12, the bound of
    test_gpu_offtarget_summary.test_report_columns_equal_the_table_route: the table route sums floats in row order, the summary
    integers), and no offtargets_*.tsv"""
    from crisprhawk_hip import pipeline
    fx, fa, bed, vcf = _g10_files(tmp_path)
    text = {}
    for summary in (False, True):
        out = tmp_path / f"out{int(summary)}"
        (path,) = pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(out), cfd_tables=synth.cfd_tables(),
                                        estimate_offtargets=fx["genome"], mm=fx["mm"], bdna=1, brna=1, offtargets_summary=summary).values()
        text[summary] = [ln.split("\t") for ln in open(path).read().splitlines()]
        assert len(list(out.glob("offtargets_*.tsv"))) == int(not summary)
    head = text[False][0]
    assert text[True][0] == head and len(text[True]) == len(text[False]) > 10
    c_n, c_cfd = head.index("offtargets"), head.index("cfd")
    differed = 0
    for a, b in zip(text[False][1:], text[True][1:]):
        assert [x for k, x in enumerate(a) if k != c_cfd] == [x for k, x in enumerate(b) if k != c_cfd]
        assert abs(float(a[c_cfd]) - float(b[c_cfd])) <= 1e-4 + 1e-12
        differed += a[c_cfd] != b[c_cfd]
    print("rows whose cfd text differed:", differed, "of", len(text[False]) - 1)
    # the bulged rows are in the count: more rows than the mismatch-only summary sees
    (path,) = pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "out2"), cfd_tables=synth.cfd_tables(),
                                    estimate_offtargets=fx["genome"], mm=fx["mm"], offtargets_table=False).values()
    plain = [ln.split("\t") for ln in open(path).read().splitlines()]
    assert sum(int(a[c_n]) for a in text[True][1:]) > sum(int(a[c_n]) for a in plain[1:])


def test_specificity_by_spacer_with_bulges():
    from crisprhawk_hip.offtargets import estimate_offtargets_spacers, specificity_by_spacer
    rng = np.random.default_rng(12)
    scoring.set_cfd_tables(*synth.cfd_tables())
    sp = [synth.random_sequence(rng, 20) for _ in range(4)]
    g = list(synth.random_sequence(rng, 40_000))
    for k in range(80):
        kind, b = (("DNA", 1), ("RNA", 1), ("DNA", 2), ("RNA", 2), ("", 0))[k % 5]
        B.place(g, 300 + 480 * k, B.mutate(rng, sp[k % 4], kind, b, k % 3), "CGG", False, bool(k & 8))
    contigs = {"y": "".join(g)}
    ngg = _pam("NGG", False)
    differed = 0
    for bdna, brna in ((1, 1), (2, 0), (0, 2), (2, 2)):
        want = estimate_offtargets_spacers(sp, ngg, contigs, None, 3, bdna, brna, 20, False, "", 0, True)
        got = specificity_by_spacer(sp + [sp[0].lower()], ngg, contigs, 3, 20, False, True, bdna, brna)
        assert {k: v[0] for k, v in got.items()} == {k: v[0] for k, v in want.items()} and min(v[0] for v in got.values()) > 8
        for k in want:
            assert abs(float(got[k][1]) - float(want[k][1])) <= 1e-4 + 1e-12
            differed += got[k][1] != want[k][1]
    print("cfd texts that differed:", differed, "of", 16)
    # an ambiguous base under a lookup in a BULGED row: the table route's error class and message
    site = sp[0][:12] + B.other_base(rng, sp[0][11], sp[0][12]) + sp[0][12:]  # a DNA bulge of 1 at position 12 ...
    g[20_000:20_024] = list(site[:4] + "N" + site[5:] + "TGG")                # ... and an aligned N in front of it
    bad = {"y": "".join(g)}
    assert GenomeIndex(bad, 20, 3).summary(sorted(sp), ngg, False, 3, cfd_tables=synth.cfd_tables())["n_unscorable"] == 0
    with pytest.raises(CrisprHawkCfdScoreError, match="CFDon score calculation failed"):
        specificity_by_spacer(sp, ngg, bad, 3, 20, False, True, 1, 0)
    with pytest.raises(CrisprHawkCfdScoreError, match="CFDon score calculation failed"):
        estimate_offtargets_spacers(sp, ngg, bad, None, 3, 1, 0, 20, False, "", 0, True)
    # sizes outside 0..2: the table route's error class
    from crisprhawk_hip.crisprhawk_error import CrisprHawkOffTargetsError
    with pytest.raises(CrisprHawkOffTargetsError):
        specificity_by_spacer(sp, ngg, contigs, 3, 20, False, True, 3, 0)
