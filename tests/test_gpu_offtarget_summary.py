"""The off-target summary (hawk_offtarget_summary -> GenomeIndex.summary -> offtargets.specificity_by_spacer ->
pipeline.search_files(offtargets_table=False)) against the per-site route it stands in for: the per-guide mismatch histogram
and the integer sum of the sites' CFD must equal, exactly, what the listed hits of GenomeIndex.scan give on the host."""
import ctypes as C

import numpy as np
import pytest

from crisprhawk_hip import _lib, scoring, synth
from crisprhawk_hip.crisprhawk_error import CrisprHawkCfdScoreError
from crisprhawk_hip.genome import GenomeIndex, encode_guides
from crisprhawk_hip.hapset import _p
from crisprhawk_hip.pam import PAM
from oracle import oracle as ora

pytestmark = pytest.mark.gpu

_CONCRETE = {"NGG": "TGG", "TTTV": "TTTA", "NGN": "TGA"}


def _pam(pam_s: str, right: bool) -> PAM:
    pam = PAM(pam_s, right, True)
    pam.encode(0)
    return pam


def _plant(rng, genome: list, guide: str, pam_seq: str, right: bool, n: int, max_mm: int):
    """mutated copies of guide + PAM, either strand, written into the genome"""
    L = len(guide) + len(pam_seq)
    for _ in range(n):
        g = list(guide)
        for p in rng.integers(0, len(g), size=int(rng.integers(0, max_mm + 2))):
            g[p] = "ACGT"[rng.integers(0, 4)]
        w = (pam_seq + "".join(g)) if right else ("".join(g) + pam_seq)
        if rng.random() < 0.5:
            w = ora.revcomp(w)
        pos = int(rng.integers(0, len(genome) - L))
        genome[pos:pos + L] = list(w)


def _planted_case(pam_s: str, guidelen: int, right: bool, max_mm: int, n_guides: int, n_in_pam: bool = False):
    """The genome of the scan's brute-force test - three contigs with IUPAC codes sprinkled in, families of near-identical
    guides, mutated copies of the first six guides planted on both strands, an N run - plus, so that the unscorable case is
    there at every size, three copies of guide 0 with an ambiguous base inside the spacer (and, `n_in_pam`, two whose PAM ends
    in an ambiguous base: only a PAM that ends in N admits such a site)."""
    rng = np.random.default_rng(77)
    guides = [synth.random_sequence(rng, guidelen) for _ in range(n_guides)]
    for k in range(6, n_guides, 9):
        g = list(guides[k % 6])
        g[int(rng.integers(0, guidelen))] = "ACGT"[int(rng.integers(0, 4))]
        guides[k] = "".join(g)
    concrete = _CONCRETE[pam_s]
    contigs = {}
    for name, n in (("c1", 60_000), ("c2", 25_001), ("c3", 300)):
        g = list(synth.random_sequence(rng, n, iupac_frac=0.001))
        for gd in guides[:6]:
            _plant(rng, g, gd, concrete, right, 12 if n > 1000 else 1, max_mm)
        if n > 5000:
            g[3000:3400] = "N" * 400
        contigs[name] = g
    extra = [(10_000, 3, "N", concrete), (20_000, 11, "R", concrete), (40_000, 19, "N", concrete)]
    if n_in_pam:
        extra += [(45_000, None, None, concrete[:-1] + "N"), (50_000, None, None, concrete[:-1] + "Y")]
    for pos, at, code, pm in extra:
        sp = list(guides[0])
        if at is not None and at < guidelen:
            sp[at] = code
        w = (pm + "".join(sp)) if right else ("".join(sp) + pm)
        contigs["c1"][pos:pos + len(w)] = list(w)
    return {k: "".join(v) for k, v in contigs.items()}, guides


def _host_summary(hits, guides, guidelen: int, pamlen: int, right: bool, max_mm: int, tables):
    """What the per-site route makes of listed hits: bincount of (guide, mm); per guide the sum of round(CFD, 4) in 1e-4 units
    over the hits compute_cfd can score; how many it cannot (a non-ACGT base among the first 20 spacer bases or in PAM[-2:])."""
    hist = np.zeros((len(guides), max_mm + 1), dtype=np.int64)
    e4 = np.zeros(len(guides), dtype=np.int64)
    bad_spacer = bad_pam = 0
    for h in hits:
        hist[h.guide, h.mm] += 1
        sp, pm = (h.window[pamlen:], h.window[:pamlen]) if right else (h.window[:guidelen], h.window[guidelen:])
        if tables is None:
            continue
        if "N" in sp[:20] or "N" in pm[-2:]:
            bad_spacer += "N" in sp[:20]
            bad_pam += "N" in pm[-2:] and "N" not in sp[:20]
            continue
        e4[h.guide] += int(round(round(ora.cfd(guides[h.guide], sp, pm[-2:], *tables), 4) * 1e4))
    return hist, e4, bad_spacer, bad_pam


@pytest.mark.parametrize("allpairs", [False, True])
@pytest.mark.parametrize("n_guides", [6, 200, 2300, -2300])  # all pairs; pair seeds; pair seeds; 2300 at max_mm = 7: single-block seeds
def test_summary_equals_the_per_site_route(n_guides, allpairs, monkeypatch):
    max_mm = 4
    if n_guides < 0:
        n_guides, max_mm = -n_guides, 7
    if allpairs:
        monkeypatch.setenv("HAWK_OT_ALLPAIRS", "1")
    contigs, guides = _planted_case("NGG", 20, False, max_mm, n_guides)
    pam = _pam("NGG", False)
    tables = synth.cfd_tables()
    idx = GenomeIndex(contigs, 20, 3)
    hits = idx.scan(guides, pam, False, max_mm)
    got = idx.summary(guides, pam, False, max_mm, cfd_tables=tables)
    hist, e4, bad_spacer, bad_pam = _host_summary(hits, guides, 20, 3, False, max_mm, tables)
    assert bad_spacer >= 1, "the planted genome must hold a hit with an ambiguous base in the spacer"
    assert bad_pam == 0  # a site whose PAM[-2:] is ambiguous cannot be a hit of NGG (test_unscorable_pam... covers that branch)
    assert got["hist"].dtype == np.uint32 and got["cfd_e4"].dtype == np.int64
    assert np.array_equal(got["hist"], hist)
    assert got["n_hits"] == len(hits) == int(hist.sum()) > 100
    assert got["n_unscorable"] == bad_spacer
    assert np.array_equal(got["cfd_e4"], e4) and int(e4.sum()) > 0
    # the brute force's rows give the same histogram
    want = np.zeros_like(hist)
    for seq in contigs.values():
        r = ora.offtargets(seq, guides, "NGG", False, max_mm)
        np.add.at(want, (r["guide"], r["mm"]), 1)
    assert np.array_equal(got["hist"], want)
    # counts only: the same histogram, no CFD
    plain = idx.summary(guides, pam, False, max_mm)
    assert plain["cfd_e4"] is None and plain["n_unscorable"] == 0 and np.array_equal(plain["hist"], hist)
    assert idx.last_timing["n_sites"] > 0 and idx.last_timing["match_ms"] > 0


@pytest.mark.parametrize("n_guides", [6, 200])
def test_unscorable_pam_is_counted(n_guides):
    """An ambiguous base in PAM[-2:] can only belong to a hit when the PAM ends in N (an N of the PAM accepts any genome base,
    an ambiguous one included): NGN.  Such a hit counts in hist and in n_unscorable and adds nothing to cfd_e4."""
    contigs, guides = _planted_case("NGN", 20, False, 3, n_guides, n_in_pam=True)
    pam = _pam("NGN", False)
    tables = synth.cfd_tables()
    idx = GenomeIndex(contigs, 20, 3)
    hits = idx.scan(guides, pam, False, 3)
    got = idx.summary(guides, pam, False, 3, cfd_tables=tables)
    hist, e4, bad_spacer, bad_pam = _host_summary(hits, guides, 20, 3, False, 3, tables)
    assert bad_pam >= 2 and bad_spacer >= 1
    assert np.array_equal(got["hist"], hist) and np.array_equal(got["cfd_e4"], e4)
    assert got["n_unscorable"] == bad_spacer + bad_pam


@pytest.mark.parametrize("n_guides", [6, 100])
def test_rounding_ties_reach_the_kernel(n_guides):
    """Tables made so that a site's CFD is an exact binary tie of round(x, 4) - 0.03125 = 312.5 units, 0.09375 = 937.5 units - or
    one ulp either side of it: guide j has one site, with one mismatch at position j, whose CFD is mm[j] x 1.0."""
    vals = [0.03125, 0.09375, np.nextafter(0.03125, 1.0), np.nextafter(0.03125, 0.0), np.nextafter(0.09375, 1.0), np.nextafter(0.09375, 0.0)]
    mm = np.ones((20, 4, 4))
    for j, v in enumerate(vals):
        mm[j, :, :] = v
    pt = np.ones(16)
    rng = np.random.default_rng(31)
    guides = [synth.random_sequence(rng, 20) for _ in range(n_guides)]
    g = list(synth.random_sequence(rng, 30_000))
    for j in range(6):
        sp = list(guides[j])
        sp[j] = "ACGT"[("ACGT".index(sp[j]) + 1 + j % 3) % 4]
        w = "".join(sp) + "AGG"
        if j % 2:
            w = ora.revcomp(w)
        g[4000 * (j + 1):4000 * (j + 1) + 23] = list(w)
    idx = GenomeIndex({"t": "".join(g)}, 20, 3)
    got = idx.summary(guides, _pam("NGG", False), False, 1, cfd_tables=(mm, pt))
    assert got["hist"][:6].tolist() == [[0, 1]] * 6 and got["n_unscorable"] == 0
    assert got["cfd_e4"][:6].tolist() == [int(round(round(float(v), 4) * 1e4)) for v in vals] == [312, 938, 313, 312, 938, 937]


def test_report_columns_equal_the_table_route(tmp_path):
    """search_files(offtargets_table=False) leaves the `offtargets` column of offtargets_table=True, a `cfd` column within one unit
    of its last printed digit (1e-4: the table route sums floats in row order, the summary integers), and no offtargets_*.tsv.
    Measured on the g10 "ngg" fixture: no row's cfd text differed (the assertion below prints the number that did)."""
    from crisprhawk_hip import pipeline, readers
    from util import load_golden
    fx = load_golden("g10_offtargets.json.gz")["ngg"]
    fa, bed, vcf = str(tmp_path / "g.fa"), str(tmp_path / "r.bed"), str(tmp_path / "v.vcf")
    readers.write_fasta(fa, fx["contig"], fx["genome"][fx["contig"]], 60)
    with open(bed, "w") as f:
        f.write(f"{fx['contig']}\t{fx['bed_start']}\t{fx['bed_stop']}\n")
    rows = [[fx["contig"], str(p), ".", r, a, ".", "PASS", f"AF={af:.6g}", "GT"] + [f"{g[0]}|{g[1]}" for g in gts]
            for p, r, a, af, gts in fx["variants"]]
    readers.write_vcf(vcf, fx["contig"], fx["samples"], rows, False)
    text = {}
    for table in (True, False):
        out = tmp_path / f"out{int(table)}"
        (path,) = pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(out), cfd_tables=synth.cfd_tables(),
                                        estimate_offtargets=fx["genome"], mm=fx["mm"], offtargets_table=table).values()
        text[table] = [ln.split("\t") for ln in open(path).read().splitlines()]
        assert len(list(out.glob("offtargets_*.tsv"))) == int(table)
    head = text[True][0]
    assert text[False][0] == head and len(text[False]) == len(text[True]) > 10
    c_n, c_cfd = head.index("offtargets"), head.index("cfd")
    differed = 0
    for a, b in zip(text[True][1:], text[False][1:]):
        assert [x for k, x in enumerate(a) if k != c_cfd] == [x for k, x in enumerate(b) if k != c_cfd]
        assert abs(float(a[c_cfd]) - float(b[c_cfd])) <= 1e-4 + 1e-12
        differed += a[c_cfd] != b[c_cfd]
    assert sum(int(a[c_n]) for a in text[True][1:]) > len(text[True]) // 2  # guides of alternative haplotypes may have no site in REF
    print("rows whose cfd text differed:", differed, "of", len(text[True]) - 1)


def test_refusals_and_edges():
    L = _lib.lib()
    rng = np.random.default_rng(9)
    seq = synth.random_sequence(rng, 5000)
    guides = [seq[100:120], seq[300:320], seq[100:120]]  # a duplicate
    pam = _pam("NGG", False)
    idx = GenomeIndex({"a": seq}, 20, 3)
    tables = synth.cfd_tables()

    def raw(handle, guidelen, pamlen, g2, max_mm=2):
        par = _lib.OtParams(pam.bits, pam.bitsrc, pamlen, guidelen, 0, max_mm)
        hist = np.zeros((max(len(g2), 1), max_mm + 1), np.uint32)
        nh, nu = C.c_uint64(7), C.c_uint64(7)
        rc = L.hawk_offtarget_summary(handle, C.byref(par), _p(g2), len(g2), None, None, _p(hist), None, C.byref(nh), C.byref(nu), None)
        return rc, hist, nh.value, nu.value

    g2 = encode_guides(guides)
    assert raw(idx.ds._h, 30, 3, g2)[0] == _lib.HAWK_E_UNSUPPORTED  # a 33-base window
    assert raw(idx.ds._h, 0, 3, g2)[0] == _lib.HAWK_E_UNSUPPORTED
    # a plan view holds no planes
    from crisprhawk_hip.workload import expand_on_device
    reg = synth.make_region(11, "chrS", 9000, 1000, 8000)
    synth.add_phased_variants(reg, 12, 150, 3, frac_snv=0.7, frac_del=0.15, af_min=0.2, af_max=0.6)
    ds2, _info, _ms, _kept = expand_on_device(reg, 3, device=0, keep_plan=True)
    view = ds2.plan.view()
    assert raw(view._h, 20, 3, g2)[0] == _lib.HAWK_E_INVALID
    ds2.plan.close()
    ds2.close()
    # zero guides: zeros, defined
    rc, _hist, nh, nu = raw(idx.ds._h, 20, 3, np.zeros(0, np.uint64))
    assert (rc, nh, nu) == (_lib.HAWK_OK, 0, 0)
    z = idx.summary([], pam, False, 2, cfd_tables=tables)
    assert z["hist"].shape == (0, 3) and z["cfd_e4"].shape == (0,) and z["n_hits"] == 0
    # zero sites: a genome without a single GG
    bare = GenomeIndex({"b": "ACT" * 400}, 20, 3)
    z = bare.summary(guides, pam, False, 2, cfd_tables=tables)
    assert not z["hist"].any() and not z["cfd_e4"].any() and z["n_hits"] == 0 and bare.last_timing["n_sites"] == 0
    # duplicates: equal rows
    r = idx.summary(guides, pam, False, 2, cfd_tables=tables)
    assert np.array_equal(r["hist"][0], r["hist"][2]) and r["cfd_e4"][0] == r["cfd_e4"][2]
    # a rank without rows returns zeros
    empty = GenomeIndex({"a": seq}, 20, 3, shard=(1, 2))
    assert empty.ds is None
    z = empty.summary(guides, pam, False, 2, cfd_tables=tables)
    assert not z["hist"].any() and z["n_hits"] == 0 and z["cfd_e4"].tolist() == [0, 0, 0]


def test_specificity_by_spacer_texts_and_errors():
    from crisprhawk_hip.offtargets import _read_offtargets, _compute_cfd_score, offtargets_by_spacer, search, specificity_by_spacer
    rng = np.random.default_rng(12)
    # a non-Cas9 PAM: counts, and the global CFD the table route's NA -> 0 gives
    g = list(synth.random_sequence(rng, 20_000))
    sp = [synth.random_sequence(rng, 23) for _ in range(3)]
    for k, s in enumerate(sp):
        for c in range(k + 1):
            g[1000 + 3000 * k + 100 * c:1000 + 3000 * k + 100 * c + 27] = list("TTTA" + s)
    cpf1 = _pam("TTTV", True)
    got = specificity_by_spacer(sp + [sp[0].lower()], cpf1, {"x": "".join(g)}, 2, 23, True, True)
    assert got == {s: (k + 1, "1.0") for k, s in enumerate(sp)}
    # SpCas9: the texts of the per-site route on a genome where every hit can be scored
    scoring.set_cfd_tables(*synth.cfd_tables())
    g = list(synth.random_sequence(rng, 40_000))
    sp = [synth.random_sequence(rng, 20) for _ in range(4)]
    for k, s in enumerate(sp):
        _plant(rng, g, s, "CGG", False, 30, 3)
    genome = GenomeIndex({"y": "".join(g)}, 20, 3)
    ngg = _pam("NGG", False)
    ots = _compute_cfd_score(_read_offtargets(search(genome, sorted(sp), ngg, False, 3, 0, True), ngg, False, True), 0, True)
    want = offtargets_by_spacer(ots, sorted(sp))
    got = specificity_by_spacer(sp, ngg, genome, 3, 20, False, True)
    assert {k: v[0] for k, v in got.items()} == {k: v[0] for k, v in want.items()} and min(v[0] for v in got.values()) > 5
    for k in want:
        assert abs(float(got[k][1]) - float(want[k][1])) <= 1e-4 + 1e-12
    # an ambiguous base under a lookup: the table route's error class and message
    g[5000:5023] = list(sp[0][:7] + "N" + sp[0][8:] + "TGG")
    genome = GenomeIndex({"y": "".join(g)}, 20, 3)
    with pytest.raises(CrisprHawkCfdScoreError, match="CFDon score calculation failed"):
        specificity_by_spacer(sp, ngg, genome, 3, 20, False, True)
    with pytest.raises(CrisprHawkCfdScoreError, match="CFDon score calculation failed"):
        _compute_cfd_score(_read_offtargets(search(genome, sorted(sp), ngg, False, 3, 0, True), ngg, False, True), 0, True)


def test_shards_add_up():
    """Two (and three) GenomeIndex shards of one genome on one GPU: their integer arrays sum to the unsharded ones exactly."""
    rng = np.random.default_rng(78)
    contigs = {f"c{i}": synth.random_sequence(rng, 90_000 + 7000 * i, iupac_frac=0.0005) for i in range(5)}
    guides = [seq[p:p + 20] for seq in contigs.values() for p in range(100, 70_000, 1000)]  # every shard holds on-targets
    guides = [g for g in guides if set(g) <= set("ACGT")]
    pam = _pam("NGG", False)
    tables = synth.cfd_tables()
    whole = GenomeIndex(contigs, 20, 3, piece=20_000).summary(guides, pam, False, 4, cfd_tables=tables)
    assert whole["n_hits"] >= 5 and whole["cfd_e4"].sum() > 0
    for world in (2, 3):
        parts = [GenomeIndex(contigs, 20, 3, piece=20_000, shard=(r, world)).summary(guides, pam, False, 4, cfd_tables=tables) for r in range(world)]
        assert all(p["n_hits"] > 0 for p in parts)
        assert np.array_equal(sum(p["hist"].astype(np.int64) for p in parts), whole["hist"])
        assert np.array_equal(sum(p["cfd_e4"] for p in parts), whole["cfd_e4"])
        assert sum(p["n_hits"] for p in parts) == whole["n_hits"] and sum(p["n_unscorable"] for p in parts) == whole["n_unscorable"]


def test_far_more_hits_than_the_scan_capacity():
    """Four guides planted 8 x 10^5 times per contig at 0..3 mismatches, either strand, in two contigs: 1.6 x 10^6 hits, more than
    one and a half times the default capacity of `scan` (2^20), in one summary call without a retry; equal to a host count made
    in chunks of 10^6 bases."""
    rng = np.random.default_rng(2024)
    guides = [synth.random_sequence(rng, 20) for _ in range(4)]
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    per_contig, want = 200_000, np.zeros((4, 4), dtype=np.int64)
    contigs = {}
    for name in ("u", "v"):
        gi = rng.integers(0, 4, size=per_contig * 4)
        sites = np.frombuffer("".join(guides).encode(), dtype=np.uint8).reshape(4, 20)[gi].copy()
        nmm = rng.integers(0, 4, size=len(gi))
        for k in range(3):  # up to three substitutions at distinct positions, each to a different base
            on = nmm > k
            col = (rng.integers(0, 6, size=len(gi)) + 7 * k) % 20
            cur = sites[np.arange(len(gi)), col]
            new = np.frombuffer(b"ACGT", dtype=np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), cur) + 1 + k) % 4]
            sites[np.arange(len(gi)), col] = np.where(on, new, cur)
        fwd = np.concatenate([sites, np.tile(np.frombuffer(b"TGGAC", dtype=np.uint8), (len(gi), 1))], axis=1)  # site + TGG + 2 spacer bases
        flip = rng.random(len(gi)) < 0.5
        text = b"".join((row.tobytes().translate(comp)[::-1] if f else row.tobytes()) for row, f in zip(fwd, flip))
        contigs[name] = text.decode()
    pam = _pam("NGG", False)
    idx = GenomeIndex(contigs, 20, 3)
    got = idx.summary(guides, pam, False, 3, cfd_tables=synth.cfd_tables())
    for seq in contigs.values():  # the host count, in chunks that overlap by a window less one
        step = 25 * 40_000
        for o in range(0, len(seq), step):
            r = ora.offtargets(seq[o:o + step + 22], guides, "NGG", False, 3, cap=1 << 17)
            np.add.at(want, (r["guide"], r["mm"]), 1)
    assert got["n_hits"] == int(want.sum()) > (1 << 20) + (1 << 19)
    assert np.array_equal(got["hist"], want) and got["n_unscorable"] == 0 and (got["cfd_e4"] > 0).all()
