"""The off-target scan over a variant-enriched genome on the device (hawk_genome_variants: k_ov_fill; hawk_offtarget_variant_scan:
k_scan_raw over the allele planes, k_ov_filter, k_ov_sites, k_ov_match) against its host twin with `==` on sorted rows, against the
brute force over strings (offtarget_variant_refs.brute), against an oracle made of code that was there before (the plain scan of
genomes with one ALT base substituted), and through the product's routes to offtargets_*.tsv."""
import ctypes as C
import random

import numpy as np
import pytest

import offtarget_variant_refs as V
import ottable_refs as R
from crisprhawk_hip import _lib, scoring, synth
from crisprhawk_hip.coordinate import Coordinate
from crisprhawk_hip.genome import GenomeIndex, encode_guides, host_variant_scan
from crisprhawk_hip.offtargets import OTREPCNAMES, estimate_offtargets_spacers
from util import load_golden

pytestmark = pytest.mark.gpu

SYSTEMS = (("NGG", 20, False), ("TTTV", 23, True))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _both(sc, max_mm, piece=V.PIECE, guides=None, cap=1 << 20):
    """(index, device columns) after holding them to the host twin: rows as sorted tuples, stats as dicts"""
    contigs = sc.text()
    guides = sc.guides if guides is None else guides
    pam = V.make_pam(sc.pam_text, sc.right)
    idx = GenomeIndex(contigs, sc.G, sc.P, piece=piece, variants=sc.records)
    h, tm = idx.variant_arrays(guides, pam, sc.right, max_mm, cap=cap)
    hh, stats = host_variant_scan(contigs, sc.G, sc.P, piece, sc.records, guides, pam, sc.right, max_mm)
    assert V.raw_tuples(h) == V.raw_tuples(hh)
    assert idx.variant_stats == stats
    assert tm["n_sites"] > 0 or len(h["guide"]) == 0
    return idx, h


@pytest.mark.parametrize("pam_text,G,right", SYSTEMS)
@pytest.mark.parametrize("max_mm", (0, 2, 4))
def test_device_rows_equal_the_host_twin_on_placed_cases(pam_text, G, right, max_mm):
    sc = V.standard_scene(pam_text, G, right, max_mm)
    idx, h = _both(sc, max_mm)
    want = V.brute(sc.text(), sc.records, sc.guides, pam_text, right, max_mm)
    assert V.rows_as_tuples(h, idx.rows, sc.L) == want
    have = {(g, c, p, s) for g, c, p, s, _mm, _w, _a in want}
    for label, must in V.expect_rows(sc, max_mm).items():
        assert (sc.placed[label] in have) == must, label


def _seam_scene():
    """A variant at in-row positions 31, 32, 63, 64, at piece - 1 and piece, in the overlap of two rows (entered in both) and at
    the last base of a contig - each needed by a site, on both strands (chr1 / chr2: +, chr3 / chr4: -)."""
    sc = V.Scene("NGG", 20, False, 23, lengths=(3000, 2500, 3000, 2500))
    L = sc.L
    for strand, (ca, cb) in enumerate((("chr1", "chr2"), ("chr3", "chr4"))):
        for contig, spots in ((ca, (31, 64, V.PIECE - 1, 2 * V.PIECE + 6)), (cb, (32, 63, V.PIECE, 2 * V.PIECE + 6))):
            n = len(sc.contigs[contig])
            for k, p in enumerate(spots + (n - 1,)):
                start = min(p - 10, n - L)
                o = p - start
                i = L - 1 - o if strand else o  # the window position that lies on genome position p
                gi = k % len(sc.guides)
                w = sc.window(gi)
                bad = sc.other(w[i], "G" if i >= sc.G else "")
                label = f"{contig}:{p}"
                sc.place(label, contig, start, strand, gi, {i: bad}, {i: w[i]})
    return sc


def test_seams_of_words_pieces_overlaps_and_contig_ends():
    sc = _seam_scene()
    idx, h = _both(sc, 0)
    got = V.rows_as_tuples(h, idx.rows, sc.L)
    assert got == V.brute(sc.text(), sc.records, sc.guides, "NGG", False, 0)
    have = {(g, c, p, s): (mm, w, a) for g, c, p, s, mm, w, a in got}
    for label, key in sc.placed.items():
        mm, w, a = have[key]
        assert mm == 0 and w == sc.window(key[0]) and bin(a).count("1") == 1, label
    # the overlap: the variant is entered in two rows, its site is reported once, by the row that owns the window start
    for contig in ("chr1", "chr2", "chr3", "chr4"):
        gi, _c, pos, strand = sc.placed[f"{contig}:{2 * V.PIECE + 6}"]
        mine = [(r, q) for g, r, q, s in zip(h["guide"].tolist(), h["row"].tolist(), h["q"].tolist(), h["strand"].tolist())
                if g == gi and s == strand and idx.rows[r][0] == contig and idx.rows[r][1] + q == pos]
        assert len(mine) == 1 and idx.rows[mine[0][0]][1] == V.PIECE and pos < 2 * V.PIECE
    assert idx.variant_stats["applied"] == len(sc.records)


def test_site_records_cross_a_workgroup():
    """One row of more than 1024 bitmap words (two workgroups of k_ov_filter / k_ov_sites), sites in its first and its last word."""
    sc = V.Scene("NGG", 20, False, 31, lengths=(40000,), n_guides=8)
    n, L = 40000, sc.L
    for k, (start, strand) in enumerate(((2, 0), (5 + L, 1), (n - L, 0), (n - 2 * L - 3, 1), (32768 - 10, 0), (32768 + 40, 1))):
        g = sc.guides[k]
        sc.place(f"s{k}", "chr1", start, strand, k, {sc.sp(9): sc.other(g[9])}, {sc.sp(9): g[9]})
    rng = random.Random(3)
    for pos in range(200, n - 200, 97):  # and variants all along the row
        c = sc.contigs["chr1"][pos]
        sc.records.append(("chr1", pos, c, rng.choice([x for x in "ACGT" if x != c])))
    idx, h = _both(sc, 1, piece=1 << 16)
    assert len(idx.rows) == 1 and idx.ds.stride > 1024
    got = V.rows_as_tuples(h, idx.rows, L)
    assert got == V.brute(sc.text(), sc.records, sc.guides, "NGG", False, 1)
    have = {(g, c, p, s) for g, c, p, s, *_r in got}
    assert all(key in have for key in sc.placed.values())
    words = {(idx.rows[r][1] + q) // 32 for r, q in zip(h["row"].tolist(), h["q"].tolist())}
    assert 0 in words and (n - L) // 32 in words


@pytest.mark.parametrize("n_guides", (1, 1024, 1025))
def test_guide_counts_around_the_lds_chunk(n_guides):
    sc = V.Scene("NGG", 20, False, 41, lengths=(700, 600), n_guides=3)
    rng = random.Random(n_guides)
    filler = ["".join(rng.choice("ACGT") for _ in range(20)) for _ in range(n_guides)]
    # the guides that have sites sit at the chunk's first and last slots and behind it
    slots = sorted({0, min(1023, n_guides - 1), n_guides - 1})
    for k, slot in enumerate(slots):
        filler[slot] = sc.guides[k]
    for k, slot in enumerate(slots):
        g = sc.guides[k]
        for strand, contig in enumerate(("chr1", "chr2")):
            sc.place(f"g{slot}{'+-'[strand]}", contig, 60 + 70 * k, strand, k, {sc.sp(3): sc.other(g[3])}, {sc.sp(3): g[3]})
    idx, h = _both(sc, 1, guides=filler)
    have = {(g, idx.rows[r][0], idx.rows[r][1] + q, s) for g, r, q, s in zip(h["guide"].tolist(), h["row"].tolist(), h["q"].tolist(), h["strand"].tolist())}
    for k, slot in enumerate(slots):
        for strand, contig in enumerate(("chr1", "chr2")):
            assert (slot, contig, 60 + 70 * k, strand) in have


def test_capacity_protocol_and_the_retry():
    sc = V.standard_scene("NGG", 20, False, 2)
    idx, h = _both(sc, 2, cap=3)  # variant_arrays meets HAWK_E_CAPACITY and calls again with room
    n_rows = len(h["guide"])
    assert n_rows > 3
    pam = V.make_pam("NGG", False)
    g2 = encode_guides(sc.guides)
    par = _lib.OtParams(pam.bits, pam.bitsrc, 3, 20, 0, 2)
    out = {k: np.full(3, 0xEE, t) for k, t in (("guide", np.uint32), ("row", np.uint32), ("q", np.uint32), ("strand", np.uint8), ("mm", np.uint8),
                                               ("code", np.uint64), ("nmask", np.uint32), ("alt", np.uint32))}
    n, tm = C.c_uint64(0), _lib.OtTiming()
    rc = idx.ds._L.hawk_offtarget_variant_scan(idx.ds._h, C.byref(par), _p(g2), len(g2), *[_p(v) for v in out.values()], C.c_uint64(3), C.byref(n), C.byref(tm))
    assert rc == _lib.HAWK_E_CAPACITY and n.value == n_rows
    assert tm.total_ms >= tm.match_ms >= 0 and tm.n_sites > 0  # device clock stamps: never negative, never huge
    assert tm.total_ms < 10_000


def test_without_variants_the_scan_is_refused():
    sc = V.Scene("NGG", 20, False, 5, lengths=(500,))
    idx = GenomeIndex(sc.text(), 20, 3, piece=V.PIECE)
    pam = V.make_pam("NGG", False)
    g2 = encode_guides(sc.guides)
    par = _lib.OtParams(pam.bits, pam.bitsrc, 3, 20, 0, 2)
    n = C.c_uint64(0)
    rc = idx.ds._L.hawk_offtarget_variant_scan(idx.ds._h, C.byref(par), _p(g2), len(g2), None, None, None, None, None, None, None, None,
                                               C.c_uint64(0), C.byref(n), None)
    assert rc == _lib.HAWK_E_INVALID
    with pytest.raises(ValueError):
        idx.scan(sc.guides, pam, False, 2, variants=True)
    with pytest.raises(ValueError):
        idx.offtarget_arrays(sc.guides, pam, False, 2, variants=True)
    # an index with an empty variant list has its planes and no rows
    idx.add_variants([])
    h, _tm = idx.variant_arrays(sc.guides, pam, False, 2)
    assert len(h["guide"]) == 0


def test_oracle_of_merged_code_one_variant_per_window():
    """With the variants at least L bases apart a window holds at most one.  For each variant the EXISTING scan of the genome
    with the ALT base substituted lists the rows of the windows that read it; those that cover the variant and where the ALT base
    is the guide's (spacer) or REF's base is outside the PAM's set (PAM) are the variant rows."""
    for pam_text, G, right in SYSTEMS:
        sc = V.Scene(pam_text, G, right, 61, lengths=(900, 700), n_guides=8)
        L, rng = sc.L, random.Random(9)
        spots = [(name, p + rng.randrange(12)) for name, seq in sc.contigs.items() for p in range(40, len(seq) - 60, L + 14)]
        alts = {}
        for k, (name, p) in enumerate(spots[::3]):  # every third variant is needed by a site: spacer positions and the PAM
            strand, gi = k & 1, k % 8
            o = (3, 11, L - 1, 0)[k % 4] if not right else (5, 12, 0, L - 1)[k % 4]
            start = p - o
            i = L - 1 - o if strand else o
            w = sc.window(gi)
            in_pam = (i >= G) if not right else (i < sc.P)
            bad = sc.other(w[i], V.IUPAC[pam_text[i - sc.pm(0)]] if in_pam else "")
            sc.place(f"o{k}", name, start, strand, gi, {i: bad})
            alts[(name, p)] = V.COMP[w[i]] if strand else w[i]
        for name, p in spots:
            c = sc.contigs[name][p]
            sc.records.append((name, p, c, alts.get((name, p)) or rng.choice([x for x in "ACGT" if x != c])))
        max_mm = 2
        pam = V.make_pam(pam_text, right)
        contigs = sc.text()
        idx = GenomeIndex(contigs, G, sc.P, piece=V.PIECE, variants=sc.records)
        assert idx.variant_stats["applied"] == len(sc.records)
        h, _tm = idx.variant_arrays(sc.guides, pam, right, max_mm)
        got = sorted((g, c, p, s, mm, w) for g, c, p, s, mm, w, _a in V.rows_as_tuples(h, idx.rows, L))
        want = []
        for name, p, ref, alt in sc.records:
            sub = dict(contigs)
            sub[name] = contigs[name][:p] + alt + contigs[name][p + 1:]
            for hit in GenomeIndex(sub, G, sc.P, piece=V.PIECE).scan(sc.guides, pam, right, max_mm):
                if hit.contig != name or not hit.position <= p < hit.position + L:
                    continue
                minus = hit.strand == "-"
                i = hit.position + L - 1 - p if minus else p - hit.position
                a, r = (V.COMP[alt], V.COMP[ref]) if minus else (alt, ref)
                if (i < sc.P) if right else (i >= G):  # a PAM position
                    k = i - sc.pm(0)
                    keep = pam_text[k] != "N" and r not in V.IUPAC[pam_text[k]]
                else:
                    keep = a == sc.guides[hit.guide][i - sc.sp(0)]
                if keep:
                    want.append((hit.guide, name, hit.position, int(minus), hit.mm, hit.window))
        assert got == sorted(want) and len(got) >= len(alts)


def test_the_plain_scan_does_not_see_the_variants():
    sc = V.standard_scene("NGG", 20, False, 3)
    pam = V.make_pam("NGG", False)
    contigs = sc.text()
    a, _ = GenomeIndex(contigs, 20, 3, piece=V.PIECE).scan_arrays(sc.guides, pam, False, 3)
    idx = GenomeIndex(contigs, 20, 3, piece=V.PIECE, variants=sc.records)
    idx.variant_arrays(sc.guides, pam, False, 3)
    b, _ = idx.scan_arrays(sc.guides, pam, False, 3)
    assert len(a["guide"]) > 0
    oa = np.lexsort((a["strand"], a["q"], a["row"], a["guide"]))
    ob = np.lexsort((b["strand"], b["q"], b["row"], b["guide"]))
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k][oa], b[k][ob]), k
    # and scan(variants=True) is the plain list with the variant rows added
    plain = idx.scan(sc.guides, pam, False, 3)
    both = idx.scan(sc.guides, pam, False, 3, variants=True)
    hv, _ = idx.variant_arrays(sc.guides, pam, False, 3)
    assert len(both) == len(plain) + len(hv["guide"]) and all(x in both for x in plain)


# ---- through the product's routes ---------------------------------------------------------------------------------------------
def _table(path):
    lines = path.read_text().splitlines()
    return lines[0].split("\t"), [ln.split("\t") for ln in lines[1:]]


def test_estimate_offtargets_spacers_with_variants(tmp_path):
    from crisprhawk_hip.utils import round_score
    tables = synth.cfd_tables()
    scoring.set_cfd_tables(*tables)
    sc = V.standard_scene("NGG", 20, False, 2, with_n=False)
    pam = V.make_pam("NGG", False)
    contigs = {k: v for k, v in sc.text().items() if k != "tiny"}
    coord = Coordinate("chr1", 200, 900, 100)
    plain_dir, var_dir, off_dir = tmp_path / "plain", tmp_path / "var", tmp_path / "off"
    for d in (plain_dir, var_dir, off_dir):
        d.mkdir()
    idx = GenomeIndex(contigs, 20, 3, piece=V.PIECE, variants=sc.records)
    res_plain = estimate_offtargets_spacers(sc.guides, pam, GenomeIndex(contigs, 20, 3, piece=V.PIECE), coord, 2, 0, 0, 20, False, str(plain_dir), 0, True)
    res_off = estimate_offtargets_spacers(sc.guides, pam, idx, coord, 2, 0, 0, 20, False, str(off_dir), 0, True)
    res = estimate_offtargets_spacers(sc.guides, pam, idx, coord, 2, 0, 0, 20, False, str(var_dir), 0, True, variants=True)
    (fp,), (fo,), (fv,) = (list(d.glob("offtargets_*.tsv")) for d in (plain_dir, off_dir, var_dir))
    # without the switch: byte for byte the route as it was, also on an index that holds variants
    assert fp.read_bytes() == fo.read_bytes() and res_plain == res_off
    head, rows = _table(fv)
    assert head == OTREPCNAMES + ["origin", "variant_id"]
    assert _table(fp)[0] == OTREPCNAMES
    ref_rows = [r[:11] for r in rows if r[11] == "ref"]
    assert ref_rows == _table(fp)[1] and all(r[12] == "NA" for r in rows if r[11] == "ref")
    alt_rows = [r for r in rows if r[11] == "alt"]
    assert len(alt_rows) > 10 and {r[11] for r in rows} == {"ref", "alt"}
    # every row - the alt rows with their RESOLVED window - is what the host emitter prints for the record, in the file's order
    arr = idx.offtarget_arrays(sorted(sc.guides), pam, False, 2, variants=True)
    rc, roff, _nb, _no, names = idx.row_table()
    pos = roff[arr["row"]].astype(np.int64) + arr["q"]
    rank = {n: i for i, n in enumerate(sorted(names))}
    order = np.lexsort((pos, np.array([rank[names[c]] for c in rc[arr["row"]]])))
    st, text, _off, units, n_uns = R.host_text(arr, sorted(sc.guides), 20, "NGG", False, rc, roff, names, order.astype(np.uint64), tables)
    assert st == _lib.HAWK_OK and n_uns == 0
    assert ["\t".join(r[:11]) for r in rows] == text
    assert [r[11] for r in rows] == ["alt" if a else "ref" for a in (arr["alt"][order] != 0).tolist()]
    # variant_id: contig-pos1-REF/ALT of the ALT bases the row reads, ascending, as the records spell them
    known = {f"{c}-{p + 1}-{r}/{a}" for c, p, r, alts in sc.records for a in alts.split(",") if len(r) == 1}
    for r in alt_rows:
        ids = r[12].split(",")
        assert all(i in known for i in ids) and ids == sorted(ids, key=lambda s: int(s.split("-")[1]))
        assert all(r[0] == i.split("-")[0] and int(r[1]) <= int(i.split("-")[1]) - 1 < int(r[1]) + 23 for i in ids)
    # counts and global CFD: recomputed from the file
    for sp in sc.guides:
        mine = [r for r in rows if r[3][:20].upper() == sp]
        tot = 0.0
        for r in mine:
            tot += float(r[9])
        assert res[sp] == (len(mine), str(round_score(100 / (100 + tot))))
    assert sum(v[0] for v in res.values()) == len(rows) == sum(v[0] for v in res_plain.values()) + len(alt_rows)


def test_refusals_write_nothing(tmp_path):
    from crisprhawk_hip import pipeline, readers
    sc = V.standard_scene("NGG", 20, False, 1, with_n=False)
    pam = V.make_pam("NGG", False)
    contigs = {k: v for k, v in sc.text().items() if k != "tiny"}
    coord = Coordinate("chr1", 200, 900, 100)
    idx = GenomeIndex(contigs, 20, 3, piece=V.PIECE, variants=sc.records, max_bulge=1)
    out = tmp_path / "out"
    out.mkdir()
    for kw in (dict(bdna=1), dict(brna=1), dict(engine="objects")):
        with pytest.raises(ValueError):
            estimate_offtargets_spacers(sc.guides, pam, idx, coord, 1, kw.get("bdna", 0), kw.get("brna", 0), 20, False, str(out), 0, True,
                                        engine=kw.get("engine", "device"), variants=True)
    with pytest.raises(ValueError):  # an index nobody added variants to
        estimate_offtargets_spacers(sc.guides, pam, GenomeIndex(contigs, 20, 3, piece=V.PIECE), coord, 1, 0, 0, 20, False, str(out), 0, True, variants=True)
    fa, bed, vcf = str(tmp_path / "g.fa"), str(tmp_path / "r.bed"), str(tmp_path / "v.vcf")
    readers.write_fasta(fa, "chr1", contigs["chr1"], 60)
    with open(bed, "w") as f:
        f.write("chr1\t300\t800\n")
    readers.write_vcf(vcf, "chr1", ["s1"], [["chr1", "401", ".", contigs["chr1"][400], "A" if contigs["chr1"][400] != "A" else "C", ".", "PASS", "AF=0.1", "GT", "0|1"]], False)
    for kw in (dict(bdna=1), dict(brna=1), dict(offtargets_table=False), dict(offtargets_summary=True), dict(estimate_offtargets=None)):
        args = dict(estimate_offtargets=contigs, mm=1, offtargets_variants=True)
        args.update(kw)
        with pytest.raises(ValueError):
            pipeline.search_files(fa, bed, [vcf], "NGG", 20, False, str(out), cfd_tables=synth.cfd_tables(), **args)
    assert list(out.iterdir()) == []


def test_search_files_with_offtargets_variants(tmp_path):
    from crisprhawk_hip import pipeline, readers
    fx = load_golden("g10_offtargets.json.gz")["ngg"]
    fa, bed, vcf = str(tmp_path / "g.fa"), str(tmp_path / "r.bed"), str(tmp_path / "v.vcf")
    readers.write_fasta(fa, fx["contig"], fx["genome"][fx["contig"]], 60)
    with open(bed, "w") as f:
        f.write(f"{fx['contig']}\t{fx['bed_start']}\t{fx['bed_stop']}\n")
    rows = [[fx["contig"], str(p), ".", r, a, ".", "PASS", f"AF={af:.6g}", "GT"] + [f"{g[0]}|{g[1]}" for g in gts]
            for p, r, a, af, gts in fx["variants"]]
    readers.write_vcf(vcf, fx["contig"], fx["samples"], rows, False)
    outs = {}
    for tag, kw in (("plain", {}), ("off", dict(offtargets_variants=False)), ("var", dict(offtargets_variants=True)),
                    ("list", dict(offtargets_variants=[vcf]))):
        d = tmp_path / tag
        pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(d), cfd_tables=synth.cfd_tables(),
                              estimate_offtargets=fx["genome"], mm=fx["mm"], **kw)
        outs[tag] = {p.name: p.read_bytes() for p in sorted(d.iterdir()) if p.is_file()}
    # without the switch (None, the default) and with False: today's behaviour byte for byte, every file of the run
    assert outs["plain"] == outs["off"] and outs["var"] == outs["list"]
    name = f"offtargets_{fx['contig']}_{fx['bed_start']}_{fx['bed_stop']}.tsv"
    assert sorted(outs["plain"][name].decode().splitlines()) == sorted(fx["nobulge_offtargets_tsv"].splitlines())
    lines = outs["var"][name].decode().splitlines()
    head, body = lines[0].split("\t"), [ln.split("\t") for ln in lines[1:]]
    assert head == OTREPCNAMES + ["origin", "variant_id"]
    assert ["\t".join(r[:11]) for r in body if r[11] == "ref"] == outs["plain"][name].decode().splitlines()[1:]
    # the alt rows are those of the index's own variant scan over the report's spacers
    idx = GenomeIndex(fx["genome"], fx["guidelen"], len(fx["pam"]), variants=[vcf])
    spacers = sorted({r[3][:fx["guidelen"]].upper() for r in body}) if not fx["right"] else sorted({r[3][len(fx["pam"]):].upper() for r in body})
    hv, _tm = idx.variant_arrays(spacers, V.make_pam(fx["pam"], fx["right"]), fx["right"], fx["mm"])
    assert sum(r[11] == "alt" for r in body) == len(hv["guide"])
    assert idx.variant_stats["applied"] + sum(idx.variant_stats["dropped"].values()) == sum(len(a.split(",")) for _p, _r, a, _af, _g in fx["variants"])
