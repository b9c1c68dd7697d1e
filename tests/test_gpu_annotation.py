"""The BED annotation join on the device (hawk_annot.hip, bedannot.AnnotTable) against the brute force of tests/annot_refs.py,
`==` on blob and offsets; then end to end: pipeline.search_files with G11's annotation files against the TSVs the reference wrote
(tests/golden/make_golden_annotation.py).  Rows whose byte offsets cross 2^32 are not built here: a 4 GiB blob plus its brute
force does not fit a test's time; the 64-bit scan is exercised at workgroup seams (n = 2047, 2048, 2049 rows and 10^6) instead."""
import io
import os

import numpy as np
import pytest

import annot_refs as ar
from util import load_golden

from crisprhawk_hip import bedannot, pipeline, readers, reports, synth

pytestmark = pytest.mark.gpu
G11 = load_golden("g11_annotation.json.gz")


def _check(starts, ends, labels, qs, qe, brute=ar.join_rows):
    wb, wo = ar.ragged(brute(starts, ends, labels, qs, qe))
    lb, lo = ar.ragged(labels)
    tab = bedannot.AnnotTable(np.asarray(starts, np.int64), np.asarray(ends, np.int64), lb, lo)
    try:
        got = tab.query(np.asarray(qs, np.int64), np.asarray(qe, np.int64))
        assert got.off.dtype == np.uint64 and np.array_equal(got.off, wo)
        assert np.array_equal(got.blob, wb)
        return got, tab.n_overlaps
    finally:
        tab.close()


@pytest.mark.parametrize("case", ["ngg", "cpf1", "unphased"])
def test_g11_panels(case):
    fx = G11[case]
    qs = [s for s, _ in fx["guide_intervals"]]
    qe = [e for _, e in fx["guide_intervals"]]
    ot = [ln.split("\t") for ln in (fx["offtargets_tsv"] or "").splitlines()[1:]]
    for texts, label in ((fx["annotation_files"], ar.func_label), (fx["gene_annotation_files"], ar.gene_label)):
        for text in texts:
            feats = ar.parse_bed(text)
            for contig in list(feats) + ["chrAbsent"]:
                s, e, lab = ar.table_arrays(feats.get(contig, []), label)
                a = [int(r[1]) for r in ot if r[0] == contig] if label is ar.func_label else []
                b = [int(r[1]) + len(r[4]) for r in ot if r[0] == contig] if label is ar.func_label else []
                _check(s, e, lab, qs + a, qe + b)


@pytest.mark.parametrize("n,nq", [(0, 0), (0, 1), (1, 0), (1, 1), (0, 5), (3, 0)])
def test_empty_and_single(n, nq):
    got, _ = _check([10] * n, [20] * n, ["f"] * n, [15] * nq, [16] * nq)
    assert len(got) == nq


def test_empty_labels():
    """A label may have no bytes (the table's offsets only have to be non-decreasing).  The row is the join of the overlapping
    labels whatever their length - one overlap with an empty label gives the empty row, '' then 'x' gives ',x' - and NA only
    when nothing overlaps, as the reference's `",".join(...) if annotation else "NA"` tests the list, not the text."""
    got, _ = _check([10], [20], [""], [15, 30], [16, 31])  # single overlap, and the row behind it
    assert got.strings() == ["", "NA"]
    got, _ = _check([10, 12], [20, 22], ["", "x"], [15, 10, 21], [16, 11, 22])  # leading empty label
    assert got.strings() == [",x", "", "x"]
    got, _ = _check([10, 12, 14], [20, 22, 24], ["x", "", "y"], [15, 30], [16, 31])
    assert got.strings() == ["x,,y", "NA"]
    got, nov = _check([10, 11, 12], [20, 21, 22], ["", "", ""], [15, 0, 20, 21], [16, 5, 21, 22])  # all empty, last row too
    assert got.strings() == [",,", "NA", ",", ""] and nov == 6
    rng = np.random.default_rng(3)
    starts = np.sort(rng.integers(0, 3000, 300))
    ends = starts + rng.integers(1, 200, 300)
    labels = [("" if rng.random() < 0.5 else f"l{i % 5}") for i in range(300)]
    qs = np.sort(rng.integers(0, 3200, 700))
    _check(starts, ends, labels, qs, qs + 23, ar.join_rows_np)


def test_coordinates_at_zero_and_beyond_2_31():
    big = 1 << 33
    starts = [0, 0, 5, (1 << 31) - 1, 1 << 31, big, big + 10]
    ends = [1, big + 5, 6, (1 << 31) + 1, (1 << 31) + 2, big + 1, big + 20]
    labels = ["zero", "span", "five", "edge", "past", "big", "bigger"]
    qs = [0, 0, 1, (1 << 31) - 1, 1 << 31, big, big + 1, big + 19, big + 20, 1 << 40]
    qe = [1, 0, 5, 1 << 31, (1 << 31) + 1, big + 1, big + 12, big + 20, big + 30, (1 << 40) + 1]
    _check(starts, ends, labels, qs, qe)


def test_every_relative_position_of_query_and_feature():
    """a 10-base feature and queries of 1..14 bases from 2 bases before it to 2 bases after it, both ends: exactly the queries
    with fs < qe and fe > qs name it (touching at one base counts, abutting does not)"""
    fs, fe = 100, 110
    qs, qe = [], []
    for a in range(fs - 16, fe + 3):
        for b in range(a + 1, fe + 17):
            if a >= fs - 2 - 14 and b <= fe + 2 + 14:
                qs.append(a)
                qe.append(b)
    got, nov = _check([fs], [fe], ["F"], qs, qe)
    assert nov == sum(1 for a, b in zip(qs, qe) if fs < b and fe > a)
    rows = got.strings()
    at = {(a, b): r for a, b, r in zip(qs, qe, rows)}
    assert at[(fs - 2, fs)] == "NA" and at[(fs - 2, fs + 1)] == "F" and at[(fe - 1, fe + 2)] == "F" and at[(fe, fe + 2)] == "NA"
    # and the mirror: one query, features at every offset
    starts = list(range(80, 125))
    for w in (1, 2, 10):
        _check(starts, [s + w for s in starts], [f"w{w}_{s}" for s in starts], [100, 100, 99], [110, 101, 112])


def _assert_blocks_are_skipped(starts, ends, labels, n):
    """One query on the last short feature under the contig-long first one: the walk starts at feature 0 and ends behind
    feature n - 1.  It may test every feature of the first block (the long one makes its maximum large: 64 steps) and of the
    last block, and must take ONE step for each whole block in between, not one per feature.  A query abutting a block whose maximum equals its start (`<=`, not `<`) is held to the same bound."""
    lb, lo = ar.ragged(labels)
    tab = bedannot.AnnotTable(np.asarray(starts, np.int64), np.asarray(ends, np.int64), lb, lo)
    try:
        for qs in (starts[n - 1], ends[n - 2] if n > 2 else starts[n - 1]):  # on the last feature; abutting the one before it
            tab.query(np.array([qs], np.int64), np.array([starts[n - 1] + 1], np.int64))
            bound = min(64, n) + max((n - 1) // 64 - 1, 0) + ((n - 1) % 64 + 1 if n > 64 else 0)  # first block, one per whole block, last block
            assert tab.timing["walk_steps"] <= bound, (n, tab.timing["walk_steps"], bound)
            if n >= 4095:
                assert tab.timing["walk_steps"] < n // 8
    finally:
        tab.close()


@pytest.mark.parametrize("n", [63, 64, 65, 4095, 4096, 4097])
def test_block_seams_of_the_skip(n):
    """short features 10 bases apart under one long first feature (so every walk starts at 0 and has to skip whole 64-blocks):
    queries that match only the last feature of a block, only the first of the next, and the last feature of all"""
    starts = [0] + [100 + 10 * i for i in range(n - 1)]
    ends = [10 ** 7] + [s + 5 for s in starts[1:]]
    labels = ["long"] + [f"s{i}" for i in range(1, n)]
    qs, qe = [], []
    probe = sorted({63, 64, 65, 127, 128, n - 2, n - 1} & set(range(1, n)))
    for i in probe:
        qs += [starts[i], starts[i] + 4, starts[i] - 5]
        qe += [starts[i] + 1, starts[i] + 5, starts[i]]
    got, _ = _check(starts, ends, labels, qs, qe)
    _assert_blocks_are_skipped(starts, ends, labels, n)
    assert got.strings()[:3] == [f"long,s{probe[0]}", f"long,s{probe[0]}", "long"]
    # without the long feature: lo is found by the running maximum alone
    _check(starts[1:], ends[1:], labels[1:], qs, qe)


def test_contig_long_feature_over_1e5_short_ones():
    rng = np.random.default_rng(5)
    n = 100_000
    starts = np.concatenate([[0], np.sort(rng.integers(0, 5_000_000, n))]).astype(np.int64)
    ends = starts + np.concatenate([[6_000_000], rng.integers(1, 300, n)])
    labels = ["chrom"] + [f"e{i % 977}" for i in range(n)]
    qs = np.sort(rng.integers(0, 5_000_000, 3000))
    qe = qs + 23
    got, _ = _check(starts, ends, labels, qs, qe, ar.join_rows_np)
    assert all(r.startswith("chrom") for r in got.strings())


def test_thousand_identical_features_under_one_query():
    n = 1000
    got, nov = _check([50] * n, [60] * n, [f"same{i % 3}" for i in range(n)], [55, 0, 59, 60], [56, 50, 70, 61])
    assert nov == 2 * n and got.strings()[1] == "NA"


@pytest.mark.parametrize("nq", [1, 255, 256, 257, 2047, 2048, 2049])
def test_batch_sizes(nq):
    rng = np.random.default_rng(nq)
    starts = np.sort(rng.integers(0, 20000, 500))
    ends = starts + rng.integers(1, 400, 500)
    qs = rng.integers(0, 21000, nq)  # unsorted on purpose: order is a matter of speed alone
    _check(starts, ends, [f"L{i}" for i in range(500)], qs, qs + rng.integers(1, 40, nq), ar.join_rows_np)


def test_million_random_queries_on_1e5_features():
    """10^6 queries x 10^5 features: the brute force runs on a window of the sorted features per chunk of sorted queries (every
    feature outside the window starts behind the chunk or ends - by the running maximum - in front of it), every pair inside
    the window is tested.  The window is found the way the kernel finds its bounds, so for `lo` / `hi` this test is not
    independent of the kernel: it rests on the smaller tests above, which take the full cross product."""
    rng = np.random.default_rng(77)
    n, nq = 100_000, 1_000_000
    starts = np.sort(rng.integers(0, 50_000_000, n)).astype(np.int64)
    ends = starts + rng.integers(1, 2000, n)
    labels = np.array([f"c{i % 4099}" for i in range(n)], dtype=object)
    qs = np.sort(rng.integers(0, 50_000_000, nq)).astype(np.int64)
    qe = qs + 23
    lb, lo = ar.ragged(labels.tolist())
    tab = bedannot.AnnotTable(starts, ends, lb, lo)
    got = tab.query(qs, qe)
    tab.close()
    rmax = np.maximum.accumulate(ends)
    rows = []
    for c in range(0, nq, 4096):
        a, b = qs[c:c + 4096], qe[c:c + 4096]
        lo_i = int(np.searchsorted(rmax, a.min(), side="right"))
        hi_i = int(np.searchsorted(starts, b.max(), side="left"))
        s_, e_, l_ = starts[lo_i:hi_i], ends[lo_i:hi_i], labels[lo_i:hi_i]
        m = (s_[None, :] < b[:, None]) & (e_[None, :] > a[:, None])
        for r in m:
            idx = np.flatnonzero(r)
            rows.append(",".join(l_[idx]) if len(idx) else "NA")
    wb, wo = ar.ragged(rows)
    assert np.array_equal(got.off, wo) and np.array_equal(got.blob, wb)


# ---------------------------------------------------------------------------------------------------- end to end
def _files(fx, tmp_path, unphased=False):
    fa, bed, vcf = str(tmp_path / "g.fa"), str(tmp_path / "r.bed"), str(tmp_path / "v.vcf")
    readers.write_fasta(fa, fx["contig"], fx["genome"][fx["contig"]], 60)
    with open(bed, "w") as f:
        f.write(f"{fx['contig']}\t{fx['bed_start']}\t{fx['bed_stop']}\n")
    sep = "/" if unphased else "|"
    rows = [[fx["contig"], str(p), ".", r, a, ".", "PASS", f"AF={af:.6g}", "GT"] + [f"{g[0]}{sep}{g[1]}" for g in gts]
            for p, r, a, af, gts in fx["variants"]]
    readers.write_vcf(vcf, fx["contig"], fx["samples"], rows, False)
    func, gene = [], []
    for k, t in enumerate(fx["annotation_files"]):
        p = str(tmp_path / f"f{k}.bed")
        if k == 0:
            readers.write_bgzf(p + ".gz", t.encode())  # one of the files as BGZF
            p += ".gz"
        else:
            open(p, "w").write(t)
        func.append(p)
    for k, t in enumerate(fx["gene_annotation_files"]):
        p = str(tmp_path / f"g{k}.bed")
        open(p, "w").write(t)
        gene.append(p)
    ann = dict(annotations=func, annotation_colnames=fx["annotation_colnames"] or None, gene_annotations=gene,
               gene_annotation_colnames=fx["gene_annotation_colnames"] or None)
    return fa, bed, vcf, ann


def _ann_names(fx):
    return reports.annotation_colnames(len(fx["annotation_files"]), fx["annotation_colnames"], len(fx["gene_annotation_files"]),
                                       fx["gene_annotation_colnames"])


def _same_report(got_text, want_text, names, skip=()):
    """The two TSVs column for column: `==` everywhere except that a cell of an annotation column with more than one label is
    compared as a set - the reference joins such a cell in Python's set order, which changes with the interpreter's hash seed -
    and must list, here, its labels once each."""
    import pandas as pd
    got = pd.read_csv(io.StringIO(got_text), sep="\t", dtype=str, keep_default_na=False)
    want = pd.read_csv(io.StringIO(want_text), sep="\t", dtype=str, keep_default_na=False)
    assert list(got.columns) == list(want.columns) and len(got) == len(want)
    for c in got.columns:
        if c in skip:
            continue
        if c in names:
            for g, w in zip(got[c].tolist(), want[c].tolist()):
                if "," in w:
                    assert set(g.split(",")) == set(w.split(",")) and len(g.split(",")) == len(set(w.split(","))), (c, g, w)
                else:
                    assert g == w, (c, g, w)
        else:
            assert (got[c] == want[c]).all(), c
    return got


def _canon(text, names):
    """the TSV with every annotation cell's labels sorted: byte-for-byte comparison up to the reference's set order"""
    lines = text.splitlines()
    head = lines[0].split("\t")
    idx = [head.index(n) for n in names]
    out = [lines[0]]
    for ln in lines[1:]:
        f = ln.split("\t")
        for i in idx:
            f[i] = ",".join(sorted(f[i].split(",")))
        out.append("\t".join(f))
    return "\n".join(out) + "\n"


@pytest.mark.parametrize("case,forced_fallback", [("ngg", False), ("cpf1", False), ("ngg", True)])
def test_search_files_phased_matches_reference(tmp_path, monkeypatch, case, forced_fallback):
    """Plan-view route and host-built phased route: G11's guide report byte for byte up to the order of labels inside a cell
    (see _same_report), the off-targets table's rows byte for byte (the order among equal (chrom, position) is the scan's,
    as in test_search_files_with_estimate_offtargets); the same call without annotation arguments writes the same files minus
    the annotation columns."""
    fx = G11[case]
    fa, bed, vcf, ann = _files(fx, tmp_path)
    if forced_fallback:
        from crisprhawk_hip.expand import HaplotypeBuildError

        def refuse(*a, **k):
            raise HaplotypeBuildError("a chromosome copy carries overlapping variants")
        monkeypatch.setattr(pipeline, "expand_from_vcf", refuse)
    names = _ann_names(fx)
    kw = dict(cfd_tables=synth.cfd_tables() if fx["cfd"] else None)
    ot_kw = dict(kw, cfd_tables=synth.cfd_tables(), estimate_offtargets=fx["genome"], mm=fx["mm"])
    out = tmp_path / "out"
    timings = {}
    (path,) = pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(out), timings=timings,
                                    **(ot_kw if fx["report_with_offtargets"] else kw), **ann).values()
    got = open(path).read()
    _same_report(got, fx["report_tsv"], names)
    assert _canon(got, names) == _canon(fx["report_tsv"], names)
    assert pipeline.ANN_STAGE in timings and "open annotation BED files" in timings
    if not fx["report_with_offtargets"]:  # Cpf1: the reference cannot write the report with off-targets on; the table comes from its own call
        pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(out), **ot_kw, **ann)
    ot_path = out / f"offtargets_{fx['contig']}_{fx['bed_start']}_{fx['bed_stop']}.tsv"
    got_ot = ot_path.read_text()
    assert got_ot.splitlines()[0] == fx["offtargets_tsv"].splitlines()[0]
    assert sorted(got_ot.splitlines()) == sorted(fx["offtargets_tsv"].splitlines())
    keys = [tuple(r.split("\t")[:2]) for r in got_ot.splitlines()[1:]]
    assert keys == sorted(keys, key=lambda k: (k[0], int(k[1])))
    # without the annotation arguments: today's files = these files minus the annotation columns
    out2 = tmp_path / "plain"
    (p2,) = pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(out2), **ot_kw).values()
    plain = [ln.split("\t") for ln in open(p2).read().splitlines()]
    (pa,) = pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "ann2"), **ot_kw, **ann).values()
    full = [ln.split("\t") for ln in open(pa).read().splitlines()]
    keep = [i for i, h in enumerate(full[0]) if h not in names]
    assert [[r[i] for i in keep] for r in full] == plain
    ot2 = (out2 / ot_path.name).read_text().splitlines()
    assert sorted("\t".join(ln.split("\t")[:11]) for ln in got_ot.splitlines()) == sorted(ot2)


def test_search_files_unphased_matches_reference(tmp_path):
    """column for column, haplotype ids matched by count as G7's unphased test does"""
    fx = G11["unphased"]
    fa, bed, vcf, ann = _files(fx, tmp_path, unphased=True)
    (path,) = pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "out"),
                                    cfd_tables=synth.cfd_tables(), **ann).values()
    got = _same_report(open(path).read(), fx["report_tsv"], _ann_names(fx), skip=("haplotype_id",))
    import pandas as pd
    want = pd.read_csv(io.StringIO(fx["report_tsv"]), sep="\t", dtype=str, keep_default_na=False)
    assert (got["haplotype_id"].str.count(",") == want["haplotype_id"].str.count(",")).all()


def test_report_offtargets_and_ann_guides_take_annotations(tmp_path):
    """the refusal is gone: report_offtargets(annotations=[...]) writes G11's table; ann_guides fills funcann / geneann"""
    from crisprhawk_hip import offtargets as ot_mod
    from crisprhawk_hip.annotation import ann_guides
    from crisprhawk_hip.coordinate import Coordinate
    from crisprhawk_hip.guide import Guide
    from crisprhawk_hip.pam import PAM
    fx = G11["ngg"]
    _, _, _, ann = _files(fx, tmp_path)
    pam = PAM(fx["pam"], fx["right"], True)
    pam.encode(0)
    from crisprhawk_hip import scoring
    scoring.set_cfd_tables(*synth.cfd_tables())
    region = Coordinate(fx["contig"], fx["bed_start"], fx["bed_stop"], 100)
    tf = str(tmp_path / "x.targets.txt")
    open(tf, "w").write(fx["targets_txt"])
    ot_mod.report_offtargets(tf, region, pam, fx["guidelen"], ann["annotations"], ann["annotation_colnames"], False, fx["right"], str(tmp_path), 0, True)
    got = (tmp_path / f"offtargets_{fx['contig']}_{fx['bed_start']}_{fx['bed_stop']}.tsv").read_text()
    assert got == fx["offtargets_tsv"]  # same input file order, same stable sort: byte for byte
    iv = fx["guide_intervals"][:20]
    L = fx["guidelen"] + 3 + 20
    guides = [Guide(s, e, "A" * L, fx["guidelen"], 3, 0, True, False, "REF", "NA", {}, [], "hap_0") for s, e in iv]
    for files, atype, label in ((ann["annotations"], 0, ar.func_label), (ann["gene_annotations"], 1, ar.gene_label)):
        ann_guides(guides, fx["contig"], files, atype, 0, True)
        texts = fx["annotation_files"] if atype == 0 else fx["gene_annotation_files"]
        for k, text in enumerate(texts):
            feats = ar.parse_bed(text).get(fx["contig"], [])
            want = ar.join_rows(*ar.table_arrays(feats, label), [s for s, _ in iv], [e for _, e in iv])
            assert [(g.funcann if atype == 0 else g.geneann)[k] for g in guides] == want


def test_tiled_report_equals_one_piece_with_annotations():
    """MergedGroups.groups() feeds reports.group_columns: a tiled report is annotated once, on the merged groups, and equals
    the one-piece device report with the same annotation (haplotype ids aside, as in test_gpu_tiling)"""
    from crisprhawk_hip.pam import PAM
    from crisprhawk_hip.tiling import TiledRegionSearch, VariantPanel
    from crisprhawk_hip.workload import expand_on_device, row_labels
    reg = synth.make_region(4471, "chrU", 30_000, 1_000, 27_000)
    synth.add_phased_variants(reg, 4472, 500, 6, frac_snv=0.6, frac_del=0.2, af_min=0.2, af_max=0.6)
    pam = PAM("NGG", False, True)
    pam.encode(0)
    mm, pt = synth.cfd_tables()
    rng = np.random.default_rng(9)
    fs = np.sort(rng.integers(500, 28_000, 400)).astype(np.int64)
    fe = fs + rng.integers(1, 900, 400)
    labels = [f"r{i % 7}" for i in range(400)]
    tab_a = bedannot.AnnotTable(fs, fe, *ar.ragged(labels))
    calls = []

    def annotate(starts, stops):
        calls.append(len(starts))
        return {"regions": tab_a.query(starts, stops)}
    ds, info, _ms, kept = expand_on_device(reg, 3)
    tab = ds.search(pam.bits, pam.bitsrc, 3, 20, False, mm, pt, download=False, collapse=True)
    target = f"{reg.contig}:{reg.bed_start}-{reg.bed_stop}"
    df1 = reports.report_frame(reports.ReportInput.from_table(tab), row_labels(reg, ds, info, kept), pam, reg.contig, target, annotations=annotate)
    trs = TiledRegionSearch(lambda lo, hi: reg.contig_seq[lo - 1:hi], reg.contig, reg.startp, reg.stopp, VariantPanel.from_region(reg),
                            pam, 20, False, tile_nt=2600, flank=300)
    mg = trs.run(cfd=(mm, pt))
    assert len(trs.tiles) >= 8
    calls.clear()
    df3 = reports.report_from_groups(mg.groups(), mg.labels, pam, reg.contig, target, annotations=annotate)
    assert calls == [len(df3)]  # one join, over the merged groups
    tab_a.close()
    cols = [c for c in df1.columns if c != "haplotype_id"]
    assert "regions" in cols and len(df1) == len(df3) and len(df1) > 1000
    assert df1[cols].to_csv(sep="\t", index=False) == df3[cols].to_csv(sep="\t", index=False)
    want = ar.join_rows_np(fs, fe, labels, df3["start"].to_numpy(), df3["stop"].to_numpy())
    assert [set(x.split(",")) for x in df3["regions"]] == [set(x.split(",")) for x in want] and (df3["regions"] != "NA").any()
