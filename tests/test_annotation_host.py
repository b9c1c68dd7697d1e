"""BED / gene annotation, host side: the reader, the labels, the refusals, column names and order, argument checks - and the
brute-force yardstick (tests/annot_refs.py) held to the reference-generated fixture G11 (tests/golden/make_golden_annotation.py:
the reference's own annotate / report / off-target code over a brute-force stand-in for pysam.TabixFile).  The overlap rule is
tabix's documented half-open rule on both sides: parity unpinned, pysam absent."""
import gzip
import io
import os

import numpy as np
import pytest

import annot_refs as ar
from util import load_golden

from crisprhawk_hip import bedannot, pipeline, readers, reports
from crisprhawk_hip.crisprhawk_error import CrisprHawkAnnotationError
from crisprhawk_hip.pam import PAM

G11 = load_golden("g11_annotation.json.gz")
CASES = ["ngg", "cpf1", "unphased"]


def _pam(seq, right):
    p = PAM(seq, right, True)
    p.encode(0)
    return p


def _report(fx):
    import pandas as pd
    return pd.read_csv(io.StringIO(fx["report_tsv"]), sep="\t", dtype=str, keep_default_na=False)


def _names(fx):
    return reports.annotation_colnames(len(fx["annotation_files"]), fx["annotation_colnames"], len(fx["gene_annotation_files"]),
                                       fx["gene_annotation_colnames"])


@pytest.mark.parametrize("case", CASES)
def test_brute_force_reproduces_the_reference_report_columns(case):
    """Every annotation cell of G11's guide report = the brute-force row of (start, stop), as a set of labels (the reference's
    collapse joins a cell in set order); single-label and NA cells byte for byte.  Column names and their place too."""
    fx = G11[case]
    df = _report(fx)
    names = _names(fx)
    head = list(df.columns)
    at = head.index("af") + 1
    assert head[at:at + len(names)] == names
    assert head == reports.select_reportcols(_pam(fx["pam"], fx["right"]), fx["right"], fx["report_with_offtargets"], names)
    texts = [(t, ar.func_label) for t in fx["annotation_files"]] + [(t, ar.gene_label) for t in fx["gene_annotation_files"]]
    qs, qe = df["start"].astype(int).tolist(), df["stop"].astype(int).tolist()
    multi = 0
    for name, (text, label) in zip(names, texts):
        feats = ar.parse_bed(text).get(fx["contig"], [])
        want = ar.join_rows(*ar.table_arrays(feats, label), qs, qe)
        for got, w in zip(df[name].tolist(), want):
            assert ar.dedup(got) == ar.dedup(w)
            assert len(got.split(",")) == len(ar.dedup(w))  # listed once
            if len(ar.dedup(w)) == 1:
                assert got == w.split(",")[0]
            multi += len(ar.dedup(w)) > 1
    assert multi > 0


@pytest.mark.parametrize("case", ["ngg", "cpf1"])
def test_brute_force_reproduces_the_reference_offtargets_columns(case):
    """offtargets_*.tsv of G11: one column per functional file behind `elevation`, row = brute force of (chrom, position,
    position + len(spacer)), byte for byte (no collapse here: file order, duplicates kept)."""
    fx = G11[case]
    lines = fx["offtargets_tsv"].splitlines()
    head = lines[0].split("\t")
    names = fx["annotation_colnames"] or [f"annotation_{i + 1}" for i in range(len(fx["annotation_files"]))]
    assert head[11:] == names
    rows = [ln.split("\t") for ln in lines[1:]]
    hits = 0
    for k, text in enumerate(fx["annotation_files"]):
        feats = ar.parse_bed(text)
        for r in rows:
            f = feats.get(r[0], [])
            (want,) = ar.join_rows(*ar.table_arrays(f, ar.func_label), [int(r[1])], [int(r[1]) + len(r[4])])
            assert r[11 + k] == want
            hits += want != "NA"
    assert hits > 0


@pytest.mark.parametrize("how", ["plain", "gzip", "bgzf"])
def test_reader_plain_gzip_bgzf(tmp_path, how):
    fx = G11["ngg"]
    text = "#comment\ntrack name=x\nbrowser position chrA:1-2\n\n" + fx["gene_annotation_files"][0]
    path = str(tmp_path / ("a.bed" if how == "plain" else "a.bed.gz"))
    if how == "plain":
        open(path, "w").write(text)
    elif how == "gzip":
        with gzip.open(path, "wb") as f:
            f.write(text.encode())
    else:
        readers.write_bgzf(path, text.encode(), block=700)
    bed = bedannot.BedAnnotation(path, 0, True)
    feats = ar.parse_bed(text)
    assert bed.contigs == list(feats)
    for kind, label in ((bedannot.FUNC, ar.func_label), (bedannot.GENE, ar.gene_label)):
        for c, f in feats.items():
            s, e, blob, off = bed.features(c, kind)
            ws, we, wl = ar.table_arrays(f, label)
            assert s.tolist() == ws and e.tolist() == we and s.dtype == np.int64 and off.dtype == np.uint64
            wb, wo = ar.ragged(wl)
            assert np.array_equal(blob, wb) and np.array_equal(off, wo)
    s, e, blob, off = bed.features("chrNone", bedannot.FUNC)
    assert len(s) == 0 and len(e) == 0 and len(blob) == 0 and off.tolist() == [0]
    assert bed.fetch_features("chrNone", 0, 10) is None
    c = fx["contig"]
    (s0, e0, f0) = feats[c][2]
    assert bed.fetch_features(c, s0, s0 + 1) == ["\t".join(f[2]) for f in feats[c] if f[0] < s0 + 1 and f[1] > s0]


def test_gene_name_cases():
    assert bedannot.gene_name("gene_id=G1;gene_name=ABC1;level=2") == "ABC1"
    assert bedannot.gene_name("gene_id=G2;gene_name=XYZ9") == "XYZ"  # last attribute, no ';': the reference's slice drops a character
    assert bedannot.gene_name("gene_id=G3;level=1") == ""
    assert bedannot.gene_name("gene_name=LONE;") == "LONE"
    for a in ("gene_id=G1;gene_name=ABC1;level=2", "gene_id=G2;gene_name=XYZ9", "gene_id=G3;level=1", "gene_name=LONE;"):
        assert ar.gene_label(["c", "0", "1", "n", "0", "+", "s", "exon", ".", a]) == f"exon:{bedannot.gene_name(a)}"


def test_the_three_refusals(tmp_path):
    def bed(text):
        p = str(tmp_path / "x.bed")
        open(p, "w").write(text)
        return p
    with pytest.raises(CrisprHawkAnnotationError):  # not sorted by start within a contig
        bedannot.BedAnnotation(bed("c\t10\t20\ta\nc\t5\t8\tb\n"), 0, True)
    with pytest.raises(CrisprHawkAnnotationError):  # end < start
        bedannot.BedAnnotation(bed("c\t10\t9\ta\n"), 0, True)
    three = bedannot.BedAnnotation(bed("c\t1\t5\n"), 0, True)
    with pytest.raises(CrisprHawkAnnotationError):  # 4 columns for the functional label
        three.features("c", bedannot.FUNC)
    four = bedannot.BedAnnotation(bed("c\t1\t5\tname\n"), 0, True)
    assert four.features("c", bedannot.FUNC)[2].tobytes() == b"name"
    with pytest.raises(CrisprHawkAnnotationError):  # 10 for the gene label
        four.features("c", bedannot.GENE)
    ok = bedannot.BedAnnotation(bed("c\t3\t3\tempty\nc\t3\t9\tb\nd\t1\t2\tz\nc\t9\t12\tlater\n"), 0, True)  # equal starts, end == start, contigs interleaved
    assert ok.features("c")[0].tolist() == [3, 3, 9]


@pytest.mark.parametrize("pam_s,right", [("NGG", False), ("NGN", False), ("TTTV", True), ("NNGRRT", False)])
@pytest.mark.parametrize("n_func,n_gene", [(0, 0), (1, 0), (2, 0), (0, 1), (0, 2), (2, 1), (1, 2)])
@pytest.mark.parametrize("named", [False, True])
@pytest.mark.parametrize("ot", [False, True])
def test_column_names_and_order(pam_s, right, n_func, n_gene, named, ot):
    """select_reportcols: the annotation columns - the caller's names or annotation_{i} / gene_annotation_{i}, functional files
    first - behind `af`, in front of `offtargets` / `cfd`, `target` and `haplotype_id` (reports.py:352-381, 612-660)."""
    pam = _pam(pam_s, right)
    names = reports.annotation_colnames(n_func, [f"F{i}" for i in range(n_func)] if named else None, n_gene,
                                        [f"G{i}" for i in range(n_gene)] if named else None)
    want = ([f"F{i}" for i in range(n_func)] + [f"G{i}" for i in range(n_gene)]) if named else \
        ([f"annotation_{i + 1}" for i in range(n_func)] + [f"gene_annotation_{i + 1}" for i in range(n_gene)])
    assert names == want
    cols = reports.select_reportcols(pam, right, ot, names)
    base = reports.select_reportcols(pam, right, ot)
    assert [c for c in cols if c not in names] == base
    at = cols.index("af") + 1
    assert cols[at:at + len(names)] == names
    assert cols[-2:] == ["target", "haplotype_id"]
    if ot:
        assert cols[at + len(names)] == "offtargets"


def test_dedup_labels_keeps_first_occurrence_order():
    col = reports.Ragged.from_strings(["NA", "a", "b,a,b", "a,a", "x,y,z", ""])
    assert reports.dedup_labels(col).strings() == ["NA", "a", "b,a", "a", "x,y,z", ""]
    same = reports.Ragged.from_strings(["NA", "a", "x,y"])
    assert reports.dedup_labels(same) is same


def test_search_files_argument_checks(tmp_path):
    """crisprhawk_argparse.py:252-330, raised before any input is opened or the library is needed."""
    good = str(tmp_path / "a.bed")
    open(good, "w").write("c\t1\t5\tx\n")
    empty = str(tmp_path / "e.bed")
    open(empty, "w").close()
    call = lambda **kw: pipeline.search_files("no.fa", "no.bed", [], "NGG", 20, False, str(tmp_path / "out"), **kw)
    for kw in (dict(annotation_colnames=["a"]), dict(gene_annotation_colnames=["g"]), dict(annotations=[good], annotation_colnames=["a", "b"]),
               dict(gene_annotations=[good, good], gene_annotation_colnames=["g"]), dict(annotations=[str(tmp_path / "missing.bed")]),
               dict(annotations=[empty]), dict(gene_annotations=[empty])):
        with pytest.raises(ValueError):
            call(**kw)
    assert not os.path.exists(tmp_path / "out")
