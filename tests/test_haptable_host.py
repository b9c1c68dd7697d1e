"""The host half of the haplotypes table (haplotypes.haplotypes_table, the reference's haplotypes.py:818-859): the writer on
hand-made rows, the file name, the planner that cuts a plan's rows into batches of whole rows under a byte budget, and the
refusals.  Nothing here touches a device; tests/test_gpu_haptext.py covers the text kernel and the pipeline."""
import inspect
import os

import numpy as np
import pytest

from crisprhawk_hip import haplotypes as H

HEADER = "id\thaplotype\tvariants\tsamples\n"


def test_writer_writes_header_and_lines_exactly(tmp_path):
    """rows handed over as two chunks (one buffer holding two rows back to back, one holding the third behind a gap the offsets
    skip), labels as str and as bytes: the file is the header and one line per row, bytes as given, case included"""
    ids = ["hap_00000000", "hap_00000001", b"hap_00000002"]
    variants = ["NA", "chr1-101-A/G,chr1-140-CT/C", b"chr1-120-G/GAAT"]
    samples = ["REF", "S1:1|0,S2:0|1", "S3:1|1"]
    a = np.frombuffer(b"ACGTNACgTN", dtype=np.uint8)
    b = np.frombuffer(b"xxACGaatTN", dtype=np.uint8)
    path = H.write_haplotypes_table(str(tmp_path / "t.tsv"), ids, variants, samples,
                                    [(a, np.array([0, 5, 10], dtype=np.uint64)), (b, np.array([2, 10], dtype=np.uint64))])
    want = HEADER + "hap_00000000\tACGTN\tNA\tREF\n" + "hap_00000001\tACgTN\tchr1-101-A/G,chr1-140-CT/C\tS1:1|0,S2:0|1\n" \
        + "hap_00000002\tACGaatTN\tchr1-120-G/GAAT\tS3:1|1\n"
    assert open(path, "rb").read() == want.encode("ascii")


def test_writer_refuses_a_row_count_that_differs_from_the_labels(tmp_path):
    with pytest.raises(ValueError, match="1 sequences for 2 rows"):
        H.write_haplotypes_table(str(tmp_path / "t.tsv"), ["a", "b"], ["NA", "NA"], ["REF", "x"], [(b"ACGT", (0, 4))])


def test_table_from_host_sequences_and_its_file_name(tmp_path):
    """the routes that hold the strings on the host (a region without variants, the host-built haplotypes) use the same
    writer; the file is named as the reference names it, from the PADDED region's coordinates"""
    assert H.haplotypes_table_filename("chr7", 901, 2100) == "haplotypes_table_chr7_901_2100.tsv"
    assert H.HAPTABCNAMES == ["id", "haplotype", "variants", "samples"]
    path = H.haplotypes_table("chr7", 901, 2100, str(tmp_path), ["hap_00000000", "hap_00000001"], ["NA", "chr7-950-A/R"], ["REF", "S9"],
                              sequences=["ACGT", b"ACrT"])
    assert path == os.path.join(str(tmp_path), "haplotypes_table_chr7_901_2100.tsv")
    assert open(path).read() == HEADER + "hap_00000000\tACGT\tNA\tREF\n" + "hap_00000001\tACrT\tchr7-950-A/R\tS9\n"
    with pytest.raises(ValueError, match="rows of a plan or host sequences"):
        H.haplotypes_table("chr7", 901, 2100, str(tmp_path), [], [], [])


LENGTHS = [1000, 1003, 997, 1000, 5, 1000, 2500, 1]


@pytest.mark.parametrize("budget", [1, LENGTHS[0], LENGTHS[0] + 1, LENGTHS[0] + LENGTHS[1], sum(LENGTHS), sum(LENGTHS) + 1, 2500])
def test_batch_planner_whole_rows_in_order_under_the_budget(budget):
    batches = H.text_batches(LENGTHS, budget)
    assert all(b > a for a, b in batches), "an empty batch"
    assert [i for a, b in batches for i in range(a, b)] == list(range(len(LENGTHS))), "every row once, in order"
    for a, b in batches:
        assert b - a == 1 or sum(LENGTHS[a:b]) <= budget, "a batch of several rows beyond the budget"
    for (a, b), (c, _d) in zip(batches, batches[1:]):  # greedy: the next row did not fit any more
        assert sum(LENGTHS[a:b]) + LENGTHS[c] > budget
    if budget == 1:
        assert len(batches) == len(LENGTHS)
    if budget == LENGTHS[0]:
        assert batches[0] == (0, 1)
    if budget == LENGTHS[0] + 1:
        assert batches[0] == (0, 1), "one row + 1 byte does not hold two rows"
    if budget >= sum(LENGTHS):
        assert batches == [(0, len(LENGTHS))]


def test_batch_planner_edges():
    assert H.text_batches([], 100) == []
    assert H.text_batches([7], 1) == [(0, 1)]
    assert H.text_batches(np.array([3, 3, 3], dtype=np.uint32), 6) == [(0, 2), (2, 3)]


def test_batch_budget_argument_environment_default(monkeypatch):
    monkeypatch.delenv("HAWK_HAPTEXT_BATCH_BYTES", raising=False)
    assert H.text_batch_bytes() == 256 << 20
    monkeypatch.setenv("HAWK_HAPTEXT_BATCH_BYTES", "12345")
    assert H.text_batch_bytes() == 12345
    assert H.text_batch_bytes(77) == 77


def test_tiled_search_refuses_a_haplotypes_table():
    """haplotype identity is per tile there: no whole-region row set exists"""
    from crisprhawk_hip.tiling import TiledRegionSearch
    t = TiledRegionSearch(lambda lo, hi: "A" * (hi - lo + 1), "chr1", 1, 50_000, None, "NGG", 20, False, tile_nt=20_000)
    with pytest.raises(ValueError, match="per tile"):
        t.run(haplotype_table=True)


def test_search_files_keyword_is_appended_and_off_by_default():
    from crisprhawk_hip import pipeline
    params = list(inspect.signature(pipeline.search_files).parameters.values())
    names = [p.name for p in params]
    assert names[-2:] == ["haplotype_table", "tables"] and names[-3] == "gene_annotation_colnames"
    assert params[-2].default is False and params[-1].default is None


def test_library_exports_the_text_call():
    from crisprhawk_hip import _lib
    assert "hawk_xplan_text" in _lib.EXPORTS
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "hawk.h")).read()
    assert "int hawk_xplan_text(hawk_xplan* x, uint32_t n_rows, const uint32_t* rows, const uint64_t* out_off, char* out, float* kernel_ms);" in header
