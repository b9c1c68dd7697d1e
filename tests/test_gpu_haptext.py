"""The haplotypes table on the device path: hawk_xplan_text (k_hx_text, hawk_haptext.hip) turns the rows of an expansion plan
into the cased IUPAC strings the reference writes into haplotypes_table_*.tsv (haplotypes.py:818-859), and
haplotypes.haplotypes_table / pipeline.search_files(haplotype_table=True) write the file.  Expected strings are the
string-level oracle's (oracle.hap_build per chromosome copy, through the seam cases of tests/expansion_refs.py) and the
reference's own haplotypes stored in the g3 / g7 fixtures; every comparison is byte for byte."""
import ctypes as C
import functools
import hashlib
import os

import numpy as np
import pytest

import expansion_refs as xr
from crisprhawk_hip import _lib, haplotypes as H, synth
from crisprhawk_hip.hapset import _p
from crisprhawk_hip.workload import expand_on_device, row_labels
from oracle import oracle as ora
from util import G3_CASES, load_golden, oracle_haplotypes, synth_region_from_fixture

pytestmark = pytest.mark.gpu

SEAM_CASES = ["tile_seams", "word_seams", "allele_lengths", "record_capacity", "ref_window", "row_ends", "identity", "identity_wide",
              "rows_4096", "rows_4097"]
GUARD = 0xA5
HEADER = "id\thaplotype\tvariants\tsamples\n"


@functools.lru_cache(maxsize=None)
def _case(name):
    """a seam case and the oracle's string of every row of its plan (REF, then the chromosome copies that carry something, in
    column order), built once and shared"""
    case = xr.CASES[name]()
    assert all(any(frag in label for label in case.proved) for frag in xr.REQUIRED[name])
    want = [case.ref.encode("ascii")] + [case.row(si, c).seq.encode("ascii") for si, c in case.live_columns()]
    return case, want


def _plan(case):
    """the plan-building step of tests/test_gpu_expansion.py, restated: the case's region expanded on the device, plan kept"""
    ds, info, _ms, kept = expand_on_device(case.region(), case.pamlen, keep_plan=True)
    assert ds.plan is not None and ds.plan.n_hap == 1 + len(case.live_columns())
    return ds, info, kept


def _close(ds):
    ds.plan.close()
    ds.close()


def _first_difference(name, r, got, want):
    n = min(len(got), len(want))
    d = np.flatnonzero(np.frombuffer(got[:n], dtype=np.uint8) != np.frombuffer(want[:n], dtype=np.uint8))
    at = int(d[0]) if len(d) else n
    return (f"{name}: row {r} ({len(want)} bases, got {len(got)}) differs at position {at} (tile {at // xr.TILE}, word {at // 32}, bit {at % 32}): "
            f"got {got[max(at - 8, 0):at + 24]!r} want {want[max(at - 8, 0):at + 24]!r}")


# ---------------------------------------------------------------------------------------------------------------------------
# 1. seams
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SEAM_CASES)
def test_text_of_every_row_on_the_expansion_seams_against_the_oracle(name):
    case, want = _case(name)
    ds, _info, _kept = _plan(case)
    buf, off = ds.plan.text()
    assert len(off) == len(want) + 1 and int(off[0]) == 0 and int(off[-1]) == len(buf) == sum(len(w) for w in want)
    for r, w in enumerate(want):
        got = buf[int(off[r]):int(off[r + 1])].tobytes()
        if got != w:
            pytest.fail(_first_difference(name, r, got, w))
    _close(ds)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the reference's own haplotypes
# ---------------------------------------------------------------------------------------------------------------------------
def _signature(seq, variants, samples):
    """(g3 fixtures store a haplotype's samples as a sorted list, g7 fixtures as the reference's joined string)"""
    return (seq, frozenset(variants.split(",")), frozenset(samples.split(",") if isinstance(samples, str) else samples))


def _table_lines(path):
    text = open(path).read()
    assert text.startswith(HEADER) and text.endswith("\n")
    return [line.split("\t") for line in text[len(HEADER):].splitlines()]


def _check_against_fixture_haplotypes(lines, haplotypes):
    assert all(len(x) == 4 for x in lines) and len(lines) == len(haplotypes)
    got = sorted((_signature(seq, var, smp.split(",")) for _id, seq, var, smp in lines), key=repr)
    want = sorted((_signature(h["seq"], h["variants"], h["samples"]) for h in haplotypes), key=repr)
    assert got == want
    assert lines[0][1:] == [haplotypes[0]["seq"], "NA", "REF"] and haplotypes[0]["samples"] in (["REF"], "REF"), "REF is the first line"


def _fixture_haplotypes(fx):
    """the reference's haplotypes of a fixture; the phased g7 fixtures store the labels only (seq is null): their strings are
    the oracle's, rebuilt from the fixture's raw inputs in the reference's order as tests/test_reports.py pairs them"""
    haps = fx["haplotypes"]
    if all(h["seq"] is not None for h in haps):
        return haps
    built = oracle_haplotypes(fx)
    assert len(built) == len(haps)
    for h, b in zip(haps, built):
        assert sorted(h["samples"].split(",")) == b["samples"]
    return [dict(seq=b["seq"], variants=h["variants"], samples=h["samples"]) for h, b in zip(haps, built)]


def _table_of_fixture(fx, outdir, batch_bytes=None):
    reg = synth_region_from_fixture(fx)
    ds, info, _ms, kept = expand_on_device(reg, len(fx["pam"]), keep_plan=True)
    plan = getattr(ds, "plan", None)
    if plan is None:  # no variants: REF alone, the string is on the host
        assert not fx["variants"] and kept == [0]
        path = H.haplotypes_table(reg.contig, reg.startp, reg.stopp, outdir, ["hap_00000000"], ["NA"], ["REF"], sequences=[reg.sequence])
    else:
        labels = row_labels(reg, ds, info, kept)
        path = H.haplotypes_table(reg.contig, reg.startp, reg.stopp, outdir, [labels[r].id for r in kept], [labels[r].variants for r in kept],
                                  [labels[r].samples for r in kept], plan=plan, rows=kept, batch_bytes=batch_bytes)
        plan.close()
    ds.close()
    assert os.path.basename(path) == f"haplotypes_table_{fx['contig']}_{fx['startp']}_{fx['stopp']}.tsv"
    return path


@pytest.mark.parametrize("case", G3_CASES)
def test_table_of_the_reference_fixtures_holds_the_reference_haplotypes(tmp_path, case):
    fx = load_golden(f"g3_search_{case}.json.gz")
    lines = _table_lines(_table_of_fixture(fx, str(tmp_path)))
    _check_against_fixture_haplotypes(lines, fx["haplotypes"])
    assert len({x[0] for x in lines}) == len(lines), "ids are unique"


# ---------------------------------------------------------------------------------------------------------------------------
# 3. placement: any order, repeats, every alignment phase, nothing outside the rows' ranges
# ---------------------------------------------------------------------------------------------------------------------------
def _text_call(plan, rows, off, out, ms=None):
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    return _lib.lib().hawk_xplan_text(plan._x, C.c_uint32(len(rows)), _p(rows), _p(off), _p(out), ms)


def test_rows_land_where_asked_at_every_alignment_phase_and_nowhere_else():
    """row_ends: rows of one to two tiles and a bit (32k - 1, 32k, 32k + 1, 128k +- 1 ... bases), packed end to end, so a row's head
    and tail sit where the rows before it end; out_off[0] sweeps 0 .. 15, which takes every listed row's head and tail, and with
    them its tile starts, through every phase of the 16-byte grid (counted below, not assumed)"""
    case, want = _case("row_ends")
    ds, _info, _kept = _plan(case)
    n = len(want)
    heads, tails = {}, {}  # listed position / single row -> the phases its first and its one-past-last byte took
    listed = list(range(n - 1, -1, -1)) + [3, 3, 0, n - 1]  # reverse order, then repeats
    singles = [0, 1, n - 1]
    for phase in range(16):
        for rows in [listed] + ([[r] for r in singles] if phase in (0, 1, 15) else [[singles[phase % 3]]]):
            off = np.zeros(len(rows) + 1, dtype=np.uint64)
            off[0] = phase
            off[1:] = phase + np.cumsum([len(want[r]) for r in rows])
            out = np.full(int(off[-1]) + 64, GUARD, dtype=np.uint8)
            assert _text_call(ds.plan, rows, off, out) == _lib.HAWK_OK
            assert (out[:phase] == GUARD).all() and (out[int(off[-1]):] == GUARD).all(), (phase, rows, "bytes outside the rows' ranges")
            for i, r in enumerate(rows):
                got = out[int(off[i]):int(off[i + 1])].tobytes()
                if got != want[r]:
                    pytest.fail(f"phase {phase}, listed row {i}: " + _first_difference("row_ends", r, got, want[r]))
                if rows is listed:
                    heads.setdefault(i, set()).add(int(off[i]) % 16)
                    tails.setdefault(i, set()).add(int(off[i + 1]) % 16)
    _close(ds)
    assert len(heads) == len(listed) and all(heads[i] == tails[i] == set(range(16)) for i in range(len(listed)))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_buffer_untouched():
    case, want = _case("word_seams")
    ds, _info, _kept = _plan(case)
    n = len(want)
    lens = [len(w) for w in want]
    out = np.full(sum(lens[:3]) + 64, GUARD, dtype=np.uint8)
    good = np.concatenate(([0], np.cumsum(lens[:3]))).astype(np.uint64)
    bad_row = (np.array([0, n, 2]), good)                                        # a row index equal to n_hap
    short = (np.array([0, 1, 2]), good - np.array([0, 0, 1, 1], dtype=np.uint64))  # the second row one byte short
    long_ = (np.array([0, 1, 2]), good + np.array([0, 0, 0, 1], dtype=np.uint64))  # the last row one byte long
    descending = (np.array([0, 1, 2]), np.array([good[1], good[0], good[2], good[3]], dtype=np.uint64))
    for rows, off in (bad_row, short, long_, descending):
        assert _text_call(ds.plan, rows, off, out) == _lib.HAWK_E_INVALID
        assert (out == GUARD).all()
    ms = C.c_float(-1.0)
    assert _lib.lib().hawk_xplan_text(ds.plan._x, C.c_uint32(0), None, None, None, C.byref(ms)) == _lib.HAWK_OK and ms.value == 0.0
    assert _lib.lib().hawk_xplan_text(ds.plan._x, C.c_uint32(0), None, None, None, None) == _lib.HAWK_OK
    buf, off = ds.plan.text([])
    assert len(buf) == 0 and off.tolist() == [0]
    with pytest.raises(IndexError):
        ds.plan.text([n])
    assert _text_call(ds.plan, [0, 1, 2], good, out) == _lib.HAWK_OK and out[:int(good[-1])].tobytes() == b"".join(want[:3])  # and the good call goes through
    _close(ds)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the plan is only read
# ---------------------------------------------------------------------------------------------------------------------------
COLS = ("hap", "pos", "strand", "start", "stop", "flags")


def _table_digest(t):
    """the table in the reference's emission order (haplotype, strand, position), as columns and as one digest"""
    o = np.lexsort((t.pos, t.strand, t.hap))
    cols = {c: np.ascontiguousarray(getattr(t, c)[o]) for c in COLS}
    cols["win"] = np.ascontiguousarray(t.win[:, o])
    cols["cfdon"] = np.ascontiguousarray(t.cfdon[o])
    h = hashlib.blake2b(digest_size=16)
    for c in sorted(cols):
        h.update(cols[c].tobytes())
    return (t.n_rows, t.n_candidates, t.n_hits, h.hexdigest()), cols


@pytest.mark.parametrize("path", ["clusters", "words"])
def test_a_text_call_leaves_the_plan_as_it_was(monkeypatch, path):
    monkeypatch.setenv("HAWK_CLUSTER_MIN_SHARE", "0")
    if path == "words":
        monkeypatch.setenv("HAWK_VIEW_SEARCH", "words")
    else:
        monkeypatch.delenv("HAWK_VIEW_SEARCH", raising=False)
    case, want = _case("record_capacity")
    ds, _info, _kept = _plan(case)
    bits, bitsrc, _, _ = ora.pam_encode("NGG")
    mm, pt = synth.cfd_tables()
    view = ds.plan.view()
    before, cols_b = _table_digest(view.search(bits, bitsrc, 3, 20, False, mm, pt))
    buf, off = ds.plan.text()
    after, cols_a = _table_digest(view.search(bits, bitsrc, 3, 20, False, mm, pt))
    assert before == after and before[0] > 0
    for c in cols_b:
        assert np.array_equal(cols_b[c], cols_a[c], equal_nan=(c == "cfdon")), c
    assert buf.tobytes() == b"".join(want)
    buf2, _ = ds.plan.text()  # and a search between two text calls changes no text
    assert buf2.tobytes() == buf.tobytes()
    _close(ds)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. batch seams end to end
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_table_does_not_depend_on_the_batch_budget(tmp_path, monkeypatch):
    from crisprhawk_hip.hapset import ExpansionPlan
    fx = load_golden("g3_search_phased16.json.gz")
    lens = [len(h["seq"]) for h in fx["haplotypes"]]
    calls = []
    real = ExpansionPlan.text

    def counted(self, rows=None, timed=False):
        calls.append(len(rows))
        return real(self, rows, timed)
    monkeypatch.setattr(ExpansionPlan, "text", counted)
    texts, n_calls = [], []
    for k, budget in enumerate((min(lens) - 1, None, 1 << 62)):
        if budget is None:  # exactly the first two rows of the table (the kept rows are the fixture's haplotypes, in order)
            budget = lens[0] + lens[1]
        del calls[:]
        os.makedirs(str(tmp_path / f"b{k}"))
        path = _table_of_fixture(fx, str(tmp_path / f"b{k}"), batch_bytes=budget)
        texts.append(open(path, "rb").read())
        n_calls.append(list(calls))
    assert n_calls[0] == [1] * len(lens), "a budget below one row: one row per call"
    assert n_calls[1][0] == 2 and len(n_calls[1]) > 1 and sum(n_calls[1]) == len(lens)
    assert n_calls[2] == [len(lens)]
    assert texts[0] == texts[1] == texts[2]
    _check_against_fixture_haplotypes([x.split("\t") for x in texts[0].decode()[len(HEADER):].splitlines()], fx["haplotypes"])


def test_the_batch_budget_comes_from_the_environment(tmp_path, monkeypatch):
    from crisprhawk_hip.hapset import ExpansionPlan
    fx = load_golden("g3_search_phased4.json.gz")
    calls = []
    real = ExpansionPlan.text
    monkeypatch.setattr(ExpansionPlan, "text", lambda self, rows=None, timed=False: (calls.append(len(rows)), real(self, rows, timed))[1])
    monkeypatch.setenv("HAWK_HAPTEXT_BATCH_BYTES", "1")
    _table_of_fixture(fx, str(tmp_path))
    assert calls == [1] * len(fx["haplotypes"])


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the pipeline
# ---------------------------------------------------------------------------------------------------------------------------
def _write_inputs(fx, tmp_path, phased=True):
    from crisprhawk_hip import readers
    contig_seq = "N" * (fx["startp"] - 1) + fx["region_seq"] + "ACGT" * 10
    fa, bed, vcf = str(tmp_path / "g.fa"), str(tmp_path / "r.bed"), str(tmp_path / "v.vcf.gz")
    readers.write_fasta(fa, fx["contig"], contig_seq, 80)
    with open(bed, "w") as f:
        f.write(f"{fx['contig']}\t{fx['bed_start']}\t{fx['bed_stop']}\n")
    vcfs = []
    if fx["variants"]:
        sep = "|" if phased else "/"
        rows = [[fx["contig"], str(p), ".", r, a, ".", "PASS", f"AF={af:.6g}", "GT"] + [f"{g[0]}{sep}{g[1]}" for g in gts]
                for p, r, a, af, gts in fx["variants"]]
        readers.write_vcf(vcf, fx["contig"], fx["samples"], rows, True)
        vcfs = [vcf]
    return fa, bed, vcfs


def _report_ids(path):
    import pandas as pd
    df = pd.read_csv(path, sep="\t", dtype=str, keep_default_na=False)
    return {x for cell in df["haplotype_id"] for x in cell.split(",")}


@pytest.mark.parametrize("case", ["phased4", "phased16", "cpf1", "indel_dense", "sacas9"])
def test_search_files_writes_the_table_and_leaves_the_report_alone(tmp_path, case):
    from crisprhawk_hip import pipeline
    fx = load_golden(f"g7_report_{case}.json.gz")
    fa, bed, vcfs = _write_inputs(fx, tmp_path)
    cfd = synth.cfd_tables() if fx["cfd"] else None
    plain = pipeline.search_files(fa, bed, vcfs, fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "plain"), cfd_tables=cfd)
    assert os.listdir(str(tmp_path / "plain")) == [os.path.basename(next(iter(plain.values())))], "no table unless asked for"
    tables = {}
    paths = pipeline.search_files(fa, bed, vcfs, fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "out"), cfd_tables=cfd,
                                  haplotype_table=True, tables=tables)
    assert list(paths) == list(plain) == list(tables) and len(paths) == 1
    (report,), (table,), (report0,) = paths.values(), tables.values(), plain.values()
    assert open(report, "rb").read() == open(report0, "rb").read() == fx["report_tsv"].encode()
    assert table == os.path.join(str(tmp_path / "out"), f"haplotypes_table_{fx['contig']}_{fx['startp']}_{fx['stopp']}.tsv")
    lines = _table_lines(table)
    _check_against_fixture_haplotypes(lines, _fixture_haplotypes(fx))
    ids = [x[0] for x in lines]
    assert len(set(ids)) == len(ids)
    used = _report_ids(report)
    assert used and all(ids.count(i) == 1 for i in used), "every haplotype_id of the report is one line of the table"


def test_search_files_table_of_a_region_without_variants(tmp_path):
    from crisprhawk_hip import pipeline
    fx = load_golden("g3_search_c1.json.gz")
    assert not fx["variants"]
    fa, bed, vcfs = _write_inputs(fx, tmp_path)
    tables = {}
    paths = pipeline.search_files(fa, bed, vcfs, fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "out"), haplotype_table=True, tables=tables)
    (table,) = tables.values()
    assert os.path.basename(table) == f"haplotypes_table_{fx['contig']}_{fx['startp']}_{fx['stopp']}.tsv"
    assert open(table).read() == HEADER + f"hap_00000000\t{fx['region_seq']}\tNA\tREF\n"
    assert fx["haplotypes"][0]["seq"] == fx["region_seq"] and len(fx["haplotypes"]) == 1
    assert _report_ids(next(iter(paths.values()))) <= {"hap_00000000"}


def test_search_files_table_of_an_unphased_input_comes_from_the_host_route(tmp_path, monkeypatch):
    from crisprhawk_hip import pipeline
    from crisprhawk_hip.hapset import ExpansionPlan
    fx = load_golden("g7_report_unphased.json.gz")
    fa, bed, vcfs = _write_inputs(fx, tmp_path, phased=False)

    def no_kernel(self, rows=None, timed=False):
        raise AssertionError("the host route holds the strings: no text call")
    monkeypatch.setattr(ExpansionPlan, "text", no_kernel)
    tables = {}
    paths = pipeline.search_files(fa, bed, vcfs, fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "out"), cfd_tables=synth.cfd_tables(),
                                  haplotype_table=True, tables=tables)
    (table,), (report,) = tables.values(), paths.values()
    assert os.path.basename(table) == f"haplotypes_table_{fx['contig']}_{fx['startp']}_{fx['stopp']}.tsv"
    lines = _table_lines(table)
    _check_against_fixture_haplotypes(lines, _fixture_haplotypes(fx))
    ids = [x[0] for x in lines]
    assert all(ids.count(i) == 1 for i in _report_ids(report))


def test_host_built_fallback_of_a_phased_input_writes_the_same_table(tmp_path, monkeypatch):
    """records the device expansion declines go through the host builder: forced here on inputs the device does take, the table
    must hold the same haplotypes as the device route's"""
    from crisprhawk_hip import pipeline
    from crisprhawk_hip.expand import HaplotypeBuildError
    fx = load_golden("g7_report_indel_dense.json.gz")
    fa, bed, vcfs = _write_inputs(fx, tmp_path)

    def refuse(*a, **k):
        raise HaplotypeBuildError("a chromosome copy carries overlapping variants")
    monkeypatch.setattr(pipeline, "expand_from_vcf", refuse)
    tables = {}
    pipeline.search_files(fa, bed, vcfs, fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "out"), cfd_tables=synth.cfd_tables(),
                          haplotype_table=True, tables=tables)
    _check_against_fixture_haplotypes(_table_lines(next(iter(tables.values()))), _fixture_haplotypes(fx))
