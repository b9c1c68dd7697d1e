"""The gnomAD converter on the device (k_gn_scan, k_gn_text_len, k_gn_text_fill behind hawk_gnomad_*): the reference's output
(g13), the chunk and sweep seams of the scan, decoy keys, values, FILTER, AF, record counts, batches, and the host twin.
Every expected byte comes from tests/gnomad_refs.py or g13; every run asserts that the device engine ran (scan ms > 0)."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import gnomad_refs as refs
from crisprhawk_hip import _lib, converter, readers, synth
from crisprhawk_hip.coordinate import Coordinate
from crisprhawk_hip.crisprhawk_error import CrisprHawkConverterError
from test_gnomad_refs import G13, case_input

pytestmark = pytest.mark.gpu


def batch_of(lines, joint, keep, engine="device", ends=None):
    """one batch through the converter's own batch code: (lines blob as str or None, kept, failure, the _Batch)"""
    raw = "".join(ln + (ends[i] if ends else "\n") for i, ln in enumerate(lines)).encode()
    text = np.frombuffer(raw, np.uint8).copy()
    nl = np.flatnonzero(text == 10)
    line_off = np.zeros(len(nl) + 1, np.uint64)
    line_off[1:] = nl + 1
    b = converter._Batch(text, line_off, converter.format_ac(joint), keep, engine, 0)
    secs = {"float_pool": 0.0, "lines_call": 0.0}
    try:
        out, kept, failure = converter._convert_batch(b, 2, secs)
        out = None if out is None else bytes(out).decode()
    finally:
        b.close()
    if engine == "device":
        assert b.engine == "device" and b.ms["scan_ms"] > 0
    return out, kept, failure, b


def expected(lines, joint, keep):
    out = [refs.convert_line(ln, joint, keep) for ln in lines]
    return "".join(o + "\n" for o in out if o is not None)


def check(lines, joint=False, keep=True, ends=None):
    got, kept, failure, b = batch_of(lines, joint, keep, ends=ends)
    assert failure is None
    want = expected(lines, joint, keep)
    assert got == want and kept == want.count("\n")
    return b


# ------------------------------------------------------------------------------------------------ g13
@pytest.mark.parametrize("name", sorted(G13["cases"]))
def test_g13_byte_for_byte(tmp_path, name):
    case = G13["cases"][name]
    kind, text = case_input(case)
    p = tmp_path / kind["input_name"]
    readers.write_bgzf(str(p), text.encode())
    r = converter.convert_vcf(str(p), kind["joint"], case["keep"], case["suffix"], str(tmp_path), 0, True)
    assert r["engine"] == "device" and r["timing"]["scan_ms"] > 0
    with gzip.open(r["path"], "rb") as f:
        assert f.read().decode() == case["output"]
    assert os.path.basename(r["path"]) == case["output_name"]


@pytest.mark.parametrize("k", range(len(G13["errors"])))
def test_g13_errors(tmp_path, k):
    err = G13["errors"][k]
    p = tmp_path / "x.vcf"
    p.write_text(err["input"])
    assert err["class"] == CrisprHawkConverterError.__name__
    with pytest.raises(CrisprHawkConverterError) as ei:
        converter.convert_vcf(str(p), err["joint"], err["keep"], "conv", str(tmp_path), 0, True)
    assert err["where"] in str(ei.value)


# ------------------------------------------------------------------------------------------------ chunk and sweep seams
HEAD = "chr21\t100\t.\tA\tG\t.\tPASS\t"


def line_with_key_at(offset, value="5", rest="0"):
    """a record whose `AC_afr=` starts at byte `offset` of the line (a padding entry in front of it)"""
    pad = offset - len(HEAD) - len("pad=;")
    assert pad >= 0
    ents = ["pad=" + "x" * pad, f"AC_afr={value}"] + [f"{k}={rest}" for k in refs.keys_of(False)[1:]] + ["AF=0.25"]
    line = HEAD + ";".join(ents)
    assert line.index("AC_afr=") == offset
    return line


def test_key_at_every_chunk_phase_and_both_sides_of_the_sweep():
    lines = [line_with_key_at(o) for o in range(4080, 4098)]
    lines += [line_with_key_at(o, value="0", rest="5") for o in range(4080, 4098)]
    lines += [line_with_key_at(o + 4096) for o in (4080, 4095, 4096, 4097)]  # the second sweep's end
    b = check(lines)
    assert [int(m) & 1 for m in b.mask[:18]] == [1] * 18 and [int(m) for m in b.mask[18:36]] == [0x3fe] * 18


def test_value_straddling_the_sweep():
    lines = [line_with_key_at(o, value="0,0,0,0,5") for o in range(4082, 4097)]
    lines += [line_with_key_at(o, value="0,0,0,0,.") for o in range(4082, 4097)]
    got, kept, failure, b = batch_of(lines[:15], False, True)
    assert failure is None and got == expected(lines[:15], False, True)
    got, kept, failure, b = batch_of(lines, False, True)
    assert got is None and "chr21:100" in failure and [int(f) for f in b.flags] == [0] * 15 + [converter.GN_BAD_VALUE] * 15


@pytest.mark.parametrize("length", [4095, 4096, 4097, 12289, 70001])
def test_whole_record_lengths(length):
    lines = []
    for at_end in (False, True):  # the real key in front of the padding, and as the record's last entry
        base = refs.make_line(counts="0", overrides={"AC_afr": None}, af=None, front=["AC_afr=7"] if not at_end else [], back=["pad="])
        line = base + "y" * (length - 1 - len(base) - (len(";AC_afr=7") if at_end else 0)) + (";AC_afr=7" if at_end else "")
        assert len(line) + 1 == length
        lines.append(line)
    b = check(lines)
    assert [int(m) for m in b.mask] == [1, 1]


def test_shortest_record_and_key_first_last_with_every_line_end():
    short = refs.make_line(counts="1", af=None, chrom="1", pos=1)
    first = refs.make_line(counts="0", overrides={"AC_afr": "3"}, af=None)
    last = refs.make_line(counts="0", overrides={"AC_afr": None}, af=None, back=["AC_afr=3"])
    lines, ends = [], []
    for ln in (short, first, last):
        for tail, end in (("", "\n"), ("", "\r\n"), ("\tninth", "\n"), ("\tninth\ttenth", "\r\n"), ("\t", "\n")):
            lines.append(ln + tail)
            ends.append(end)
    b = check(lines, ends=ends)
    assert [int(m) for m in b.mask] == [0x3ff] * 5 + [1] * 10


# ------------------------------------------------------------------------------------------------ decoys, values, FILTER, AF
@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("keep", [False, True])
def test_case_panel(joint, keep):
    lines = refs.case_lines(joint, with_bad_dropped=not keep)  # records in error with a failing FILTER: dropped, never raised
    b = check(lines, joint, keep)
    if not keep:
        assert int((b.flags == converter.GN_DROPPED).sum()) > 20 and not (b.flags & ~np.uint8(converter.GN_DROPPED)).any()


@pytest.mark.parametrize("value", refs.BAD_VALUES, ids=[repr(v) for v in refs.BAD_VALUES])
@pytest.mark.parametrize("keep", [False, True])
def test_bad_values_are_the_error(value, keep):
    k = "AC_sas"
    bad = refs.make_line(pos=222, overrides={k: k if value is None else value})
    lines = [refs.make_line(pos=111), refs.make_line(pos=112, filt="AC0", overrides={k: "x"}), bad, refs.make_line(pos=333, alt=".")]
    with pytest.raises(refs.RefError) as want:
        expected(lines, False, keep)
    got, kept, failure, b = batch_of(lines, False, keep)
    first = 2 if not keep else 1
    assert want.value.where == ("chr21:222" if not keep else "chr21:112")
    assert got is None and want.value.where in failure
    assert int(b.flags[first]) == converter.GN_BAD_VALUE and int(b.flags[0]) == 0 and int(b.flags[3]) == converter.GN_ALT_MISSING
    assert int(b.flags[1]) == (converter.GN_DROPPED if not keep else converter.GN_BAD_VALUE)


def test_every_flag():
    good = refs.make_line(pos=1)
    lines = [good, "\t".join(good.split("\t")[:7]), refs.make_line(alt="."), refs.make_line(pos="1e3"), refs.make_line(overrides={"AC_mid": None}),
             refs.make_line(overrides={"AC_mid": ""}), refs.make_line(filt="q10"), "x", refs.make_line(pos="", alt=".", overrides={"AC_mid": None, "AC_afr": "."})]
    for keep, want in ((True, [0, 8, 16, 32, 2, 4, 0, 8, 16 | 32 | 2 | 4]), (False, [0, 8, 16, 32, 2, 4, 1, 8, 54])):
        _, _, failure, b = batch_of(lines, False, keep)
        assert [int(f) for f in b.flags] == want and failure is not None
        _, _, _, h = batch_of(lines, False, keep, engine="host")
        for name in ("mask", "flags", "fo", "qs", "afs"):
            assert np.array_equal(getattr(b, name), getattr(h, name)), name


# ------------------------------------------------------------------------------------------------ counts and batches
_MANY = {}


def many_lines():
    if not _MANY:
        rng = np.random.default_rng(7)
        vals, filt = refs.GOOD_VALUES, refs.FILTERS
        lines = [refs.make_line(pos=10 + i, counts=vals[int(rng.integers(0, 7))], filt=filt[int(rng.integers(0, 6))], af=None,
                                overrides={"AC_eas": vals[i % 7]}) for i in range(65537)]
        _MANY["lines"] = lines
        _MANY["out"] = [refs.convert_line(ln, False, False) for ln in lines]
    return _MANY["lines"], _MANY["out"]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_record_counts(n):
    lines, outs = many_lines()
    lines, outs = lines[-n:], outs[-n:]
    got, kept, failure, b = batch_of(lines, False, False)
    assert failure is None and got == "".join(o + "\n" for o in outs if o is not None) and kept == sum(o is not None for o in outs)


def test_many_small_batches_equal_one(tmp_path, monkeypatch):
    lines = synth.gnomad_sites_lines(99, 300, False, 0)
    rng = np.random.default_rng(5)
    lines = [ln + ";pad=" + "z" * int(rng.integers(0, 4800)) for ln in lines]
    lines.insert(150, refs.make_line(pos=5020000, back=["pad=" + "w" * 20000]))  # longer than a batch: a batch of its own
    text = "".join(ln + "\n" for ln in synth.gnomad_sites_header(False) + lines)
    p = tmp_path / "many.sites.vcf"
    p.write_text(text)
    want = refs.convert_text(text, False, False)
    outs = []
    for limit in (None, 8192):
        if limit:
            monkeypatch.setenv("HAWK_GNOMAD_BATCH_BYTES", str(limit))
        r = converter.convert_vcf(str(p), False, False, f"b{limit}", str(tmp_path), 0, True)
        assert r["engine"] == "device" and r["timing"]["scan_ms"] > 0
        assert r["timing"]["batches"] == (1 if limit is None else r["timing"]["batches"]) and (limit is None or r["timing"]["batches"] >= 20)
        with gzip.open(r["path"], "rb") as f:
            outs.append(f.read().decode())
    assert outs[0] == want and outs[1] == want


def test_handle_reuse_empty_batch_and_refused_arguments():
    L, ctx = _lib.lib(), _lib.context(0)
    lines = refs.case_lines(False, False)
    for _ in range(3):  # a handle destroyed, the next one created on the same context
        check(lines)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    kb, ko = converter._key_table(converter.format_ac(False))
    text = np.frombuffer((lines[0] + "\n").encode(), np.uint8).copy()
    lo = np.array([0, len(text)], np.uint64)

    def scan(text, lo, n, kb, ko, nk):
        h, tm = C.c_void_p(), _lib.GnomadTiming()
        rc = L.hawk_gnomad_scan(ctx, p(text), C.c_uint64(len(text)), p(lo), C.c_uint64(n), p(kb), p(ko), C.c_uint32(nk), 1, C.byref(h), C.byref(tm))
        return rc, h, tm
    rc, h, tm = scan(text, lo, 0, kb, ko, 10)  # n_lines = 0: HAWK_OK, an empty blob
    assert rc == _lib.HAWK_OK
    nb, nk, off = C.c_uint64(7), C.c_uint64(7), np.full(1, 9, np.uint64)
    assert L.hawk_gnomad_text(h, None, p(np.zeros(1, np.uint64)), C.byref(nb), C.byref(nk), None) == _lib.HAWK_OK and nb.value == 0 and nk.value == 0
    assert L.hawk_gnomad_text_download(h, None, p(off)) == _lib.HAWK_OK and int(off[0]) == 0
    L.hawk_gnomad_destroy(h)
    rc, h, tm = scan(text, lo, 1, kb, ko, 10)
    assert rc == _lib.HAWK_OK and tm.scan_ms > 0 and tm.n_records == 1
    L.hawk_gnomad_destroy(h)
    many = converter._key_table([f"K{i}" for i in range(32)])
    for t2, lo2, n2, kb2, ko2, nk2 in ((text, lo, 1, many[0], many[1], 32), (text, lo, 1, *converter._key_table(["a;b"]), 1),
                                       (text, lo, 1, *converter._key_table(["a=b"]), 1), (text, lo, 1, *converter._key_table(["a\tb"]), 1),
                                       (text, lo, 1, kb, np.zeros(11, np.uint64), 10), (text[:-1].copy(), lo, 1, kb, ko, 10),
                                       (text, np.array([0, len(text) + 1], np.uint64), 1, kb, ko, 10), (text, np.array([0, 5], np.uint64), 1, kb, ko, 10)):
        h = C.c_void_p()
        rc = L.hawk_gnomad_scan(ctx, p(t2), C.c_uint64(len(t2)), p(lo2), C.c_uint64(n2), p(kb2), p(ko2), C.c_uint32(nk2), 1, C.byref(h), None)
        assert rc == _lib.HAWK_E_INVALID and h.value is None
    check(lines)  # the context is usable as before
    b = check([refs.make_line()])  # and the scan of a real batch reports its time
    assert b.ms["scan_ms"] > 0


# ------------------------------------------------------------------------------------------------ device against the host twin
@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_device_equals_host_twin(seed, joint):
    lines = synth.gnomad_sites_lines(seed, 2000, joint)
    for keep in (False, True):
        d_out, d_kept, d_fail, d = batch_of(lines, joint, keep)
        h_out, h_kept, h_fail, h = batch_of(lines, joint, keep, engine="host")
        assert d_fail is None and h_fail is None and d_kept == h_kept and d_out == h_out
        for name in ("mask", "flags", "fo", "qs", "afs"):
            assert np.array_equal(getattr(d, name), getattr(h, name)), name
    sample = lines[::97]
    assert expected(sample, joint, True) == batch_of(sample, joint, True)[0]


# ------------------------------------------------------------------------------------------------ files
def test_convert_gnomad_vcf_files(tmp_path):
    alts = ["G", "G,T", "G,T,AC"]
    filters = [f for f in refs.FILTERS if f != "."]  # the package's reader splits at white space: an empty FILTER would shift its columns
    lines = [refs.make_line(pos=100 + 3 * k, alt=alts[k % 3], counts=refs.GOOD_VALUES[k % 7], filt=filters[k % 5],
                            af="AF=" + ",".join(f"{(k + 1) / (977 + a):.6e}" for a in range(k % 3 + 1))) for k in range(90)]
    text = "".join(ln + "\n" for ln in refs.HEADER + lines)
    names = ["one.sites.vcf.bgz", "two.sites.vcf.bgz"]
    for nm in names:
        readers.write_bgzf(str(tmp_path / nm), text.encode(), block=4000)
    out = tmp_path / "out"
    out.mkdir()
    converter.convert_gnomad_vcf([str(tmp_path / nm) for nm in names], False, True, "gt", str(out), 4, 0, True)  # keep: all 90 records
    assert sorted(os.listdir(out)) == ["one.sites.gt.vcf.gz", "two.sites.gt.vcf.gz"]
    want = refs.convert_text(text, False, True)
    for nm in os.listdir(out):
        assert readers._TextSource(str(out / nm)).kind == "bgzf"
        with gzip.open(out / nm, "rb") as f:
            assert f.read().decode() == want
    vcf = readers.VCF(str(out / "one.sites.gt.vcf.gz"))
    assert vcf.samples == converter.GNOMADPOPS and vcf.phased is False
    recs = vcf.fetch(Coordinate("chr21", 0, 10 ** 6, 0))
    body = [ln for ln in want.split("\n") if ln and not ln.startswith("#")]
    assert len(recs) == len(body) == 90
    for ln, rec in zip(body, recs):
        assert rec.position == int(ln.split("\t")[1]) and [float(x) for x in ln.split("\t")[7][3:].split(",")] == [float(a) for a in rec.afs]
