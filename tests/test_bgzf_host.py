"""BGZF inflate without a device: the panel of tests/bgzf_refs.py through hawk_host_bgzf_inflate (csrc/hawk_inflate.h as one lane per
host thread), and readers._TextSource(inflate="native") - with VCF and convert_vcf on top of it - against the "zlib" route."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import bgzf_refs as R
from crisprhawk_hip import _lib, converter, pipeline, readers, synth
from crisprhawk_hip.coordinate import Coordinate
from test_gnomad_refs import G13, case_input

CANARY = 0xA5
p = lambda a: a.ctypes.data_as(C.c_void_p)


def host_inflate(members, threads, margin=64):
    """the members in one call into a text buffer with `margin` canary bytes on either side: (rc, text between the canaries, status)"""
    raw, c_off, u_off = R.pack(members)
    raw = raw.copy()  # exactly the members' bytes
    u_off = u_off + np.uint64(margin)
    out = np.full(int(u_off[-1]) + margin, CANARY, np.uint8)
    status = np.full(len(members), 0x77, np.uint8)
    rc = _lib.lib().hawk_host_bgzf_inflate(p(raw), C.c_uint64(raw.size), p(c_off), p(u_off), C.c_uint32(len(members)), p(out), p(status), C.c_uint32(threads))
    assert (out[:margin] == CANARY).all() and (out[int(u_off[-1]):] == CANARY).all(), "a byte outside the text was written"
    return rc, out, u_off, status


def test_panel_is_what_zlib_says():
    """the judge, asked again: every member zlib can judge gives its text there, or fails there"""
    n = 0
    for ms in R.panel().values():
        for m in ms:
            if m.judged:
                xlen = int.from_bytes(m.raw[10:12], "little")
                assert R.zlib_verdict(m.raw[12 + xlen:-8]) == m.text
                n += 1
    assert n >= 55
    hc4 = R.panel()["dyn_hclen_4"][0]
    assert hc4.text is None  # see the module's docstring: zlib refuses what HCLEN = 4 can say
    valid = [k for k, ms in R.panel().items() if not k.startswith("bad_") and k != "dyn_hclen_4"]
    assert all(m.text is not None for k in valid for m in R.panel()[k])
    assert all(m.text is None for k, ms in R.panel().items() if k.startswith("bad_") for m in ms)


def test_golden_file_is_the_panel():
    """what `make asan-inflate` reads is this panel: every member the bit writer made byte for byte, zlib's own output by its text"""
    gold, ms = R.read_golden(), R.unique_members()
    assert len(gold) == len(ms)
    for (raw, isize, crc, status, built), m in zip(gold, ms):
        assert (isize, crc, status, built) == (int.from_bytes(m.raw[-4:], "little"), zlib.crc32(m.text or b"") & 0xffffffff, m.status, int(m.built))
        if m.built:
            assert raw == m.raw
        else:
            xlen = int.from_bytes(raw[10:12], "little")
            assert R.zlib_verdict(raw[12 + xlen:-8]) == m.text


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("name", list(R.panel()))
def test_panel_case(name, threads):
    members = R.panel()[name]
    rc, out, u_off, status = host_inflate(members, threads)
    R.check_result(members, u_off, out, status)
    assert rc == (_lib.HAWK_OK if all(m.text is not None for m in members) else _lib.HAWK_E_INVALID)


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("n", R.LAUNCH_SIZES)
def test_launch_sizes(n, threads):
    """valid and malformed members in turn: a failure leaves the bytes of its neighbours as they must be"""
    members = R.launch(n)
    rc, out, u_off, status = host_inflate(members, threads)
    R.check_result(members, u_off, out, status)
    assert rc == (_lib.HAWK_E_INVALID if any(m.text is None for m in members) else _lib.HAWK_OK)
    if n >= 4:
        assert [len(m.text) for m in members[:4]] == [0, 1, 65536, 65536]


def test_refusals():
    m = R.panel()["zlib_level_6"][0]
    raw, c_off, u_off = R.pack([m])
    out = np.full(len(m.text), CANARY, np.uint8)
    status = np.full(1, 0x77, np.uint8)
    fn = _lib.lib().hawk_host_bgzf_inflate
    call = lambda raw_p=p(raw), nbytes=raw.size, c=c_off, u=u_off, n=1, o=p(out), s=p(status): fn(
        raw_p, C.c_uint64(nbytes), None if c is None else p(c), None if u is None else p(u), C.c_uint32(n), o, s, C.c_uint32(1))
    u64 = lambda *v: np.array(v, np.uint64)
    assert call(c=u64(4, 0)) == _lib.HAWK_E_INVALID                      # offsets that do not ascend
    assert call(u=u64(len(m.text), 0)) == _lib.HAWK_E_INVALID
    assert call(nbytes=raw.size - 1) == _lib.HAWK_E_INVALID              # a member outside in_bytes
    assert call(c=None) == call(u=None) == call(raw_p=None) == call(o=None) == call(s=None) == _lib.HAWK_E_INVALID
    assert status[0] == 0x77 and (out == CANARY).all()                   # nothing was written
    assert call(n=0, c=None, u=None, raw_p=None, o=None, s=None) == _lib.HAWK_OK
    assert call() == _lib.HAWK_OK and bytes(out) == m.text and status[0] == R.BZ_OK
    # a text range that is not the member's ISIZE is the member's failure, not the call's
    assert call(u=u64(0, len(m.text) - 1)) == _lib.HAWK_E_INVALID and status[0] == R.BZ_SIZE


@pytest.fixture(scope="module")
def bgzf_vcf(tmp_path_factory):
    """VCF-like text in members of 4000 bytes (the last one shorter), and the same file with a member no bgzip writes and with a
    member whose stream is broken"""
    d = tmp_path_factory.mktemp("bgzf")
    text = R.vcf_text(300001, 21)
    good = R.bgzf_file(d / "good.vcf.gz", text, 4000)
    c_off, _ = R.member_offsets(good)
    blob = bytearray(open(good, "rb").read())
    odd = bytearray(blob)
    odd[c_off[5] + 3] |= 1                               # FLG gains FTEXT: zlib never looks, the library declines the member
    open(d / "odd.vcf.gz", "wb").write(odd)
    broken = bytearray(blob)
    broken[c_off[40] + 18] = 0x07                        # the stream's first block is of type 3: zlib raises
    open(d / "broken.vcf.gz", "wb").write(broken)
    return {"text": text, "good": good, "odd": str(d / "odd.vcf.gz"), "broken": str(d / "broken.vcf.gz")}


def test_text_source_native_equals_zlib(bgzf_vcf):
    src = R.assert_routes_agree(bgzf_vcf["good"], "native", 50000)
    assert b"".join(c for _, c in R.all_chunks(bgzf_vcf["good"], "native", 50000)) == bgzf_vcf["text"]
    assert src.inflate_ms == 0.0


def test_text_source_fallback(bgzf_vcf, capsys):
    """a member the library refuses sends its chunk to the zlib loop: the same bytes where zlib reads the member, zlib's error where not"""
    R.assert_routes_agree(bgzf_vcf["odd"], "native", 50000)
    capsys.readouterr()
    got = R.all_chunks(bgzf_vcf["odd"], "native", 50000, verbosity=3)
    assert b"".join(c for _, c in got) == bgzf_vcf["text"]
    said = capsys.readouterr().out
    assert "BGZF member 5 " in said and "a gzip header bgzip does not write" in said
    assert R.all_chunks(bgzf_vcf["odd"], "native", 50000, verbosity=2) == got and capsys.readouterr().out == ""
    want = R.all_chunks(bgzf_vcf["broken"], "zlib", 50000)
    assert want is zlib.error and R.all_chunks(bgzf_vcf["broken"], "native", 50000) is want
    a, b = readers._TextSource(bgzf_vcf["broken"], "zlib"), readers._TextSource(bgzf_vcf["broken"], "native")
    _, u_off = R.member_offsets(bgzf_vcf["broken"])
    assert bytes(b.read(u_off[3] - 1, u_off[9] + 1)) == bytes(a.read(u_off[3] - 1, u_off[9] + 1))
    for src in (a, b):
        with pytest.raises(zlib.error):
            src.read(u_off[39], u_off[42])


def test_switch(tmp_path, monkeypatch, bgzf_vcf):
    f = bgzf_vcf["good"]
    monkeypatch.delenv("HAWK_BGZF_INFLATE", raising=False)
    assert readers._TextSource(f).inflate == "zlib"
    monkeypatch.setenv("HAWK_BGZF_INFLATE", "native")
    assert readers._TextSource(f).inflate == "native" and readers._TextSource(f, "zlib").inflate == "zlib"
    monkeypatch.setenv("HAWK_BGZF_INFLATE", "fast")
    with pytest.raises(ValueError, match="HAWK_BGZF_INFLATE='fast'"):
        readers._TextSource(f)
    monkeypatch.delenv("HAWK_BGZF_INFLATE")
    for make in (lambda: readers._TextSource(f, "gpu"), lambda: readers.VCF(f, inflate="gpu"),
                 lambda: converter.convert_vcf(f, False, False, "conv", str(tmp_path), 0, True, engine="host", inflate="gpu"),
                 lambda: pipeline.search_files("no.fa", "no.bed", [], "NGG", 20, False, str(tmp_path), bgzf_inflate="gpu")):
        with pytest.raises(ValueError, match="'gpu': None, 'zlib', 'native' or 'device'"):
            make()
    # plain text and plain gzip have no members: the switch is taken and not used
    plain = tmp_path / "plain.vcf"
    plain.write_bytes(bgzf_vcf["text"])
    assert b"".join(bytes(c) for _, c in readers._TextSource(str(plain), "native").chunks()) == bgzf_vcf["text"]
    monkeypatch.setenv("OMP_NUM_THREADS", "3")
    assert readers.host_inflate_threads() == 3
    monkeypatch.delenv("OMP_NUM_THREADS")
    assert readers.host_inflate_threads() == 16


def test_vcf_index_native_equals_zlib(tmp_path, monkeypatch):
    reg = synth.make_region(9301, "chrF", 9000, 2000, 7000)
    synth.add_phased_variants(reg, 9302, 120, 6)
    plain = str(tmp_path / "v.vcf")
    readers.write_vcf(plain, reg.contig, reg.samples, [reg.vcf_fields(v) for v in reg.variants], False)
    vcf = R.bgzf_file(tmp_path / "v.vcf.gz", open(plain, "rb").read(), 777)
    monkeypatch.setattr(readers._TextSource, "CHUNK", 3000)  # several chunks, lines cut by their ends
    a, b = readers.VCF(vcf, inflate="zlib"), readers.VCF(vcf, inflate="native")
    assert b._src.inflate == "native" and len(a._pos) == len(reg.variants)
    for k in ("_starts", "_ends", "_pos"):
        assert np.array_equal(getattr(a, k), getattr(b, k))
    assert (a.samples, a.contig, a.phased, a._total) == (b.samples, b.contig, b.phased, b._total)
    c = Coordinate(reg.contig, reg.startp + 500, reg.stopp - 500, 0)
    ba, bb = a.fetch_block(c), b.fetch_block(c)
    assert len(ba) > 10 and bytes(ba.text) == bytes(bb.text) and np.array_equal(ba.line_off, bb.line_off) and np.array_equal(ba.gt_off, bb.gt_off)


def test_convert_vcf_native_equals_zlib(tmp_path):
    case = G13["cases"]["plain_keep0"]
    kind, text = case_input(case)
    src = R.bgzf_file(tmp_path / "in.sites.vcf.gz", text.encode(), 1000)
    res = {}
    for route in ("zlib", "native"):
        os.makedirs(tmp_path / route)
        res[route] = converter.convert_vcf(src, kind["joint"], case["keep"], "conv", str(tmp_path / route), 0, True, engine="host", threads=2, inflate=route)
        assert res[route]["timing"]["inflate_route"] == route and "inflate_ms" not in res[route]["timing"]
    assert open(res["native"]["path"], "rb").read() == open(res["zlib"]["path"], "rb").read()
    assert res["native"]["kept"] == res["zlib"]["kept"] > 0
