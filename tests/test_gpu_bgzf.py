"""BGZF inflate on the device: the panel of tests/bgzf_refs.py through hawk_bgzf_inflate (k_bz_inflate, one wavefront per member),
and readers._TextSource(inflate="device") - with search_files and convert_vcf on top of it - against the "zlib" route.  The
malformed members are those of tests/golden/bgzf_panel.bin, which `make asan-inflate` has run through the same header on the host."""
import ctypes as C
import os

import numpy as np
import pytest

import bgzf_refs as R
from crisprhawk_hip import _lib, converter, pipeline, readers, synth
from test_gnomad_refs import G13, case_input
from util import load_golden

pytestmark = pytest.mark.gpu
CANARY = 0xA5
p = lambda a: a.ctypes.data_as(C.c_void_p)


def device_inflate(members, pinned=False, margin=64):
    raw, c_off, u_off = R.pack(members)
    u_off = u_off + np.uint64(margin)
    n_out = int(u_off[-1]) + margin
    if pinned:
        src = _lib.pinned_empty(max(raw.size, 1 << 20), np.uint8)
        out = _lib.pinned_empty(max(n_out, 1 << 20), np.uint8)[:n_out]
        src[:raw.size] = raw
        raw = src[:raw.size]
    else:
        raw, out = raw.copy(), np.empty(n_out, np.uint8)
    out[:] = CANARY
    status = np.full(len(members), 0x77, np.uint8)
    tm = _lib.BgzfTiming()
    rc = _lib.lib().hawk_bgzf_inflate(_lib.context(), p(raw), C.c_uint64(raw.size), p(c_off), p(u_off), C.c_uint32(len(members)), p(out), p(status),
                                      C.byref(tm))
    assert (out[:margin] == CANARY).all() and (out[int(u_off[-1]):] == CANARY).all(), "a byte outside the text was written"
    assert rc == (_lib.HAWK_OK if all(m.text is not None for m in members) else _lib.HAWK_E_INVALID)
    R.check_result(members, u_off, out, status)
    assert tm.inflate_ms > 0 and tm.total_ms >= tm.inflate_ms, "the kernel did not run"
    assert (tm.n_members, tm.n_failed, tm.in_bytes, tm.out_bytes) == (len(members), sum(m.text is None for m in members), raw.size, n_out - 2 * margin)
    return tm


def test_whole_panel_case_by_case():
    for name, members in R.panel().items():
        try:
            device_inflate(members)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("n", R.LAUNCH_SIZES)
def test_launch_sizes(n, pinned):
    """valid and malformed members in turn, the first workgroup's waves with the end marker, one byte and twice 65536 bytes"""
    device_inflate(R.launch(n), pinned)


def test_all_members_in_one_call():
    device_inflate(R.unique_members(), pinned=True)


def test_refusals_and_empty():
    m = R.panel()["zlib_level_6"][0]
    raw, c_off, u_off = R.pack([m])
    out, status = np.full(len(m.text), CANARY, np.uint8), np.full(1, 0x77, np.uint8)
    fn, ctx = _lib.lib().hawk_bgzf_inflate, _lib.context()
    u64 = lambda *v: np.array(v, np.uint64)
    assert fn(ctx, p(raw), C.c_uint64(raw.size), p(u64(4, 0)), p(u_off), C.c_uint32(1), p(out), p(status), None) == _lib.HAWK_E_INVALID
    assert fn(ctx, p(raw), C.c_uint64(raw.size - 1), p(c_off), p(u_off), C.c_uint32(1), p(out), p(status), None) == _lib.HAWK_E_INVALID
    assert fn(ctx, p(raw), C.c_uint64(raw.size), p(c_off), None, C.c_uint32(1), p(out), p(status), None) == _lib.HAWK_E_INVALID
    assert fn(None, p(raw), C.c_uint64(raw.size), p(c_off), p(u_off), C.c_uint32(1), p(out), p(status), None) == _lib.HAWK_E_INVALID
    assert status[0] == 0x77 and (out == CANARY).all()
    assert fn(ctx, None, C.c_uint64(0), None, None, C.c_uint32(0), None, None, None) == _lib.HAWK_OK
    assert fn(ctx, p(raw), C.c_uint64(raw.size), p(c_off), p(u_off), C.c_uint32(1), p(out), p(status), None) == _lib.HAWK_OK
    assert bytes(out) == m.text


def test_text_source_device_equals_zlib(tmp_path, capsys):
    text = R.vcf_text(300001, 21)
    good = R.bgzf_file(tmp_path / "good.vcf.gz", text, 4000)
    src = R.assert_routes_agree(good, "device", 50000)
    assert src.inflate_ms > 0
    c_off, _ = R.member_offsets(good)
    odd = bytearray(open(good, "rb").read())
    odd[c_off[5] + 3] |= 1  # FLG gains FTEXT: the kernel declines the member, zlib reads it
    open(tmp_path / "odd.vcf.gz", "wb").write(odd)
    got = R.all_chunks(str(tmp_path / "odd.vcf.gz"), "device", 50000, verbosity=3)
    assert b"".join(c for _, c in got) == text and "BGZF member 5 " in capsys.readouterr().out


def test_search_files_device_inflate(tmp_path):
    """FASTA + BED + a BGZF VCF -> report: the same bytes whoever inflates"""
    fx = load_golden("g7_report_phased4.json.gz")
    contig_seq = "N" * (fx["startp"] - 1) + fx["region_seq"] + "ACGT" * 10
    fa, bed, vcf = str(tmp_path / "g.fa"), str(tmp_path / "r.bed"), str(tmp_path / "v.vcf.gz")
    readers.write_fasta(fa, fx["contig"], contig_seq, 80)
    with open(bed, "w") as f:
        f.write(f"{fx['contig']}\t{fx['bed_start']}\t{fx['bed_stop']}\n")
    rows = [[fx["contig"], str(q), ".", r, a, ".", "PASS", f"AF={af:.6g}", "GT"] + [f"{g[0]}|{g[1]}" for g in gts] for q, r, a, af, gts in fx["variants"]]
    plain = str(tmp_path / "v.vcf")
    readers.write_vcf(plain, fx["contig"], fx["samples"], rows, False)
    R.bgzf_file(vcf, open(plain, "rb").read(), 300)
    assert readers._TextSource(vcf).kind == "bgzf"
    out = {}
    for route in (None, "device"):
        (path,) = pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / str(route)), cfd_tables=synth.cfd_tables(),
                                        bgzf_inflate=route).values()
        out[route] = open(path, "rb").read()
    assert out["device"] == out[None] and out[None].decode() == fx["report_tsv"]


def test_convert_vcf_device_inflate(tmp_path):
    case = G13["cases"]["plain_keep0"]
    kind, text = case_input(case)
    src = R.bgzf_file(tmp_path / "in.sites.vcf.gz", text.encode(), 1000)
    res = {}
    for route in ("zlib", "device"):
        os.makedirs(tmp_path / route)
        res[route] = converter.convert_vcf(src, kind["joint"], case["keep"], "conv", str(tmp_path / route), 0, True, engine="device", threads=2, inflate=route)
        assert res[route]["timing"]["inflate_route"] == route
    assert res["device"]["timing"]["inflate_ms"] > 0 and "inflate_ms" not in res["zlib"]["timing"]
    assert open(res["device"]["path"], "rb").read() == open(res["zlib"]["path"], "rb").read()
