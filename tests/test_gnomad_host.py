"""The gnomAD converter without a device: hawk_host_gnomad_lines (csrc/hawk_gnomad.h run on the host) through
convert_vcf(engine="host"), and hawk_host_f32_repr.  Expected values: the reference's output (g13) and tests/gnomad_refs.py."""
import gzip
import os

import numpy as np
import pytest

import gnomad_refs as refs
from crisprhawk_hip import converter, readers
from crisprhawk_hip.coordinate import Coordinate
from crisprhawk_hip.crisprhawk_error import CrisprHawkConverterError
from test_gnomad_refs import G13, case_input


def convert(tmp_path, text, joint, keep, name="in.sites.vcf", batch=None, engine="host", monkeypatch=None, raw=None):
    p = tmp_path / name
    p.write_bytes(raw if raw is not None else text.encode())
    if batch is not None:
        monkeypatch.setenv("HAWK_GNOMAD_BATCH_BYTES", str(batch))
    r = converter.convert_vcf(str(p), joint, keep, "conv", str(tmp_path), 0, True, engine=engine, threads=2)
    assert r["engine"] == engine
    with gzip.open(r["path"], "rb") as f:
        return r, f.read().decode()


@pytest.mark.parametrize("batch", [None, 8192])
@pytest.mark.parametrize("name", sorted(G13["cases"]))
def test_g13_byte_for_byte(tmp_path, monkeypatch, name, batch):
    case = G13["cases"][name]
    kind, text = case_input(case)
    r, got = convert(tmp_path, text, kind["joint"], case["keep"], name=kind["input_name"].replace(".bgz", ".gz"), batch=batch, monkeypatch=monkeypatch)
    assert got == case["output"]
    assert os.path.basename(r["path"]) == case["output_name"]
    assert r["kept"] == case["output"].count("\n") - len(kind["header"]) - 1
    assert r["timing"]["batches"] == 1 if batch is None else r["timing"]["batches"] >= 20
    assert sorted(os.listdir(tmp_path)) == sorted([kind["input_name"].replace(".bgz", ".gz"), case["output_name"]])  # no temporary file


F32_EDGES = ["0", "-0.0", "1e-4", "9.9999e-5", "1e-5", "1e15", "1e16", "1e17", "1.401298464324817e-45", "3.4028235e38", "1234", "0.1", "+5", ".5", "5.",
             "123456789", "0.000123456789", "16777217", "1E3"]


def test_f32_repr_matches_python():
    rng = np.random.default_rng(13)
    strs = list(F32_EDGES)
    for _ in range(10_000):
        kind = int(rng.integers(0, 4))
        m = rng.random() * 10 ** int(rng.integers(-3, 4))
        if kind == 0:
            strs.append(f"{m:.{int(rng.integers(0, 12))}f}")
        elif kind == 1:
            strs.append(f"{m:.{int(rng.integers(0, 10))}e}".replace("e", "e" if rng.random() < 0.5 else "E"))
        elif kind == 2:
            strs.append(f"{m * 10.0 ** int(rng.integers(-48, 35)):.{int(rng.integers(1, 17))}g}")
        else:
            strs.append(str(int(rng.integers(-10 ** 9, 10 ** 9))))
    blob = ",".join(strs).encode()
    text = np.frombuffer(blob, np.uint8)
    lens = np.array([len(s) for s in strs], np.uint32)
    start = np.concatenate(([0], np.cumsum(lens[:-1] + 1))).astype(np.uint64)
    out, off, status = converter.f32_repr(text, start, lens, "None", 3)
    assert not status.any()
    got = [bytes(out[int(off[i]):int(off[i + 1])]).decode() for i in range(len(strs))]
    with np.errstate(over="ignore", under="ignore"):
        want = [str(float(np.float32(float(t)))) for t in strs]
    assert got == want
    # the whole blob as ONE comma list gives the same entries, joined
    out1, off1, st1 = converter.f32_repr(text, np.zeros(1, np.uint64), np.array([len(blob)], np.uint32), "None", 1)
    assert not st1.any() and bytes(out1).decode() == ",".join(want)


@pytest.mark.parametrize("t", ["1e39", "nan", "abc", "", "inf", "-inf", "0x10", " 1", "1 ", "1,,2", "1e", "--1", "3.4028236e38"])
def test_f32_repr_refuses(t):
    text = np.frombuffer((t or " ").encode(), np.uint8)
    out, off, status = converter.f32_repr(text, np.zeros(1, np.uint64), np.array([len(t)], np.uint32), ".", 1)
    assert status[0] == 1 and int(off[1]) == 0


def test_f32_repr_missing_and_absent():
    text = np.frombuffer(b".,0.5,.", np.uint8)
    out, off, status = converter.f32_repr(text, np.zeros(2, np.uint64), np.array([7, 0xFFFFFFFF], np.uint32), "None", 1)
    assert not status.any() and bytes(out).decode() == "None,0.5,None" and int(off[2]) == int(off[1])


GOOD = refs.make_line(pos=50)
REFUSALS = [
    ("few fields", "\t".join(GOOD.split("\t")[:7]).replace("\t50\t", "\t51\t"), "chr21:51"),
    ("ALT .", refs.make_line(pos=52, alt="."), "chr21:52"),
    ("POS", refs.make_line(pos="5x3"), "chr21:5x3"),
    ("POS empty", refs.make_line(pos=""), "chr21:"),
    ("QUAL", refs.make_line(pos=54, qual="abc"), "chr21:54"),
    ("QUAL nan", refs.make_line(pos=55, qual="nan"), "chr21:55"),
    ("AF", refs.make_line(pos=56, af="AF=0.5,x"), "chr21:56"),
    ("AF inf", refs.make_line(pos=57, af="AF=1e39"), "chr21:57"),
    ("AF flag", refs.make_line(pos=58, af="AF"), "chr21:58"),
    ("absent key", refs.make_line(pos=59, overrides={"AC_fin": None}), "chr21:59"),
    ("key without =", refs.make_line(pos=60, overrides={"AC_fin": "AC_fin"}), "chr21:60"),
] + [(f"value {v!r}", refs.make_line(pos=61 + k, overrides={"AC_remaining": v}), f"chr21:{61 + k}")
     for k, v in enumerate([".", ".,3", "", "1x", "12345678901", "0,", "-", "0,.,5"])]


@pytest.mark.parametrize("what,line,where", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_the_first_record(tmp_path, what, line, where):
    text = "".join(ln + "\n" for ln in refs.HEADER + [GOOD, line, refs.make_line(pos=99, alt=".")])
    with pytest.raises(refs.RefError) as want:
        refs.convert_text(text, False, True)
    assert want.value.where == where
    with pytest.raises(CrisprHawkConverterError) as ei:
        convert(tmp_path, text, False, True)
    assert where in str(ei.value)
    assert os.listdir(tmp_path) == ["in.sites.vcf"]  # neither an output nor a temporary file


def test_refused_files(tmp_path):
    with_samples = refs.HEADER[:-1] + [refs.HEADER[-1] + "\tFORMAT\tS1"]
    for text in ("".join(ln + "\n" for ln in with_samples + [GOOD + "\tGT\t0/1"]),  # sample columns already
                 "".join(ln + "\n" for ln in refs.HEADER + [refs.make_line(filt="AC0")]),  # nothing kept
                 "".join(ln + "\n" for ln in refs.HEADER),  # no record at all
                 "".join(ln + "\n" for ln in refs.HEADER[:-1] + [GOOD])):  # no column line
        with pytest.raises(CrisprHawkConverterError):
            convert(tmp_path, text, False, False)
        assert os.listdir(tmp_path) == ["in.sites.vcf"]
    with pytest.raises(SystemExit) as ei:  # the exit-code contract of exception_handler
        converter.convert_vcf(str(tmp_path / "in.sites.vcf"), False, False, "conv", str(tmp_path), 0, False, engine="host")
    assert ei.value.code == os.EX_DATAERR


def test_dropped_records_raise_nothing(tmp_path):
    bad = [ln for _, ln, _ in REFUSALS[1:]]
    bad = ["\t".join(ln.split("\t")[:6] + ["AC0"] + ln.split("\t")[7:]) for ln in bad]
    text = "".join(ln + "\n" for ln in refs.HEADER + [GOOD] + bad)
    r, got = convert(tmp_path, text, False, False)
    assert got == refs.convert_text(text, False, False) and r["records"] == len(bad) + 1 and r["kept"] == 1


@pytest.mark.parametrize("name,out", [("x.vcf.bgz", "x.s1.vcf.gz"), ("x.sites.vcf.gz", "x.sites.s1.vcf.gz"), ("x.vcf", "x.s1.vcf.gz")])
def test_output_naming(tmp_path, name, out):
    assert converter.output_name(f"/a/b/{name}", "s1", "o") == os.path.join("o", out) == refs.output_name(f"/a/b/{name}", "s1", "o")


@pytest.mark.parametrize("joint", [False, True])
def test_header(tmp_path, joint):
    head = refs.HEADER_JOINT if joint else refs.HEADER
    text = "".join(ln + "\n" for ln in head + [refs.make_line(joint=joint, af="AF_joint=0.5" if joint else "AF=0.5")])
    _, got = convert(tmp_path, text, joint, True)
    lines = got.split("\n")
    assert lines[:len(head) - 1] == [ln.replace("<ID=AF_joint,", "<ID=AF,") for ln in head[:-1]]
    assert lines[len(head) - 1] == converter.GTLINE == refs.GTLINE
    assert lines[len(head)] == head[-1] + "\tFORMAT\t" + "\t".join(converter.GNOMADPOPS)
    assert ("AF_joint" in got) == False and got == refs.convert_text(text, joint, True)
    assert converter.format_ac(joint) == refs.keys_of(joint) and converter.GNOMADPOPS == refs.GNOMADPOPS


@pytest.mark.parametrize("container", ["plain", "gzip", "bgzf", "crlf", "no_final_newline"])
def test_containers_and_line_ends(tmp_path, container):
    lines = refs.case_lines(False, True)
    text = "".join(ln + "\n" for ln in refs.HEADER + lines)
    want = refs.convert_text(text, False, False)
    raw, name = text.encode(), "in.sites.vcf"
    if container == "gzip":
        raw, name = gzip.compress(raw), "in.vcf.gz"
    elif container == "bgzf":
        readers.write_bgzf(str(tmp_path / "tmp.bgz"), raw, block=1000)
        raw, name = (tmp_path / "tmp.bgz").read_bytes(), "in.vcf.bgz"
        os.remove(tmp_path / "tmp.bgz")
    elif container == "crlf":
        raw = text.replace("\n", "\r\n").encode()
    elif container == "no_final_newline":
        raw = raw[:-1]
    _, got = convert(tmp_path, text, False, False, name=name, raw=raw)
    assert got == want


def test_converted_file_reads_back(tmp_path):
    alts = ["G", "G,T", "G,T,AC"]  # the reader wants one number per ALT allele, and no empty FILTER (it splits at white space)
    filters = [f for f in refs.FILTERS if f != "."]
    lines = [refs.make_line(pos=100 + 3 * k, alt=alts[k % 3], counts=refs.GOOD_VALUES[k % 7], filt=filters[k % 5], qual=[".", "30"][k % 2],
                            af=[None, "AF=" + ",".join(f"{(k + 1) / (977 + a):.6e}" for a in range(k % 3 + 1))][k % 4 > 0]) for k in range(72)]
    text = "".join(ln + "\n" for ln in refs.HEADER + lines)
    r, got = convert(tmp_path, text, False, True)
    vcf = readers.VCF(r["path"])
    assert vcf.samples == converter.GNOMADPOPS and vcf.phased is False and vcf.contig == "chr21"
    recs = vcf.fetch(Coordinate("chr21", 0, 10 ** 7, 0))
    body = [ln for ln in got.split("\n") if ln and not ln.startswith("#")]
    assert len(recs) == len(body) == r["kept"]
    assert len(body) > 50
    for ln, rec in zip(body, recs):
        f = ln.split("\t")
        assert rec.position == int(f[1])
        assert [float(x) for x in f[7][3:].split(",")] == [float(a) for a in rec.afs]
