"""The gnomAD converter's rules restated per line in plain Python, for the tests: what a data line of a sites VCF becomes
(reference converter.py:148-214, 246-250 on what pysam would hand it), the header, the output name.  Nothing here calls the
package; tests/test_gnomad_refs.py holds it to the reference's own output (tests/golden/g13_gnomad.json.gz)."""
import os
import re

import numpy as np

GNOMADPOPS = ["afr", "ami", "amr", "asj", "eas", "fin", "nfe", "mid", "sas", "remaining"]
GTLINE = '##FORMAT=<ID=GT,Number=1,Type=String,Description="Sample Collapsed Genotype">'
_INT = re.compile(r"[+-]?[0-9]{1,10}")
_DEC = re.compile(r"[+-]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)?")


class RefError(Exception):
    """what the package raises as CrisprHawkConverterError; `where` = CHROM:POS of the record"""

    cls = "CrisprHawkConverterError"

    def __init__(self, message, where=None):
        super().__init__(message)
        self.where = where


def keys_of(joint):
    return [f"AC_joint_{p}" if joint else f"AC_{p}" for p in GNOMADPOPS]


def f32_str(t):
    """str() of what pysam hands over for a Float entry: strtod, narrowed to float32, widened again"""
    if not _DEC.fullmatch(t):
        raise ValueError(t)
    with np.errstate(over="ignore"):
        v = float(np.float32(float(t)))
    if not np.isfinite(v):
        raise ValueError(t)
    return str(v)


def info_entry(info, key):
    """the first entry of INFO whose key is `key`: its value, None for the key without '=', KeyError without the key"""
    for e in info.split(";"):
        if e == key:
            return None
        if e.startswith(key + "="):
            return e[len(key) + 1:]
    raise KeyError(key)


def observed(value):
    """any(ac > 0 for ac in tuple) read left to right; TypeError at a '.', ValueError at what is no integer"""
    for e in value.split(","):
        if e == ".":
            raise TypeError("'>' not supported between instances of 'NoneType' and 'int'")
        if not _INT.fullmatch(e):
            raise ValueError(e)
        if int(e) > 0:
            return True
    return False


def convert_line(line, joint, keep):
    """The output line (without '\\n') of a data line (without its line end); None for a record the keep rule drops."""
    f = line.split("\t")
    where = f"{f[0]}:{f[1]}" if len(f) > 1 else repr(line[:40])
    if len(f) < 8:
        raise RefError(f"fewer than eight fields in record {where}", where)
    chrom, pos, vid, ref, alt, qual, filt, info = f[:8]
    if not keep and "PASS" not in filt.split(";"):
        return None
    if alt == ".":
        raise RefError(f"missing ALT in record {where}", where)
    if not re.fullmatch(r"[0-9]+", pos):
        raise RefError(f"POS is not a number in record {where}", where)
    gts = []
    for key in keys_of(joint):
        try:
            v = info_entry(info, key)
            if v is None:
                raise ValueError(key)
            gts.append("0/1" if observed(v) else "0/0")
        except (KeyError, TypeError, ValueError) as e:
            raise RefError(f"Failed genotyoe assessment on variant {line}", where) from e
    try:
        q = "." if qual == "." else f32_str(qual)
        try:
            v = info_entry(info, "AF")
            af = ",".join("None" if e == "." else f32_str(e) for e in ("" if v is None else v).split(","))
        except KeyError:
            af = ",".join("0.0" for _ in alt.split(","))
    except ValueError as e:
        raise RefError(f"QUAL or AF is not a finite decimal number in record {where}", where) from e
    return "\t".join([chrom, pos, vid, ref, alt, q, "" if filt == "." else filt, f"AF={af}", "GT"] + gts)


def header_text(header_lines, joint):
    meta = [ln for ln in header_lines if ln.startswith("##")]
    cols = [ln for ln in header_lines if not ln.startswith("##")]
    assert len(cols) == 1
    if len(cols[0].split("\t")) > 8:
        raise RefError("input already has FORMAT / sample columns")
    text = "".join(ln + "\n" for ln in meta) + GTLINE + "\n" + "\t".join(cols[0].split("\t") + ["FORMAT"] + GNOMADPOPS) + "\n"
    return text.replace("<ID=AF_joint,", "<ID=AF,") if joint else text


def convert_text(text, joint, keep):
    """a whole sites VCF (text) -> the converted VCF (text)"""
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    lines = [ln[:-1] if ln.endswith("\r") else ln for ln in lines]
    head = [ln for ln in lines if ln.startswith("#")]
    body = [convert_line(ln, joint, keep) for ln in lines if not ln.startswith("#")]
    body = [b for b in body if b is not None]
    if not body:
        raise RefError("Empty converted VCF")
    return header_text(head, joint) + "".join(b + "\n" for b in body)


def output_name(vcf_fname, suffix, outdir):
    stem = os.path.splitext(os.path.splitext(os.path.basename(vcf_fname))[0])[0]
    return os.path.join(outdir, f"{stem}.{suffix}.vcf.gz")


# ---------------------------------------------------------------------------------------------- building records
def make_line(counts="0", joint=False, chrom="chr21", pos=100, vid=".", ref="A", alt="G", qual=".", filt="PASS", af="AF=0.5", front=(), back=(),
              overrides=None, tail=""):
    """One data line: INFO = front entries, the ten allele-count entries (value `counts`, or per key from `overrides`: a value,
    or a whole entry when it holds no '=' ... or None to leave the key out), the AF entry (None: none), back entries."""
    overrides = overrides or {}
    ents = list(front)
    for k in keys_of(joint):
        if k in overrides:
            o = overrides[k]
            if o is None:
                continue
            ents.append(o if o.startswith(k) else f"{k}={o}")
        else:
            ents.append(f"{k}={counts}")
    if af is not None:
        ents.append(af)
    ents += list(back)
    return "\t".join([chrom, str(pos), vid, ref, alt, qual, filt, ";".join(ents)]) + tail


HEADER = ["##fileformat=VCFv4.2", '##INFO=<ID=AF,Number=A,Type=Float,Description="Alternate allele frequency">',
          "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
HEADER_JOINT = ["##fileformat=VCFv4.2", '##INFO=<ID=AF_joint,Number=A,Type=Float,Description="Alternate allele frequency">',
                "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]

GOOD_VALUES = ["0", "00", "5", "0,0,5", "-3", "2147483647", "3,."]
BAD_VALUES = [".", ".,3", "", None, "1x", "12345678901"]  # None: the key present without '='
FILTERS = ["PASS", ".", "AC0", "AC0;PASS", "PASSED", "NOPASS"]


def case_lines(joint, with_bad_dropped, pos0=1000):
    """The value, decoy, FILTER and AF cases the tests name, as convertible records (under keep on AND off unless they are the
    `with_bad_dropped` ones: records in error whose FILTER fails, which only a keep-off run may see)."""
    k0 = keys_of(joint)[0]
    other = keys_of(not joint)[0]
    out, pos = [], pos0

    def add(**kw):
        nonlocal pos
        pos += 7
        out.append(make_line(joint=joint, pos=pos, **kw))

    for v in GOOD_VALUES:
        for filt in FILTERS:
            add(counts=v, filt=filt)
    for real, decoy in (("0", "5"), ("5", "0")):  # every decoy carries the opposite of the real key
        for d in (f"{k0}_XX={decoy}", f"X{k0}={decoy}", f"{other}={decoy}", f"nhomalt_afr={decoy}", f"x={k0}={decoy}"):
            add(counts=real, front=[d])
            add(counts=real, back=[d])
        add(counts=real, back=[f"{k0}={decoy}"])  # a duplicate: the first occurrence is read
    for alt in ("G", "G,T", "G,T,AC"):
        add(af=None, alt=alt)
        add(af="AF_joint=0.25", alt=alt)
    for af in ("AF=.", "AF=0.5,.", "AF=0.125,1e-05,3", "AF=1e-10", "AF=0.1"):
        add(af=af, alt="G,T,C")
    for q in (".", "1234", "0.1", "1e16", "9.9999e-5", "-0.0", "100"):
        add(qual=q)
    add(front=["flag"], back=["last"], vid="rs12", ref="ACGT", alt="A")
    if with_bad_dropped:
        for v in BAD_VALUES:
            add(overrides={k0: k0 if v is None else v}, filt="AC0")
        add(overrides={k0: None}, filt=".")
        add(alt=".", filt="NOPASS")
        add(qual="abc", filt="PASSED")
    return out
