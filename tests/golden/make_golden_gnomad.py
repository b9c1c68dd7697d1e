#!/usr/bin/env python3
"""Generate tests/golden/g13_gnomad.json.gz by running the REFERENCE's gnomAD converter.

    python tests/golden/make_golden_gnomad.py

Build container only, like make_golden.py (whose stand-ins are imported).  pysam is absent, so PYSAM ITSELF IS RESTATED: the
reference's own `convert_vcf` -> `_convert` -> `_asses_genotype` / `_format_vrecord` / `_update_header` (converter.py) run over
an in-process stand-in for `pysam.VariantFile` / `VariantHeader` / `VariantRecord` whose records hold what pysam would hand
over: tuples of ints or None for the allele counts, float32-narrowed floats or None for QUAL and AF, `filter.keys()`, `alts`,
`id` None for '.'.  `load_vcf` hands out the stand-in and `pysam.tabix_compress` is a gzip copy, so the output NAME is the
reference's own too.

Pinned by the fixture: the keep rule, the genotype rule (any(ac > 0) left to right, the TypeError at None, the KeyError at an
absent key), the field order, the None / empty handling (FILTER '.' -> '', AF '.' -> None, QUAL '.' -> '.'), the names.
NOT pinned: htslib's parsing of the text (which occurrence of a duplicated key it keeps, what it refuses) and the header text
it would regenerate - the stand-in keeps the FIRST occurrence and copies the header lines.

Only the input text and the reference's output text are stored.  Per kind (joint or not) one list of data lines; the records
in error whose FILTER fails are listed by index: a keep-off run sees them (and drops them), the keep-on input leaves them out.
"""
import gzip
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (installs the stand-ins, puts the reference and the package on sys.path)

import numpy as np  # noqa: E402

import gnomad_refs as refs  # noqa: E402  (record builders only: nothing of its rules is used here)
from crisprhawk_hip import synth  # noqa: E402


class _Filter:
    def __init__(self, text):
        self._keys = [] if text == "." else text.split(";")

    def keys(self):
        return list(self._keys)


def _f32(t):
    return float(np.float32(float(t)))


class _Info:
    """INFO unpacked when first read, as htslib unpacks a record's parts on demand: a record the keep rule drops is never parsed"""

    def __init__(self, text):
        self._text, self._d = text, None

    def __getitem__(self, key):
        if self._d is None:
            self._d = {}
            for e in self._text.split(";"):
                k, eq, val = e.partition("=")
                if k in self._d or not eq:
                    continue  # the first occurrence is kept (unpinned); flags are never read
                if k.startswith("AC"):
                    self._d[k] = tuple(None if x == "." else int(x) for x in val.split(","))
                elif k.startswith("AF"):
                    self._d[k] = tuple(None if x == "." else _f32(x) for x in val.split(","))
                else:
                    self._d[k] = val
        return self._d[key]


class VariantRecord:
    def __init__(self, line):
        self._line = line
        f = line.split("\t")
        self._f = f
        self.chrom, self.pos, self.ref = f[0], int(f[1]), f[3]
        self.id = None if f[2] == "." else f[2]
        self.filter = _Filter(f[6])
        self.info = _Info(f[7])

    alts = property(lambda self: None if self._f[4] == "." else tuple(self._f[4].split(",")))
    qual = property(lambda self: None if self._f[5] == "." else _f32(self._f[5]))

    def __str__(self):
        return self._line


class VariantHeader:
    def __init__(self, lines):
        self._lines = list(lines)

    def copy(self):
        return VariantHeader(self._lines)

    def add_line(self, line):
        self._lines.insert(len(self._lines) - 1, line)

    def add_samples(self, samples):
        self._lines[-1] = "\t".join([self._lines[-1], "FORMAT"] + list(samples))

    def __str__(self):
        return "".join(ln + "\n" for ln in self._lines)


class VariantFile:
    def __init__(self, text):
        lines = text.split("\n")[:-1]
        self.header = VariantHeader([ln for ln in lines if ln.startswith("#")])
        self._records = [ln for ln in lines if not ln.startswith("#")]

    def __iter__(self):
        return (VariantRecord(ln) for ln in self._records)


ps = sys.modules["pysam"]
ps.VariantFile, ps.VariantHeader, ps.VariantRecord = VariantFile, VariantHeader, VariantRecord


def _gzip_copy(src, dst, force=True):
    with open(src, "rb") as a, gzip.open(dst, "wb") as b:
        shutil.copyfileobj(a, b)


ps.tabix_compress = _gzip_copy

from crisprhawk import converter as R_conv  # noqa: E402
from crisprhawk.crisprhawk_error import CrisprHawkConverterError  # noqa: E402


def run_reference(text, joint, keep, input_name, suffix):
    """(output file's base name, its text) by the reference's convert_vcf"""
    R_conv.load_vcf = lambda fname, verbosity, debug: VariantFile(text)
    with tempfile.TemporaryDirectory() as td:
        R_conv.convert_vcf(os.path.join("/somewhere", input_name), joint, keep, suffix, td, 0, True)
        names = os.listdir(td)
        assert len(names) == 1, names  # no temporary file survives
        with gzip.open(os.path.join(td, names[0]), "rt") as f:
            return names[0], f.read()


def kind(joint, seed):
    good = refs.case_lines(joint, False)
    both = refs.case_lines(joint, True)
    assert both[:len(good)] == good
    lines = synth.gnomad_sites_lines(seed, 100, joint, 0) + both + synth.gnomad_sites_lines(seed + 1, 110, joint, 0)
    bad = list(range(100 + len(good), 100 + len(both)))
    return synth.gnomad_sites_header(joint), lines, bad


def text_of(header, lines):
    return "".join(ln + "\n" for ln in header + lines)


if __name__ == "__main__":
    out = {"kinds": {}, "cases": {}, "errors": []}
    names = {False: "gnomad.genomes.v4.1.sites.chr21.vcf.bgz", True: "gnomad.joint.v4.1.sites.chr21.vcf.gz"}
    for joint in (False, True):
        header, lines, bad = kind(joint, 13010 + 10 * joint)
        kname = "joint" if joint else "plain"
        out["kinds"][kname] = {"joint": joint, "header": header, "lines": lines, "bad_dropped": bad, "input_name": names[joint]}
        for keep in (False, True):
            use = lines if not keep else [ln for i, ln in enumerate(lines) if i not in set(bad)]
            oname, otext = run_reference(text_of(header, use), joint, keep, names[joint], "conv")
            out["cases"][f"{kname}_keep{int(keep)}"] = {"kind": kname, "keep": keep, "suffix": "conv", "output_name": oname, "output": otext}
            print(f"   {kname} keep={keep}: {len(use)} records -> {otext.count(chr(10)) - len(header) - 1} lines, {oname}")
    k0 = refs.keys_of(False)[0]
    for what, line in (("absent key", refs.make_line(pos=77, overrides={k0: None})), (".,3", refs.make_line(pos=78, overrides={k0: ".,3"}))):
        text = text_of(refs.HEADER, [refs.make_line(pos=70), line])
        try:
            run_reference(text, False, True, "x.vcf.gz", "conv")
            raise SystemExit(f"{what}: the reference raised nothing")
        except CrisprHawkConverterError as e:
            out["errors"].append({"what": what, "joint": False, "keep": True, "input": text, "class": type(e).__name__, "message": str(e),
                                  "where": f"chr21:{77 if what == 'absent key' else 78}"})
            print(f"   {what}: {type(e).__name__}")
    mg.dump("g13_gnomad.json.gz", out)
