"""Records that put the gnomAD converter's device code (csrc/hawk_gnomad.hip) on its seams, and what the scan and the fill pass
must report for them, in plain Python: numpy and tests/gnomad_refs.py only, nothing from the package.

  k_gn_scan        sweeps a record in 4096-byte pieces of 16-byte chunks (SWEEP, CHUNK): field starts, ALT commas and the AF entry
                   are found by the thread whose chunk holds them, with the field index carried from chunk to chunk by a workgroup
                   scan and from sweep to sweep by `field_base`.  record_facts() says what it must find from line.split("\\t") alone.
  k_gn_text_fill   a wave owns 64 records (WAVE) and stages their lines in an 8192-byte LDS slot (SLOT) at the phase
                   a = off[r0] & 15 of the wave's range on the blob's 16-byte grid; a + total > SLOT goes straight to global memory.
                   wave_figures() says, from gnomad_refs.convert_line alone, which route every wave takes and at which phase.

tests/test_gnomad_seams.py asserts, on these panels and from this file alone, every figure a case is named for, and runs them
through the host twin; tests/test_gpu_gnomad_seams.py runs them on the device."""
from collections import namedtuple

import numpy as np

import gnomad_refs as refs

CHUNK, SWEEP, SLOT, WAVE, WG_WAVES = 16, 4096, 8192, 64, 4
ABSENT = 0xFFFFFFFF
GN_DROPPED, GN_FEW_FIELDS = 1, 8
SHORTEST_LINE = 67  # bytes of the shortest output line with ten keys: 1 1 . A G . PASS AF=0.0 GT 10 x "0/1", tabs, '\n'

Case = namedtuple("Case", "label line end")  # end: the record's line end, "\n" or "\r\n"


# ---------------------------------------------------------------------------------------------- what the scan must report
def record_facts(line):
    """dict(fo, full, qs, afs, n_alt) of a data line (without its line end), by the definitions of hawk_gnomad.h:
    fo[f] the start of field f or len(line) for a missing one; full: eight fields or more; qs = {QUAL start, length} (to the
    line's end where FILTER is missing: gn_spans reads no further field then); afs = {n_alt, ABSENT} without an AF entry (and for
    a record that is not full), {value start, value length} for the first `AF=` entry, {pos + 2, 0} for a bare `AF`."""
    f = line.split("\t")
    n = len(line)
    starts, p = [], 0
    for x in f:
        starts.append(p)
        p += len(x) + 1
    fo = [starts[k] if k < len(f) else n for k in range(8)]
    full = len(f) >= 8
    q1 = fo[6] - 1 if full else n
    qs = [fo[5], max(q1 - fo[5], 0)]
    n_alt = (f[4].count(",") if len(f) > 4 else 0) + 1
    afs = [n_alt, ABSENT]
    if full:
        p = fo[7]
        for e in f[7].split(";"):
            if e == "AF":
                afs = [p + 2, 0]
                break
            if e.startswith("AF="):
                afs = [p + 3, len(e) - 3]
                break
            p += len(e) + 1
    return dict(fo=fo, full=full, qs=qs, afs=afs, n_alt=n_alt)


def facts_arrays(lines):
    """(fo[n, 8], qs[n, 2], afs[n, 2]) as the batch reports them"""
    fs = [record_facts(ln) for ln in lines]
    return (np.array([x["fo"] for x in fs], np.uint32).reshape(len(fs), 8), np.array([x["qs"] for x in fs], np.uint32).reshape(len(fs), 2),
            np.array([x["afs"] for x in fs], np.uint32).reshape(len(fs), 2))


# ---------------------------------------------------------------------------------------------- field starts
def _rep(unit, n):
    return (unit * (n // len(unit) + 1))[:n]


def _alt_of_len(n):
    """n bytes of ALT made of `,T` alleles behind a first allele of one or two bases"""
    return "G" + ",T" * ((n - 1) // 2) if n & 1 else "GA" + ",T" * ((n - 2) // 2)


def _filter_of_len(n):
    """n bytes of FILTER: PASS and `;q` tokens behind it (one `;qq` for the parity); under four bytes there is no room for PASS"""
    if n < 4:
        return "q" * n
    rem = n - 4
    assert rem != 1, "no FILTER of five bytes holds the token PASS and a second token"
    return "PASS" + (";qq" + ";q" * ((rem - 3) // 2) if rem & 1 else ";q" * (rem // 2))


_GROW = {0: lambda n: _rep("chrX", n), 1: lambda n: _rep("1234567890", n), 2: lambda n: _rep("rs77", n), 3: lambda n: _rep("ACGT", n),
         4: _alt_of_len, 6: _filter_of_len}
_BASE = ["1", "1", ".", "A", "G", ".", "PASS"]


def line_with_field_at(f, o, how, tail=""):
    """A record whose field f (1..7) starts at byte o of the line, by lengthening field `how` < f (CHROM letters, POS digits, ID
    text, REF bases, ALT `,T` alleles, FILTER `;q` tokens; never QUAL: the float parser refuses more than 400 characters).  Every
    other field is as short as a field can be.  AC_afr is 0 and every other count 5; a record whose ALT was lengthened has no AF
    entry, so its output prints one 0.0 per allele.  Convertible under keep on; under keep off too unless FILTER had to be
    shorter than PASS (f = 7 at o = 15, 16)."""
    assert 1 <= f <= 7 and 0 <= how < f and how != 5
    fields = list(_BASE)
    start_how = sum(len(x) + 1 for x in fields[:how])
    between = sum(len(x) + 1 for x in fields[how + 1:f])
    n = o - start_how - 1 - between
    assert n >= 1, (f, o, how)
    fields[how] = _GROW[how](n)
    line = refs.make_line(counts="5", overrides={"AC_afr": "0"}, af=None if how == 4 else "AF=0.5", chrom=fields[0], pos=fields[1], vid=fields[2],
                          ref=fields[3], alt=fields[4], qual=fields[5], filt=fields[6], tail=tail)
    assert len("\t".join(line.split("\t")[:f])) + 1 == o and len(line.split("\t")[how]) == n
    return line


FIELD_OFFSETS = [15, 16, 17, SWEEP - 1, SWEEP, SWEEP + 1, SWEEP + CHUNK * 7, 2 * SWEEP - 1, 2 * SWEEP, 2 * SWEEP + 1]
NINTH = "\tAC_afr=5;AF=0.9"  # behind INFO: entries the scan's `f == 7` must not read


def field_cases():
    """(f, o, how): every field at every offset; around the sweep's end with every field in front of it lengthened in turn"""
    out = []
    for f in range(1, 8):
        for o in FIELD_OFFSETS:
            near = o in (SWEEP - 1, SWEEP, SWEEP + 1)
            hows = [h for h in range(f) if h != 5] if near else [f - 1 if f - 1 != 5 else 4]
            out += [(f, o, h) for h in hows]
    return out


def field_panel():
    """The records of field_cases() three times: as they are, with a ninth field of decoys, with '\\r\\n'."""
    out = []
    for tail, end, tag in (("", "\n", ""), (NINTH, "\n", " +ninth"), ("", "\r\n", " +crlf")):
        out += [Case(f"field {f} at {o} by {h}{tag}", line_with_field_at(f, o, h, tail), end) for f, o, h in field_cases()]
    return out


def few_fields_panel():
    """Records with 7 and with 2 fields whose last tab is at 4095 / 4096, and each cut behind that tab (the tab its last byte):
    GN_FEW_FIELDS, fo = len for the missing fields.  Not convertible: a batch of their own."""
    out = []
    for tab in (SWEEP - 1, SWEEP):
        seven = "\t".join(line_with_field_at(6, tab + 1, 3).split("\t")[:7])
        two = _rep("chrX", tab) + "\t5"
        for label, line in (("7 fields", seven), ("2 fields", two)):
            assert line.rindex("\t") == tab
            out.append(Case(f"{label}, last tab at {tab}", line, "\n"))
            out.append(Case(f"{label}, last tab at {tab} and the last byte", line[:tab + 1], "\n"))
    return out


# ---------------------------------------------------------------------------------------------- ALT commas
def alt_record(alt, start, vid=".", chrom="1", front=(), k=0):
    """a record without an AF entry whose ALT is `alt` and starts at byte `start` (REF lengthened)"""
    ref_start = len(chrom) + 1 + 2 + len(vid) + 1
    n = start - 1 - ref_start
    assert n >= 1
    line = refs.make_line(counts=("0", "5", "0,3")[k % 3], overrides={"AC_eas": ("7", "0")[k & 1]}, af=None, chrom=chrom, pos=1, vid=vid, ref=_rep("ACGT", n),
                          alt=alt, front=front)
    assert line.split("\t")[4] == alt and record_facts(line)["fo"][4] == start
    return line


ALT_COUNTS = [1, 2, 16, 17, 2048, 2049, 5000]


def alleles(n):
    return ",".join(("G", "TA", "CAT")[k % 3] for k in range(n))


def alt_panel():
    out = []
    for k, n in enumerate(ALT_COUNTS):
        out.append(Case(f"{n} alleles", alt_record(alleles(n), 12 + n % 17, k=k), "\n"))
    for s in range(12, 29):  # commas at s + 1, s + 3, ...: every chunk phase over the seventeen starts
        out.append(Case(f"17 alleles from {s}", alt_record(",".join("GTCA"[k & 3] for k in range(17)), s, k=s), "\n"))
    for s in range(SWEEP - 10, SWEEP + 2):  # commas on both sides of the sweep's end
        out.append(Case(f"6 alleles from {s}", alt_record("G,T,C,A,G,T", s, k=s), "\n"))
    for n in range(1, 17):  # commas of ID and INFO around a one-byte ALT at every chunk phase
        out.append(Case(f"comma decoys, CHROM of {n}", alt_record("G", n + 12, vid="a,b,c", chrom=_rep("chrX", n), front=["x=1,2,3"], k=n), "\n"))
    return out


def comma_offsets(line):
    fo = record_facts(line)["fo"]
    return [p for p in range(fo[4], fo[5] - 1) if line[p] == ","]


# ---------------------------------------------------------------------------------------------- the AF entry
_AF_HEAD = "1\t1\t.\tA\tG,T,C\t.\tPASS\t"
AF_VALUE = "0.125,1e-05,3"


def af_line(at, entry, joint, tail=""):
    """a record whose AF entry `entry` starts at byte `at`, behind a padding entry and in front of the keys"""
    pad = at - len(_AF_HEAD) - len("pad=;")
    assert pad >= 0
    line = _AF_HEAD + ";".join(["pad=" + "x" * pad, entry] + [f"{k}={'05'[i & 1]}" for i, k in enumerate(refs.keys_of(joint))]) + tail
    assert line.index(";" + entry) + 1 == at
    return line


def af_panel(joint):
    out = []
    for at in list(range(SWEEP - 16, SWEEP + 2)) + list(range(2 * SWEEP - 2, 2 * SWEEP + 3)):
        out.append(Case(f"AF= at {at}", af_line(at, "AF=0.25", joint), "\n"))
    for split in range(1, len(AF_VALUE)):  # `split` bytes of the value in front of the sweep's end
        out.append(Case(f"AF value split at {split}", af_line(SWEEP - split - 3, "AF=" + AF_VALUE, joint), "\n"))
    last = refs.make_line(counts="5", joint=joint, chrom="1", pos=7, alt="G,T")  # AF=0.5 is its last entry
    assert last.endswith(";AF=0.5")
    out.append(Case("AF=0.5 the last bytes", last, "\n"))
    out.append(Case("AF=0.5 the last bytes of INFO, a ninth field behind", last + NINTH, "\r\n"))
    for decoy in ("XAF=0.9", "AF_joint=0.9", "AFR=0.9", "AF_=0.9"):
        out.append(Case(f"decoy {decoy}", refs.make_line(counts="0", joint=joint, front=[decoy], af="AF=0.25"), "\n"))
        out.append(Case(f"decoy {decoy} alone", refs.make_line(counts="0", joint=joint, front=[decoy], af=None, alt="G,T") + "\tAF=0.9", "\n"))
    out.append(Case("AF= twice", refs.make_line(counts="0", joint=joint, af="AF=0.25", back=["AF=0.9"]), "\n"))
    out.append(Case("AF= twice, the first at the sweep's end", af_line(SWEEP - 1, "AF=0.25", joint) + ";AF=0.9", "\n"))
    return out


def af_bare_panel():
    """`AF` without a value: the scan reports {pos + 2, 0}; the reference then fails on float(''), so each is a batch of its own
    that ends in the QUAL-or-AF message."""
    last = refs.make_line(counts="5", chrom="1", pos=7, af="AF")
    assert last.endswith(";AF")
    out = [Case("AF the last bytes", last, "\n"), Case("AF the last bytes of INFO, a ninth field behind", last + NINTH, "\n"),
           Case("AF the last bytes, crlf", last, "\r\n")]
    out += [Case(f"bare AF at {at}", af_line(at, "AF", False), "\n") for at in (SWEEP - 2, SWEEP - 1, SWEEP)]
    return out


# ---------------------------------------------------------------------------------------------- the fill pass
def out_len(line, joint=False, keep=False):
    o = refs.convert_line(line, joint, keep)
    return 0 if o is None else len(o) + 1


def wave_figures(lines, joint, keep):
    """(off[n + 1], [(a, total, route)] per 64-record wave): off the cumsum of the expected line lengths (0 for a dropped
    record), a = off[r0] & 15 (the blob's base is 16-aligned), route "staged" (a + total <= SLOT), "direct" or "empty"."""
    off = np.zeros(len(lines) + 1, np.uint64)
    off[1:] = np.cumsum([out_len(ln, joint, keep) for ln in lines], dtype=np.uint64)
    figs = []
    for r0 in range(0, len(lines), WAVE):
        r1 = min(r0 + WAVE, len(lines))
        a, total = int(off[r0]) & 15, int(off[r1] - off[r0])
        figs.append((a, total, "empty" if total == 0 else ("staged" if a + total <= SLOT else "direct")))
    return off, figs


SHORTEST = refs.make_line(counts="1", af=None, chrom="1", pos=1)
LONG_ALT = 100_000


def _natural(i):
    """a kept record of 67 .. 95 output bytes, its genotypes, AF and QUAL varying with i"""
    return refs.make_line(counts="05"[i & 1], overrides={"AC_afr": ("0", "7", "0,0,3")[i % 3], "AC_sas": ("0", "1")[(i >> 2) & 1]}, chrom="1", pos=1 + i,
                          af=(None, "AF=0.5", "AF=0.125,1e-05")[i % 3], alt=("G", "G,T")[(i >> 1) & 1], qual=(".", "30")[(i >> 3) & 1])


def _dropped(i):
    return refs.make_line(counts="5", chrom="1", pos=1 + i, filt=("AC0", ".", "NOPASS")[i % 3])


def _padded(line, k):
    """the record with k more bases of REF: k more bytes of output"""
    assert k >= 0
    f = line.split("\t")
    f[3] += _rep("CGTA", k)
    return "\t".join(f)


class _Waves:
    """a batch built wave by wave; `named[name]` is the wave's index"""

    def __init__(self):
        self.lines, self.named, self.pos = [], {}, 0

    def wave(self, name, total=None, kept=range(WAVE), n=WAVE, special=None):
        """n records of which the lanes `kept` are kept; the last kept lane's REF is padded so that the wave's lines are `total` bytes"""
        assert len(self.lines) % WAVE == 0 and name not in self.named
        r0, kept = len(self.lines), sorted(kept)
        recs = {lane: (special or {}).get(lane) or _natural(r0 + lane) for lane in kept}
        have = sum(out_len(r) for r in recs.values())
        if total is not None:
            recs[kept[-1]] = _padded(recs[kept[-1]], total - have)
            have = total
        self.lines += [recs.get(lane) or _dropped(r0 + lane) for lane in range(n)]
        self.named[name] = r0 // WAVE
        self.pos += have

    def staged_to_phase(self, name, a):
        """a staged wave that leaves the next wave at phase a"""
        self.wave(name, total=5600 + ((a - self.pos - 5600) & 15))
        assert self.pos & 15 == a


def fill_panel():
    """(lines, named) of the main batch, keep off.  Its waves, in order (the figures are asserted in tests/test_gnomad_seams.py):
    16 staged waves of totals = 1 (mod 16): phases 0..15, the ranges of the first and the last ending one byte past and exactly
    on a 16-byte boundary; 16 direct waves likewise; a + total = 8192 (staged) and 8193 (direct) at a = 0 and at a = 15; 64
    dropped records between two kept waves; only lane 0, only lane 63, every second lane kept; one 100 000-byte ALT among 63
    short lines; a single record of the shortest line there is (67 bytes: no wave's lines can be shorter than a 16-byte piece
    plus its edges); and as the last workgroup a direct wave, an empty one, a wave of ONE record and a wave beyond n."""
    w = _Waves()
    for j in range(16):
        w.wave(f"staged phase {j}", total=5601 + 16 * (j % 3))
    for j in range(16):
        w.wave(f"direct phase {j}", total=SLOT + 17 + 16 * (j % 3))
    assert w.pos & 15 == 0
    w.wave("a=0 sum 8192", total=SLOT)
    w.wave("a=0 sum 8193", total=SLOT + 1)
    w.staged_to_phase("to 15 (1)", 15)
    w.wave("a=15 sum 8192", total=SLOT - 15)
    w.staged_to_phase("to 15 (2)", 15)
    w.wave("a=15 sum 8193", total=SLOT - 14)
    w.wave("kept before empty")
    w.wave("empty", kept=[])
    w.wave("kept after empty")
    w.wave("lane 0 only", kept=[0])
    w.wave("lane 63 only", kept=[63])
    w.wave("alternating", kept=range(0, WAVE, 2))
    big = refs.make_line(counts="5", chrom="1", pos=99, alt=_rep("ACGT", LONG_ALT), af=None)
    w.wave("long ALT", special={31: big})
    w.wave("shortest alone", kept=[17], special={17: SHORTEST})
    while (len(w.lines) // WAVE) % WG_WAVES:
        w.wave(f"filler {len(w.lines) // WAVE}")
    w.wave("last workgroup: direct", total=SLOT + 500)
    w.wave("last workgroup: empty", kept=[])
    w.wave("last workgroup: one record", kept=[0], n=1)
    return w.lines, w.named


def fill_panel_63():
    """(lines, named) of the second batch: an empty, a direct and two staged waves, then a last wave of 63 records"""
    w = _Waves()
    w.wave("empty", kept=[])
    w.wave("direct", total=SLOT + 3)
    w.wave("staged")
    w.wave("staged 2", kept=range(1, WAVE, 2))
    w.wave("63 records", n=WAVE - 1, kept=range(WAVE - 1))
    return w.lines, w.named
