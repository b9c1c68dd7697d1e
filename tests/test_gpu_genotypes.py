"""The VCF genotype kernels (hawk_vcf.hip) at their sweep, wave and column seams.
k_gt_parse against oracle.vcf_genotype_codes (pinned to the reference's VariantRecord.read_vcf_line by G8 / G12) on codes AND
flags; k_gt_count / k_gt_fill against the vectorised statement of oracle.carried_lists in genotype_refs.py (proved equal to
it in test_genotype_refs.py).  Every seam-named case asserts from genotype_refs.field_seams that its input holds the seam."""
import ctypes as C

import numpy as np
import pytest

import genotype_refs as gr
from oracle import oracle as ora

pytestmark = pytest.mark.gpu

HEAD = b"chrV\t77\t.\tA\tC,G,T\t.\tPASS\t.\tGT\t"
TAIL_CHARS = np.frombuffer(b"0123456789|/.:abXY-+", dtype=np.uint8)


def _L():
    from crisprhawk_hip import _lib
    return _lib, _lib.lib(), _lib.context(None)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------------ text builders
def _field(rng, tail=True):
    """one genotype of the grammar: alleles of 1 to 3 digits or '.', '|' between them, optionally ':' and 0 to 20 bytes that
    may hold digits, separators, dots and further colons"""
    def allele():
        if rng.random() < 0.08:
            return b"."
        return str(int(rng.integers(0, 10 ** int(rng.integers(1, 4))))).encode()
    f = allele() + b"|" + allele()
    if tail and rng.random() < 0.5:
        f += b":" + TAIL_CHARS[rng.integers(0, len(TAIL_CHARS), int(rng.integers(0, 21)))].tobytes()
    return f


def _pad_field(rng, width):
    """a well-formed field of exactly `width` >= 3 bytes"""
    assert width >= 3
    return b"0|1" if width == 3 else b"1|2:" + TAIL_CHARS[rng.integers(0, len(TAIL_CHARS), width - 4)].tobytes()


def _section(rng, length):
    """a list of well-formed fields whose tab-joined text is exactly `length` >= 3 bytes long"""
    fields, cur = [], 0
    while length - cur > 60:
        fields.append(_field(rng))
        cur += len(fields[-1]) + 1
    fields.append(_pad_field(rng, length - cur))
    assert len(b"\t".join(fields)) == length
    return fields


def _start_at(rng, rel, field, after=3):
    """fields such that `field` starts exactly `rel` bytes into the section (the tab before it is byte rel - 1)"""
    fields = _section(rng, rel - 1) + [field] + [_field(rng) for _ in range(after)]
    return fields, len(fields) - after - 1


class Batch:
    """records -> the arguments of hawk_gt_parse; every record is HEAD + its section + its terminator"""

    def __init__(self):
        self.chunks, self.line_off, self.gt_off, self.n = [], [0], [], 0

    def add(self, section, term=b"\n", gt_shift=0, head=HEAD):
        sec = section if isinstance(section, bytes) else b"\t".join(section)
        self.gt_off.append(self.line_off[-1] + len(head) + gt_shift)
        self.chunks.append(head + sec + term)
        self.line_off.append(self.line_off[-1] + len(self.chunks[-1]))
        self.n += 1
        return self.n - 1

    def arrays(self):
        return b"".join(self.chunks), np.array(self.line_off, np.uint64), np.array(self.gt_off, np.uint64)

    def seams(self, i):
        text = b"".join(self.chunks)
        return gr.field_seams(text, self.gt_off[i], self.line_off[i + 1])


def _device_parse(text, line_off, gt_off, n_samples):
    _lib, L, ctx = _L()
    buf = np.frombuffer(text, dtype=np.uint8) if len(text) else np.zeros(1, np.uint8)
    n = len(gt_off)
    g, ms = C.c_void_p(), C.c_float()
    _lib.check(L.hawk_gt_parse(ctx, _p(buf), C.c_uint64(len(text)), _p(line_off), _p(gt_off), C.c_uint64(n), n_samples, C.byref(g),
                               C.byref(ms)), "hawk_gt_parse")
    codes = np.zeros((n, 2 * n_samples), dtype=np.uint8)
    flags = np.full(n, 0xee, dtype=np.uint8)
    try:
        _lib.check(L.hawk_gt_codes(g, _p(codes), _p(flags)), "hawk_gt_codes")
    except Exception:
        L.hawk_gt_destroy(g)
        raise
    return g, codes, flags


def _want(text, line_off, gt_off, n_samples):
    recs = [gr.oracle_record(text, int(gt_off[i]), int(line_off[i + 1])) for i in range(len(gt_off))]
    return ora.vcf_genotype_codes(recs, n_samples)


def _check_batch(b, n_samples, keep=False):
    """device == parse reference on codes and flags of every record; -> (codes, flags[, handle])"""
    text, line_off, gt_off = b.arrays()
    want, wflags = _want(text, line_off, gt_off, n_samples)
    g, codes, flags = _device_parse(text, line_off, gt_off, n_samples)
    try:
        bad = np.flatnonzero(flags != wflags)
        assert len(bad) == 0, f"flags differ on records {bad[:8].tolist()}: device {flags[bad[:8]].tolist()} reference {wflags[bad[:8]].tolist()}"
        if not np.array_equal(codes, want):
            r, c = np.argwhere(codes != want)[0]
            rel, sweep, thread, phase = b.seams(int(r))
            s = int(c) // 2
            where = (int(rel[s]), int(sweep[s]), int(thread[s]), int(phase[s])) if s < len(rel) else None
            fields = gr.section_fields(text, int(gt_off[r]), int(line_off[r + 1]))
            raise AssertionError(f"codes differ: record {r} sample {s} copy {c % 2}: device {codes[r, c]} reference {want[r, c]}; field "
                                 f"{fields[s] if s < len(fields) else None!r} at (rel, sweep, thread, phase) = {where}")
    except Exception:
        _L()[1].hawk_gt_destroy(g)
        raise
    if keep:
        return codes, flags, g
    _L()[1].hawk_gt_destroy(g)
    return codes, flags


# ------------------------------------------------------------------------------------------------ k_gt_parse
@pytest.mark.parametrize("length", [4095, 4096, 4097, 8191, 8192, 8193, 4 * 4096 + 77])
def test_parse_sweep_lengths_and_terminators(length):
    """Sections that end one byte before, on and one byte behind a sweep seam; '\\n', '\\r\\n' and nothing behind the last record."""
    rng = np.random.default_rng(8100 + length)
    fields = _section(rng, length)
    for term in (b"\n", b"\r\n", b""):
        b = Batch()
        b.add([b"0|1"] * 3)           # a short record in front: the wide one is not record 0
        i = b.add(fields, term)
        text, line_off, gt_off = b.arrays()
        assert gr.section_bounds(text, int(gt_off[i]), int(line_off[i + 1]))[1] - int(gt_off[i]) == length
        assert gr.n_sweeps(text, int(gt_off[i]), int(line_off[i + 1])) == -(-length // gr.SWEEP)
        codes, flags = _check_batch(b, len(fields))
        assert flags.tolist() == [2, 0] and (codes[0, 6:] == 255).all()


def test_parse_every_chunk_phase_and_sweep_seam():
    """Field starts at each of the 16 byte phases of a chunk, at byte 0 of thread 0 of a later sweep (the tab is the last byte
    of the sweep before, `prev` comes from there), and in the last thread of a sweep."""
    rng = np.random.default_rng(8201)
    b, marks = Batch(), []
    for rel in (gr.SWEEP, 2 * gr.SWEEP):                      # phase 0 of thread 0 of sweeps 1 and 2
        fields, k = _start_at(rng, rel, b"12|3:7")
        marks.append((b.add(fields), k, rel, len(fields)))
    for ph in (0, 7, 15):                                       # the last thread of sweep 0 and of sweep 1
        for sw in (0, 1):
            rel = sw * gr.SWEEP + gr.SWEEP - gr.CHUNK + ph
            fields, k = _start_at(rng, rel, b"3|21")
            marks.append((b.add(fields), k, rel, len(fields)))
    for ph in range(16):                                        # every phase, in sweep 1
        rel = gr.SWEEP + 16 * (3 + ph) + ph
        fields, k = _start_at(rng, rel, b".|105:x")
        marks.append((b.add(fields), k, rel, len(fields)))
    ns = max(m[3] for m in marks)
    seen_phase = set()
    for i, k, want_rel, _ in marks:
        rel, sweep, thread, phase = b.seams(i)
        assert rel[k] == want_rel
        seen_phase.add(int(phase[k]))
    assert seen_phase == set(range(16))
    rel, sweep, thread, phase = b.seams(marks[0][0])
    k = marks[0][1]
    assert (sweep[k], thread[k], phase[k]) == (1, 0, 0) and b.chunks[marks[0][0]][len(HEAD) + gr.SWEEP - 1:len(HEAD) + gr.SWEEP] == b"\t"
    rel, sweep, thread, phase = b.seams(marks[1][0])
    assert (sweep[marks[1][1]], thread[marks[1][1]], phase[marks[1][1]]) == (2, 0, 0)
    rel, sweep, thread, phase = b.seams(marks[2][0])
    assert (sweep[marks[2][1]], thread[marks[2][1]]) == (0, gr.THREADS - 1)
    codes, flags = _check_batch(b, ns)
    for i, k, _, n in marks:
        assert flags[i] == (0 if n == ns else 2)
    assert codes[marks[0][0], 2 * marks[0][1]] == 12 and codes[marks[0][0], 2 * marks[0][1] + 1] == 3


def test_parse_tokens_straddling_chunk_and_sweep_seams():
    """A multi-digit allele, the '|' and a ':'-tail each lying across a 16-byte chunk seam and across a 4096-byte sweep seam."""
    rng = np.random.default_rng(8202)
    b, marks = Batch(), []
    for unit, seam in ((gr.CHUNK, 16 * 40), (gr.CHUNK, gr.SWEEP + 16 * 9), (gr.SWEEP, gr.SWEEP), (gr.SWEEP, 2 * gr.SWEEP)):
        cases = [(seam - 2, b"123|45", 0, 3),            # first allele: bytes seam-2 .. seam
                 (seam - 4, b"7|100:q", 2, 3),           # second allele across the seam
                 (seam - 2, b"12|99", 0, 3),             # '|' is the first byte behind the seam: "12" / "|99"
                 (seam - 4, b"120|9", 3, 1),             # '|' is the last byte before the seam (checked with its right neighbour)
                 (seam - 6, b"1|2:ab|/.9:77", 3, 10)]    # the tail across the seam
        for rel, field, tok_off, tok_len in cases:
            fields, k = _start_at(rng, rel, field)
            i = b.add(fields)
            marks.append((i, k, rel, unit, tok_off, tok_len, field))
    for i, k, want_rel, unit, tok_off, tok_len, field in marks:
        rel = b.seams(i)[0]
        assert rel[k] == want_rel and gr.section_fields(b.chunks[i], len(HEAD), len(b.chunks[i]))[k].encode() == field
        span = tok_len + 1 if field == b"120|9" else tok_len   # the bar and the byte behind it
        assert gr.crosses(int(rel[k]) + tok_off, span, unit), (field, want_rel, unit)
        if field == b"12|99":
            assert (int(rel[k]) + 2) % unit == 0               # the bar itself opens the chunk / the sweep
        if field == b"120|9":
            assert (int(rel[k]) + 3) % unit == unit - 1        # the bar closes it
    ns = max(len(gr.section_fields(c, len(HEAD), len(c))) for c in b.chunks)
    codes, flags = _check_batch(b, ns)
    assert not (flags & 5).any()
    i, k = marks[0][0], marks[0][1]
    assert codes[i, 2 * k:2 * k + 2].tolist() == [123, 45]


def test_parse_field_count_decided_in_a_later_sweep():
    rng = np.random.default_rng(8301)
    fields = _section(rng, 2 * gr.SWEEP + 500)
    n = len(fields)
    b = Batch()
    i = b.add(fields)
    rel, sweep, _, _ = b.seams(i)
    assert len(rel) == n and sweep[n - 2] == 2 and sweep[n - 1] == 2 and sweep[0] == 0  # the deciding fields lie in sweep 2
    for ns, flag in ((n - 1, 2), (n, 0), (n + 1, 2)):
        codes, flags = _check_batch(b, ns)
        assert flags[0] == flag
        if ns == n + 1:
            assert codes[0, 2 * n:].tolist() == [255, 255] and (codes[0, :2 * n] != 255).any()
    # a trailing tab: one more field, empty - the genotype "" is one part and no number (flags 1 | 4), its codes are 255
    b = Batch()
    i = b.add(b"\t".join(fields) + b"\t")
    rel = b.seams(i)[0]
    assert len(rel) == n + 1 and rel[-1] == 2 * gr.SWEEP + 501
    codes, flags = _check_batch(b, n + 1)
    assert flags[0] == 5 and codes[0, 2 * n:].tolist() == [255, 255]
    codes, flags = _check_batch(b, n)          # the empty field is beyond the samples: the count alone is wrong
    assert flags[0] == 2
    codes, flags = _check_batch(b, n + 2)
    assert flags[0] == 7 and (codes[0, 2 * n:] == 255).all()


def test_parse_empty_fields_gt_off_on_a_tab_and_no_section():
    rng = np.random.default_rng(8302)
    b = Batch()
    r_mid = b.add([b"0|1", b"", b"1|0"])                                  # empty field in the middle
    fields, k = _start_at(rng, gr.SWEEP, b"", after=2)                     # the same on a sweep seam: tab, tab
    bs = Batch()
    bs.add(fields)
    rel, sweep, thread, phase = bs.seams(0)
    assert rel[k] == gr.SWEEP and rel[k + 1] == gr.SWEEP + 1 and (sweep[k], thread[k], phase[k]) == (1, 0, 0)
    codes, flags = _check_batch(bs, len(fields))
    assert flags[0] == 5 and codes[0, 2 * k:2 * k + 2].tolist() == [255, 255] and (codes[0, 2 * k + 2:2 * k + 4] != 255).any()
    r_tab = b.add([b"2|1", b"0|3"], gt_shift=-1)                           # gt_off points at the tab in front of the first sample
    r_none = b.add(b"", term=b"")                                          # gt_off == line_off[i + 1]: no section at all
    r_nl = b.add(b"", term=b"\r\n")                                        # only the terminator behind gt_off
    r_last = b.add([b"1|1", b"0|2", b"3|0"], term=b"")                     # a good record behind them, unterminated
    text, line_off, gt_off = b.arrays()
    assert gt_off[r_none] == line_off[r_none + 1] and text[int(gt_off[r_tab]):int(gt_off[r_tab]) + 1] == b"\t"
    assert gr.section_fields(text, int(gt_off[r_tab]), int(line_off[r_tab + 1])) == ["", "2|1", "0|3"]
    codes, flags = _check_batch(b, 3)
    assert flags[[r_mid, r_tab, r_none, r_nl, r_last]].tolist() == [5, 5, 2, 2, 0]
    assert codes[r_mid].tolist() == [0, 1, 255, 255, 1, 0] and codes[r_tab].tolist() == [255, 255, 2, 1, 0, 3]
    assert (codes[r_none] == 255).all() and (codes[r_nl] == 255).all() and codes[r_last].tolist() == [1, 1, 0, 2, 3, 0]


@pytest.mark.parametrize("n_samples", [1, 2, 37, 1023, 1024, 1025, 2504])
def test_parse_widths(n_samples):
    rng = np.random.default_rng(8400 + n_samples)
    b = Batch()
    for r in range(5):
        b.add([_field(rng, tail=(r % 2 == 0)) for _ in range(n_samples)], term=b"\r\n" if r == 3 else b"\n")
    if n_samples == 2504:
        text, line_off, gt_off = b.arrays()
        assert gr.n_sweeps(text, int(gt_off[0]), int(line_off[1])) >= 3   # the panel's width: three sweeps and more
    codes, flags = _check_batch(b, n_samples)
    assert not flags.any()


def test_parse_many_short_records():
    """The per-megabase record count: blockIdx.x in the tens of thousands, every record short."""
    rng = np.random.default_rng(8450)
    pool = [[_field(rng) for _ in range(3)] for _ in range(97)] + [[b"0|1", b"1"], [b"0|1", b"1|0", b"2|2", b"0|0"], [b"0/1", b"x|1", b""]]
    b = Batch()
    for k in rng.integers(0, len(pool), 20011):
        b.add(pool[int(k)])
    codes, flags = _check_batch(b, 3)
    assert set(flags.tolist()) == {0, 2, 3, 5}


def test_parse_on_a_recycled_dirty_block():
    """Codes live in pool memory: a block freed full of alleles and handed out again must still read 255 where a short record
    has no sample."""
    rng = np.random.default_rng(8500)
    ns, nl = 600, 8
    full = Batch()
    for _ in range(nl):
        full.add([b"%d|%d" % (int(rng.integers(1, 4)), int(rng.integers(1, 4))) for _ in range(ns)])
    codes, flags = _check_batch(full, ns)
    assert not flags.any() and (codes != 255).all()
    for _ in range(2):   # the handle above is destroyed: the next block of this size is the dirty one, if the pool recycles
        short = Batch()
        for r in range(nl):
            short.add([b"1|2"] * (1 + r))
        codes, flags = _check_batch(short, ns)
        assert (flags == 2).all()
        for r in range(nl):
            assert (codes[r, :2 * (1 + r)].reshape(-1, 2) == [1, 2]).all() and (codes[r, 2 * (1 + r):] == 255).all()


def test_parse_allele_numbers_clamp_at_254():
    """0 REF, k = k-th ALT, every number >= 254 reads 254 (255 is kept for missing), leading zeros are numbers."""
    vals = ["0", "9", "10", "99", "100", "253", "254", "255", "256", "4294967296", "9" * 30, "007", "0000", "00256", "0" * 25 + "31"]
    want = [0, 9, 10, 99, 100, 253, 254, 254, 254, 254, 254, 7, 0, 254, 31]
    fields = [f"{a}|{vals[-1 - i]}".encode() for i, a in enumerate(vals)] + [f".|{a}:{a}".encode() for a in vals]
    b = Batch()
    b.add(fields)
    codes, flags = _check_batch(b, len(fields))
    assert flags[0] == 0
    n = len(vals)
    assert codes[0, 0:2 * n:2].tolist() == want and codes[0, 1:2 * n:2].tolist() == want[::-1]
    assert (codes[0, 2 * n::2] == 255).all() and codes[0, 2 * n + 1::2].tolist() == want


# Malformed genotypes, by class -> (string, flags).  Bit 1 is the reference's arity refusal (variant.py:514-520: the genotype
# split at '|' is not two parts), bit 4 says that one of the first two parts is no number; where the reference raises the arity
# error it never looks at the alleles, so 4 next to 1 is this project's addition and 1 decides the message.  Two '|'-parts of
# which one is no number ("|1", "0|1/2", "0/1|2", "0|") fail in the reference's int(): 4 alone.  The reference's int() would
# take "+1" or " 1"; alleles here are digits only, as the VCF specification has them.
MALFORMED = {
    "unphased": [("0/1", 1), ("./.", 1), ("12/3:5", 1)],
    "haploid": [("1", 1), (".", 1), ("17:0|1", 1)],
    "triploid": [("0|1|2", 1), ("0/1/2", 1), ("0|1|x", 1), ("0|x|2", 5), ("0|1|", 1), ("1||2", 5)],
    "mixed_separators": [("0|1/2", 4), ("0/1|2", 4), ("0/1|2/3", 4), ("0|1/2|3", 5)],
    "leading_separator": [("|1", 4), ("/1", 5), ("|", 4), ("/", 5)],
    "trailing_separator": [("0|", 4), ("0/", 5), ("0|:9", 4)],
    "empty": [("", 5), (":0|1", 5)],
    "letters": [("x", 5), ("a|b", 4), ("0|x", 4), ("x|0", 4), ("1a|0", 4), ("0|1a", 4), ("0|1 ", 4)],
    "signs": [("+1|0", 4), ("0|-1", 4), ("-1", 5), ("0|1+", 4)],
    "dots": [(".|.", 0), ("..|1", 4), ("0|..", 4), (".1|0", 4), ("0|1.", 4), ("...", 5)],
}
# classes whose codes are NOT compared with the reference (flags always are): none - gt_classify and the oracle state one rule
CODES_EXEMPT = frozenset()


@pytest.mark.parametrize("cls", sorted(MALFORMED))
def test_parse_malformed_genotypes_by_class(cls):
    text_of = lambda b, i: b.chunks[i]
    b, expect = Batch(), []
    for s, fl in MALFORMED[cls]:
        for slot in range(3):     # first, middle and last field of the record
            f = [b"0|1", b"2|0", b"1|1"]
            f[slot] = s.encode()
            i = b.add(f, term=b"\r\n" if slot == 1 else b"\n")
            assert gr.section_fields(text_of(b, i), len(HEAD), len(text_of(b, i)))[slot] == s
            expect.append(fl)
    text, line_off, gt_off = b.arrays()
    want, wflags = _want(text, line_off, gt_off, 3)
    assert wflags.tolist() == expect          # the parse reference follows the table ...
    g, codes, flags = _device_parse(text, line_off, gt_off, 3)
    _L()[1].hawk_gt_destroy(g)
    assert ((flags != 0) == (wflags != 0)).all()      # ... the device accepts and rejects the same strings ...
    assert flags.tolist() == expect                   # ... with the same bits ...
    if cls not in CODES_EXEMPT:
        assert np.array_equal(codes, want)            # ... and the same codes


def test_parse_reference_fixture_at_panel_width():
    """G12: records of 2504 samples read by the reference's own VariantRecord.read_vcf_line (three sweeps and more per record,
    multi-digit alleles, ':'-tails of varying length, '.' alleles, three ALT alleles): the per-allele sample sets the
    reference built must follow from the device codes."""
    from util import load_golden
    fx = load_golden("g12_vcf_wide.json.gz")
    samples = fx["samples"]
    ns = len(samples)
    assert ns >= 2504
    b = Batch()
    for rec in fx["records"]:
        head = ("\t".join(rec["fields"][:9]) + "\t").encode()
        b.add([x.encode() for x in rec["fields"][9:]], head=head)
    text, line_off, gt_off = b.arrays()
    assert min(gr.n_sweeps(text, int(gt_off[i]), int(line_off[i + 1])) for i in range(b.n)) >= 3
    codes, flags = _check_batch(b, ns)
    assert not flags.any()
    names = np.array(samples)
    for i, rec in enumerate(fx["records"]):
        for k in range(len(rec["alt"])):
            for c in range(2):
                assert sorted(names[np.flatnonzero(codes[i, c::2] == k + 1)].tolist()) == rec["samples"][k][c]


def test_parse_refusals_launch_nothing_and_leave_the_library_usable():
    _lib, L, ctx = _L()
    b = Batch()
    b.add([b"0|1", b"1|0"])
    b.add([b"1|1", b"0|2"])
    text, line_off, gt_off = b.arrays()
    buf = np.frombuffer(text, dtype=np.uint8)
    n = len(text)

    def status(text_len=n, lo=line_off, go=gt_off, ns=2, tx=buf):
        g = C.c_void_p()
        st = L.hawk_gt_parse(ctx, _p(tx), C.c_uint64(text_len), _p(lo), _p(go), C.c_uint64(2), ns, C.byref(g), None)
        assert g.value is None or st == 0
        if g.value:
            L.hawk_gt_destroy(g)
        return st

    mod = lambda a, i, v: np.concatenate([a[:i], np.array([v], np.uint64), a[i + 1:]])
    assert status() == 0
    assert status(text_len=n - 1) == _lib.HAWK_E_INVALID                                   # line_off beyond text_len
    assert status(lo=mod(line_off, 1, line_off[0])) == _lib.HAWK_E_INVALID                 # an empty line
    assert status(lo=mod(line_off, 1, line_off[2] + np.uint64(1))) == _lib.HAWK_E_INVALID  # descending / beyond the text
    assert status(go=mod(gt_off, 1, line_off[1] - np.uint64(1))) == _lib.HAWK_E_INVALID    # gt_off before its line
    assert status(go=mod(gt_off, 0, line_off[1] + np.uint64(1))) == _lib.HAWK_E_INVALID    # gt_off behind its line
    assert status(ns=0) == _lib.HAWK_E_INVALID
    assert status(tx=None) == _lib.HAWK_E_INVALID and status(lo=None) == _lib.HAWK_E_INVALID and status(go=None) == _lib.HAWK_E_INVALID
    codes, flags = _check_batch(b, 2)
    assert not flags.any() and codes.tolist() == [[0, 1, 1, 0], [1, 1, 0, 2]]


def test_files_to_device_haplotypes_at_panel_width(tmp_path):
    """VCF file -> device parser -> lists -> expansion against the in-memory route, at 1100 samples (records of about 9 kB: three
    sweeps), every record multi-allelic (a first ALT allele nobody carries, the carried one second, so genotypes read 0|2) and
    every genotype with a ':'-tail."""
    from crisprhawk_hip import readers, synth
    from crisprhawk_hip.workload import expand_from_vcf, expand_on_device
    rng = np.random.default_rng(8801)
    reg = synth.make_region(8802, "chrW", 24_000, 3_000, 21_000)
    synth.add_phased_variants(reg, 8803, 160, 1100, af_min=0.002, af_max=0.2)
    rows = []
    for v in reg.variants:
        f = reg.vcf_fields(v)
        if len(v.ref) == 1 and len(v.alt) == 1:
            other = [x for x in "ACGT" if x not in (v.ref.upper(), v.alt.upper())][0]
            f[4] = other + "," + v.alt
            f[7] = f"AF=0,{v.af:.6g}"
            gts = [g.replace("1", "2") for g in f[9:]]
        else:
            gts = f[9:]
        f[8] = "GT:DP:PL"
        tails = rng.integers(0, 10 ** 9, len(gts))
        rows.append(f[:9] + [f"{g}:{int(t) % 97}:{str(int(t))[:int(t) % 9]}" for g, t in zip(gts, tails)])
    fa, bed, vcf = str(tmp_path / "r.fa"), str(tmp_path / "r.bed"), str(tmp_path / "v.vcf")
    readers.write_fasta(fa, reg.contig, reg.contig_seq, 60)
    with open(bed, "w") as fh:
        fh.write(f"{reg.contig}\t{reg.bed_start}\t{reg.bed_stop}\n")
    readers.write_vcf(vcf, reg.contig, reg.samples, rows, False)
    coord = readers.Bed(bed, synth.PADDING)[0]
    seq = readers.Fasta(fa).fetch(coord).sequence
    v = readers.VCF(vcf)
    blk = v.fetch_block(coord)
    assert len(blk) == len(rows) and len(v.samples) == 1100
    text = bytes(blk.text)
    assert min(gr.n_sweeps(text, int(blk.gt_off[i]), int(blk.line_off[i + 1])) for i in range(len(blk))) >= 3
    ds1, info1, ms, kept1, vt = expand_from_vcf(seq, coord.start, coord.stop, blk, v.samples, 3, v.phased)
    ds0, info0, _, kept0 = expand_on_device(reg, 3)
    assert len(vt) > len(reg.variants) and int(vt.allele.max()) == 2
    assert kept0 == kept1 and len(kept0) > 200 and [i.samples for i in info0] == [i.samples for i in info1]
    ids = [f"{reg.contig}-{s.pos}-{s.ref}/{s.alt}" for s in reg.variants]
    assert all([ids[int(j)] for j in a.variant_idx] == [vt.id[int(j)] for j in b.variant_idx] for a, b in zip(info0, info1))
    assert np.array_equal(ds0.planes(), ds1.planes())


# ------------------------------------------------------------------------------------------------ hawk_gt_lists
class Lists:
    """a hawk_gt handle from a code matrix, and hawk_gt_lists on it against the lists reference"""

    def __init__(self, codes=None, handle=None, n_samples=None):
        self._lib, self.L, ctx = _L()
        if handle is not None:
            self.g, self.n_cols = handle, 2 * n_samples
            return
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        self.n_cols = codes.shape[1]
        self.g = C.c_void_p()
        self._lib.check(self.L.hawk_gt_from_codes(ctx, _p(codes), C.c_uint64(codes.shape[0]), self.n_cols // 2, C.byref(self.g)),
                        "hawk_gt_from_codes")

    def close(self):
        if self.g is not None:
            self.L.hawk_gt_destroy(self.g)
            self.g = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def status(self, vl, va, r0, ch, n_var=None, with_off=True):
        col_off = np.zeros(self.n_cols + 1, dtype=np.uint64)
        return self.L.hawk_gt_lists(self.g, _p(vl), _p(va), _p(r0), _p(ch), len(vl) if n_var is None else n_var,
                                    _p(col_off) if with_off else None, None, None)

    def run(self, vl, va, r0, ch):
        vl, va = np.ascontiguousarray(vl, np.uint32), np.ascontiguousarray(va, np.uint8)
        r0, ch = np.ascontiguousarray(r0, np.int32), np.ascontiguousarray(ch, np.int32)
        col_off = np.full(self.n_cols + 1, 0xdead, dtype=np.uint64)
        delta = np.full(self.n_cols, -77, dtype=np.int64)
        ms = C.c_float()
        self._lib.check(self.L.hawk_gt_lists(self.g, _p(vl), _p(va), _p(r0), _p(ch), len(vl), _p(col_off), _p(delta), C.byref(ms)),
                        "hawk_gt_lists")
        ne = int(col_off[-1])
        idx, o = np.full(ne + 2, 0xabcdef, np.uint32), np.full(ne + 2, -5, np.int32)   # two guard words behind the lists
        self._lib.check(self.L.hawk_gt_lists_download(self.g, _p(idx), _p(o)), "hawk_gt_lists_download")
        assert idx[ne:].tolist() == [0xabcdef] * 2 and o[ne:].tolist() == [-5, -5]
        ni = C.c_uint64(1 << 40)
        self._lib.check(self.L.hawk_gt_lists_indels(self.g, None, C.c_uint64(0), C.byref(ni)), "hawk_gt_lists_indels")
        ind = np.full(ni.value + 2, 0xfeed, np.uint32)
        self._lib.check(self.L.hawk_gt_lists_indels(self.g, _p(ind), C.c_uint64(ni.value), C.byref(ni)), "hawk_gt_lists_indels")
        assert ind[ni.value:].tolist() == [0xfeed] * 2
        return col_off, idx[:ne], o[:ne], delta, ind[:ni.value]

    def check(self, codes, vl, va, r0, ch):
        got = self.run(vl, va, r0, ch)
        want = gr.carried_lists_np(codes, vl, va, r0, ch)
        for name, a, w in zip(("col_off", "hv_idx", "hv_o", "col_delta", "indel entries"), got, want):
            if not np.array_equal(a, w):
                m = min(len(a), len(w))
                diff = np.flatnonzero(a[:m] != w[:m])
                k = int(diff[0]) if len(diff) else m
                col = int(np.searchsorted(want[0], k, side="right") - 1) if name in ("hv_idx", "hv_o") else k
                raise AssertionError(f"{name} differs (lengths {len(a)} / {len(w)}) first at {k} (column {col}): "
                                     f"device {a[k:k + 4].tolist()} reference {w[k:k + 4].tolist()}")
        return got


def _panel(rng, n_lines, n_cols, max_alt=1, af_lo=0.002, af_hi=0.5, missing=0.01):
    """codes by allele frequency: log-uniform per line, so most columns carry few variants"""
    af = np.exp(rng.uniform(np.log(af_lo), np.log(af_hi), n_lines))
    u = rng.random((n_lines, n_cols))
    codes = np.zeros((n_lines, n_cols), np.uint8)
    carried = u < af[:, None]
    codes[carried] = rng.integers(1, max_alt + 1, int(carried.sum()))
    codes[u > 1 - missing] = 255
    return codes


def _variants(rng, n_var, n_lines=None, chain_lim=12, frac_indel=0.3):
    vl = np.arange(n_var, dtype=np.uint32) if n_lines is None else np.sort(rng.integers(0, n_lines, n_var)).astype(np.uint32)
    va = np.ones(n_var, np.uint8)
    r0 = (np.arange(n_var, dtype=np.int64) * 40 + 100).astype(np.int32)
    ch = (rng.integers(-chain_lim, chain_lim + 1, n_var) * (rng.random(n_var) < frac_indel)).astype(np.int32)
    return vl, va, r0, ch


@pytest.mark.parametrize("n_samples", [1, 31, 32, 33, 63, 64, 65, 2504])
def test_lists_grid_of_column_and_variant_counts(n_samples):
    """Columns 2 .. 5008 (below, on and above the 64-column wave of k_gt_count) x variants 1 .. 2049 (the 64-variant chunk, the
    256-variant wave and the 1024-variant blockIdx.y, each at -1 / 0 / +1)."""
    n_cols = 2 * n_samples
    for n_var in (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049):
        rng = np.random.default_rng(9000 + 7 * n_samples + n_var)
        codes = _panel(rng, n_var, n_cols)
        codes[n_var - 1, rng.integers(0, n_cols)] = 1     # the last variant is carried somewhere
        codes[0, n_cols - 1] = 1                           # and the first one by the last column
        vl, va, r0, ch = _variants(rng, n_var)
        ch[-1] = -4
        with Lists(codes) as h:
            col_off, idx, o, delta, ind = h.check(codes, vl, va, r0, ch)
        assert col_off[-1] >= 1 and (idx == n_var - 1).any() and len(ind) >= 1


def test_lists_product_sized():
    """About 31 000 variants (31 blockIdx.y of k_gt_count, 485 chunks per column in k_gt_fill) x 600 columns."""
    rng = np.random.default_rng(9100)
    n_var, n_cols = 31013, 600
    codes = _panel(rng, n_var, n_cols, af_hi=0.3)
    vl, va, r0, ch = _variants(rng, n_var)
    with Lists(codes) as h:
        col_off, idx, o, delta, ind = h.check(codes, vl, va, r0, ch)
    assert col_off[-1] > 100_000 and len(ind) > 10_000


def test_lists_column_extremes():
    """Empty first / last column and an empty 64-column group, a column carrying everything, only variant 0, only the last
    variant, a first carried variant behind all-zero ballot words, and zero words between populated ones."""
    rng = np.random.default_rng(9200)
    n_var, n_cols = 64 * 9 + 5, 64 * 4 + 6
    codes = _panel(rng, n_var, n_cols, af_lo=0.05)
    codes[:, 0] = 0
    codes[:, n_cols - 1] = 255
    codes[:, 64:128] = 0                      # the columns of one whole wave of k_gt_count
    codes[:, 3] = 1                           # every variant
    codes[:, 4] = 0; codes[0, 4] = 1          # only variant 0
    codes[:, 5] = 0; codes[n_var - 1, 5] = 1  # only the last: eight zero words and a partial chunk
    codes[:, 6] = 0; codes[64 * 3 + 17, 6] = 1; codes[64 * 3 + 18, 6] = 1          # behind three zero words
    codes[:, 130] = 0; codes[5, 130] = 1; codes[64 * 4 + 63, 130] = 1; codes[64 * 8, 130] = 1   # zero words in between
    vl, va, r0, ch = _variants(rng, n_var, frac_indel=0.5)
    ch[[0, n_var - 1, 64 * 3 + 17, 64 * 4 + 63]] = [5, -2, 3, -7]
    with Lists(codes) as h:
        col_off, idx, o, delta, ind = h.check(codes, vl, va, r0, ch)
    n = np.diff(col_off.astype(np.int64))
    assert n[0] == 0 and n[-1] == 0 and (n[64:128] == 0).all() and n[3] == n_var and n[4] == 1 and n[5] == 1 and n[6] == 2 and n[130] == 3
    assert idx[int(col_off[5])] == n_var - 1 and idx[int(col_off[6]):int(col_off[7])].tolist() == [64 * 3 + 17, 64 * 3 + 18]
    assert o[int(col_off[6]) + 1] == r0[64 * 3 + 18] + 3 and delta[3] == ch.astype(np.int64).sum()


def test_lists_chains_large_mixed_signs_all_snv_all_indel():
    rng = np.random.default_rng(9300)
    n_var, n_cols = 700, 70
    codes = _panel(rng, n_var, n_cols, af_lo=0.05)
    codes[:, 2] = 1
    vl, va, _, _ = _variants(rng, n_var)
    r0 = (2_000_000 + np.arange(n_var) * 1000).astype(np.int32)
    # magnitudes up to 10^5, mixed signs; column 2 carries all: its running sum dips below zero and comes back
    ch = rng.integers(-100_000, 100_001, n_var).astype(np.int32)
    ch[:10] = -100_000
    ch[10:25] = 100_000
    run = np.concatenate([[0], np.cumsum(ch.astype(np.int64))])
    assert run.min() < 0 < run.max() and np.abs(run).max() + r0.max() < 2**31 and (run[1:11] < 0).all() and run[25] > 0
    with Lists(codes) as h:
        col_off, idx, o, delta, ind = h.check(codes, vl, va, r0, ch)
        assert (o[int(col_off[2]):int(col_off[3])] < r0[:n_var]).any() and delta.dtype == np.int64
        col_off, idx, o, delta, ind = h.check(codes, vl, va, r0, np.zeros(n_var, np.int32))      # all SNV
        assert len(ind) == 0 and not delta.any() and np.array_equal(o, r0[idx])
        col_off, idx, o, delta, ind = h.check(codes, vl, va, r0, np.where(ch == 0, 1, ch))      # all indel
        assert np.array_equal(ind, np.arange(len(idx)))


def test_lists_multiallelic_lines_and_the_254_contract():
    """Up to three variants per line with alleles 1..3, lines in non-monotone order (positions are re-sorted after the
    multi-allelic adjustment, so "ascending" means ascending j, not ascending var_line), missing codes never match.
    254: the parser clamps every allele number >= 254 to it and k_gt_count fills dead lanes with it; the host check admits
    var_allele 254, and the contract is the plain definition - code 254 matches allele 254 in live columns and nowhere else
    (no entry may appear from a filler: columns beyond n_cols and variants beyond n_var do not exist)."""
    rng = np.random.default_rng(9400)
    n_lines, n_cols = 300, 2 * 33                      # 66 columns: 62 dead lanes in the second wave of columns
    codes = _panel(rng, n_lines, n_cols, max_alt=3, af_lo=0.05, missing=0.05)
    codes[rng.random(codes.shape) < 0.02] = 253
    codes[rng.random(codes.shape) < 0.02] = 254
    codes[:, 65] = 254                                 # the last live lane, all at the clamp value
    line, allele = [], []
    for i in range(n_lines):
        for a in ([1], [1, 2], [1, 2, 3], [2, 253, 254], [254])[i % 5]:
            line.append(i); allele.append(a)
    order = rng.permutation(len(line))                 # var_line not monotone
    vl, va = np.array(line, np.uint32)[order], np.array(allele, np.uint8)[order]
    n_var = len(vl)
    assert (np.diff(vl.astype(np.int64)) < 0).any() and n_var % 64 != 0
    r0 = (np.arange(n_var) * 30 + 50).astype(np.int32)
    ch = (rng.integers(-6, 7, n_var) * (rng.random(n_var) < 0.4)).astype(np.int32)
    with Lists(codes) as h:
        col_off, idx, o, delta, ind = h.check(codes, vl, va, r0, ch)
    assert (np.diff(idx[int(col_off[7]):int(col_off[8])].astype(np.int64)) > 0).all()
    n254 = int((va == 254).sum())
    assert int(col_off[66] - col_off[65]) == n254 > 0          # exactly the 254 alleles, each once
    assert (va[idx] == codes[vl[idx], np.repeat(np.arange(n_cols), np.diff(col_off.astype(np.int64)))]).all()
    assert (codes == 255).sum() > 100


def test_lists_from_parsed_text_equal_lists_from_codes():
    rng = np.random.default_rng(9500)
    ns, n_lines = 130, 150
    b = Batch()
    for _ in range(n_lines):
        b.add([b"%d|%d:%d" % (int(rng.choice(4, p=[0.7, 0.1, 0.1, 0.1])), int(rng.choice(4, p=[0.7, 0.1, 0.1, 0.1])), int(rng.integers(0, 999)))
               for _ in range(ns)])
    codes, flags, g = _check_batch(b, ns, keep=True)
    assert not flags.any()
    line, allele = np.repeat(np.arange(n_lines, dtype=np.uint32), 3), np.tile(np.array([1, 2, 3], np.uint8), n_lines)
    r0 = (line.astype(np.int32) * 50 + 10)
    ch = (rng.integers(-5, 6, len(line)) * (rng.random(len(line)) < 0.5)).astype(np.int32)
    with Lists(handle=g, n_samples=ns) as hp, Lists(codes) as hc:
        a = hp.check(codes, line, allele, r0, ch)
        c = hc.check(codes, line, allele, r0, ch)
    assert all(np.array_equal(x, y) for x, y in zip(a, c)) and a[0][-1] > 1000


def test_lists_handle_reuse_large_small_empty():
    """hawk_gt_lists frees and rebuilds the handle's buffers: a large, a small and an empty table on one handle, and the indel
    query with no buffer, the exact capacity and a capacity below the count (only `cap` entries are written)."""
    rng = np.random.default_rng(9600)
    n_lines, n_cols = 2100, 140
    codes = _panel(rng, n_lines, n_cols, af_lo=0.02)
    z32, zu8 = np.zeros(0, np.int32), np.zeros(0, np.uint8)
    with Lists(codes) as h:
        for n_var in (2100, 40, 0, 70):
            vl, va, r0, ch = _variants(rng, n_var, frac_indel=0.6) if n_var else (np.zeros(0, np.uint32), zu8, z32, z32)
            col_off, idx, o, delta, ind = h.check(codes, vl, va, r0, ch)
            if n_var == 0:
                assert col_off[-1] == 0 and len(ind) == 0 and not delta.any()
                continue
            assert len(ind) > 4
            ni = C.c_uint64(0)
            part = np.full(len(ind), 0xfeed, np.uint32)
            h._lib.check(h.L.hawk_gt_lists_indels(h.g, _p(part), C.c_uint64(len(ind) - 3), C.byref(ni)), "hawk_gt_lists_indels")
            assert ni.value == len(ind) and np.array_equal(part[:-3], ind[:-3]) and part[-3:].tolist() == [0xfeed] * 3


def test_lists_refusals_launch_nothing_and_leave_the_handle_usable():
    _lib = _L()[0]
    rng = np.random.default_rng(9700)
    codes = _panel(rng, 50, 20, af_lo=0.1)
    vl, va, r0, ch = _variants(rng, 50)
    with Lists(codes) as h:
        bad = vl.copy(); bad[17] = 50
        assert h.status(bad, va, r0, ch) == _lib.HAWK_E_INVALID                      # var_line >= n_lines
        for a in (0, 255):
            bad = va.copy(); bad[49] = a
            assert h.status(vl, bad, r0, ch) == _lib.HAWK_E_INVALID                  # allele 0 / 255
        for k in range(4):
            args = [vl, va, r0, ch]
            args[k] = None
            assert h.L.hawk_gt_lists(h.g, _p(args[0]), _p(args[1]), _p(args[2]), _p(args[3]), 50, _p(np.zeros(21, np.uint64)), None,
                                     None) == _lib.HAWK_E_INVALID                   # a NULL array with n_var > 0
        assert h.status(vl, va, r0, ch, with_off=False) == _lib.HAWK_E_INVALID
        h.check(codes, vl, va, r0, ch)
    g = C.c_void_p()
    assert _L()[1].hawk_gt_from_codes(_L()[2], _p(codes), C.c_uint64(50), 0, C.byref(g)) == _lib.HAWK_E_INVALID and not g.value
    assert _L()[1].hawk_gt_from_codes(_L()[2], None, C.c_uint64(50), 10, C.byref(g)) == _lib.HAWK_E_INVALID and not g.value
    with Lists(codes) as h:
        h.check(codes, vl, va, r0, ch)
