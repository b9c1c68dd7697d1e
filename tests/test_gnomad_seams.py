"""The seam panels of tests/gnomad_seam_refs.py, without a device.  First every figure a case is named for is asserted on the
panel from the reference alone (field offsets and chunk phases, comma offsets, AF entry and value offsets, per-wave phase, total
and route of the fill pass), so that an edit of a builder cannot quietly move a case off its seam; then the panels go through the
host twin (engine="host": hawk_host_gnomad_lines, which runs csrc/hawk_gnomad.h) and are held to tests/gnomad_refs.py byte for
byte and to record_facts() field for field.  tests/test_gpu_gnomad_seams.py runs the same panels on the device.
`pytest -s` prints the per-record seam offsets and the per-wave figures."""
import numpy as np
import pytest

import gnomad_refs as refs
import gnomad_seam_refs as sr
from test_gpu_gnomad import batch_of

SWEEP, CHUNK, SLOT = sr.SWEEP, sr.CHUNK, sr.SLOT


def want_mask(line, joint):
    """bit k: key k observed, read from INFO (field 8 alone) as the reference reads it"""
    info = line.split("\t")[7]
    return sum(1 << k for k, key in enumerate(refs.keys_of(joint)) if refs.observed(refs.info_entry(info, key)))


def run_panel(cases, joint, keep, engine):
    """One batch of `cases` through `engine`, held to the reference: the bytes, the kept count, flags (0, or GN_DROPPED where the
    keep rule drops the record), the genotype mask, fo / qs / afs against record_facts.  Returns the _Batch."""
    lines, ends = [c.line for c in cases], [c.end for c in cases]
    want = [refs.convert_line(ln, joint, keep) for ln in lines]
    got, kept, failure, b = batch_of(lines, joint, keep, engine=engine, ends=ends)
    assert failure is None
    fo, qs, afs = sr.facts_arrays(lines)
    for name, mine, theirs in (("fo", b.fo, fo), ("qs", b.qs, qs), ("afs", b.afs, afs)):
        bad = np.flatnonzero((mine != theirs).any(axis=1))
        assert not len(bad), (name, cases[int(bad[0])].label, mine[bad[0]].tolist(), theirs[bad[0]].tolist())
    flags = [0 if o is not None else sr.GN_DROPPED for o in want]
    assert [int(f) for f in b.flags] == flags
    assert [int(m) for m in b.mask] == [0 if o is None else want_mask(ln, joint) for ln, o in zip(lines, want)]
    assert kept == sum(o is not None for o in want)
    text = "".join(o + "\n" for o in want if o is not None)
    if got != text:  # name the first record whose line differs
        at = next((i for i, (x, y) in enumerate(zip(got, text)) if x != y), min(len(got), len(text)))
        rec = text.count("\n", 0, at)
        raise AssertionError(f"output differs at byte {at}, kept record {rec}: got {got[max(at - 30, 0):at + 30]!r}, want {text[max(at - 30, 0):at + 30]!r}")
    return b


def run_refused(cases, engine, flag, message):
    """each case a batch of its own that must be refused: its flags, its facts, the message"""
    for c in cases:
        got, kept, failure, b = batch_of([c.line], False, False, engine=engine, ends=[c.end])
        assert got is None and failure is not None and message in failure, (c.label, failure)
        assert int(b.flags[0]) == flag and int(b.mask[0]) == (0 if flag else want_mask(c.line, False)), c.label
        fo, qs, afs = sr.facts_arrays([c.line])
        assert b.fo.tolist() == fo.tolist() and b.qs.tolist() == qs.tolist() and b.afs.tolist() == afs.tolist(), c.label


# ------------------------------------------------------------------------------------------------ the panels sit on their seams
def test_field_panel_sits_on_its_seams():
    cases = sr.field_cases()
    assert len(cases) == 7 * 7 + 3 * (1 + 2 + 3 + 4 + 5 + 5 + 6)
    seen = set()
    for f, o, how in cases:
        line = sr.line_with_field_at(f, o, how)
        facts = sr.record_facts(line)
        assert facts["fo"][f] == o and line[o - 1] == "\t" and facts["full"]
        assert refs.convert_line(line, False, True) is not None
        assert (refs.convert_line(line, False, False) is None) == (f == 7 and o in (15, 16))  # no room for PASS in front of INFO
        seen.add((f, o))
        print(f"field {f} at {o:5d} (chunk phase {o & 15:2d}, sweep {o // SWEEP}) by field {how}: fo = {facts['fo']}")
    assert seen == {(f, o) for f in range(1, 8) for o in sr.FIELD_OFFSETS}
    for f in range(1, 8):
        phases = {o & 15 for ff, o in seen if ff == f}
        assert {0, 1, 15} <= phases  # 0: the tab is the last byte of the chunk in front; 15: the start is a chunk's last byte; 1: the tab a chunk's first
        assert {o for ff, o in seen if ff == f and o % SWEEP == 0} == {SWEEP, 2 * SWEEP}  # the tab the sweep's last byte: `prev` from text[a - 1]
        assert {(ff, o, h) for ff, o, h in cases if ff == f and o == SWEEP} == {(f, SWEEP, h) for h in range(f) if h != 5}
    panel = sr.field_panel()
    assert len(panel) == 3 * len(cases)
    for c in panel[len(cases):2 * len(cases)]:  # the ninth field is a decoy of the OPPOSITE value, and holds an AF the record must not print
        f = c.line.split("\t")
        assert len(f) == 9 and f[8] == "AC_afr=5;AF=0.9" and "AC_afr=0;" in f[7] and "AF=0.9" not in refs.convert_line(c.line, False, True)
    assert all(c.end == "\r\n" for c in panel[2 * len(cases):])


def test_few_fields_panel_sits_on_its_seams():
    cases = sr.few_fields_panel()
    tabs = set()
    for c in cases:
        facts = sr.record_facts(c.line)
        nf = len(c.line.split("\t"))
        assert nf in (2, 7) and not facts["full"] and facts["fo"][nf:] == [len(c.line)] * (8 - nf)
        tabs.add((nf, c.line.rindex("\t"), c.line.endswith("\t")))
        with pytest.raises(refs.RefError):
            refs.convert_line(c.line, False, True)
        print(f"{c.label}: fo = {facts['fo']}, len {len(c.line)}")
    assert tabs == {(nf, t, e) for nf in (2, 7) for t in (SWEEP - 1, SWEEP) for e in (False, True)}


def test_alt_panel_sits_on_its_seams():
    cases = sr.alt_panel()
    counts, phases, offsets, decoy_phases = [], set(), set(), set()
    for c in cases:
        facts = sr.record_facts(c.line)
        commas = sr.comma_offsets(c.line)
        assert facts["afs"] == [len(commas) + 1, sr.ABSENT] and facts["n_alt"] == len(commas) + 1
        out = refs.convert_line(c.line, False, False)
        assert out.split("\t")[7] == "AF=" + ",".join(["0.0"] * facts["n_alt"])
        counts.append(facts["n_alt"])
        if c.label.startswith("comma decoys"):
            f = c.line.split("\t")
            assert f[2] == "a,b,c" and f[4] == "G" and f[7].startswith("x=1,2,3;") and facts["n_alt"] == 1
            alt = facts["fo"][4]
            near = [p for p in range(len(c.line)) if c.line[p] == "," and p // CHUNK == alt // CHUNK]
            decoy_phases.add((alt & 15, bool([p for p in near if p < alt]), bool([p for p in near if p > alt])))
        elif "alleles from" in c.label:
            phases |= {p & 15 for p in commas}
            offsets |= set(commas)
        print(f"{c.label}: ALT at {facts['fo'][4]}, {len(commas)} commas, first {commas[:3]}, last {commas[-2:]}, QUAL at {facts['fo'][5]}")
    assert counts[:len(sr.ALT_COUNTS)] == sr.ALT_COUNTS == [1, 2, 16, 17, 2048, 2049, 5000]
    assert phases == set(range(16)) and {SWEEP - 2, SWEEP - 1, SWEEP, SWEEP + 1} <= offsets
    long_commas = sr.comma_offsets(cases[6].line)
    assert long_commas[0] < SWEEP < 2 * SWEEP < 3 * SWEEP < long_commas[-1]  # 5000 alleles: commas in four sweeps
    # the decoy commas share the ALT byte's chunk: ID's in front of it, INFO's behind it, at every phase of the ALT byte
    assert {p for p, _, _ in decoy_phases} == set(range(16))
    assert any(before for _, before, _ in decoy_phases) and any(after for _, _, after in decoy_phases)


@pytest.mark.parametrize("joint", [False, True])
def test_af_panel_sits_on_its_seams(joint):
    cases = sr.af_panel(joint)
    starts, splits = set(), set()
    for c in cases:
        facts = sr.record_facts(c.line)
        v0, vl = facts["afs"]
        assert vl != sr.ABSENT or "alone" in c.label
        out = refs.convert_line(c.line, joint, False)
        if c.label.startswith("AF= at"):
            assert c.line[v0 - 3:v0 + vl] == "AF=0.25" and c.line[v0 - 4] == ";"
            starts.add(v0 - 3)
        elif c.label.startswith("AF value split"):
            assert c.line[v0:v0 + vl] == sr.AF_VALUE and v0 < SWEEP < v0 + vl
            splits.add(SWEEP - v0)
            assert out.split("\t")[7] == "AF=0.125,9.999999747378752e-06,3.0"
        elif "last bytes" in c.label:
            assert v0 + vl == len(c.line.split(sr.NINTH)[0]) and out.split("\t")[7] == "AF=0.5"
        elif "alone" in c.label:
            assert facts["afs"] == [2, sr.ABSENT] and out.split("\t")[7] == "AF=0.0,0.0"
        else:
            assert out.split("\t")[7] == "AF=0.25", c.label
        print(f"{c.label}: AF value at {v0} ({'absent' if vl == sr.ABSENT else vl} bytes), record of {len(c.line)}")
    assert starts == set(range(SWEEP - 16, SWEEP + 2)) | set(range(2 * SWEEP - 2, 2 * SWEEP + 3))
    assert splits == set(range(1, len(sr.AF_VALUE)))
    for c in sr.af_bare_panel():
        facts = sr.record_facts(c.line)
        assert facts["afs"][1] == 0 and c.line[facts["afs"][0] - 2:facts["afs"][0]] == "AF"
        with pytest.raises(refs.RefError):
            refs.convert_line(c.line, False, False)


_FILL = {}


def fill(which):
    """(lines, named, off, figures) of a fill batch, built once"""
    if which not in _FILL:
        lines, named = (sr.fill_panel if which == "main" else sr.fill_panel_63)()
        off, figs = sr.wave_figures(lines, False, False)
        _FILL[which] = (lines, named, off, figs)
    return _FILL[which]


def test_fill_panel_sits_on_its_seams():
    lines, named, off, figs = fill("main")
    assert 2000 <= len(lines) <= 5000 and sum(len(ln) + 1 for ln in lines) < 3_000_000
    name_of = {v: k for k, v in named.items()}
    for w, (a, total, route) in enumerate(figs):
        print(f"wave {w:2d} {name_of[w]:28s} phase {a:2d} total {total:6d} a+total {a + total:6d} end&15 {(a + total) & 15:2d} {route}")
    fig = lambda name: figs[named[name]]
    for j in range(16):
        assert fig(f"staged phase {j}")[::2] == (j, "staged") and fig(f"direct phase {j}")[::2] == (j, "direct")
        assert fig(f"staged phase {j}")[1] % 16 == 1 and fig(f"direct phase {j}")[1] % 16 == 1
    assert {a for a, _, r in figs if r == "staged"} == set(range(16)) == {a for a, _, r in figs if r == "direct"}
    assert fig("a=0 sum 8192") == (0, SLOT, "staged") and fig("a=0 sum 8193") == (0, SLOT + 1, "direct")
    assert fig("a=15 sum 8192") == (15, SLOT - 15, "staged") and fig("a=15 sum 8193") == (15, SLOT - 14, "direct")
    ends = {(a + t) & 15 for a, t, r in figs if r == "staged"}
    assert 0 in ends and 1 in ends  # a staged range ends on a 16-byte boundary, another one byte past it
    w = named["empty"]
    assert figs[w][1:] == (0, "empty") and figs[w - 1][2] == "staged" and figs[w + 1][2] == "staged"
    kept = lambda name: [i for i in range(64) if off[named[name] * 64 + i + 1] > off[named[name] * 64 + i]]
    assert kept("lane 0 only") == [0] and kept("lane 63 only") == [63] and kept("alternating") == list(range(0, 64, 2)) and kept("empty") == []
    a, total, route = fig("long ALT")
    assert route == "direct" and len(kept("long ALT")) == 64 and sr.LONG_ALT < total < sr.LONG_ALT + 64 * 100
    assert max(len(ln) for ln in lines) < sr.LONG_ALT + 300  # nothing larger than the 100 000-byte record
    a, total, route = fig("shortest alone")
    assert total == sr.SHORTEST_LINE == sr.out_len(sr.SHORTEST) and route == "staged" and kept("shortest alone") == [17]
    # the last workgroup: direct, empty, one record (staged), and a wave beyond n
    last = len(figs) - 1
    assert last % 4 == 2 and len(lines) == last * 64 + 1 and last == named["last workgroup: one record"]
    assert [figs[last - 2][2], figs[last - 1][2], figs[last][2]] == ["direct", "empty", "staged"] and figs[last][1] > 0
    lines63, named63, off63, figs63 = fill("63")
    assert len(lines63) == 4 * 64 + 63 and [r for _, _, r in figs63] == ["empty", "direct", "staged", "staged", "staged"]
    assert off63[-1] - off63[4 * 64] == sum(sr.out_len(ln) for ln in lines63[-63:]) and all(sr.out_len(ln) for ln in lines63[-63:])
    for w, (a, total, route) in enumerate(figs63):
        print(f"second batch wave {w} phase {a:2d} total {total:6d} {route}")


# ------------------------------------------------------------------------------------------------ the host twin on the panels
@pytest.mark.parametrize("keep", [False, True])
def test_host_field_panel(keep):
    cases = sr.field_panel()
    b = run_panel(cases, False, keep, "host")
    want = [refs.convert_line(c.line, False, keep) for c in cases]
    assert [int(m) for m in b.mask] == [0x3fe if o is not None else 0 for o in want]
    assert sum(o is None for o in want) == (0 if keep else 6)


def test_host_few_fields_panel():
    run_refused(sr.few_fields_panel(), "host", flag=sr.GN_FEW_FIELDS, message="fewer than eight fields")


def test_host_alt_panel():
    cases = sr.alt_panel()
    b = run_panel(cases, False, False, "host")
    assert [int(x) for x in b.afs[:, 0]] == [sr.record_facts(c.line)["n_alt"] for c in cases] and (b.afs[:, 1] == sr.ABSENT).all()


@pytest.mark.parametrize("joint", [False, True])
def test_host_af_panel(joint):
    run_panel(sr.af_panel(joint), joint, False, "host")


def test_host_af_bare_panel():
    run_refused(sr.af_bare_panel(), "host", flag=0, message="AF is not a finite decimal number")


@pytest.mark.parametrize("which", ["main", "63"])
def test_host_fill_panel(which):
    lines, named, off, figs = fill(which)
    run_panel([sr.Case(str(i), ln, "\n") for i, ln in enumerate(lines)], False, False, "host")
