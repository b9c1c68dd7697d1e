"""The gnomAD converter's kernels (csrc/hawk_gnomad.hip) on the seams its first suite never reached: field starts, ALT commas and
the AF entry anywhere in a record's 16-byte chunks and 4096-byte sweeps (k_gn_scan), and the fill pass at every phase of the
blob's 16-byte grid, on both of its routes and on the sums that decide between them (k_gn_text_fill).  The panels are those of
tests/gnomad_seam_refs.py; tests/test_gnomad_seams.py proves on the CPU that each sits on the seam it is named after.  One batch
per panel; every batch asserts that the device engine ran (scan ms > 0, in batch_of), the bytes and the kept count against
tests/gnomad_refs.py, the flags, the genotype masks, and fo / qs / afs against record_facts() - not against the host twin."""
import ctypes as C

import numpy as np
import pytest

import gnomad_refs as refs
import gnomad_seam_refs as sr
from crisprhawk_hip import _lib, converter
from test_gnomad_seams import fill, run_panel, run_refused

pytestmark = pytest.mark.gpu


def test_field_starts_in_every_chunk_and_sweep():
    cases = sr.field_panel()
    b = run_panel(cases, False, False, "device")
    assert b.ms["scan_ms"] > 0
    n = len(cases) // 3
    assert [int(m) for m in b.mask[n:2 * n]] == [0 if int(f) else 0x3fe for f in b.flags[n:2 * n]]  # the ninth field's AC_afr=5 is not read
    assert int((b.flags == sr.GN_DROPPED).sum()) == 6  # field 7 at 15 / 16: no room for PASS


def test_few_fields_with_the_last_tab_at_the_sweep():
    run_refused(sr.few_fields_panel(), "device", flag=sr.GN_FEW_FIELDS, message="fewer than eight fields")


def test_alt_commas_in_every_chunk_and_sweep():
    cases = sr.alt_panel()
    b = run_panel(cases, False, False, "device")
    assert [int(x) for x in b.afs[:, 0]] == [sr.record_facts(c.line)["n_alt"] for c in cases] and (b.afs[:, 1] == sr.ABSENT).all()


@pytest.mark.parametrize("joint", [False, True])
def test_af_entry_at_the_sweeps(joint):
    run_panel(sr.af_panel(joint), joint, False, "device")


def test_bare_af_is_an_empty_value():
    run_refused(sr.af_bare_panel(), "device", flag=0, message="AF is not a finite decimal number")


@pytest.mark.parametrize("which", ["main", "63"])
def test_fill_at_every_phase_on_both_routes(which):
    """The batch through the converter's own code, but with the device's line offsets read back before the handle goes: a wrong
    length (off differs) and a wrong placement (off equal, bytes differ) are told apart."""
    lines, named, off, figs = fill(which)
    raw = "".join(ln + "\n" for ln in lines).encode()
    text = np.frombuffer(raw, np.uint8).copy()
    nl = np.flatnonzero(text == 10)
    line_off = np.zeros(len(nl) + 1, np.uint64)
    line_off[1:] = nl + 1
    b = converter._Batch(text, line_off, converter.format_ac(False), False, "device", 0)
    try:
        out, kept, failure = converter._convert_batch(b, 2, {"float_pool": 0.0, "lines_call": 0.0})
        assert failure is None and b.engine == "device" and b.ms["scan_ms"] > 0 and b.ms["fill_ms"] > 0
        got_off = np.full(len(lines) + 1, 77, np.uint64)
        _lib.check(_lib.lib().hawk_gnomad_text_download(b.handle, None, got_off.ctypes.data_as(C.c_void_p)), "hawk_gnomad_text_download")
        out = bytes(out)
    finally:
        b.close()
    bad = np.flatnonzero(got_off != off)
    assert not len(bad), f"line offset of record {int(bad[0])}: {int(got_off[bad[0]])}, expected {int(off[bad[0]])}"
    want = [refs.convert_line(ln, False, False) for ln in lines]
    assert kept == sum(o is not None for o in want) and [int(f) for f in b.flags] == [0 if o is not None else sr.GN_DROPPED for o in want]
    assert len(out) == int(off[-1])
    name_of = {v: k for k, v in named.items()}
    for w, (a, total, route) in enumerate(figs):  # wave by wave: the failure names the wave, its phase and its route
        r0 = w * sr.WAVE
        exp = "".join(o + "\n" for o in want[r0:r0 + sr.WAVE] if o is not None).encode()
        mine = out[int(off[r0]):int(off[r0]) + total]
        if mine != exp:
            at = next(i for i, (x, y) in enumerate(zip(mine, exp)) if x != y)
            raise AssertionError(f"wave {w} ({name_of[w]}: phase {a}, total {total}, {route}) differs at byte {at} of its range: "
                                 f"{mine[max(at - 20, 0):at + 20]!r}, expected {exp[max(at - 20, 0):at + 20]!r}")
    fo, qs, afs = sr.facts_arrays(lines)
    assert np.array_equal(b.fo, fo) and np.array_equal(b.qs, qs) and np.array_equal(b.afs, afs)
