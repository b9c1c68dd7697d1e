"""The unphased resolution on the host (csrc/hawk_resolve.h through hawk_host_resolve_unphased) against resolve_guide +
remove_redundant_guides: on the reference's own g4 lists, on the seam panel the device tests share (tests/resolve_refs.py) and on
each decline.  No GPU."""
import numpy as np
import pytest

import resolve_refs as rr
from crisprhawk_hip import _lib
from crisprhawk_hip.search_guides import flatten_variant_alleles, resolve_guide, search, is_pamhit_valid
from util import load_golden

PANEL = rr.panel()


def test_abi_exports_the_resolve_calls():
    L = _lib.lib()
    for name in ("hawk_table_resolve_unphased", "hawk_resolve_download", "hawk_resolve_free", "hawk_host_resolve_unphased"):
        assert name in _lib.EXPORTS and hasattr(L, name)


def test_engine_parameter_is_validated_before_any_device_work():
    with pytest.raises(ValueError, match="unphased_engine"):
        search(None, None, [], None, 20, False, True, False, 0, True, unphased_engine="gpu")


@pytest.mark.parametrize("fixture", rr.G4_FIXTURES)
def test_twin_gives_the_references_own_lists(fixture):
    """The fixture's haplotypes and PAM hits -> rows as retrieve_guides derives them -> the twin: the reference's guide list,
    complete and in order.  The Python restatement is held to the same list, which is what pins it for the panel below."""
    fx = load_golden(f"{fixture}.json.gz")
    region, haps, pam = rr.haplotypes_from_fixture(fx)
    assert [h.samples == "REF" for h in haps].count(True) == 1 and haps[0].samples == "REF"
    assert all(len(v) == 1 for h in haps for v in h.variant_alleles.values())
    t = rr.derive_rows(haps, fx["hits"], len(pam), fx["guidelen"], fx["right"])
    want = [list(g) for g in fx["guides"]]
    assert rr.expected_guides(haps, t, pam, fx["guidelen"], fx["right"]) == want
    res = rr.twin(haps, t, pam, fx["guidelen"], fx["right"])
    assert int(res.n_kept.sum()) == len(res.src_row) == len(want)
    assert rr.guides_of(res, haps, t, fx["right"]) == want


def _python_counts(haps, t, pam, guidelen, right):
    """per row, in table order: combinations resolve_guide returns (0 for an invalid row)"""
    out = []
    for i in range(t.n_rows):
        h = haps[int(t.hap[i])]
        strand = int(t.strand[i])
        r = (not right) if strand else right
        ok = is_pamhit_valid(int(t.pos[i]), len(h), guidelen, len(pam), r)
        out.append(len(resolve_guide(t.seqs[i], pam, strand, r, int(t.pos[i]), guidelen, h, True)) if ok else 0)
    return out


@pytest.mark.parametrize("name", sorted(PANEL))
def test_panel_scene(name):
    s = PANEL[name]
    region, haps, pam, t = s.rows()
    want = rr.expected_guides(haps, t, pam, s.guidelen, s.right)
    res = rr.twin(haps, t, pam, s.guidelen, s.right)
    py_res = _python_counts(haps, t, pam, s.guidelen, s.right)
    assert res.n_resolved.tolist() == py_res
    assert rr.guides_of(res, haps, t, s.right) == want
    assert np.all(np.diff(res.src_row.astype(np.int64)) >= 0) and np.array_equal(np.bincount(res.src_row, minlength=t.n_rows), res.n_kept)
    # the scene is what it says it is (counts by the Python restatement, not by the code under test)
    py_kept = np.bincount([next(i for i in range(t.n_rows) if (int(t.start[i]), int(t.strand[i]), int(t.hap[i])) == (g[0], g[2], g[4])) for g in want],
                          minlength=t.n_rows).tolist()
    if "n_resolved" in s.claims:
        assert py_res == s.claims["n_resolved"], (py_res, t.seqs)
    if "n_kept" in s.claims:
        assert py_kept == s.claims["n_kept"], py_kept
    assert res.n_kept.tolist() == py_kept


def test_k2_gives_every_base_twice_in_acgt_order():
    s = PANEL["options"]
    region, haps, pam, t = s.rows()
    res = rr.twin(haps, t, pam, s.guidelen, s.right)
    seqs = res.windows()
    row = 1  # S1's row: 'd' with two entries at window offset 20
    mine = [seqs[k][20] for k in np.flatnonzero(res.src_row == row)]
    assert res.n_resolved[row] == 6 and mine == ["g", "g", "t", "t"]           # A, A dropped: REF's core
    assert [seqs[k][15] for k in np.flatnonzero(res.src_row == 2)] == ["c", "g", "t"]   # the 4-letter code
    assert [seqs[k][10] for k in np.flatnonzero(res.src_row == 3)] == ["g"]    # multi-base ref: a and g, the a is REF's core


def test_ref_last_changes_the_list_order_only():
    s = PANEL["ref_last"]
    region, haps, pam, t = s.rows()
    assert haps[-1].samples == "REF"
    got = rr.guides_of(rr.twin(haps, t, pam, s.guidelen, s.right), haps, t, s.right)
    s.ref_last = False
    try:
        region2, haps2, pam2, t2 = s.rows()
        first = rr.guides_of(rr.twin(haps2, t2, pam2, s.guidelen, s.right), haps2, t2, s.right)
    finally:
        s.ref_last = True
    strip = lambda gs: sorted((g[0], g[1], g[2], g[3], g[6]) for g in gs)
    assert strip(got) == strip(first) and [g[:4] for g in got] != [g[:4] for g in first]


def _declined(s, **kw):
    region, haps, pam, t = s.rows()
    with pytest.raises(_lib.HawkResolveDeclined) as e:
        rr.twin(haps, t, pam, s.guidelen, s.right, **kw)
    return e.value, haps, pam, t


def test_decline_no_allele_entry():
    s, reason, exc = rr.decline_scenes()["no_entry"]
    e, haps, pam, t = _declined(s)
    assert (e.status, e.reason, e.row) == (_lib.HAWK_E_UNSUPPORTED, 1, 1)
    with pytest.raises(exc):  # what the host route raises there
        rr.expected_guides(haps, t, pam, s.guidelen, s.right)


def test_decline_more_than_one_ref():
    s, reason, _ = rr.decline_scenes()["multi_ref"]
    e, haps, pam, t = _declined(s)
    assert (e.status, e.reason, e.row) == (_lib.HAWK_E_UNSUPPORTED, 2, -1)


def test_decline_ref_row_with_two_combinations():
    s, reason, exc = rr.decline_scenes()["ref_ambig"]
    e, haps, pam, t = _declined(s)
    assert (e.status, e.reason, e.row) == (_lib.HAWK_E_UNSUPPORTED, 3, 0)
    with pytest.raises(exc, match="Duplicate REF guide"):  # what the host route raises there
        rr.expected_guides(haps, t, pam, s.guidelen, s.right)


def test_decline_row_above_2_32_and_counts_saturate():
    """(2^33 combinations cannot be walked by the host route in a test: this decline is checked as a status, here and on the device,
    not through search())"""
    s = rr.wide_row_scene(29, "wide33")   # 29 two-way positions in the left pad and the spacer, four more in the PAM's N and the right pad
    for p in (200, 205, 207, 209):   # 2^33
        s.haps[0][2][p] = ("w", [(s.ref[p], "T" if s.ref[p] == "A" else "A")])
    e, haps, pam, t = _declined(s)
    assert (e.status, e.reason, e.row) == (_lib.HAWK_E_CAPACITY, 4, 1)
    # every position 4-way with two entries: 8^43 combinations saturate the 64-bit count instead of wrapping to something small
    hap_len = np.array([100, 100], np.uint32)
    seqs = ["A" * 30 + "AGG" + "A" * 10, "n" * 43]
    key = np.array([(1 << 32) | p for p in range(43)], np.uint64)
    off = np.arange(0, 2 * 44, 2, dtype=np.uint32)
    ref = np.zeros(86, np.uint8)
    with pytest.raises(_lib.HawkResolveDeclined) as ex:
        from crisprhawk_hip.hapset import resolve_columns_host
        resolve_columns_host([0, 1], [30, 30], [0, 0], [1000, 1000], [1, 1], rr.encode_windows(seqs), hap_len, [1, 0], (key, off, ref), 0xF44, 0x22F, 20, 3, False)
    assert (ex.value.reason, ex.value.row) == (4, 1)


def test_decline_row_above_the_batch_budget_and_budget_changes_nothing_else():
    s = rr.wide_row_scene(10)
    region, haps, pam, t = s.rows()
    full = rr.twin(haps, t, pam, s.guidelen, s.right)
    assert full.n_kept.tolist() == [1, 1023]
    fits = rr.twin(haps, t, pam, s.guidelen, s.right, batch_bytes=1023 * 44)
    assert np.array_equal(fits.src_row, full.src_row) and np.array_equal(fits.win, full.win)
    e, *_ = _declined(s, batch_bytes=1023 * 44 - 1)
    assert (e.status, e.reason, e.row) == (_lib.HAWK_E_CAPACITY, 5, 1)


def test_malformed_allele_tables_are_invalid():
    from crisprhawk_hip.hapset import resolve_columns_host
    args = ([0], [30], [0], [1000], [0], rr.encode_windows(["A" * 30 + "AGG" + "A" * 10]), [100], [1])
    for key, off, ref in (([5, 5], [0, 1, 2], [0, 0]), ([5, 4], [0, 1, 2], [0, 0]), ([4, 5], [0, 2, 1], [0, 0]), ([4, 5], [0, 1, 2], [0, 7])):
        with pytest.raises(_lib.HawkStatusError) as e:
            resolve_columns_host(*args, (np.array(key, np.uint64), np.array(off, np.uint32), np.array(ref, np.uint8)), 0xF44, 0x22F, 20, 3, False)
        assert e.value.status == _lib.HAWK_E_INVALID


def test_flatten_variant_alleles():
    s = PANEL["options"]
    _, haps, _ = s.build()
    key, off, ref = flatten_variant_alleles(haps)
    assert key.tolist() == [(1 << 32) | 190, (2 << 32) | 185, (3 << 32) | 180]
    assert off.tolist() == [0, 2, 3, 4] and ref.tolist() == [0, 0, 0, 255]
