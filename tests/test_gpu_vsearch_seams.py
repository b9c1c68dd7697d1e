"""The per-dirty-word view search (hawk_vsearch.hip: k_vsearch, k_ref_hits, k_ref_hits_prefix; hawk_vc.h) on its seams: the
hand-built cases of tests/vsearch_refs.py - each proved on the CPU to sit on the seam it is named after - expanded on the device,
searched through the plan's view with HAWK_VIEW_SEARCH=words, and compared with the ORACLE's search of the oracle's haplotypes.
Counts, coordinates, windows, REF-partner flags and CFDon are bit-exact; the table is held to its raw order before any sorting -
(row, tile, strand, window start) ascending, strand 0 of every chunk of a tile ahead of strand 1 - and to the per-tile row counts
of the CPU restatement.  The plane search of the materialised rows must then give the same table, column for column, in the same
order.  The last test leaves both environment switches unset: a small panel takes this route by default."""
import numpy as np
import pytest

import vsearch_refs as vr
from crisprhawk_hip import synth
from crisprhawk_hip.workload import expand_on_device
from oracle import oracle as ora

pytestmark = pytest.mark.gpu

SEAM_CASES = [n for n in vr.CASES if n != "default_route"]
COLS = ("hap", "pos", "strand", "start", "stop", "flags")
_built = {}


def built(name: str) -> vr.Case:
    """a case, its oracle result and its restated tile plans, built once per module"""
    if name not in _built:
        c = vr.CASES[name]()
        c.tally()
        _built[name] = c
    return _built[name]


def _words_search_against_the_oracle(c: vr.Case, monkeypatch, force_words: bool):
    _haps, _scan, is_ref, want = c.oracle()
    bits, bitsrc, _, _ = ora.pam_encode(c.pam)
    score = c.pam == "NGG" and not c.right and c.guidelen >= 20
    mm, pt = synth.cfd_tables() if score else (None, None)
    ds, _info, _ms, kept = expand_on_device(c.region(), c.pamlen, keep_plan=True)
    rows = c.device_rows()
    assert ds.n_hap == 1 + len(rows) and list(kept) == [0] + [r for r, x in enumerate(rows, 1) if x[3]]
    assert ds.stride == vr.stride_words(max([len(c.ref)] + [c.row(si, cp).len for si, cp, _, _ in rows]))
    planes = ds.search(bits, bitsrc, c.pamlen, c.guidelen, c.right, mm, pt)
    view = ds.plan.view()
    if force_words:
        monkeypatch.setenv("HAWK_VIEW_SEARCH", "words")
    else:
        assert not ds.plan.cluster_stats()["usable"], ds.plan.cluster_stats()
    tab = view.search(bits, bitsrc, c.pamlen, c.guidelen, c.right, mm, pt)
    assert tab.timing["v_path"] == 1
    assert (tab.n_rows, tab.n_candidates, tab.n_hits) == (len(want.guides), want.n_candidates, want.n_hits)
    # the raw table: (row, tile, strand, window start) ascending; the per-tile row counts of the restatement
    bph = c.bph
    q = c.qstart(tab.pos, tab.strand)
    tile = q // vr.TILE
    assert np.array_equal(np.lexsort((q, tab.strand, tile, tab.hap)), np.arange(tab.n_rows)), "rows are not in (row, tile, strand, start) order"
    per = np.bincount(tab.hap.astype(np.int64) * bph + tile, minlength=ds.n_hap * bph)
    for (r, t), v in c.tally().items():
        assert per[r * bph + t] == v, (r, t, int(per[r * bph + t]), v)
    # the table in the reference's order
    order = tab.reference_order()
    g = want.guides
    rowmap = np.full(ds.n_hap, -1, dtype=np.int64)
    rowmap[np.asarray(kept)] = np.arange(len(kept))
    assert np.array_equal(rowmap[tab.hap[order]], g["hap"])
    for col in ("start", "stop", "pos", "strand"):
        assert np.array_equal(getattr(tab, col)[order], g[col]), col
    wins = tab.windows()
    assert [wins[i] for i in order] == want.windows
    assert np.array_equal(tab.flags[order], c.expected_flags())
    if score:
        _, _, _, cfd, _ = ora.reverse_and_cfdon(want, is_ref, c.guidelen, c.pamlen, mm, pt, decode=False)
        mine = tab.cfdon[order]
        assert np.array_equal(np.isnan(mine), np.isnan(cfd)) and np.array_equal(mine[~np.isnan(cfd)], cfd[~np.isnan(cfd)])
        alt = ~np.asarray(is_ref)[g["hap"]]
        assert np.array_equal(np.isnan(cfd[alt]), c.expected_flags()[alt] == 0)  # an alt row scores iff REF has a guide at its key
    else:
        assert np.isnan(tab.cfdon).all()
    # the plane search of the materialised rows: the same table in the same order
    assert (planes.n_rows, planes.n_candidates, planes.n_hits) == (tab.n_rows, tab.n_candidates, tab.n_hits)
    for col in COLS:
        assert np.array_equal(getattr(planes, col), getattr(tab, col)), col
    assert np.array_equal(planes.win, tab.win)
    assert np.array_equal(planes.cfdon, tab.cfdon, equal_nan=True)
    ds.plan.close()
    ds.close()


@pytest.mark.parametrize("name", SEAM_CASES)
def test_words_search_on_a_seam_against_the_oracle(name, monkeypatch):
    c = built(name)
    missing = [frag for frag in vr.REQUIRED[name] if not any(frag in label for label in c.proved)]
    assert not missing, (name, missing)
    monkeypatch.delenv("HAWK_CLUSTER_MIN_SHARE", raising=False)
    _words_search_against_the_oracle(c, monkeypatch, force_words=True)


def test_a_small_panel_takes_the_words_route_by_default(monkeypatch):
    """neither HAWK_VIEW_SEARCH nor HAWK_CLUSTER_MIN_SHARE set: two samples share no cluster three times, hawk_api_cldict.hip
    declines the dictionary and the view search runs per dirty word"""
    monkeypatch.delenv("HAWK_VIEW_SEARCH", raising=False)
    monkeypatch.delenv("HAWK_CLUSTER_MIN_SHARE", raising=False)
    c = built("default_route")
    assert all(any(frag in label for label in c.proved) for frag in vr.REQUIRED["default_route"])
    _words_search_against_the_oracle(c, monkeypatch, force_words=False)
