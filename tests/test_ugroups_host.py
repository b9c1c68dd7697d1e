"""The report groups of an unphased table on the host (csrc/hawk_ugroups.h through hawk_host_unphased_groups) against a plain
Python restatement (tests/ugroups_refs.py) and against the grouping reports.report_from_guides does today, on the seam panel of
the resolution and on the scenes that are about grouping.  All comparisons are bit-equal.  No GPU."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import resolve_refs as rr
import ugroups_refs as ug
from crisprhawk_hip import _lib, reports, synth
from crisprhawk_hip.guide import GUIDESEQPAD
from crisprhawk_hip.utils import round_score

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "crispr-hawk_amd", "csrc")
SCENES = ug.scenes()
TABLES = synth.cfd_tables()
_RES = {}


def _resolved(name):
    """the twin's kept guides of a scene, computed once"""
    if name not in _RES:
        haps, pam, t, guidelen, right = SCENES[name]
        _RES[name] = rr.twin(haps, t, pam, guidelen, right)
    return _RES[name]


def test_abi_exports_the_group_calls():
    L = _lib.lib()
    for name in ("hawk_resolve_groups", "hawk_ugroups_download", "hawk_ugroups_free", "hawk_host_unphased_groups"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert "memory" in _lib.strerror(_lib.HAWK_E_OOM)


def test_header_compiles_as_plain_cpp(tmp_path):
    src = tmp_path / "h.cpp"
    src.write_text('#include "hawk_ugroups.h"\nint main() { UgGeom g = {20, 3, 0, 43, 23, 0, 0}; return ug_check_geom(g, 0, 0); }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(tmp_path / "h")])
    subprocess.check_call([str(tmp_path / "h")])


@pytest.mark.parametrize("with_tables", [False, True])
@pytest.mark.parametrize("flank", ug.FLANKS)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_twin_equals_restatement(name, flank, with_tables):
    haps, pam, t, guidelen, right = SCENES[name]
    res = _resolved(name)
    tables = TABLES if with_tables else None
    g = ug.host_groups(haps, t, res, pam, guidelen, right, flank, tables)
    want = ug.restate(haps, t, res, guidelen, len(pam), right, flank, tables)
    ug.assert_groups_equal_restatement(g, want)
    assert g.n_kept == len(res.src_row) == sum(len(w.guides) for w in want)
    if not with_tables:
        assert np.all(np.isnan(g.cfdon))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_twin_equals_todays_grouping(name, monkeypatch):
    """reports.report_from_guides on the same guides (in the reference's list order, CFDon per guide by the restatement): the same
    partition, the same representative core, the same rounded CFDon.  Its ReportInput is caught where it hands it to report_frame."""
    haps, pam, t, guidelen, right = SCENES[name]
    res = _resolved(name)
    W = guidelen + len(pam) + 2 * GUIDESEQPAD
    seqs = res.windows()
    per_guide = {}
    for w in ug.restate(haps, t, res, guidelen, len(pam), right, (0, 0), TABLES):
        for k in w.guides:
            per_guide[k] = w.cfdon
    order = res.reference_order(t).tolist()
    guides = []
    for k in order:
        i = int(res.src_row[k])
        strand = int(t.strand[i])
        guides.append(SimpleNamespace(start=int(t.start[i]), stop=int(t.stop[i]), strand=strand, sequence=seqs[k], guidelen=guidelen, pamlen=len(pam),
                                      right=(not right) if strand else right, _hip_hap=int(t.hap[i]), _hip_pos=int(t.pos[i])))
    caught = {}
    monkeypatch.setattr(reports, "report_frame", lambda inp, *a, **kw: caught.setdefault("inp", inp))
    reports.report_from_guides(guides, haps, pam, "chrP", "chrP:1-2", [per_guide[k] for k in order])
    inp = caught["inp"]
    perm, off = np.asarray(inp.group_perm), np.asarray(inp.group_off)
    theirs = {}
    for gi in range(len(off) - 1):
        rows = perm[off[gi]:off[gi + 1]].tolist()
        rep = rows[0]
        c = inp.cfdon[rep]
        theirs[frozenset(order[r] for r in rows)] = (seqs[order[rep]][GUIDESEQPAD:W - GUIDESEQPAD], None if c != c else round_score(float(c)),
                                                    int(inp.gc_num[gi]), int(inp.gc_den[gi]))
    g = ug.host_groups(haps, t, res, pam, guidelen, right, (0, 0), TABLES)
    want = ug.restate(haps, t, res, guidelen, len(pam), right, (0, 0), TABLES)
    ug.assert_groups_equal_restatement(g, want)
    wins = g.windows()
    mine = {frozenset(w.guides): (wins[gi][GUIDESEQPAD:W - GUIDESEQPAD], None if np.isnan(g.cfdon[gi]) else round_score(float(g.cfdon[gi])),
                                  int(g.gc_num[gi]), int(g.gc_den[gi])) for gi, w in enumerate(want)}
    assert mine == theirs


def test_scene_claims():
    """each added scene is what it says it is, by the restatement"""
    def groups(name, flank=(0, 0), tables=None):
        haps, pam, t, guidelen, right = SCENES[name]
        return ug.restate(haps, t, _resolved(name), guidelen, len(pam), right, flank, tables), haps
    w, haps = groups("shared_core")
    alt = [x for x in w if not x.is_ref]
    assert len(alt) == 1 and alt[0].members == [1, 2] and alt[0].hap == 1 and len(alt[0].guides) == 2
    w, _ = groups("pads")
    alt = [x for x in w if not x.is_ref]
    assert len(alt) == 1 and len(alt[0].guides) == 1024 and alt[0].members == [1] and alt[0].rep_k == min(alt[0].guides)
    w43, _ = groups("pads", (4, 3))
    assert len([x for x in w43 if not x.is_ref]) == 2 ** 7  # four ambiguous bases left of the core, three right of it
    w, _ = groups("core10_no_partner", tables=TABLES)
    assert len(w) == 1024 and all(np.isnan(x.cfdon) and len(x.guides) == 1 for x in w)
    w, _ = groups("core10", tables=TABLES)
    assert len(w) == 1 + 1023 and not any(np.isnan(x.cfdon) for x in w)
    w, _ = groups("no_partner", tables=TABLES)
    assert w and all(np.isnan(x.cfdon) for x in w)
    haps, pam, t, guidelen, right = SCENES["short_ref"]
    res = _resolved("short_ref")
    assert t.flags.tolist() == [1, 1] and res.n_kept.tolist() == [0, 2]  # REF's row is in the table and keeps nothing
    w, _ = groups("short_ref", tables=TABLES)
    assert len(w) == 2 and all(np.isnan(x.cfdon) and not x.is_ref for x in w)
    assert {SCENES[n][3] + len(SCENES[n][1]) + 20 for n in ("widest", "w33")} == {64, 33}
    assert any(int(s) == 1 for s in SCENES["strands_left"][2].strand) and any(int(s) == 0 for s in SCENES["strands_right"][2].strand)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_no_group_repeats_refs_core_under_another_origin(name):
    """the redundancy rule has removed every non-REF guide whose upper-cased core is REF's: no two groups differ in origin alone"""
    haps, pam, t, guidelen, right = SCENES[name]
    w = ug.restate(haps, t, _resolved(name), guidelen, len(pam), right)
    W = guidelen + len(pam) + 2 * GUIDESEQPAD
    seen = {}
    for x in w:
        seen.setdefault((x.start, x.strand, x.window[GUIDESEQPAD:W - GUIDESEQPAD].upper()), set()).add(x.is_ref)
    assert all(len(v) == 1 for v in seen.values())


def test_strand_one_flank_is_in_guide_orientation():
    """on strand 1 the guide's 5' side is the window's high side: (4, 0) reads four bases RIGHT of the core there"""
    haps, pam, t, guidelen, right = SCENES["strands_left"]
    res = _resolved("strands_left")
    for flank in [(4, 0), (0, 3), (10, 10)]:
        g = ug.host_groups(haps, t, res, pam, guidelen, right, flank, TABLES)
        ug.assert_groups_equal_restatement(g, ug.restate(haps, t, res, guidelen, len(pam), right, flank, TABLES))


def test_statuses_and_empty_input():
    haps, pam, t, guidelen, right = SCENES["options"]
    res = _resolved("options")
    for flank in [(11, 0), (0, 11)]:
        with pytest.raises(_lib.HawkStatusError) as e:
            ug.host_groups(haps, t, res, pam, guidelen, right, flank)
        assert e.value.status == _lib.HAWK_E_UNSUPPORTED
    empty = SimpleNamespace(src_row=np.zeros(0, np.uint32), win=np.zeros((5, 0), np.uint64))
    g = ug.host_groups(haps, t, empty, pam, guidelen, right)
    assert g.n_groups == 0 and g.n_members == 0 and g.member_off.tolist() == [0] and g.windows() == []
    bad = SimpleNamespace(src_row=res.src_row[::-1].copy(), win=res.win)  # not ascending: not what the resolution gives
    with pytest.raises(_lib.HawkStatusError) as e:
        ug.host_groups(haps, t, bad, pam, guidelen, right)
    assert e.value.status == _lib.HAWK_E_INVALID


def test_non_acgt_base_under_a_lookup_is_a_cfd_error():
    """an N in the spacer of a kept guide, where REF has a base: HAWK_E_CFD with tables, fine without"""
    haps, pam, t, guidelen, right = SCENES["options"]
    res = _resolved("options")
    win = res.win.copy()
    k = int(np.flatnonzero(res.src_row == 1)[0])
    for p in range(4):
        win[p, k] |= np.uint64(1) << np.uint64(GUIDESEQPAD + 3)
    broken = SimpleNamespace(src_row=res.src_row, win=win)
    with pytest.raises(_lib.HawkStatusError) as e:
        ug.host_groups(haps, t, broken, pam, guidelen, right, (0, 0), TABLES)
    assert e.value.status == _lib.HAWK_E_CFD
    assert ug.host_groups(haps, t, broken, pam, guidelen, right).n_groups > 0
