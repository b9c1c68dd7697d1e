"""Shared by tests/test_ugroups_host.py and tests/test_gpu_unphased_groups.py: the report groups of an unphased table restated
in plain Python from resolve_refs objects (haplotypes, table rows, the twin's kept guides), the host twin
(hawk_host_unphased_groups) on the same objects, and the scenes the panel of resolve_refs lacks.

The restatement keys a dict as reports.report_from_guides keys it - (start, stop, strand, origin, cased core) - with the core
widened by the flank in guide orientation; CFDon is a plain ascending-position product over the tables on the reversed strings;
the representative is the minimum (hap, pos, k); the members are the sorted unique haplotypes.  Groups are listed in the order
csrc/hawk_ugroups.h documents: (start, strand, origin, stop, planes A, C, G, T, case of the key slice)."""
from types import SimpleNamespace

import numpy as np

import resolve_refs as rr
from crisprhawk_hip.coordinate import Coordinate
from crisprhawk_hip.guide import GUIDESEQPAD
from crisprhawk_hip.haplotype import Haplotype
from crisprhawk_hip.hapset import unphased_groups_host
from crisprhawk_hip.sequence import Sequence

FLANKS = [(0, 0), (4, 3)]
FIELDS = ("rep_src_row", "hap", "pos", "strand", "start", "stop", "is_ref", "cfdon", "win", "gc_num", "gc_den", "member_off", "member_hap")
_RC = str.maketrans("ACGTacgt", "TGCAtgca")
_CODE = rr._CODE


def _planes(s: str):
    """the five plane words of a string, bit 0 = leftmost base"""
    return tuple(sum(((_CODE[ch] >> p) & 1) << i for i, ch in enumerate(s)) for p in range(5))


def py_cfdon(core: str, refcore: str, strand: int, guidelen: int, mm, pt) -> float:
    """compute_cfd (cfdscore.py:53-95) on the two + strand cores: reverse complement on strand 1, then the mismatching positions of
    the first min(guidelen, 20) spacer bases in ascending order, then PAM[-2:] of the guide - one multiply each, left to right"""
    g, r = core.upper(), refcore.upper()
    if strand:
        g, r = g[::-1].translate(_RC), r[::-1].translate(_RC)
    score = 1.0
    for t in range(min(guidelen, 20)):
        if g[t] != r[t]:
            score *= float(mm[t, "ACGT".index(r[t]), "ACGT".index(g[t])])
    return score * float(pt[4 * "ACGT".index(g[-2]) + "ACGT".index(g[-1])])


def restate(haps, t, res, guidelen: int, pamlen: int, right: bool, flank=(0, 0), tables=None):
    """-> list of groups (SimpleNamespace), in the documented order"""
    W = guidelen + pamlen + 2 * GUIDESEQPAD
    seqs = res.windows()
    up, down = flank
    refguide = {}
    for k, i in enumerate(res.src_row.tolist()):
        if haps[int(t.hap[i])].samples == "REF":
            assert (int(t.start[i]), int(t.strand[i])) not in refguide
            refguide[(int(t.start[i]), int(t.strand[i]))] = seqs[k]
    groups = {}
    for k, i in enumerate(res.src_row.tolist()):
        strand = int(t.strand[i])
        fl, fr = (down, up) if strand else (up, down)
        key = (int(t.start[i]), int(t.stop[i]), strand, haps[int(t.hap[i])].samples == "REF", seqs[k][GUIDESEQPAD - fl:W - GUIDESEQPAD + fr])
        groups.setdefault(key, []).append((int(t.hap[i]), int(t.pos[i]), k))
    out = []
    for key, members in groups.items():
        hap, pos, k = min(members)
        start, stop, strand, origin, kslice = key
        core = seqs[k][GUIDESEQPAD:W - GUIDESEQPAD]
        partner = refguide.get((start, strand))
        cfd = float("nan")
        if tables is not None and partner is not None:
            cfd = py_cfdon(core, partner[GUIDESEQPAD:W - GUIDESEQPAD], strand, guidelen, *tables)
        spacer = core[pamlen:] if (right != bool(strand)) else core[:guidelen]
        gc = sum(spacer.count(c) for c in "CGScgs")
        out.append(SimpleNamespace(sort=(start, strand, int(origin), stop) + _planes(kslice), rep_src_row=int(res.src_row[k]), hap=hap, pos=pos,
                                   strand=strand, start=start, stop=stop, is_ref=int(origin), cfdon=cfd, window=seqs[k], gc_num=gc,
                                   gc_den=gc + sum(spacer.count(c) for c in "ATWUatwu"), members=sorted({m[0] for m in members}),
                                   guides=sorted(m[2] for m in members), rep_k=k))
    out.sort(key=lambda g: g.sort)
    return out


def host_groups(haps, t, res, pam, guidelen: int, right: bool, flank=(0, 0), tables=None):
    """hawk_host_unphased_groups on the rows and the twin's kept guides"""
    hap_len = np.array([len(h) for h in haps], np.uint32)
    is_ref = np.array([h.samples == "REF" for h in haps], np.uint8)
    return unphased_groups_host(t.hap, t.pos, t.strand, t.start, t.stop, t.flags, t.win, hap_len, is_ref, res.src_row, res.win, pam.bits, pam.bitsrc,
                                guidelen, len(pam), right, tables, flank)


def assert_groups_equal_restatement(g, want):
    """every array of an UnphasedGroups against the restatement, bit for bit"""
    assert g.n_groups == len(want) and g.n_members == sum(len(w.members) for w in want)
    for f in ("rep_src_row", "hap", "pos", "strand", "start", "stop", "is_ref", "gc_num", "gc_den"):
        assert np.asarray(getattr(g, f)).tolist() == [getattr(w, f) for w in want], f
    assert g.windows() == [w.window for w in want]
    mine, theirs = np.asarray(g.cfdon, np.float64), np.array([w.cfdon for w in want], np.float64)
    assert mine.tobytes() == theirs.tobytes() or (np.array_equal(np.isnan(mine), np.isnan(theirs))
                                                  and np.array_equal(mine[~np.isnan(mine)].view(np.uint64), theirs[~np.isnan(theirs)].view(np.uint64)))
    off = np.asarray(g.member_off).astype(np.int64)
    assert off[0] == 0 and off[-1] == g.n_members
    assert [np.asarray(g.member_hap)[off[i]:off[i + 1]].tolist() for i in range(g.n_groups)] == [w.members for w in want]


def assert_groups_equal(a, b):
    """two UnphasedGroups, every output array, bit for bit (NaN payloads aside: both sides write the same quiet NaN)"""
    assert (a.n_groups, a.n_members) == (b.n_groups, b.n_members)
    for f in FIELDS:
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f


# ---------------------------------------------------------------------------- scenes the panel lacks
def shared_core_scene() -> rr.Scene:
    """two haplotypes with the same variant base in one guide's spacer: one group, two members"""
    s = rr.Scene("shared_core", "NGG", 20, False, seed=50)
    s.plant(200, "AGG")
    s.ref[190] = "A"
    s.copy("S1", {190: ("r", rr.AG)})
    s.copy("S2", {190: ("r", rr.AG), 150: ("w", [(s.ref[150], "T" if s.ref[150] == "A" else "A")])})
    return s


def pads_scene() -> rr.Scene:
    """ten two-way positions all in the pads (five on either side) behind one fixed variant base in the spacer: 1024 kept
    guides with ONE core - one group at flank (0, 0); (4, 3) reads four of the left and three of the right ones"""
    s = rr.Scene("pads", "NGG", 20, False, seed=51)
    s.plant(200, "AGG")
    s.ref[190] = "A"
    edits = {190: ("g", None)}
    for p in list(range(175, 180)) + list(range(203, 208)):
        edits[p] = ("w", [(s.ref[p], "T" if s.ref[p] == "A" else "A")])
    s.copy("S1", edits)
    return s


def short_ref_rows(guidelen: int = 20):
    """A REF haplotype that ends where the window of its strand-1 guide ends (a row of the table, not valid: it keeps nothing) and
    a longer copy with a variant base in that guide: the copy's guide has a REF ROW at its (start, strand) and no REF partner.
    -> (region, haps, pam, t)"""
    s = rr.Scene("short_ref", "NGG", guidelen, False, seed=52)
    p = s.plant(200, "CCA")
    s.ref[p + 8] = "A"
    s.copy("S1", {p + 8: ("r", rr.AG)})
    region, haps, pam = s.build()
    m = p + guidelen + 3 + GUIDESEQPAD  # the window [p - 10, m) ends with REF
    ref = Haplotype(Sequence("".join(s.ref[:m]), True), Coordinate("chrP", s.g0, s.g0 + m - 1, 0), False, 0, True)
    ref.id = haps[0].id
    haps = [ref] + haps[1:]
    t = rr.derive_rows(haps, [([], [p]), ([], [p])], len(pam), guidelen, False)
    return region, haps, pam, t


def scenes(with_region: bool = False):
    """name -> (haps, pam, t, guidelen, right) of the panel and of the scenes added here; with_region: the region in front (what
    search_guides._device_set needs to put the same haplotypes on the device)"""
    out = {}
    added = [shared_core_scene(), pads_scene(), rr.wide_row_scene(10, "core10"), rr.wide_row_scene(10, "core10_no_partner", partner=False)]
    for s in list(rr.panel().values()) + added:
        region, haps, pam, t = s.rows()
        out[s.name] = (region, haps, pam, t, s.guidelen, s.right)
    out["short_ref"] = short_ref_rows() + (20, False)
    return out if with_region else {k: v[1:] for k, v in out.items()}
