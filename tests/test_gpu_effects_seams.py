"""The variant-effect stage on the device (csrc/hawk_effects.hip) past its first tile: every seam panel of effects_refs.py through
hawk_effects_create_columns and hawk_effects_rank, bit for bit against the plain reference (effects_refs.plain_effects: Python
floats, sets and sorted(), nothing of the library) and against the host twin, whose selection is a std::partial_sort.

What each family of cases is there for (the panels prove it of themselves, effects_refs.REQUIRED):
  round    fx_round4 / fx_delta as the device compiles them: ties, their neighbours, specials, the sign of zero
  merge    k_fx_topk_merge over 8 tiles of workgroup results: the filter against L[K-1], the join with L, the early return, the
           carry of a short L between tiles; K = 1, 25, 63, 64; candidates up to n_cand == K
  stride   k_fx_topk_part's own second tile (262 401 groups, the smallest table at which its loop iterates)
  queue    k_fx_samples_long taking a second queue entry: the bitmap cleared between entries; groups long by their entries
  edge     the short / long classification at 16 / 17 entries, bitmaps of 1, 2 and 3 words
  alts     k_fx_alts over positions of more than 64 groups, several REF groups, the running sum of alt_off over 64 positions
  shape    the widest and the narrowest core, both strands and `right`; k_fx_groups' counters over several workgroups
One handle serves every rank call of a case, as in the product: a call must not depend on what the one before left behind."""
import numpy as np
import pytest

from crisprhawk_hip import graphical_reports as gr
import effects_refs as refs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", refs.SEAM_CASES)
def test_device_equals_the_plain_reference_and_the_host_twin(name):
    p, order, calls, n_long = refs.seam_case(name)
    refs.check_required(p)
    dev = gr.GroupEffects(p, p.hap_samples, p.is_ref_hap, order, "device")
    host = gr.GroupEffects(p, p.hap_samples, p.is_ref_hap, order, "host")
    assert dev.perm is None and host.perm is None  # collapse order: group numbers mean the same to all three
    try:
        if n_long is not None:
            assert dev.timing["n_long"] == n_long
            if name == "queue":
                assert n_long > refs.FX_LONG_WAVES
        for family, score, cands, K in calls:
            got = dev.rank(family, score, cands, K)
            refs.results_equal(got, refs.plain_effects(p, order, family, score, cands, K))
            refs.results_equal(got, host.rank(family, score, cands, K))
    finally:
        dev.close(); host.close()


def test_round_panel_is_pythons_round_on_the_device():
    """stated without the plain reference: score, delta and abs_delta of every pair are round(a, 4), round(a, 4) - round(b, 4)
    and its abs() bit for bit, the sign of zero included"""
    p, order, score = refs.round_panel()
    dev = gr.GroupEffects(p, p.hap_samples, p.is_ref_hap, order, "device")
    try:
        r = dev.rank(gr.ABSOLUTE, score, (), 25)
    finally:
        dev.close()
    want = [round(x, 4) for x in score.tolist()]
    nan = float("nan")
    delta = []
    for i in range(0, len(want), 2):  # (REF, alternative)
        d = want[i + 1] - want[i]
        e = want[i] - want[i]
        delta += [nan if e != e else e, nan if d != d else d]
    for got, exp in ((r.score, want), (r.delta, delta), (r.abs_delta, [abs(x) for x in delta])):
        exp = np.array(exp, dtype=np.float64)
        bad = np.flatnonzero(got.view(np.uint64) != exp.view(np.uint64))
        assert len(bad) == 0, [(int(i), score[i - i % 2], score[i - i % 2 + 1], got[i], exp[i]) for i in bad[:10]]
