"""The cutting passes of the cluster dictionary (k_cl_count / k_cl_fill, cl_cut in hawk_cldict.hip) beyond the seams
tests/test_gpu_clusters.py pins, and the table passes at the size where the head of the list is a launch of its own:
  1. clusters of 5, 8, 9 and 70 records (the walk takes a cluster's second and third record from the lanes above and every further
     one from memory) that end at a wave's last lane, one before it and one past it, or run through the end of a slice or a chunk;
     one of 130 records across two whole waves;
  2. pairs of records 64 / 65 reference bases apart whose second record is the first lane of a wave, a slice or a chunk - the
     record in front of it belongs to another wave - or the last lane;
  3. variants carried only by the rows of the first 96 chunks (the counting pass describes them and claims them in the bitmap),
     only by later rows (the cutting pass describes them), and by both; the dictionary built twice;
  4. hash collisions among instances that the two launches of k_cl_enter meet (the hooks library, a process of its own).
Every case compares the view's table with the plane search's and with the oracle's rows, and the dictionary's counts with a host count."""
import os
import subprocess
import sys

import numpy as np
import pytest

from crisprhawk_hip import _lib, synth
from crisprhawk_hip.workload import expand_on_device
from oracle import oracle as ora
from test_gpu_clusters import Panel, _host_clusters, _host_distinct, _same_rows, _view_check
from test_gpu_clusters import _by_label, _sub_region
from test_gpu_vsearch import _oracle_rows, _table_rows

pytestmark = pytest.mark.gpu

BASES = "ACGT"


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("HAWK_VIEW_SEARCH", "HAWK_CLUSTER_MAX_SLOTS", "HAWK_CLUSTER_WEAK_HASH"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("HAWK_CLUSTER_MIN_SHARE", "0")


def _layout_panel(seed, layouts):
    """Rows laid out record by record, as test_gpu_clusters._seams_panel does: isolated SNVs 70 nt apart, cluster members 20 nt
    apart; a layout = {record index: cluster size}, carried by two copies that differ in a last private SNV."""
    n_rec = max(max(k + size for k, size in lay.items()) for lay in layouts) + 3
    p = Panel(seed, n_rec * 70 + 2_000, len(layouts))
    for li, multi in enumerate(layouts):
        cols = [2 * li, 2 * li + 1]
        n = max(k + size for k, size in multi.items()) + 2  # two isolated records behind the last cluster
        i, k = 300, 0
        while k < n:
            size = multi.get(k, 1)
            for m in range(size):
                p.snv(i, cols)
                i += 20 if m + 1 < size else 70
            k += size
        p.snv(i, cols[:1])
        p.snv(i + 1, cols[1:])
    return p.region()


# ---- 1: the walk leaves the wave ---------------------------------------------------------------------------------------------
SIZES = (5, 8, 9, 70)
WAVE_STARTS = (55, 56, 58, 59, 60, 63, 64)  # 5 @ 58 / 59 / 60, 8 @ 55 / 56, 9 @ 55 / 56: last record at lane 62 / 63 / 64
SLICE_STARTS = (250, 255)
CHUNK_STARTS = (1018, 1023)


def _walk_layouts():
    """one layout per (size, start in the first wave); the slice-end and chunk-end starts ride along in the first layouts (another
    wave of the same row: the walks do not meet), the 130-record cluster in one of its own"""
    layouts = [{start: size} for size in SIZES for start in WAVE_STARTS]
    extra = [(size, start) for size in SIZES for start in SLICE_STARTS] + [(size, start) for size in SIZES for start in CHUNK_STARTS]
    for lay, (size, start) in zip(layouts, extra):
        lay[start] = size
    layouts.append({40: 130})  # records 40..169: lanes 40..63 of the first wave, all of the second, 0..41 of the third
    return layouts


def test_walk_leaves_the_wave():
    layouts = _walk_layouts()
    want = {(size, start) for size in SIZES for start in WAVE_STARTS + SLICE_STARTS + CHUNK_STARTS} | {(130, 40)}
    assert {(size, start) for lay in layouts for start, size in lay.items()} == want
    reg = _layout_panel(9901, layouts)

    def counts(st, plan, info, kept):
        inst, distinct = _host_clusters(reg, info)
        assert {len(d) for d in distinct} == {1, 5, 8, 9, 70, 130}
        assert st["status"] == 0 and st["instances"] == inst and st["distinct"] == len(distinct), (st, inst, len(distinct))
        assert st["distinct"] == _host_distinct(reg, plan, info, kept)
    _view_check(reg, "NGG", 20, False, 2, stats=counts)


# ---- 2: the record in front comes from another wave ------------------------------------------------------------------------
def _front_panel(seed):
    """Rows of isolated SNVs 70 nt apart in which the records at k - 1 and k are a pair 64 (one cluster) or 65 (two) reference bases
    apart, the first of the pair an SNV, an insertion or a deletion in turn: k = 64, 128, 256, 1024 in one layout, 63, 255, 1023 in
    the other; each layout with either gap, carried by two copies that differ in a last private SNV."""
    layouts = [(ks, gap) for ks in ((64, 128, 256, 1024), (63, 255, 1023)) for gap in (64, 65)]
    p = Panel(seed, 1030 * 70 + 3_000, len(layouts))
    kinds = ("snv", "ins", "del")
    for li, (ks, gap) in enumerate(layouts):
        cols = [2 * li, 2 * li + 1]
        i, turn = 300, li
        for k in range(max(ks) + 3):
            if k + 1 in ks:  # the first record of a pair: the next one starts `gap` bases behind its allele
                kind = kinds[turn % 3]
                turn += 1
                e = {"snv": lambda: p.snv(i, cols), "ins": lambda: p.insertion(i, 4, cols), "del": lambda: p.deletion(i, 4, cols)}[kind]()
                i = e + gap
            else:
                i = p.snv(i, cols) + 69
        p.snv(i, cols[:1])
        p.snv(i + 1, cols[1:])
    return p.region(), layouts


def test_record_in_front_from_another_wave():
    reg, layouts = _front_panel(9911)

    def counts(st, plan, info, kept):
        inst, distinct = _host_clusters(reg, info)
        pairs = sum(len(ks) for ks, gap in layouts if gap == 64)
        assert sum(1 for d in distinct if len(d) == 2) == pairs and max(len(d) for d in distinct) == 2
        assert st["status"] == 0 and st["instances"] == inst and st["distinct"] == len(distinct), (st, inst, len(distinct))
        assert st["distinct"] == _host_distinct(reg, plan, info, kept)
        # the records sit where the layout says: the pair's second record is record k of its row
        pos = np.array([v.pos for v in reg.variants], dtype=np.int64)
        end = pos + np.array([len(v.ref) for v in reg.variants], dtype=np.int64)
        rows = [np.sort(np.asarray(inf.variant_idx, dtype=np.int64)) for inf in info if len(inf.variant_idx)]
        seen = []
        for idx in rows:  # (the two layouts differ in their rows' lengths)
            ks = next(ks for ks, _ in layouts if len(idx) == max(ks) + 4)
            gaps = {int(pos[idx[k]] - end[idx[k - 1]]) for k in ks}
            assert len(gaps) == 1, (len(idx), gaps)
            seen.append((ks, gaps.pop()))
        assert sorted(seen) == sorted(layouts + layouts)
    _view_check(reg, "NGG", 20, False, 2, stats=counts)


# ---- 3: claims from the counting pass --------------------------------------------------------------------------------------
HEAD_CHUNKS = 96  # CL_HEAD_CHUNKS (hawk_cldict.hip)


def _claims_panel(seed, n_var=2000, step=40, af=0.05, n_samples=800):
    """n_var SNVs `step` nt apart, every copy carries each with probability af; then, by hand, variants carried only by some of the
    first HEAD_CHUNKS copies, only by later copies, and by both - alone in their cluster in every carrier (the neighbours within
    reach are taken from it), so that each of them is a cluster that is its variant.  -> region, {kind: variant indices}"""
    length = step * n_var + 600
    reg = synth.make_region(seed, "chrK", length + 2_000, 1_000, 1_000 + length - 201)
    rng = np.random.default_rng(seed + 1)
    seq = reg.sequence.upper()
    n_col = 2 * n_samples
    G = (rng.random((n_var, n_col), dtype=np.float32) < af).astype(np.uint8)
    forced = {"head": (300, 700, 1100), "later": (400, 800, 1200), "both": (500, 900, 1300)}
    carriers = {"head": np.array([0, 5, 40, 95]), "later": np.array([96, 97, 700, 1599]), "both": np.array([3, 95, 96, 1000])}
    for kind, vs in forced.items():
        for v in vs:
            G[v] = 0
            G[v, carriers[kind]] = 1
            for d in (-2, -1, 1, 2):  # 64 nt reach at 40 nt spacing: the next variant each way; the one after it for good measure
                G[v + d, carriers[kind]] = 0
    reg.samples = [f"S{s:04d}" for s in range(n_samples)]
    out = []
    for k in range(n_var):
        i = 300 + step * k
        r = seq[i]
        out.append(synth.VariantSite(reg.startp + i, r, BASES[(BASES.index(r) + 1 + k % 3) % 4], float(G[k].mean()), G[k].reshape(n_samples, 2)))
    reg.variants = out
    reg.gt_matrix = G
    return reg, forced, carriers


def test_claims_from_the_counting_pass():
    reg, forced, carriers = _claims_panel(9921)
    pam_s, guidelen = "NGG", 20
    bits, bitsrc, _, _ = ora.pam_encode(pam_s)
    mm, pt = synth.cfd_tables()
    ds, info, _ms, kept = expand_on_device(reg, 3, keep_plan=True)
    try:
        # the chunk geometry the launches see: rows in plan order, chunks of 1024 records; every row here is one chunk
        rows = [np.sort(np.asarray(inf.variant_idx, dtype=np.int64)) for inf in info if len(inf.variant_idx)]
        assert len(rows) == 2 * len(reg.samples) and max(len(r) for r in rows) <= 1024
        bound = sum(len(r) for r in rows) // 1024 + ds.plan.n_hap
        assert bound >= 16 * HEAD_CHUNKS  # the counting pass leaves claims (hawk_launch_cl_count)
        for kind, vs in forced.items():
            for v in vs:
                chunks = [b for b, r in enumerate(rows) if v in r]
                assert len(chunks) == len(carriers[kind])
                assert {"head": all(b < HEAD_CHUNKS for b in chunks), "later": all(b >= HEAD_CHUNKS for b in chunks),
                        "both": any(b < HEAD_CHUNKS for b in chunks) and any(b >= HEAD_CHUNKS for b in chunks)}[kind], (kind, v, chunks)
        view = ds.plan.view()
        a = ds.search(bits, bitsrc, 3, guidelen, False, mm, pt)
        inst, _ = _host_clusters(reg, info)
        distinct = _host_distinct(reg, ds.plan, info, kept)
        seen = []
        for rebuild in (False, True):  # the second build sizes its table from the first one's count
            if rebuild:
                ds.plan.rebuild_dictionary()
            st = ds.plan.cluster_stats()
            assert st["status"] == 0 and st["usable"] and st["instances"] == inst and st["distinct"] == distinct, (rebuild, st, inst, distinct)
            seen.append((st["instances"], st["distinct"], st["template_slots"]))
            c = view.search(bits, bitsrc, 3, guidelen, False, mm, pt)
            assert c.timing["v_path"] == 2
            _same_rows(a, c)
        assert seen[0] == seen[1]
        got = _by_label(_table_rows(c, info, kept, True))
        # a dozen sampled carriers against the oracle: the samples whose copies carry the forced variants among them
        picks = sorted({int(col) // 2 for cols in carriers.values() for col in cols} | {100, 400, 600})
        assert len(picks) == 12
        sub = _sub_region(reg, picks)
        want, _, _ = _oracle_rows(sub, pam_s, guidelen, False, mm, pt)
        want = _by_label(want)
        assert want.pop(("REF",)) == got[("REF",)]
        assert len(want) >= 2 * len(picks) - 2
        for lab, rws in want.items():
            mine = [k for k in got if lab[0] in k]
            assert len(mine) == 1 and set(lab) <= set(mine[0]), lab
            assert got[mine[0]] == rws, lab
    finally:
        ds.plan.close()
        ds.close()


# ---- 4: collisions at the size of the head launch ---------------------------------------------------------------------------------------------------
def test_collisions_on_a_list_with_a_head_launch():
    """The record-by-record compare against real collisions on a list long enough that k_cl_enter runs its head as a launch of its own
    (the colliding instances enter the table in either launch): only the hooks library (-DHAWK_TEST_HOOKS) can weaken the dictionary's
    key, so the check runs in a process of its own that loads it (tests/hooks_dictionary_entry_check.py)."""
    here = os.path.dirname(os.path.abspath(__file__))
    hooks = os.path.join(os.path.dirname(_lib.LIB_PATH), "libhawk_hip_hooks.so")
    assert os.path.exists(hooks), "make -C crispr-hawk_amd/csrc builds libhawk_hip_hooks.so beside the product library"
    env = dict(os.environ, CRISPRHAWK_HIP_LIB=hooks)
    r = subprocess.run([sys.executable, os.path.join(here, "hooks_dictionary_entry_check.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "hooks ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
