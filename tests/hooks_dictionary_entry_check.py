"""Run by tests/test_gpu_dictionary_walk.py::test_collisions_on_a_list_with_a_head_launch in a process of its own, with
CRISPRHAWK_HIP_LIB naming libhawk_hip_hooks.so - the library built with -DHAWK_TEST_HOOKS, the only build in which the cluster
dictionary's key can be weakened.

The panel is large enough (records + rows >= 16 x 16384) that k_cl_enter runs the head of the list as a launch of its own, and
every cluster has listed instances in both launches: those of the later launch find their clusters' slots taken and numbered.  With
HAWK_CLUSTER_WEAK_HASH=1 every cluster that starts with the same record lands in one slot: clusters that differ behind the first
record ({A, B} / {A, B'} / {A, B''}, {A, B} / {A, B, C}) set status bit 2 and the per-word search takes the plan; clusters that
really are the same ({A, B} everywhere) are merged.  With the full key all three panels give status 0.  At this size the view's
table is compared with the plane search's (the small panels of hooks_cluster_check.py are compared with the oracle)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "crispr-hawk_amd"), HERE]

from crisprhawk_hip import _lib, synth  # noqa: E402
from crisprhawk_hip.workload import expand_on_device  # noqa: E402
from oracle import oracle as ora  # noqa: E402
from test_gpu_clusters import Panel, _same_rows  # noqa: E402

N_SAMPLES = 800
HEAD_LISTED = 16384  # CL_HEAD_LISTED (hawk_cldict.hip)


def entry_panel(seed, kind):
    """test_gpu_clusters.collision_panel at scale: 170 isolated SNVs carried by all 1600 copies, then 12 clusters that share their
    first record A - 'alt': {A, B}, {A, B'} (another ALT at B's site), {A, B''} (1 nt from B), a third of the copies each; 'longer':
    {A, B}, {A, B, C}, half of the copies each; 'same': {A, B} in every copy - the carriers of each spread over all rows, so that
    every one of them is met in both launches of k_cl_enter; every copy with a private SNV elsewhere."""
    n_col = 2 * N_SAMPLES
    p = Panel(seed, 170 * 100 + 12 * 1_000 + 3 * n_col + 2_000, N_SAMPLES)
    everyone = range(n_col)
    i = 500
    for _ in range(170):
        p.snv(i, everyone)
        i += 100
    for _ in range(12):
        p.snv(i, everyone)
        if kind == "alt":
            p.snv(i + 20, range(0, n_col, 3), shift=1)
            p.snv(i + 20, range(1, n_col, 3), shift=2)
            p.snv(i + 21, range(2, n_col, 3))
        elif kind == "longer":
            p.snv(i + 20, everyone)
            p.snv(i + 40, range(1, n_col, 2))
        else:
            p.snv(i + 20, everyone)
        i += 1_000
    for c in range(n_col):
        p.snv(i + 3 * c, [c])
    return p.region()


def check(kind, path):
    """the default search of the plan's view takes `path`; its table holds the plane search's rows -> cluster_stats()"""
    reg = entry_panel(9931, kind)
    bits, bitsrc, _, _ = ora.pam_encode("NGG")
    mm, pt = synth.cfd_tables()
    ds, info, _ms, kept = expand_on_device(reg, 3, keep_plan=True)
    try:
        records = sum(len(inf.variant_idx) for inf in info)
        assert ds.plan.n_hap == 2 * N_SAMPLES + 1 and records + ds.plan.n_hap >= 16 * HEAD_LISTED  # the head launch of k_cl_enter runs
        assert 12 * 2 * N_SAMPLES > HEAD_LISTED  # ... and leaves listed instances of every cluster to the later launch
        a = ds.search(bits, bitsrc, 3, 20, False, mm, pt)
        view = ds.plan.view()
        st = ds.plan.cluster_stats()
        c = view.search(bits, bitsrc, 3, 20, False, mm, pt)
        assert c.timing["v_path"] == path, (kind, c.timing["v_path"], st)
        assert st["usable"] == (path == 2), (kind, st)
        assert c.n_rows > 0
        _same_rows(a, c)
        return st
    finally:
        ds.plan.close()
        ds.close()


def main() -> int:
    assert os.path.basename(_lib.LIB_PATH) == "libhawk_hip_hooks.so", _lib.LIB_PATH
    os.environ["HAWK_CLUSTER_MIN_SHARE"] = "0"
    for k in ("HAWK_VIEW_SEARCH", "HAWK_CLUSTER_MAX_SLOTS", "HAWK_CLUSTER_WEAK_HASH"):
        os.environ.pop(k, None)
    for kind in ("alt", "longer", "same"):  # the full key: no collision, the dictionary is used
        st = check(kind, 2)
        assert st["status"] == 0, (kind, st)
    os.environ["HAWK_CLUSTER_WEAK_HASH"] = "1"
    for kind in ("alt", "longer"):
        st = check(kind, 1)
        assert st["status"] & 2 and not st["usable"], (kind, st)
    st = check("same", 2)  # colliding and equal: merged, and right
    assert st["status"] == 0, st
    print("hooks ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
