"""Run by tests/test_gpu_clusters.py::test_dictionary_compare_catches_hash_collisions in a process of its own, with
CRISPRHAWK_HIP_LIB naming libhawk_hip_hooks.so - the library built with -DHAWK_TEST_HOOKS, the only build in which the cluster
dictionary's key can be weakened.

With HAWK_CLUSTER_WEAK_HASH=1 a listed instance's key is the hash of its FIRST record alone, so every cluster that starts with
the same record lands in one slot of the table.  k_cl_uid compares each instance with the one that opened its slot, record by
record: clusters that differ behind the first record ({A, B} / {A, B'}, {A, B} / {A, B, C}) set status bit 2, the dictionary is
not used and the per-word search gives the oracle's rows; clusters that really are the same ({A, B} everywhere) are merged and the
per-cluster search gives the oracle's rows."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "crispr-hawk_amd"), HERE]

from crisprhawk_hip import _lib  # noqa: E402
from test_gpu_clusters import _view_check, collision_panel  # noqa: E402


def main() -> int:
    assert os.path.basename(_lib.LIB_PATH) == "libhawk_hip_hooks.so", _lib.LIB_PATH
    os.environ["HAWK_CLUSTER_MIN_SHARE"] = "0"
    for k in ("HAWK_VIEW_SEARCH", "HAWK_CLUSTER_MAX_SLOTS", "HAWK_CLUSTER_WEAK_HASH"):
        os.environ.pop(k, None)
    st = _view_check(collision_panel(9801, "alt"), "NGG", 20, False, 2)  # the full key: no collision, the dictionary is used
    assert st["status"] == 0, st
    os.environ["HAWK_CLUSTER_WEAK_HASH"] = "1"
    for kind in ("alt", "longer"):
        st = _view_check(collision_panel(9801, kind), "NGG", 20, False, 1)
        assert st["status"] & 2 and not st["usable"], (kind, st)
    st = _view_check(collision_panel(9801, "same"), "NGG", 20, False, 2)  # colliding and equal: merged, and right
    assert st["status"] == 0, st
    print("hooks ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
