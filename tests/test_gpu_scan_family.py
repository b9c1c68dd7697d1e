"""The offset scans on every route, called on their own: hawk_launch_mscan (hawk_search.hip: k_mscan1 + k_mscan23, the wide pair
k_mscan1w + k_mscan23w, k_mscan1 / k_mscan2 / k_mscan3 with and without shard sums, with counts or offsets off their 16-byte boundary)
and hawk_launch_scan2_u32 (hawk_meta.hip) at the sizes where their loops take another trip - which no search or dictionary build of
test size reaches.  Only the hooks library exports the entry points (hawk_hooks_scan.hip), so every group runs in a process of its own
that loads it (tests/hooks_scan_check.py); tests/scan_refs.py names the cases, tests/test_scan_refs.py proves them on the CPU.

Every comparison is == on integers against np.cumsum in uint64.  The `big` panel (counts <= 65 536, totals of 2^33 ... 2^39) fails on
the M1_M23 route at 4 194 304 counts and on every WIDE case when the wave reductions of the second kernel sum the two 32-bit halves
apart (as they did before wave_sum64): the carries out of the low half are lost."""
import os
import subprocess
import sys

import pytest

import scan_refs as sc
from crisprhawk_hip import _lib

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", sc.GROUPS)
def test_scan_group(group):
    here = os.path.dirname(os.path.abspath(__file__))
    hooks = os.path.join(os.path.dirname(_lib.LIB_PATH), "libhawk_hip_hooks.so")
    assert os.path.exists(hooks), "make -C crispr-hawk_amd/csrc builds libhawk_hip_hooks.so beside the product library"
    env = dict(os.environ, CRISPRHAWK_HIP_LIB=hooks)
    r = subprocess.run([sys.executable, os.path.join(here, "hooks_scan_check.py"), group], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"hooks ok: {group}" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
