"""The hand-over between the two per-instance passes of the cluster search: k_cs_count leaves one 16-byte record per instance
{rows, first template row, haplotype row << HAWK_ROW_HAP_SHIFT, position}, and k_cs_emit_rows reads that stream and nothing of
the dictionary's arrays.

test_emit_group: k_cs_emit_rows at its own seams, on records and template rows of the test's making, against a numpy gather-copy
(tests/hooks_emit_check.py, in a process of its own that loads the hooks library: only that has hawk_hook_cs_emit).  The cases
follow the instantiation the launcher keeps (W instances per wave, C rows per chunk, both asked of the library): instance counts
on either side of a wave group and of one and four waves; a wave's row total on either side of one, two and three chunks; a wave
of no rows between two with rows; instances of no rows at a wave's ends; one instance of 2 C + 7 rows; the last haplotype row a
packed row can name; negative positions and adds that carry into bit 31; capacity exact, one row short (HAWK_E_CAPACITY, guard
untouched) and the template counter above its reservation (nothing written).

test_cluster_path_equals_word_path: whole searches of small panels, the cluster path against the per-word search of the same
view, row for row (sorted by content, == on every column): a view of fewer than 64 instances, views whose instance count is no
multiple of 64, one beyond 1024 instances, and a search whose first template reservation overflows and is rerun."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hooks_emit_check as he
from crisprhawk_hip import _lib, synth
from crisprhawk_hip.workload import expand_on_device
from oracle import oracle as ora
from test_gpu_vsearch import _canonical, COLS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", he.GROUPS)
def test_emit_group(group):
    here = os.path.dirname(os.path.abspath(__file__))
    hooks = os.path.join(os.path.dirname(_lib.LIB_PATH), "libhawk_hip_hooks.so")
    assert os.path.exists(hooks), "make -C crispr-hawk_amd/csrc builds libhawk_hip_hooks.so beside the product library"
    env = dict(os.environ, CRISPRHAWK_HIP_LIB=hooks)
    r = subprocess.run([sys.executable, os.path.join(here, "hooks_emit_check.py"), group], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"hooks ok: {group}" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("HAWK_VIEW_SEARCH", "HAWK_CLUSTER_MIN_SHARE", "HAWK_CLUSTER_MAX_SLOTS", "HAWK_CLUSTER_ROWS0"):
        monkeypatch.delenv(k, raising=False)


def _same_rows(a, c):
    assert (c.n_rows, c.n_candidates, c.n_hits) == (a.n_rows, a.n_candidates, a.n_hits)
    ca, cc = _canonical(a), _canonical(c)
    for k in COLS:
        assert np.array_equal(ca[k], cc[k]), k
    assert np.array_equal(ca["win"], cc["win"])
    assert np.array_equal(ca["cfdon"], cc["cfdon"], equal_nan=True)


# (seed, region length, variant sites, samples, first template reservation or None)
PANELS = [(7101, 3_000, 3, 2, None), (7102, 6_000, 14, 3, None), (7103, 9_000, 60, 4, None), (7104, 30_000, 1_400, 6, None),
          (7104, 30_000, 1_400, 6, 8)]


def test_cluster_path_equals_word_path(monkeypatch):
    monkeypatch.setenv("HAWK_CLUSTER_MIN_SHARE", "0")
    bits, bitsrc, _, _ = ora.pam_encode("NGG")
    mm, pt = synth.cfd_tables()
    seen = []
    for seed, length, n_var, n_samples, rows0 in PANELS:
        reg = synth.make_region(seed, "chrE", length, 500, length - 500)
        synth.add_phased_variants(reg, seed + 1, n_var, n_samples, frac_snv=0.6, frac_del=0.2, max_indel=6, af_min=0.2, af_max=0.8)
        ds, _info, _ms, _kept = expand_on_device(reg, 3, keep_plan=True)
        try:
            view = ds.plan.view()
            st = ds.plan.cluster_stats()
            assert st["usable"], st
            if rows0 is not None:
                monkeypatch.setenv("HAWK_CLUSTER_ROWS0", str(rows0))  # far fewer than the panel's template rows: the search is rerun
            c = view.search(bits, bitsrc, 3, 20, False, mm, pt)
            monkeypatch.delenv("HAWK_CLUSTER_ROWS0", raising=False)
            assert c.timing["v_path"] == 2
            monkeypatch.setenv("HAWK_VIEW_SEARCH", "words")
            b = view.search(bits, bitsrc, 3, 20, False, mm, pt)
            monkeypatch.delenv("HAWK_VIEW_SEARCH")
            assert b.timing["v_path"] == 1
            assert c.n_rows > 0
            _same_rows(b, c)
            seen.append(st["instances"])
        finally:
            ds.plan.close()
            ds.close()
    # conditions on the sweep, not measurements: what the panels above are there for
    assert any(n < 64 for n in seen), seen
    assert any(n % 64 for n in seen), seen
    assert any(n > 1024 for n in seen), seen
