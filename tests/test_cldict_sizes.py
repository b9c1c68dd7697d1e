"""The sizes of a cluster-dictionary build (cl_build_sizes, csrc/hawk_cl.h): bounds, the two table sizes, the first attempt's probe
limit and status bit, the layout of the zero block and the plans the build declines.  The header is plain C++17: a small main is
compiled with the host compiler alone and prints what the function returns.  The expected values follow from the expressions of
the build as it was inline in xplan_build_dict; the two declined cases at the end are the sizes at which those expressions wrapped
(records + rows >= 2^32) or the packed rows of a cluster search could not hold the haplotype row (rows >= 2^23).  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "crispr-hawk_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "hawk_cl.h"
int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const ClBuildSizes s = cl_build_sizes(strtoull(argv[1], nullptr, 10), (uint32_t)strtoull(argv[2], nullptr, 10),
                                        (uint32_t)strtoull(argv[3], nullptr, 10), (uint32_t)strtoull(argv[4], nullptr, 10));
  printf("declined %d\n", (int)s.declined);
  printf("ch_bound %u\ninst_bound %u\nbm_words %u\ntsize %u\ntsmall %u\n", s.ch_bound, s.inst_bound, s.bm_words, s.tsize, s.tsmall);
  printf("max_probe %u\nfail_bit %u\nu_bound %u\nu_bound_repeat %u\n", s.max_probe, s.fail_bit, s.u_bound, s.u_bound_repeat);
  printf("status %zu\ncounters %zu\nresults %zu\ncnt %zu\nlcnt %zu\nclaim %zu\nvdesc %zu\nspan2 %zu\ntab %zu\nend %zu\n", s.z_status,
         s.z_counters, s.z_results, s.z_cnt, s.z_lcnt, s.z_claim, s.z_vdesc, s.z_span2, s.z_tab, s.z_end);
  printf("slot_bytes %zu\nresult_bytes %zu\n", sizeof(ClSlot), sizeof(ClResults));
  return 0;
}
"""
REGIONS = ["status", "counters", "results", "cnt", "lcnt", "claim", "vdesc", "span2", "tab", "end"]
FULL, FIRST = (0xFFFFFFFF, 2), (64, 8)  # (max_probe, fail_bit) of a first attempt that is the full table / a small one
C3 = (8_000_000, 5009, 30_000)          # a panel of the benchmark's order: records, rows, variants


@pytest.fixture(scope="module")
def sizes(tmp_path_factory):
    d = tmp_path_factory.mktemp("cldict_sizes")
    (d / "main.cpp").write_text(MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(d / "main.cpp"), "-o", str(d / "main")])
    seen = {}

    def run(ncar, rows, n_var, last):
        key = (ncar, rows, n_var, last)
        if key not in seen:
            out = subprocess.check_output([str(d / "main")] + [str(v) for v in key], text=True)
            seen[key] = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
        return seen[key]

    return run


def check_layout(s, n_var):
    """every offset a multiple of 256 - lcnt of 16 -, the regions in order, none inside another, cnt and lcnt in front of claim"""
    assert s["slot_bytes"] == 32 and s["result_bytes"] == 64
    for name in REGIONS:
        assert s[name] % (16 if name == "lcnt" else 256) == 0, name
    need = {"status": 4, "counters": 32, "results": 64, "cnt": 4 * s["ch_bound"], "lcnt": 4 * s["ch_bound"], "claim": 4 * s["bm_words"],
            "vdesc": 8 * max(n_var, 1), "span2": 4 * s["u_bound"], "tab": 32 * s["tsmall"]}
    for a, b in zip(REGIONS, REGIONS[1:]):
        assert s[a] + need[a] <= s[b], (a, b)
    assert s["end"] == s["tab"] + need["tab"]


def test_small_plan(sizes):
    s = sizes(1000, 10, 50, 0)
    assert s["declined"] == 0
    assert (s["ch_bound"], s["inst_bound"], s["bm_words"]) == (10, 1010, 2)
    assert (s["tsize"], s["tsmall"]) == (2048, 2048)
    assert (s["max_probe"], s["fail_bit"]) == FULL
    assert s["u_bound"] == 1060 and s["u_bound_repeat"] == 1060
    assert [s[k] for k in REGIONS] == [0, 256, 512, 768, 816, 1024, 1280, 1792, 6144, 71680]
    check_layout(s, 50)


def test_panel_first_build(sizes):
    s = sizes(*C3, 0)
    assert s["declined"] == 0
    assert (s["ch_bound"], s["inst_bound"]) == (12_821, 8_005_009)
    assert (s["tsize"], s["tsmall"]) == (1 << 24, 1 << 20)
    assert (s["max_probe"], s["fail_bit"]) == FIRST
    assert s["u_bound"] == 1_078_576 and s["u_bound_repeat"] == 8_035_009
    check_layout(s, C3[2])


def test_panel_sized_by_the_last_build(sizes):
    s = sizes(*C3, 40_000)
    assert s["tsmall"] == 131_072 and s["tsize"] == 1 << 24 and (s["max_probe"], s["fail_bit"]) == FIRST
    check_layout(s, C3[2])
    s = sizes(*C3, 10_000_000)  # more expected than the full table holds: the first attempt is the full one
    assert s["tsmall"] == s["tsize"] == 1 << 24 and (s["max_probe"], s["fail_bit"]) == FULL
    assert s["u_bound"] == s["u_bound_repeat"] == 8_035_009
    check_layout(s, C3[2])


@pytest.mark.parametrize("ncar,rows", [(0, 10), (1000, 1), ((1 << 32) - 3, 5), (1 << 31, 1 << 23)],
                         ids=["no-records", "one-row", "records+rows-wrap", "rows-beyond-packed-layout"])
def test_declined(sizes, ncar, rows):
    assert sizes(ncar, rows, 50, 0)["declined"] == 1


def test_largest_sizes_in_64_bits(sizes):
    s = sizes((1 << 31) + 5, 3, 50, 0)  # 2 x instances is beyond 32 bits: the table stops at 2^30 slots instead of wrapping to 1024
    assert s["declined"] == 0
    assert s["inst_bound"] == (1 << 31) + 8 and s["tsize"] == 1 << 30
    check_layout(s, 50)
    assert sizes((1 << 32) - 3, 2, 50, 0)["declined"] == 0  # records + rows = 2^32 - 1 still fits
