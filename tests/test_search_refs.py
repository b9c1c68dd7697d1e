"""The case builders of tests/test_gpu_search_seams.py, checked on the CPU: every case builds, proves from the oracle's output and
the position maps that it sits on the seam it is listed for, and stays inside the reference's domain - the scan range never
reaches where scan_haplotype would read past the row, which the oracle now refuses instead of comparing against stale memory."""
import numpy as np
import pytest

import search_refs as sr
from oracle import oracle as ora


def test_the_gpu_module_runs_exactly_these_cases():
    import test_gpu_search_seams as tg
    assert tg.SEARCH_CASES == list(sr.CASES) and sorted(sr.CASES) == sorted(sr.REQUIRED)
    assert set(sr.PAM_SCAN_SETS) <= set(sr.CASES)
    assert {f"tiles_{n}" for n in (1, 7, 8, 9, 15, 16, 17, 255, 256, 257, 1024, 1025, 2047, 2048, 2049, 3073)} <= set(sr.CASES)


@pytest.mark.parametrize("name", list(sr.CASES))
def test_every_case_proves_its_seam_from_the_oracle(name):
    c = sr.CASES[name]()
    assert c.name == name and c.proved
    missing = [frag for frag in sr.REQUIRED[name] if not any(frag in label for label in c.proved)]
    assert not missing, (name, missing)
    # inside the reference's domain: one REF row with the identity map, every scan range where scan_haplotype can read
    assert sum(c.is_ref) == 1 and c.is_ref[0] and len(sr.segment_starts(c.posmaps[0])) == 1
    assert c.in_domain()
    for seq, pm, (a, b) in zip(c.seqs, c.posmaps, c.scan):
        assert len(pm) == len(seq) and 0 <= a <= b <= len(seq) - c.pamlen + 1
        assert (np.diff(pm) >= 0).all()
    assert 13 <= c.L <= 44  # one padded window fits 64 bits
    t = c.tally()  # asserts its own totals against the oracle's n_hits / n_candidates
    assert sum(v["valid"] for v in t.values()) == len(c.want.guides)
    assert all(v["survivors"] <= 2 * sr.TILE and v["TF"] <= sr.TILE and v["TR"] <= sr.TILE for v in t.values())
    print(c.summary())


def test_a_case_off_its_seam_fails():
    c = sr.Case("drift", "NGG", 20, False, 1)
    ref = c.fill(400)
    c.plant(ref, 100, 0)
    c.add(ref, is_ref=True)
    with pytest.raises(AssertionError, match="off its seam"):
        c.prove("two rows", len(c.want.guides) == 2)
    assert len(c.want.guides) == 1 and not c.proved
    with pytest.raises(AssertionError, match="PAM letter"):
        c.swap(ref[121])


def test_the_tally_on_a_hand_made_pair():
    c = sr.Case("hand", "NGG", 20, False, 2)
    # + strand guides at 40 and 100, a - strand guide at 160; the alt row: a real SNV in the first, REF's own letter in lower
    # case in the second, a PAM REF lacks at 220
    sr.planted_pair(c, 400, [(40, 0, "snv"), (100, 0, "same"), (160, 1, "snv"), (220, 0, "new")])
    t = c.tally()
    assert c.bph == 1 and (t[(0, 0)]["survivors"], t[(0, 0)]["valid"], t[(0, 0)]["TF"], t[(0, 0)]["TR"]) == (3, 3, 2, 1)
    assert (t[(1, 0)]["survivors"], t[(1, 0)]["valid"], t[(1, 0)]["TF"], t[(1, 0)]["TR"], t[(1, 0)]["path"]) == (4, 3, 3, 1, "list")
    q, strand, _ = c.rows_of(1)
    assert sorted(zip(q.tolist(), strand.tolist())) == [(40, 0), (160, 1), (220, 0)]
    assert sorted(c.expected_flags().tolist()) == [0, 1, 1, 1, 1, 1]  # REF's three rows, the two SNV rows; not the new PAM's
    assert c.seqs[1][220 + 22] == "g" and c.seqs[0][220 + 22] in "AT" and c.seqs[0][220 + 21] == "G"
    # the arithmetic restated from the kernels
    assert sr.stride_words(32704) == 1024 and sr.tiles_per_row(32704) == 1 and sr.tiles_per_row(32705) == 2
    assert sr.scan_kernel(2048) == "k_mscan_one ipt=2" and sr.scan_kernel(2049) == "k_mscan1+k_mscan23 3 partials"
    assert sr.scan_kernel(1026, shards=False) == "k_mscan1/2/3 2 partials" and sr.pam_scan_partials(2049) == "k_mscan1/2/3 5 partials"
    assert sr.emit_path(512, False, 600) == "list" and sr.emit_path(513, False, 1100) == "recompute" and sr.emit_path(65536, True, 65536) == "128 rounds"
    pm = np.array([5, 6, 7, 7, 7, 8, 12, 13])
    assert sr.segment_starts(pm).tolist() == [0, 3, 4, 6]


@pytest.mark.parametrize("filler", ["A", "G"])
def test_the_oracle_refuses_a_scan_range_that_reads_past_the_row(filler):
    """ora_scan read hap[pos + i] behind the row when scan_stop > len - pamlen + 1 - stale heap or the previous row's bases, so
    the hit count depended on what lay there.  The reference raises IndexError in that range and compute_scan_start_stop never
    produces it: both entry points now return an error of their own, whatever the bases behind the row would have been."""
    assert -8 in ora.ERRORS
    bits, bitsrc, _, _ = ora.pam_encode("NGG")
    row = "AT" * 50 + "AGG" + "AT" * 13 + "TAG"  # 132 bases, ends on a G: one more G behind it would be a hit
    n = len(row)
    assert n == 132
    nib = ora.encode(row)
    fwd, rev = ora.scan(nib, 0, n - 2, bits, bitsrc, 3)  # the last range inside the domain
    assert fwd.tolist() == [100] and rev.tolist() == []
    for stop in (n - 1, n, n + 5):
        with pytest.raises(ora.OracleError) as e:
            ora.scan(nib, 0, stop, bits, bitsrc, 3)
        assert e.value.code == -8
    with pytest.raises(ora.OracleError) as e:
        ora.scan(nib, -1, 50, bits, bitsrc, 3)
    assert e.value.code == -8
    assert all(len(x) == 0 for x in ora.scan(nib, n + 5, n + 5, bits, bitsrc, 3))  # an empty range reads nothing
    pm = np.arange(1, n + 1, dtype=np.int64)
    prev = filler * 200  # the row whose bases the shared buffer still holds behind the short row
    pm0 = np.arange(1, 201, dtype=np.int64)
    good = ora.search(ora.HapSet([prev, row], [pm0, pm], [True, False], [(0, 198), (0, n - 2)]), "NGG", 20, False)
    assert good.n_hits == (198 if filler == "G" else 0) + 1
    for stop in (n - 1, n):
        with pytest.raises(ora.OracleError) as e:
            ora.search(ora.HapSet([prev, row], [pm0, pm], [True, False], [(0, 198), (0, stop)]), "NGG", 20, False)
        assert e.value.code == -8


def test_the_scan_routes_change_where_the_launcher_says():
    """hawk_mscan_route (hawk_search.hip) restated by sr.scan_route: both sides of every threshold, for every combination of shard
    sums and alignment."""
    route = lambda n, shards=True, aligned=True: sr.scan_route(n, shards, aligned)["route"]
    # one workgroup up to 2048 counts, with shard sums only
    assert [route(n) for n in (1, 2048, 2049)] == ["ONE", "ONE", "M1_M23"]
    assert [route(n, shards=False) for n in (1, 2048, 2049)] == ["M1_M2_M3"] * 3
    assert route(2048, aligned=False) == "ONE"
    # the fused second kernel up to 4096 partials of 1024, whatever the alignment
    assert [route(n) for n in (4096 * 1024, 4096 * 1024 + 1)] == ["M1_M23", "WIDE"]
    assert [route(n, aligned=False) for n in (4096 * 1024, 4096 * 1024 + 1)] == ["M1_M23", "M1_M2_M3"]
    # the wide pair up to 4096 partials of 4096, aligned and with shard sums only
    assert [route(n) for n in (4096 * 4096, 4096 * 4096 + 1)] == ["WIDE", "M1_M2_M3"]
    assert all(route(n, shards=False, aligned=a) == "M1_M2_M3" for n in (4096 * 1024, 4096 * 1024 + 1, 4096 * 4096) for a in (True, False))
    # the figures behind the route
    assert sr.scan_route(262_144)["partials"] == 256 and sr.scan_route(262_144)["trips"] == 1 and sr.scan_route(262_145)["trips"] == 1
    assert sr.scan_route(262_145)["partials"] == 257 and sr.scan_route(263_169)["trips"] == 2 and sr.scan_route(4096 * 1024)["trips"] == 16
    w = sr.scan_route(4_194_305)
    assert (w["partials"], w["tail"], w["trips"]) == (1025, 1, 4) and sr.scan_route(4096 * 4096)["partials"] == 4096
    u = sr.scan_route(4_194_305, aligned=False)
    assert (u["partials"], u["chunks"], u["last_chunk"], u["tail"]) == (4097, 5, 1, 1)
    m = sr.scan_route(1_048_577, shards=False)
    assert (m["partials"], m["chunks"], m["last_chunk"]) == (1025, 2, 1) and sr.scan_route(1_048_576, shards=False)["chunks"] == 1
    assert sr.scan_kernel(4_194_305) == "k_mscan1w+k_mscan23w 1025 partials"
    assert sr.scan_kernel(4_194_305, aligned=False) == "k_mscan1/2/3 4097 partials"
