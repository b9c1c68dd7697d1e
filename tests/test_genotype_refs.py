"""The references tests/test_gpu_genotypes.py measures the device against, checked on the CPU: the vectorised lists reference
equals oracle.carried_lists (the double loop it restates), and the seam helpers say where a field start falls."""
import numpy as np
import pytest

import genotype_refs as gr
from oracle import oracle as ora


def _random_case(rng, n_lines, n_cols, n_var, max_alt=3, chain_lim=9):
    codes = rng.choice(np.array([0, 1, 2, 3, 255], np.uint8), (n_lines, n_cols), p=[0.55, 0.2, 0.1, 0.1, 0.05])
    var_line = rng.integers(0, n_lines, n_var).astype(np.uint32)  # not monotone, lines shared by several variants
    var_allele = rng.integers(1, max_alt + 1, n_var).astype(np.uint8)
    var_r0 = rng.integers(0, 5000, n_var).astype(np.int32)
    var_chain = (rng.integers(-chain_lim, chain_lim + 1, n_var) * (rng.random(n_var) < 0.6)).astype(np.int32)
    return codes, var_line, var_allele, var_r0, var_chain


@pytest.mark.parametrize("seed", range(12))
def test_vectorised_lists_equal_the_oracle_loop(seed):
    rng = np.random.default_rng(7100 + seed)
    n_lines, n_cols, n_var = int(rng.integers(1, 40)), 2 * int(rng.integers(1, 40)), int(rng.integers(0, 150))
    codes, vl, va, r0, ch = _random_case(rng, n_lines, n_cols, n_var)
    codes[:, 0] = 0                       # an empty column in front
    codes[:, -1] = 255                    # a column of missing alleles behind: 255 never matches
    if n_cols > 4:
        codes[:, 2] = 1                   # a column that is one allele throughout
    got = gr.carried_lists_np(codes, vl, va, r0, ch, col_block=int(rng.integers(1, 9)))
    w_off, w_idx, w_o, w_delta = ora.carried_lists(codes, vl, va, r0, ch)
    assert np.array_equal(got[0], w_off) and got[0].dtype == np.uint64
    assert np.array_equal(got[1], w_idx) and np.array_equal(got[2], w_o) and np.array_equal(got[3], w_delta)
    assert np.array_equal(got[4], np.flatnonzero(ch[w_idx] != 0))
    assert got[0][1] == 0 and got[0][-1] == got[0][-2]


def test_vectorised_lists_negative_runs_and_empty_tables():
    codes = np.array([[1, 0], [1, 2], [1, 2], [1, 1]], np.uint8)
    vl, va = np.array([0, 1, 1, 2, 3], np.uint32), np.array([1, 1, 2, 1, 1], np.uint8)
    r0, ch = np.array([10, 20, 20, 30, 40], np.int32), np.array([-100000, 7, 3, 99999, 0], np.int32)
    off, idx, o, delta, ind = gr.carried_lists_np(codes, vl, va, r0, ch)
    assert off.tolist() == [0, 4, 6] and idx.tolist() == [0, 1, 3, 4, 2, 4]
    assert o.tolist() == [10, 20 - 100000, 30 - 99993, 40 + 6, 20, 43] and delta.tolist() == [6, 3] and ind.tolist() == [0, 1, 2, 4]
    w = ora.carried_lists(codes, vl, va, r0, ch)
    assert np.array_equal(off, w[0]) and np.array_equal(idx, w[1]) and np.array_equal(o, w[2]) and np.array_equal(delta, w[3])
    z = np.zeros(0, np.int32)
    off, idx, o, delta, ind = gr.carried_lists_np(codes, z, z, z, z)
    assert off.tolist() == [0, 0, 0] and len(idx) == len(o) == len(ind) == 0 and delta.tolist() == [0, 0]
    with pytest.raises(AssertionError):
        gr.carried_lists_np(codes, vl, va, r0, np.array([2**31 - 5, 7, 3, 0, 0], np.int32))


def test_seam_helpers():
    assert (gr.CHUNK, gr.THREADS, gr.SWEEP) == (16, 256, 4096)
    head = b"c\t1\t.\tA\tC\t.\tP\t.\tGT\t"
    sec = b"0|1\t" + b"1|0:" + b"x" * (4096 - 8 - 1) + b"\t12|3\t.|.\t"
    text = head + sec + b"\r\n"
    lo = len(head)
    assert gr.section_bounds(text, lo, len(text)) == (lo, lo + len(sec))
    f = gr.section_fields(text, lo, len(text))
    assert f[0] == "0|1" and f[2:] == ["12|3", ".|.", ""] and len(f[1]) == 4 + 4087
    assert gr.oracle_record(text, lo, len(text))[9:] == f
    rel, sweep, thread, phase = gr.field_seams(text, lo, len(text))
    assert rel.tolist() == [0, 4, 4096, 4101, 4105] and sweep.tolist() == [0, 0, 1, 1, 1]
    assert thread.tolist() == [0, 0, 0, 0, 0] and phase.tolist() == [0, 4, 0, 5, 9]
    assert rel[-1] == len(sec)  # the empty last field behind the trailing tab
    assert gr.n_sweeps(text, lo, len(text)) == 2 and gr.n_sweeps(text, lo, lo + 4096) == 1
    assert gr.section_fields(text, len(text), len(text)) == [] and len(gr.field_seams(text, len(text), len(text))[0]) == 0
    assert gr.section_fields(b"ab\n", 2, 3) == []  # only the terminator behind gt_off
    rel, sweep, thread, phase = gr.field_seams(b"\t" * 4 + b"0|1\t" * 1100, 4, 4404)
    assert thread[sweep == 0].max() == 255 and set(phase.tolist()) == {0, 4, 8, 12}
    assert gr.crosses(15, 2, 16) and not gr.crosses(14, 2, 16) and not gr.crosses(16, 2, 16) and gr.crosses(4094, 3, 4096)
    assert not gr.crosses(5, 0, 16)


def test_parse_reference_follows_the_wide_reference_fixture():
    """G12: the per-allele sample sets VariantRecord.read_vcf_line built from records of 2504 samples follow from the codes of
    oracle.vcf_genotype_codes - the parse reference is the reference's reading at panel width too."""
    from util import load_golden
    fx = load_golden("g12_vcf_wide.json.gz")
    names = np.array(fx["samples"])
    assert len(names) == 2504
    codes, flags = ora.vcf_genotype_codes([r["fields"] for r in fx["records"]], len(names))
    assert not flags.any()
    for i, rec in enumerate(fx["records"]):
        text = ("\t".join(rec["fields"]) + "\n").encode()
        lo = len(("\t".join(rec["fields"][:9]) + "\t").encode())
        assert gr.n_sweeps(text, lo, len(text)) >= 3 and gr.oracle_record(text, lo, len(text))[9:] == rec["fields"][9:]
        for k in range(len(rec["alt"])):
            for c in range(2):
                assert sorted(names[np.flatnonzero(codes[i, c::2] == k + 1)].tolist()) == rec["samples"][k][c]
    assert max(len(r["alt"]) for r in fx["records"]) == 12 and (codes == 255).any() and (codes >= 10).any()


def test_largest_lists_case_stays_cheap_on_the_host():
    """The product-sized case of the GPU module (about 31 000 variants x 600 columns): the reference must not dominate the test."""
    import time
    rng = np.random.default_rng(7200)
    codes = (rng.random((31000, 600)) < 0.02).astype(np.uint8)
    vl = np.arange(31000, dtype=np.uint32)
    va = np.ones(31000, np.uint8)
    t0 = time.perf_counter()
    off, idx, o, delta, ind = gr.carried_lists_np(codes, vl, va, vl.astype(np.int32), np.ones(31000, np.int32))
    dt = time.perf_counter() - t0
    assert int(off[-1]) == int(codes.sum()) == len(idx) == len(ind)
    assert np.array_equal(delta, codes.sum(axis=0))
    print(f"carried_lists_np 31000 x 600: {dt:.3f} s")
