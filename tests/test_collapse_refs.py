"""tests/collapse_refs.py without a GPU: the reference grouping against oracle.collapse_rows on the reference-generated search
fixtures, the per-strand orientation of the flanks against what the model scorers read, the key-width arithmetic at its steps,
and every case builder - each proves from the oracle's search of its own set that it sits on the seam it is named after."""
import numpy as np
import pytest

import collapse_refs as cr
from oracle import oracle as ora
from util import G3_CASES, hapset_from_golden, load_golden


@pytest.mark.parametrize("case", G3_CASES)
def test_reference_equals_oracle_grouping_without_flanks(case):
    fx = load_golden(f"g3_search_{case}.json.gz")
    hs = hapset_from_golden(fx)
    pam, guidelen, right = fx["pam"], fx["guidelen"], fx["right"]
    res = ora.search(hs, pam, guidelen, right)
    g = res.guides
    assert len(g) > 0
    isref_row = np.asarray(hs.is_ref)[g["hap"]]
    want, want_gc = ora.collapse_rows(g["start"], g["stop"], g["strand"], isref_row, res.windows, guidelen, len(pam), right)
    got, got_gc = cr.group_rows(g["start"], g["stop"], g["strand"], isref_row, res.windows, guidelen, len(pam), right, (0, 0))
    assert got == want and got_gc == want_gc and list(got) == list(want)
    # a flank never merges what the plain key keeps apart, and every flank-aware group agrees on the scorers' k-mer
    wide, _ = cr.group_rows(g["start"], g["stop"], g["strand"], isref_row, res.windows, guidelen, len(pam), right, (4, 3))
    assert len(wide) >= len(got)
    for key, rows in wide.items():
        assert any(set(rows) <= set(v) for v in want.values())


def test_flank_orientation_is_the_scorers_kmer():
    """The model scorers read sequence[10 - 4 : -10 + 3] of the guide AFTER strand-1 guides were reverse-complemented
    (scoring.py:50-67 behind annotation.py:27-51).  On the stored + strand window that is w[10 - 3 : len - 10 + 4] for strand 1:
    the slice the reference grouping and the header of hawk_collapse.hip both name."""
    rng = np.random.default_rng(5)
    for L in (4, 23, 44):
        w = "".join(rng.choice(list("ACGTacgtRrNn"), size=L + 20))
        for up, down in cr.FLANKS + ((1, 0), (0, 1)):
            n = len(w)
            assert cr.key_slice(w, 0, up, down) == w[10 - up:n - 10 + down]
            rc = cr.revcomp(w)
            assert cr.revcomp(cr.key_slice(w, 1, up, down)) == rc[10 - up:n - 10 + down]
            assert len(cr.key_slice(w, 1, up, down)) == L + up + down
    # the scorers' literal slice (scoring.py:65: sequence[GUIDESEQPAD - 4 : -GUIDESEQPAD + 3]) on the reverse-complemented window
    w = "".join(rng.choice(list("ACGTacgt"), size=43))
    assert ora.revcomp(w)[10 - 4:-10 + 3] == ora.revcomp(cr.key_slice(w, 1, 4, 3)) and w[10 - 4:-10 + 3] == cr.key_slice(w, 0, 4, 3)
    assert cr.revcomp("ACGTN") == ora.revcomp("ACGTN") and cr.revcomp("acgR") == "Ycgt"


def test_reference_arrays_orders_groups_and_names_faults():
    groups = {(5, 9, 0, False, "AC"): [2, 4], (5, 9, 0, False, "AG"): [0], (3, 7, 1, True, "TT"): [1, 3]}
    gc = {k: (1, 2) for k in groups}
    perm, off = [1, 3, 0, 2, 4], [0, 2, 3, 5]
    p, o, a, b = cr.reference_arrays(groups, gc, perm, off)
    assert p.tolist() == perm and o.tolist() == off and a.tolist() == [1, 1, 1] and b.tolist() == [2, 2, 2]
    p, o, _, _ = cr.reference_arrays(groups, gc, [1, 3, 2, 4, 0], [0, 2, 4, 5])  # the other hash order inside start 5
    assert p.tolist() == [1, 3, 2, 4, 0]
    for bad_perm, bad_off in (([0, 1, 3, 2, 4], [0, 1, 3, 5]),    # start order
                              ([1, 3, 4, 2, 0], [0, 2, 4, 5]),    # a group opened by its second member
                              ([1, 3, 0, 2, 4], [0, 2, 3, 4, 5])):  # over-split
        with pytest.raises(AssertionError):
            cr.reference_arrays(groups, gc, bad_perm, bad_off)
    # members out of table order, or in the wrong group, show in the array comparison
    p, _, _, _ = cr.reference_arrays(groups, gc, [1, 3, 0, 2, 4], [0, 2, 3, 5])
    assert not np.array_equal(p, [3, 1, 0, 2, 4])


def test_key_bits_at_every_step():
    for span, want in cr.SPAN_BITS.items():
        kb = cr.key_bits(span)
        assert (kb["end_bit"], kb["begin_bit"], kb["passes"]) == want, hex(span)
        assert 24 <= kb["hash_bits"] <= 31 and (kb["end_bit"] - kb["begin_bit"]) % 8 == 0 or kb["hash_bits"] == 31
    assert not cr.key_bits(0x100000000)["accepted"]
    assert cr.key_bits(0xfffffffe)["hash_table"] and not cr.key_bits(0xffffffff)["hash_table"]
    # every step of end_bit, begin_bit or the pass count between 1 and 2^32 lies at a power of two
    prev = cr.key_bits(1)
    for k in range(1, 32):
        below, at = cr.key_bits((1 << k) - 1), cr.key_bits(1 << k)
        assert below == cr.key_bits((1 << (k - 1))) or k == 1
        assert at["end_bit"] == below["end_bit"] + 1
        prev = at
    assert prev["end_bit"] == 64


@pytest.mark.parametrize("i", range(len(cr.CASES_A)))
def test_builders_key_fields(i):
    c = cr.CASES_A[i]()
    assert c.proofs and len(c.rows()[0]) > 0


def test_builders_flanks():
    cases = cr.flank_cases()
    assert len(cases) == 8
    for c in cases:
        assert len(c.proofs) >= 4 * (2 + len(cr.FLANKS))
    assert sum(1 for c in cases if c.L == cr.MAX_CORE) == 4


@pytest.mark.parametrize("span", cr.SPANS + [0x100000000])
def test_builders_key_width(span):
    c = cr.case_span(span)
    assert c.span() == span and c.proofs


def test_builder_many_distinct_rows():
    c = cr.case_many_distinct()
    assert c.expected_pairs >= 1.0
    groups, _ = c.reference()
    assert len(groups) == len(c.rows()[0])  # every row its own group: nothing to merge, nothing to refuse


def test_builder_table_memory():
    few, every = cr.case_table_memory()
    assert few.seqs == every.seqs and few.scan != every.scan
