"""Host side of the off-target summary: the rounding rule the device applies to a site's CFD restated on the host and held to
Python's round(x, 4), and the pipeline's refusal of a summary with bulges."""
import math
from fractions import Fraction

import numpy as np
import pytest

from crisprhawk_hip import synth


def round_e4(x: float) -> int:
    """ot_round_e4 of csrc/hawk_offtarget.hip: k = floor(fl(x * 1e4)); the sign of the exact x * 1e4 - (k + 0.5) picks k + 1 or k,
    zero is a true tie and goes to even.  The device takes the sign from one fma; here the residual is exact through Fraction."""
    k = math.floor(x * 1e4)
    r = Fraction(x) * 10000 - (Fraction(k) + Fraction(1, 2))
    if r > 0:
        return k + 1
    if r < 0:
        return k
    return k + (k & 1)


def python_e4(x: float) -> int:
    return int(round(round(x, 4) * 1e4))


def test_rounding_rule_equals_python_round_on_table_products():
    mm, pt = synth.cfd_tables()
    rng = np.random.default_rng(4)
    flat = mm.reshape(-1)
    for n_mm in rng.integers(0, 6, size=100_000).tolist():
        x = 1.0
        for v in flat[rng.integers(0, flat.size, size=n_mm)].tolist():
            x *= v
        x *= float(pt[rng.integers(0, 16)])
        assert round_e4(x) == python_e4(x), x


@pytest.mark.parametrize("tie,units", [(0.03125, 312), (0.09375, 938), (0.15625, 1562), (0.21875, 2188), (0.00005, 1), (0.5, 5000), (1.0, 10000), (0.0, 0)])
def test_rounding_rule_on_exact_ties_and_their_neighbours(tie, units):
    assert round_e4(tie) == python_e4(tie) == units
    for x in (float(np.nextafter(tie, 2.0)), float(np.nextafter(tie, -1.0))):
        if x >= 0.0:
            assert round_e4(x) == python_e4(x), x
    if tie in (0.03125, 0.09375, 0.15625, 0.21875):  # k + 0.5 exactly: one ulp decides
        assert round_e4(float(np.nextafter(tie, 2.0))) == math.floor(tie * 1e4) + 1
        assert round_e4(float(np.nextafter(tie, -1.0))) == math.floor(tie * 1e4)


def test_rint_alone_is_not_the_rule():
    """Why the residual is taken exactly: fl(x * 1e4) can land on k + 0.5 when x * 1e4 does not."""
    found = 0
    for k in range(1, 2000):
        for x in (float(np.nextafter((k + 0.5) / 1e4, 2.0)), (k + 0.5) / 1e4, float(np.nextafter((k + 0.5) / 1e4, -1.0))):
            assert round_e4(x) == python_e4(x), x
            found += int(np.rint(x * 1e4)) != python_e4(x)
    print("values near k + 0.5 where rint(x * 1e4) alone differs from round(x, 4):", found)


def test_summary_route_refuses_bulges(tmp_path):
    from crisprhawk_hip import pipeline
    for kw in (dict(brna=1), dict(bdna=2)):
        with pytest.raises(ValueError, match="mismatch-only"):
            pipeline.search_files(str(tmp_path / "g.fa"), str(tmp_path / "r.bed"), [], "NGG", 20, False, str(tmp_path), estimate_offtargets={"c": "ACGT" * 20},
                                  offtargets_table=False, **kw)


def test_summary_symbol_is_declared_and_bound():
    from crisprhawk_hip import _lib
    import os
    assert "hawk_offtarget_summary" in _lib.EXPORTS
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hawk.h")).read()
    assert "int hawk_offtarget_summary(" in header
