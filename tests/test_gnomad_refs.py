"""tests/gnomad_refs.py (the per-line restatement every gnomAD converter test takes its expected values from) against the
reference's own converter output: tests/golden/g13_gnomad.json.gz, four files and two errors, byte for byte."""
import pytest

import gnomad_refs as refs
from util import load_golden

G13 = load_golden("g13_gnomad.json.gz")


def case_input(case):
    kind = G13["kinds"][case["kind"]]
    bad = set(kind["bad_dropped"]) if case["keep"] else set()
    lines = [ln for i, ln in enumerate(kind["lines"]) if i not in bad]
    return kind, "".join(ln + "\n" for ln in kind["header"] + lines)


@pytest.mark.parametrize("name", sorted(G13["cases"]))
def test_refs_reproduce_the_reference(name):
    case = G13["cases"][name]
    kind, text = case_input(case)
    assert refs.convert_text(text, kind["joint"], case["keep"]) == case["output"]
    assert refs.output_name("/data/" + kind["input_name"], case["suffix"], "out") == "out/" + case["output_name"]


def test_fixture_holds_the_cases_it_should():
    assert sorted(G13["cases"]) == ["joint_keep0", "joint_keep1", "plain_keep0", "plain_keep1"]
    for kind in G13["kinds"].values():
        assert 280 <= len(kind["lines"]) <= 320 and len(kind["bad_dropped"]) >= 8
        infos = [ln.split("\t")[7] for ln in kind["lines"]]
        k0 = refs.keys_of(kind["joint"])[0]
        for v in refs.GOOD_VALUES:
            assert any(f"{k0}={v};" in i or i.endswith(f"{k0}={v}") for i in infos), v
        assert {ln.split("\t")[6] for ln in kind["lines"]} >= set(refs.FILTERS)


@pytest.mark.parametrize("k", range(len(G13["errors"])))
def test_refs_reproduce_the_errors(k):
    err = G13["errors"][k]
    with pytest.raises(refs.RefError) as ei:
        refs.convert_text(err["input"], err["joint"], err["keep"])
    assert refs.RefError.cls == err["class"]
    # exception_handler puts two line feeds in front; the reference's error classes print repr(message)
    assert repr("\n\n" + str(ei.value)) == err["message"]
    assert ei.value.where == err["where"]
