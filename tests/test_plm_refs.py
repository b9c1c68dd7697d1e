"""G15 without a device: the numpy statements of PLM-CRISPR (tests/plm_refs.py) against what the reference's own sgrna_net
gave for the seeded parameters (tests/golden/g15_plmcrispr.json.gz, made by tests/golden/make_golden_plmcrispr.py), the
binding's host-side refusals, and the checkpoint converter on a synthetic full-object checkpoint."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from crisprhawk_hip import scoring, synth
from crisprhawk_hip.crisprhawk_error import CrisprHawkPlmCrisprScoreError, CrisprHawkScoreError
from plm_refs import plm_f32, plm_f64, plm_tolerance, protein_f32, protein_f64
from util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def g15():
    """the fixture, its parameters rebuilt from the seed, and the float64 restatement: computed once, never modified"""
    fx = load_golden("g15_plmcrispr.json.gz")
    params = synth.plmcrispr_weights(fx["seed"])
    protein = synth.plmcrispr_protein(fx["seed"], fx["L"])
    f64 = plm_f64(fx["guides"], params, protein)
    f64.setflags(write=False)
    return fx, params, protein, f64


def test_fixture_meets_its_condition():
    fx = load_golden("g15_plmcrispr.json.gz")
    s = np.array(fx["scores"])
    assert len(fx["guides"]) == 512 and all(len(g) == 23 for g in fx["guides"])
    assert s.std() >= 0.05 and s.min() > 0.02 and s.max() < 0.98
    assert sum("N" in g.upper() for g in fx["guides"]) >= 25 and sum(g != g.upper() for g in fx["guides"]) >= 25
    assert {len(r[0]) for r in fx["refused"]} >= {22, 24} and {"R", "U", "-"} <= set("".join(r[0] for r in fx["refused"]))
    assert len(fx["refused"]) >= 12


def test_f64_restatement_against_the_reference_network():
    """Any structural mistake - the reshape quirk, the concat order, the flatten order - moves scores by more than 1e-3 at this
    spread; the reference's own fp32 noise is some 5e-7."""
    fx, params, protein, f64 = g15()
    d_score = float(np.max(np.abs(f64 - np.array(fx["scores"]))))
    d_prot = float(np.max(np.abs(protein_f64(params, protein) - np.array(fx["protein"]))))
    print(f"plm_f64 vs the reference's fp32 scores: {d_score:.3e}; protein vector: {d_prot:.3e}")
    assert d_score <= 1e-5 and d_prot <= 1e-5


def test_a_transpose_instead_of_the_view_is_seen():
    """the one-hot transposed - what the comment at train_general.py:75 claims - is not what .view(-1, 5, 59) gives, and the
    first convolution already differs far beyond 1e-5"""
    import plm_refs
    fx, params, protein, f64 = g15()
    codes = plm_refs.encode(fx["guides"][:32])
    onehot = np.zeros((32, 59, 5))
    onehot[np.arange(32)[:, None], np.arange(59)[None, :], codes] = 1
    w, b = params["conv4.weight"].astype(np.float64), params["conv4.bias"].astype(np.float64)
    viewed = plm_refs._conv_same(onehot.reshape(32, 5, 59), w, b)
    transposed = plm_refs._conv_same(np.ascontiguousarray(onehot.transpose(0, 2, 1)), w, b)
    assert np.max(np.abs(viewed - transposed)) > 1e-2


def test_f32_restatement_distance():
    fx, params, protein, f64 = g15()
    f32 = plm_f32(fx["guides"], params, protein)
    tol, err = plm_tolerance(f32, f64)
    tol_fx, err_fx = plm_tolerance(fx["scores"], f64)
    p_err = float(np.max(np.abs(protein_f32(params, protein).astype(np.float64) - protein_f64(params, protein))))
    print(f"plm_f32 vs plm_f64: {err:.3e} (tolerance {tol:.3e}); fixture vs plm_f64: {err_fx:.3e} (tolerance {tol_fx:.3e}); "
          f"protein f32 vs f64: {p_err:.3e}")
    assert f32.dtype == np.float32 and err < 1e-5 and tol >= np.spacing(np.float32(f64.max()))


def test_refused_inputs_raise_on_the_host(monkeypatch):
    """the reference's ValueError / KeyError (plm_crispr.py:152-158, 199) reach the caller as CrisprHawkPlmCrisprScoreError
    (scoring.py:550-559) from the binding's own checks: no library call, no device"""
    fx = load_golden("g15_plmcrispr.json.gz")
    assert issubclass(CrisprHawkPlmCrisprScoreError, CrisprHawkScoreError)
    for seq, cls in fx["refused"]:
        with pytest.raises({"ValueError": ValueError, "KeyError": KeyError}[cls]):
            scoring._plmcrispr_check_inputs(["ACGTACGTACGTACGTACGTAGG", seq])
    scoring._plmcrispr_check_inputs(fx["guides"])  # N and lower case are legal
    monkeypatch.setattr(scoring, "_PLM", {3: None})
    monkeypatch.setattr(scoring._lib, "lib", lambda: pytest.fail("the library is not reached"))
    for seq, _ in fx["refused"]:
        with pytest.raises(CrisprHawkPlmCrisprScoreError):
            scoring.plmcrispr(["ACGTACGTACGTACGTACGTAGG", seq], 3)
    with pytest.raises(CrisprHawkPlmCrisprScoreError):
        scoring.plmcrispr(["ACGTACGTACGTACGTACGTAGG"], 4)  # no model for xCas9
    assert scoring.plmcrispr([], 3) == []
    assert scoring.plmcrispr_score([], 3, 1, 0, True) == [] and scoring._plmcrispr_score is scoring.plmcrispr_score


def test_pack_checks_names_and_shapes():
    params = synth.plmcrispr_weights(7)
    block = scoring.pack_plmcrispr_params(params)
    assert block.dtype == np.float32 and block.size == sum(int(np.prod(s)) for _, s in synth.PLMCRISPR_SHAPES) == 20659075
    assert np.array_equal(block[:1600], params["conv1.weight"].reshape(-1)) and np.array_equal(block[-2:], params["weight_net.2.bias"])
    bad = dict(params)
    bad["lin3.weight"] = bad["lin3.weight"].T
    with pytest.raises(ValueError):
        scoring.pack_plmcrispr_params(bad)
    del bad["lin3.weight"]
    with pytest.raises(ValueError):
        scoring.pack_plmcrispr_params(bad)
    assert "plmcrispr" not in scoring.OUT_OF_SCOPE_SCORERS
    with pytest.raises(ValueError):
        scoring.skip_scorers("plm")
    scoring.skip_scorers("plmcrispr")
    scoring.skip_scorers()


def test_convert_models_round_trips_a_full_object_checkpoint(tmp_path):
    import sys

    import torch
    spec = importlib.util.spec_from_file_location("convert_models", os.path.join(ROOT, "tools", "convert_models.py"))
    cm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cm)
    params = synth.plmcrispr_weights(11)
    with cm._PlmModules() as mods:
        net = mods["train_general"].sgrna_net()
        assert list(net.state_dict()) == [k for k, _ in synth.PLMCRISPR_SHAPES]
        net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        torch.save(net, tmp_path / "100.pt")  # the full object, as the published checkpoint was saved
    assert "train_general" not in sys.modules and "Protein" not in sys.modules
    emb = synth.plmcrispr_protein(11, 17)
    torch.save({"label": "SpCas9", "representations": torch.from_numpy(emb)}, tmp_path / "SpCas9.esm.pt")
    cm.convert_plmcrispr(str(tmp_path / "100.pt"), {"protein_spcas9": str(tmp_path / "SpCas9.esm.pt")}, str(tmp_path / "plmcrispr_model.npz"))
    z = np.load(tmp_path / "plmcrispr_model.npz")
    assert set(z.files) == {k for k, _ in synth.PLMCRISPR_SHAPES} | {"protein_spcas9"}
    for k, v in params.items():
        assert z[k].dtype == np.float32 and np.array_equal(z[k], v)
    assert np.array_equal(z["protein_spcas9"], emb)
    assert "train_general" not in sys.modules and "Protein" not in sys.modules
