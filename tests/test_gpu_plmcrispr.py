"""PLM-CRISPR on the device (csrc/hawk_plm.hip through hawk_plm_* and scoring.plmcrispr): against the reference network's own
scores for seeded parameters (g15), against the float64 restatement at the batch, tile and index seams, bit for bit against
itself wherever a guide's place in the call changes, and through the dispatcher and the file pipeline.

Tolerances are plm_refs.plm_tolerance: 4 x the distance of an fp32 evaluation (the reference's torch one for the fixture,
numpy's for everything else) from float64, floored at one fp32 ulp."""
import functools

import numpy as np
import pytest

from crisprhawk_hip import _lib, scoring, synth
from crisprhawk_hip.crisprhawk_error import CrisprHawkPlmCrisprScoreError
from crisprhawk_hip.pam import SPCAS9, XCAS9
from plm_refs import plm_f32, plm_f64, plm_tolerance, protein_f32, protein_f64
from util import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_model_left_behind():
    """tests/test_gpu_scoring_dispatch.py runs after this file and asserts that the PLM slot stays empty"""
    yield
    scoring.clear_plmcrispr_model()
    scoring.skip_scorers()


@functools.lru_cache(maxsize=None)
def g15():
    fx = load_golden("g15_plmcrispr.json.gz")
    params = synth.plmcrispr_weights(fx["seed"])
    protein = synth.plmcrispr_protein(fx["seed"], fx["L"])
    return fx, params, protein


@functools.lru_cache(maxsize=None)
def pool():
    """300 guides (N and mixed case among them) with their float64 and numpy-fp32 scores under g15's parameters: computed once"""
    fx, params, protein = g15()
    rng = np.random.default_rng(15)
    seqs = ["".join(r) for r in np.array(list("ACGTNacgtn"))[rng.choice(10, size=(300, 23), p=[.21, .21, .21, .21, .02, .03, .03, .03, .03, .02])]]
    f64, f32 = plm_f64(seqs, params, protein), plm_f32(seqs, params, protein)
    f64.setflags(write=False)
    f32.setflags(write=False)
    return seqs, f64, f32


def _set(params=None, protein=None, cas=SPCAS9):
    fx, p0, e0 = g15()
    scoring.set_plmcrispr_model(p0 if params is None else params, {cas: e0 if protein is None else protein})


def _score(seqs, batch=None, cas=SPCAS9):
    return np.array(scoring.plmcrispr(list(seqs), cas, True, batch), dtype=np.float32)


def _close(got, f32, f64, what):
    tol, err = plm_tolerance(f32, f64)
    d = float(np.max(np.abs(got.astype(np.float64) - f64)))
    print(f"{what}: device vs float64 {d:.3e}; fp32 reference vs float64 {err:.3e}; tolerance {tol:.3e}")
    assert d <= tol, what


def test_fixture_parity_with_the_reference_network():
    fx, params, protein = g15()
    _set()
    f64 = plm_f64(fx["guides"], params, protein)
    _close(_score(fx["guides"]), np.array(fx["scores"], dtype=np.float32), f64, "512 fixture guides")
    _close(scoring.plmcrispr_protein_vector(SPCAS9), np.array(fx["protein"], dtype=np.float32), protein_f64(params, protein), "out_protein")


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257])
def test_tile_seams(n):
    """the GEMM's M tile is 128 rows (four waves of 2 x 2 MFMA tiles of 32)"""
    seqs, f64, f32 = pool()
    _set()
    _close(_score(seqs[:n]), f32[:n], f64[:n], f"n = {n}")


@pytest.mark.parametrize("n,batch", [(200, 96), (3, 1), (257, 128), (130, 129)])
def test_batch_seams(n, batch):
    seqs, f64, f32 = pool()
    _set()
    _close(_score(seqs[:n], batch), f32[:n], f64[:n], f"n = {n}, batch = {batch}")


def test_position_independence_bit_for_bit():
    seqs, f64, f32 = pool()
    _set()
    whole = _score(seqs).view(np.uint32)
    one_by_one = np.concatenate([_score([s]) for s in seqs]).view(np.uint32)
    assert np.array_equal(one_by_one, whole)
    assert np.array_equal(_score(seqs[::-1])[::-1].view(np.uint32), whole)
    for batch in (64, 96, 0):
        assert np.array_equal(_score(seqs, batch).view(np.uint32), whole), batch
    assert np.array_equal(_score(seqs[100:250] + seqs[:7]).view(np.uint32), np.concatenate([whole[100:250], whole[:7]]))


PROBES = (0, 58, 59, 3775, 3776, 3834, 7551)  # channel, branch and end seams of the 7552-vector


def test_index_probes_of_the_feature_vector():
    """lin1's unit i reads feature PROBES[i] alone and lin3's output i reads that unit alone: a feature written to or read from
    a neighbouring slot changes out_sgrna[i]"""
    fx, p0, protein = g15()
    params = dict(p0)
    w1, w3 = np.zeros((2048, 7552), np.float32), np.zeros((256, 2048), np.float32)
    for i, j in enumerate(PROBES):
        w1[5 + 293 * i, j] = 4.0
        w3[i, 5 + 293 * i] = 3.0
    params["lin1.weight"], params["lin3.weight"] = w1, w3
    params["lin1.bias"] = np.zeros(2048, np.float32)
    seqs = pool()[0][:40]
    f64, f32 = plm_f64(seqs, params, protein), plm_f32(seqs, params, protein)
    assert f64.std() > 1e-3, "the probes move the score"
    _set(params)
    _close(_score(seqs), f32, f64, "index probes")
    # one probe at a time with nothing else feeding out_sgrna: the device sees exactly the feature the restatement sees
    for i, j in enumerate(PROBES):
        one = dict(params)
        w1 = np.zeros((2048, 7552), np.float32)
        w1[5 + 293 * i, j] = 4.0
        one["lin1.weight"] = w1
        f64, f32 = plm_f64(seqs[:8], one, protein), plm_f32(seqs[:8], one, protein)
        _set(one)
        _close(_score(seqs[:8]), f32, f64, f"probe {j}")


def test_scaffold_positions():
    """the last symbols of the guide and the first of the scaffold share convolution windows and, through the quirk, channels"""
    fx, params, protein = g15()
    rng = np.random.default_rng(16)
    base = ["".join(r) for r in np.array(list("ACGT"))[rng.integers(0, 4, size=(24, 22))]]
    sets = [[b + last for b in base] for last in "ACGTN"]
    flat = [s for st in sets for s in st] + ["N" * 23, "A" * 23, "G" * 23, "T" * 23, "C" * 23, "n" * 23, "a" * 23]
    f64, f32 = plm_f64(flat, params, protein), plm_f32(flat, params, protein)
    _set()
    got = _score(flat)
    _close(got, f32, f64, "last-base sets and homopolymers")
    assert np.max(np.abs(f64[:24] - f64[24:48])) > 1e-3, "the last base matters to the reference"
    assert np.array_equal(got[-2:].view(np.uint32), np.array([got[-7], got[-6]]).view(np.uint32)), "case does not matter"


@pytest.mark.parametrize("L", [13, 14, 29, 200])
def test_protein_lengths(L):
    """at L = 13 the kernel-13 convolution has exactly one position"""
    fx, params, _ = g15()
    protein = synth.plmcrispr_protein(99, L)
    _set(protein=protein, cas=XCAS9)
    _close(scoring.plmcrispr_protein_vector(XCAS9), protein_f32(params, protein), protein_f64(params, protein), f"out_protein, L = {L}")
    seqs = pool()[0][:5]
    _close(_score(seqs, cas=XCAS9), plm_f32(seqs, params, protein), plm_f64(seqs, params, protein), f"scores, L = {L}")


def test_protein_embedding_is_rounded_through_fp16_and_short_ones_are_refused():
    fx, params, _ = g15()
    raw = np.random.default_rng(5).standard_normal((21, 1280)).astype(np.float32)
    _set(protein=raw)
    a = scoring.plmcrispr_protein_vector(SPCAS9)
    _set(protein=raw.astype(np.float16).astype(np.float32))
    assert np.array_equal(a.view(np.uint32), scoring.plmcrispr_protein_vector(SPCAS9).view(np.uint32))
    _close(a, protein_f32(params, raw), protein_f64(params, raw), "unrounded embedding")
    with pytest.raises(ValueError):
        _set(protein=raw[:12])
    block = scoring.pack_plmcrispr_params(params)
    import ctypes as C
    h = C.c_void_p()
    rc = _lib.lib().hawk_plm_create(_lib.context(), block.ctypes.data_as(C.c_void_p), raw.ctypes.data_as(C.c_void_p), C.c_uint32(12), C.byref(h))
    assert rc == _lib.HAWK_E_INVALID and not h.value
    out = np.zeros(3, np.float32)
    assert _lib.lib().hawk_plm_score(scoring._PLM[SPCAS9], b"", C.c_uint32(23), C.c_uint64(0), C.c_uint32(0), None) == _lib.HAWK_OK
    assert _lib.lib().hawk_plm_score(scoring._PLM[SPCAS9], b"A" * 66, C.c_uint32(22), C.c_uint64(3), C.c_uint32(0),
                                     out.ctypes.data_as(C.c_void_p)) == _lib.HAWK_E_INVALID


def test_refusals_and_the_call_after_them():
    fx, params, protein = g15()
    seqs, f64, f32 = pool()
    with pytest.raises(CrisprHawkPlmCrisprScoreError):
        scoring.plmcrispr(seqs[:3], SPCAS9)  # no model loaded
    _set()
    want = _score(seqs[:130])
    for seq, _cls in fx["refused"]:
        with pytest.raises(CrisprHawkPlmCrisprScoreError):
            scoring.plmcrispr([seqs[0], seq, seqs[1]], SPCAS9)
        assert np.array_equal(_score(seqs[:2]).view(np.uint32), want[:2].view(np.uint32))
    with pytest.raises(CrisprHawkPlmCrisprScoreError):
        scoring.plmcrispr(seqs[:3], XCAS9)  # a model, but not for this Cas system
    # the device's own check (the host check stepped over): a bad character in the first, a middle and the last guide of 130
    import ctypes as C
    for where in (0, 64, 129):
        bad = list(seqs[:130])
        bad[where] = bad[where][:22] + "R"
        out = np.empty(130, np.float32)
        rc = _lib.lib().hawk_plm_score(scoring._PLM[SPCAS9], "".join(bad).encode(), C.c_uint32(23), C.c_uint64(130), C.c_uint32(64),
                                       out.ctypes.data_as(C.c_void_p))
        assert rc == _lib.HAWK_E_IUPAC, where
        with pytest.raises(CrisprHawkPlmCrisprScoreError):
            scoring.plmcrispr(bad, SPCAS9)
        assert np.array_equal(_score(seqs[:130]).view(np.uint32), want.view(np.uint32))


def test_dispatcher_scores_between_rs3_and_cfdon():
    from test_gpu_scoring_dispatch import SLOTS, _args, _filled, _guides_for
    assert SLOTS.index("rs3_score") < SLOTS.index("plmcrispr_score") < SLOTS.index("cfdon_score")
    g9 = load_golden("g9_azimuth.json.gz")
    scoring.set_azimuth_model({k: (np.array(v) if isinstance(v, list) else v) for k, v in g9["model"].items()})
    scoring.set_cfd_tables(*synth.cfd_tables())
    scoring.set_deepcpf1_weights(synth.deepcpf1_weights(2002))
    rs3_model = dict(tree_off=np.array([0, 3], np.int32), feature=np.array([0, -1, -1], np.int32), left=np.array([1, 0, 0], np.int32),
                     right=np.array([2, 0, 0], np.int32), threshold=np.array([0.5, 0, 0]), value=np.array([0.0, -1.0, 1.0]), init=0.0,
                     learning_rate=1.0, n_features=1)
    scoring.set_rs3_model(rs3_model, lambda kmers: np.array([[1.0 if k[0] in "AC" else 0.0] for k in kmers]))
    scoring.skip_scorers()
    _set()
    order = []
    real = {name: getattr(scoring, name) for name in ("azimuth_score", "rs3_score", "plmcrispr_score", "cfdon_score")}
    try:
        for name, fn in real.items():
            setattr(scoring, name, (lambda name, fn: lambda *a, **k: (order.append(name), fn(*a, **k))[1])(name, fn))
        fx, region, pam, guides = _guides_for("phased4")
        assert pam.cas_system == SPCAS9
        ids = {id(g): i for i, g in enumerate(guides)}
        want = scoring.plmcrispr([g.guidepam for g in guides], SPCAS9)
        scored = scoring.scoring_guides({region: guides}, pam, None, _args())[region]
    finally:
        for name, fn in real.items():
            setattr(scoring, name, fn)
    assert order == ["azimuth_score", "rs3_score", "plmcrispr_score", "cfdon_score"]  # scoring.py:774-781
    assert _filled(scored) == {"azimuth_score", "rs3_score", "plmcrispr_score", "cfdon_score"}
    assert [ids[id(g)] for g in scored] == fx["cfdon_order"]
    for g in scored:
        assert g.plmcrispr_score == str(round(want[ids[id(g)]], 4))
    # skipped by name: the slot stays NA
    scoring.skip_scorers("plmcrispr")
    fx, region, pam, guides = _guides_for("phased4")
    assert _filled(scoring.scoring_guides({region: guides}, pam, None, _args())[region]) == {"azimuth_score", "rs3_score", "cfdon_score"}
    scoring.skip_scorers()
    # Cpf1 and SaCas9 are untouched by a loaded model
    fx, region, pam, guides = _guides_for("cpf1")
    assert _filled(scoring.scoring_guides({region: guides}, pam, None, _args(guidelen=23, right=True))[region]) == {"deepcpf1_score"}
    fx, region, pam, guides = _guides_for("iupac")
    assert _filled(scoring.scoring_guides({region: guides}, pam, None, _args(guidelen=21))[region]) == set()
    # a model for the other Cas system only: SpCas9 guides keep NA, nothing raises
    _set(cas=XCAS9)
    fx, region, pam, guides = _guides_for("phased4")
    assert _filled(scoring.scoring_guides({region: guides}, pam, None, _args())[region]) == {"azimuth_score", "rs3_score", "cfdon_score"}


def test_load_models_reads_plmcrispr_npz(tmp_path):
    fx, params, protein = g15()
    np.savez(tmp_path / "plmcrispr_model.npz", protein_xcas9=protein, **params)
    have = scoring.load_models(str(tmp_path))
    assert have["plmcrispr"] and not have["azimuth"] and set(scoring._PLM) == {XCAS9}
    seqs, f64, f32 = pool()
    _close(_score(seqs[:9], cas=XCAS9), f32[:9], f64[:9], "through load_models")


def test_pipeline_fills_score_plmcrispr(tmp_path):
    import pandas as pd

    from crisprhawk_hip import pipeline
    from test_gpu_haptext import _write_inputs
    fx, params, protein = g15()
    g7 = load_golden("g7_report_phased4.json.gz")
    assert g7["guidelen"] + len(g7["pam"]) == 23 and not g7["right"]
    fa, bed, vcfs = _write_inputs(g7, tmp_path)
    cfd = synth.cfd_tables() if g7["cfd"] else None
    (plain,) = pipeline.search_files(fa, bed, vcfs, g7["pam"], g7["guidelen"], g7["right"], str(tmp_path / "plain"), cfd_tables=cfd).values()
    (with_plm,) = pipeline.search_files(fa, bed, vcfs, g7["pam"], g7["guidelen"], g7["right"], str(tmp_path / "plm"), cfd_tables=cfd,
                                        plmcrispr_model=(params, {SPCAS9: protein})).values()
    assert open(plain).read() == g7["report_tsv"]
    a = pd.read_csv(plain, sep="\t", dtype=str, keep_default_na=False)
    b = pd.read_csv(with_plm, sep="\t", dtype=str, keep_default_na=False)
    assert list(a.columns) == list(b.columns) and len(a) == len(b) > 0
    for c in a.columns:
        if c != "score_plmcrispr":
            assert a[c].tolist() == b[c].tolist(), c
    assert set(a["score_plmcrispr"]) == {"NA"}
    want = scoring.plmcrispr([s + p for s, p in zip(b["sgRNA_sequence"], b["pam"])], SPCAS9)
    assert b["score_plmcrispr"].tolist() == [str(round(x, 4)) for x in want]
    # plmcrispr_model=True: the model that is already set
    (again,) = pipeline.search_files(fa, bed, vcfs, g7["pam"], g7["guidelen"], g7["right"], str(tmp_path / "again"), cfd_tables=cfd,
                                     plmcrispr_model=True).values()
    assert open(again, "rb").read() == open(with_plm, "rb").read()
    with pytest.raises(CrisprHawkPlmCrisprScoreError):
        pipeline.search_files(fa, bed, vcfs, g7["pam"], 19, g7["right"], str(tmp_path / "short"), cfd_tables=cfd,
                              plmcrispr_model=(params, {SPCAS9: protein}))
    assert not (tmp_path / "short").exists(), "refused before any search"
