"""PLM-CRISPR on the device, layer by layer: the parameter sets of tests/plm_lens.py make the score a well-conditioned function
of out_sgrna (head lens), of every lin1 output (route lens), of one stretch of lin1's K (K-slice lenses) or of every feature
(feature lens), and out_protein one of every pooled text_cnn maximum (protein lens).  tests/test_plm_lens.py holds each set
to its condition: a 2^-10 error in one observed element moves that row's float64 score by more than twice the tolerance used
here.  So a wrong row at a tile seam, a dropped flush or a wrong last position, which the dense g15 parameters hide behind a
softmax weight of 6e-4, a relu and a max-pool, leaves the tolerance.

Every row is held to the call's plm_refs.plm_tolerance: 4 x the largest distance of numpy's fp32 evaluation from float64 over
the call's rows, floored at one fp32 ulp."""
import functools

import numpy as np
import pytest

import plm_lens
from crisprhawk_hip import scoring
from crisprhawk_hip.pam import SPCAS9, XCAS9
from plm_refs import plm_f32, plm_f64, plm_tolerance, protein_f32, protein_f64
from test_gpu_plmcrispr import _no_model_left_behind  # noqa: F401  (autouse: no model is left in the PLM slot)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _small_lens(name):
    """head and route share g15's lin1: their parameters are kept"""
    return plm_lens.lens(name)


def _use(name):
    """load the lens on the device; (guides, float64, fp32) of its rows, computed once per lens"""
    params = _small_lens(name) if name in ("head", "route") else plm_lens.lens(name)
    ref = plm_lens.reference(name, params)
    scoring.set_plmcrispr_model(params, {SPCAS9: plm_lens.g15()[1]})
    return ref


def _score(seqs, batch=None, cas=SPCAS9):
    return np.array(scoring.plmcrispr(list(seqs), cas, True, batch), dtype=np.float32)


def _rows_close(got, f32, f64, what):
    """every row within the call's tolerance; the worst row and its ratio to the tolerance are printed"""
    tol, err = plm_tolerance(f32, f64)
    d = np.abs(np.asarray(got, dtype=np.float64) - f64)
    worst = int(np.argmax(d))
    print(f"{what}: worst row {worst} of {len(d)}: device vs float64 {d[worst]:.3e} = {d[worst] / tol:.2f} x tolerance {tol:.3e}; "
          f"fp32 reference vs float64 {err:.3e}")
    bad = np.flatnonzero(~(d <= tol))
    assert len(bad) == 0, f"{what}: rows {bad[:8].tolist()} of {len(d)} leave the tolerance, first by {d[bad[0]] / tol:.1f} x"


@pytest.mark.parametrize("name", ["head", "route"])
def test_tile_seams_row_by_row(name):
    """the GEMM's M tile is 128 rows, a wave's 64, an MFMA tile 32; under these lenses row n - 1 answers for its own lin1 and
    lin3 outputs (under g15 its response to a 10^-3 error in a lin1 unit is below the tolerance at 13 of these 14 n)"""
    seqs, f64, f32 = _use(name)
    for n in (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257):
        _rows_close(_score(seqs[:n]), f32[:n], f64[:n], f"{name} lens, n = {n}")


@pytest.mark.parametrize("name", ["head", "route"])
def test_batch_seams_row_by_row(name):
    seqs, f64, f32 = _use(name)
    for n, batch in ((200, 96), (257, 128), (130, 129), (3, 1)):
        _rows_close(_score(seqs[:n], batch), f32[:n], f64[:n], f"{name} lens, n = {n}, batch = {batch}")


@pytest.mark.parametrize("which", list(plm_lens.K_SLICES))
def test_flush_and_stage_seams(which):
    """lin1 sees one stretch of K alone - the first, the second and the last flush period (PLM_TK x PLM_FLUSH = 128), the one
    that holds the branch seam 3776, the last 32-wide stage - and every one of its 2048 outputs reaches the score: a dropped
    or doubled flush, a stage fetched from the wrong place and a last stage left out change h1 by far more than 2^-10"""
    seqs, f64, f32 = _use(f"k:{which}")
    _rows_close(_score(seqs), f32, f64, f"K-slice {which}, {plm_lens.K_SLICES[which][:2]}")


@pytest.mark.parametrize("part", range(len(plm_lens.FEATURE_SETS)))
def test_feature_seams(part):
    """every feature of the set reaches the score through a unit of its own: the padding at positions 0, 1, 57 and 58, the
    thread-group seams 14/15, 29/30 and 44/45, the 14-position last group, the .view(-1, 5, 59) quirk and the conv4 branch,
    which is written from xb before conv2 overwrites it.  The guides hold N at positions 0 and 22, lower case, the homopolymers
    and the 24 x 5 last-base sets."""
    seqs, f64, f32 = _use(f"feature:{part}")
    lo, hi = plm_lens.FEATURE_SETS[part][:2]
    _rows_close(_score(seqs), f32, f64, f"features {lo}..{hi - 1}")


@pytest.mark.parametrize("n", [8191, 8192, 8193])
def test_default_batch_seam(n):
    """batch 0 is PLM_DEFAULT_BATCH = 8192 guides: the GEMM's grid has 64 row tiles, the last of them one row short at n = 8191,
    and n = 8193 takes the batch loop's second iteration with one guide.  Every row is held to its pool reference under the head lens, and
    the call is bit-identical to the same call in batches of 128.  HAWK_PLM_MAX_BATCH (65536 guides, a 2.6 GB workspace) is
    not exercised."""
    seqs, f64, f32 = _use("head")
    idx = np.arange(n) % len(seqs)
    many = [seqs[i] for i in idx]
    got = _score(many, 0)
    _rows_close(got, f32[idx], f64[idx], f"head lens, n = {n}, default batch")
    assert np.array_equal(got.view(np.uint32), _score(many, 128).view(np.uint32))
    assert np.array_equal(got[:len(seqs)].view(np.uint32), got[len(seqs):2 * len(seqs)].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------ protein branch
def _protein_vector(params, emb, cas=XCAS9):
    scoring.set_plmcrispr_model(params, {cas: emb})
    return scoring.plmcrispr_protein_vector(cas)


@pytest.mark.parametrize("L", [13, 20, 21, 24, 25, 28, 29, 36, 37, 200])
def test_protein_pool_seams(L):
    """P = L - ks + 1 positions in tiles of PLM_PROT_P = 16: over the three kernel sizes these lengths give P = 1, 16, 17, 32,
    33 and their neighbours, and at L = 28 and L = 200 the last tile of the kernel-13 launch starts at or past P and returns
    early.  The argmax of every live channel is forced to position 0, 15, 16 and P - 1 in turn (tests/test_plm_lens.py), six
    channels of each convolution are negative everywhere and pool to +0, and no lin4 unit is relu'd: every unit of out_protein
    is held to its tolerance."""
    params0 = plm_lens.g15()[0]
    for conv in range(3):
        for pos in plm_lens.forced_positions(L, conv):
            params, emb = plm_lens.protein_lens(15, params0, L, conv, pos)
            got = _protein_vector(params, emb)
            _rows_close(got, protein_f32(params, emb), protein_f64(params, emb),
                        f"out_protein, L = {L}, kernel {plm_lens.KERNELS[conv]} forced to position {pos}")


def test_scratch_reuse_between_models():
    """the atomic-max scratch comes from the caching allocator: a model with large pooled maxima, then one with small ones,
    then the first again"""
    params0 = plm_lens.g15()[0]
    params, big = plm_lens.protein_lens(15, params0, 37, 0, 16, amplitude=1.0)
    small = (plm_lens.protein_lens(16, params0, 37, 0, 16, amplitude=0.0, noise=0.01)[1])
    first = _protein_vector(params, big)
    _rows_close(first, protein_f32(params, big), protein_f64(params, big), "large maxima")
    second = _protein_vector(params, small)
    _rows_close(second, protein_f32(params, small), protein_f64(params, small), "small maxima after large ones")
    assert np.max(np.abs(first - second)) > 1e-2, "the two models differ"
    third = _protein_vector(params, big)
    assert np.array_equal(third.view(np.uint32), first.view(np.uint32))
    scoring.clear_plmcrispr_model()
    assert np.array_equal(_protein_vector(params, small).view(np.uint32), second.view(np.uint32))


def test_two_handles_alive():
    """SPCAS9 and XCAS9 with different embeddings, scored alternately: each handle's scores and out_protein are bit-identical
    to those it gives alone.  Under g15 the score leans on out_protein, so a handle that read the other's vector is seen."""
    params, e3 = plm_lens.g15()
    from crisprhawk_hip import synth
    e4 = synth.plmcrispr_protein(98, 21)
    seqs = plm_lens.pool_guides()[:70]
    alone = {}
    for cas, emb in ((SPCAS9, e3), (XCAS9, e4)):
        scoring.set_plmcrispr_model(params, {cas: emb})
        alone[cas] = (_score(seqs, cas=cas), scoring.plmcrispr_protein_vector(cas))
    assert np.max(np.abs(alone[SPCAS9][0] - alone[XCAS9][0])) > 1e-3
    _rows_close(alone[XCAS9][0], plm_f32(seqs, params, e4), plm_f64(seqs, params, e4), "XCAS9 alone")
    scoring.set_plmcrispr_model(params, {SPCAS9: e3, XCAS9: e4})
    for turn in range(2):
        for cas in (SPCAS9, XCAS9):
            assert np.array_equal(_score(seqs, 32 if turn else None, cas=cas).view(np.uint32), alone[cas][0].view(np.uint32)), (turn, cas)
            assert np.array_equal(scoring.plmcrispr_protein_vector(cas).view(np.uint32), alone[cas][1].view(np.uint32)), (turn, cas)
