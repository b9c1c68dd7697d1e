"""The scorer kernels (k_deepcpf1, k_azimuth, k_tm_nn, k_gbt, k_cfd) at batch seams, split edges and exact weights, against the
plain references of tests/scorer_refs.py (checked on the CPU by tests/test_scorer_refs.py) and the reference-made rows of
g5_cfd_edges.  NaN features are out of scope: the tree flatteners document that missing values are not modelled."""
import ctypes as C

import numpy as np
import pytest

import scorer_refs as R
from crisprhawk_hip import _lib, scoring, synth
from crisprhawk_hip.crisprhawk_error import CrisprHawkAzimuthScoreError, CrisprHawkCfdScoreError, CrisprHawkDeepCpf1ScoreError
from oracle import oracle as ora

pytestmark = pytest.mark.gpu

_vp = lambda a: a.ctypes.data_as(C.c_void_p)
_bits = lambda x: np.asarray(x, dtype=np.float32).view(np.uint32)


def _dc(seqs, w=None):
    if w is not None:
        scoring.set_deepcpf1_weights(w)
    return np.asarray(scoring.deepcpf1(list(seqs)), dtype=np.float32)


def _gm(model):
    arrs = {k: np.ascontiguousarray(model[k], dtype=(np.float64 if k in ("threshold", "value") else np.int32))
            for k in ("tree_off", "feature", "left", "right", "threshold", "value")}
    gm = _lib.GbtModel(len(arrs["tree_off"]) - 1, len(arrs["feature"]), *[arrs[k].ctypes.data for k in
                       ("tree_off", "feature", "left", "right", "threshold", "value")], float(model["init"]), float(model["learning_rate"]))
    return gm, arrs


def _raw_azimuth(seqs, model, out):
    gm, keep = _gm(model)
    return _lib.lib().hawk_azimuth(_lib.context(), "".join(seqs).encode("ascii"), C.c_uint64(len(seqs)), C.byref(gm), _vp(out), None)


def _raw_gbt(x, model, cast, out):
    gm, keep = _gm(model)
    x = np.ascontiguousarray(x, dtype=np.float64)
    return _lib.lib().hawk_gbt_predict(_lib.context(), _vp(x), C.c_uint64(x.shape[0]), x.shape[1], C.byref(gm), int(cast), _vp(out))


def _azimuth(seqs, model, feats=False):
    scoring.set_azimuth_model(model)
    if feats:
        got, f = scoring.azimuth(seqs, return_features=True)
        return np.asarray(got), f
    return np.asarray(scoring.azimuth(seqs))


# ---------------------------------------------------------------------------------------------- k_deepcpf1
DC_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 64 * 1000 + 1, 2 ** 20 + 37)


def test_deepcpf1_batch_sizes_exact():
    """every size next to the 64-guide workgroup, one, and two large grids; exact weights, so each score equals float64"""
    rng = np.random.default_rng(101)
    pool = R.random_kmers(rng, 293, 34)
    w = R.deepcpf1_exact_weights("dense", 0)
    want = R.deepcpf1_f64(pool, w).astype(np.float32)
    scoring.set_deepcpf1_weights(w)
    for n in DC_SIZES:
        idx = (np.arange(n, dtype=np.int64) * 7 + 3) % len(pool)
        got = _dc([pool[i] for i in idx])
        assert got.shape == (n,) and np.array_equal(_bits(got), _bits(want[idx])), n


def test_deepcpf1_position_independence_bit_for_bit():
    rng = np.random.default_rng(102)
    for name, sigma in R.DC_SCALES:
        scoring.set_deepcpf1_weights(R.deepcpf1_scaled_weights(sigma))
        one = R.random_kmers(rng, 1, 34)[0]
        got = _dc([one] * (3 * 64 + 17))
        assert len(np.unique(_bits(got))) == 1, name
        seqs = R.random_kmers(rng, 3 * 64 + 17, 34)
        base = _dc(seqs)
        perm = rng.permutation(len(seqs))
        assert np.array_equal(_bits(_dc([seqs[i] for i in perm])), _bits(base[perm])), name
        # a guide's neighbours and block do not matter: alone, it scores the same
        for i in (0, 63, 64, 200, len(seqs) - 1):
            assert _bits(_dc([seqs[i]]))[0] == _bits(base)[i], (name, i)


@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_deepcpf1_exact_weights_equal_float64(kind):
    rng = np.random.default_rng(103)
    seqs = R.random_kmers(rng, 5 * 64 + 9, 34) + [b * 34 for b in "ACGT"]
    for seed in (0, 1):
        w = R.deepcpf1_exact_weights(kind, seed)
        want = R.deepcpf1_f64(seqs, w)
        got = _dc(seqs, w)
        assert np.array_equal(got.astype(np.float64), want), (kind, seed, np.flatnonzero(got != want)[:5])


def test_deepcpf1_probe_family():
    """every time step, every wavefront's channel quarter and every tap decides a score alone, once"""
    rng = np.random.default_rng(104)
    seqs = R.random_kmers(rng, 64 + 37, 34)
    for t, c, k, base, o, o2, o3 in R.deepcpf1_probe_sweep():
        w = R.deepcpf1_probe(t, c, k, base, o, o2, o3)
        want = R.deepcpf1_probe_closed_form(seqs, t, k, base)
        got = _dc(seqs, w)
        assert np.array_equal(got.astype(np.float64), want), (t, c, k, base, o, o2, o3)


def test_deepcpf1_random_weights_at_three_scales():
    """tolerance per weight set from the references alone: 4 x the fp32 oracle's distance to float64 (a second legitimate fp32
    order: fused multiply-adds, accumulators split over wavefronts), floored at one fp32 ulp of the largest score"""
    rng = np.random.default_rng(105)
    seqs = R.random_kmers(rng, 1000, 34)
    for name, sigma in R.DC_SCALES:
        w = R.deepcpf1_scaled_weights(sigma)
        f64 = R.deepcpf1_f64(seqs, w)
        tol, ref_err = R.deepcpf1_tolerance(ora.deepcpf1(seqs, w), f64)
        got = _dc(seqs, w).astype(np.float64)
        err = float(np.max(np.abs(got - f64)))
        print(f"deepcpf1 {name}: max|f64| {np.max(np.abs(f64)):.4g}  max|kernel - f64| {err:.3g}  max|oracle - f64| {ref_err:.3g}  tol {tol:.3g}")
        assert err <= tol, name


def test_deepcpf1_inputs_and_refusals():
    rng = np.random.default_rng(106)
    w = R.deepcpf1_exact_weights("sparse", 0)
    scoring.set_deepcpf1_weights(w)
    homo = [b * 34 for b in "ACGT"]
    assert np.array_equal(_dc(homo).astype(np.float64), R.deepcpf1_f64(homo, w))
    seqs = R.random_kmers(rng, 65, 34)
    want = R.deepcpf1_f64(seqs, w)
    mixed = ["".join(c.lower() if rng.random() < 0.5 else c for c in s) for s in seqs]
    assert np.array_equal(_dc(mixed).astype(np.float64), want) and np.array_equal(_dc([s.lower() for s in seqs]).astype(np.float64), want)
    for pos in range(34):  # positions are encoded by wavefront pos % 4
        for ch in "NU- ":
            for n, at in ((64, 0), (64, 63), (65, 64)):  # lane 0, lane 63, the only guide of a partial block
                bad = list(seqs[:n])
                bad[at] = bad[at][:pos] + ch + bad[at][pos + 1:]
                with pytest.raises(CrisprHawkDeepCpf1ScoreError):
                    scoring.deepcpf1(bad)
        assert np.array_equal(_dc(seqs).astype(np.float64), want), pos  # a valid call after a refused one is unaffected


# ---------------------------------------------------------------------------------------------- k_azimuth
@pytest.fixture(scope="module")
def batch():
    seqs = R.azimuth_extreme_batch()
    return seqs, ora.azimuth_features(seqs)


def test_azimuth_features_at_their_extremes(batch):
    seqs, want = batch
    _, feats = _azimuth(seqs, R.pack_model([R.leaf_tree(1.0)]), feats=True)
    assert np.array_equal(feats[:, :623], want[:, :623])
    assert np.max(np.abs(feats[:, 623:] - want[:, 623:])) < 1e-9
    rng = np.random.default_rng(41)
    for group in (R.azimuth_homopolymers(), R.azimuth_dinucleotide_repeats(), [s for s, _ in R.azimuth_gc_window_cases(rng)],
                  R.azimuth_nggx_cases(rng)):  # each family alone as well: other batch sizes, other lanes
        _, f = _azimuth(group, R.pack_model([R.leaf_tree(1.0)]), feats=True)
        assert np.array_equal(f[:, :623], ora.azimuth_features(group)[:, :623])
    pairs = R.azimuth_tm_window_pairs(rng)
    _, fa = _azimuth([p[1] for p in pairs], R.pack_model([]), feats=True)
    _, fb = _azimuth([p[2] for p in pairs], R.pack_model([]), feats=True)
    for j, (col, a, b, inside) in enumerate(pairs):  # a base just outside a Tm window leaves its column bit for bit alone
        assert (fa[j, col] != fb[j, col]) == inside, (col, a, b)


def test_azimuth_every_feature_decides_once(batch):
    """stumps over each of the 627 columns, thresholds on a value taken, one float32 below and one above (and, for the Tm
    columns, between Tm and float32(Tm)); right leaves are powers of two, so the sum names every branch taken, exactly"""
    seqs, feats = batch
    specs = R.azimuth_stump_specs(feats)
    plain = [s for f in range(623) for s in specs[f]]
    for part, model in R.bit_stump_models(plain):
        _, leaves = R.gbt_eval(feats, model, True)
        got = _azimuth(seqs, model)
        want = R.bits_of(leaves)
        if not np.array_equal(got, want):
            i = int(np.flatnonzero(got != want)[0])
            wrong = [part[j] for j in range(len(part)) if (int(got[i]) >> j) & 1 != (int(want[i]) >> j) & 1]
            raise AssertionError(f"{seqs[i]}: stumps (feature, threshold) {wrong[:4]} went the other way")
    for col in range(623, 627):
        keep = R.f32_boundary_distance(feats[:, col]) > R.TM_BAND  # the device's log may differ from libm's in the last bits
        assert 1.0 - keep.mean() <= R.TM_LEFT_OUT_CAP
        for part, model in R.bit_stump_models(specs[col]):
            _, leaves = R.gbt_eval(feats, model, True)
            got = _azimuth(seqs, model)
            assert np.array_equal(got[keep], R.bits_of(leaves)[keep]), col


def test_azimuth_tree_shapes(batch):
    seqs, feats = batch
    for name, model in R.shape_ensembles(np.random.default_rng(9)).items():
        want, leaves = R.gbt_eval(feats, model, True)
        got = _azimuth(seqs, model)
        bound = R.gbt_sum_bound(model, leaves)
        assert np.all(np.abs(got - want) <= bound), (name, float(np.max(np.abs(got - want) - bound)))
        if name in ("no_trees", "one_leaf"):
            assert np.array_equal(got, want), name
    assert np.array_equal(_azimuth(seqs[:3], R.shape_ensembles(np.random.default_rng(9))["no_trees"]), [0.37] * 3)


def test_azimuth_batch_sizes(batch):
    seqs, feats = batch
    model = R.shape_ensembles(np.random.default_rng(9))["mixed_60"]
    want, leaves = R.gbt_eval(feats, model, True)
    bound = R.gbt_sum_bound(model, leaves)
    for n in (1, 255, 256, 257, 2 ** 18 + 5):
        idx = (np.arange(n, dtype=np.int64) * 11 + 5) % len(seqs)
        sub = [seqs[i] for i in idx]
        if n < 1000:
            got, f = _azimuth(sub, model, feats=True)
            assert f.shape == (n, 627) and np.array_equal(f[:, :623], feats[idx, :623]) and np.max(np.abs(f[:, 623:] - feats[idx, 623:])) < 1e-9
        else:
            got = _azimuth(sub, model)
        assert got.shape == (n,) and np.all(np.abs(got - want[idx]) <= bound[idx]), n
    with pytest.raises(CrisprHawkAzimuthScoreError):
        scoring.azimuth(seqs[:256] + ["ACGTN" + "A" * 25])


def test_tree_refusals_launch_nothing(batch):
    seqs, _ = batch
    for what, model in R.broken_models(627):
        out = np.full(4, -7.0)
        assert _raw_azimuth(seqs[:4], model, out) == _lib.HAWK_E_INVALID, what
        assert (out == -7.0).all(), what
    x = np.zeros((4, 9))
    for what, model in R.broken_models(9):
        for cast in (0, 1):
            out = np.full(4, -7.0)
            assert _raw_gbt(x, model, cast, out) == _lib.HAWK_E_INVALID, what
            assert (out == -7.0).all(), what
    good = R.pack_model([R.stump(8, 0.5, 1.0, 2.0)])  # the last column is in range
    out = np.full(4, -7.0)
    assert _raw_gbt(x, good, 0, out) == _lib.HAWK_OK and (out == 1.0).all()


def test_tm_nn_at_the_ends_of_its_range():
    rng = np.random.default_rng(107)
    for ln in (2, 32):
        seqs = [b * ln for b in "ACGT"] + R.random_kmers(rng, 300, ln)
        got = np.asarray(scoring.tm_nn(seqs))
        assert np.max(np.abs(got - np.array([ora.tm_nn(s) for s in seqs]))) < 1e-9, ln
    for ln in (1, 33):
        with pytest.raises(_lib.HawkStatusError) as e:
            scoring.tm_nn(["A" * ln])
        assert e.value.status == _lib.HAWK_E_UNSUPPORTED
    with pytest.raises(_lib.HawkStatusError):
        scoring.tm_nn(["AC", "AN"])


# ---------------------------------------------------------------------------------------------- k_gbt
@pytest.mark.parametrize("nf,first", [(1, True), (627, True), (627, False), (5000, True), (5000, False)])
def test_gbt_cast_on_and_off(nf, first):
    for n in (1, 255, 256, 257):
        x, specs = R.gbt_cast_cases(n, nf, first)
        (part, model), = R.bit_stump_models(specs)
        parted = 0
        got = {}
        for cast in (False, True):
            with np.errstate(over="ignore"):
                _, leaves = R.gbt_eval(x, model, cast)
            got[cast] = scoring.gbt_predict(x, model, cast_f32=cast)
            want = R.bits_of(leaves)
            assert np.array_equal(got[cast], want), (n, cast, [part[j] for j in range(len(part))
                                                               if any((int(a) >> j) & 1 != (int(b) >> j) & 1 for a, b in zip(got[cast], want))][:4])
        if n >= 16:
            assert (got[False] != got[True]).sum() >= len(R.GBT_HARD_VALUES)
        # the same splits under a learning rate that is no power of two: the sum inside its derived bound
        m2 = dict(model, learning_rate=0.1, value=model["value"] * 1e-3 + 0.25)
        for cast in (False, True):
            with np.errstate(over="ignore"):
                want, leaves = R.gbt_eval(x, m2, cast)
            assert np.all(np.abs(scoring.gbt_predict(x, m2, cast_f32=cast) - want) <= R.gbt_sum_bound(m2, leaves)), (n, cast)


def test_gbt_tree_shapes_over_a_supplied_matrix():
    seqs = R.azimuth_extreme_batch()[:300]
    feats = ora.azimuth_features(seqs)
    for name, model in R.shape_ensembles(np.random.default_rng(9)).items():
        for cast in (False, True):
            want, leaves = R.gbt_eval(feats, model, cast)
            got = scoring.gbt_predict(feats, model, cast_f32=cast)
            assert np.all(np.abs(got - want) <= R.gbt_sum_bound(model, leaves)), (name, cast)


# ---------------------------------------------------------------------------------------------- k_cfd
def test_cfd_edge_rows_against_the_reference():
    fx = R.cfd_edges()
    scoring.set_cfd_tables(*synth.cfd_tables(fx["seed"]))
    good = [r for r in fx["rows"] if not isinstance(r[3], dict)]
    bad = [r for r in fx["rows"] if isinstance(r[3], dict)]
    got = scoring.compute_cfd_batch([r[0] for r in good], [r[1] for r in good], [r[2] for r in good], True)
    assert got.tolist() == [r[3] for r in good]  # all lengths in one call: the wrapper batches them per length
    for ln in sorted({len(r[0]) for r in good}):
        rows = [r for r in good if len(r[0]) == ln]
        for n in (1, 255, 256, 257):
            sub = [rows[(i * 5 + 1) % len(rows)] for i in range(n)]
            got = scoring.compute_cfd_batch([r[0] for r in sub], [r[1] for r in sub], [r[2] for r in sub], True)
            assert got.tolist() == [r[3] for r in sub], (ln, n)
    for wt, sg, pam, _ in bad:
        with pytest.raises(CrisprHawkCfdScoreError):
            scoring.compute_cfd_batch([wt], [sg], [pam], True)


def test_cfd_one_bad_row_in_a_batch():
    fx = R.cfd_edges()
    mm, pt = synth.cfd_tables(fx["seed"])
    good = [r for r in fx["rows"] if not isinstance(r[3], dict) and len(r[0]) == 23]
    bad = [r for r in fx["rows"] if isinstance(r[3], dict) and len(r[0]) == 23]
    assert len(good) >= 300 and bad
    for at, b in ((0, bad[0]), (255, bad[1]), (256, bad[-1]), (599, bad[len(bad) // 2])):
        rows = [good[i % len(good)] for i in range(600)]
        rows[at] = b
        out = np.full(600, -7.0)
        mmc, ptc = np.ascontiguousarray(mm), np.ascontiguousarray(pt)
        rc = _lib.lib().hawk_cfd(_lib.context(), "".join(r[0] for r in rows).encode("ascii"), "".join(r[1] for r in rows).encode("ascii"), 23,
                                 "".join(r[2] for r in rows).encode("ascii"), C.c_uint64(600), _vp(mmc), _vp(ptc), _vp(out))
        assert rc == _lib.HAWK_E_CFD and np.isnan(out[at])
        keep = np.arange(600) != at
        assert out[keep].tolist() == [r[3] for i, r in enumerate(rows) if i != at]
