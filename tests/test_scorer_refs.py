"""The references of tests/scorer_refs.py checked without a GPU, and every condition the GPU scorer tests rest on: the exact
DeepCpf1 weight sets stay inside fp32, the fp32 oracle reproduces float64 on them, the share of 30-mers a Tm stump has to leave
out stays under its cap, the case builders reach the extremes they are named after, and the CPU oracle's CFD equals the
reference's compute_cfd on the edge rows of g5_cfd_edges."""
import numpy as np
import pytest

import scorer_refs as R
from crisprhawk_hip import synth
from oracle import oracle as ora
from util import load_golden


# ---------------------------------------------------------------------------------------------- DeepCpf1
def test_deepcpf1_f64_against_reference_forward_and_oracle():
    g6 = load_golden("g6_deepcpf1.json.gz")  # SeqDeepCpf1 in torch fp32, run by the reference
    w = synth.deepcpf1_weights(g6["seed"])
    f64 = R.deepcpf1_f64(g6["seqs"], w)
    # fp32 evaluations of a 1200-term layer sit a few 1e-8 from float64 at |score| ~ 0.15; two of them (torch's blocked order,
    # the oracle's sequential one) against one float64 statement
    assert np.max(np.abs(f64 - np.array(g6["scores"]))) < 5e-7
    assert np.max(np.abs(f64 - ora.deepcpf1(g6["seqs"], w))) < 5e-7
    assert np.array_equal(R.deepcpf1_f64([s.lower() for s in g6["seqs"]], w), f64)
    with pytest.raises(KeyError):
        R.deepcpf1_f64(["ACGT" * 8 + "AN"], w)


@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_exact_weight_sets_stay_inside_fp32(kind):
    """the bit budget of the builder's docstring, recomputed from the weights themselves; then the fp32 oracle must
    reproduce float64 exactly, on scores that are not trivially zero"""
    rng = np.random.default_rng(5)
    seqs = R.random_kmers(rng, 300, 34) + [b * 34 for b in "ACGT"]
    for seed in (0, 1):
        w = R.deepcpf1_exact_weights(kind, seed)
        for k in R.DC_KEYS:
            assert w[k].dtype == np.float32
        budget = R.deepcpf1_bit_budget(w)
        assert all(bits <= 24.0 for _, bits, _, _ in budget), budget
        f64 = R.deepcpf1_f64(seqs, w)
        got = ora.deepcpf1(seqs, w)
        assert np.array_equal(got.astype(np.float64), f64)
        assert len(np.unique(f64)) > 200 and np.max(np.abs(f64)) > 8.0


def test_probe_family_has_one_deciding_path():
    rng = np.random.default_rng(6)
    seqs = R.random_kmers(rng, 100, 34)
    sweep = R.deepcpf1_probe_sweep()
    assert {p[0] for p in sweep} == set(range(15)) and {p[2] for p in sweep} == set(range(5))
    assert {(p[0], p[2], p[1] // 20) for p in sweep} == {(t, k, q) for t in range(15) for k in range(5) for q in range(4)}
    assert {p[4] // 20 for p in sweep} == {0, 1, 2, 3}
    for t, c, k, base, o, o2, o3 in sweep[::7]:
        w = R.deepcpf1_probe(t, c, k, base, o, o2, o3)
        assert all(bits <= 24.0 for _, bits, _, _ in R.deepcpf1_bit_budget(w))
        want = R.deepcpf1_probe_closed_form(seqs, t, k, base)
        assert np.array_equal(R.deepcpf1_f64(seqs, w), want)
        assert np.array_equal(ora.deepcpf1(seqs, w).astype(np.float64), want)
        assert len(np.unique(want)) == 3  # 0, 1 or 2 of the pooled pair answer


def test_random_weight_scales_reach_their_ranges():
    rng = np.random.default_rng(7)
    seqs = R.random_kmers(rng, 400, 34)
    seen = {}
    for name, sigma in R.DC_SCALES:
        w = R.deepcpf1_scaled_weights(sigma)
        f64 = R.deepcpf1_f64(seqs, w)
        tol, ref_err = R.deepcpf1_tolerance(ora.deepcpf1(seqs, w), f64)
        seen[name] = (float(np.max(np.abs(f64))), ref_err, tol)
        print(f"deepcpf1 {name}: sigma {sigma} max|f64| {seen[name][0]:.4g} max|oracle - f64| {ref_err:.3g} tol {tol:.3g}")
        assert tol >= float(np.spacing(np.float32(seen[name][0]))) and tol >= 4 * ref_err
    assert seen["n01"][0] < 1.0
    assert 5.0 < seen["near10"][0] < 20.0
    assert 25.0 < seen["near50"][0] < 100.0


# ---------------------------------------------------------------------------------------------- trees
def _random_complete(rng, n_trees, nfeat):
    trees = []
    for _ in range(n_trees):
        nodes = []
        for k in range(15):
            if k < 7:
                nodes.append((int(rng.integers(0, nfeat)), 2 * k + 1, 2 * k + 2, float(rng.normal()), 0.0))
            else:
                nodes.append((-1, 0, 0, 0.0, float(rng.normal())))
        trees.append(nodes)
    return R.pack_model(trees, init=0.37, lr=0.1)


def test_gbt_eval_against_oracle():
    rng = np.random.default_rng(8)
    x = rng.normal(size=(200, 9))
    x[::7, 3] = np.float64(np.float32(x[::7, 3]))
    m = _random_complete(rng, 30, 9)
    m["threshold"][::5] = x[rng.integers(0, 200, size=len(m["threshold"][::5])), m["feature"][::5].clip(0)]  # ties
    total, leaves = R.gbt_eval(x, m, cast_f32=True)
    assert np.array_equal(total, ora.gbt_predict(x, m))  # the oracle casts, and sums in the same order
    assert leaves.shape == (200, 30) and (m["feature"][m["tree_off"][:-1][None, :] + leaves] == -1).all()
    t0, l0 = R.gbt_eval(x, m, cast_f32=False)
    assert (l0 != leaves).any()  # thresholds equal to a float64 the cast moves: the two modes part
    for name, model in R.shape_ensembles(np.random.default_rng(9)).items():
        feats = ora.azimuth_features(R.azimuth_extreme_batch()[:120])
        total, leaves = R.gbt_eval(feats, model, True)
        assert np.array_equal(total, ora.gbt_predict(feats, model)), name
        assert np.all(R.gbt_sum_bound(model, leaves) >= 0)


def test_gbt_eval_against_sklearn_with_single_leaf_trees():
    sk = pytest.importorskip("sklearn.ensemble")
    from crisprhawk_hip.scoring import azimuth_model_from_sklearn
    rng = np.random.default_rng(10)
    x = rng.normal(size=(300, 5)) / 3.0
    y = x[:, 0] - 2 * (x[:, 3] > 0.1) + rng.normal(0, 0.05, 300)
    gbr = sk.GradientBoostingRegressor(n_estimators=40, max_depth=3, learning_rate=0.1, random_state=2).fit(x, y)
    m = azimuth_model_from_sklearn(gbr)
    total, leaves = R.gbt_eval(x, m, True)
    assert np.max(np.abs(total - gbr.predict(x)) - R.gbt_sum_bound(m, leaves)) <= 0
    # sklearn's own leaf ids are node ids of its tree_: the flattener keeps them
    assert np.array_equal(leaves, gbr.apply(x).astype(np.int64))
    # a constant target leaves nothing to split: every tree is a single leaf
    flat = sk.GradientBoostingRegressor(n_estimators=5, max_depth=3, random_state=2).fit(x, np.full(300, 1.5))
    mf = azimuth_model_from_sklearn(flat)
    assert len(mf["feature"]) == 5 and (mf["feature"] == -1).all()
    total, leaves = R.gbt_eval(x, mf, True)
    assert (leaves == 0).all() and np.max(np.abs(total - flat.predict(x))) <= 5 * 2.0 ** -52 * 1.5 * 2


def test_shape_ensembles_cover_the_shapes():
    ms = R.shape_ensembles(np.random.default_rng(9))
    sizes = lambda m: np.diff(m["tree_off"])
    assert len(ms["no_trees"]["tree_off"]) == 1 and len(ms["no_trees"]["feature"]) == 0
    assert sizes(ms["one_leaf"]).tolist() == [1] and sizes(ms["left_chain_12"]).tolist() == [25]
    assert len(sizes(ms["mixed_1000"])) == 1000 and len(set(sizes(ms["mixed_1000"]).tolist())) >= 6 and 1 in sizes(ms["mixed_1000"])
    v = np.abs(ms["leaf_1e-8_to_1e8"]["value"])
    assert v[v > 0].min() <= 1e-8 and v.max() >= 1e8
    feats = ora.azimuth_features(R.azimuth_extreme_batch())
    for name in ("left_chain_12", "right_chain_12"):
        _, leaves = R.gbt_eval(feats, ms[name], True)
        assert len(np.unique(leaves)) >= 4, name  # the batch leaves the chain at several depths
    for name, m in ms.items():  # children point forward and stay inside: what the entry points accept
        for t in range(len(m["tree_off"]) - 1):
            lo, hi = m["tree_off"][t], m["tree_off"][t + 1]
            for k in range(lo, hi):
                if m["feature"][k] >= 0:
                    assert k - lo < m["left"][k] < hi - lo and k - lo < m["right"][k] < hi - lo


# ---------------------------------------------------------------------------------------------- Azimuth features
def test_extreme_batch_reaches_the_extremes():
    rng = np.random.default_rng(41)
    f = ora.azimuth_features(R.azimuth_homopolymers())
    assert sorted(f[:, 120:124].max(axis=1).tolist()) == [30.0] * 4 and f[:, 120:124].min() == 0.0
    assert sorted(f[:, 588:604].max(axis=1).tolist()) == [29.0] * 4
    f = ora.azimuth_features(R.azimuth_dinucleotide_repeats())
    assert f[:, 588:604].max() == 29.0 and {15.0, 14.0} <= set(np.unique(f[:, 588:604]))
    cases = R.azimuth_gc_window_cases(rng)
    f = ora.azimuth_features([s for s, _ in cases])
    assert f[:, 606].tolist() == [float(g) for _, g in cases] and {g for _, g in cases} == {0, 9, 10, 11, 20}
    for s, g in cases:  # a window one base to the left or to the right counts differently
        assert sum(c in "CG" for c in s[3:23]) != g and sum(c in "CG" for c in s[5:25]) != g
    for g in (0, 9, 10, 11):  # and so does the whole 30-mer (at 20 the flanks hold no G or C to add)
        assert sum(sum(c in "CG" for c in s) != g for s, g2 in cases if g2 == g) >= 2
    assert np.array_equal(f[:, 604], f[:, 606] > 10) and np.array_equal(f[:, 605], f[:, 606] < 10)
    nggx = R.azimuth_nggx_cases(rng)
    f = ora.azimuth_features(nggx)
    assert (f[:, 607:623].sum(axis=1) == 1).all() and (f[:, 607:623].sum(axis=0) == 16).all()
    for col, a, b, inside in R.azimuth_tm_window_pairs(rng):
        fa, fb = ora.azimuth_features([a, b])[:, col]
        assert (fa != fb) == inside, (col, a, b)
    feats = ora.azimuth_features(R.azimuth_extreme_batch())
    assert (feats[:, :623].min(axis=0) < feats[:, :623].max(axis=0)).all()  # every column takes two values: a stump can split it


def test_tm_stumps_leave_out_at_most_their_cap():
    feats = ora.azimuth_features(R.azimuth_extreme_batch())
    for col in range(623, 627):
        tm = feats[:, col]
        out = R.f32_boundary_distance(tm) <= R.TM_BAND
        print(f"Tm column {col}: {out.sum()} of {len(tm)} within {R.TM_BAND} of a float32 rounding boundary, |Tm| from {np.abs(tm).min():.3g}")
        assert out.mean() <= R.TM_LEFT_OUT_CAP
        specs = R.azimuth_stump_specs(feats)[col]
        between = [t for _, t in specs[-6:]]
        t32, l32 = R.gbt_eval(feats, R.pack_model([R.stump(col, t, 0, 1) for t in between]), True)
        t64, l64 = R.gbt_eval(feats, R.pack_model([R.stump(col, t, 0, 1) for t in between]), False)
        assert ((l32 != l64).sum(axis=0) >= 1).all()  # each of them parts a cast evaluation from an uncast one


def test_stump_specs_put_thresholds_on_values_taken():
    feats = ora.azimuth_features(R.azimuth_extreme_batch())
    specs = R.azimuth_stump_specs(feats)
    assert sorted(specs) == list(range(627))
    f32 = feats.astype(np.float32).astype(np.float64)
    for f, sp in specs.items():
        ths = [t for _, t in sp]
        assert any((f32[:, f] == t).any() for t in ths)
        m = R.pack_model([R.stump(f, t, 0, 1) for t in ths])
        _, leaves = R.gbt_eval(feats, m, True)
        assert len(np.unique(leaves)) == 2, f  # both branches are taken on the batch
    part, model = R.bit_stump_models([s for f in range(3) for s in specs[f]])[0]
    total, leaves = R.gbt_eval(feats, model, True)
    assert np.array_equal(total, R.bits_of(leaves)) and total.max() < 2.0 ** 53


def test_gbt_cast_cases_part_the_two_modes():
    for nf, first in ((1, True), (627, True), (627, False), (5000, False)):
        x, specs = R.gbt_cast_cases(64, nf, first)
        _, model = R.bit_stump_models(specs)[0]
        with np.errstate(over="ignore"):
            t1, l1 = R.gbt_eval(x, model, True)
        t0, l0 = R.gbt_eval(x, model, False)
        assert (l1 != l0).any(axis=0).sum() >= 2 * len(R.GBT_HARD_VALUES)
        assert np.array_equal(t1, R.bits_of(l1)) and np.array_equal(t0, R.bits_of(l0))
        zero = [j for j, (_, t) in enumerate(specs) if t == 0.0]
        rows = np.flatnonzero(x[:, specs[0][0]] == 0.0)
        assert len(rows) >= 2 and (l1[np.ix_(rows, zero)] == 1).all() and (l0[np.ix_(rows, zero)] == 1).all()  # +-0 <= +-0: left


def test_broken_models_are_broken_and_named():
    names = [n for n, _ in R.broken_models(627)]
    assert len(set(names)) == len(names) >= 10


# ---------------------------------------------------------------------------------------------- CFD
def test_oracle_cfd_on_the_reference_edge_rows():
    """pins the oracle's bulge branch, U and case folding and its 20-base limit to compute_cfd itself"""
    fx = R.cfd_edges()
    mm, pt = synth.cfd_tables(fx["seed"])
    n_err = 0
    for wt, sg, pam, want in fx["rows"]:
        if isinstance(want, dict):
            assert want["error"] == "KeyError"
            with pytest.raises(ora.OracleError):
                ora.cfd(wt, sg, pam, mm, pt)
            n_err += 1
        else:
            assert ora.cfd(wt, sg, pam, mm, pt) == want, (wt, sg, pam)
    rows = fx["rows"]
    assert n_err > 100 and len(rows) > 3000
    assert {len(r[0]) for r in rows} >= {1, 2, 16, 19, 20, 21, 24, 25}
    assert any("-" in r[0] and "-" in r[1] for r in rows) and any("U" in r[0] for r in rows) and any("u" in r[0] for r in rows)
    # every table entry is the only factor of some row
    vals = {r[3] for r in rows if not isinstance(r[3], dict)}
    gg = pt[4 * 2 + 2]
    for i in range(20):
        for a in range(4):
            for b in range(4):
                if a != b:
                    assert mm[i, a, b] * gg in vals or 1.0 * mm[i, a, b] * gg in vals
    assert all(float(p) in vals for p in pt)
