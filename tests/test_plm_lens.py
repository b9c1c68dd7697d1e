"""The conditions of the PLM-CRISPR lenses (tests/plm_lens.py), without a device: under each set the float64 score of every row
used on the device answers a 2^-10 error in any single element of the observed layer with more than twice the tolerance the
device is held to under that set, and the mutations of the restatement that the plain g15 parameters let pass are seen."""
import functools

import numpy as np
import pytest

import plm_lens
import plm_refs
from plm_lens import PERTURBATION
from plm_refs import plm_layers, plm_tolerance


@functools.lru_cache(maxsize=4)
def layers(name):
    """(params, float64 layers, tolerance) of a sgrna-branch lens on its device rows; the last few are kept"""
    params, protein = plm_lens.lens(name), plm_lens.g15()[1]
    seqs = plm_lens.lens_guides(name)
    l64 = plm_layers(seqs, params, protein, np.float64)
    tol, err = plm_tolerance(plm_refs.plm_f32(seqs, params, protein), l64["score"])
    return params, l64, tol


def _edges(width, count):
    """first and last element of `count` consecutive stretches of `width`"""
    first = np.arange(count) * width
    return np.concatenate([first, first + width - 1])


def _moves(name, layer, elems):
    """|change of each row's float64 score| when PERTURBATION is added to element e of `layer` in every row: (len(elems), n)"""
    params, l64, tol = layers(name)
    P = plm_refs._cast(params, np.float64)
    out = np.empty((len(elems), len(l64["score"])))
    for i, e in enumerate(elems):
        if layer == "sg":
            sg = l64["sg"].copy()
            sg[:, e] += PERTURBATION
        else:
            if layer == "h1":
                units, dh = np.array([e]), np.full((len(out[i]), 1), PERTURBATION)
            else:  # the feature's column of lin1 is sparse: only the units that read it change
                units = np.flatnonzero(P["lin1.weight"][:, e])
                feat = l64["feat"].copy()
                feat[:, e] += PERTURBATION
                dh = plm_refs._sigmoid(feat @ P["lin1.weight"][units].T + P["lin1.bias"][units]) - l64["h1"][:, units]
            sg = l64["sg"] + dh @ P["lin3.weight"][:, units].T
        out[i] = np.abs(plm_refs._tail(sg, l64["prot"], P) - l64["score"])
    return out, tol


def _observed(name):
    kind, _, arg = name.partition(":")
    if kind == "head":
        return "sg", np.arange(256)
    if kind in ("route", "k"):  # every 7th unit and both ends of every 32-column MFMA tile (so of every wave half and N tile)
        return "h1", np.unique(np.concatenate([np.arange(0, 2048, 7), _edges(32, 64)]))
    e = plm_lens.observed_features(int(arg))
    if e[0] >= 3776:
        return "feat", e
    ends = np.concatenate([_edges(59, 128), [3775, 3776]])  # both ends of every channel of both branches
    return "feat", np.unique(np.concatenate([e[::7], ends[(ends >= e[0]) & (ends <= e[-1])]]))


@pytest.mark.parametrize("name", plm_lens.SGRNA_LENSES)
def test_every_row_answers_a_single_element_error(name):
    """2^-10 in one observed element moves that row's float64 score by more than 2 x plm_tolerance of the lens's own fp32 /
    float64 pair, for every row of the lens's device rows.  Under plain g15 the same error moves 7 % (feature 3775) to 10 %
    (lin1 unit 2047) of the pool's scores past the tolerance at all.  Measured weakest answers, in tolerances: head 3.3, route
    3.1, the K-slices 8.1 to 11.8, the first branch's two feature sets 9.3 and 7.1, conv4's sixteen 2.6 to 5.0."""
    layer, elems = _observed(name)
    moves, tol = _moves(name, layer, elems)
    ratio = moves.min() / tol
    e, r = np.unravel_index(np.argmin(moves), moves.shape)
    print(f"{name}: {len(elems)} elements of {layer} x {moves.shape[1]} rows, tolerance {tol:.3e}; weakest answer {moves.min():.3e} "
          f"= {ratio:.2f} x tolerance (element {elems[e]}, row {r}); strongest {moves.max() / tol:.1f} x")
    assert ratio > 2.0


def test_lens_structure():
    params = plm_lens.g15()[0]
    head = plm_lens.head_lens(15, params)
    assert np.array_equal(np.count_nonzero(head["lin5.weight"], axis=0), np.ones(256)), "every sg unit is read once"
    assert np.array_equal(np.count_nonzero(head["lin5.weight"], axis=1), np.full(128, 2))
    l6 = head["lin6.weight"][0]
    assert np.array_equal(np.sort(l6[l6 > 0]), np.sort(-l6[l6 < 0])) and (l6 > 0).sum() == 64 and np.abs(l6).min() >= 0.7
    assert head["lin1.weight"] is params["lin1.weight"] and head["lin3.weight"] is params["lin3.weight"], "the GEMM pair as shipped"
    # w0 = 1 in fp32: the softmax of (+60, -60)
    lg = np.array([60.0, -60.0], np.float32)
    e = np.exp(lg - lg.max())
    assert (e / e.sum())[0] == np.float32(1.0) and (e / e.sum())[1] == 0
    route = plm_lens.route_lens(15, params)
    w3 = route["lin3.weight"]
    assert np.array_equal(np.count_nonzero(w3, axis=0), np.ones(2048)) and np.array_equal(np.count_nonzero(w3, axis=1), np.full(256, 8))
    for s in (0, 77, 255):
        g = w3[s][np.flatnonzero(w3[s])]
        assert len(set(np.abs(g).tolist())) == 8 and (g > 0).sum() == 4, "the gains differ within a unit"
        assert np.array_equal(np.flatnonzero(w3[s]) // 128, 2 * np.arange(8) + (s >= 128)), "eight different N tiles"
    for which, (lo, hi, gain) in plm_lens.K_SLICES.items():
        w1 = plm_lens.kslice_lens(15, params, which)["lin1.weight"]
        cols = np.flatnonzero(np.any(w1 != 0, axis=0))
        assert cols[0] == lo and cols[-1] == hi - 1 and len(cols) == hi - lo
    assert plm_lens.K_SLICES["seam"][0] < 3776 < plm_lens.K_SLICES["seam"][1] and plm_lens.K_SLICES["seam"][0] % 128 == 0
    # the feature sets: together every feature is read by exactly one unit, at most four per unit
    read = np.zeros(7552, int)
    per_unit = np.zeros(2048, int)
    for part in range(len(plm_lens.FEATURE_SETS)):
        p = plm_lens.feature_lens(15, params, part)
        w1 = p["lin1.weight"]
        u, e = np.nonzero(w1)
        assert np.array_equal(np.sort(e), plm_lens.observed_features(part)) and np.array_equal(plm_lens.feature_unit(e), u)
        assert np.all(p["lin1.bias"][np.setdiff1d(np.arange(2048), u)] == -40)
        read[e] += 1
        per_unit[u] += 1
    assert np.all(read == 1) and per_unit.max() == 4 and per_unit.min() == 3


def _affected_rows_move(name, layer, mutated, what, least=PERTURBATION):
    """rows whose `layer` the mutation changes by at least 2^-10 somewhere (the error size a lens answers for) must leave the
    lens's tolerance"""
    params, l64, tol = layers(name)
    affected = np.flatnonzero(np.max(np.abs(mutated - l64[layer]), axis=1) >= least)
    move = np.abs(plm_refs.plm_resume(layer, mutated, params, l64["prot"]) - l64["score"])
    print(f"{what} under {name}: {len(affected)} of {len(move)} rows affected; weakest move {move[affected].min():.3e} = "
          f"{move[affected].min() / tol:.1f} x tolerance {tol:.3e}")
    assert len(affected) >= 0.8 * len(move), "the mutation is a real one for most rows"
    assert np.all(move[affected] > tol), what


def _feature_set_of(e):
    return next(i for i, (lo, hi, _, _) in enumerate(plm_lens.FEATURE_SETS) if lo <= e < hi)


@pytest.mark.parametrize("branch", [0, 1])
def test_mutation_last_position_copied_from_its_neighbour(branch):
    """feature (channel 63, position 58) copied from (63, 57): a convolution that stops one position early.  Under plain g15 a
    10^-3 error in feature 3775 moves 7 % of the pool's scores past the tolerance."""
    e = 3776 * branch + 63 * 59 + 58
    name = f"feature:{_feature_set_of(e)}"
    feat = layers(name)[1]["feat"].copy()
    feat[:, e] = feat[:, e - 1]
    _affected_rows_move(name, "feat", feat, f"feature {e} copied from {e - 1}")


def test_mutation_first_position_of_the_linear_branch_zeroed():
    """feature (5, 0) of `be` zeroed: a padding column read in place of position 0"""
    e = 3776 + 5 * 59
    name = f"feature:{_feature_set_of(e)}"
    feat = layers(name)[1]["feat"].copy()
    feat[:, e] = 0
    _affected_rows_move(name, "feat", feat, f"feature {e} zeroed")


@pytest.mark.parametrize("name", ["route", "k:last", "k:stage"])
def test_mutation_lin1_unit_without_its_last_flush(name):
    """lin1 unit 2047 without its last 128 products: the last flush dropped.  Under plain g15 a 10^-3 error in that unit moves
    10 % of the pool's scores past the tolerance."""
    params, l64, tol = layers(name)
    w = params["lin1.weight"][2047].astype(np.float64)
    h1 = l64["h1"].copy()
    pre = l64["feat"] @ w + np.float64(params["lin1.bias"][2047])
    assert np.allclose(plm_refs._sigmoid(pre), h1[:, 2047], rtol=0, atol=1e-12)
    h1[:, 2047] = plm_refs._sigmoid(pre - l64["feat"][:, 7424:] @ w[7424:])
    _affected_rows_move(name, "h1", h1, "unit 2047 without k = 7424..7551")


def test_mutation_rows_swapped_within_a_tile():
    """units 64..95 of h1 (one 32-column MFMA tile) swapped between rows 4 and 8, which the C/D register mapping
    (r & 3) + 8 (r >> 2) + 4 (lane >> 5) places in different registers.  Under plain g15 the same swap moved no score by more
    than 1.8e-8, a fiftieth of the tolerance."""
    params, l64, tol = layers("route")
    h1 = l64["h1"].copy()
    h1[4, 64:96], h1[8, 64:96] = l64["h1"][8, 64:96], l64["h1"][4, 64:96]
    move = np.abs(plm_refs.plm_resume("h1", h1, params, l64["prot"]) - l64["score"])
    print(f"rows 4 and 8 swapped in units 64..95: moves {move[4]:.3e}, {move[8]:.3e}; tolerance {tol:.3e}")
    assert move[4] > tol and move[8] > tol and np.all(np.delete(move, [4, 8]) < 1e-12)
    # the same under plain g15, for the record
    g15, protein = plm_lens.g15()
    d = plm_layers(plm_lens.pool_guides()[:16], g15, protein, np.float64)
    h1 = d["h1"].copy()
    h1[4, 64:96], h1[8, 64:96] = d["h1"][8, 64:96], d["h1"][4, 64:96]
    plain = np.abs(plm_refs.plm_resume("h1", h1, g15, d["prot"]) - d["score"])
    print(f"under plain g15: {plain[4]:.3e}, {plain[8]:.3e}")


# ------------------------------------------------------------------------------------------------------------ protein branch
PROTEIN_L = [13, 20, 21, 24, 25, 28, 29, 36, 37, 200]


@pytest.mark.parametrize("L", PROTEIN_L)
def test_protein_lens_conditions(L):
    """No lin4 unit is relu'd, every pooled feature has a gain, the forced position is the argmax of every live channel in
    float64 and in fp32, and the forced position's value replaced by the runner-up's moves out_protein past twice its
    tolerance.  Under plain g15 116-121 of the 256 units are relu'd to a constant at every tested length, and at L = 200 the
    last position of the kernel-13 convolution is the argmax of none of its channels."""
    g15 = plm_lens.g15()[0]
    for conv in range(3):
        for pos in plm_lens.forced_positions(L, conv):
            params, emb = plm_lens.protein_lens(15, g15, L, conv, pos)
            y64, y32 = plm_lens.conv_outputs(params, emb, conv, np.float64), plm_lens.conv_outputs(params, emb, conv, np.float32)
            live = params[f"text_cnn.convs.{conv}.bias"] > -1
            assert (~live).sum() == plm_lens.DEAD_CHANNELS and np.all(y64[:, ~live] < 0)
            assert np.all(y64.argmax(axis=0)[live] == pos) and np.all(y32.argmax(axis=0)[live] == pos), (L, conv, pos)
            pooled = plm_refs._pooled(params, emb, np.float64)
            lo = 128 * conv
            assert np.all(pooled[lo:lo + 128][~live] == 0) and np.all(pooled[lo:lo + 128][live] == y64[pos, live])
            w4 = params["lin4.weight"].astype(np.float64)
            assert np.all(np.count_nonzero(w4, axis=0) == 1) and np.all(w4 >= 0)
            pre = w4 @ pooled + params["lin4.bias"]
            assert pre.min() > 0.1 and pre.max() < 2.0
            p64, p32 = plm_refs.protein_head(pooled, params, np.float64), plm_refs.protein_f32(params, emb)
            assert np.array_equal(p64, plm_refs.protein_f64(params, emb))
            tol, err = plm_tolerance(p32, p64)
            if y64.shape[0] > 1:  # the pool without the forced position: the runner-up's value
                second = pooled.copy()
                second[lo:lo + 128] = np.maximum(np.delete(y64, pos, axis=0), 0).max(axis=0)
                units = np.r_[lo:lo + 128] if conv < 2 else np.r_[0:128]
                move = np.abs(plm_refs.protein_head(second, params, np.float64) - p64)[units][live]
                assert move.min() > 2 * tol, (L, conv, pos, move.min(), tol)


@pytest.mark.parametrize("conv", [0, 1, 2])
def test_mutation_last_text_cnn_position_dropped(conv):
    """the pool without the convolution's last position, at L = 200 and at L = 28 (where a kernel-13 tile starts at P and
    returns early): every live channel's unit leaves the tolerance"""
    g15 = plm_lens.g15()[0]
    for L in (28, 200):
        pos = L - plm_lens.KERNELS[conv]
        params, emb = plm_lens.protein_lens(15, g15, L, conv, pos)
        pooled = plm_refs._pooled(params, emb, np.float64)
        p64 = plm_refs.protein_head(pooled, params, np.float64)
        tol, err = plm_tolerance(plm_refs.protein_f32(params, emb), p64)
        dropped = pooled.copy()
        dropped[128 * conv:128 * conv + 128] = np.maximum(plm_lens.conv_outputs(params, emb, conv, np.float64)[:-1], 0).max(axis=0)
        move = np.abs(plm_refs.protein_head(dropped, params, np.float64) - p64)
        seen = int((move > tol).sum())
        print(f"kernel {plm_lens.KERNELS[conv]}, L = {L}: {seen} units leave the tolerance {tol:.3e}; largest move {move.max():.3e}")
        assert seen == 128 - plm_lens.DEAD_CHANNELS
