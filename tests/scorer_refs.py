"""Plain references and case builders for the scorer tests (numpy and the CPU oracle only, no GPU): what
tests/test_scorer_refs.py checks on the CPU and tests/test_gpu_scorers.py then holds the kernels to.

  deepcpf1_f64        SeqDeepCpf1 (scores/deepCpf1/seqdeepcpf1.py:22-92) in float64, from the network's definition
  gbt_eval            a flattened tree ensemble in pure Python: the sum AND the leaf reached in every tree
  exact / probe / scaled weight sets for DeepCpf1, the worst-case bit budget of a weight set
  30-mers at the extremes of the Azimuth features, stump ensembles with power-of-two leaves, tree-shape ensembles
"""
import math

import numpy as np

DC_KEYS = ("conv_w", "conv_b", "w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4")
DC_SHAPES = ((80, 4, 5), (80,), (80, 1200), (80,), (40, 80), (40,), (40, 40), (40,), (1, 40), (1,))


# ---------------------------------------------------------------------------------------------- DeepCpf1
def deepcpf1_f64(seqs, w):
    """The network in float64: one-hot (A, C, G, T) -> Conv1d(4, 80, k = 5) -> ReLU -> AvgPool1d(2) ->
    flatten(transpose) (index t * 80 + c) -> Linear 1200-80, ReLU, 80-40, ReLU, 40-40, ReLU, 40-1."""
    code = np.full(256, -1, dtype=np.int64)
    for i, c in enumerate("ACGT"):
        code[ord(c)] = code[ord(c.lower())] = i
    idx = code[np.frombuffer("".join(seqs).encode("ascii"), dtype=np.uint8)].reshape(len(seqs), 34)
    if (idx < 0).any():
        raise KeyError("not A, C, G or T")  # seqdeepcpf1.py:91
    p = {k: np.asarray(w[k], dtype=np.float64) for k in DC_KEYS}
    onehot = np.zeros((len(seqs), 4, 34))
    np.put_along_axis(onehot, idx[:, None, :], 1.0, axis=1)
    conv = np.zeros((len(seqs), 80, 30))
    for k in range(5):  # out[n, c, t] = b[c] + sum_{b, k} w[c, b, k] * x[n, b, t + k]
        conv += np.einsum("cb,nbt->nct", p["conv_w"][:, :, k], onehot[:, :, k:k + 30])
    conv = np.maximum(conv + p["conv_b"][None, :, None], 0.0)
    pooled = 0.5 * (conv[:, :, 0::2] + conv[:, :, 1::2])           # [n, 80, 15]
    x = pooled.transpose(0, 2, 1).reshape(len(seqs), 1200)         # flatten(transpose): t * 80 + c
    for i in (1, 2, 3):
        x = np.maximum(x @ p[f"w{i}"].T + p[f"b{i}"], 0.0)
    return (x @ p["w4"].T + p["b4"])[:, 0]


def _granule_log2(a):
    """smallest e >= 0 with every entry of a an integer multiple of 2^-e"""
    a = np.asarray(a, dtype=np.float64)
    for e in range(0, 60):
        s = a * 2.0 ** e
        if np.array_equal(s, np.round(s)):
            return e
    raise ValueError("not dyadic")


def deepcpf1_bit_budget(w):
    """Worst case over all inputs and all summation orders: per layer (bits, bound, granule exponent), where every
    partial sum of the layer is an integer multiple of 2^-granule and at most `bound` in magnitude, so that it needs
    bits = log2(bound * 2^granule) significand bits.  Any subset of a layer's terms sums to at most the sum of their
    magnitudes, so the bound holds for any order, for fused multiply-adds (one rounding of an exact value) and for
    accumulators split over wavefronts.  fp32 holds such a value exactly when bits <= 24."""
    p = {k: np.asarray(w[k], dtype=np.float64) for k in DC_KEYS}
    out = []
    g = max(_granule_log2(p["conv_w"]), _granule_log2(p["conv_b"]))
    bound = float(np.max(np.abs(p["conv_b"]) + np.abs(p["conv_w"]).max(axis=1).sum(axis=1)))  # one base per tap
    out.append(("conv", math.log2(bound) + g if bound else 0.0, bound, g))
    g += 1  # the average of a pair: half the granule, same bound
    out.append(("pool", math.log2(bound) + g if bound else 0.0, bound, g))
    for i in (1, 2, 3, 4):
        wi, bi = p[f"w{i}"], p[f"b{i}"]
        g = max(_granule_log2(wi) + g, _granule_log2(bi))
        bound = float(np.max(np.abs(bi) + np.abs(wi).sum(axis=1) * bound))
        out.append((f"fc{i}", math.log2(bound) + g if bound else 0.0, bound, g))
    return out


def _dyadic(rng, shape, den, nnz=None):
    """entries k / den with k uniform in [-den, den]; with nnz, all but nnz entries of each row are zero"""
    a = rng.integers(-den, den + 1, size=shape).astype(np.float64) / den
    if nnz is not None:
        keep = np.zeros(shape, dtype=bool)
        for r in range(shape[0]):
            keep[r, rng.choice(shape[1], size=nnz, replace=False)] = True
        a = np.where(keep, a, 0.0)
    return a.astype(np.float32)


def _signs(rng, shape, nnz, halves):
    vals = np.array([1.0, -1.0, 0.5, -0.5] if halves else [1.0, -1.0])
    a = np.zeros(shape)
    for r in range(shape[0]):
        a[r, rng.choice(shape[1], size=nnz, replace=False)] = vals[rng.integers(0, len(vals), size=nnz)]
    return a.astype(np.float32)


def deepcpf1_exact_weights(kind, seed=0):
    """Dyadic weight sets whose every partial sum fits fp32 exactly (deepcpf1_bit_budget <= 24 at every layer).

    "dense": w1 is dense.                                       granule   bound                     bits
        conv_w, conv_b  k/4, |.| <= 1; one tap per k            2^-2      1 + 5 = 6                 < 5
        pool            mean of two                             2^-3      6                         < 6
        w1, b1          k/4, |.| <= 1, all 1200 columns         2^-5      1 + 1200 * 6 = 7201       < 18
        w2  4 per row of +-1, +-1/2; b2 k/4                     2^-6      1 + 4 * 7201 = 28805      < 21
        w3  2 per row of +-1;        b3 k/4                     2^-6      1 + 2 * 28805 = 57611     < 22
        w4  4 of +-1;                b4 k/4                     2^-6      1 + 4 * 57611 = 230445    < 24
    "sparse": the later layers carry more.
        conv_w, conv_b  k/16                                    2^-4      6                         < 7
        pool                                                    2^-5      6                         < 8
        w1  48 per row of k/4; b1 k/4                           2^-7      1 + 48 * 6 = 289          < 16
        w2  8 per row of +-1, +-1/2; b2 k/4                     2^-8      1 + 8 * 289 = 2313        < 20
        w3  4 per row of +-1, +-1/2; b3 k/4                     2^-9      1 + 4 * 2313 = 9253       < 23
        w4  2 of +-1;                b4 k/4                     2^-9      1 + 2 * 9253 = 18507      < 24
    """
    rng = np.random.default_rng([77, seed, 0 if kind == "dense" else 1])
    b = lambda n: np.abs(_dyadic(rng, (n,), 4))  # biases >= 0 keep more of the ReLUs alive
    if kind == "dense":
        return dict(conv_w=_dyadic(rng, (80, 4, 5), 4), conv_b=b(80), w1=_dyadic(rng, (80, 1200), 4), b1=b(80),
                    w2=_signs(rng, (40, 80), 4, True), b2=b(40), w3=_signs(rng, (40, 40), 2, False), b3=b(40),
                    w4=_signs(rng, (1, 40), 4, False), b4=b(1))
    if kind == "sparse":
        return dict(conv_w=_dyadic(rng, (80, 4, 5), 16), conv_b=_dyadic(rng, (80,), 16), w1=_dyadic(rng, (80, 1200), 4, nnz=48), b1=b(80),
                    w2=_signs(rng, (40, 80), 8, True), b2=b(40), w3=_signs(rng, (40, 40), 4, True), b3=b(40),
                    w4=_signs(rng, (1, 40), 2, False), b4=b(1))
    raise ValueError(kind)


def deepcpf1_probe(t, c, k, base, o, o2, o3):
    """One path through the network: conv channel c answers `base` at tap k and nothing else, w1 has the single entry
    [o, t * 80 + c], one entry each in w2 [o2, o], w3 [o3, o2] and w4 [o3].  The score of a 34-mer s is then
    0.25 - 1.5 * 0.5 * 0.75 * (1/2) * ([s[2t + k] == base] + [s[2t + 1 + k] == base]): time step t, channel c and tap k
    decide it alone."""
    w = {key: np.zeros(shp, dtype=np.float32) for key, shp in zip(DC_KEYS, DC_SHAPES)}
    w["conv_w"][c, base, k] = 1.0
    w["w1"][o, t * 80 + c] = 0.75
    w["w2"][o2, o] = 0.5
    w["w3"][o3, o2] = 1.0
    w["w4"][0, o3] = -1.5
    w["b4"][0] = 0.25
    return w


def deepcpf1_probe_closed_form(seqs, t, k, base):
    hit = lambda s, j: 1.0 if "ACGT".index(s[j].upper()) == base else 0.0
    return np.array([0.25 - 1.5 * 0.5 * 0.75 * 0.5 * (hit(s, 2 * t + k) + hit(s, 2 * t + 1 + k)) for s in seqs])


def deepcpf1_probe_sweep():
    """(t, c, k, base, o, o2, o3) for every time step x every tap x every wavefront's quarter of the channels (the
    kernel gives wavefront q channels [20q, 20q + 20) of the convolution and outputs [20q, 20q + 20) of w1)"""
    out = []
    for t in range(15):
        for k in range(5):
            for q in range(4):
                i = (t * 5 + k) * 4 + q
                out.append((t, 20 * q + (i * 7) % 20, k, i % 4, (i * 13) % 80, (i * 11) % 40, (i * 17) % 40))
    return out


def deepcpf1_scaled_weights(sigma, seed=2002):
    """N(0, sigma) fp32 parameters in the layout of synth.deepcpf1_weights (sigma = 0.1 there)"""
    rng = np.random.default_rng([seed, int(round(sigma * 1e6))])
    return {k: rng.normal(0.0, sigma, size=shp).astype(np.float32) for k, shp in zip(DC_KEYS, DC_SHAPES)}


# |score| of random 34-mers: about 0.15 at sigma 0.1 (the suite's synthetic set), near 10 and near 50 (the real model's range)
DC_SCALES = (("n01", 0.1), ("near10", 0.232), ("near50", 0.345))


def deepcpf1_tolerance(oracle_f32, f64):
    """4 x the fp32 oracle's own distance from float64, floored at one fp32 ulp of the largest score"""
    f64 = np.asarray(f64, dtype=np.float64)
    ref_err = float(np.max(np.abs(np.asarray(oracle_f32, dtype=np.float64) - f64)))
    ulp = float(np.spacing(np.float32(np.max(np.abs(f64)))))
    return max(4.0 * ref_err, ulp), ref_err


def random_kmers(rng, n, k):
    return ["".join(r) for r in np.array(list("ACGT"))[rng.integers(0, 4, size=(n, k))]]


# ---------------------------------------------------------------------------------------------- trees
def gbt_eval(feats, model, cast_f32):
    """-> (sum[n], leaf[n, n_trees]): init + lr * value of the leaf each tree ends in, summed tree by tree in float64;
    leaf = node index inside its tree.  A node sends x left iff x <= threshold, x rounded to float32 first when
    cast_f32 (sklearn casts the matrix, LightGBM does not)."""
    feats = np.asarray(feats, dtype=np.float64)
    off = [int(v) for v in model["tree_off"]]
    feature, left, right = ([int(v) for v in model[k]] for k in ("feature", "left", "right"))
    thr, val = ([float(v) for v in model[k]] for k in ("threshold", "value"))
    init, lr = float(model["init"]), float(model["learning_rate"])
    n, nt = feats.shape[0], len(off) - 1
    x_all = feats.astype(np.float32).astype(np.float64) if cast_f32 else feats
    total = np.empty(n, dtype=np.float64)
    leaves = np.empty((n, nt), dtype=np.int64)
    for i in range(n):
        x = x_all[i].tolist()
        acc = init
        for t in range(nt):
            base, node = off[t], 0
            while feature[base + node] >= 0:
                node = left[base + node] if x[feature[base + node]] <= thr[base + node] else right[base + node]
            leaves[i, t] = node
            acc += lr * val[base + node]
        total[i] = acc
    return total, leaves


def gbt_sum_bound(model, leaves):
    """n_trees * 2^-52 * sum |lr * value| over the leaves taken, per row: two sequential float64 summations of the same
    n_trees terms (products rounded on their own, or fused into the addition) are each within n_trees * 2^-53 * sum |term|
    of the exact sum to first order.  `init` is no term of that sum: ensembles held to this bound have init = 0 or a
    learning rate that is a power of two (exact products, so the two orders round alike)."""
    off = np.asarray(model["tree_off"], dtype=np.int64)
    val = np.abs(float(model["learning_rate"]) * np.asarray(model["value"], dtype=np.float64))
    taken = val[off[:-1][None, :] + leaves] if leaves.shape[1] else np.zeros((leaves.shape[0], 0))
    return leaves.shape[1] * 2.0 ** -52 * taken.sum(axis=1)


def pack_model(trees, init=0.0, lr=1.0):
    """trees: lists of nodes (feature, left, right, threshold, value), child indices relative to the tree"""
    off, cols = [0], [[], [], [], [], []]
    for tr in trees:
        for node in tr:
            for col, v in zip(cols, node):
                col.append(v)
        off.append(len(cols[0]))
    f, l, r, th, v = cols
    return dict(tree_off=np.array(off, np.int32), feature=np.array(f, np.int32), left=np.array(l, np.int32), right=np.array(r, np.int32),
                threshold=np.array(th, np.float64), value=np.array(v, np.float64), init=float(init), learning_rate=float(lr))


def stump(f, thr, lo, hi):
    return [(f, 1, 2, float(thr), 0.0), (-1, 0, 0, 0.0, float(lo)), (-1, 0, 0, 0.0, float(hi))]


def leaf_tree(value):
    return [(-1, 0, 0, 0.0, float(value))]


def chain_tree(feats_thr, values, go_left):
    """A chain of len(feats_thr) splits: the chain continues on the left (go_left) or right child, the other child is
    a leaf.  Nodes 0..d-1 are the splits, d..2d the leaves (d..2d-1 beside the splits, 2d at the chain's end)."""
    d = len(feats_thr)
    nodes = []
    for j, (f, th) in enumerate(feats_thr):
        nxt, side = (j + 1 if j + 1 < d else 2 * d), d + j
        nodes.append((f, nxt, side, float(th), 0.0) if go_left else (f, side, nxt, float(th), 0.0))
    for j in range(d + 1):
        nodes.append((-1, 0, 0, 0.0, float(values[j])))
    return nodes


def bit_stump_models(specs, per_call=50):
    """specs: [(feature, threshold)] -> ensembles of at most per_call stumps whose left leaf is 0 and whose right leaf is
    2^j: with init = 0 and a learning rate of 1 the sum is an integer below 2^53, exact in float64 in any order, and bit j
    of it says which way stump j went."""
    out = []
    for s in range(0, len(specs), per_call):
        part = specs[s:s + per_call]
        out.append((part, pack_model([stump(f, th, 0.0, 2.0 ** j) for j, (f, th) in enumerate(part)], 0.0, 1.0)))
    return out


def bits_of(leaves):
    """the exact sum a bit-stump ensemble must give, from gbt_eval's leaves (node 2 = right)"""
    return ((leaves == 2) * (2.0 ** np.arange(leaves.shape[1]))[None, :]).sum(axis=1)


def f32_next(v, up):
    return float(np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf)))


def f32_boundary_distance(v):
    """distance of the float64 v from the nearest point where its float32 rounding changes"""
    v = np.asarray(v, dtype=np.float64)
    f = v.astype(np.float32)
    lo = (f.astype(np.float64) + np.nextafter(f, np.float32(-np.inf)).astype(np.float64)) / 2
    hi = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2
    return np.minimum(np.abs(v - lo), np.abs(v - hi))


TM_BAND = 2e-9       # twice the 1e-9 the suite holds the device's Tm to
TM_LEFT_OUT_CAP = 0.02
TM_WINDOWS = ((0, 30), (19, 24), (11, 19), (6, 11))  # columns 623..626 (featurization.py:358-397)


# ---------------------------------------------------------------------------------------------- 30-mers at the extremes
def _fill(rng, n, letters):
    return "".join(letters[i] for i in rng.integers(0, len(letters), size=n))


def azimuth_homopolymers():
    return [b * 30 for b in "ACGT"]


def azimuth_dinucleotide_repeats():
    """(XY)^15 and Y(XY)^14 X for the sixteen ordered pairs"""
    out = []
    for x in "ATCG":
        for y in "ATCG":
            out += [(x + y) * 15, y + (x + y) * 14 + x]
    return out


def azimuth_gc_window_cases(rng):
    """[(30-mer, GC count of s[4:24])]: counts 0, 9, 10, 11, 20 with the GC bases at the window's left end, at its right
    end or spread; the flank s[0:4] is of the class s[23] is not and s[24:30] of the class s[4] is not, so a window
    shifted by one base to either side counts differently"""
    out = []
    for gc in (0, 9, 10, 11, 20):
        for layout in ("left", "right", "spread", "spread"):
            is_gc = np.zeros(20, dtype=bool)
            if layout == "left":
                is_gc[:gc] = True
            elif layout == "right":
                is_gc[20 - gc:] = True
            else:
                is_gc[rng.choice(20, size=gc, replace=False)] = True
            win = "".join(_fill(rng, 1, "CG") if g else _fill(rng, 1, "AT") for g in is_gc)
            out.append((_fill(rng, 4, "AT" if is_gc[19] else "CG") + win + _fill(rng, 6, "AT" if is_gc[0] else "CG"), gc))
    return out


def azimuth_nggx_cases(rng):
    """every (s[24], s[27]) pair under every s[25:27]"""
    out = []
    for a in "ATCG":
        for b in "ATCG":
            for m in (x + y for x in "ATCG" for y in "ATCG"):
                out.append(_fill(rng, 24, "ACGT") + a + m + b + _fill(rng, 2, "ACGT"))
    return out


_SWAP = {"A": "G", "G": "A", "C": "T", "T": "C"}  # changes the base's class too: the end terms of Tm_NN move with it


def azimuth_tm_window_pairs(rng, n_base=6):
    """[(column, base 30-mer, changed 30-mer, inside)]: one base changed just outside and just inside each end of each Tm
    window"""
    out = []
    for _ in range(n_base):
        s = _fill(rng, 30, "ACGT")
        for col, (lo, hi) in enumerate(TM_WINDOWS):
            for pos, inside in ((lo - 1, False), (lo, True), (hi - 1, True), (hi, False)):
                if 0 <= pos < 30:
                    out.append((623 + col, s, s[:pos] + _SWAP[s[pos]] + s[pos + 1:], inside))
    return out


def azimuth_extreme_batch(seed=41, n_random=400):
    """the batch the feature and stump tests run on: every extreme above plus random 30-mers"""
    rng = np.random.default_rng(seed)
    seqs = azimuth_homopolymers() + azimuth_dinucleotide_repeats()
    seqs += [s for s, _ in azimuth_gc_window_cases(rng)] + azimuth_nggx_cases(rng)
    for _, a, b, _ in azimuth_tm_window_pairs(rng):
        seqs += [a, b]
    seqs += random_kmers(rng, n_random, 30)
    return seqs


def azimuth_stump_specs(feats):
    """For every one of the 627 columns: thresholds at a value the column takes on the batch (its upper median and its
    maximum), the next float32 below and the next above.  Columns 623..626 use float32(Tm), the value the kernel's cast
    makes of them, and add thresholds strictly between Tm and float32(Tm), where only the cast decides.
    -> {column: [(column, threshold)]}"""
    specs = {}
    for f in range(627):
        col = feats[:, f]
        vals = sorted({float(np.float32(np.sort(col)[len(col) // 2])), float(np.float32(col.max()))})
        th = []
        for v in vals:
            th += [v, f32_next(v, False), f32_next(v, True)]
        if f >= 623:
            order = np.argsort(-np.abs(col - col.astype(np.float32)))  # the rows whose cast moves them furthest
            for i in order[:6]:
                th.append((float(col[i]) + float(np.float32(col[i]))) / 2)
        specs[f] = [(f, t) for t in th]
    return specs


# ---------------------------------------------------------------------------------------------- tree shapes
def shape_ensembles(rng, nfeat=623):
    """{name: model}: the shapes a flattener can hand over.  Splits use columns below `nfeat` with thresholds k + 0.5 or
    0.5, so the features of the CPU oracle decide them the way the device's do."""
    def split():
        f = int(rng.integers(0, nfeat))
        counts = f in (606,) or 120 <= f < 124 or 588 <= f < 604
        return f, (float(rng.integers(0, 12)) + 0.5 if counts else 0.5)

    def split_right():  # counts with low thresholds: most 30-mers go right
        f = int(rng.choice([120, 121, 122, 123, 606, 588, 593, 598, 603]))
        return f, float(rng.integers(3, 7) if f < 124 else (rng.integers(6, 10) if f == 606 else 0)) + 0.5

    def rand_tree():
        kind = int(rng.integers(0, 4))
        if kind == 0:
            return leaf_tree(rng.normal())
        if kind == 1:
            return stump(*split(), rng.normal(), rng.normal())
        d = int(rng.integers(2, 9))
        return chain_tree([split() if kind == 2 else split_right() for _ in range(d)], rng.normal(size=d + 1), go_left=(kind == 2))

    out = {}
    out["no_trees"] = pack_model([], init=0.37, lr=0.1)
    out["one_leaf"] = pack_model([leaf_tree(1.25)], init=0.37, lr=0.5)
    out["one_stump"] = pack_model([stump(606, 9.5, -3.0, 7.0)], init=0.0, lr=0.1)
    out["leaves_only"] = pack_model([leaf_tree(v) for v in rng.normal(size=40)], init=0.0, lr=0.1)
    out["left_chain_12"] = pack_model([chain_tree([split() for _ in range(12)], rng.normal(size=13), True)], init=0.0, lr=0.1)
    out["right_chain_12"] = pack_model([chain_tree([split_right() for _ in range(12)], rng.normal(size=13), False)], init=0.0, lr=0.1)
    out["mixed_60"] = pack_model([rand_tree() for _ in range(60)], init=0.0, lr=0.1)
    out["mixed_1000"] = pack_model([rand_tree() for _ in range(1000)], init=0.0, lr=0.1)
    mags = 10.0 ** np.arange(-8, 9)
    out["leaf_1e-8_to_1e8"] = pack_model([stump(*split(), -m, m * 1.7) for m in mags] + [leaf_tree(m) for m in mags[::4]], init=0.0, lr=0.1)
    return out


def broken_models(n_features):
    """[(what is wrong, model)] every one of which the entry point must refuse before anything is launched"""
    good = [stump(0, 0.5, 1.0, 2.0), chain_tree([(1, 0.5), (2, 0.5)], [1.0, 2.0, 3.0], True)]

    def edit(tree, node, **kw):
        trees = [list(t) for t in good]
        f, l, r, th, v = trees[tree][node]
        d = dict(f=f, l=l, r=r)
        d.update(kw)
        trees[tree][node] = (d["f"], d["l"], d["r"], th, v)
        return pack_model(trees)

    out = [("left child points backwards", edit(1, 1, l=0)),
           ("right child points at itself", edit(1, 1, r=1)),
           ("left child points at itself (root)", edit(0, 0, l=0)),
           ("child outside the tree", edit(0, 0, r=3)),
           ("child far outside the tree", edit(1, 0, l=1 << 20)),
           ("negative child", edit(1, 0, r=-1)),
           (f"feature {n_features}", edit(0, 0, f=n_features)),
           ("feature far out of range", edit(1, 1, f=1 << 30))]
    m = pack_model(good)
    m["tree_off"] = np.array([0, 3, 3], np.int32)
    out.append(("tree_off not increasing", m))
    m = pack_model(good)
    m["tree_off"] = np.array([0, 5, 3], np.int32)
    out.append(("tree_off decreasing", m))
    m = pack_model(good)
    m["tree_off"] = np.array([0, 3, 9], np.int32)
    out.append(("last offset beyond n_nodes", m))
    m = pack_model(good)
    m["tree_off"] = np.array([-1, 3, 8], np.int32)
    out.append(("negative first offset", m))
    return out


# ---------------------------------------------------------------------------------------------- k_gbt
GBT_HARD_VALUES = (1.0 / 3.0, 0.1, 16777217.0, 1e-50, -1.0 / 3.0, -16777217.0, -1e-50)  # none is a float32


def gbt_cast_cases(n, nf, first):
    """A matrix [n, nf] whose deciding column (the first or the last) cycles through values float32 cannot hold, +-0, +-inf
    and plain ones, the other columns filled with values that would decide otherwise; and the stump specs on that column:
    thresholds at x, at float32(x), strictly between the two, at 0 for the zeros, and at the largest finite double."""
    f = 0 if first else nf - 1
    vals = list(GBT_HARD_VALUES) + [0.0, -0.0, np.inf, -np.inf, 1.0, -2.5, 3.0e38, 1e39]
    x = np.full((n, nf), 12345.0)
    if nf > 1:
        x[:, (nf - 1 if first else 0)] = -12345.0
    x[:, f] = [vals[i % len(vals)] for i in range(n)]
    th = [0.0, -0.0, 1.0, np.finfo(np.float64).max, -np.finfo(np.float64).max]
    for v in GBT_HARD_VALUES:
        v32 = float(np.float32(v))
        th += [v, v32, (v + v32) / 2]
    return x, [(f, t) for t in th]


# ---------------------------------------------------------------------------------------------- CFD
def cfd_edges():
    from util import load_golden
    return load_golden("g5_cfd_edges.json.gz")
