"""Parameter sets ("lenses") under which PLM-CRISPR's score, or its out_protein vector, is a well-conditioned function of one
intermediate layer.  Under the seeded dense parameters (g15) the softmax weight on the sgRNA branch has median 6e-4, 116-121
of the 256 lin4 pre-activations are relu'd to a constant and the max-pool hides every position but a channel's argmax, so a
score within plm_tolerance says little about lin1's tiles or the convolutions' edges.  Every set here is a function of a
seed and the g15 parameters; tests/test_plm_lens.py holds each to its condition without a device.

  head_lens      the softmax mix is out_sgrna itself; lin5 reads every sg unit once: observes the GEMM pair as shipped
  route_lens     + lin3 with one nonzero per column: every lin1 output reaches the score through its own gain
  kslice_lens    + lin1 nonzero only in one stretch of K: a flush period, the branch seam, the last LDS stage
  feature_lens   + lin1 with one nonzero per column: every one of the 7552 features reaches the score (in FEATURE_SETS)
  protein_lens   lin4 sparse and positive, an embedding whose argmax position is forced: observes the text_cnn pooling"""
import functools

import numpy as np

import plm_refs

PERTURBATION = 2.0 ** -10  # the single-element error a sgrna-branch lens must show in every row's score

# [lo, hi) of K and the factor on g15's lin1 weights inside it.  PLM_TK x PLM_FLUSH = 128 is one flush period, PLM_TK = 32 one stage
K_SLICES = {"first": (0, 128, 2.0), "second": (128, 256, 2.0), "seam": (3712, 3840, 2.0), "last": (7424, 7552, 2.0),
            "stage": (7520, 7552, 4.0)}


def _centred(p, seed, at, spread=None):
    """The bias of lin5 (at = "lin5.bias") or of lin3 such that lin5's pre-activations, or out_sgrna, have mean 0 over 64 seeded
    guides.  The means of out_sgrna's units are 1.7 apart under g15 while a unit moves by 0.6 from guide to guide; uncentred,
    some lin5 units sit at |z| = 2 for every guide.  Where lin3 is the lens's own its bias does it, so that lin5 does not have
    to cancel two large numbers in fp32.  With `spread`, lin6 is then scaled so that the final pre-activation has that standard
    deviation over the same guides (a factor within 1/2 .. 4): how much of the score's range a set's features take is chance."""
    rng = np.random.default_rng([seed, 0])
    seqs = ["".join(r) for r in np.array(list("ACGT"))[rng.integers(0, 4, size=(64, 23))]]
    p["lin5.bias"] = np.zeros(128, np.float32)
    if at == "lin3.bias":
        p[at] = np.zeros(256, np.float32)
    P = plm_refs._cast(p, np.float32)
    sg = plm_refs._lin3(plm_refs._lin1(plm_refs._features(plm_refs.encode(seqs), P, np.float32), P), P)
    mean = sg.astype(np.float64).mean(axis=0)
    if at == "lin5.bias":
        mean = mean @ p["lin5.weight"].astype(np.float64).T
    p[at] = (-np.round(mean * 64) / 64).astype(np.float32)  # a coarse grid: the last bits of a BLAS sum do not matter
    if spread is not None:
        z = (sg.astype(np.float64) + p["lin3.bias"]) @ p["lin5.weight"].astype(np.float64).T + p["lin5.bias"]
        t = plm_refs._sigmoid(z) @ p["lin6.weight"][0].astype(np.float64)
        p["lin6.weight"] = p["lin6.weight"] * np.float32(np.round(np.clip(spread / t.std(), 0.5, 4.0) * 16) / 16)
    return p


def head_lens(seed, g15, centre=True):
    """weight_net gives the logits (+60, -60) whatever its input: w0 = 1 and mix = out_sgrna in fp32.  lin5's unit u reads two
    sg units with gains 0.25 and -0.22, every sg unit read once; lin6 is +-m in pairs (sum 0), m in [0.7, 0.8], shuffled."""
    rng = np.random.default_rng([seed, 1])
    p = dict(g15)
    p["weight_net.0.weight"] = np.zeros((128, 512), np.float32)
    p["weight_net.0.bias"] = np.zeros(128, np.float32)
    p["weight_net.2.weight"] = np.zeros((2, 128), np.float32)
    p["weight_net.2.bias"] = np.array([60.0, -60.0], np.float32)
    perm = rng.permutation(256)
    w5 = np.zeros((128, 256), np.float32)
    w5[np.arange(128), perm[:128]] = 0.25
    w5[np.arange(128), perm[128:]] = -0.22
    p["lin5.weight"] = w5
    m = rng.uniform(0.7, 0.8, size=64)
    p["lin6.weight"] = rng.permutation(np.concatenate([m, -m])).astype(np.float32).reshape(1, 128)
    return _centred(p, seed, "lin5.bias") if centre else p


def route_lens(seed, g15, centre=True):
    """the head lens, and lin1 unit u feeds sg unit u % 256 alone: the eight units of an sg unit lie in eight different N
    tiles and have the gains +-(1.2 .. 1.55) in a seeded order, four of either sign"""
    rng = np.random.default_rng([seed, 2])
    p = head_lens(seed, g15, False)
    gains = np.linspace(1.2, 1.55, 8) * np.array([1, -1, 1, -1, -1, 1, -1, 1])
    w3 = np.zeros((256, 2048), np.float32)
    for s in range(256):
        w3[s, s + 256 * np.arange(8)] = rng.permutation(gains)
    p["lin3.weight"] = w3
    return _centred(p, seed, "lin3.bias") if centre else p


def kslice_lens(seed, g15, which):
    """the route lens with g15's lin1 weights kept (times a factor) for K_SLICES[which] and zero elsewhere"""
    lo, hi, gain = K_SLICES[which]
    p = route_lens(seed, g15, False)
    w1 = np.zeros((2048, 7552), np.float32)
    w1[:, lo:hi] = g15["lin1.weight"][:, lo:hi] * np.float32(gain)
    p["lin1.weight"] = w1
    return _centred(p, seed, "lin3.bias")


def feature_unit(e):
    """the lin1 unit that reads feature e under the feature lens: 1408 units read four features, 640 read three"""
    return e % 2048


# [lo, hi) of the features a set observes, the magnitude of their lin1 gains and the factor on the route lens's lin3: the first
# branch (sigmoids, in (0, 1)) in two sets, conv4's branch (which reaches +-6) four channels to a set
FEATURE_SETS = [(0, 2048, 1.8, 8.0), (2048, 3776, 1.8, 8.0)] + [(3776 + 236 * k, 4012 + 236 * k, 0.22, 11.0) for k in range(16)]


def feature_lens(seed, g15, part):
    """The route lens with lin1 sparse: feature e is read by unit e % 2048 alone, so over the sets every feature is read by
    exactly one unit and a unit reads at most four.  One set observes the features FEATURE_SETS[part]: a unit's pre-activation
    is one gain times one feature and stays on the straight part of the sigmoid; the units that read nothing in this set have
    the bias -40 and give 0, so out_sgrna is a short sum.  The score is one number: a row's score shares its range among the
    observed features, and 2^-10 is 1 / 12000 of conv4's range, so that branch needs the narrow sets."""
    lo, hi, g1, g3 = FEATURE_SETS[part]
    rng = np.random.default_rng([seed, 3, part])
    p = route_lens(seed, g15, False)
    e = np.arange(lo, hi)
    # the sign of d score / d feature alternates along a channel: a homopolymer's equal features cancel instead of piling up
    u, s = feature_unit(e), feature_unit(e) % 256
    v = np.argmax(p["lin5.weight"][:, s] != 0, axis=0)
    path = np.sign(p["lin3.weight"][s, u] * p["lin5.weight"][v, s] * p["lin6.weight"][0, v])
    gain = rng.uniform(0.9 * g1, 1.1 * g1, size=len(e)) * path * np.where(e % 2, -1.0, 1.0)
    w1 = np.zeros((2048, 7552), np.float32)
    w1[feature_unit(e), e] = gain
    b1 = np.full(2048, -40.0, np.float32)
    b1[feature_unit(e)] = np.where(e < 3776, -0.5 * gain, 0.0)  # the first branch's features centre on 0.5
    p["lin1.weight"], p["lin1.bias"] = w1, b1
    p["lin3.weight"] = p["lin3.weight"] * np.float32(g3)
    return _centred(p, seed, "lin3.bias", spread=0.5)


def observed_features(part):
    return np.arange(*FEATURE_SETS[part][:2])


# ------------------------------------------------------------------------------------------------------------ protein branch
KERNELS = (5, 9, 13)
DEAD_CHANNELS = 6  # per convolution: bias -50, pooled value exactly +0


def forced_positions(L, conv):
    """0, 15, 16 (either side of a PLM_PROT_P = 16 tile edge) and the last position, where the convolution has them"""
    P = L - KERNELS[conv] + 1
    return sorted({q for q in (0, 15, 16, P - 1) if 0 <= q < P})


def protein_lens(seed, g15, L, conv, pos, amplitude=0.2, noise=0.05):
    """(params, embedding): position `pos` of convolution `conv` is the argmax of every live channel of it, and out_protein sees
    every pooled feature.  The embedding is N(0, noise^2) plus, in rows pos .. pos + ks - 1, amplitude x the sum of that
    convolution's 128 filters (each filter answers it with amplitude x |filter|^2, about 9 x amplitude; a shifted window or
    another filter bank sees it as noise), rounded through fp16.  DEAD_CHANNELS channels of each convolution get the bias -50.
    lin4's unit v reads pooled feature v, and 256 + v for v < 128, with gain c / max(the float64 pooled value, 0.25), c in
    [0.3, 0.6]: a feature adds at most c; the bias is 0.1 + |g15's|, so every pre-activation lies in (0.1, 1.8)."""
    rng = np.random.default_rng([seed, 4, L, conv, pos])
    ks = KERNELS[conv]
    p = dict(g15)
    emb = rng.normal(0.0, noise, size=(L, 1280))
    w = g15[f"text_cnn.convs.{conv}.weight"].astype(np.float64)  # (128, 1280, ks)
    emb[pos:pos + ks] += amplitude * w.sum(axis=0).T
    emb = emb.astype(np.float16).astype(np.float32)
    for i in range(3):
        b = g15[f"text_cnn.convs.{i}.bias"].copy()
        b[rng.choice(128, size=DEAD_CHANNELS, replace=False)] = -50.0
        p[f"text_cnn.convs.{i}.bias"] = b
    pooled = plm_refs._pooled(p, emb, np.float64)
    c = rng.uniform(0.3, 0.6, size=384)
    gain = c / np.maximum(pooled, 0.25)
    w4 = np.zeros((256, 384), np.float32)
    w4[np.arange(256), np.arange(256)] = gain[:256]
    w4[np.arange(128), 256 + np.arange(128)] = gain[256:]
    p["lin4.weight"] = w4
    p["lin4.bias"] = (0.1 + np.abs(g15["lin4.bias"])).astype(np.float32)
    return p, emb


def conv_outputs(params, emb, conv, dt):
    """(P, 128): convolution `conv` of the text_cnn before relu and pooling"""
    ks = KERNELS[conv]
    e = np.asarray(emb, np.float32).astype(np.float16).astype(dt)
    win = np.lib.stride_tricks.sliding_window_view(e, ks, axis=0)
    return win.reshape(win.shape[0], -1) @ params[f"text_cnn.convs.{conv}.weight"].astype(dt).reshape(128, -1).T \
        + params[f"text_cnn.convs.{conv}.bias"].astype(dt)


# ------------------------------------------------------------------------------------------------------------------- guides
def pool_guides():
    """the 300 guides of tests/test_gpu_plmcrispr.py's pool (N and mixed case among them)"""
    rng = np.random.default_rng(15)
    return ["".join(r) for r in np.array(list("ACGTNacgtn"))[rng.choice(10, size=(300, 23), p=[.21, .21, .21, .21, .02, .03, .03, .03, .03, .02])]]


def seam_guides():
    """129 guides: the 24 x 5 last-base sets of test_scaffold_positions, the five homopolymers, N at positions 0 and 22, lower case"""
    rng = np.random.default_rng(16)
    base = ["".join(r) for r in np.array(list("ACGT"))[rng.integers(0, 4, size=(24, 22))]]
    flat = [b + last for last in "ACGTN" for b in base]
    flat += ["N" * 23, "A" * 23, "C" * 23, "G" * 23, "T" * 23]
    flat += ["N" + base[0][1:] + "G", base[1] + "N", (base[2] + "g").lower(), "n" + base[3][1:].lower() + "n"]
    assert len(flat) == 129
    return flat


# --------------------------------------------------------------------------------------------------------------- references
SEED = 15
SGRNA_LENSES = ["head", "route"] + [f"k:{k}" for k in K_SLICES] + [f"feature:{i}" for i in range(len(FEATURE_SETS))]


@functools.lru_cache(maxsize=None)
def g15():
    """the seeded dense parameters and embedding of tests/golden/g15_plmcrispr.json.gz"""
    from crisprhawk_hip import synth
    from util import load_golden
    fx = load_golden("g15_plmcrispr.json.gz")
    return synth.plmcrispr_weights(fx["seed"]), synth.plmcrispr_protein(fx["seed"], fx["L"])


def lens(name):
    """the parameters of a sgrna-branch lens by name; not cached (a set with its own lin1 is 62 MB)"""
    params = g15()[0]
    kind, _, arg = name.partition(":")
    if kind == "head":
        return head_lens(SEED, params)
    if kind == "route":
        return route_lens(SEED, params)
    if kind == "k":
        return kslice_lens(SEED, params, arg)
    if kind == "feature":
        return feature_lens(SEED, params, int(arg))
    raise KeyError(name)


def lens_guides(name):
    """the rows a lens is used with on the device: the pool for the head lens, its first 257 for the route lens, else seam_guides"""
    return pool_guides() if name == "head" else pool_guides()[:257] if name == "route" else seam_guides()


_REFERENCES = {}


def reference(name, params=None):
    """(guides, float64 scores, numpy-fp32 scores) of a lens on its rows: computed once, read-only.  `params` spares building
    the lens again where the caller holds it."""
    if name not in _REFERENCES:
        seqs, params, protein = lens_guides(name), lens(name) if params is None else params, g15()[1]
        f64, f32 = plm_refs.plm_f64(seqs, params, protein), plm_refs.plm_f32(seqs, params, protein)
        f64.setflags(write=False)
        f32.setflags(write=False)
        _REFERENCES[name] = (seqs, f64, f32)
    return _REFERENCES[name]
