"""Plain numpy statements of PLM-CRISPR's forward pass (the reference's scores/plm_crispr/train_general.py:53-131 with
train=False, behind the wrapper scores/plm_crispr/plm_crispr.py:136-258), in float64 and in float32, and the tolerance rule
the device kernels are held to.  Parameters are a dict by state_dict name in torch layout (synth.PLMCRISPR_SHAPES)."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

SCAFFOLD = ("gtttCagagctaTGCTGgaaaCAGCAtagcaagttGaaataaggctagtcc" "gttatcaacttgaaaaagtggcaccgagtcggtgcttt")[:36].upper()
CODES = {nt: i for i, nt in enumerate("ATCGN")}


def encode(seqs):
    """(n, 59) codes; ValueError for a length other than 59 with the scaffold, KeyError for a symbol outside A T C G N"""
    rows = []
    for g in seqs:
        s = (g + SCAFFOLD).upper()
        if len(s) != 59:
            raise ValueError(f"PLM-CRISPR input sequence has length {len(s)}, expected 59")
        rows.append([CODES[ch] for ch in s])
    return np.array(rows, dtype=np.int64).reshape(len(rows), 59)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _conv_same(x, w, b):
    """Conv1d(kernel 5, padding 2): x (n, C, 59), w (O, C, 5) -> (n, O, 59)"""
    n, c, p = x.shape
    xp = np.zeros((n, c, p + 4), dtype=x.dtype)
    xp[:, :, 2:-2] = x
    win = sliding_window_view(xp, 5, axis=2)  # (n, C, 59, 5)
    cols = np.ascontiguousarray(win.transpose(0, 2, 1, 3)).reshape(n * p, c * 5)
    out = cols @ w.reshape(w.shape[0], -1).T + b
    return out.reshape(n, p, -1).transpose(0, 2, 1)


def _pooled(params, protein, dt):
    """the 384 max-pooled relu'd text_cnn outputs, [kernel 5 | kernel 9 | kernel 13] x 128 channels"""
    emb = np.asarray(protein, dtype=np.float32).astype(np.float16).astype(dt)  # plm_crispr.py:133
    feats = []
    for i, ks in enumerate((5, 9, 13)):
        w = params[f"text_cnn.convs.{i}.weight"].astype(dt)
        b = params[f"text_cnn.convs.{i}.bias"].astype(dt)
        win = sliding_window_view(emb, ks, axis=0)  # (P, 1280, ks)
        y = win.reshape(win.shape[0], -1) @ w.reshape(128, -1).T + b
        feats.append(np.maximum(y, 0).max(axis=0))
    return np.concatenate(feats)


def protein_head(pooled, params, dt):
    """sigmoid(relu(lin4(pooled)))"""
    y = params["lin4.weight"].astype(dt) @ pooled + params["lin4.bias"].astype(dt)
    return _sigmoid(np.maximum(y, 0)).astype(dt)


def _protein(params, protein, dt):
    return protein_head(_pooled(params, protein, dt), params, dt)


def _cast(params, dt):
    return {k: np.asarray(v).astype(dt) for k, v in params.items() if not k.startswith("text_cnn")}


def _features(cd, P, dt):
    n = len(cd)
    onehot = np.zeros((n, 59, 5), dtype=dt)
    onehot[np.arange(n)[:, None], np.arange(59)[None, :], cd] = 1
    x = onehot.reshape(n, 5, 59)  # .view(-1, 5, 59): a reshape, NOT a transpose (train_general.py:75)
    be = _conv_same(x, P["conv4.weight"], P["conv4.bias"])
    y = _sigmoid(_conv_same(x, P["conv1.weight"], P["conv1.bias"]))
    y = _sigmoid(_conv_same(y, P["conv2.weight"], P["conv2.bias"]))
    y = _sigmoid(_conv_same(y, P["conv3.weight"], P["conv3.bias"]))
    return np.concatenate([y.reshape(n, -1), be.reshape(n, -1)], axis=1)  # each branch channel-major


def _lin1(feat, P):
    return _sigmoid(feat @ P["lin1.weight"].T + P["lin1.bias"])


def _lin3(h1, P):
    return h1 @ P["lin3.weight"].T + P["lin3.bias"]


def _tail(sg, prot, P):
    n = len(sg)
    comb = np.concatenate([sg, np.broadcast_to(prot, (n, 256))], axis=1)
    hid = np.maximum(comb @ P["weight_net.0.weight"].T + P["weight_net.0.bias"], 0)
    lg = hid @ P["weight_net.2.weight"].T + P["weight_net.2.bias"]
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    wts = e / e.sum(axis=1, keepdims=True)
    mix = wts[:, :1] * sg + wts[:, 1:] * prot
    z = _sigmoid(mix @ P["lin5.weight"].T + P["lin5.bias"])
    return _sigmoid(z @ P["lin6.weight"].T + P["lin6.bias"])[:, 0]


def plm_layers(seqs, params, protein, dt, chunk=256):
    """Every layer of the forward pass: feat (n, 7552), h1 (n, 2048) = sigmoid(lin1), sg (n, 256) = out_sgrna, prot (256) =
    out_protein, pooled (384) = the text_cnn maxima, score (n).  The guides are evaluated `chunk` at a time."""
    P = _cast(params, dt)
    pooled = _pooled(params, protein, dt)
    prot = protein_head(pooled, params, dt)
    codes = encode(seqs)
    n = len(codes)
    out = {"feat": np.empty((n, 7552), dtype=dt), "h1": np.empty((n, 2048), dtype=dt), "sg": np.empty((n, 256), dtype=dt),
           "prot": prot, "pooled": pooled, "score": np.empty(n, dtype=dt)}
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        out["feat"][lo:hi] = feat = _features(codes[lo:hi], P, dt)
        out["h1"][lo:hi] = h1 = _lin1(feat, P)
        out["sg"][lo:hi] = sg = _lin3(h1, P)
        out["score"][lo:hi] = _tail(sg, prot, P)
    return out


def plm_resume(layer, value, params, prot, dt=np.float64):
    """the scores that follow from `value` standing for the intermediate `layer` ("feat", "h1" or "sg"): what a mistake in that
    layer does to the score.  prot is out_protein (plm_layers(...)["prot"])."""
    P = _cast(params, dt)
    value = np.asarray(value, dtype=dt)
    if layer == "feat":
        value, layer = _lin1(value, P), "h1"
    if layer == "h1":
        value, layer = _lin3(value, P), "sg"
    if layer != "sg":
        raise ValueError(layer)
    return _tail(value, np.asarray(prot, dtype=dt), P)


def _forward(seqs, params, protein, dt, chunk=256):
    return plm_layers(seqs, params, protein, dt, chunk)["score"]


def plm_f64(seqs, params, protein):
    return _forward(seqs, params, protein, np.float64)


def plm_f32(seqs, params, protein):
    return _forward(seqs, params, protein, np.float32)


def protein_f64(params, protein):
    """out_protein: sigmoid(relu(lin4(text_cnn(embedding)))), 256 values"""
    return _protein(params, protein, np.float64)


def protein_f32(params, protein):
    return _protein(params, protein, np.float32)


def plm_tolerance(f32_scores, f64_scores):
    """4 x the largest distance of the fp32 scores from float64, floored at one fp32 ulp of the largest score (the rule
    scorer_refs.deepcpf1_tolerance sets for DeepCpf1); returns (tolerance, that distance)"""
    f64 = np.asarray(f64_scores, dtype=np.float64)
    ref_err = float(np.max(np.abs(np.asarray(f32_scores, dtype=np.float64) - f64)))
    ulp = float(np.spacing(np.float32(np.max(np.abs(f64)))))
    return max(4.0 * ref_err, ulp), ref_err
