#!/usr/bin/env python3
"""Generate tests/golden/g15_plmcrispr.json.gz by running the REFERENCE's own PLM-CRISPR network.

    python tests/golden/make_golden_plmcrispr.py <reference>/src

The published checkpoint (100.pt) and the ESM embeddings are downloads this project does not have, so - as G6 does for
DeepCpf1 - the reference's module (scores/plm_crispr/train_general.py: sgrna_net, with Protein.py: TextCNN) is loaded by
path, given the seeded parameters of synth.plmcrispr_weights / synth.plmcrispr_protein and run with the torch that is
installed, through the wrapper's own input functions (plm_crispr.py: _build_input_sequences, _encode_sequences) and in its
batches of 64.  Stored: the seeds, L, 512 guide+PAM 23-mers, their fp32 scores, the protein branch's 256 values and the inputs
the wrapper refuses with the exception class each raises.  The parameters are NOT stored: both sides rebuild them from the seed.

Condition: the scores have a standard deviation >= 0.05 and lie in (0.02, 0.98) - otherwise change the seed, not the test."""
import gzip
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "crispr-hawk_amd"))
from crisprhawk_hip import synth  # noqa: E402

SEED, L, N = 2003, 64, 512


def load_reference(src):
    """train_general.py imports `.Protein` relatively: give the directory a package name of its own (its __init__ is not run)"""
    pkg = types.ModuleType("ref_plm")
    pkg.__path__ = [os.path.join(src, "crisprhawk", "scores", "plm_crispr")]
    sys.modules["ref_plm"] = pkg
    return importlib.import_module("ref_plm.train_general"), importlib.import_module("ref_plm.plm_crispr")


def guides(rng):
    out = ["".join(r) for r in np.array(list("ACGT"))[rng.integers(0, 4, size=(N, 23))]]
    for i in rng.choice(N, 30, replace=False):  # ~30 with one to three N
        s = list(out[i])
        for p in rng.choice(23, int(rng.integers(1, 4)), replace=False):
            s[p] = "N"
        out[i] = "".join(s)
    for k, i in enumerate(rng.choice(N, 30, replace=False)):  # ~30 lower or mixed case
        out[i] = out[i].lower() if k % 2 == 0 else "".join(c.lower() if rng.random() < 0.5 else c for c in out[i])
    out[0] = "N" * 23
    out[1] = "A" * 23
    out[2] = "G" * 23
    return out


def main():
    R_net, R_wrap = load_reference(sys.argv[1])
    torch.manual_seed(0)
    torch.set_num_threads(8)
    params = synth.plmcrispr_weights(SEED)
    protein = synth.plmcrispr_protein(SEED, L)
    net = R_net.sgrna_net()
    missing = net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    assert [k for k in net.state_dict()] == [k for k, _ in synth.PLMCRISPR_SHAPES]
    net.eval()
    emb = torch.from_numpy(protein).to(torch.float16)  # plm_crispr.py:133
    seqs = guides(np.random.default_rng(SEED))
    enc = R_wrap._encode_sequences(R_wrap._build_input_sequences(seqs)).long()
    scores = []
    with torch.no_grad():
        for lo in range(0, N, R_wrap.BATCH_SIZE):  # compute_plm_crispr_score's loop, plm_crispr.py:225-238
            b = enc[lo:lo + R_wrap.BATCH_SIZE]
            scores.extend(net(b, 0, emb.unsqueeze(0).repeat(len(b), 1, 1), train=False).view(-1).tolist())
        feat = net.text_cnn(emb.unsqueeze(0))
        prot = torch.sigmoid(torch.nn.functional.relu(net.lin4(feat.float())))[0].tolist()
    scores = np.array(scores, dtype=np.float32)
    print(f"scores: std {scores.std():.4f}, range {scores.min():.4f} .. {scores.max():.4f}")
    assert scores.std() >= 0.05 and scores.min() > 0.02 and scores.max() < 0.98, "change the seed"
    good = "ACGTACGTACGTACGTACGTAGG"
    refused = []
    for s in (good[:22], good + "A", "", good * 2, "R" + good[1:], good[:11] + "U" + good[12:], good[:22] + "-", good[:5] + "r" + good[6:],
              good[:22] + "Y", "u" + good[1:], good[:10] + " " + good[11:], good[:22] + "*"):
        try:
            R_wrap._encode_sequences(R_wrap._build_input_sequences([s]))
        except Exception as e:  # noqa: BLE001
            refused.append([s, type(e).__name__])
        else:
            raise AssertionError(f"the reference accepts {s!r}")
    obj = dict(seed=SEED, L=L, guides=seqs, scores=[float(x) for x in scores], protein=[float(np.float32(x)) for x in prot],
               refused=refused, torch=torch.__version__)
    path = os.path.join(HERE, "g15_plmcrispr.json.gz")
    raw = json.dumps(obj, separators=(",", ":")).encode()
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(raw)
    print(f"g15_plmcrispr.json.gz: {len(raw)} B json -> {os.path.getsize(path)} B gz; refused: {refused}")


if __name__ == "__main__":
    main()
