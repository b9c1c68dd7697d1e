#!/usr/bin/env python3
"""One-off converter, run by the user on the machine that holds the reference's downloaded scoring models
(`crisprhawk` fetches them from Zenodo at run time, config_utils.py:34-70; that machine has scikit-learn / h5py /
lightgbm because the reference needs them).  Writes dependency-free files crisprhawk_hip.scoring.load_models() reads
with numpy alone:

    cfd_tables.npz         mm[20,4,4] (position, wildtype RNA base A,C,G,U, sgRNA base A,C,G,T), pam[16] (PAM[-2:], 4*b0+b1)
                           <- scores/cfdscore/models/mismatch_score.pkl + pam_scores.pkl
    azimuth_model.npz      tree_off[T+1], feature[N] (-1 = leaf), left[N], right[N] (node indices relative to their
                           tree), threshold[N], value[N], init, learning_rate
                           <- azimuth/saved_models/V3_model_nopos.pickle (sklearn GradientBoostingRegressor)
    deepcpf1_weights.npz   conv_w[80,4,5] conv_b[80] w1[80,1200] b1[80] w2[40,80] b2[40] w3[40,40] b3[40] w4[1,40] b4[1]
                           (torch layout of SeqDeepCpf1) <- deepCpf1/weights/Seq_deepCpf1_weights.h5 (Keras)
    rs3_model.txt          LightGBM text model <- rs3's pickled booster (rs3 package data, RuleSet3.pkl)
    plmcrispr_model.npz    the state_dict of PLM-CRISPR's sgrna_net by name (crisprhawk_hip.synth.PLMCRISPR_SHAPES) plus
                           protein_spcas9 / protein_xcas9, the (L, 1280) ESM embeddings
                           <- plm_crispr/models/100.pt (a full-object pickle of train_general.sgrna_net) + SpCas9.esm.pt +
                           xCas9.esm.pt.  UNTESTED AGAINST THE REAL CHECKPOINT: those files are a download this project
                           has never had; the route is tested on a synthetic checkpoint saved with the stand-in classes below.

    python tools/convert_models.py --models-dir <reference>/src/crisprhawk/scores --out <dir>
"""
import argparse
import glob
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crispr-hawk_amd")]

import numpy as np  # noqa: E402


def find(root, pattern):
    hits = glob.glob(os.path.join(root, "**", pattern), recursive=True)
    return hits[0] if hits else None


def plm_standins():
    """Modules named `train_general` and `Protein` holding nn.Module classes of this project's own under the names 100.pt was
    pickled with (sgrna_net; TextCNN, GlobalMaxPool1d).  Unpickling a full-object checkpoint needs the classes only as
    containers - pickle fills their __dict__ and never calls __init__ - and state_dict() then reads the stored submodules.
    The constructors build the same tree of layers so that a synthetic checkpoint can be saved for the tests."""
    import types

    from torch import nn

    class GlobalMaxPool1d(nn.Module):
        pass

    class TextCNN(nn.Module):
        def __init__(self):
            super().__init__()
            self.pool = GlobalMaxPool1d()
            self.dropout = nn.Dropout(0.0)
            self.convs = nn.ModuleList(nn.Conv1d(1280, 128, k) for k in (5, 9, 13))

    class sgrna_net(nn.Module):  # noqa: N801 - the pickled name
        def __init__(self):
            super().__init__()
            self.conv1, self.conv2 = nn.Conv1d(5, 64, 5, padding=2), nn.Conv1d(64, 64, 5, padding=2)
            self.conv3, self.conv4 = nn.Conv1d(64, 64, 5, padding=2), nn.Conv1d(5, 64, 5, padding=2)
            self.text_cnn = TextCNN()
            self.lin1, self.lin3, self.lin4 = nn.Linear(7552, 2048), nn.Linear(2048, 256), nn.Linear(384, 256)
            self.lin5, self.lin6 = nn.Linear(256, 128), nn.Linear(128, 1)
            self.weight_net = nn.Sequential(nn.Linear(512, 128), nn.ReLU(), nn.Linear(128, 2), nn.Softmax(dim=1))

    mods = {"train_general": types.ModuleType("train_general"), "Protein": types.ModuleType("Protein")}
    for cls, home in ((GlobalMaxPool1d, "Protein"), (TextCNN, "Protein"), (sgrna_net, "train_general")):
        cls.__module__, cls.__qualname__ = home, cls.__name__
        setattr(mods[home], cls.__name__, cls)
    mods["train_general"].TextCNN = TextCNN
    return mods


class _PlmModules:
    """the stand-ins under their bare names in sys.modules, for the length of one torch.save / torch.load"""

    def __enter__(self):
        self.mods = plm_standins()
        self.prev = {k: sys.modules.get(k) for k in self.mods}
        sys.modules.update(self.mods)
        return self.mods

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def plm_state_dict(checkpoint):
    """100.pt -> {state_dict name: fp32 array}"""
    import torch
    with _PlmModules():
        net = torch.load(checkpoint, map_location="cpu", weights_only=False)
    return {k: v.detach().to(torch.float32).numpy() for k, v in net.state_dict().items()}


def plm_embedding(path):
    """SpCas9.esm.pt / xCas9.esm.pt -> (L, 1280) fp32 (the reference reads `representations`, plm_crispr.py:130-133)"""
    import torch
    rep = torch.load(path, map_location="cpu", weights_only=False)["representations"]
    rep = rep.detach().to(torch.float32).numpy()
    return rep.reshape(-1, rep.shape[-1])


def convert_plmcrispr(checkpoint, proteins, out_path):
    """proteins: {"protein_spcas9" / "protein_xcas9": path}; checks every tensor's shape before anything is written"""
    from crisprhawk_hip import scoring
    sd = plm_state_dict(checkpoint)
    scoring.pack_plmcrispr_params(sd)
    np.savez(out_path, **sd, **{k: plm_embedding(p) for k, p in proteins.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models-dir", required=True)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    from crisprhawk_hip import scoring
    os.makedirs(args.out, exist_ok=True)
    mmf, pamf = find(args.models_dir, "mismatch_score.pkl"), find(args.models_dir, "pam_scores.pkl")
    if mmf and pamf:
        mm, pam = scoring.cfd_tables_from_dicts(pickle.load(open(mmf, "rb")), pickle.load(open(pamf, "rb")))
        np.savez(os.path.join(args.out, "cfd_tables.npz"), mm=mm, pam=pam)
        print("cfd_tables.npz")
    azf = find(args.models_dir, "V3_model_nopos.pickle")
    if azf:
        obj = pickle.load(open(azf, "rb"))  # (model, learn_options), model_comparison.py:538-550
        gbr = obj[0] if isinstance(obj, (tuple, list)) else obj
        np.savez(os.path.join(args.out, "azimuth_model.npz"), **scoring.azimuth_model_from_sklearn(gbr))
        print("azimuth_model.npz")
    h5f = find(args.models_dir, "Seq_deepCpf1_weights.h5")
    if h5f:
        import h5py
        kw = {}
        with h5py.File(h5f, "r") as f:  # seqdeepcpf1.py:95-124 reads the same datasets
            f.visititems(lambda name, ds: kw.__setitem__(name.split("/")[-1], np.array(ds)) if hasattr(ds, "shape") else None)
        np.savez(os.path.join(args.out, "deepcpf1_weights.npz"), **scoring.deepcpf1_weights_from_keras(kw))
        print("deepcpf1_weights.npz")
    rsf = find(args.models_dir, "RuleSet3.pkl")
    if rsf:
        booster = pickle.load(open(rsf, "rb"))
        booster = getattr(booster, "booster_", booster)
        open(os.path.join(args.out, "rs3_model.txt"), "w").write(booster.model_to_string())
        print("rs3_model.txt")
    plm = find(args.models_dir, "100.pt")
    prot = {k: find(args.models_dir, f) for k, f in (("protein_spcas9", "SpCas9.esm.pt"), ("protein_xcas9", "xCas9.esm.pt"))}
    prot = {k: f for k, f in prot.items() if f}
    if plm and prot:  # untested against the real checkpoint (see the module docstring)
        convert_plmcrispr(plm, prot, os.path.join(args.out, "plmcrispr_model.npz"))
        print("plmcrispr_model.npz")


if __name__ == "__main__":
    main()
