#!/usr/bin/env python3
"""Time PLM-CRISPR on the device (scoring.plmcrispr -> hawk_plm_score) and write profiles/plmcrispr.json.

    python tools/time_plmcrispr.py [--runs 3] [--sizes 220000 1400000] [--batch 0]
    python tools/time_plmcrispr.py --reference-cpu /path/to/reference/src [--guides 10000]

Sizes: 2.2x10^5 guides (the report groups of C3) and 1.4x10^6 (those of one C4 tile); the model has seeded weights
(synth.plmcrispr_weights) and a protein of L = 1368 residues (SpCas9).  Per size, after a warm-up call, --runs calls of
scoring.plmcrispr timed by the host clock (the call ends in a device synchronise and includes the upload of the guides, the
download of the scores and the Python list on either side), then --runs calls in the library's timed mode (hawk_plm_timing: HIP
events around each kernel, summed over the batches; the call waits per batch, so its wall time is not reported).  Reported as
min / max over the runs: wall seconds, guides per second, seconds per kernel, and the achieved TFLOP/s of k_plm_lin1 on lin1
(2 x 7552 x 2048 FLOP per guide, the operations the layer needs; padding rows of the last tile are not counted) beside 122 TFLOP/s,
the reported rate of an untuned LDS-tiled 4096^3 GEMM on the same f32-input MFMA, and the 157.3 TFLOP/s fp32 matrix peak of the MI355X.
hawk_plm_create (upload of 83 MB + the protein branch, once per model) is timed by the host clock.

--reference-cpu (build machine only, no GPU, nothing else runs): the reference's own torch path - sgrna_net in batches of 64 with
the protein embedding repeated per batch, as compute_plm_crispr_score runs it (plm_crispr.py:225-238) - on this machine's CPU for
--guides guides; merged into the JSON as `reference_cpu` with the machine named."""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "crispr-hawk_amd"))
OUT = os.path.join(ROOT, "profiles", "plmcrispr.json")
L_SPCAS9 = 1368
LIN1_FLOP = 2.0 * 7552 * 2048
GUIDE_FLOP = 2.0 * (2 * 64 * 25 * 59 + 2 * 64 * 320 * 59 + 7552 * 2048 + 2048 * 256 + 512 * 128 + 2 * 128 + 256 * 128 + 128)
KERNELS = ("k_plm_front", "k_plm_lin1 (lin1)", "k_plm_lin1 (lin3)", "k_plm_tail")


def guides(n, seed=31):
    rng = np.random.default_rng(seed)
    return ["".join(r) for r in np.array(list("ACGT"))[rng.integers(0, 4, size=(n, 23))]]


def cpu_name():
    try:
        with open("/proc/cpuinfo") as f:
            return next(ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name"))
    except (OSError, StopIteration):
        return platform.processor() or platform.machine()


def reference_cpu(src, n, out):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_golden_plmcrispr import load_reference
    from crisprhawk_hip import synth
    R_net, R_wrap = load_reference(src)
    net = R_net.sgrna_net()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.plmcrispr_weights().items()})
    net.eval()
    emb = torch.from_numpy(synth.plmcrispr_protein(2003, L_SPCAS9)).to(torch.float16)
    enc = R_wrap._encode_sequences(R_wrap._build_input_sequences(guides(n))).long()
    t0 = time.perf_counter()
    with torch.no_grad():
        for lo in range(0, n, R_wrap.BATCH_SIZE):
            b = enc[lo:lo + R_wrap.BATCH_SIZE]
            net(b, 0, emb.unsqueeze(0).repeat(len(b), 1, 1), train=False).view(-1).tolist()
    dt = time.perf_counter() - t0
    res = json.load(open(out)) if os.path.exists(out) else {}
    res["reference_cpu"] = {"what": "the reference's sgrna_net through torch on the CPU, batches of 64, the protein branch recomputed for every "
                                    "row of every batch as compute_plm_crispr_score does; seeded weights, L = 1368",
                            "machine": f"build machine: {cpu_name()}, {os.cpu_count()} cores, {torch.get_num_threads()} torch threads, "
                                       f"torch {torch.__version__}",
                            "guides": n, "seconds": dt, "guides_per_second": n / dt}
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res["reference_cpu"]))


def measure(n, runs, batch):
    import ctypes as C

    from crisprhawk_hip import _lib, scoring
    from crisprhawk_hip.pam import SPCAS9
    seqs = guides(n)
    scoring.plmcrispr(seqs[:min(n, 10000)], SPCAS9, True, batch)  # warm-up: code objects, the allocator's blocks
    first = scoring.plmcrispr(seqs, SPCAS9, True, batch)
    wall = []
    for _ in range(runs):
        t0 = time.perf_counter()
        got = scoring.plmcrispr(seqs, SPCAS9, True, batch)
        wall.append(time.perf_counter() - t0)
        assert got == first, "scores differ between runs"
    h, ms = scoring._PLM[SPCAS9], (C.c_float * 4)()
    kern = []
    _lib.check(_lib.lib().hawk_plm_timing(h, 1, None), "hawk_plm_timing")
    for _ in range(runs):
        assert scoring.plmcrispr(seqs, SPCAS9, True, batch) == first
        _lib.check(_lib.lib().hawk_plm_timing(h, 1, ms), "hawk_plm_timing")
        kern.append([x / 1e3 for x in ms])
    _lib.check(_lib.lib().hawk_plm_timing(h, 0, None), "hawk_plm_timing")
    mm = lambda v: {"min": min(v), "max": max(v)}
    res = {"guides": n, "batch": batch or 8192, "wall_seconds": mm(wall), "guides_per_second": mm([n / w for w in wall]),
           "end_to_end_tflops": mm([n * GUIDE_FLOP / w / 1e12 for w in wall]),
           "kernel_seconds": {name: mm([k[i] for k in kern]) for i, name in enumerate(KERNELS)},
           "kernel_seconds_sum": mm([sum(k) for k in kern]),
           "k_plm_lin1_tflops": mm([n * LIN1_FLOP / k[1] / 1e12 for k in kern]),
           "score_mean": float(np.mean(first)), "score_std": float(np.std(first))}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[220_000, 1_400_000])
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--reference-cpu", metavar="REFERENCE_SRC")
    ap.add_argument("--guides", type=int, default=10_000)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.reference_cpu:
        return reference_cpu(a.reference_cpu, a.guides, a.out)
    from crisprhawk_hip import scoring, synth
    from crisprhawk_hip.pam import SPCAS9
    old = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res = {"units": "seconds", "runs": a.runs, "protein_L": L_SPCAS9,
           "yardsticks_tflops": {"untuned f32-MFMA GEMM, 4096^3": 122.0, "fp32 matrix peak": 157.3},
           "flop_per_guide": GUIDE_FLOP, "lin1_flop_per_guide": LIN1_FLOP, **{k: v for k, v in old.items() if k == "reference_cpu"}}
    params, protein = synth.plmcrispr_weights(), synth.plmcrispr_protein(2003, L_SPCAS9)
    create = []
    for _ in range(a.runs + 1):
        t0 = time.perf_counter()
        scoring.set_plmcrispr_model(params, {SPCAS9: protein})
        create.append(time.perf_counter() - t0)
    res["set_plmcrispr_model_seconds"] = {"min": min(create[1:]), "max": max(create[1:]),
                                          "what": "pack + hawk_plm_create: 83 MB upload and the protein branch (6 GFLOP), once per model"}
    for n in a.sizes:
        res[f"n_{n}"] = measure(n, a.runs, a.batch)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    scoring.clear_plmcrispr_model()


if __name__ == "__main__":
    main()
