#!/usr/bin/env python3
"""The rows of the C3 expansion plan as text (hawk_xplan_text: k_hx_text, hawk_haptext.hip), all rows in batches of whole rows
under the byte budget of haplotypes.haplotypes_table: kernel ms and bytes written per second, the wall time of the calls
(kernel + the copy into page-locked host memory), and hawk_xplan_run on the same plan for comparison - that path writes the
same rows as five bit planes (3.13 GB against about 5 GB of text).  One warm-up pass, then `--repeats` timed passes; the
median with the smallest and largest value is reported, as JSON on stdout and into `--out`."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crispr-hawk_amd")]
from crisprhawk_hip import haplotypes as H, synth  # noqa: E402
from crisprhawk_hip.workload import expand_on_device  # noqa: E402


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch-bytes", type=int, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reg = synth.config_c3()
    ds, _info, _ms, _kept = expand_on_device(reg, 3, keep_plan=True)
    plan = ds.plan
    budget = H.text_batch_bytes(args.batch_bytes)
    lens = plan.hap_len.tolist()
    batches = H.text_batches(lens, budget)
    total = int(sum(lens))
    k_ms, wall_ms, run_ms = [], [], []
    for rep in range(args.repeats + 1):
        ms, t0 = 0.0, time.perf_counter()
        for a, b in batches:
            buf, _off, m = plan.text(range(a, b), timed=True)
            ms += m
            del buf
        w = (time.perf_counter() - t0) * 1e3
        ds2, _h, r = plan.run(timed=True)
        ds2.close()
        if rep:  # the first pass warms the allocators up
            k_ms.append(ms); wall_ms.append(w); run_ms.append(r)
    S = ds.stride
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = None
    res = {"workload": "C3", "rows": plan.n_hap, "text_bytes": total, "batch_bytes": budget, "batches": len(batches),
           "text_kernel_ms": spread(k_ms), "text_kernel_bytes_per_s": total / (statistics.median(k_ms) * 1e-3),
           "text_call_wall_ms": spread(wall_ms), "text_call_bytes_per_s": total / (statistics.median(wall_ms) * 1e-3),
           "xplan_run_kernel_ms": spread(run_ms), "xplan_run_plane_bytes": 5 * 4 * S * plan.n_hap,
           "xplan_run_bytes_per_s": 5 * 4 * S * plan.n_hap / (statistics.median(run_ms) * 1e-3), "parent_commit": commit}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    plan.close()
    ds.close()


if __name__ == "__main__":
    main()
