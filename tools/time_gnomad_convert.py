#!/usr/bin/env python3
"""Time the gnomAD converter, device route against host twin, on a synthetic sites VCF (BGZF).

    python tools/time_gnomad_convert.py [--records 200000] [--info-keys 230] [--runs 3] [--threads 16]

The input comes from synth.gnomad_sites_lines (about 4 kB of INFO per record at the default --info-keys); --unique records are
generated and repeated with shifted positions up to --records.  Both engines convert the file --runs times; the stages are
reported in seconds with their spread (min / median / max over the runs): inflate, upload, k_gn_scan, text kernels, float pool,
the lines call as a whole (for the device: pool upload, kernels, download), deflate + write, and the wall time.  The scan
kernel's bytes per second stand beside the HBM peak.  The two output files must be byte-equal.  Writes
profiles/gnomad_convert.json.  The reference itself cannot run here (pysam absent): the comparison is device against host twin.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "crispr-hawk_amd"))

from crisprhawk_hip import converter, readers, synth  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, MI355X


def make_input(path, n_records, unique, info_keys, threads):
    base = synth.gnomad_sites_lines(20261019, min(unique, n_records), False, info_keys)
    w = readers.BgzfWriter(path, threads)
    w.write(("\n".join(synth.gnomad_sites_header(False)) + "\n").encode())
    n = raw = rep = 0
    while n < n_records:
        part = base[:n_records - n]
        if rep:
            part = ["\t".join([f[0], str(int(f[1]) + rep * 100_000_000)] + f[2:]) for f in (ln.split("\t") for ln in part)]
        data = ("\n".join(part) + "\n").encode()
        w.write(data)
        raw += len(data)
        n += len(part)
        rep += 1
    w.close()
    return raw


def spread(vals):
    return {"min": min(vals), "median": statistics.median(vals), "max": max(vals)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=200_000)
    ap.add_argument("--unique", type=int, default=4_000)
    ap.add_argument("--info-keys", type=int, default=230)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gnomad_convert.json"))
    a = ap.parse_args()
    res = {"records": a.records, "info_keys": a.info_keys, "runs": a.runs, "threads": a.threads, "hbm_peak_bytes_per_s": HBM_PEAK, "engines": {}}
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "synthetic.sites.vcf.bgz")
        t0 = time.perf_counter()
        res["text_bytes"] = make_input(src, a.records, a.unique, a.info_keys, a.threads)
        res["input_file_bytes"] = os.path.getsize(src)
        print(f"input: {a.records} records, {res['text_bytes'] / 1e6:.1f} MB of text, {res['input_file_bytes'] / 1e6:.1f} MB BGZF, made in {time.perf_counter() - t0:.1f} s",
              flush=True)
        digests = {}
        for engine in ("device", "host"):
            runs = []
            for k in range(a.runs):
                r = converter.convert_vcf(src, False, False, engine, td, 0, True, engine=engine, threads=a.threads)
                t = r["timing"]
                kernels = (t["len_ms"] + t["prefix_ms"] + t["fill_ms"]) / 1e3
                runs.append({"inflate": t["inflate"], "upload": t["upload_ms"] / 1e3, "k_gn_scan": t["scan_ms"] / 1e3, "text_kernels": kernels,
                             "float_pool": t["float_pool"], "lines_call": t["lines_call"], "deflate_write": t["deflate_write"], "wall": t["total"]})
                print(f"  {engine} run {k}: " + ", ".join(f"{n} {v:.3f}" for n, v in runs[-1].items()), flush=True)
            with open(r["path"], "rb") as f:
                digests[engine] = hashlib.sha256(f.read()).hexdigest()
            e = {n: spread([x[n] for x in runs]) for n in runs[0]}
            e.update(kept=r["kept"], batches=t["batches"], out_file_bytes=os.path.getsize(r["path"]))
            scan = e["k_gn_scan"]["median"]
            e["scan_bytes_per_s"] = res["text_bytes"] / scan if scan > 0 else None
            if engine == "device":
                e["scan_fraction_of_hbm_peak"] = e["scan_bytes_per_s"] / HBM_PEAK
            res["engines"][engine] = e
        res["outputs_byte_equal"] = digests["device"] == digests["host"]
        res["sha256"] = digests["device"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "engines"}))
    if not res["outputs_byte_equal"]:
        sys.exit("the two engines' files differ")


if __name__ == "__main__":
    main()
