#!/usr/bin/env python3
"""Time the three BGZF inflate routes of readers._TextSource - "zlib" (one member at a time on the Python thread: the code every
reader ran before the switch existed, and the baseline here), "native" (hawk_host_bgzf_inflate on host threads) and "device"
(hawk_bgzf_inflate: k_bz_inflate, one wavefront per member) - on one synthetic sites VCF.

    python tools/time_bgzf_inflate.py [--mib 256] [--runs 3] [--threads 16] [--out profiles/bgzf_inflate.json]

The file is made by the project's own generator and writer: synth.gnomad_sites_lines (repeated with shifted positions) through
readers.BgzfWriter, at least --mib MiB of text in members of 0xff00 bytes; its compression ratio is recorded.  One process.  After a
warm-up pass per route (whose text must hash alike on all three), every lap is taken --runs times, the routes in turn inside a
run, and reported min - median - max:

  chunks_wall      a whole `chunks()` pass, wall clock (for "device": read, upload, kernel, download per 32 MiB chunk)
  kernel / upload / download   the device calls' laps by the context's device clock stamps, summed over the pass ("device" only)
  vcf_wall         `readers.VCF(fname, inflate=route)`: the index pass
  convert_wall, convert_inflate   `converter.convert_vcf(engine="device", inflate=route)` and its `inflate` lap

Nothing here runs without a GPU: the "device" route and the converter's device engine raise.
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

ROUTES = ("zlib", "native", "device")


def make_input(path, n_bytes, unique, info_keys, threads):
    base = synth.gnomad_sites_lines(20261021, unique, False, info_keys)
    w = readers.BgzfWriter(path, threads)
    head = ("\n".join(synth.gnomad_sites_header(False)) + "\n").encode()
    w.write(head)
    raw, rep, records = len(head), 0, 0
    while raw < n_bytes:
        part = base if not rep else ["\t".join([f[0], str(int(f[1]) + rep * 100_000_000)] + f[2:]) for f in (ln.split("\t") for ln in base)]
        data = ("\n".join(part) + "\n").encode()
        w.write(data)
        raw += len(data)
        records += len(part)
        rep += 1
    w.close()
    return raw, records


def spread(vals):
    return {"min": min(vals), "median": statistics.median(vals), "max": max(vals)}


def chunks_pass(fname, route, digest=False):
    src = readers._TextSource(fname, route)
    h = hashlib.sha256() if digest else None
    t0 = time.perf_counter()
    n = 0
    for _, chunk in src.chunks():
        n += len(chunk)
        if h is not None:
            h.update(chunk)
    wall = time.perf_counter() - t0
    return {"chunks_wall": wall, "kernel": src.inflate_ms / 1e3, "upload": src.upload_ms / 1e3, "download": src.download_ms / 1e3}, n, h.hexdigest() if h else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--unique", type=int, default=4000)
    ap.add_argument("--info-keys", type=int, default=230)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_inflate.json"))
    a = ap.parse_args()
    os.environ["OMP_NUM_THREADS"] = str(a.threads)  # what the "native" route reads
    res = {"runs": a.runs, "threads": a.threads, "chunk_bytes": readers._TextSource.CHUNK, "routes": {}}
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "synthetic.sites.vcf.bgz")
        t0 = time.perf_counter()
        res["text_bytes"], res["records"] = make_input(src, a.mib << 20, a.unique, a.info_keys, a.threads)
        res["file_bytes"] = os.path.getsize(src)
        res["compression_ratio"] = res["text_bytes"] / res["file_bytes"]
        res["members"] = len(readers._TextSource(src, "zlib")._c_off) - 1
        print(f"input: {res['text_bytes'] / 2 ** 20:.1f} MiB of text in {res['members']} members, {res['file_bytes'] / 2 ** 20:.1f} MiB BGZF "
              f"(ratio {res['compression_ratio']:.2f}), made in {time.perf_counter() - t0:.1f} s", flush=True)
        digests = {}
        for route in ROUTES:  # warm-up: code objects, the page-locked cache, the file in the page cache
            _, n, digests[route] = chunks_pass(src, route, digest=True)
            assert n == res["text_bytes"]
        res["text_equal"] = len(set(digests.values())) == 1
        res["text_sha256"] = digests["zlib"]
        laps = {r: {} for r in ROUTES}
        add = lambda route, name, v: laps[route].setdefault(name, []).append(v)
        outs = {}
        for k in range(a.runs):
            for route in ROUTES:
                t, _, _ = chunks_pass(src, route)
                for name, v in t.items():
                    if route == "device" or name == "chunks_wall":
                        add(route, name, v)
                t0 = time.perf_counter()
                v = readers.VCF(src, inflate=route)
                add(route, "vcf_wall", time.perf_counter() - t0)
                res["vcf_records"] = len(v._pos)
                del v
                od = os.path.join(td, route)
                os.makedirs(od, exist_ok=True)
                r = converter.convert_vcf(src, False, False, "conv", od, 0, True, engine="device", threads=a.threads, inflate=route)
                add(route, "convert_wall", r["timing"]["total"])
                add(route, "convert_inflate", r["timing"]["inflate"])
                if route == "device":
                    add(route, "convert_kernel", r["timing"]["inflate_ms"] / 1e3)
                with open(r["path"], "rb") as f:
                    outs[route] = hashlib.sha256(f.read()).hexdigest()
                print(f"  run {k} {route}: " + ", ".join(f"{n} {x[-1]:.3f}" for n, x in laps[route].items()), flush=True)
        res["converted_files_equal"] = len(set(outs.values())) == 1
        for route in ROUTES:
            e = {n: spread(x) for n, x in laps[route].items()}
            e["chunks_text_bytes_per_s"] = res["text_bytes"] / e["chunks_wall"]["median"]
            if route == "device" and e["kernel"]["median"] > 0:
                e["kernel_text_bytes_per_s"] = res["text_bytes"] / e["kernel"]["median"]
            res["routes"][route] = e
        z = res["routes"]["zlib"]["chunks_wall"]["median"]
        res["chunks_speedup_over_zlib"] = {r: z / res["routes"][r]["chunks_wall"]["median"] for r in ROUTES}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "routes"}))
    if not (res["text_equal"] and res["converted_files_equal"]):
        sys.exit("the routes disagree")


if __name__ == "__main__":
    main()
