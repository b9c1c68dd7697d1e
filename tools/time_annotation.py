#!/usr/bin/env python3
"""The BED annotation join on the device (hawk_annot_create / hawk_annot_query) against the yardstick there is: the same join
on the host with numpy (`searchsorted` for the two bounds, then the same walk in Python) - the parent of this path had no
annotation at all and the reference's needs pysam.  One process on the card.

  panels   ccre    10^6 short features (150-350 nt) on a chr22-sized contig (5.08 x 10^7 nt), seeded
           genes   3 x 10^6 nested features: genes > transcripts > exons, a few genes of 2 Mb
  queries  c3      2.2 x 10^5 intervals of 23 nt, sorted by start (the groups of a C3 report)
           c4      3.0 x 10^7 (the groups of a C4 report)                                          [--c4]

Per (panel, queries): create (wall, index kernels), query (wall; upload, k_ann_count, scan, k_ann_fill, download by HIP events),
median / min / max of `--repeats` runs after `--warmup`; overlaps, bytes out, walk steps of the count pass; the host join's wall
clock on `--host-queries` queries taken evenly across the batch (so the last of them lie at the end of the blob: on the nested
C4 column past 2^32 bytes), EXTRAPOLATED linearly to the batch, and the identity of those rows with the device's.

`--files`: what a user pays - pipeline.search_files on the C3 file set (tools/files_to_tsv.py) without and with two annotation
files (the cCRE panel as a 4-column BED, the genes panel as a 10-column GENCODE-style BED, both on the region's contig), the
`timings` stages of both runs side by side.

    python tools/time_annotation.py [--c4] [--files] [--out profiles/annotation.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "crispr-hawk_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

CONTIG = 50_800_000


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def panel_ccre(rng, n=1_000_000):
    s = np.sort(rng.integers(0, CONTIG - 400, n)).astype(np.int64)
    return s, s + rng.integers(150, 350, n), [f"cCRE{k}" for k in rng.integers(0, 9, n).tolist()]


def panel_genes(rng, n=3_000_000):
    """genes (a few of 2 Mb), ~8 transcripts each over the gene's span, exons inside the transcripts; sorted by start, stable"""
    n_genes = n // 100
    gs = np.sort(rng.integers(0, CONTIG - 2_100_000, n_genes))
    glen = rng.integers(2_000, 120_000, n_genes)
    glen[rng.choice(n_genes, 8, replace=False)] = 2_000_000
    per = n // n_genes - 1
    owner = np.repeat(np.arange(n_genes), per)
    off = (rng.random(len(owner)) * (glen[owner] - 200)).astype(np.int64)
    is_tx = (np.arange(len(owner)) % per) < 8
    length = np.where(is_tx, np.maximum((glen[owner] - off) * rng.random(len(owner)), 200).astype(np.int64), rng.integers(50, 200, len(owner)))
    s = np.concatenate([gs, gs[owner] + off]).astype(np.int64)
    e = np.concatenate([gs + glen, gs[owner] + off + length]).astype(np.int64)
    kind = np.concatenate([np.zeros(n_genes, np.int64), np.where(is_tx, 1, 2)])
    gene = np.concatenate([np.arange(n_genes), owner])
    o = np.argsort(s, kind="stable")
    names = np.array(["gene", "transcript", "exon"], dtype=object)
    return s[o], e[o], [f"{k}:G{g}" for k, g in zip(names[kind[o]].tolist(), gene[o].tolist())]


def host_join(starts, ends, rmax, labels, qs, qe):
    hi = np.searchsorted(starts, qe, side="left")
    lo = np.searchsorted(rmax, qs, side="right")
    rows = []
    for a, b, s in zip(lo.tolist(), hi.tolist(), qs.tolist()):
        hit = [labels[i] for i in range(a, b) if ends[i] > s]
        rows.append(",".join(hit) if hit else "NA")
    return rows


def files_run(reps):
    """search_files on the C3 file set, without and with two annotation files: wall clock and `timings` stages per run"""
    import shutil
    import tempfile
    from crisprhawk_hip import synth
    from crisprhawk_hip.pipeline import search_files
    reg = synth.config_c3()
    d = tempfile.mkdtemp(prefix="hawk_c3_ann_", dir=os.environ.get("HAWK_SCRATCH", "/tmp"))
    try:
        fa, bed, vcf = synth.write_region_files(reg, d, "c3")
        rng = np.random.default_rng(2212)
        span = max(CONTIG, reg.bed_stop + 1000)
        s1, e1, l1 = panel_ccre(rng)
        s2, e2, l2 = panel_genes(rng)
        f1, f2 = os.path.join(d, "ccre.bed"), os.path.join(d, "genes.bed")
        with open(f1, "w") as f:
            f.writelines(f"{reg.contig}\t{a}\t{b}\t{c}\n" for a, b, c in zip(s1.tolist(), e1.tolist(), l1))
        with open(f2, "w") as f:
            f.writelines(f"{reg.contig}\t{a}\t{b}\tENS{k}\t0\t+\tHAVANA\t{c.split(':')[0]}\t.\tgene_id=E{k};gene_name={c.split(':')[1]};level=2\n"
                         for k, (a, b, c) in enumerate(zip(s2.tolist(), e2.tolist(), l2)))
        mm, pt = synth.cfd_tables()
        out = {"region": f"{reg.contig}:{reg.bed_start}-{reg.bed_stop}", "contig_span_of_the_files": int(span),
               "annotation_file_bytes": [os.path.getsize(f1), os.path.getsize(f2)], "annotation_file_lines": [len(s1), len(s2)], "runs": {}}
        for name, kw in (("without", {}), ("with", dict(annotations=[f1], gene_annotations=[f2]))):
            runs = []
            for r in range(reps):
                tm = {}
                t0 = time.perf_counter()
                paths = search_files(fa, bed, [vcf], "NGG", 20, False, os.path.join(d, f"out_{name}{r}"), cfd_tables=(mm, pt), timings=tm, **kw)
                wall = time.perf_counter() - t0
                runs.append({"wall_s": wall, "stages_s": tm, "tsv_bytes": os.path.getsize(list(paths.values())[0])})
                print(json.dumps({name: runs[-1]}), file=sys.stderr, flush=True)
            out["runs"][name] = runs
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", action="store_true", help="only: search_files on the C3 file set without / with two annotation files")
    ap.add_argument("--file-reps", type=int, default=2)
    ap.add_argument("--c4", action="store_true", help="also the 3.0e7-query batch")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-queries", type=int, default=20_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "annotation.json"))
    args = ap.parse_args()
    if args.files:
        prev = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                prev = json.load(f)
        prev["search_files_c3"] = files_run(args.file_reps)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(prev, f, indent=1)
        print(json.dumps(prev["search_files_c3"]))
        return
    from crisprhawk_hip.bedannot import AnnotTable
    rng = np.random.default_rng(2211)
    out = {"contig_nt": CONTIG, "warmup": args.warmup, "repeats": args.repeats, "panels": {}}
    batches = [("c3", 220_000)] + ([("c4", 30_000_000)] if args.c4 else [])
    for pname, make in (("ccre", panel_ccre), ("genes", panel_genes)):
        s, e, labels = make(rng)
        enc = [x.encode() for x in labels]
        loff = np.zeros(len(enc) + 1, np.uint64)
        loff[1:] = np.cumsum([len(x) for x in enc])
        blob = np.frombuffer(b"".join(enc), dtype=np.uint8)
        wall, idx_ms = [], []
        tab = None
        for _ in range(args.warmup + args.repeats):
            if tab is not None:
                tab.close()
            t0 = time.perf_counter()
            tab = AnnotTable(s, e, blob, loff)
            wall.append(time.perf_counter() - t0)
            idx_ms.append(tab.index_ms)
        res = {"features": len(s), "label_bytes": int(loff[-1]), "table_bytes_in_hbm": int(len(s) * 8 * 4 + len(s) // 64 * 8 + loff[-1]),
               "create_wall_s": spread(wall[args.warmup:]), "index_kernels_ms": spread(idx_ms[args.warmup:]), "queries": {}}
        rmax = np.maximum.accumulate(e)
        for qname, nq in batches:
            qs = np.sort(rng.integers(0, CONTIG - 23, nq)).astype(np.int64)
            qe = qs + 23
            wall, tms, col = [], [], None
            for _ in range(args.warmup + args.repeats):
                col = None
                t0 = time.perf_counter()
                col = tab.query(qs, qe)
                wall.append(time.perf_counter() - t0)
                tms.append(dict(tab.timing))
            tms, wall = tms[args.warmup:], wall[args.warmup:]
            r = {"n_queries": nq, "overlaps": tab.n_overlaps, "out_bytes": tms[-1]["out_bytes"], "walk_steps": tms[-1]["walk_steps"],
                 "wall_s": spread(wall)}
            for k in ("upload_ms", "count_ms", "scan_ms", "fill_ms", "download_ms", "total_ms"):
                r[k] = spread([t[k] for t in tms])
            # bytes k_ann_count has to move at the least: the queries in, the row bytes out, and - the lanes of a wave sharing their lines -
            # one pass over the feature columns it walks (end, label offsets) and the block maxima
            r["count_min_bytes"] = int(nq * 24 + len(s) * 16 + len(s) // 64 * 8)
            r["fill_min_bytes"] = int(nq * 24 + len(s) * 16 + int(loff[-1]) + tms[-1]["out_bytes"])
            pick = np.unique(np.linspace(0, nq - 1, min(args.host_queries, nq)).astype(np.int64))  # evenly across the batch, its last row included
            nh = len(pick)
            t0 = time.perf_counter()
            rows = host_join(s, e, rmax, labels, qs[pick], qe[pick])
            r["host_numpy_wall_s"] = time.perf_counter() - t0
            r["host_numpy_queries"] = nh
            r["host_rows_equal_device"] = rows == col.take(pick)
            r["host_rows_checked_past_2_32"] = int((col.off[pick] >= (1 << 32)).sum())
            r["host_numpy_wall_s_extrapolated_to_batch"] = r["host_numpy_wall_s"] * nq / nh
            res["queries"][qname] = r
        tab.close()
        out["panels"][pname] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
