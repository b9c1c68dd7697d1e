"""Brute-force yardstick of the BED annotation join: every query x every feature, in file order.  Plain Python / numpy; shares
no code with the package.  Overlap is tabix's documented rule, 0-based half-open on both sides (parity unpinned: pysam absent)."""
import numpy as np


def parse_bed(text):
    """{contig: [(start, end, fields)]} in file order; comment, track, browser and empty lines skipped."""
    out = {}
    for ln in text.splitlines():
        if not ln.strip() or ln.startswith(("#", "track", "browser")):
            continue
        f = ln.split()
        out.setdefault(f[0], []).append((int(f[1]), int(f[2]), f))
    return out


def func_label(fields):
    return fields[3]


def gene_label(fields):
    attrs = fields[9]
    i = attrs.find("gene_name=")
    if i == -1:
        name = ""
    else:
        j = attrs.find(";", i + 10)
        name = attrs[i + 10:j] if j != -1 else attrs[i + 10:len(attrs) - 1]  # the reference's slice ends at -1 without a ';'
    return f"{fields[7]}:{name}"


def join_rows(starts, ends, labels, qstart, qstop):
    """Row per query: labels of the features with fs < qe and fe > qs joined by ',', or 'NA'."""
    rows = []
    for qs, qe in zip(qstart, qstop):
        hit = [lab for fs, fe, lab in zip(starts, ends, labels) if fs < qe and fe > qs]
        rows.append(",".join(hit) if hit else "NA")
    return rows


def join_rows_np(starts, ends, labels, qstart, qstop, chunk=2048):
    """join_rows for large inputs: the same every-query-x-every-feature mask, chunks of queries at a time."""
    starts, ends = np.asarray(starts, dtype=np.int64), np.asarray(ends, dtype=np.int64)
    qstart, qstop = np.asarray(qstart, dtype=np.int64), np.asarray(qstop, dtype=np.int64)
    rows = []
    for c in range(0, len(qstart), chunk):
        m = (starts[None, :] < qstop[c:c + chunk, None]) & (ends[None, :] > qstart[c:c + chunk, None])
        for r in m:
            idx = np.flatnonzero(r)
            rows.append(",".join(labels[i] for i in idx) if len(idx) else "NA")
    return rows


def ragged(rows):
    """(blob uint8, off uint64[n + 1]) of a list of strings"""
    enc = [r.encode("ascii") for r in rows]
    off = np.zeros(len(enc) + 1, dtype=np.uint64)
    if enc:
        off[1:] = np.cumsum([len(e) for e in enc])
    return np.frombuffer(b"".join(enc), dtype=np.uint8), off


def table_arrays(feats, label):
    """(start, end, labels) of one contig's parsed features"""
    return [f[0] for f in feats], [f[1] for f in feats], [label(f[2]) for f in feats]


def dedup(cell):
    """a report cell as the collapse leaves it, order aside: the set of its labels"""
    return set(cell.split(","))
