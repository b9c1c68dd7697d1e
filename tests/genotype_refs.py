"""Plain references for the VCF genotype stage (hawk_vcf.hip): the carried-variant lists as one vectorised numpy statement,
the text -> fields split the parse reference (oracle.vcf_genotype_codes) is fed with, and the geometry of a record's field
starts in k_gt_parse's sweeps.  Shares no code with the package and never calls its library."""
import numpy as np

# k_gt_parse geometry: GT_CHUNK bytes per thread and __launch_bounds__(256) threads per workgroup in hawk_vcf.hip, so one sweep
# of the workgroup covers 256 * 16 = 4096 bytes of a record's sample columns.
CHUNK = 16
THREADS = 256
SWEEP = CHUNK * THREADS


def carried_lists_np(codes, var_line, var_allele, var_r0, var_chain, col_block=1024):
    """oracle.carried_lists without the double loop: column c carries variant j iff codes[var_line[j], c] == var_allele[j];
    its list is the carried j ascending, hv_o = var_r0[j] + the summed var_chain of the entries before it in the column
    (int64 arithmetic, must fit int32), col_delta the column's whole sum.  Also returns the indices of the entries with
    var_chain != 0 (what hawk_gt_lists_indels hands out).  -> col_off u64, hv_idx u32, hv_o i32, col_delta i64, indel u32."""
    codes = np.asarray(codes, dtype=np.uint8)
    var_line = np.asarray(var_line, dtype=np.int64)
    var_allele = np.asarray(var_allele, dtype=np.uint8)
    r0 = np.asarray(var_r0, dtype=np.int64)
    chain = np.asarray(var_chain, dtype=np.int64)
    n_cols = codes.shape[1]
    cols, js = [], []
    for c0 in range(0, n_cols, col_block):  # blocks of columns only bound the size of the boolean matrix
        m = codes[var_line, c0:c0 + col_block] == var_allele[:, None] if len(var_line) else np.zeros((0, min(col_block, n_cols - c0)), bool)
        c, j = np.nonzero(m.T)  # row-major over the transpose: by column, then ascending j
        cols.append(c + c0)
        js.append(j)
    cols = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    js = np.concatenate(js) if js else np.zeros(0, np.int64)
    col_off = np.zeros(n_cols + 1, dtype=np.uint64)
    col_off[1:] = np.cumsum(np.bincount(cols, minlength=n_cols))
    ech = chain[js]
    g = np.concatenate([[0], np.cumsum(ech)])  # g[e] = summed chain of all entries before e, over all columns
    start = col_off[:-1].astype(np.int64)
    o = r0[js] + g[:-1] - g[start[cols]]
    assert len(o) == 0 or (o.min() >= -2**31 and o.max() < 2**31), "hv_o leaves int32: not a valid input of the stage"
    col_delta = g[col_off[1:].astype(np.int64)] - g[start]
    return col_off, js.astype(np.uint32), o.astype(np.int32), col_delta.astype(np.int64), np.flatnonzero(ech != 0).astype(np.uint32)


def section_bounds(text, gt_off, line_end):
    """[lo, hi) of a record's sample columns: from gt_off to the record's end without its trailing '\\n' / '\\r' bytes."""
    hi = line_end
    while hi > gt_off and text[hi - 1:hi] in (b"\n", b"\r"):
        hi -= 1
    return gt_off, hi


def section_fields(text, gt_off, line_end):
    """The sample columns as the strings a tab split gives; an empty section has no field at all."""
    lo, hi = section_bounds(text, gt_off, line_end)
    return text[lo:hi].decode("ascii").split("\t") if hi > lo else []


def oracle_record(text, gt_off, line_end):
    """A tab-split record for oracle.vcf_genotype_codes (it reads fields 9..)"""
    return ["."] * 9 + section_fields(text, gt_off, line_end)


def field_seams(text, gt_off, line_end):
    """Per field of the section, where its first byte falls in k_gt_parse: (rel, sweep, thread, phase) int64 arrays with
    rel = start - gt_off, sweep = rel // 4096, thread = rel % 4096 // 16, phase = rel % 16.  A trailing tab leaves a last
    field that starts at the section's end (rel == hi - lo): it is listed too, no thread owns it."""
    lo, hi = section_bounds(text, gt_off, line_end)
    if hi == lo:
        z = np.zeros(0, np.int64)
        return z, z, z, z
    sec = np.frombuffer(text[lo:hi], dtype=np.uint8)
    rel = np.concatenate([[0], np.flatnonzero(sec == 9) + 1]).astype(np.int64)
    return rel, rel // SWEEP, rel % SWEEP // CHUNK, rel % CHUNK


def crosses(rel, length, unit):
    """does the byte range [rel, rel + length) hold bytes on both sides of a multiple of `unit`"""
    return length > 0 and rel // unit != (rel + length - 1) // unit


def n_sweeps(text, gt_off, line_end):
    lo, hi = section_bounds(text, gt_off, line_end)
    return -(-(hi - lo) // SWEEP)
