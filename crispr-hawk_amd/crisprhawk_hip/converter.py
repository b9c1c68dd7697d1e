"""gnomAD sites VCF -> population-genotype VCF (`crisprhawk convert-gnomad-vcf`; reference converter.py:99-413).

gnomAD sites files carry no genotypes.  The reference treats the ten gnomAD populations as samples: a population whose
`AC_<pop>` (or `AC_joint_<pop>`) INFO entry holds a count above zero gets `0/1`, every other one `0/0`, and the record is
rewritten as `CHROM POS ID REF ALT QUAL FILTER AF=<af> GT <ten genotypes>`.  It does so through one pysam object per record.
Here the text of a batch of whole lines goes to HBM once: `k_gn_scan` finds the fields, the keys and their values,
`k_gn_text_len` / `k_gn_text_fill` write the output lines (csrc/hawk_gnomad.hip; the rules themselves, once, in
csrc/hawk_gnomad.h).  The float32 texts of QUAL and AF - what pysam would hand Python - are made on the host
(`hawk_host_f32_repr`) and travel as a string pool.  `engine="host"` runs the same header through `hawk_host_gnomad_lines`
instead of the device calls; everything around it (reading, batching, pool, BGZF output) is the same code.

Kept as the reference has it: FILTER `.` becomes the empty string, an AF entry `.` becomes `None`.  Not pinned (pysam is
absent where the fixtures are made): htslib's own parsing and header text, and which occurrence of a duplicated key is read
(here: the first).
"""
import ctypes as C
import os
import time
from typing import Dict, Iterator, List, Optional, Tuple

import numpy as np

from . import _lib
from .crisprhawk_error import CrisprHawkConverterError
from .exception_handlers import exception_handler
from .readers import BgzfWriter, _TextSource, inflate_route
from .utils import VERBOSITYLVL, print_verbosity

# gnomAD populations (9 superpopulations and 1 collecting minority samples), the reference's order (converter.py:19-30)
GNOMADPOPS = ["afr", "ami", "amr", "asj", "eas", "fin", "nfe", "mid", "sas", "remaining"]
GTLINE = '##FORMAT=<ID=GT,Number=1,Type=String,Description="Sample Collapsed Genotype">'
COLUMNS = ["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO"]

GN_DROPPED, GN_KEY_ABSENT, GN_BAD_VALUE, GN_FEW_FIELDS, GN_ALT_MISSING, GN_BAD_POS = 1, 2, 4, 8, 16, 32
_ABSENT = 0xFFFFFFFF


def format_ac(joint: bool) -> List[str]:
    """The allele-count key of every population (converter.py:99-112)."""
    return [f"AC_joint_{p}" if joint else f"AC_{p}" for p in GNOMADPOPS]


def batch_bytes() -> int:
    return max(1, int(os.environ.get("HAWK_GNOMAD_BATCH_BYTES", 256 << 20)))


def output_name(vcf_fname: str, suffix: str, outdir: str) -> str:
    """`<outdir>/<input basename minus its last two extensions>.<suffix>.vcf.gz` (converter.py:343-352)."""
    stem = os.path.splitext(os.path.splitext(os.path.basename(vcf_fname))[0])[0]
    return os.path.join(outdir, f"{stem}.{suffix}.vcf.gz")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _key_table(keys: List[str]) -> Tuple[np.ndarray, np.ndarray]:
    raw = [k.encode() for k in keys]
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in raw])
    return np.frombuffer(b"".join(raw), dtype=np.uint8).copy(), off


# ------------------------------------------------------------------------------------------------ reading
def _split_header(chunks: Iterator[Tuple[int, np.ndarray]]) -> Tuple[List[bytes], Iterator[np.ndarray]]:
    """The '#' lines at the head of the stream (without their line ends) and an iterator over the rest of the text."""
    buf, pos, header, done = b"", 0, [], False
    it = iter(chunks)
    while not done:
        try:
            _, chunk = next(it)
        except StopIteration:
            if pos < len(buf) and buf[pos] == 35:  # an unterminated last header line
                header.append(buf[pos:])
                pos = len(buf)
            break
        buf = buf[pos:] + chunk.tobytes()
        pos = 0
        while pos < len(buf):
            if buf[pos] != 35:
                done = True
                break
            nl = buf.find(b"\n", pos)
            if nl < 0:
                break
            header.append(buf[pos:nl])
            pos = nl + 1
    rest0 = np.frombuffer(buf[pos:], dtype=np.uint8)

    def rest():
        if len(rest0):
            yield rest0
        for _, chunk in it:
            yield chunk
    return header, rest()


def _find_nl(buf: np.ndarray, lo: int, hi: int, last: bool) -> int:
    """Index of the last (or first) '\\n' of buf[lo:hi], -1 without one; searched in windows so that nothing of the buffer's size
    is allocated."""
    W = 1 << 20
    if last:
        e = hi
        while e > lo:
            s = max(lo, e - W)
            hit = np.flatnonzero(buf[s:e] == 10)
            if len(hit):
                return s + int(hit[-1])
            e = s
    else:
        s = lo
        while s < hi:
            e = min(hi, s + W)
            hit = np.flatnonzero(buf[s:e] == 10)
            if len(hit):
                return s + int(hit[0])
            s = e
    return -1


def _batches(pieces_in: Iterator[np.ndarray], limit: int) -> Iterator[np.ndarray]:
    """Whole lines, at most `limit` bytes a batch; a record longer than that is a batch of its own.  The last line gets its
    '\\n' if the file lacks it."""
    nl1 = np.array([10], np.uint8)

    def drain(buf, final):
        start, n = 0, len(buf)
        while start < n:
            if n - start <= limit:
                if final:
                    yield buf[start:] if buf[n - 1] == 10 else np.concatenate((buf[start:], nl1))
                    start = n
                break
            nl = _find_nl(buf, start, start + limit, True)
            if nl < 0:  # the record at `start` is longer than a batch: up to its own line end
                nl = _find_nl(buf, start + limit, n, False)
                if nl < 0:
                    if final:
                        yield np.concatenate((buf[start:], nl1))
                        start = n
                    break
            yield buf[start:nl + 1]
            start = nl + 1
        return start

    pieces, total = [], 0
    for piece in pieces_in:
        pieces.append(piece)
        total += len(piece)
        if total <= limit:
            continue
        buf = pieces[0] if len(pieces) == 1 else np.concatenate(pieces)
        start = yield from drain(buf, False)
        rest = buf[start:]
        pieces, total = ([rest] if len(rest) else []), len(rest)
    if total:
        yield from drain(pieces[0] if len(pieces) == 1 else np.concatenate(pieces), True)


# ------------------------------------------------------------------------------------------------ one batch
class _Batch:
    """The per-record results of one batch and the means to turn them into lines: the device route or the host twin."""

    def __init__(self, text: np.ndarray, line_off: np.ndarray, keys: List[str], keep: bool, engine: str, device: Optional[int]):
        self.text, self.line_off, self.n = text, line_off, len(line_off) - 1
        self.kb, self.ko = _key_table(keys)
        self.nk, self.keep, self.engine, self.device = len(keys), int(bool(keep)), engine, device
        self.handle = None
        self.ms = {"upload_ms": 0.0, "scan_ms": 0.0, "len_ms": 0.0, "prefix_ms": 0.0, "fill_ms": 0.0}
        n = self.n
        self.mask = np.zeros(n, np.uint32)
        self.flags = np.zeros(n, np.uint8)
        self.fo = np.zeros((n, 8), np.uint32)
        self.qs = np.zeros((n, 2), np.uint32)
        self.afs = np.zeros((n, 2), np.uint32)

    def _host(self, pool, poff, blob, cap, off):
        nb, nk = C.c_uint64(0), C.c_uint64(0)
        rc = _lib.lib().hawk_host_gnomad_lines(_p(self.text), C.c_uint64(len(self.text)), _p(self.line_off), C.c_uint64(self.n), _p(self.kb),
                                               _p(self.ko), C.c_uint32(self.nk), C.c_int(self.keep), _p(self.mask), _p(self.flags), _p(self.fo),
                                               _p(self.qs), _p(self.afs), _p(pool), _p(poff), _p(blob), C.c_uint64(cap), _p(off),
                                               C.byref(nb), C.byref(nk))
        return rc, int(nb.value), int(nk.value)

    def scan(self) -> None:
        L = _lib.lib()
        if self.engine == "host":
            t0 = time.perf_counter()
            rc, _, _ = self._host(None, None, None, 0, None)
            _lib.check(rc, "hawk_host_gnomad_lines")
            self.ms["scan_ms"] = (time.perf_counter() - t0) * 1e3
            return
        h, tm = C.c_void_p(), _lib.GnomadTiming()
        _lib.check(L.hawk_gnomad_scan(_lib.context(self.device), _p(self.text), C.c_uint64(len(self.text)), _p(self.line_off), C.c_uint64(self.n),
                                      _p(self.kb), _p(self.ko), C.c_uint32(self.nk), C.c_int(self.keep), C.byref(h), C.byref(tm)), "hawk_gnomad_scan")
        self.handle = h
        self.ms["upload_ms"], self.ms["scan_ms"] = tm.upload_ms, tm.scan_ms
        _lib.check(L.hawk_gnomad_records(h, _p(self.mask), _p(self.flags), _p(self.fo), _p(self.qs), _p(self.afs)), "hawk_gnomad_records")

    def lines(self, pool: np.ndarray, poff: np.ndarray) -> Tuple[np.ndarray, int]:
        """(the kept records' lines, their number)"""
        L = _lib.lib()
        if self.engine == "host":
            t0 = time.perf_counter()
            rc, nb, nk = self._host(pool, poff, None, 0, None)
            if rc not in (_lib.HAWK_OK, _lib.HAWK_E_CAPACITY):
                _lib.check(rc, "hawk_host_gnomad_lines")
            blob = np.empty(max(nb, 1), np.uint8)
            rc, nb, nk = self._host(pool, poff, blob, nb, None)
            _lib.check(rc, "hawk_host_gnomad_lines")
            self.ms["fill_ms"] = (time.perf_counter() - t0) * 1e3
            return blob[:nb], nk
        nb, nk, tm = C.c_uint64(0), C.c_uint64(0), _lib.GnomadTiming()
        _lib.check(L.hawk_gnomad_text(self.handle, _p(pool), _p(poff), C.byref(nb), C.byref(nk), C.byref(tm)), "hawk_gnomad_text")
        self.ms["upload_ms"] += tm.upload_ms
        self.ms["len_ms"], self.ms["prefix_ms"], self.ms["fill_ms"] = tm.len_ms, tm.prefix_ms, tm.fill_ms
        blob = _lib.pinned_empty(max(int(nb.value), 1), np.uint8, self.device)
        _lib.check(L.hawk_gnomad_text_download(self.handle, _p(blob), None), "hawk_gnomad_text_download")
        return blob[:int(nb.value)], int(nk.value)

    def close(self) -> None:
        if self.handle is not None:
            _lib.lib().hawk_gnomad_destroy(self.handle)
            self.handle = None

    # -- what a record is called in a message: CHROM:POS, or the head of the line when it has no two fields
    def where(self, i: int) -> str:
        lo, end = int(self.line_off[i]), int(self.line_off[i + 1]) - 1
        parts = bytes(self.text[lo:min(end, lo + 4096)]).decode(errors="replace").split("\t")
        return f"{parts[0]}:{parts[1]}" if len(parts) > 2 else repr(parts[0][:40])


def f32_repr(text: np.ndarray, start: np.ndarray, length: np.ndarray, missing: str, threads: int):
    """hawk_host_f32_repr: (blob, off[n + 1], status[n])"""
    n = len(start)
    start = np.ascontiguousarray(start, dtype=np.uint64)
    length = np.ascontiguousarray(length, dtype=np.uint32)
    present = length != _ABSENT
    cap = int(13 * int(length[present].astype(np.int64).sum()) + 26 * n + 8)
    out, off, status = np.empty(cap, np.uint8), np.zeros(n + 1, np.uint64), np.zeros(max(n, 1), np.uint8)
    _lib.check(_lib.lib().hawk_host_f32_repr(_p(text), _p(start), _p(length), C.c_uint64(n), missing.encode(), _p(out), C.c_uint64(cap), _p(off),
                                             _p(status), C.c_uint32(max(0, threads))), "hawk_host_f32_repr")
    return out[:int(off[n])], off, status[:n]


_FLAG_TEXT = [(GN_FEW_FIELDS, "fewer than eight fields in record"), (GN_ALT_MISSING, "missing ALT (.) in record"),
              (GN_BAD_POS, "POS is not a number in record"), (GN_KEY_ABSENT, "Failed genotype assessment (allele count key absent) on variant"),
              (GN_BAD_VALUE, "Failed genotype assessment (allele count missing or not an integer) on variant")]


def _convert_batch(b: _Batch, threads: int, secs: Dict[str, float]) -> Tuple[np.ndarray, int, Optional[str]]:
    """(lines, kept records, None) or (None, 0, the message of the first record in error)"""
    b.scan()
    err = np.flatnonzero(b.flags & ~np.uint8(GN_DROPPED))
    first = int(err[0]) if len(err) else b.n  # the first record with a flag; a float in error before it comes first
    t0 = time.perf_counter()
    kept = np.flatnonzero(b.flags[:first] == 0)
    lo = b.line_off[:-1][kept]
    qblob, qoff, qst = f32_repr(b.text, lo + b.qs[kept, 0], b.qs[kept, 1], ".", threads)
    alen = b.afs[kept, 1]
    absent = alen == _ABSENT
    ablob, aoff, ast = f32_repr(b.text, np.where(absent, 0, lo + b.afs[kept, 0]), alen, "None", threads)
    badf = np.flatnonzero(qst | ast)
    if len(badf):
        k = int(badf[0])
        return None, 0, f"{'QUAL' if qst[k] else 'AF'} is not a finite decimal number in record {b.where(int(kept[k]))}"
    if first < b.n:
        what = next(t for f, t in _FLAG_TEXT if int(b.flags[first]) & f)
        return None, 0, f"{what} {b.where(first)}"
    pool = np.concatenate((qblob, ablob)) if len(kept) else np.zeros(0, np.uint8)
    poff = np.concatenate((qoff[:-1], aoff + qoff[-1])).astype(np.uint64) if len(kept) else np.zeros(1, np.uint64)
    secs["float_pool"] += time.perf_counter() - t0
    t0 = time.perf_counter()
    lines, nk = b.lines(pool, poff)
    secs["lines_call"] += time.perf_counter() - t0
    assert nk == len(kept)
    return lines, nk, None


# ------------------------------------------------------------------------------------------------ one file
def make_header(header_lines: List[bytes], joint: bool, fname: str, debug: bool) -> bytes:
    """The input's '##' lines, the GT FORMAT line, the column line with FORMAT and the populations (converter.py:129-145).
    htslib may regenerate or add header lines of its own (a PASS FILTER line, for one): unpinned."""
    meta = [ln.rstrip(b"\r") for ln in header_lines if ln.startswith(b"##")]
    cols = [ln.rstrip(b"\r") for ln in header_lines if not ln.startswith(b"##")]
    if len(cols) != 1 or not cols[0].startswith(b"#CHROM"):
        exception_handler(CrisprHawkConverterError, f"Input VCF {fname} has no #CHROM header line", os.EX_DATAERR, debug)
    fields = cols[0].decode().split("\t")
    if len(fields) > 8:
        exception_handler(CrisprHawkConverterError, f"Input VCF {fname} already has FORMAT / sample columns", os.EX_DATAERR, debug)
    if fields != COLUMNS:
        exception_handler(CrisprHawkConverterError, f"Input VCF {fname}: unexpected column line {cols[0].decode()!r}", os.EX_DATAERR, debug)
    text = b"".join(ln + b"\n" for ln in meta) + GTLINE.encode() + b"\n" + "\t".join(fields + ["FORMAT"] + GNOMADPOPS).encode() + b"\n"
    return text.replace(b"<ID=AF_joint,", b"<ID=AF,") if joint else text


def convert_vcf(vcf_fname: str, joint: bool, keep: bool, suffix: str, outdir: str, verbosity: int, debug: bool, engine: str = "device",
                device: Optional[int] = None, threads: int = 1, inflate: Optional[str] = None) -> dict:
    """One sites VCF (plain, gzip or BGZF) -> `<outdir>/<name>.<suffix>.vcf.gz` (BGZF, no index: the package's reader builds its
    own).  Returns {"path", "engine", "records", "kept", "timing"}; failures go through exception_handler as
    CrisprHawkConverterError / os.EX_DATAERR, and no temporary file survives one.  `inflate`: who inflates a BGZF input's members
    (readers.inflate_route: None reads HAWK_BGZF_INFLATE, default "zlib"); timing["inflate_route"] names it, and on "device"
    timing["inflate_ms"] is the sum of the kernel's laps."""
    if engine not in ("device", "host"):
        raise ValueError(f"engine must be 'device' or 'host', not {engine!r}")
    route = inflate_route(inflate)
    source = None
    print_verbosity(f"Converting VCF {os.path.basename(vcf_fname)}", verbosity, VERBOSITYLVL[2])
    t_start = time.perf_counter()
    if not os.path.isfile(vcf_fname):
        exception_handler(CrisprHawkConverterError, f"Failed loading VCF {vcf_fname}", os.EX_DATAERR, debug)
    if engine == "device" and _lib.device_count() == 0:
        raise _lib.HawkDeviceError("convert_vcf(engine='device'): no GPU visible")
    out_path = output_name(vcf_fname, suffix, outdir)
    tmp_path = os.path.join(outdir, f"{os.path.basename(out_path)[:-len('.vcf.gz')]}.tmp.vcf.gz")
    secs = {"inflate": 0.0, "float_pool": 0.0, "lines_call": 0.0, "deflate_write": 0.0}
    ms = {"upload_ms": 0.0, "scan_ms": 0.0, "len_ms": 0.0, "prefix_ms": 0.0, "fill_ms": 0.0}
    records = kept = n_batches = in_bytes = 0
    failure = None
    keys = format_ac(joint)
    limit = batch_bytes()

    def timed_chunks():
        nonlocal source
        source = _TextSource(vcf_fname, route, verbosity)
        it = source.chunks()
        while True:
            t0 = time.perf_counter()
            try:
                item = next(it)
            except StopIteration:
                return
            finally:
                secs["inflate"] += time.perf_counter() - t0
            yield item

    writer = None
    try:
        try:
            header, rest = _split_header(timed_chunks())
        except (OSError, EOFError, ValueError) as e:
            exception_handler(CrisprHawkConverterError, f"Failed loading VCF {vcf_fname}", os.EX_DATAERR, debug, e)
        head = make_header(header, joint, vcf_fname, debug)
        writer = BgzfWriter(tmp_path, threads)
        writer.write(head)
        for text in _batches(rest, limit):
            n_batches += 1
            in_bytes += len(text)
            if engine == "device":  # page-locked: the upload runs at link speed
                pin = _lib.pinned_empty(len(text), np.uint8, device)
                pin[:] = text
                text = pin
            else:
                text = np.ascontiguousarray(text)
            nl = np.flatnonzero(text == 10)
            line_off = np.zeros(len(nl) + 1, np.uint64)
            line_off[1:] = nl + 1
            b = _Batch(text, line_off, keys, keep, engine, device)
            try:
                lines, nk, failure = _convert_batch(b, threads, secs)
            finally:
                b.close()
            if failure:
                break
            for k in ms:
                ms[k] += b.ms[k]
            records += b.n
            kept += nk
            t0 = time.perf_counter()
            writer.write(lines)
            secs["deflate_write"] += time.perf_counter() - t0
        if not failure and kept == 0:
            failure = f"Empty converted VCF {out_path}"  # converter.py:259-265
        t0 = time.perf_counter()
        writer.close()
        writer = None
        secs["deflate_write"] += time.perf_counter() - t0
        if not failure:
            os.replace(tmp_path, out_path)
    finally:
        if writer is not None:
            writer.abort()
        if os.path.exists(tmp_path):
            os.remove(tmp_path)
    if failure:
        exception_handler(CrisprHawkConverterError, f"{failure} ({vcf_fname})", os.EX_DATAERR, debug)
    timing = dict(secs, **ms, total=time.perf_counter() - t_start, batches=n_batches, in_bytes=in_bytes, inflate_route=route)
    if route == "device":
        timing["inflate_ms"] = source.inflate_ms
    print_verbosity(f"{os.path.basename(vcf_fname)} converted in {timing['total']:.2f}s", verbosity, VERBOSITYLVL[3])
    return {"path": out_path, "engine": engine, "records": records, "kept": kept, "timing": timing}


def convert_gnomad_vcf(gnomad_vcfs: List[str], joint: bool, keep: bool, suffix: str, outdir: str, threads: int, verbosity: int,
                       debug: bool) -> None:
    """The reference's entry point (converter.py:363-413), same arguments.  The files are converted one after another in this
    process - a forked pool worker must not inherit an initialised device -; `threads` sizes the inflate, deflate and float
    helpers."""
    try:
        for fname in gnomad_vcfs:
            convert_vcf(fname, joint, keep, suffix, outdir, verbosity, debug, threads=max(1, int(threads)))
    except OSError as e:
        exception_handler(CrisprHawkConverterError, "GnomAD VCF conversion failed", os.EX_DATAERR, debug, e)
