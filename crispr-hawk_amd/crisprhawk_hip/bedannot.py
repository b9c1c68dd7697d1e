"""BED annotation files without pysam and without .tbi files, and their join with guides / off-target sites on the device.

Reference: `BedAnnotation` (`bedfile.py:315-429`: pysam.TabixFile over a tabix-indexed BED) and its three callers, which do
one `fetch_features` and one Python join per row (`annotation.py:373-462`, `offtargets.py:407-483`).  Here one streaming pass
over the text (plain, gzip or BGZF through `readers._TextSource`, as the VCF reader indexes its file) leaves, per contig and in
file order, `start` / `end` (int64) and the two labels a feature can contribute, each kind as one byte blob + offsets:

    FUNC  line.split()[3]                              (annotation.py:401, offtargets.py:444)
    GENE  f"{fields[7]}:{gene_name}"                   (annotation.py:406-419, 450-457)

`AnnotTable` puts one (contig, kind) into HBM (`hawk_annot_create`) and answers whole batches of intervals
(`hawk_annot_query`): per row the labels of the overlapping features joined by ',' in file order, or `NA`, as a `reports.Ragged`.
Overlap is tabix's rule, 0-based half-open on both sides: `fs < qe and fe > qs` (parity unpinned: pysam absent).

Kept divergences: a file whose features of one contig are not sorted by start, a line with fewer columns than the
requested label needs, and `end < start` raise CrisprHawkAnnotationError - tabix cannot index the first, the reference's label
expressions die with an IndexError on the second, and tabix mis-indexes the third.
"""
import ctypes as C
import os
from typing import Dict, List, Optional, Tuple

import numpy as np

from .crisprhawk_error import CrisprHawkAnnotationError
from .exception_handlers import exception_handler

FUNC, GENE = 0, 1  # ann_guides' atype
_MINCOLS = {FUNC: 4, GENE: 10}
_SKIP = (b"#", b"track", b"browser")  # what tabix's bed preset passes over, besides empty lines


def gene_name(field: str) -> str:
    """The gene name the reference takes from a GENCODE-style attribute column (annotation.py:406-419): the text between
    `gene_name=` and the next `;`.  Absent -> ''; as the LAST attribute without a closing `;` the reference's slice ends at
    find() = -1, i.e. it loses the name's last character - kept, the report is compared byte for byte."""
    i = field.find("gene_name=")
    if i < 0:
        return ""
    return field[i + 10:field.find(";", i + 10)]


class _Contig:
    __slots__ = ("start", "end", "lo", "hi", "labels")

    def __init__(self):
        self.start, self.end, self.lo, self.hi = [], [], [], []
        self.labels = {FUNC: [], GENE: []}


class BedAnnotation:
    """bedfile.py:315-429 with the reference's constructor.  `features(contig, kind)` is what the device table is made of;
    `fetch_features(contig, start, stop)` has the reference's meaning (the overlapping lines in file order, None for a contig
    the file does not have) and is the host-side statement of the overlap rule."""

    def __init__(self, fname: str, verbosity: int = 0, debug: bool = True, inflate: Optional[str] = None) -> None:
        from .readers import _TextSource
        self._fname, self._verbosity, self._debug = fname, verbosity, debug
        try:
            self._src = _TextSource(fname, inflate, verbosity)  # `inflate`: who inflates a BGZF file's members (readers.inflate_route)
        except OSError as e:
            exception_handler(CrisprHawkAnnotationError, f"Cannot read annotation BED {fname}", os.EX_DATAERR, debug, e)
        self._contigs: Dict[str, _Contig] = {}
        self._short = {FUNC: None, GENE: None}  # first line (1-based) with too few columns for the kind
        self._arrays: Dict[Tuple[str, int], tuple] = {}
        self._tables: Dict[Tuple[str, int, Optional[int]], "AnnotTable"] = {}
        self._parse()

    # -------------------------------------------------------------------------------------------- the one pass
    def _parse(self) -> None:
        tail, tail_off, linenum = b"", 0, 0
        for off, chunk in self._src.chunks():
            data = tail + chunk.tobytes()
            base = off - len(tail)
            lines = data.split(b"\n")
            tail = lines.pop()
            pos = base
            for ln in lines:
                linenum += 1
                self._line(ln, pos, linenum)
                pos += len(ln) + 1
            tail_off = pos
        if tail:
            self._line(tail, tail_off, linenum + 1)

    def _line(self, raw: bytes, pos: int, linenum: int) -> None:
        text = raw.strip()
        if not text or text.startswith(_SKIP):
            return
        fields = text.decode("ascii", "replace").split()
        try:
            contig, start, end = fields[0], int(fields[1]), int(fields[2])
        except (IndexError, ValueError) as e:
            exception_handler(CrisprHawkAnnotationError, f"{self._fname}: line {linenum} is not a BED feature", os.EX_DATAERR, self._debug, e)
        if end < start:
            exception_handler(CrisprHawkAnnotationError, f"{self._fname}: end < start ({end} < {start}) at line {linenum}", os.EX_DATAERR,
                              self._debug)
        c = self._contigs.get(contig)
        if c is None:
            c = self._contigs[contig] = _Contig()
        elif start < c.start[-1]:
            exception_handler(CrisprHawkAnnotationError,
                              f"{self._fname}: features of {contig} are not sorted by start (line {linenum}): tabix cannot index this file",
                              os.EX_DATAERR, self._debug)
        c.start.append(start)
        c.end.append(end)
        c.lo.append(pos)
        c.hi.append(pos + len(raw))
        for kind in (FUNC, GENE):
            if len(fields) < _MINCOLS[kind]:
                if self._short[kind] is None:
                    self._short[kind] = linenum
                c.labels[kind].append("")
            else:
                c.labels[kind].append(fields[3] if kind == FUNC else f"{fields[7]}:{gene_name(fields[9])}")

    # -------------------------------------------------------------------------------------------- what callers read
    @property
    def contigs(self) -> List[str]:
        return list(self._contigs)

    def require(self, kind: int) -> None:
        """Raise unless every feature line has the columns label `kind` needs (4, or 10 for genes)."""
        if self._short[kind] is not None:
            exception_handler(CrisprHawkAnnotationError,
                              f"{self._fname}: line {self._short[kind]} has fewer than {_MINCOLS[kind]} columns "
                              f"({'gene ' if kind == GENE else ''}annotation label)", os.EX_DATAERR, self._debug)

    def features(self, contig: str, kind: int = FUNC):
        """(start int64[n], end int64[n], label blob uint8[], label offsets uint64[n + 1]) of a contig in file order; n = 0 for
        a contig the file does not have."""
        self.require(kind)
        key = (contig, kind)
        hit = self._arrays.get(key)
        if hit is None:
            c = self._contigs.get(contig)
            if c is None:
                hit = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint8), np.zeros(1, np.uint64))
            else:
                lab = [s.encode("ascii", "replace") for s in c.labels[kind]]
                off = np.zeros(len(lab) + 1, dtype=np.uint64)
                np.cumsum([len(b) for b in lab], out=off[1:])
                hit = (np.array(c.start, dtype=np.int64), np.array(c.end, dtype=np.int64), np.frombuffer(b"".join(lab), dtype=np.uint8), off)
            self._arrays[key] = hit
        return hit

    def fetch_features(self, contig: str, start: int, stop: int) -> Optional[List[str]]:
        c = self._contigs.get(contig)
        if c is None:
            return None
        return [self._src.read(c.lo[i], c.hi[i]).tobytes().decode("ascii", "replace").strip()
                for i in range(len(c.start)) if c.start[i] < stop and c.end[i] > start]

    def table(self, contig: str, kind: int = FUNC, device: Optional[int] = None) -> "AnnotTable":
        """The device table of (contig, kind), made once and kept until close()."""
        key = (contig, kind, device)
        t = self._tables.get(key)
        if t is None:
            t = self._tables[key] = AnnotTable(*self.features(contig, kind), device=device)
        return t

    def close(self) -> None:
        for t in self._tables.values():
            t.close()
        self._tables.clear()


class AnnotTable:
    """The features of one (file, contig, label kind) in HBM (include/hawk.h: hawk_annot_*).  There is no host path: without
    the library or a device this raises like every other entry point of the package."""

    def __init__(self, start, end, label_blob, label_off, device: Optional[int] = None):
        from . import _lib
        self._L = _lib.lib()
        start = np.ascontiguousarray(start, dtype=np.int64)
        end = np.ascontiguousarray(end, dtype=np.int64)
        label_blob = np.ascontiguousarray(label_blob, dtype=np.uint8)
        label_off = np.ascontiguousarray(label_off, dtype=np.uint64)
        if len(end) != len(start) or len(label_off) != len(start) + 1:
            raise ValueError("AnnotTable: start, end and label_off[n + 1] disagree on n")
        self.n = len(start)
        self._device = device
        self._h = C.c_void_p()
        ms = C.c_float(0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(self._L.hawk_annot_create(_lib.context(device), p(start), p(end), p(label_blob), p(label_off), C.c_uint64(self.n),
                                             C.byref(self._h), C.byref(ms)), "hawk_annot_create")
        self.index_ms = float(ms.value)
        self.timing: Dict[str, float] = {}
        self.n_overlaps = 0

    def query(self, qstart, qstop):
        """Ragged column: row q = labels of the features overlapping [qstart[q], qstop[q]) joined by ',', or NA."""
        from . import _lib
        from .reports import Ragged
        if self._h is None:
            raise ValueError("AnnotTable.query on a closed table")
        qs = np.ascontiguousarray(qstart, dtype=np.int64)
        qe = np.ascontiguousarray(qstop, dtype=np.int64)
        if qs.shape != qe.shape or qs.ndim != 1:
            raise ValueError("AnnotTable.query: qstart and qstop must be 1-d arrays of one length")
        nq = len(qs)
        nbytes, nov, tm, dl = C.c_uint64(0), C.c_uint64(0), _lib.AnnotTiming(), C.c_float(0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(self._L.hawk_annot_query(self._h, p(qs), p(qe), C.c_uint64(nq), C.byref(nbytes), C.byref(nov), C.byref(tm)), "hawk_annot_query")
        # the rows come down into page-locked blocks of the package's cache (_lib.pinned_empty: plain numpy when they are small)
        o = _lib.pinned_empty(nq + 1, np.uint64, self._device)
        b = _lib.pinned_empty(int(nbytes.value), np.uint8, self._device)
        _lib.check(self._L.hawk_annot_download(self._h, p(b), p(o), C.byref(dl)), "hawk_annot_download")
        self.n_overlaps = int(nov.value)
        self.timing = {k: float(getattr(tm, k)) for k in ("upload_ms", "count_ms", "scan_ms", "fill_ms")}
        self.timing["download_ms"] = float(dl.value)
        self.timing["total_ms"] = float(tm.total_ms) + float(dl.value)
        self.timing["out_bytes"], self.timing["walk_steps"] = int(nbytes.value), int(tm.walk_steps)
        return Ragged(b, o)

    def close(self) -> None:
        if self._h is not None and self._h.value:
            self._L.hawk_annot_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def plain_labels(col) -> bool:
    """no byte of a Ragged column is one csv's minimal quoting reacts to (a quote, a tab, a line break)"""
    b = col.blob
    return not bool(np.isin(b, np.frombuffer(b'"\t\n\r', dtype=np.uint8)).any()) if len(b) else True
