"""Reference for the off-targets table written from hit records (hawk_offtarget_text / hawk_host_offtarget_text).

A record {guide, row, q, strand, mm, code, nmask, gaps, kind, size} is turned into the (crRNA, DNA, PAM) strings by a pure-Python
mirror of GenomeIndex._bulge_hit; the expected row text then comes through the package's own host chain - crispritz_report_line /
crispritz_bulge_line -> Offtarget -> the oracle's compute_cfd -> set_cfd -> offtargets_table - which test_oracle_golden holds to
the reference on fixture g10.  Nothing here knows how the emitter under test works."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

from crisprhawk_hip import _lib
from crisprhawk_hip.genome import BulgeHit, OffTargetHit, decode_window, encode_guides
from crisprhawk_hip.offtarget import Offtarget
from crisprhawk_hip.offtargets import OTREPCNAMES, crispritz_bulge_line, crispritz_report_line, offtargets_table
from oracle import oracle as ora

COLUMNS = (("guide", np.uint32), ("row", np.uint32), ("q", np.uint32), ("strand", np.uint8), ("mm", np.uint8), ("code", np.uint64),
           ("nmask", np.uint32), ("gaps", np.uint64), ("kind", np.uint8), ("size", np.uint8))
KINDS = ("X", "DNA", "RNA")


def encode_window(win: str):
    """(code, nmask) of a window in guide orientation (any case; anything but ACGT is ambiguous)"""
    code = nmask = 0
    for i, ch in enumerate(win.upper()):
        k = "ACGT".find(ch)
        if k < 0:
            nmask |= 1 << i
        else:
            code |= k << (2 * i)
    return code, nmask


def columns(records):
    """list of dicts -> the ten columns"""
    return {k: np.array([r[k] for r in records], dtype=t) for k, t in COLUMNS}


def site_len(G: int, kind: int, size: int) -> int:
    return G + size if kind == 1 else G - size if kind == 2 else G


def record_strings(rec, guide: str, P: int, right: bool):
    """(crRNA spacer, DNA spacer, site PAM) of a record: '-' where the other string has no partner, mismatches of the DNA in
    lower case (N -> n), a DNA-bulged base as it is - GenomeIndex._bulge_hit; for kind 0 what crispritz_report_line makes."""
    G, kind, size, gaps = len(guide), int(rec["kind"]), int(rec["size"]), int(rec["gaps"])
    Gs = site_len(G, kind, size)
    win = decode_window(int(rec["code"]), int(rec["nmask"]), Gs + P)
    sp_site = win[P:] if right else win[:Gs]
    pam_site = win[:P] if right else win[Gs:]
    cr, dn = [], []
    si = gi = 0
    while si < Gs or gi < G:
        if kind == 1 and si < Gs and (gaps >> si) & 1:
            cr.append("-"); dn.append(sp_site[si]); si += 1
        elif kind == 2 and gi < G and (gaps >> gi) & 1:
            cr.append(guide[gi]); dn.append("-"); gi += 1
        else:
            t, q = sp_site[si], guide[gi]
            cr.append(q); dn.append(t if t == q else t.lower())
            si += 1; gi += 1
    return "".join(cr), "".join(dn), pam_site


def expected(cols, guides, pam_text: str, right: bool, row_names, row_offsets, tables=None):
    """The expected result for the records `cols` in input order: (row texts without newline, CFD units int64 (-1: NA or
    unscorable), number of unscorable rows).  tables = (mm[20,4,4], pam[16]) or None."""
    P = len(pam_text)
    n = len(cols["guide"])
    rows, units, n_uns = [], np.full(n, -1, dtype=np.int64), 0
    for i in range(n):
        rec = {k: cols[k][i] for k, _t in COLUMNS}
        g = guides[int(rec["guide"])]
        name, pos = row_names[int(rec["row"])], int(row_offsets[int(rec["row"])]) + int(rec["q"])
        strand = "-" if rec["strand"] else "+"
        if int(rec["kind"]) == 0:
            hit = OffTargetHit(int(rec["guide"]), name, pos, strand, int(rec["mm"]), decode_window(int(rec["code"]), int(rec["nmask"]), len(g) + P))
            line = crispritz_report_line(hit, g, P, right)
        else:
            cr, dn, pm = record_strings(rec, g, P, right)
            hit = BulgeHit(int(rec["guide"]), name, pos, strand, int(rec["mm"]), KINDS[int(rec["kind"])], int(rec["size"]), cr, dn, pm, int(rec["gaps"]))
            line = crispritz_bulge_line(hit, P, right)
        ot = Offtarget(line, pam_text, right, True)
        if tables is not None:
            try:
                ot.set_cfd(ora.cfd(*ot.cfd_inputs(), tables[0], tables[1]))
                units[i] = int(round(float(ot.cfd) * 1e4))
            except ora.OracleError:
                n_uns += 1
        text = offtargets_table([ot])  # header, the row, a trailing newline
        head, row, tail = text.split("\n")
        assert head == "\t".join(OTREPCNAMES) and tail == ""
        rows.append(row)
    return rows, units, n_uns


def ragged_rows(blob, off):
    b = bytes(np.asarray(blob, dtype=np.uint8)[: int(off[-1])])
    return [b[int(off[i]):int(off[i + 1])].decode("ascii") for i in range(len(off) - 1)]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def call_args(cols, guides, G: int, pam_text: str, right: bool, row_contig, row_off, names, order=None, tables=None):
    """the argument list hawk_offtarget_text and hawk_host_offtarget_text share, from `n` to `cfd_pam`, and what it points into"""
    n = len(cols["guide"])
    a = {k: np.ascontiguousarray(cols[k], dtype=t) for k, t in COLUMNS}
    g2 = encode_guides(list(guides)) if len(guides) else np.zeros(0, np.uint64)
    par = _lib.OtParams(0, 0, len(pam_text), G, int(bool(right)), 0)
    rc = np.ascontiguousarray(row_contig, dtype=np.uint32)
    ro = np.ascontiguousarray(row_off, dtype=np.uint64)
    enc = [s.encode("ascii") for s in names]
    noff = np.zeros(len(enc) + 1, dtype=np.uint64)
    np.cumsum([len(b) for b in enc], out=noff[1:])
    nblob = np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8).copy()
    od = None if order is None else np.ascontiguousarray(order, dtype=np.uint64)
    mm = pt = None
    if tables is not None:
        mm = np.ascontiguousarray(tables[0], dtype=np.float64).reshape(20, 4, 4)
        pt = np.ascontiguousarray(tables[1], dtype=np.float64).reshape(16)
    keep = SimpleNamespace(a=a, g2=g2, par=par, rc=rc, ro=ro, nblob=nblob, noff=noff, od=od, mm=mm, pt=pt, pam=pam_text.encode("ascii"))
    args = [C.c_uint64(n)] + [_p(a[k]) for k in ("guide", "row", "q", "strand", "mm", "code", "nmask", "gaps", "kind", "size")] + \
        [_p(g2), C.c_uint32(len(g2)), C.byref(par), _p(rc), _p(ro), C.c_uint32(len(rc)), _p(nblob), _p(noff), C.c_uint32(len(enc)), keep.pam,
         _p(od), _p(mm), _p(pt)]
    return args, keep


def host_text(cols, guides, G: int, pam_text: str, right: bool, row_contig, row_off, names, order=None, tables=None):
    """hawk_host_offtarget_text: (status, rows, off uint64[n + 1], cfd units int64[n], n_unscorable)"""
    L = _lib.lib()
    n = len(cols["guide"])
    args, keep = call_args(cols, guides, G, pam_text, right, row_contig, row_off, names, order, tables)
    off = np.full(n + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    cfd = np.full(n, -7, dtype=np.int64)
    nb, nu = C.c_uint64(0), C.c_uint64(0)
    rc = L.hawk_host_offtarget_text(*args, None, C.c_uint64(0), _p(off), _p(cfd), C.byref(nb), C.byref(nu))
    if rc not in (_lib.HAWK_OK, _lib.HAWK_E_CAPACITY):
        return rc, None, off, cfd, 0
    blob = np.zeros(max(int(nb.value), 1), dtype=np.uint8)
    rc = L.hawk_host_offtarget_text(*args, _p(blob), C.c_uint64(int(nb.value)), _p(off), _p(cfd), C.byref(nb), C.byref(nu))
    return rc, ragged_rows(blob, off), off, cfd, int(nu.value)


def device_text(cols, guides, G: int, pam_text: str, right: bool, row_contig, row_off, names, order=None, tables=None, device=None):
    """hawk_offtarget_text + hawk_offtarget_text_download: (status, blob, off, cfd units, n_unscorable, n_bytes)"""
    L, ctx = _lib.lib(), _lib.context(device)
    n = len(cols["guide"])
    args, keep = call_args(cols, guides, G, pam_text, right, row_contig, row_off, names, order, tables)
    nb, nu, tm = C.c_uint64(0xDEAD), C.c_uint64(0xDEAD), _lib.OtTextTiming()
    rc = L.hawk_offtarget_text(ctx, *args, C.byref(nb), C.byref(nu), C.byref(tm))
    if rc != _lib.HAWK_OK:
        return rc, None, None, None, int(nu.value), int(nb.value)
    off = np.full(n + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    cfd = np.full(n, -7, dtype=np.int64)
    blob = np.full(int(nb.value) + 32, 0xAA, dtype=np.uint8)  # 32 guard bytes behind the blob
    _lib.check(L.hawk_offtarget_text_download(ctx, _p(blob), _p(off), _p(cfd), None), "hawk_offtarget_text_download")
    assert (blob[int(nb.value):] == 0xAA).all()
    return rc, blob[: int(nb.value)], off, cfd, int(nu.value), int(nb.value)


# ---- fixture g10: records from the lines of a CRISPRitz targets.txt -------------------------------------------------------
def records_from_targets(targets_txt: str, pam_text: str, right: bool):
    """Every line of a targets.txt -> a record over one genome row per contig (offset 0, q = position), with the guides and
    contigs it names: (columns, guides, names).  The windows and the bulge positions are recovered from the two strings: a '-'
    in the crRNA is a DNA bulge (bit = the site spacer's position), a '-' in the DNA an RNA bulge (bit = the guide's position)."""
    P = len(pam_text)
    lines = targets_txt.splitlines()[1:]
    guides, names, recs = [], [], []
    for ln in lines:
        f = ln.split()
        cr = f[1][P:] if right else f[1][: len(f[1]) - P]
        dn = f[2][P:] if right else f[2][: len(f[2]) - P]
        pm = f[2][:P] if right else f[2][len(f[2]) - P:]
        assert len(cr) == len(dn)
        g = cr.replace("-", "")
        if g not in guides:
            guides.append(g)
        if f[3] not in names:
            names.append(f[3])
        kind = KINDS.index(f[0])
        gaps, si, gi = 0, 0, 0
        for a, b in zip(cr, dn):
            if a == "-":
                gaps |= 1 << si
                si += 1
            elif b == "-":
                gaps |= 1 << gi
                gi += 1
            else:
                si += 1
                gi += 1
        site = dn.replace("-", "")
        code, nmask = encode_window(pm + site if right else site + pm)
        recs.append(dict(guide=guides.index(g), row=names.index(f[3]), q=int(f[4]), strand=int(f[6] == "-"), mm=int(f[7]), code=code,
                         nmask=nmask, gaps=gaps, kind=kind, size=int(f[8])))
    return columns(recs), guides, names


# ---- fabricated records ---------------------------------------------------------------------------------------------------
def make_record(guide_idx: int, guide: str, site: str, pam_site: str, right: bool, kind: int = 0, gaps: int = 0, row: int = 0, q: int = 0,
                strand: int = 0, mm=None):
    """A record whose window is `site` (the site's spacer, N allowed) with `pam_site`; mm defaults to the mismatches among the
    paired bases (an ambiguous base counts)."""
    size = bin(gaps).count("1")
    assert len(site) == site_len(len(guide), kind, size)
    code, nmask = encode_window(pam_site + site if right else site + pam_site)
    if mm is None:
        rec = dict(code=code, nmask=nmask, gaps=gaps, kind=kind, size=size)
        cr, dn, _pm = record_strings(rec, guide, len(pam_site), right)
        mm = sum(1 for a, b in zip(cr, dn) if a != "-" and b != "-" and a != b)
    return dict(guide=guide_idx, row=row, q=q, strand=strand, mm=mm, code=code, nmask=nmask, gaps=gaps, kind=kind, size=size)


def random_records(rng, n: int, guides, P: int, right: bool, n_rows: int, p_n: float = 0.02, max_q: int = 1 << 31):
    """n records of every kind and size over random windows (a base is N with probability p_n, bulged DNA bases included: the
    emitter takes any valid record), random interior gaps, both strands"""
    G = len(guides[0])
    recs = []
    for _ in range(n):
        kind = int(rng.integers(0, 3))
        size = 0 if kind == 0 else int(rng.integers(1, 3))
        Gs = site_len(G, kind, size)
        span = Gs if kind == 1 else G
        gaps = sum(1 << int(b) for b in rng.choice(np.arange(1, span - 1), size=size, replace=False)) if size else 0
        gi = int(rng.integers(0, len(guides)))
        # a site near the guide: the paired bases copied, a few changed
        letters = rng.choice(list("ACGT"), size=Gs + P)
        site = list(letters[:Gs])
        si = g = 0
        while si < Gs and g < G:
            if kind == 1 and (gaps >> si) & 1:
                si += 1
            elif kind == 2 and (gaps >> g) & 1:
                g += 1
            else:
                if rng.random() < 0.8:
                    site[si] = guides[gi][g]
                si += 1; g += 1
        pam_site = list(letters[Gs:])
        for arr in (site, pam_site):
            for k in range(len(arr)):
                if rng.random() < p_n:
                    arr[k] = "N"
        recs.append(make_record(gi, guides[gi], "".join(site), "".join(pam_site), right, kind, gaps, int(rng.integers(0, n_rows)),
                                int(rng.integers(0, max_q)), int(rng.integers(0, 2))))
    return recs


def malformed_cases(G: int = 20, P: int = 3):
    """(what, changes to a valid DNA-bulge record / call) that hawk_offtarget_text and its host twin refuse"""
    return [("kind out of range", dict(kind=3)), ("size out of range", dict(size=3, gaps=0b1110)), ("a bulge without size", dict(size=0, gaps=0)),
            ("a size without bulge", dict(kind=0, gaps=0)), ("gaps at position 0", dict(gaps=0b1)),
            ("gaps at the last position", dict(gaps=1 << (G + 1 - 1))), ("gaps beyond the span", dict(gaps=1 << 40)),
            ("popcount above size", dict(gaps=0b110)), ("popcount below size", dict(gaps=0)), ("RNA gap at the guide's last base", dict(kind=2, gaps=1 << (G - 1))),
            ("row beyond the table", dict(row=2)), ("guide beyond the guides", dict(guide=1))]


def valid_dna_record(guide):
    site = guide[:5] + "T" + guide[5:]
    return make_record(0, guide, site, "TGG", False, kind=1, gaps=1 << 5, q=7)
