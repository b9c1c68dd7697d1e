"""Haplotype-set construction for a synthetic (or VCF-derived) phased panel.

Mirrors the reference's reconstruct_haplotypes() phased branch (haplotypes.py:132-159,
297-368, 232-294): REF first, then per sample chromosome copy 0 / copy 1 (one entry with
``1|1`` when both copies give the same sequence), identical cased sequences collapsed keeping
the first member's position map.  Used by bench.py and the tests to build the resident input of
the search kernels; the search itself is hawk_search().
"""

import hashlib
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .expand import expand_haplotype, scan_bounds, scan_start, scan_stop
from .hapset import HostHaplotype, PosSegments
from .synth import SynthRegion


class HapInfo:
    """Host-side labels of one device haplotype (what Guide rows inherit from it).  `variant_idx` may be given as a callable:
    the carried-variant lists of a device-built plan stay in HBM until a label is asked for (CarriedLists)."""

    __slots__ = ("samples", "_v")

    def __init__(self, samples: List[str], variant_idx):
        self.samples = samples
        self._v = variant_idx

    @property
    def variant_idx(self):
        if callable(self._v):
            self._v = self._v()
        return self._v


class CarriedLists:
    """The carried-variant lists of a genotype inversion (hawk_gt_lists), left on the device: `idx` downloads the variant
    indices once, when something on the host (a report label) first asks, and releases the device object."""

    def __init__(self, g, n_entries: int):
        self._g, self._n, self._idx = g, int(n_entries), None

    @property
    def idx(self) -> np.ndarray:
        if self._idx is None:
            import ctypes as C
            from . import _lib
            from .hapset import _p
            out = np.zeros(max(self._n, 1), dtype=np.uint32)
            _lib.check(_lib.lib().hawk_gt_lists_download(self._g, _p(out), None), "hawk_gt_lists_download")
            self._idx = out[:self._n]
            self.close()
        return self._idx

    def rows(self, a: int, b: int):
        return lambda: self.idx[a:b]

    def close(self) -> None:
        if self._g is not None:
            from . import _lib
            _lib.lib().hawk_gt_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _digest(arr: np.ndarray) -> bytes:
    return hashlib.blake2b(arr.tobytes(), digest_size=16).digest()


def build_phased_haplotypes(reg: SynthRegion, pamlen: int, max_haplotypes: Optional[int] = None,
                            sample_slice: Optional[slice] = None) -> Tuple[List[HostHaplotype], List[HapInfo]]:
    ref = np.frombuffer(reg.sequence.encode("ascii"), dtype=np.uint8)
    startp, stopp = reg.startp, reg.stopp
    haps: List[HostHaplotype] = [HostHaplotype(ref, PosSegments.identity(startp, len(ref)), True,
                                               scan_bounds(PosSegments.identity(startp, len(ref)), startp, stopp, pamlen))]
    info: List[HapInfo] = [HapInfo(["REF"], ())]
    if not reg.variants:
        return haps, info
    site = [(v.pos, v.ref.encode(), v.alt.encode()) for v in reg.variants]
    G = np.stack([v.gt.reshape(-1) for v in reg.variants])  # [site, 2*sample]
    index: Dict[bytes, int] = {_digest(ref): 0}
    samples = range(len(reg.samples))
    if sample_slice is not None:
        samples = samples[sample_slice]
    for si in samples:
        name = reg.samples[si]
        built = []
        for c in (0, 1):
            idx = np.flatnonzero(G[:, 2 * si + c])
            if len(idx) == 0:
                built.append((ref, PosSegments.identity(startp, len(ref)), ()))
            else:
                arr, seg = expand_haplotype(ref, startp, [site[k] for k in idx])
                built.append((arr, seg, tuple(int(k) for k in idx)))
        if not built[0][2] and not built[1][2]:
            continue  # sample carries no variant in this region (haplotypes.py:157)
        homo = len(built[0][0]) == len(built[1][0]) and np.array_equal(built[0][0], built[1][0])
        entries = [(built[0], f"{name}:1|1")] if homo else [(built[0], f"{name}:1|0"), (built[1], f"{name}:0|1")]
        for (arr, seg, vidx), label in entries:
            d = _digest(arr)
            j = index.get(d)
            if j is not None:
                if j != 0:  # collapsing onto REF keeps samples == "REF" (haplotypes.py:255-258)
                    info[j].samples.append(label)
                continue
            index[d] = len(haps)
            haps.append(HostHaplotype(arr, seg, False, scan_bounds(seg, startp, stopp, pamlen)))
            info.append(HapInfo([label], vidx))
            if max_haplotypes is not None and len(haps) >= max_haplotypes:
                return haps, info
    return haps, info


# ---------------------------------------------------------------------------------------------
# the same haplotype set, expanded on the device
# ---------------------------------------------------------------------------------------------
_NIB = np.zeros(256, dtype=np.uint8)
for _c, _v in {"A": 1, "C": 2, "G": 4, "T": 8, "N": 15, "R": 5, "Y": 10, "S": 6, "W": 9, "K": 12, "M": 3, "B": 14, "D": 13,
               "H": 11, "V": 7}.items():
    _NIB[ord(_c)] = _v
    _NIB[ord(_c.lower())] = _v


def _variant_table(pos: np.ndarray, refs: List[str], alts: List[str], seq: str, startp: int):
    """Per-variant arrays the expansion kernels index with (validated against the reference string)."""
    from .expand import HaplotypeBuildError
    n_ref = len(seq)
    nv = len(refs)
    r0 = np.asarray(pos, dtype=np.int64) - startp
    reflen = np.array([len(x) for x in refs], dtype=np.int64)
    altlen = np.array([len(x) for x in alts], dtype=np.int64)
    if np.any(np.diff(r0) < 0):
        raise HaplotypeBuildError("variants must be sorted by position")
    # replaced span as the reference computes it (haplotype.py:197-201): |chain|+1 for deletions, else 1
    chain = altlen - reflen
    span = np.where(chain < 0, -chain + 1, 1)
    if np.any((chain < 0) & (altlen != 1)) or np.any((chain == 0) & (reflen != 1)):
        raise HaplotypeBuildError("device expansion handles SNVs, deletions (alt of one base) and insertions")
    if np.any(r0 < 0) or np.any(r0 + span > n_ref):
        raise HaplotypeBuildError("variant outside the region")
    # REF allele must match (haplotype.py:203-208): its first base for all records at once, the rest of a deletion's
    # span (the few records with span > 1) one by one
    if nv:
        seq_u8 = np.frombuffer(seq.encode("ascii"), dtype=np.uint8) if isinstance(seq, str) else np.asarray(seq, dtype=np.uint8)
        first = np.frombuffer("".join(x[:1] or "\0" for x in refs).encode("ascii"), dtype=np.uint8)
        bad = np.flatnonzero(((seq_u8[r0] ^ first) & 0xDF) != 0)  # case-insensitive (letters only)
        if len(bad):
            raise HaplotypeBuildError(f"Mismatching reference alleles at position {int(pos[int(bad[0])])}")
        for i in np.flatnonzero(span > 1).tolist():
            a, sp = int(r0[i]), int(span[i])
            if len(refs[i]) < sp or seq[a:a + sp].upper() != refs[i][:sp].upper():
                raise HaplotypeBuildError(f"Mismatching reference alleles at position {int(pos[i])}")
    alt_blob = "".join(alts).encode("ascii")
    alt_codes = _NIB[np.frombuffer(alt_blob, dtype=np.uint8)] if alt_blob else np.zeros(0, np.uint8)
    alt_off = np.zeros(nv, dtype=np.int64)
    if nv:
        alt_off[1:] = np.cumsum(altlen)[:-1]
    return r0, span, chain, altlen, alt_off, alt_codes


def _variant_table_columns(cols, seq, startp: int):
    """_variant_table from records held as columns (SynthRegion.variant_columns): the same arrays and the same checks,
    without a Python step per record."""
    from .expand import HaplotypeBuildError
    n_ref = len(seq)
    pos = np.asarray(cols["pos"], dtype=np.int64)
    nv = len(pos)
    ref_off, alt_off_all = np.asarray(cols["ref_off"], dtype=np.int64), np.asarray(cols["alt_off"], dtype=np.int64)
    reflen, altlen = np.diff(ref_off), np.diff(alt_off_all)
    r0 = pos - startp
    if np.any(np.diff(r0) < 0):
        raise HaplotypeBuildError("variants must be sorted by position")
    chain = altlen - reflen
    span = np.where(chain < 0, -chain + 1, 1)
    if np.any((chain < 0) & (altlen != 1)) or np.any((chain == 0) & (reflen != 1)):
        raise HaplotypeBuildError("device expansion handles SNVs, deletions (alt of one base) and insertions")
    if np.any(r0 < 0) or np.any(r0 + span > n_ref):
        raise HaplotypeBuildError("variant outside the region")
    if nv:
        seq_u8 = np.frombuffer(seq.encode("ascii"), dtype=np.uint8) if isinstance(seq, str) else np.asarray(seq, dtype=np.uint8)
        ref_blob = np.asarray(cols["ref_blob"], dtype=np.uint8)
        if np.any(reflen < span):
            i = int(np.flatnonzero(reflen < span)[0])
            raise HaplotypeBuildError(f"Mismatching reference alleles at position {int(pos[i])}")
        # REF allele must match over the replaced span (haplotype.py:203-208), letters compared case-insensitively
        rec = np.repeat(np.arange(nv), span)
        k = np.arange(len(rec)) - np.repeat(np.cumsum(span) - span, span)
        bad = np.flatnonzero(((seq_u8[r0[rec] + k] ^ ref_blob[ref_off[rec] + k]) & 0xDF) != 0)
        if len(bad):
            raise HaplotypeBuildError(f"Mismatching reference alleles at position {int(pos[int(rec[int(bad[0])])])}")
    alt_blob = np.asarray(cols["alt_blob"], dtype=np.uint8)
    alt_codes = _NIB[alt_blob] if len(alt_blob) else np.zeros(0, np.uint8)
    return r0, span, chain, altlen, alt_off_all[:-1].copy(), alt_codes


class ScanOwnership:
    """Which PAM positions of a haplotype row this set scans, for a row string that is one tile of a larger region
    (tiling.py).  `own_lo` / `own_hi`: genomic positions of the seams (None = the region's own rule at that end,
    compute_scan_start_stop, search_guides.py:49-84); a seam maps to the LAST relative position with that genomic
    position (the reference's posmap_rev rule), walking forward when the position is deleted - the same rule in both
    neighbouring tiles, so every haplotype position is scanned by exactly one of them.  `partner` = the region's scan
    range in the REF row's relative positions (hawk_hapset_set_ref_partner_range).  `guard`: haplotype bases that must
    exist on either side of an interior seam so that is_pamhit_in_range (search_guides.py:395-420) cannot fire there."""

    def __init__(self, own_lo: Optional[int], own_hi: Optional[int], partner: Optional[Tuple[int, int]], guard: int):
        self.own_lo, self.own_hi, self.partner, self.guard = own_lo, own_hi, partner, guard


def _seam_rel(seg: PosSegments, g: int) -> int:
    r = seg.rev(g)
    if r >= 0:
        return r
    upper = seg.max_gen()
    for p in range(g + 1, upper + 1):
        r = seg.rev(p)
        if r >= 0:
            return r
    return seg.length


def _scan_for(seg: PosSegments, startp: int, stopp: int, pamlen: int, own: Optional[ScanOwnership]) -> Tuple[int, int]:
    if own is None:
        return scan_bounds(seg, startp, stopp, pamlen)
    if own.own_lo is None:
        lo = scan_start(seg, startp)
    if own.own_hi is None:
        hi = scan_stop(seg, stopp, pamlen)
    if own.own_lo is not None:
        lo = _seam_rel(seg, own.own_lo)
        if lo < own.guard:
            raise ValueError("tile flank too small: a guide window at the seam would leave the tile (left)")
    if own.own_hi is not None:
        hi = _seam_rel(seg, own.own_hi)
        if hi + own.guard > seg.length:
            raise ValueError("tile flank too small: a guide window at the seam would leave the tile (right)")
    return lo, max(lo, hi)


class RowMeta:
    """Position maps and scan ranges of the rows of a device-built plan, with list-like access to per-row `HostHaplotype`
    views for the few callers that want one (labels keep `host_meta[r].seg`).  Replaces 5009 Python objects and as many
    numpy calls per expansion."""

    def __init__(self, fetch, hap_len: np.ndarray, alias: np.ndarray):
        """`fetch`: a callable returning (seg_start, seg_rel, seg_gen) - the plan's segments are downloaded only when
        something on the host reads them."""
        self._segs, self._fetch = None, fetch
        self.hap_len, self.alias = np.asarray(hap_len, dtype=np.int64), alias
        self.n = len(hap_len)
        self.scan_lo = np.zeros(self.n, dtype=np.int64)
        self.scan_hi = np.zeros(self.n, dtype=np.int64)

    def _need(self):
        if self._segs is None:
            self._segs = self._fetch()
        return self._segs

    seg_start = property(lambda self: self._need()[0])
    seg_rel = property(lambda self: self._need()[1])
    seg_gen = property(lambda self: self._need()[2])

    def __len__(self):
        return self.n

    def seg(self, r: int) -> PosSegments:
        a, b = int(self.seg_start[r]), int(self.seg_start[r + 1])
        return PosSegments(self.seg_rel[a:b], self.seg_gen[a:b], int(self.hap_len[r]))

    def __getitem__(self, r: int) -> HostHaplotype:
        return HostHaplotype(b"", self.seg(r), r == 0, (int(self.scan_lo[r]), int(self.scan_hi[r])))

    def __iter__(self):
        return (self[r] for r in range(self.n))

    def compute_scans(self, lo: np.ndarray, hi: np.ndarray, startp: int, stopp: int, pamlen: int,
                      own: Optional["ScanOwnership"]) -> None:
        """compute_scan_start_stop (search_guides.py:49-84), or a tile's ownership range, for every live row.  `lo` / `hi`:
        posmap_rev of every row at the two genomic positions the bounds start from (the last relative position with that
        genomic position, -1 where it is deleted; computed on the device beside the segments).  Rows whose boundary
        position is deleted (rare) take the per-row walk of `_scan_for`."""
        live = self.alias == np.arange(self.n)
        if own is None or own.own_hi is None:
            hi = np.where(hi >= 0, hi - pamlen + 1, hi)
        slow = live & ((lo < 0) | (hi < 0))
        if own is not None and own.own_lo is not None and np.any(live & (lo >= 0) & (lo < own.guard)):
            raise ValueError("tile flank too small: a guide window at the seam would leave the tile (left)")
        if own is not None and own.own_hi is not None and np.any(live & (hi >= 0) & (hi + own.guard > self.hap_len)):
            raise ValueError("tile flank too small: a guide window at the seam would leave the tile (right)")
        self.scan_lo = np.where(live, lo, 0)
        self.scan_hi = np.where(live, hi if own is None else np.maximum(lo, hi), 0)
        for r in np.flatnonzero(slow).tolist():
            a, b = _scan_for(self.seg(r), startp, stopp, pamlen, own)
            self.scan_lo[r], self.scan_hi[r] = a, b


class _RowInfos:
    """The HapInfo of every row of an expansion (None for rows collapsed onto another), built when first read: the sample
    labels of 5009 rows are Python strings nobody needs before a report is written."""

    def __init__(self, n_hap, samples, e_s, e_g, e_r, e_owner, rows_of):
        self._args = (n_hap, samples, e_s, e_g, e_r, e_owner, rows_of)
        self._info = None

    def _build(self):
        if self._info is None:
            n_hap, samples, e_s, e_g, e_r, e_owner, rows_of = self._args
            gts = ("1|1", "1|0", "0|1")
            labels_e = [f"{samples[si]}:{gts[g]}" for si, g in zip(e_s.tolist(), e_g.tolist())]
            info: List[Optional[HapInfo]] = [HapInfo(["REF"], ())] + [None] * (n_hap - 1)
            for lab, r, o in zip(labels_e, e_r.tolist(), e_owner.tolist()):
                if o == 0:
                    continue  # collapses onto REF, which keeps samples == "REF" (haplotypes.py:255-258)
                if info[o] is None:
                    info[o] = HapInfo([lab], rows_of(o))
                else:
                    info[o].samples.append(lab)
            self._info = info
        return self._info

    def __getitem__(self, i):
        return self._build()[i]

    def __len__(self):
        return self._args[0]

    def __iter__(self):
        return iter(self._build())


class _KeptInfos:
    """info of the kept rows, in row order (what the expansion entry points return), as lazily as _RowInfos"""

    def __init__(self, infos: _RowInfos, kept: List[int]):
        self._infos, self._kept = infos, kept

    def __getitem__(self, j):
        if isinstance(j, slice):
            return [self._infos[i] for i in self._kept[j]]
        return self._infos[self._kept[j]]

    def __len__(self):
        return len(self._kept)

    def __iter__(self):
        return (self._infos[i] for i in self._kept)


def _exact_keys(ds, hashes: np.ndarray) -> np.ndarray:
    """Rows grouped by content, exactly: rows sharing a 128-bit content hash are compared base for base on the device
    (hawk_hapset_rows_equal) against the first row of their hash group; a row that differs (a hash collision - never seen)
    opens a group of its own with the rows that equal IT.  Returns one key per row."""
    import ctypes as C
    from . import _lib
    from .hapset import _p
    h64 = hashes[:, 0] * np.uint64(0x9e3779b97f4a7c15) + (hashes[:, 1] ^ (hashes[:, 1] >> np.uint64(29)))
    _, first_idx, key_id = np.unique(h64, return_index=True, return_inverse=True)
    key_id = key_id.reshape(-1).astype(np.int64)
    n = len(key_id)
    head = first_idx[key_id]
    todo = np.flatnonzero(head != np.arange(n))  # rows that would be merged with an earlier row
    next_key = int(key_id.max()) + 1 if n else 0
    while len(todo):
        a = np.ascontiguousarray(todo, dtype=np.uint32)
        b = np.ascontiguousarray(head[todo], dtype=np.uint32)
        eq = np.zeros(len(todo), dtype=np.uint8)
        _lib.check(_lib.lib().hawk_hapset_rows_equal(ds._h, len(todo), _p(a), _p(b), _p(eq)), "hawk_hapset_rows_equal")
        bad = todo[eq == 0]
        if len(bad) == 0:
            break
        # per old group: its first mismatching row heads a new group, the other mismatching rows are tried against it
        for k in np.unique(key_id[bad]).tolist():
            rows = bad[key_id[bad] == k]
            key_id[rows] = next_key
            head[rows] = rows[0]
            next_key += 1
        todo = bad[head[bad] != bad]
    return key_id


def _collapse_rows(hashes: np.ndarray, samples: List[str], live: np.ndarray, n_hap: int, rows_of, ds=None):
    """Labels, homozygous merge and collapse by content of the rows of an expansion (haplotypes.py:232-368), all rows at
    once on their 16-byte content hashes.  `rows_of(r)` -> the carried-variant indices of row r (or a callable yielding
    them).  Returns (alias[n_hap], info[n_hap] with None for rows collapsed onto another)."""
    # entries in the reference's order (haplotypes.py:297-368): samples in panel order, copy 0 then copy 1; a sample
    # whose two copies hold the same sequence contributes one "1|1" entry; a copy without variants is the REF sequence
    # rows that hold the same bases: grouped on the 128-bit content hash and then compared on the device, base for base
    # (the reference compares the strings, haplotypes.py:274-294); without a set to compare on, the hash alone
    if ds is not None:
        key_id = _exact_keys(ds, hashes)
    else:
        _, key_id = np.unique(hashes, axis=0, return_inverse=True)
        key_id = key_id.reshape(-1)
    ns = len(samples)
    row_of_col = np.zeros(2 * ns, dtype=np.int64)          # 0 = "no row" (the copy carries nothing: it IS REF)
    row_of_col[np.asarray(live, dtype=np.int64)] = np.arange(1, n_hap)
    r_a, r_b = row_of_col[0::2], row_of_col[1::2]           # rows of copy 0 / copy 1 per sample (0: none)
    k_a, k_b = key_id[r_a], key_id[r_b]                     # row 0 is REF, so "none" reads REF's key
    present = (r_a > 0) | (r_b > 0)
    homo = present & (k_a == k_b)
    alias = np.arange(n_hap)
    alias[(key_id == key_id[0]) & (alias > 0)] = 0          # a copy whose variants reproduce the REF sequence
    both = homo & (r_a > 0) & (r_b > 0)
    # entry list: (sample, row, genotype code 0 = 1|1, 1 = 1|0, 2 = 0|1), rows that do not exist dropped
    e_s = np.concatenate((np.flatnonzero(homo), np.flatnonzero(present & ~homo), np.flatnonzero(present & ~homo)))
    e_r = np.concatenate((r_a[homo], r_a[present & ~homo], r_b[present & ~homo]))
    e_g = np.concatenate((np.zeros(int(homo.sum()), np.int64), np.ones(int((present & ~homo).sum()), np.int64),
                          np.full(int((present & ~homo).sum()), 2, np.int64)))
    ok = e_r > 0
    e_s, e_r, e_g = e_s[ok], e_r[ok], e_g[ok]
    order = np.lexsort((e_g, e_s))                          # sample order, then 1|1 / 1|0 before 0|1
    e_s, e_r, e_g = e_s[order], e_r[order], e_g[order]
    # the first row seen with a key owns it (REF owns its own key); later rows with that key alias onto the owner
    e_k = key_id[e_r]
    owner_of_key = np.full(int(key_id.max()) + 1, -1, dtype=np.int64)
    uk, first_pos = np.unique(e_k, return_index=True)
    owner_of_key[uk] = e_r[first_pos]
    owner_of_key[key_id[0]] = 0
    e_owner = owner_of_key[e_k]
    alias[e_r] = e_owner
    alias[r_b[both]] = alias[r_a[both]]                     # the second copy of a homozygous sample follows the first
    return alias, _RowInfos(n_hap, samples, e_s, e_g, e_r, e_owner, rows_of)


def _expand_rows_gt(ref_set, seq, startp: int, stopp: int, pamlen: int, samples: List[str], tab, g, col_off: np.ndarray, device,
                    keep_plan: bool = False, own: Optional[ScanOwnership] = None):
    """Common tail of the device expansions: rows = REF + every chromosome copy (column) with a non-empty carried list, in
    column order.  `g` is a hawk_gt after hawk_gt_lists whose lists are still on the device: the expansion plan is created
    from them in place (hawk_xplan_create_gt) - checks, position-map segments and the scan bounds' reverse look-ups are
    kernels over the lists; the host sees a few words per ROW (lengths, content hashes, two look-ups) and does the labels /
    homozygous merge / collapse on the 16-byte content hashes (haplotypes.py:232-368).  Labels read the lists / segments
    lazily (CarriedLists, RowMeta's fetch).  With `keep_plan` the plan stays attached as `ds.plan`, so the set can be
    re-expanded with device work only.  Takes ownership of `g`."""
    import ctypes as C
    from . import _lib
    from .expand import HaplotypeBuildError
    from .hapset import ExpansionPlan, _p
    r0, span, chain, altlen, alt_off, alt_codes = tab
    L = _lib.lib()
    counts = np.diff(col_off.astype(np.int64))
    live = np.flatnonzero(counts)
    lists = CarriedLists(g, int(col_off[-1]))
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
    arrs = [u32(r0), u32(span), u32(alt_off), u32(altlen), np.ascontiguousarray(chain, dtype=np.int32), np.ascontiguousarray(alt_codes)]
    xh, n_hap_c = C.c_void_p(), C.c_uint32(0)
    # where the scan bounds start from: the region's own rule (search_guides.py:49-84) or, for a tile of a larger region, its
    # seams; the end-of-region clamp is the region's and cannot be reproduced by a tile (divergences)
    lo_g = startp + 100 if (own is None or own.own_lo is None) else own.own_lo
    hi_g = stopp - 100 if (own is None or own.own_hi is None) else own.own_hi
    rc = L.hawk_xplan_create_gt(ref_set._h, g, len(r0), _p(arrs[0]), _p(arrs[1]), _p(arrs[2]), _p(arrs[3]), _p(arrs[4]), _p(arrs[5]),
                                len(alt_codes), C.c_int64(startp), 1 if own is None else 0, C.c_int64(lo_g), C.c_int64(hi_g),
                                C.byref(n_hap_c), C.byref(xh))
    if rc == _lib.HAWK_E_OVERLAP:
        raise HaplotypeBuildError("a chromosome copy carries overlapping variants")
    if rc == _lib.HAWK_E_CLAMP:
        raise HaplotypeBuildError("variant beyond the original region length (haplotype.py:199-201 clamp)")
    _lib.check(rc, "hawk_xplan_create_gt")
    n_hap = n_hap_c.value
    hap_len = np.zeros(n_hap, dtype=np.uint32)
    rev0, rev1 = np.zeros(n_hap, dtype=np.int64), np.zeros(n_hap, dtype=np.int64)
    _lib.check(L.hawk_xplan_rows(xh, _p(hap_len), _p(rev0), _p(rev1)), "hawk_xplan_rows")
    plan = ExpansionPlan(xh, hap_len, device)
    plan.n_records = int(col_off[-1])
    ds, hashes, ms_val = plan.run(want_hash=True)
    row_end = np.concatenate(([0, 0], col_off.astype(np.int64)[live + 1]))  # row r's list: [row_end[r], row_end[r + 1])
    alias, info = _collapse_rows(hashes, samples, live, n_hap, lambda o: lists.rows(int(row_end[o]), int(row_end[o + 1])), ds)

    def fetch():
        nseg = C.c_uint64(0)
        _lib.check(L.hawk_xplan_segments(plan._x, None, None, None, C.c_uint64(0), C.byref(nseg)), "hawk_xplan_segments")
        so = np.zeros(n_hap + 1, dtype=np.uint32)
        sr, sg = np.zeros(nseg.value, dtype=np.uint32), np.zeros(nseg.value, dtype=np.int64)
        _lib.check(L.hawk_xplan_segments(plan._x, _p(so), _p(sr), _p(sg), C.c_uint64(nseg.value), None), "hawk_xplan_segments")
        return so.astype(np.int64), sr, sg
    haps = RowMeta(fetch, hap_len, alias)
    haps.compute_scans(rev0, rev1, startp, stopp, pamlen, own)
    _lib.check(L.hawk_xplan_finish_meta(plan._x, _p(haps.scan_lo.astype(np.int32)), _p(haps.scan_hi.astype(np.int32))), "hawk_xplan_finish_meta")
    if own is not None and own.partner is not None:
        _lib.check(L.hawk_xplan_set_ref_partner_range(plan._x, int(own.partner[0]), int(own.partner[1])), "hawk_xplan_set_ref_partner_range")
    is_ref = np.zeros(n_hap, dtype=np.uint8)
    is_ref[0] = 1
    plan.ref_index, plan.is_ref = 0, is_ref
    _lib.check(L.hawk_xplan_install_meta(plan._x, ds._h), "hawk_xplan_install_meta")
    ds.ref_index, ds.is_ref = 0, is_ref
    ds.alias = alias
    ds.host_meta = haps
    plan.alias, plan.host_meta = alias, haps
    plan._lists = lists  # the labels' lists die with the plan at the latest
    if keep_plan:
        ds.plan = plan
    else:
        ds._plan_keepalive = plan  # the lazy segment download reads the plan
    kept = np.flatnonzero(alias == np.arange(n_hap)).tolist()
    return ds, _KeptInfos(info, kept), float(ms_val), kept


def _ref_only_set(seq, startp: int, stopp: int, pamlen: int, device, own: Optional[ScanOwnership] = None):
    from . import _lib
    from .hapset import DeviceHapSet
    ref_u8 = np.frombuffer(seq.encode("ascii"), dtype=np.uint8) if isinstance(seq, str) else np.asarray(seq, dtype=np.uint8)
    ref_seg = PosSegments.identity(startp, len(ref_u8))
    meta = HostHaplotype(ref_u8, ref_seg, True, _scan_for(ref_seg, startp, stopp, pamlen, own))
    ds = DeviceHapSet([meta], device)
    if own is not None and own.partner is not None:
        _lib.check(_lib.lib().hawk_hapset_set_ref_partner_range(ds._h, int(own.partner[0]), int(own.partner[1])),
                   "hawk_hapset_set_ref_partner_range")
    ds.host_meta = [meta]
    return ds


def invert_on_device(ctx, G: np.ndarray, r0: np.ndarray, chain: np.ndarray):
    """A 0/1 genotype matrix G[variant, chromosome copy] -> (hawk_gt handle whose carried-variant lists are in HBM,
    col_off[n_cols + 1]).  The caller owns the handle (hawk_gt_destroy, or hand it to _expand_rows_gt)."""
    import ctypes as C
    from . import _lib
    from .hapset import _p
    G = np.ascontiguousarray(G, dtype=np.uint8)
    nv, n_cols = G.shape
    if n_cols % 2:
        raise ValueError("genotype matrix needs two columns per sample")
    L = _lib.lib()
    g = C.c_void_p()
    _lib.check(L.hawk_gt_from_codes(ctx, _p(G), C.c_uint64(nv), n_cols // 2, C.byref(g)), "hawk_gt_from_codes")
    try:
        col_off = np.zeros(n_cols + 1, dtype=np.uint64)
        _lib.check(L.hawk_gt_lists(g, _p(np.arange(nv, dtype=np.uint32)), _p(np.ones(nv, dtype=np.uint8)),
                                   _p(np.ascontiguousarray(r0, dtype=np.int32)), _p(np.ascontiguousarray(chain, dtype=np.int32)), nv,
                                   _p(col_off), None, None), "hawk_gt_lists")
    except Exception:
        L.hawk_gt_destroy(g)
        raise
    return g, col_off


def expand_on_device(reg: SynthRegion, pamlen: int, device: Optional[int] = None, sample_range: Optional[Tuple[int, int]] = None,
                     keep_plan: bool = False):
    """build_phased_haplotypes() with the sequence work done on the device (hawk_gt_lists, hawk_xplan_create_gt,
    hawk_xplan_run): the host only prepares the variant table and labels; no haplotype string is ever formed.
    Returns (DeviceHapSet, [HapInfo] of the kept rows, kernel ms, kept row indices).  Rows that collapse onto an earlier row
    (haplotypes.py:274-294; homozygous copies, 326-333) stay in HBM with an empty scan range."""
    seq, startp, stopp = reg.sequence, reg.startp, reg.stopp
    ref_set = _ref_only_set(seq, startp, stopp, pamlen, device)
    slo, shi = sample_range if sample_range is not None else (0, len(reg.samples))
    if not reg.variants or shi <= slo:
        ref_set.alias = np.zeros(1, dtype=np.int64)
        return ref_set, [HapInfo(["REF"], ())], 0.0, [0]
    if hasattr(reg, "variant_columns"):
        tab = _variant_table_columns(reg.variant_columns(), seq, startp)
    else:
        tab = _variant_table(np.array([v.pos for v in reg.variants]), [v.ref for v in reg.variants], [v.alt for v in reg.variants], seq, startp)
    r0, span, chain = tab[0], tab[1], tab[2]
    # which variants each chromosome copy carries: the in-memory genotype matrix goes to the device as allele codes and
    # is inverted there (hawk_gt_lists, the kernels of the VCF path) - a host-side nonzero scan of the 155 MB matrix
    # took 0.4 s of C3's expansion (`sample_range`: this rank's block of the panel - haplotypes shard across GPUs, REF
    # is on every rank)
    gm = getattr(reg, "gt_matrix", None)
    if gm is not None and gm.shape == (len(reg.variants), 2 * len(reg.samples)) and \
            all(np.array_equal(gm[i], reg.variants[i].gt.reshape(-1)) for i in (0, len(reg.variants) // 2, -1)):
        G = gm if (slo, shi) == (0, len(reg.samples)) else gm[:, 2 * slo:2 * shi]  # the panel already is one matrix
    else:
        G = np.stack([v.gt[slo:shi].reshape(-1) for v in reg.variants])  # [site, 2*sample]
    g, col_off = invert_on_device(ref_set._ctx, G, r0, chain)
    if int(col_off[-1]) == 0:
        from . import _lib
        _lib.lib().hawk_gt_destroy(g)
        ref_set.alias = np.zeros(1, dtype=np.int64)
        return ref_set, [HapInfo(["REF"], ())], 0.0, [0]
    return _expand_rows_gt(ref_set, seq, startp, stopp, pamlen, reg.samples[slo:shi], tab, g, col_off, device, keep_plan=keep_plan)


class VcfVariants:
    """The variant table of a VCF block after VariantRecord.split() (variant.py:313-331): one entry per ALT allele,
    alleles and position adjusted like adjust_multiallelic, ids like _compute_id, AF from INFO."""

    def __init__(self, block, contig: Optional[str] = None):
        from .variant import adjust_multiallelic
        pos, ref, alt, vid, af, line, allele = [], [], [], [], [], [], []
        nan = float("nan")
        for i, f in enumerate(block.fixed):
            chrom, p, r, alt_s, info = f[0], int(f[1]), f[3], f[4], f[7]
            k = info.find("AF=")
            if "," not in alt_s:  # one ALT allele: the usual record, no per-allele loop
                a1 = nan
                if k != -1:  # variant.py:188-206
                    e = info.find(";", k + 3)
                    a_s = info[k + 3: len(info) if e == -1 else e]
                    if "," in a_s:
                        raise ValueError(f"AF number does not match the alleles number ({a_s.count(',') + 1} - 1)")
                    a1 = float(a_s)
                if len(r) == 1 and len(alt_s) == 1:
                    r_, a_, p_ = r, alt_s, p
                else:
                    r_, a_, p_ = adjust_multiallelic(r, alt_s, p)
                pos.append(p_); ref.append(r_); alt.append(a_); af.append(a1)
                vid.append(f"{chrom}-{p}-{r}/{alt_s}")
                line.append(i); allele.append(1)
                continue
            alts = alt_s.split(",")
            afs = [nan] * len(alts)
            if k != -1:
                e = info.find(";", k + 3)
                afs = [float(x) for x in info[k + 3: len(info) if e == -1 else e].split(",")]
                if len(afs) != len(alts):
                    raise ValueError(f"AF number does not match the alleles number ({len(afs)} - {len(alts)})")
            for a, al in enumerate(alts):
                r_, a_, p_ = adjust_multiallelic(r, al, p)
                pos.append(p_); ref.append(r_); alt.append(a_); af.append(afs[a])
                vid.append(f"{chrom}-{p}-{r}/{al}")
                line.append(i); allele.append(a + 1)
        order = np.argsort(np.asarray(pos, dtype=np.int64), kind="stable")
        pick = lambda xs: [xs[int(j)] for j in order]
        self.pos = np.asarray(pos, dtype=np.int64)[order]
        self.ref, self.alt, self.id, self.af = pick(ref), pick(alt), pick(vid), pick(af)
        self.line = np.asarray(line, dtype=np.uint32)[order]
        self.allele = np.asarray(allele, dtype=np.uint8)[order]

    def __len__(self) -> int:
        return len(self.pos)


def expand_from_vcf(region_seq: str, startp: int, stopp: int, block, samples: List[str], pamlen: int, phased: bool = True,
                    device: Optional[int] = None, keep_plan: bool = False):
    """f3 -> f1: the records of a VCF block (readers.VCF.fetch_block) straight to device haplotypes.  The sample
    columns are parsed on the device (hawk_gt_parse) and inverted into carried-variant lists there
    (hawk_gt_lists); the host handles the fixed columns of the records only.
    Returns (DeviceHapSet, [HapInfo], kernel ms {parse, lists, expand}, kept rows, VcfVariants); with `keep_plan` the
    expansion plan stays attached as `ds.plan` (its view searches without planes: hawk_xplan_view)."""
    import ctypes as C
    from . import _lib
    from .hapset import _p
    if not phased:
        raise ValueError("expand_from_vcf builds phased haplotypes; the rows of an unphased VCF are built by expand_unphased_from_vcf "
                         "(or on the host, haplotypes.add_variants_unphased)")
    ref_set = _ref_only_set(region_seq, startp, stopp, pamlen, device)
    vt = VcfVariants(block)
    if len(vt) == 0:
        ref_set.alias = np.zeros(1, dtype=np.int64)
        return ref_set, [HapInfo(["REF"], ())], {"parse": 0.0, "lists": 0.0, "expand": 0.0}, [0], vt
    tab = _variant_table(vt.pos, vt.ref, vt.alt, region_seq, startp)
    r0, chain = tab[0], tab[2]
    L = _lib.lib()
    g = C.c_void_p()
    ms_parse, ms_lists = C.c_float(0), C.c_float(0)
    text = np.ascontiguousarray(block.text)
    _lib.check(L.hawk_gt_parse(ref_set._ctx, _p(text), C.c_uint64(len(text)), _p(block.line_off), _p(block.gt_off),
                               C.c_uint64(len(block)), len(samples), C.byref(g), C.byref(ms_parse)), "hawk_gt_parse")
    try:
        flags = np.zeros(len(block), dtype=np.uint8)
        _lib.check(L.hawk_gt_codes(g, None, _p(flags)), "hawk_gt_codes")
        if np.any(flags & 2):
            raise ValueError(f"VCF record {int(np.flatnonzero(flags & 2)[0])} does not have one genotype per sample")
        if np.any(flags & 1):  # variant.py:489-506: a phased VCF must hold a|b everywhere
            raise ValueError("Phased genotypes cannot have more than one allele on each copy")
        if np.any(flags & 4):
            raise ValueError(f"Malformed genotype in VCF record {int(np.flatnonzero(flags & 4)[0])}")
        n_cols = 2 * len(samples)
        col_off = np.zeros(n_cols + 1, dtype=np.uint64)
        col_delta = np.zeros(n_cols, dtype=np.int64)
        _lib.check(L.hawk_gt_lists(g, _p(vt.line), _p(vt.allele), _p(np.ascontiguousarray(r0, dtype=np.int32)),
                                   _p(np.ascontiguousarray(chain, dtype=np.int32)), len(vt), _p(col_off), _p(col_delta),
                                   C.byref(ms_lists)), "hawk_gt_lists")
        handed = False
        if int(col_off[-1]) == 0:  # no chromosome copy carries anything: REF alone
            ref_set.alias = np.zeros(1, dtype=np.int64)
            return ref_set, [HapInfo(["REF"], ())], {"parse": float(ms_parse.value), "lists": float(ms_lists.value), "expand": 0.0}, [0], vt
        handed = True
        ds, info, ms_expand, kept = _expand_rows_gt(ref_set, region_seq, startp, stopp, pamlen, samples, tab, g, col_off, device,
                                                    keep_plan=keep_plan)
    finally:
        if not locals().get("handed", False):
            L.hawk_gt_destroy(g)
    return ds, info, {"parse": float(ms_parse.value), "lists": float(ms_lists.value), "expand": ms_expand}, kept, vt


class RowLabel:
    """What the report needs to know about one device haplotype row (the Haplotype fields of guide.py:64-118)."""

    __slots__ = ("samples", "variants", "afs", "id", "segments")

    def __init__(self, samples: str, variants: str, afs, hid: str, segments):
        self.samples, self.variants, self.afs, self.id, self.segments = samples, variants, afs, hid, segments


_BASE_IDX = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _BASE_IDX[_c] = _i


def unphased_snv_table(block, vt: "VcfVariants", region_len: int, startp: int):
    """The SNV alleles of a block, in `vt`'s order, as the arrays hawk_ubuild_lists takes: (indices into vt, var_line, var_allele,
    var_off, var_mask, var_ref).  Raises _lib.UnphasedBuildDeclined for what the device builder does not take: an equal-length
    allele longer than one base (the host builder reads its first base), a base outside A/C/G/T, an SNV outside the region."""
    from ._lib import UnphasedBuildDeclined
    n = len(vt)
    snv = np.zeros(n, dtype=bool)
    for j in range(n):
        f = block.fixed[int(vt.line[j])]
        raw_alt = f[4] if vt.allele[j] == 1 and "," not in f[4] else f[4].split(",")[int(vt.allele[j]) - 1]
        if len(f[3]) == len(raw_alt):
            if len(raw_alt) != 1:
                raise UnphasedBuildDeclined(2, vt.id[j])
            snv[j] = True
    sel = np.flatnonzero(snv)
    refb = _BASE_IDX[np.frombuffer("".join(vt.ref[int(j)] for j in sel).encode("latin-1", "replace"), dtype=np.uint8)] if len(sel) else np.zeros(0, np.uint8)
    altb = _BASE_IDX[np.frombuffer("".join(vt.alt[int(j)] for j in sel).encode("latin-1", "replace"), dtype=np.uint8)] if len(sel) else np.zeros(0, np.uint8)
    bad = np.flatnonzero((refb > 3) | (altb > 3))
    if len(bad):
        raise UnphasedBuildDeclined(3, vt.id[int(sel[bad[0]])])
    off = vt.pos[sel] - int(startp)
    out = np.flatnonzero((off < 0) | (off >= region_len))
    if len(out):
        raise UnphasedBuildDeclined(5, vt.id[int(sel[out[0]])])
    return (sel, np.ascontiguousarray(vt.line[sel], dtype=np.uint32), np.ascontiguousarray(vt.allele[sel], dtype=np.uint8),
            np.ascontiguousarray(off, dtype=np.uint32), (np.uint8(1) << altb).astype(np.uint8), np.ascontiguousarray(refb, dtype=np.uint8))


def _merged_sites(pos: np.ndarray, bits: np.ndarray):
    """an ascending entry list -> its sites: distinct positions, the entries' bits OR-ed"""
    first = np.flatnonzero(np.concatenate(([True], pos[1:] != pos[:-1])))
    return pos[first], np.bitwise_or.reduceat(bits, first)


def group_unphased_rows(sample_off: np.ndarray, idx: np.ndarray, sig: np.ndarray, var_off: np.ndarray, var_mask: np.ndarray, var_ref: np.ndarray):
    """Carriers grouped into distinct rows (_merge_equal on the rows they would give): samples sharing a 128-bit signature are
    compared site for site - the signature only proposes - and a sample that differs from every row with its signature opens a
    row of its own.  -> [[sample, ...]] in first-carrier order, members ascending."""
    e_pos = var_off[idx]
    e_bits = var_mask[idx] | (np.uint8(1) << var_ref[idx])
    so = sample_off.astype(np.int64)
    sites = lambda s: _merged_sites(e_pos[so[s]:so[s + 1]], e_bits[so[s]:so[s + 1]])
    rows: List[List[int]] = []
    by_sig: Dict[Tuple[int, int], List[int]] = {}
    head_sites = {}
    for s in np.flatnonzero(np.diff(so) > 0).tolist():
        mine = None
        found = None
        for k in by_sig.get((int(sig[s, 0]), int(sig[s, 1])), ()):
            h = rows[k][0]
            if np.array_equal(idx[so[h]:so[h + 1]], idx[so[s]:so[s + 1]]):
                found = k
                break
            mine = sites(s) if mine is None else mine
            if k not in head_sites:
                head_sites[k] = sites(h)
            if np.array_equal(mine[0], head_sites[k][0]) and np.array_equal(mine[1], head_sites[k][1]):
                found = k
                break
        if found is None:
            by_sig.setdefault((int(sig[s, 0]), int(sig[s, 1])), []).append(len(rows))
            rows.append([s])
        else:
            rows[found].append(s)
    return rows


def unphased_snv_labels(groups, sample_off: np.ndarray, idx: np.ndarray, sel: np.ndarray, vt: "VcfVariants", samples: List[str], segments,
                        row_base: int) -> List["RowLabel"]:
    """The labels _merge_equal gives the distinct whole-region rows: samples and variants as sorted unions over the members (a
    member's `variants` is the id list of what it carries, in list order), afs of the first member, `hap_%08d` by row index."""
    so = sample_off.astype(np.int64)
    out = []
    for k, members in enumerate(groups):
        head = idx[so[members[0]]:so[members[0] + 1]]
        strings = {",".join(vt.id[int(sel[j])] for j in head.tolist())}
        for s in members[1:]:
            mine = idx[so[s]:so[s + 1]]
            if not np.array_equal(mine, head):
                strings.add(",".join(vt.id[int(sel[j])] for j in mine.tolist()))
        afs = {vt.id[int(sel[j])]: vt.af[int(sel[j])] for j in head.tolist()}
        out.append(RowLabel(",".join(sorted({samples[s] for s in members})), ",".join(sorted(strings)), afs, f"hap_{row_base + k:08d}", segments))
    return out


def unphased_snv_alleles(groups, sample_off: np.ndarray, idx: np.ndarray, v_off: np.ndarray, v_ref: np.ndarray, row_base: int):
    """The allele table of the distinct whole-region rows in search_guides.flatten_variant_alleles' format: one key per carried
    position of a row's first member (row << 32 | offset), one entry per carried allele there, its ref's index in "ACGT"."""
    if not groups:
        return np.zeros(0, np.uint64), np.zeros(1, np.uint32), np.zeros(0, np.uint8)
    so = sample_off.astype(np.int64)
    heads = [idx[so[m[0]]:so[m[0] + 1]] for m in groups]
    j = np.concatenate(heads).astype(np.int64)
    rows = np.repeat(np.arange(row_base, row_base + len(groups), dtype=np.uint64), [len(h) for h in heads])
    e_key = (rows << np.uint64(32)) | v_off[j].astype(np.uint64)
    first = np.flatnonzero(np.concatenate(([True], e_key[1:] != e_key[:-1])))
    return e_key[first], np.concatenate((first, [len(e_key)])).astype(np.uint32), v_ref[j].astype(np.uint8)


def unphased_rows_host(region_seq: str, startp: int, block, samples: List[str], codes: np.ndarray):
    """The distinct whole-region rows of an unphased block by the host twin (hawk_host_unphased_rows; no device): `codes` =
    the block's allele codes [n_lines][2 * n_samples] as hawk_gt_parse_unphased gives them.  -> (row strings, [RowLabel] with
    ids from hap_00000001, the rows' allele table, the twin's per-sample lists (sample_off, idx), signatures, member lists).
    Raises _lib.UnphasedBuildDeclined as expand_unphased_from_vcf does."""
    import ctypes as C
    from . import _lib
    from ._lib import UnphasedBuildDeclined
    from .hapset import _p
    vt = VcfVariants(block)
    ref = np.frombuffer(region_seq.upper().encode("ascii"), dtype=np.uint8)
    sel, v_line, v_allele, v_off, v_mask, v_ref = unphased_snv_table(block, vt, len(ref), startp)
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    ns = len(samples)
    inp = _lib.UbuildInput(codes.ctypes.data, len(block), ns, len(sel), v_line.ctypes.data, v_allele.ctypes.data, v_off.ctypes.data,
                           v_mask.ctypes.data, v_ref.ctypes.data, ref.ctypes.data, len(ref), 1)
    out, dec = _lib.UbuildRows(), _lib.UbuildDecline()
    L = _lib.lib()

    def call():
        rc = L.hawk_host_unphased_rows(C.byref(inp), C.byref(out), C.byref(dec))
        if rc != _lib.HAWK_OK and dec.reason:
            raise UnphasedBuildDeclined(dec.reason, vt.id[int(sel[dec.var])] if dec.var >= 0 else "")
        _lib.check(rc, "hawk_host_unphased_rows")
    call()  # the counts; then buffers of exactly their size
    nr, ne = int(out.n_rows), int(out.n_entries)
    seqs = np.zeros(nr * len(ref), np.uint8); member_off = np.zeros(nr + 1, np.uint32); member = np.zeros(int(out.n_members), np.uint32)
    sample_off = np.zeros(ns + 1, np.uint64); idx = np.zeros(ne, np.uint32); sig = np.zeros((ns, 2), np.uint64)
    out.row_cap, out.entry_cap = nr, ne
    out.seqs, out.member_off, out.member_sample = seqs.ctypes.data, member_off.ctypes.data, member.ctypes.data
    out.sample_off, out.list_idx, out.sig = sample_off.ctypes.data, idx.ctypes.data, sig.ctypes.data
    call()
    groups = [member[int(member_off[k]):int(member_off[k + 1])].tolist() for k in range(nr)]
    so = sample_off.astype(np.int64)
    n_al = int(sum(so[m[0] + 1] - so[m[0]] for m in groups))
    al_key = np.zeros(int(out.n_keys), np.uint64); al_off = np.zeros(int(out.n_keys) + 1, np.uint32); al_ref = np.zeros(n_al, np.uint8)
    out.seqs = out.member_off = out.member_sample = out.sample_off = out.list_idx = out.sig = None
    out.entry_cap = n_al
    out.al_key, out.al_off, out.al_ref = al_key.ctypes.data, al_off.ctypes.data, al_ref.ctypes.data
    call()
    rows = [seqs[k * len(ref):(k + 1) * len(ref)].tobytes().decode("ascii") for k in range(nr)]
    labels = unphased_snv_labels(groups, sample_off, idx, sel, vt, samples, PosSegments.identity(int(startp), len(ref)), 1)
    return rows, labels, (al_key, al_off, al_ref), (sample_off, idx), sig, groups


# ---------------------------------------------------------------------------------------------- unphased indel windows
INDEL_WINDOWS = ("host", "device")
WINDOW_FLANK = 100  # haplotypes.INDEL_WINDOW, csrc/hawk_uwin.h: UW_FLANK


class IndelTable:
    """The indel alleles of a block inside the interval as given (haplotypes.indel_in_region), in (record, allele) order, as the
    arrays hawk_uwin_instances takes, and their window geometry (csrc/hawk_uwin.h states it; here it only places labels)."""

    def __init__(self, vt: "VcfVariants", is_snv: np.ndarray, region_len: int, startp: int, coord):
        ind = np.flatnonzero(~is_snv)
        ind = ind[np.lexsort((vt.allele[ind], vt.line[ind]))]
        pos = vt.pos[ind]
        ind = ind[(pos >= coord.startp) & (pos < coord.stopp)]
        self.sel = ind
        n = len(ind)
        self.line = np.ascontiguousarray(vt.line[ind], dtype=np.uint32)
        self.allele = np.ascontiguousarray(vt.allele[ind], dtype=np.uint8)
        o = vt.pos[ind] - int(startp)
        self.off = np.where((o < 0) | (o >= region_len), 0xffffffff, o).astype(np.uint32)  # (outside the sequence: the builder declines)
        refs, alts = [vt.ref[int(j)] for j in ind], [vt.alt[int(j)] for j in ind]
        self.ref_len = np.array([len(r) for r in refs], dtype=np.uint32)
        self.alt_len = np.array([len(a) for a in alts], dtype=np.uint32)
        self.pool_off = np.zeros(n, dtype=np.uint32)
        if n:
            self.pool_off[1:] = np.cumsum((self.ref_len + self.alt_len)[:-1], dtype=np.uint64).astype(np.uint32)
        text = "".join(r + a for r, a in zip(refs, alts))
        self.pool = _BASE_IDX[np.frombuffer(text.encode("latin-1", "replace"), dtype=np.uint8)] if text else np.zeros(0, np.uint8)
        # single-base refs as the allele table wants them: the index in ACGT, 255 for anything else
        first = self.pool[self.pool_off] if n else np.zeros(0, np.uint8)
        self.ref_byte = np.where(self.ref_len == 1, first, 255).astype(np.uint8)
        # geometry (valid for the indels the builder does not decline)
        o = o.astype(np.int64)
        self.o = o
        self.grow = self.alt_len.astype(np.int64) - self.ref_len.astype(np.int64)
        self.span = np.where(self.grow > 0, 1, 1 - self.grow)
        self.a = np.maximum(0, o - WINDOW_FLANK)
        self.b = np.minimum(region_len - 1, o - self.grow + WINDOW_FLANK)
        self.rowlen = self.b - self.a + 1 + self.grow
        self.i = o - self.a

    def __len__(self) -> int:
        return len(self.sel)

    def c_input(self, rank_sample: np.ndarray, ref: np.ndarray):
        """(hawk_uwin_input, the arrays it points into)"""
        from . import _lib
        keep = (self.line, self.allele, self.off, self.ref_len, self.alt_len, self.pool_off, self.pool, rank_sample, ref)
        inp = _lib.UwinInput(len(self), len(ref), self.line.ctypes.data, self.allele.ctypes.data, self.off.ctypes.data, self.ref_len.ctypes.data,
                             self.alt_len.ctypes.data, self.pool_off.ctypes.data, self.pool.ctypes.data, len(self.pool), rank_sample.ctypes.data,
                             ref.ctypes.data)
        return inp, keep

    def segments(self, k: int, startp: int) -> PosSegments:
        """expand_haplotype's position map of indel k's rows: identity from the window's start, a deletion's jump behind the anchor,
        an insertion's bases on the anchor's position; a segment opening at the row's end is dropped"""
        i, grow, g0 = int(self.i[k]), int(self.grow[k]), int(startp) + int(self.o[k])
        if grow < 0:
            rel, gen = [0, i + 1], [int(startp) + int(self.a[k]), g0 + 1 - grow]
        else:
            rel = [0] + list(range(i + 1, i + grow + 2))
            gen = [int(startp) + int(self.a[k])] + [g0] * grow + [g0 + 1]
        rel, gen = np.asarray(rel, dtype=np.uint32), np.asarray(gen, dtype=np.int64)
        keep = rel < int(self.rowlen[k])
        return PosSegments(rel[keep], gen[keep], int(self.rowlen[k]))


def _window_scan(seg: PosSegments, lo: int, hi: int, region_start: int, region_stop: int, pamlen: int) -> Tuple[int, int]:
    """search_guides.compute_scan_start_stop for a window haplotype that covers [lo, hi], from its segments (KeyError where the
    reverse position map lacks the position, as there)"""
    def rev(p):
        r = seg.rev(p)
        if r < 0:
            raise KeyError(p)
        return r
    stop_p = min(region_stop - WINDOW_FLANK, hi)
    if stop_p == region_stop - WINDOW_FLANK and seg.rev(stop_p) < 0:
        for p in range(stop_p, seg.max_gen() + 1):
            if seg.rev(p) >= 0:
                stop_p = p
                break
    scan_stop = rev(stop_p) - pamlen + 1
    return rev(max(region_start + WINDOW_FLANK, lo)), scan_stop


def _flat_ranges(lo: np.ndarray, hi: np.ndarray):
    """ranges [lo[k], hi[k]) laid end to end: (the flat indices, the range each one belongs to)"""
    n = (hi - lo).astype(np.int64)
    owner = np.repeat(np.arange(len(n), dtype=np.int64), n)
    start = np.concatenate(([0], np.cumsum(n)[:-1])) if len(n) else np.zeros(0, np.int64)
    return lo.astype(np.int64)[owner] + (np.arange(int(n.sum()), dtype=np.int64) - start[owner]), owner


def unphased_window_rows(wt: IndelTable, inst_off: np.ndarray, inst_sample: np.ndarray, inst_lo: np.ndarray, inst_hi: np.ndarray, head: np.ndarray,
                         idx: np.ndarray, sel: np.ndarray, v_off: np.ndarray, v_ref: np.ndarray, vt: "VcfVariants", samples: List[str], startp: int,
                         region_start: int, region_stop: int, pamlen: int, row_base: int):
    """The distinct window rows of (instances, heads) - hawk_uwin_* or hawk_host_unphased_windows - with everything
    haplotypes.unphased_indel_windows attaches to them: -> (row_inst: the head instance of every row, in row order; hap_len;
    [RowLabel] with ids from hap_{row_base}; [HostHaplotype] without sequences: segments and scan bounds; the rows' allele table
    (key, off, ref) with off[0] == 0).  Labels: samples = the members' names (instances come in name order), variants = the sorted
    union of the members' own id strings (a member's SNVs in list order, skipped ones included, then the indel), afs of the head."""
    n_inst = len(head)
    inst_indel = np.repeat(np.arange(len(wt), dtype=np.int64), np.diff(inst_off.astype(np.int64)))
    head = head.astype(np.int64)
    is_head = head == np.arange(n_inst)
    row_inst = np.flatnonzero(is_head)
    n_rows = len(row_inst)
    row_of_inst = (np.cumsum(is_head) - 1)[head] if n_inst else np.zeros(0, np.int64)
    row_indel = inst_indel[row_inst]
    hap_len = wt.rowlen[row_indel].astype(np.uint32)
    lo, hi = inst_lo.astype(np.int64), inst_hi.astype(np.int64)
    # members whose entries are not their head's, one by one: the only ones that add a variants string of their own
    same = (hi - lo) == (hi - lo)[head]
    cand = np.flatnonzero(same & ~is_head & (hi > lo))
    if len(cand):
        mine, owner = _flat_ranges(lo[cand], hi[cand])
        theirs = lo[head[cand]][owner] + (mine - lo[cand][owner])
        differs = np.zeros(len(cand), dtype=bool)
        np.logical_or.at(differs, owner, idx[mine] != idx[theirs])
        same[cand[differs]] = False
    ids = vt.id
    text = lambda k: ",".join([ids[int(sel[j])] for j in idx[lo[k]:hi[k]].tolist()] + [ids[int(wt.sel[inst_indel[k]])]])
    strings = [{text(int(k))} for k in row_inst]
    for k in np.flatnonzero(~same).tolist():
        strings[int(row_of_inst[k])].add(text(k))
    order = np.argsort(row_of_inst, kind="stable")
    names = np.asarray(samples, dtype=object)[inst_sample[order]]
    cuts = np.concatenate(([0], np.cumsum(np.bincount(row_of_inst, minlength=n_rows)))) if n_inst else np.zeros(1, np.int64)
    segs = {int(k): wt.segments(int(k), startp) for k in np.unique(row_indel)}
    scans = {k: _window_scan(s, int(startp) + int(wt.a[k]), int(startp) + int(wt.b[k]), region_start, region_stop, pamlen) for k, s in segs.items()}
    labels, meta = [], []
    for r in range(n_rows):
        k, w = int(row_inst[r]), int(row_indel[r])
        members = names[cuts[r]:cuts[r + 1]].tolist()
        var_ids = [ids[int(sel[j])] for j in idx[lo[k]:hi[k]].tolist()] + [ids[int(wt.sel[w])]]
        afs = {}
        for j in idx[lo[k]:hi[k]].tolist():
            afs[ids[int(sel[j])]] = vt.af[int(sel[j])]
        afs[var_ids[-1]] = vt.af[int(wt.sel[w])]
        labels.append(RowLabel(",".join(sorted(set(members))), ",".join(sorted(strings[r])), afs, f"hap_{row_base + r:08d}", segs[w]))
        meta.append(HostHaplotype(b"", segs[w], False, scans[w]))
    # the allele table: the head's applied sites that are not strictly inside a deleted span, at their row positions, and the indel
    # behind the anchor's own alleles
    e, owner = _flat_ranges(lo[row_inst], hi[row_inst])
    w = row_indel[owner]
    off = v_off[idx[e]].astype(np.int64)
    a, o, grow = wt.a[w], wt.o[w], wt.grow[w]
    keep = (off - a < wt.rowlen[w]) & ~((off > o) & (off < o + wt.span[w]))
    e, owner, off, a, o, grow = e[keep], owner[keep], off[keep], a[keep], o[keep], grow[keep]
    pos = np.where(off <= o, off - a, off - a + grow)
    rows = np.concatenate((owner, np.arange(n_rows, dtype=np.int64)))
    pos = np.concatenate((pos, wt.i[row_indel]))
    refb = np.concatenate((v_ref[idx[e]].astype(np.uint8), wt.ref_byte[row_indel]))
    late = np.concatenate((np.zeros(len(e), np.int64), np.ones(n_rows, np.int64)))
    order = np.lexsort((late, pos, rows))
    e_key = ((rows[order] + row_base).astype(np.uint64) << np.uint64(32)) | pos[order].astype(np.uint64)
    first = np.flatnonzero(np.concatenate(([True], e_key[1:] != e_key[:-1]))) if len(e_key) else np.zeros(0, np.int64)
    alleles = (e_key[first], np.concatenate((first, [len(e_key)])).astype(np.uint32), refb[order])
    return row_inst.astype(np.uint32), hap_len, labels, meta, alleles


def _name_ranks(samples: List[str]) -> np.ndarray:
    """the sample columns in the order of their sorted names (the order unphased_indel_windows walks an indel's carriers in)"""
    return np.asarray(sorted(range(len(samples)), key=lambda s: samples[s]), dtype=np.uint32)


def unphased_windows_host(region_seq: str, startp: int, block, samples: List[str], codes: np.ndarray, coord, pamlen: int, row_base: int = 1,
                          forged_sig: Optional[np.ndarray] = None):
    """The indel-window rows of an unphased block by the host twin (hawk_host_unphased_windows over the lists of
    hawk_host_unphased_rows; no device).  -> dict(rows: the row strings, labels, meta, alleles, hap_len, row_inst, inst_off,
    inst_sample, inst_lo, inst_hi, sig, head, table: the IndelTable).  `forged_sig` [n_inst][2] replaces the signatures the grouping
    reads.  Raises _lib.UnphasedBuildDeclined as expand_unphased_from_vcf(indel_windows="device") does."""
    import ctypes as C
    from . import _lib
    from ._lib import UnphasedBuildDeclined
    vt = VcfVariants(block)
    ref = np.frombuffer(region_seq.encode("latin-1", "replace"), dtype=np.uint8)
    sel, v_line, v_allele, v_off, v_mask, v_ref = unphased_snv_table(block, vt, len(ref), startp)
    _, _, _, (sample_off, idx), _, _ = unphased_rows_host(region_seq, startp, block, samples, codes)
    is_snv = np.zeros(len(vt), dtype=bool)
    is_snv[sel] = True
    wt = IndelTable(vt, is_snv, len(ref), startp, coord)
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    inp, keep = wt.c_input(_name_ranks(samples), ref)
    lists = _lib.UwinLists(codes.ctypes.data, len(block), len(samples), len(sel), sample_off.ctypes.data, idx.ctypes.data, v_off.ctypes.data,
                           v_mask.ctypes.data, v_ref.ctypes.data)
    out, dec = _lib.UwinRows(), _lib.UbuildDecline()
    L = _lib.lib()

    def call():
        rc = L.hawk_host_unphased_windows(C.byref(inp), C.byref(lists), C.byref(out), C.byref(dec))
        if rc != _lib.HAWK_OK and dec.reason:
            raise UnphasedBuildDeclined(int(dec.reason), vt.id[int(wt.sel[dec.var])] if dec.var >= 0 else "")
        _lib.check(rc, "hawk_host_unphased_windows")
    if forged_sig is not None:
        forged_sig = np.ascontiguousarray(forged_sig, dtype=np.uint64)
        out.forged_sig = forged_sig.ctypes.data
    call()  # the counts; then buffers of exactly their size
    ni, nr, nq = int(out.n_inst), int(out.n_rows), int(out.n_seq)
    inst_off = np.zeros(len(wt) + 1, np.uint64)
    inst_sample, inst_lo, inst_hi = np.zeros(ni, np.uint32), np.zeros(ni, np.uint64), np.zeros(ni, np.uint64)
    sig, head, seqs, seq_off = np.zeros((ni, 2), np.uint64), np.zeros(ni, np.uint32), np.zeros(nq, np.uint8), np.zeros(nr + 1, np.uint64)
    out.inst_cap, out.row_cap, out.seq_cap = ni, nr, nq
    out.inst_off, out.inst_sample, out.inst_lo, out.inst_hi = inst_off.ctypes.data, inst_sample.ctypes.data, inst_lo.ctypes.data, inst_hi.ctypes.data
    out.sig, out.head, out.seqs, out.seq_off = sig.ctypes.data, head.ctypes.data, seqs.ctypes.data, seq_off.ctypes.data
    call()
    del keep
    row_inst, hap_len, labels, meta, alleles = unphased_window_rows(wt, inst_off, inst_sample, inst_lo, inst_hi, head, idx, sel, v_off, v_ref, vt, samples,
                                                                    startp, coord.start, coord.stop, pamlen, row_base)
    rows = [seqs[int(seq_off[k]):int(seq_off[k + 1])].tobytes().decode("ascii") for k in range(nr)]
    return dict(rows=rows, labels=labels, meta=meta, alleles=alleles, hap_len=hap_len, row_inst=row_inst, inst_off=inst_off, inst_sample=inst_sample,
                inst_lo=inst_lo, inst_hi=inst_hi, sig=sig, head=head, table=wt)


def expand_unphased_from_vcf(region_seq: str, startp: int, stopp: int, block, samples: List[str], pamlen: int, device: Optional[int] = None,
                             coord=None, debug: bool = True, indel_windows: str = "host"):
    """The haplotype set of an unphased interval with its whole-region rows built on the device: what
    search_guides._device_set(region, haplotypes.add_variants_unphased(...), pamlen) holds, row for row - REF, then one IUPAC row
    per distinct carrier of SNVs (hawk_gt_parse_unphased -> hawk_ubuild_lists -> hawk_ubuild_signatures -> hawk_ubuild_fill: no
    row ever exists as text), then the indel-window rows, which stay on the host builder (haplotypes.unphased_indel_windows on the
    records of the indels and of the SNVs inside their windows alone) and are packed into the same set.
    `coord`: the interval's Coordinate (default: Coordinate(contig of the block, startp, stopp, 0)).
    Returns (DeviceHapSet with is_ref / ref_index set, [RowLabel] per row, the rows' allele table (key, off, ref) in
    search_guides.flatten_variant_alleles' format, the indel-window Haplotype objects, kernel ms {parse, lists, signatures, fill}).
    `indel_windows="device"`: the window rows are built on the device too, behind the SNV rows of the same set - the indel table
    comes from VcfVariants and the block's fixed columns, the carriers of every indel from the codes in name order
    (hawk_uwin_instances), their rows are grouped on a signature over the surviving sites with an exact comparison behind it
    (hawk_uwin_signatures, hawk_uwin_group) and written by hawk_uwin_fill; labels, segments, scan bounds and the allele-table tail
    come from the instance arrays (unphased_window_rows).  No VariantRecord, no Haplotype, no row string; the fourth return value
    is then [], and the ms dict gains window_instances, window_signatures, window_groups and window_fill.
    Raises _lib.UnphasedBuildDeclined where the builder declines (include/hawk.h: HAWK_UBUILD_*); nothing is left allocated."""
    import ctypes as C
    from . import _lib
    from . import haplotypes as hap_mod
    from ._lib import UnphasedBuildDeclined
    from .coordinate import Coordinate
    from .haplotype import Haplotype
    from .hapset import DeviceHapSet, _p
    from .region import Region
    from .search_guides import compute_scan_start_stop, flatten_variant_alleles
    from .sequence import Sequence as Seq_
    from .variant import VTYPES, VariantRecord
    if len(block) == 0:
        raise ValueError("expand_unphased_from_vcf needs the records of the interval")
    if indel_windows not in INDEL_WINDOWS:
        raise ValueError(f"indel_windows {indel_windows!r}: 'host' or 'device'")
    try:
        vt = VcfVariants(block)
    except ValueError as e:
        raise UnphasedBuildDeclined(0, str(e)) from e
    L = _lib.lib()
    ctx = _lib.context(device)
    n_ref = len(region_seq)
    sel, v_line, v_allele, v_off, v_mask, v_ref = unphased_snv_table(block, vt, n_ref, startp)
    ms = {"parse": 0.0, "lists": 0.0, "signatures": 0.0, "fill": 0.0}
    if coord is None:
        coord = Coordinate(block.fixed[0][0], int(startp), int(stopp), 0)
    seq_obj = Seq_(region_seq, debug)
    region = Region(seq_obj, coord)                         # the Region and the REF haplotype the host route builds
    ref_hap = Haplotype(seq_obj, coord, False, 0, debug)
    g, u, ds, uw = C.c_void_p(), C.c_void_p(), None, C.c_void_p()
    t = C.c_float(0)
    is_snv = np.zeros(len(vt), dtype=bool)
    is_snv[sel] = True
    wt = IndelTable(vt, is_snv, n_ref, startp, coord) if indel_windows == "device" else None
    text = np.ascontiguousarray(block.text)
    _lib.check(L.hawk_gt_parse_unphased(ctx, _p(text), C.c_uint64(len(text)), _p(block.line_off), _p(block.gt_off), C.c_uint64(len(block)),
                                        len(samples), C.byref(g), C.byref(t)), "hawk_gt_parse_unphased")
    ms["parse"] = float(t.value)
    try:
        flags = np.zeros(len(block), dtype=np.uint8)
        _lib.check(L.hawk_gt_codes(g, None, _p(flags)), "hawk_gt_codes")
        if np.any(flags):
            i = int(np.flatnonzero(flags)[0])
            raise UnphasedBuildDeclined(1, f"record {i}, flags {int(flags[i])}")
        # ---- the distinct whole-region rows, from the lists
        groups: List[List[int]] = []
        sample_off = np.zeros(len(samples) + 1, dtype=np.uint64)
        idx = np.zeros(0, dtype=np.uint32)
        if len(sel) or (wt is not None and len(wt)):
            rc = L.hawk_ubuild_lists(g, _p(v_line), _p(v_allele), _p(v_off), _p(v_mask), _p(v_ref), len(sel), _p(sample_off), C.byref(u), C.byref(t))
            if rc == _lib.HAWK_E_CAPACITY:
                raise UnphasedBuildDeclined(6)
            _lib.check(rc, "hawk_ubuild_lists")
            ms["lists"] = float(t.value)
            if int(sample_off[-1]):
                sig = np.zeros((len(samples), 2), dtype=np.uint64)
                dec = C.c_int64(-1)
                rc = L.hawk_ubuild_signatures(u, _p(sig), C.byref(dec), C.byref(t))
                if rc == _lib.HAWK_E_UNSUPPORTED and dec.value >= 0:
                    raise UnphasedBuildDeclined(7, vt.id[int(sel[dec.value])])
                _lib.check(rc, "hawk_ubuild_signatures")
                ms["signatures"] = float(t.value)
                idx = np.zeros(int(sample_off[-1]), dtype=np.uint32)
                _lib.check(L.hawk_ubuild_lists_download(u, _p(idx)), "hawk_ubuild_lists_download")
                # REF holds the ref base of every variant somebody carries (the fill kernel checks the sites of the rows it writes,
                # which are each group's first member's: a later member's record is checked here)
                carried = np.unique(idx)
                wrong = np.flatnonzero(_BASE_IDX[ref_hap.array[v_off[carried]]] != v_ref[carried])
                if len(wrong):
                    raise UnphasedBuildDeclined(4, vt.id[int(sel[carried[wrong[0]]])])
                groups = group_unphased_rows(sample_off, idx, sig, v_off, v_mask, v_ref)
        n_snv_rows = len(groups)
        # ---- the indel windows, on the host: the records of the indels and of the SNVs inside their windows
        windows = []
        indel_lines = sorted(set(vt.line[~is_snv].tolist())) if wt is None else []
        win = None  # the device's window rows: (row_inst, hap_len, labels, meta, alleles)
        if wt is not None and len(wt):
            ms.update(window_instances=0.0, window_signatures=0.0, window_groups=0.0, window_fill=0.0)
            ref_bytes = np.frombuffer(region_seq.encode("latin-1", "replace"), dtype=np.uint8)
            inp, keep = wt.c_input(_name_ranks(samples), ref_bytes)
            inst_off = np.zeros(len(wt) + 1, dtype=np.uint64)
            wdec = _lib.UbuildDecline()

            def declined(rc, where):
                if rc == _lib.HAWK_E_UNSUPPORTED and wdec.reason:
                    raise UnphasedBuildDeclined(int(wdec.reason), vt.id[int(wt.sel[wdec.var])] if wdec.var >= 0 else "")
                _lib.check(rc, where)
            declined(L.hawk_uwin_instances(g, u, C.byref(inp), _p(inst_off), C.byref(uw), C.byref(wdec), C.byref(t)), "hawk_uwin_instances")
            del keep
            ms["window_instances"] = float(t.value)
            n_inst = int(inst_off[-1])
            inst_sample, inst_lo, inst_hi = np.zeros(n_inst, np.uint32), np.zeros(n_inst, np.uint64), np.zeros(n_inst, np.uint64)
            wsig, whead = np.zeros((n_inst, 2), np.uint64), np.zeros(n_inst, np.uint32)
            _lib.check(L.hawk_uwin_download(uw, _p(inst_sample), _p(inst_lo), _p(inst_hi)), "hawk_uwin_download")
            declined(L.hawk_uwin_signatures(uw, _p(wsig), C.byref(wdec), C.byref(t)), "hawk_uwin_signatures")
            ms["window_signatures"] = float(t.value)
            _lib.check(L.hawk_uwin_group(uw, _p(wsig), _p(whead), C.byref(t)), "hawk_uwin_group")
            ms["window_groups"] = float(t.value)
            win = unphased_window_rows(wt, inst_off, inst_sample, inst_lo, inst_hi, whead, idx, sel, v_off, v_ref, vt, samples, startp,
                                       region.start, region.stop, pamlen, 1 + n_snv_rows)
        if indel_lines:
            recs: Dict[int, VariantRecord] = {}

            def record(i: int) -> VariantRecord:
                if i not in recs:
                    v = VariantRecord(debug)
                    a, b = int(block.line_off[i]), int(block.line_off[i + 1])
                    v.read_vcf_line(bytes(text[a:b]).decode().strip().split(), samples, False)
                    recs[i] = v
                return recs[i]
            indels = [a for i in indel_lines for a in record(i).split() if a.vtype[0] != VTYPES[0]]
            near = np.zeros(len(sel), dtype=bool)
            snv_pos = vt.pos[sel]
            for a in indels:
                if hap_mod.indel_in_region(region, a) and len(a.samples) and a.samples[0][0]:
                    _, lo, hi = hap_mod._Stretch.around(region, a)
                    near |= (snv_pos >= lo) & (snv_pos <= hi)
            snvs = [a for i in sorted(set(v_line[near].tolist())) for a in record(i).split() if a.vtype[0] == VTYPES[0]]
            windows = hap_mod.unphased_indel_windows(region, indels, snvs, False, debug)
        # ---- the set: REF, the SNV rows, the window rows
        hap_len = np.array([n_ref] * (1 + n_snv_rows) + [len(w.sequence) for w in windows], dtype=np.uint32)
        if win is not None:
            hap_len = np.concatenate((hap_len, win[1]))
        ds = DeviceHapSet.allocate(hap_len, device)
        ds.pack_rows(0, [ref_hap.array])
        ds.pack_rows(1 + n_snv_rows, [w.array for w in windows])
        if win is not None and len(win[0]):
            _lib.check(L.hawk_uwin_fill(uw, ds._h, 0, 1 + n_snv_rows, len(win[0]), _p(win[0]), C.byref(t)), "hawk_uwin_fill")
            ms["window_fill"] = float(t.value)
        if n_snv_rows:
            row_sample = np.array([m[0] for m in groups], dtype=np.uint32)
            dec = C.c_int64(-1)
            rc = L.hawk_ubuild_fill(u, ds._h, 0, 1, n_snv_rows, _p(row_sample), C.byref(dec), C.byref(t))
            if rc == _lib.HAWK_E_UNSUPPORTED and dec.value >= 0:
                raise UnphasedBuildDeclined(4, vt.id[int(sel[dec.value])])
            _lib.check(rc, "hawk_ubuild_fill")
            ms["fill"] = float(t.value)
        ref_scan = compute_scan_start_stop(ref_hap, region.start, region.stop, pamlen)
        meta = [HostHaplotype(b"", ref_hap.segments, True, ref_scan)] + [HostHaplotype(b"", ref_hap.segments, False, ref_scan)] * n_snv_rows
        meta += [HostHaplotype(b"", w.segments, w.samples == "REF", compute_scan_start_stop(w, region.start, region.stop, pamlen)) for w in windows]
        if win is not None:
            meta += win[3]
        ds.set_meta(meta)
        # ---- labels and the allele table
        labels = [RowLabel("REF", "NA", {}, "hap_00000000", ref_hap.segments)]
        labels += unphased_snv_labels(groups, sample_off, idx, sel, vt, samples, ref_hap.segments, 1)
        for k, w in enumerate(windows):
            w.id = f"hap_{1 + n_snv_rows + k:08d}"
            labels.append(RowLabel(w.samples, w.variants, w.afs, w.id, w.segments))
        key, off, ref = unphased_snv_alleles(groups, sample_off, idx, v_off, v_ref, 1)
        if windows:
            k2, o2, r2 = flatten_variant_alleles(windows)
            key = np.concatenate((key, k2 + (np.uint64(1 + n_snv_rows) << np.uint64(32))))
            off = np.concatenate((off, o2[1:] + np.uint32(len(ref)))).astype(np.uint32)
            ref = np.concatenate((ref, r2)).astype(np.uint8)
        if win is not None:
            labels += win[2]
            k2, o2, r2 = win[4]
            key = np.concatenate((key, k2))
            off = np.concatenate((off, o2[1:] + np.uint32(len(ref)))).astype(np.uint32)
            ref = np.concatenate((ref, r2)).astype(np.uint8)
        out, ds = ds, None
        return out, labels, (key, off, ref), windows, ms
    finally:
        if ds is not None:
            ds.close()
        if uw:
            L.hawk_uwin_free(uw)
        if u:
            L.hawk_ubuild_free(u)
        L.hawk_gt_destroy(g)


def row_labels(reg: SynthRegion, ds, info: List[HapInfo], kept: List[int]) -> List[Optional[RowLabel]]:
    """Labels per device row of an expand_on_device() set (None for rows collapsed onto another row): samples
    joined as collapse_haplotypes does, variant ids `chr-pos-ref/alt`, allele frequencies by id."""
    vid = [f"{reg.contig}-{v.pos}-{v.ref}/{v.alt}" for v in reg.variants]
    af = {vid[i]: float(v.af) for i, v in enumerate(reg.variants)}
    out: List[Optional[RowLabel]] = [None] * ds.n_hap
    is_indel = [len(v.ref) != len(v.alt) for v in reg.variants]
    for r, inf in zip(kept, info):
        idx = [int(i) for i in inf.variant_idx]
        ids = [vid[i] for i in idx if not is_indel[i]] + [vid[i] for i in idx if is_indel[i]]  # haplotype.py:234-242
        out[r] = RowLabel(",".join(inf.samples), ",".join(ids) if ids else "NA", {k: af[k] for k in ids}, f"hap_{r:08d}",
                          ds.host_meta[r].seg)
    return out


class _LazySegments:
    """list-like: the PosSegments of a kept row on demand (host_meta[r].seg), None for rows that collapsed onto another"""

    def __init__(self, host_meta, kept, n: int):
        self._hm, self._kept, self._n = host_meta, set(int(r) for r in kept), n

    def __len__(self):
        return self._n

    def __getitem__(self, r):
        r = int(r)
        return self._hm[r].seg if r in self._kept else None


def hap_labels(contig: str, variants, ds, info: List[HapInfo], kept: List[int]):
    """reports.HapLabels of an expanded set, straight from the carried-variant index lists (no per-row id strings):
    `variants` = the variant records in table order with .pos .ref .alt .af (synth.VariantSite) or a VcfVariants."""
    from .reports import HapLabels
    if hasattr(variants, "id"):
        vid, af = list(variants.id), np.asarray(variants.af, dtype=np.float64)
    else:
        vid = [f"{contig}-{v.pos}-{v.ref}/{v.alt}" for v in variants]
        af = np.array([float(v.af) for v in variants], dtype=np.float64)
    n = ds.n_hap
    samples, ids = [""] * n, [""] * n
    hm = ds.host_meta
    segs = _LazySegments(hm, kept, n)  # a row's PosSegments only when the report's Python fallback asks for it
    is_ref = np.zeros(n, dtype=bool)
    cnt = np.zeros(n, dtype=np.int64)
    parts = []
    for k, (r, inf) in enumerate(zip(kept, info)):
        samples[r] = ",".join(inf.samples)
        ids[r] = f"hap_{k:08d}"
        is_ref[r] = r == 0 or samples[r] == "REF"
        idx = np.asarray(inf.variant_idx, dtype=np.int64)
        cnt[r] = len(idx)
    order = np.argsort(np.asarray(kept))
    for j in order.tolist():
        parts.append(np.asarray(info[j].variant_idx, dtype=np.int64))
    var_idx = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    lab = HapLabels(samples, ids, is_ref, np.concatenate(([0], np.cumsum(cnt))), var_idx, vid, af, segs)
    if hasattr(hm, "seg_start"):  # the rows' position maps as flat CSR arrays: what the library's polish helper walks
        lab.seg_csr = (np.ascontiguousarray(hm.seg_start, dtype=np.uint64), np.ascontiguousarray(hm.seg_rel, dtype=np.uint32),
                       np.ascontiguousarray(hm.seg_gen, dtype=np.int64))
    return lab
