"""The BGZF inflate panel: members (whole gzip members as bgzip frames them) with the text they must give, or that they must fail.

The judge is zlib: a member's text is what `zlib.decompressobj(-15)` makes of its deflate stream - the library the Python route
(`readers._TextSource._inflate`) calls - and "must fail" means zlib raises `zlib.error` or stops before the stream's end (which
`zlib.decompress` raises as well).  `Member.judged` members are checked against it when the panel is built, so a mistake in the bit
writer below shows here and not as a decoder failure.  What zlib does not see - the gzip header and ISIZE - fails by the rules of
csrc/hawk_inflate.h, with the status named there.

zlib's own encoder cannot write most of what has to be tested (a distance above 32506, a 15-bit code, a repeat code that crosses
from the literal/length lengths into the distance lengths, any malformed stream), so `BitWriter` and the block functions emit
stored, fixed and dynamic blocks from explicit token lists and code lengths.  A token is a literal (0..255) or a (length,
distance) pair.

One case the issue lists as valid cannot be: HCLEN = 4 transmits the lengths of the code-length symbols 16, 17, 18 and 0 only, so
every literal/length length is 0, there is no code for 256, and zlib refuses the block ("missing end-of-block").  The member is in
the panel with zlib's verdict; HCLEN = 5 (which adds 8: 256 codes of 8 bits) is the smallest header that can be valid and is there too.

`python tests/bgzf_refs.py --write` rewrites tests/golden/bgzf_panel.bin, what csrc/inflate_check_main.cpp (make asan-inflate) reads.
"""
import os
import struct
import zlib
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "bgzf_panel.bin")

# include/hawk.h
BZ_OK, BZ_HEADER, BZ_UNSUPPORTED, BZ_INPUT, BZ_SIZE, BZ_BLOCK, BZ_CODE, BZ_SYMBOL, BZ_DISTANCE = range(9)
ANY_FAILURE = 255

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
# a complete code over all 19 code-length symbols: 13 of 4 bits, 6 of 5
CL_LENS_ALL = [4] * 13 + [5] * 6
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32

# text None: the member must fail; status: the HAWK_BZ_* it must end in (ANY_FAILURE: any but OK); judged: zlib decides, and is asked;
# built: written by the bit writer (the same bytes wherever the panel is built), not by zlib's encoder
Member = namedtuple("Member", "raw text status judged built")


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, n):  # the value's lowest bit first
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):  # a Huffman code: its highest bit first
        for i in range(length - 1, -1, -1):
            self.bits(code >> i & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def nbits(self):
        return 8 * len(self.out) + self.n

    def value(self):
        w = bytes(self.out)
        return w + bytes([self.acc]) if self.n else w


def canonical(lens):
    """symbol -> (code, length), RFC 1951 3.2.2; the lengths need not make a complete set"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def flat_lens(symbols, n):
    """a complete code over `symbols` with lengths as equal as they can be (one symbol: a single code of one bit)"""
    m = len(symbols)
    lens = [0] * n
    if m == 1:
        lens[symbols[0]] = 1
        return lens
    k = (m - 1).bit_length()
    short = (1 << k) - m
    for i, s in enumerate(sorted(symbols)):
        lens[s] = k - 1 if i < short else k
    return lens


def len_symbol(length):
    s = max(i for i in range(29) if LEN_BASE[i] <= length) if length < 258 else 28
    return s, length - LEN_BASE[s]


def dist_symbol(dist):
    s = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return s, dist - DIST_BASE[s]


def apply_tokens(tokens, text=b""):
    out = bytearray(text)
    for t in tokens:
        if isinstance(t, tuple):
            length, dist = t
            assert 0 < dist <= len(out)
            for _ in range(length):
                out.append(out[-dist])
        else:
            out.append(t)
    return bytes(out)


def put_tokens(w, tokens, lit, dist):
    for t in tokens:
        if isinstance(t, tuple):
            s, e = len_symbol(t[0])
            w.code(*lit[257 + s])
            w.bits(e, LEN_EXTRA[s])
            d, e = dist_symbol(t[1])
            w.code(*dist[d])
            w.bits(e, DIST_EXTRA[d])
        else:
            w.code(*lit[t])
    w.code(*lit[256])


def stored_block(w, data, final=1, nlen=None):
    w.bits(final, 1)
    w.bits(0, 2)
    w.align()
    w.bits(len(data), 16)
    w.bits(len(data) ^ 0xffff if nlen is None else nlen, 16)
    w.raw(data)


def fixed_block(w, tokens, final=1):
    w.bits(final, 1)
    w.bits(1, 2)
    put_tokens(w, tokens, canonical(FIXED_LIT), canonical(FIXED_DIST))


def used_lens(tokens, extra_lit=(), extra_dist=()):
    """flat complete codes over the symbols the tokens use (plus 256): (lit_lens up to the last used symbol, at least 257; dist_lens)"""
    lit, dist = {256, *extra_lit}, set(extra_dist)
    for t in tokens:
        if isinstance(t, tuple):
            lit.add(257 + len_symbol(t[0])[0])
            dist.add(dist_symbol(t[1])[0])
        else:
            lit.add(t)
    ll = flat_lens(sorted(lit), max(max(lit) + 1, 257))
    dl = flat_lens(sorted(dist), max(dist) + 1) if dist else [0]
    return ll, dl


def dynamic_block(w, tokens, final=1, lit_lens=None, dist_lens=None, cl_items=None, cl_lens=None, hclen=19, put=True):
    """lit_lens: HLIT lengths (257..286 of them, or whatever a malformed header is to claim), dist_lens: HDIST lengths; cl_items: how
    the HLIT + HDIST lengths are transmitted, a list of (code-length symbol, value of its extra bits) - default: one symbol < 16 per
    length; cl_lens: the lengths of the 19 code-length symbols, of which the first `hclen` in the header's order are written"""
    if lit_lens is None:
        lit_lens, dist_lens = used_lens(tokens)
    if cl_items is None:
        cl_items = [(l, 0) for l in list(lit_lens) + list(dist_lens)]
    cl_lens = CL_LENS_ALL if cl_lens is None else cl_lens
    w.bits(final, 1)
    w.bits(2, 2)
    w.bits(len(lit_lens) - 257, 5)
    w.bits(len(dist_lens) - 1, 5)
    w.bits(hclen - 4, 4)
    for i in range(hclen):
        w.bits(cl_lens[CL_ORDER[i]], 3)
    cl = canonical(cl_lens)
    for s, e in cl_items:
        w.code(*cl[s])
        if s >= 16:
            w.bits(e, {16: 2, 17: 3, 18: 7}[s])
    if put:
        put_tokens(w, tokens, canonical(lit_lens), canonical(dist_lens))


def frame(deflate, isize, flg=4, magic=b"\x1f\x8b", text=None, after_extra=b""):
    """a BGZF member around a deflate stream: the BC extra field holds the member's size - 1, the trailer a CRC32 nobody checks"""
    bsize = 12 + 6 + len(after_extra) + len(deflate) + 8 - 1
    crc = zlib.crc32(text) & 0xffffffff if text is not None else 0
    return (magic + b"\x08" + bytes([flg]) + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize & 0xffff) +
            after_extra + deflate + struct.pack("<II", crc, isize))


def zlib_verdict(deflate):
    """the text zlib gives, or None when it refuses the stream or the stream ends before its final block does"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(deflate)
    except zlib.error:
        return None
    return out if d.eof else None


def good(deflate, text, built=True):
    assert zlib_verdict(deflate) == text, "the panel's own stream is not what zlib reads"
    assert len(text) <= 65536
    return Member(frame(deflate, len(text), text=text), text, BZ_OK, True, built)


def bad(deflate, isize, status=ANY_FAILURE):
    assert zlib_verdict(deflate) is None, "zlib accepts a stream the panel calls malformed"
    return Member(frame(deflate, isize), None, status, True, True)


def from_tokens(kind, tokens, **kw):
    w = BitWriter()
    (fixed_block if kind == "fixed" else dynamic_block)(w, tokens, **kw)
    return good(w.value(), apply_tokens(tokens))


def zlib_member(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), flush_mode=zlib.Z_SYNC_FLUSH):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, last = b"", 0
    for cut in flush_at:
        out += c.compress(text[last:cut]) + c.flush(flush_mode)
        last = cut
    out += c.compress(text[last:]) + c.flush()
    return good(out, text, built=False)


def vcf_text(n_bytes, seed=1):
    """VCF-like lines (a header, then records with phased genotypes) from a small generator of its own: n_bytes of them"""
    state = [seed * 2654435761 % (1 << 32) or 1]

    def rnd(k):
        state[0] = (state[0] * 1103515245 + 12345) % (1 << 31)
        return (state[0] >> 8) % k
    lines = ["##fileformat=VCFv4.2", "##contig=<ID=chr7>", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(f"S{i:03d}" for i in range(24))]
    pos, size = 10000, sum(len(l) + 1 for l in lines)
    while size < n_bytes:
        pos += 1 + rnd(300)
        ref, alt = "ACGT"[rnd(4)], "ACGT"[rnd(4)] + ("" if rnd(5) else "ACGT"[rnd(4)] * (1 + rnd(3)))
        gts = "\t".join(f"{int(rnd(7) == 0)}|{int(rnd(9) == 0)}" for _ in range(24))
        lines.append(f"chr7\t{pos}\trs{rnd(10 ** 7)}\t{ref}\t{alt}\t{rnd(1000)}\tPASS\tAF=0.{rnd(10 ** 4):04d};AC={rnd(48)}\tGT\t{gts}")
        size += len(lines[-1]) + 1
    return ("\n".join(lines) + "\n").encode()[:n_bytes]


def noise(n, seed=7):
    """bytes no encoder shortens (literal runs, stored payloads)"""
    out, x = bytearray(), seed
    for _ in range(n):
        x = (x * 1103515245 + 12345) % (1 << 31)
        out.append((x >> 11) & 255)
    return bytes(out)


_PANEL = None


def panel():
    """name -> [Member, ...], in a fixed order"""
    global _PANEL
    if _PANEL is not None:
        return _PANEL
    from crisprhawk_hip.readers import _bgzf_member
    P = {}
    text = vcf_text(0xff00)
    end_marker = Member(_bgzf_member(b""), b"", BZ_OK, True, False)
    assert len(end_marker.raw) == 28
    full = [Member(_bgzf_member(text), text, BZ_OK, True, False), Member(_bgzf_member(vcf_text(0xff00, 2)), vcf_text(0xff00, 2), BZ_OK, True, False)]
    P["end_marker"] = [end_marker]
    P["end_marker_between_full"] = [full[0], end_marker, full[1]]

    # ---- stored blocks
    def stored(*pieces, **kw):
        w = BitWriter()
        for i, p in enumerate(pieces):
            stored_block(w, p, final=int(i == len(pieces) - 1), **kw)
        return w.value()
    big = noise(65536)
    for n in (0, 1, 65535):
        P[f"stored_{n}"] = [good(stored(big[:n]), big[:n])]
    stored_65536 = good(stored(big[:65535], big[65535:]), big)
    P["stored_two_blocks_65536"] = [stored_65536]
    w = BitWriter()
    fixed_block(w, list(b"fixed, then"), final=0)  # 3 + 11 * 8 + 7 bits: the block ends two bits into a byte
    assert w.nbits() % 8 == 2
    stored_block(w, b" stored after a partial byte")
    P["stored_after_fixed_mid_byte"] = [good(w.value(), b"fixed, then stored after a partial byte")]

    # ---- zlib's own output
    small = vcf_text(0x5000, 3)
    for level in (1, 6, 9):
        P[f"zlib_level_{level}"] = [zlib_member(small, level)]
    P["zlib_fixed"] = [zlib_member(small, 6, zlib.Z_FIXED)]
    P["zlib_huffman_only"] = [zlib_member(small, 6, zlib.Z_HUFFMAN_ONLY)]
    P["zlib_rle"] = [zlib_member(small, 6, zlib.Z_RLE)]
    P["zlib_level_0_stored"] = [zlib_member(noise(40000, 3), 0)]
    P["zlib_sync_flush"] = [zlib_member(small, 6, flush_at=(0x1000, 0x1003, 0x3000))]
    P["zlib_full_flush"] = [zlib_member(small[:0x2000] + noise(0x800, 5) + small[0x2000:0x4000], 6, flush_at=(0x1800, 0x2400), flush_mode=zlib.Z_FULL_FLUSH)]
    P["write_bgzf_members"] = list(full)
    text64k = vcf_text(65536, 4)
    dyn_65536 = zlib_member(text64k, 6)
    P["member_65536"] = [dyn_65536]

    # ---- matches
    head = list(noise(300, 11))
    len_edges = sorted({LEN_BASE[s] + e for s in range(29) for e in (0, (1 << LEN_EXTRA[s]) - 1)} | {3, 10, 11, 257, 258})
    toks = head + [(l, 1 + (7 * l) % 300) for l in len_edges]
    P["length_edges_fixed"] = [from_tokens("fixed", toks)]
    P["length_edges_dynamic"] = [from_tokens("dynamic", toks)]
    dist_edges = sorted({DIST_BASE[s] + e for s in range(30) for e in (0, (1 << DIST_EXTRA[s]) - 1)})
    assert dist_edges[-1] == 32768
    far = list(noise(32768, 13))
    P["distance_edges_fixed"] = [from_tokens("fixed", far + [(3, d) for d in dist_edges] + [(258, 32768), (3, 1), (258, 1)])]
    P["distance_edges_dynamic"] = [from_tokens("dynamic", list(vcf_text(32768, 5)) + [(4 + i % 7, d) for i, d in enumerate(dist_edges)])]
    overlap = head[:70]
    for d in (1, 2, 3, 63, 64, 65):
        overlap += [(258, d), (max(3, d + 1), d), (max(3, 2 * d + 1), d), (max(3, d - 1), d)] + head[d:d + 3]
    P["overlap_fixed"] = [from_tokens("fixed", overlap)]
    P["overlap_dynamic"] = [from_tokens("dynamic", overlap)]
    # the decoder writes its tokens out 64 at a time: sources inside the batch being written, a chain of matches each reading the one
    # before it, a match as the last and as the first token of a batch, a match whose source straddles two batches
    same = head[:10] + [(5, 10), (7, 5), (3, 1), (20, 22), (9, 9)] + head[10:20] + [(30, 3), (4, 30)]
    P["source_in_same_batch"] = [from_tokens("fixed", same), from_tokens("dynamic", same)]
    strad = head[:63] + [(40, 63)] + [(50, 40), (258, 103)] + head[63:123] + [(100, 30)] + [(3, 2)] * 3 + head[:59] + [(12, 70), (33, 12)]
    P["batch_boundary"] = [from_tokens("fixed", strad), from_tokens("dynamic", strad)]
    runs = []
    for n in (63, 64, 65, 63, 65, 64, 64):
        runs += head[:n] + [(n, n), (3, 1)]
    P["literal_runs_63_64_65"] = [from_tokens("fixed", runs), from_tokens("dynamic", runs)]
    P["empty_blocks"] = [from_tokens("fixed", []), from_tokens("dynamic", [])]  # the latter: a single literal/length code, of one bit
    w = BitWriter()
    for i in range(5):  # several blocks of every type in one member, the batch carried across them
        fixed_block(w, head[:40] + [(9, 17)], final=0)
        dynamic_block(w, head[40:90] + [(30, 45 + i)], final=0)
        stored_block(w, bytes(head[:33 + i]), final=int(i == 4))
    many = b""
    for i in range(5):
        many = apply_tokens(head[:40] + [(9, 17)], many)
        many = apply_tokens(head[40:90] + [(30, 45 + i)], many)
        many += bytes(head[:33 + i])
    P["many_blocks"] = [good(w.value(), many)]

    # ---- dynamic headers
    A, B, EOB, L3 = 97, 98, 256, 257
    ab = [A, B, A, B, B, A]
    # 15-bit codes: lengths 1 .. 14, then two of 15
    deep = [0] * 257
    for i in range(14):
        deep[A + i] = i + 1
    deep[A + 14] = deep[EOB] = 15
    P["dyn_15_bit_codes"] = [from_tokens("dynamic", [A + i for i in range(15)] * 3 + [A + 14, A + 13, A + 9], lit_lens=deep, dist_lens=[0])]
    # HCLEN = 5: only 16, 17, 18, 0 and 8 have a code: 256 literal/length codes of 8 bits, no distance code
    cl5 = [0] * 19
    cl5[0], cl5[8], cl5[18], cl5[17], cl5[16] = 1, 2, 3, 4, 4
    lit8 = [8] * 255 + [0, 8]
    P["dyn_hclen_5"] = [from_tokens("dynamic", list(b"HCLEN five\n"), lit_lens=lit8, dist_lens=[0], cl_lens=cl5, hclen=5)]
    # HCLEN = 4: see the module's docstring; zlib decides
    cl4 = [0] * 19
    cl4[0], cl4[18], cl4[17], cl4[16] = 1, 2, 3, 3
    w = BitWriter()
    dynamic_block(w, [], lit_lens=[0] * 257, dist_lens=[0], cl_lens=cl4, hclen=4, put=False)
    w.bits(0, 16)
    verdict = zlib_verdict(w.value())
    P["dyn_hclen_4"] = [Member(frame(w.value(), len(verdict or b""), text=verdict), verdict, BZ_OK if verdict is not None else ANY_FAILURE, True, True)]
    P["dyn_hclen_19"] = [from_tokens("dynamic", head[:50] + [(5, 9)])]
    # 16 crossing: 256 -> 2 is written, a repeat of six gives 257, 258 and the four distance lengths
    ll = [0] * 259
    ll[A], ll[EOB], ll[L3], ll[L3 + 1] = 2, 2, 2, 2
    items = [(18, 97 - 11), (2, 0), (18, 138 - 11), (18, 256 - 98 - 138 - 11), (2, 0), (16, 6 - 3)]
    P["dyn_repeat_16_crosses"] = [from_tokens("dynamic", [A, A, A, (3, 1), (4, 2), (3, 3), (4, 4), A], lit_lens=ll, dist_lens=[2, 2, 2, 2], cl_items=items)]
    # 17 crossing: three zero lengths at the end of the literal/length lengths and three at the start of the distance lengths in one
    # repeat; one distance code of one bit
    ll = [0] * 261
    ll[A], ll[B], ll[EOB], ll[L3] = 2, 2, 2, 2
    items = [(18, 97 - 11), (2, 0), (2, 0), (18, 138 - 11), (18, 256 - 99 - 138 - 11), (2, 0), (2, 0), (17, 6 - 3), (1, 0)]
    P["dyn_repeat_17_crosses"] = [from_tokens("dynamic", ab + [(3, 4), A, (3, 4)], lit_lens=ll, dist_lens=[0, 0, 0, 1], cl_items=items)]
    # 18 crossing, HLIT = 286, HDIST = 30: 28 + 29 zero lengths in one repeat, the one distance code is symbol 29's
    ll = [0] * 286
    ll[A], ll[B], ll[EOB], ll[L3] = 2, 2, 2, 2
    items = items[:7] + [(18, 57 - 11), (1, 0)]
    P["dyn_repeat_18_crosses_hlit_286"] = [from_tokens("dynamic", ab * 3, lit_lens=ll, dist_lens=[0] * 29 + [1], cl_items=items)]
    P["dyn_hlit_257_no_distance_code"] = [from_tokens("dynamic", list(b"literals only, no distance code\n"))]
    P["dyn_one_distance_code"] = [from_tokens("dynamic", ab + [(3, 2), (5, 2), A, (258, 2)])]

    # ---- malformed streams
    w = BitWriter()
    w.bits(1, 1); w.bits(3, 2); w.bits(0, 13)
    P["bad_block_type_3"] = [bad(w.value(), 0, BZ_BLOCK)]
    P["bad_stored_nlen"] = [bad(stored(b"abc", nlen=0x1234), 3, BZ_BLOCK)]

    def dyn_bad(tokens=(), isize=0, **kw):
        w = BitWriter()
        dynamic_block(w, list(tokens), **kw)
        w.bits(0, 16)
        return bad(w.value(), isize)
    ll = [0] * 257
    ll[A], ll[EOB] = 1, 1
    P["bad_code_16_first"] = [dyn_bad(lit_lens=ll, dist_lens=[0], cl_items=[(16, 0)] + [(0, 0)] * 254 + [(1, 0), (0, 0)], put=False)]
    ll = [0] * 257
    ll[A], ll[B], ll[EOB] = 1, 1, 1
    P["bad_oversubscribed"] = [dyn_bad(lit_lens=ll, dist_lens=[0], put=False)]
    ll = [0] * 257
    ll[A], ll[EOB] = 2, 2
    P["bad_incomplete"] = [dyn_bad(lit_lens=ll, dist_lens=[0], put=False)]
    ll = [0] * 257
    ll[A], ll[B] = 1, 1
    P["bad_no_code_256"] = [dyn_bad(lit_lens=ll, dist_lens=[0], put=False)]
    ll = [0] * 257
    ll[A], ll[EOB] = 1, 1
    P["bad_repeat_past_the_lengths"] = [dyn_bad(lit_lens=ll, dist_lens=[0], cl_items=[(18, 127)] * 2, put=False)]
    P["bad_distance_code_incomplete"] = [dyn_bad(lit_lens=flat_lens([A, EOB, L3], 258), dist_lens=[2, 2], put=False)]
    fl, fd = canonical(FIXED_LIT), canonical(FIXED_DIST)
    w = BitWriter()
    w.bits(1, 1); w.bits(1, 2); w.code(*fl[A]); w.code(*fl[286]); w.code(*fd[0]); w.code(*fl[256]); w.bits(0, 16)
    P["bad_symbol_286"] = [bad(w.value(), 4, BZ_SYMBOL)]
    w = BitWriter()
    w.bits(1, 1); w.bits(1, 2); w.code(*fl[A]); w.code(*fl[257]); w.code(*fd[30]); w.code(*fl[256]); w.bits(0, 16)
    P["bad_distance_symbol_30"] = [bad(w.value(), 4, BZ_SYMBOL)]
    w = BitWriter()
    w.bits(1, 1); w.bits(1, 2); w.code(*fl[A]); w.code(*fl[257]); w.code(*fd[1]); w.code(*fl[256])
    P["bad_distance_too_far"] = [bad(w.value(), 4, BZ_DISTANCE)]
    # a single distance code of one bit, and the other bit is read
    ll = flat_lens([A, EOB, L3], 258)
    w = BitWriter()
    dynamic_block(w, [], lit_lens=ll, dist_lens=[1], put=False)
    lc = canonical(ll)
    w.code(*lc[A]); w.code(*lc[A]); w.code(*lc[L3]); w.bits(1, 1); w.code(*lc[EOB]); w.bits(0, 16)
    P["bad_code_not_in_set"] = [bad(w.value(), 5)]
    # the stream ends one bit / one byte before its end-of-block code does: 3 + 9 k + 7 bits with literals above 143
    for name, k, short in (("bad_one_bit_short", 7, 1), ("bad_one_byte_short", 6, 8)):
        w = BitWriter()
        fixed_block(w, [200] * k)
        assert w.nbits() % 8 == short % 8 and zlib_verdict(w.value()) == bytes([200] * k)
        P[name] = [bad(w.value()[:-1], k, BZ_INPUT)]
    w = BitWriter()
    stored_block(w, b"0123456789")
    P["bad_stored_runs_out"] = [bad(w.value()[:-3], 10, BZ_INPUT)]
    # ---- what zlib does not see: ISIZE and the gzip header
    w = BitWriter()
    fixed_block(w, list(b"sized") + [(5, 5)])
    ten = w.value()
    assert zlib_verdict(ten) == b"sizedsized"
    P["bad_isize_plus_1"] = [Member(frame(ten, 9), None, BZ_SIZE, False, True)]    # the stream gives ISIZE + 1 bytes
    P["bad_isize_minus_1"] = [Member(frame(ten, 11), None, BZ_SIZE, False, True)]  # ... ISIZE - 1
    w = BitWriter()
    stored_block(w, b"0123456789")
    P["bad_isize_stored"] = [Member(frame(w.value(), 9), None, BZ_SIZE, False, True)]
    P["bad_flg_fname"] = [Member(frame(ten, 10, flg=4 | 8, after_extra=b"name\x00"), None, BZ_UNSUPPORTED, False, True)]
    P["bad_magic"] = [Member(frame(ten, 10, magic=b"\x1f\x8c"), None, BZ_HEADER, False, True)]
    P["trailing_bytes_ignored"] = [Member(frame(ten + b"\x00\x01\x02", 10, text=b"sizedsized"), b"sizedsized", BZ_OK, False, True)]

    # ---- one workgroup's four waves: the end marker, one byte, 65536 bytes stored, 65536 bytes of dynamic blocks
    one = good(stored(b"\n"), b"\n")
    P["workgroup_of_extremes"] = [end_marker, one, stored_65536, dyn_65536]
    _PANEL = P
    return P


def unique_members():
    """every distinct member of the panel once, in panel order"""
    seen, out = set(), []
    for ms in panel().values():
        for m in ms:
            if m.raw not in seen:
                seen.add(m.raw)
                out.append(m)
    return out


def launch(n):
    """n members for one call: the workgroup of extremes first (members 0..3 are one workgroup), then valid and malformed members in
    turn, the small ones many times over"""
    u = unique_members()
    first = panel()["workgroup_of_extremes"]
    bad_ones = [m for m in u if m.text is None]
    small = [m for m in u if m.text is not None and len(m.raw) < 4096]
    out = list(first[:n])
    i = 0
    while len(out) < n:
        out.append(bad_ones[i // 2 % len(bad_ones)] if i % 2 else small[i // 2 % len(small)])
        i += 1
    return out


LAUNCH_SIZES = (1, 3, 4, 5, 63, 64, 65, 257)


def pack(members, isize_of=None):
    """(bytes of the members back to back, c_off, u_off) as the C ABI takes them; a member's text range is its ISIZE"""
    import numpy as np
    raw = b"".join(m.raw for m in members)
    c = np.zeros(len(members) + 1, np.uint64)
    u = np.zeros(len(members) + 1, np.uint64)
    for k, m in enumerate(members):
        c[k + 1] = c[k] + np.uint64(len(m.raw))
        u[k + 1] = u[k] + np.uint64(struct.unpack("<I", m.raw[-4:])[0])
    return np.frombuffer(raw, np.uint8), c, u


def check_result(members, u_off, out, status):
    """the texts of the valid members, the statuses of all"""
    for k, m in enumerate(members):
        got = bytes(out[int(u_off[k]):int(u_off[k + 1])])
        if m.text is None:
            assert status[k] != BZ_OK, f"member {k} must fail"
            if m.status != ANY_FAILURE:
                assert status[k] == m.status, f"member {k}: status {status[k]}, expected {m.status}"
        else:
            assert status[k] == BZ_OK, f"member {k}: status {status[k]}"
            assert got == m.text, f"member {k}: text differs"


def golden_bytes():
    """tests/golden/bgzf_panel.bin: 'BZPANEL1', uint32 n, then per member uint32 clen, uint32 ulen (its ISIZE), uint32 crc32 of the
    text, uint8 status (255: any failure), uint8 built, 2 bytes of padding, the member"""
    ms = unique_members()
    out = [b"BZPANEL1", struct.pack("<I", len(ms))]
    for m in ms:
        isize = struct.unpack("<I", m.raw[-4:])[0]
        out.append(struct.pack("<IIIBBH", len(m.raw), isize, zlib.crc32(m.text or b"") & 0xffffffff, m.status, int(m.built), 0))
        out.append(m.raw)
    return b"".join(out)


def read_golden(path=GOLDEN):
    blob = open(path, "rb").read()
    assert blob[:8] == b"BZPANEL1"
    n, at, out = struct.unpack_from("<I", blob, 8)[0], 12, []
    for _ in range(n):
        clen, isize, crc, status, built, _pad = struct.unpack_from("<IIIBBH", blob, at)
        at += 16
        out.append((blob[at:at + clen], isize, crc, status, built))
        at += clen
    assert at == len(blob)
    return out


if __name__ == "__main__":
    import sys
    sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "crispr-hawk_amd")]
    if "--write" in sys.argv:
        with open(GOLDEN, "wb") as f:
            f.write(golden_bytes())
    ms = unique_members()
    print(f"{len(panel())} cases, {len(ms)} distinct members, {sum(len(m.raw) for m in ms)} bytes, {sum(m.text is None for m in ms)} malformed")


# ---- the routes of readers._TextSource against each other (tests/test_bgzf_host.py, tests/test_gpu_bgzf.py)
def bgzf_file(path, text, block):
    from crisprhawk_hip import readers
    readers.write_bgzf(str(path), text, block=block)
    return str(path)


def member_offsets(fname):
    from crisprhawk_hip import readers
    src = readers._TextSource(fname, "zlib")
    return [int(x) for x in src._c_off], [int(x) for x in src._u_off]


def all_chunks(fname, route, chunk, verbosity=0):
    """[(offset, bytes)] of a whole pass with CHUNK = chunk, or the class of what the pass raised"""
    from crisprhawk_hip import readers
    src = readers._TextSource(fname, route, verbosity)
    assert src.kind == "bgzf" and src.inflate == route
    src.CHUNK = chunk
    try:
        return [(off, bytes(a)) for off, a in src.chunks()]
    except Exception as e:  # noqa: BLE001 - the routes must agree on it, whatever it is
        return type(e)


def seam_ranges(u_off, total):
    """byte ranges that start and end on member seams and one byte off them, inside one member and across several"""
    out = [(0, total), (0, 1), (total - 1, total), (5, 5), (7, 3)]
    seams = [u for u in u_off[1:-1] if 0 < u < total]
    for i in (0, len(seams) // 2, len(seams) - 1):
        s = seams[i]
        for lo in (s - 1, s, s + 1):
            for hi in (s, s + 1, seams[min(i + 2, len(seams) - 1)] - 1, seams[min(i + 2, len(seams) - 1)], seams[min(i + 3, len(seams) - 1)] + 1):
                out.append((max(lo, 0), min(hi, total)))
    return out


def assert_routes_agree(fname, route, chunk):
    from crisprhawk_hip import readers
    want = all_chunks(fname, "zlib", chunk)
    got = all_chunks(fname, route, chunk)
    assert isinstance(want, list) and isinstance(got, list)
    assert [o for o, _ in got] == [o for o, _ in want] and len(want) > 2
    assert got == want
    _, u_off = member_offsets(fname)
    a, b = readers._TextSource(fname, "zlib"), readers._TextSource(fname, route)
    for lo, hi in seam_ranges(u_off, u_off[-1]):
        assert bytes(b.read(lo, hi)) == bytes(a.read(lo, hi)), (lo, hi)
    return b
