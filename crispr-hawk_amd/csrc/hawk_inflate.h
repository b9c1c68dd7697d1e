// hawk_inflate.h - one BGZF member (a gzip member as bgzip writes it) -> its text, stated ONCE for the host
// (hawk_host_bgzf_inflate, hawk_hostutil.hip) and the device (k_bz_inflate, hawk_inflate.hip).  A raw-DEFLATE (RFC 1951) decoder.
//
// A member is in[0, clen): the whole gzip member, header and trailer included; its text goes to out[0, ulen).
//   header      magic 1f 8b, CM 8 (else HAWK_BZ_HEADER), FLG exactly 4 - FEXTRA alone, what bgzip writes (else
//               HAWK_BZ_UNSUPPORTED); XLEN bytes are skipped unread; the deflate stream ends 8 bytes before the member's end;
//               ISIZE must equal ulen and be at most 65536 (HAWK_BZ_SIZE)
//   blocks      any number; stored (LEN / ~LEN checked, the partial byte dropped), fixed and dynamic Huffman; type 3 is an error
//   acceptance  is zlib's inflate, which is what the Python route accepts: an over-subscribed code set is an error; an incomplete
//               one too, except a single code of length 1 in a literal/length or distance set (the code-length set must be
//               complete); no distance code at all is fine until a distance is asked for; HLIT > 286 and HDIST > 30 are errors;
//               no code for 256, code 16 with no length before it, a repeat that runs past HLIT + HDIST (a repeat may cross from
//               the literal/length lengths into the distance lengths), symbols 286 / 287, distance symbols 30 / 31, and a
//               distance that reaches back past the member's own first byte (no window from an earlier member) are errors.
//               Bytes behind the final block are ignored, as zlib.decompress ignores them.
//   CRC32       is NOT checked: the Python route drops the trailer unread (raw[12 + xlen:-8]), so nothing changes.
//
// Memory safety is part of the rules, the input being file content: the bit reader never reads outside in[0, clen) and reports
// HAWK_BZ_INPUT when it runs dry; a token is refused (HAWK_BZ_SIZE) before the first byte that would not fit out[0, ulen); a
// distance is checked against the bytes produced before the copy; every loop consumes input or ends.  A member ends in a status.
//
// The same code runs as one host thread and as one wavefront.  `X` says which: X::lanes lanes run every function together with
// EQUAL values in every variable that is not derived from X::lane() - the bit reader's state and every branch are uniform - and
// split only the loops written `for (i = X::lane(); i < n; i += X::lanes)`.  X::ballot / X::lt_mask count across the lanes,
// X::sync orders the lanes' memory accesses (tables, token batch and text are written by some lanes and read by others),
// X::uni marks a value every lane holds alike.  BzHost below is the one-lane case; the wave's is in hawk_inflate.hip.
#pragma once
#include <stdint.h>

#include "../../include/hawk.h"

#if defined(__HIPCC__)
#define HAWK_HD __host__ __device__
#else
#define HAWK_HD
#endif
#if defined(__clang__)
#define BZ_UNROLL _Pragma("unroll")
#else
#define BZ_UNROLL
#endif
#define BZ_INLINE HAWK_HD __attribute__((always_inline)) inline

#define BZ_MAX_TEXT 65536u
#define BZ_BATCH 64u       // tokens decoded before the lanes write them out
#define BZ_FAST_LIT 9u     // bits of the direct lookup in front of the canonical walk
#define BZ_FAST_DIST 8u
#define BZ_FAST_CODES 7u   // the code-length code (its table borrows fast_dist / sym_dist / cnt_dist)

enum { BZ_KIND_CODES = 0, BZ_KIND_LIT = 1, BZ_KIND_DIST = 2 };

// What a decoder works in: the wave's slice of LDS, a host thread's stack.  2944 bytes.
struct BzTables {
  uint16_t fast_lit[1u << BZ_FAST_LIT];    // the next BZ_FAST_* bits -> symbol << 4 | length, 0: take the walk
  uint16_t fast_dist[1u << BZ_FAST_DIST];
  uint16_t sym_lit[288];                   // symbols sorted by (length, symbol)
  uint16_t sym_dist[32];
  uint16_t cnt_lit[16], cnt_dist[16];      // codes per length
  uint32_t tok[BZ_BATCH];                  // distance | length << 16, or 0 | literal << 16
  uint16_t tok_pos[BZ_BATCH];              // where the token's first byte goes
  uint8_t lens[320];                       // code lengths as the block's header gives them
};

struct BzHost {
  static constexpr uint32_t lanes = 1;
  static uint32_t lane() { return 0; }
  static uint64_t ballot(bool p) { return p ? 1u : 0u; }
  static uint64_t lt_mask() { return 0; }
  static void sync() {}
  static uint32_t uni(uint32_t v) { return v; }
};

struct BzBits {
  const uint8_t* in;
  uint32_t pos, end;  // next byte, end of the deflate stream
  uint64_t buf;       // bits not yet used, the next one lowest; zero above cnt
  uint32_t cnt;
};

#define BZ_TRY(expr)              \
  do {                            \
    const uint32_t s_ = (expr);   \
    if (s_) return s_;            \
  } while (0)

BZ_INLINE uint32_t bz_popc(uint64_t m) { return (uint32_t)__builtin_popcountll(m); }

// at least 57 bits unless the stream ends first: one refill serves a whole token (15 + 5 + 15 + 13 bits)
template <class X>
BZ_INLINE void bz_refill(BzBits& b) {
  while (b.cnt <= 56 && b.pos < b.end) {
    b.buf |= (uint64_t)X::uni(b.in[b.pos]) << b.cnt;
    ++b.pos;
    b.cnt += 8;
  }
}
BZ_INLINE uint32_t bz_bits(BzBits& b, uint32_t n, uint32_t* v) {  // n <= 16
  if (b.cnt < n) return HAWK_BZ_INPUT;
  *v = (uint32_t)(b.buf & ((1u << n) - 1u));
  b.buf >>= n;
  b.cnt -= n;
  return HAWK_BZ_OK;
}

BZ_INLINE uint32_t bz_bitrev(uint32_t code, uint32_t len) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
  return r;
}

BZ_INLINE uint32_t bz_codelen_order(uint32_t i) {  // RFC 1951 3.2.7
  switch (i) {
    case 0: return 16; case 1: return 17; case 2: return 18; case 3: return 0; case 4: return 8; case 5: return 7; case 6: return 9;
    case 7: return 6; case 8: return 10; case 9: return 5; case 10: return 11; case 11: return 4; case 12: return 12; case 13: return 3;
    case 14: return 13; case 15: return 2; case 16: return 14; case 17: return 1; default: return 15;
  }
}
// length symbol 257 + s, s < 29 / distance symbol d, d < 30: base and extra bits
BZ_INLINE void bz_len_base(uint32_t s, uint32_t* base, uint32_t* extra) {
  if (s < 8) { *base = 3 + s; *extra = 0; }
  else if (s < 28) { *extra = (s >> 2) - 1; *base = 3 + ((4 + (s & 3)) << *extra); }
  else { *base = 258; *extra = 0; }
}
BZ_INLINE void bz_dist_base(uint32_t d, uint32_t* base, uint32_t* extra) {
  if (d < 4) { *base = 1 + d; *extra = 0; }
  else { *extra = (d >> 1) - 1; *base = 1 + ((2 + (d & 1)) << *extra); }
}

// The canonical code of lens[0, n): counts per length into cnt[16], the symbols sorted by (length, symbol) into sym[], the codes
// of up to fast_bits bits into fast[1 << fast_bits].  The lanes take the symbols X::lanes at a time: a ballot per length counts
// them and ranks each lane's symbol among its equals.
template <class X>
BZ_INLINE uint32_t bz_build(const uint8_t* lens, uint32_t n, uint16_t* fast, uint32_t fast_bits, uint16_t* sym, uint16_t* cnt, int kind) {
  const uint32_t lane = X::lane();
  uint32_t c[16];
BZ_UNROLL
  for (uint32_t l = 0; l < 16; ++l) c[l] = 0;
  for (uint32_t base = 0; base < n; base += X::lanes) {
    const uint32_t s = base + lane, L = s < n ? lens[s] : 0u;
BZ_UNROLL
    for (uint32_t l = 1; l < 16; ++l) c[l] += bz_popc(X::ballot(L == l));
  }
  int32_t left = 1;
  uint32_t total = 0;
BZ_UNROLL
  for (uint32_t l = 1; l < 16; ++l) {
    left = (left << 1) - (int32_t)c[l];
    if (left < 0) return HAWK_BZ_CODE;  // over-subscribed
    total += c[l];
  }
  if (left > 0) {  // incomplete: zlib lets one code of length 1 pass, and a set without any code - but not for the code lengths
    const bool lone = total == 1 && c[1] == 1;
    if (kind == BZ_KIND_CODES || !(lone || total == 0)) return HAWK_BZ_CODE;
  }
  uint32_t first[16], offs[16], run[16];
  {
    uint32_t code = 0, idx = 0;
    first[0] = offs[0] = run[0] = 0;
BZ_UNROLL
    for (uint32_t l = 1; l < 16; ++l) {
      code = (code + c[l - 1]) << 1;
      first[l] = code; offs[l] = idx; run[l] = 0;
      idx += c[l];
    }
  }
  for (uint32_t i = lane; i < (1u << fast_bits); i += X::lanes) fast[i] = 0;
  if (lane == 0) {
BZ_UNROLL
    for (uint32_t l = 0; l < 16; ++l) cnt[l] = (uint16_t)c[l];
  }
  X::sync();
  for (uint32_t base = 0; base < n; base += X::lanes) {
    const uint32_t s = base + lane, L = s < n ? lens[s] : 0u;
    uint32_t at = 0, code = 0;
BZ_UNROLL
    for (uint32_t l = 1; l < 16; ++l) {
      const uint64_t m = X::ballot(L == l);
      if (L == l) {
        const uint32_t r = run[l] + bz_popc(m & X::lt_mask());
        at = offs[l] + r;
        code = first[l] + r;
      }
      run[l] += bz_popc(m);
    }
    if (L) {
      sym[at] = (uint16_t)s;  // at < total <= n
      if (L <= fast_bits) {
        const uint16_t e = (uint16_t)(s << 4 | L);
        for (uint32_t k = bz_bitrev(code, L); k < (1u << fast_bits); k += 1u << L) fast[k] = e;
      }
    }
  }
  X::sync();
  return HAWK_BZ_OK;
}

// One symbol: the direct lookup, else the walk over the lengths (count / first code / sorted symbols).  The buffer is zero above
// cnt, so a lookup that used bits the stream does not have shows as a length above cnt.
template <class X>
BZ_INLINE uint32_t bz_symbol(BzBits& b, const uint16_t* fast, uint32_t fast_bits, const uint16_t* sym, const uint16_t* cnt, uint32_t* out) {
  const uint32_t e = X::uni(fast[b.buf & ((1u << fast_bits) - 1u)]);
  if (e) {
    const uint32_t L = e & 15u;
    if (L > b.cnt) return HAWK_BZ_INPUT;
    b.buf >>= L;
    b.cnt -= L;
    *out = e >> 4;
    return HAWK_BZ_OK;
  }
  uint32_t code = 0, first = 0, index = 0;
  for (uint32_t l = 1; l < 16; ++l) {
    if (l > b.cnt) return HAWK_BZ_INPUT;
    code |= (uint32_t)(b.buf >> (l - 1)) & 1u;
    const uint32_t count = X::uni(cnt[l]);
    if (code < first + count) {  // code >= first always
      b.buf >>= l;
      b.cnt -= l;
      *out = X::uni(sym[index + (code - first)]);
      return HAWK_BZ_OK;
    }
    index += count;
    first = (first + count) << 1;
    code <<= 1;
  }
  return HAWK_BZ_CODE;  // a code an incomplete set does not hold
}

// The batch goes out.  First, each lane takes a token: a literal is stored, and so is a match whose source lies wholly in front of
// the batch - it reads nothing this batch writes, whatever the other lanes do meanwhile (in text most matches reach back a line or
// more, further than the few hundred bytes a batch covers).  Then the remaining matches, in token order, each copied by all lanes:
// such a match may read what an earlier token of the batch wrote.  Either way byte i of a match comes from out[p - dist + i % dist].
BZ_INLINE bool bz_source_before(uint32_t p, uint32_t dist, uint32_t len, uint32_t start) {
  return p - dist + (len < dist ? len : dist) <= start;  // dist <= p
}
template <class X>
BZ_INLINE void bz_flush(BzTables* T, uint8_t* out, uint32_t n) {
  X::sync();
  const uint32_t start = n ? X::uni(T->tok_pos[0]) : 0u;
  for (uint32_t t = X::lane(); t < n; t += X::lanes) {
    const uint32_t v = T->tok[t], dist = v & 0xffffu, len = v >> 16, p = T->tok_pos[t];
    if (!dist) {
      out[p] = (uint8_t)len;
    } else if (bz_source_before(p, dist, len, start)) {
      const uint8_t* src = out + (p - dist);
      for (uint32_t i = 0; i < len; ++i) out[p + i] = src[dist >= len ? i : i % dist];
    }
  }
  X::sync();
  for (uint32_t t = 0; t < n; ++t) {
    const uint32_t v = X::uni(T->tok[t]), dist = v & 0xffffu, len = v >> 16, p = X::uni(T->tok_pos[t]);
    if (!dist || bz_source_before(p, dist, len, start)) continue;
    const uint8_t* src = out + (p - dist);
    for (uint32_t i = X::lane(); i < len; i += X::lanes) out[p + i] = src[dist >= len ? i : i % dist];
    X::sync();
  }
  X::sync();
}

struct BzOut {
  uint8_t* out;
  uint32_t ulen, produced, ntok;
};
// a token enters the batch only if its bytes fit and its source exists
template <class X>
BZ_INLINE uint32_t bz_token(BzTables* T, BzOut& o, uint32_t dist, uint32_t len_or_byte) {
  const uint32_t len = dist ? len_or_byte : 1u;
  if (dist > o.produced) return HAWK_BZ_DISTANCE;
  if (len > o.ulen - o.produced) return HAWK_BZ_SIZE;
  if (X::lane() == 0) {
    T->tok[o.ntok] = dist | len_or_byte << 16;
    T->tok_pos[o.ntok] = (uint16_t)o.produced;
  }
  o.produced += len;
  if (++o.ntok == BZ_BATCH) {
    bz_flush<X>(T, o.out, o.ntok);
    o.ntok = 0;
  }
  return HAWK_BZ_OK;
}

// the header of a dynamic block: the code-length code, then HLIT + HDIST lengths into T->lens
template <class X>
BZ_INLINE uint32_t bz_dynamic_lens(BzBits& b, BzTables* T, uint32_t* n_lit, uint32_t* n_dist) {
  const uint32_t lane = X::lane();
  uint32_t hlit, hdist, hclen, v;
  bz_refill<X>(b);
  BZ_TRY(bz_bits(b, 5, &hlit));
  BZ_TRY(bz_bits(b, 5, &hdist));
  BZ_TRY(bz_bits(b, 4, &hclen));
  hlit += 257; hdist += 1; hclen += 4;
  if (hlit > 286 || hdist > 30) return HAWK_BZ_CODE;
  for (uint32_t i = lane; i < 19; i += X::lanes) T->lens[i] = 0;
  X::sync();
  for (uint32_t i = 0; i < hclen; ++i) {
    bz_refill<X>(b);
    BZ_TRY(bz_bits(b, 3, &v));
    if (lane == 0) T->lens[bz_codelen_order(i)] = (uint8_t)v;
  }
  X::sync();
  BZ_TRY(bz_build<X>(T->lens, 19, T->fast_dist, BZ_FAST_CODES, T->sym_dist, T->cnt_dist, BZ_KIND_CODES));
  const uint32_t total = hlit + hdist;
  uint32_t have = 0, prev = 0;
  while (have < total) {
    uint32_t s;
    bz_refill<X>(b);
    BZ_TRY(bz_symbol<X>(b, T->fast_dist, BZ_FAST_CODES, T->sym_dist, T->cnt_dist, &s));
    if (s < 16) {
      if (lane == 0) T->lens[have] = (uint8_t)s;
      ++have;
      prev = s;
      continue;
    }
    uint32_t rep, val = 0;
    if (s == 16) {
      if (!have) return HAWK_BZ_CODE;
      BZ_TRY(bz_bits(b, 2, &rep));
      rep += 3;
      val = prev;
    } else if (s == 17) {
      BZ_TRY(bz_bits(b, 3, &rep));
      rep += 3;
    } else {
      BZ_TRY(bz_bits(b, 7, &rep));
      rep += 11;
    }
    if (rep > total - have) return HAWK_BZ_CODE;
    for (uint32_t i = lane; i < rep; i += X::lanes) T->lens[have + i] = (uint8_t)val;  // have + rep <= 316 < 320
    have += rep;
    prev = val;
  }
  X::sync();
  if (X::uni(T->lens[256]) == 0) return HAWK_BZ_CODE;  // no end of block
  *n_lit = hlit;
  *n_dist = hdist;
  return HAWK_BZ_OK;
}

// the fixed code as lengths: 288 literal/length symbols (286 and 287 are never valid), 32 distance symbols (30 and 31 likewise)
template <class X>
BZ_INLINE void bz_fixed_lens(BzTables* T) {
  for (uint32_t i = X::lane(); i < 320; i += X::lanes) T->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
  X::sync();
}
// both tables of a block from T->lens: n_lit literal/length lengths, then n_dist distance lengths
template <class X>
BZ_INLINE uint32_t bz_block_tables(BzTables* T, uint32_t n_lit, uint32_t n_dist) {
  for (int kind = BZ_KIND_LIT; kind <= BZ_KIND_DIST; ++kind) {
    const bool lit = kind == BZ_KIND_LIT;
    BZ_TRY(bz_build<X>(lit ? T->lens : T->lens + n_lit, lit ? n_lit : n_dist, lit ? T->fast_lit : T->fast_dist, lit ? BZ_FAST_LIT : BZ_FAST_DIST,
                       lit ? T->sym_lit : T->sym_dist, lit ? T->cnt_lit : T->cnt_dist, kind));
  }
  return HAWK_BZ_OK;
}

// the tokens of a Huffman block, up to its end-of-block symbol
template <class X>
BZ_INLINE uint32_t bz_huffman_block(BzBits& b, BzTables* T, BzOut& o) {
  for (;;) {
    uint32_t s, base, extra, v, dist = 0;
    bz_refill<X>(b);
    BZ_TRY(bz_symbol<X>(b, T->fast_lit, BZ_FAST_LIT, T->sym_lit, T->cnt_lit, &s));
    if (s == 256) return HAWK_BZ_OK;
    if (s > 256) {
      s -= 257;
      if (s >= 29) return HAWK_BZ_SYMBOL;
      bz_len_base(s, &base, &extra);
      BZ_TRY(bz_bits(b, extra, &v));
      s = base + v;  // the length
      uint32_t d;
      BZ_TRY(bz_symbol<X>(b, T->fast_dist, BZ_FAST_DIST, T->sym_dist, T->cnt_dist, &d));
      if (d >= 30) return HAWK_BZ_SYMBOL;
      bz_dist_base(d, &base, &extra);
      BZ_TRY(bz_bits(b, extra, &v));
      dist = base + v;
    }
    BZ_TRY(bz_token<X>(T, o, dist, s));
  }
}

template <class X>
BZ_INLINE uint32_t bz_stored_block(BzBits& b, BzTables* T, BzOut& o) {
  uint32_t len, nlen;
  b.buf >>= b.cnt & 7u;
  b.cnt &= ~7u;
  bz_refill<X>(b);
  BZ_TRY(bz_bits(b, 16, &len));
  BZ_TRY(bz_bits(b, 16, &nlen));
  if ((len ^ 0xffffu) != nlen) return HAWK_BZ_BLOCK;
  b.pos -= b.cnt >> 3;  // whole bytes go back: the block's bytes are copied where they lie
  b.buf = 0;
  b.cnt = 0;
  if (len > b.end - b.pos) return HAWK_BZ_INPUT;
  if (len > o.ulen - o.produced) return HAWK_BZ_SIZE;
  bz_flush<X>(T, o.out, o.ntok);
  o.ntok = 0;
  for (uint32_t i = X::lane(); i < len; i += X::lanes) o.out[o.produced + i] = b.in[b.pos + i];
  X::sync();
  b.pos += len;
  o.produced += len;
  return HAWK_BZ_OK;
}

// The member in[0, clen) -> out[0, ulen).  A HAWK_BZ_* status; on any but HAWK_BZ_OK the bytes of out[0, ulen) are unspecified.
template <class X>
BZ_INLINE uint32_t bz_inflate_member(const uint8_t* in, uint64_t clen, uint8_t* out, uint64_t ulen, BzTables* T) {
  if (clen < 20 || clen > 0xffffffffull) return HAWK_BZ_INPUT;
  if (X::uni(in[0]) != 0x1f || X::uni(in[1]) != 0x8b || X::uni(in[2]) != 8) return HAWK_BZ_HEADER;
  if (X::uni(in[3]) != 4) return HAWK_BZ_UNSUPPORTED;
  const uint32_t n = (uint32_t)clen, xlen = X::uni(in[10]) | X::uni(in[11]) << 8;
  if (xlen > n - 20) return HAWK_BZ_INPUT;
  const uint32_t isize = X::uni(in[n - 4]) | X::uni(in[n - 3]) << 8 | X::uni(in[n - 2]) << 16 | X::uni(in[n - 1]) << 24;
  if (ulen > BZ_MAX_TEXT || isize != ulen) return HAWK_BZ_SIZE;
  BzBits b = {in, 12 + xlen, n - 8, 0, 0};
  BzOut o = {out, isize, 0, 0};
  bool fixed_stand = false;  // the tables of the fixed code stand: a run of fixed blocks builds them once
  uint32_t last;
  do {
    uint32_t type;
    bz_refill<X>(b);
    BZ_TRY(bz_bits(b, 1, &last));
    BZ_TRY(bz_bits(b, 2, &type));
    if (type == 0) {
      BZ_TRY(bz_stored_block<X>(b, T, o));
    } else if (type == 3) {
      return HAWK_BZ_BLOCK;
    } else {
      uint32_t n_lit = 288, n_dist = 32;
      const bool stand = type == 1 && fixed_stand;
      if (type == 2) BZ_TRY(bz_dynamic_lens<X>(b, T, &n_lit, &n_dist));
      else if (!stand) bz_fixed_lens<X>(T);
      if (!stand) BZ_TRY(bz_block_tables<X>(T, n_lit, n_dist));
      fixed_stand = type == 1;
      BZ_TRY(bz_huffman_block<X>(b, T, o));
    }
  } while (!last);
  bz_flush<X>(T, o.out, o.ntok);
  return o.produced == isize ? (uint32_t)HAWK_BZ_OK : (uint32_t)HAWK_BZ_SIZE;
}

// Host only: what both entry points check before a member is looked at: both offset arrays ascend, the members lie inside `in`
inline bool bz_args_ok(const uint8_t* in, uint64_t in_bytes, const uint64_t* c_off, const uint64_t* u_off, uint32_t n_members, const uint8_t* out,
                       const uint8_t* status) {
  if (!n_members) return true;
  if (!c_off || !u_off || !status) return false;
  for (uint32_t k = 0; k < n_members; ++k)
    if (c_off[k + 1] < c_off[k] || u_off[k + 1] < u_off[k]) return false;
  if (c_off[n_members] > in_bytes || (c_off[n_members] > c_off[0] && !in)) return false;
  if (u_off[n_members] > u_off[0] && !out) return false;
  return true;
}
