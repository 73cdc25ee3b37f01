// lzf_encode_core.h — LZF chunk WRITER (liblzf blocks inside compress-lzf's chunk framing), written once for the device and
// for the host.
//
// Map side of S3S_CODEC_LZF (S3S_OPT_LZF_COMPRESS, key 10).  Not compress-lzf's output and not the oracle encoder's: a
// decode-compatible stream.  A segment is cut into chunks of at most kChunk source bytes; every chunk is
// compressed with no history before its own first byte, so every chunk is independent work:
//   compressed chunk  'Z' 'V' 1 | clen u16 BE | ulen u16 BE | block        when the block is at least two bytes shorter
//   stored chunk      'Z' 'V' 0 | n u16 BE | bytes                         otherwise (c >= n - 2)
//   block             ctrl 0..31: a run of ctrl + 1 literals follows
//                     else a reference: len - 2 in the top three bits (7: + next byte), offset - 1 in 13 bits; 3 .. 264 bytes
//                     from 1 .. 8192 back.  Longer matches are several references, none shorter than 3 bytes.
//
// The parse examines kStep positions per step (one wavefront on the device): every position looks its 3-byte hash up in a
// table of u16 positions AS IT WAS BEFORE THE STEP; a 16-bit table has no "empty" value, so every hit is verified (three
// bytes, 0 < distance <= 8192).  Among the hits within kLazy positions behind the first one the largest gain (hit measure,
// capped at kProbe bytes, minus the literals it skips) starts the match; the match extends forwards without limit and
// backwards (at most kStep bytes) into the pending literals.  Positions up to the match start enter the table, the latest
// position of a slot wins.  Where a byte lands is a closed form of the run / match lengths (lit_cost, match_cost), so the
// device writes literals and references one lane each.
//
// Compiled by hipcc (S3S_LZF_DEVICE: lzf_compress.hip, the wave-wide statement of the step) and by g++
// (tests/model/lzf_encode_model.cpp: compress_block below is the same step on one thread).  Both give the same bytes.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef S3S_LZF_DEVICE
#define LE_HD __device__ inline
#else
#define LE_HD static inline
#endif

namespace s3s_lzf_enc {

constexpr int kChunk = 65535;     // source bytes of a chunk (both header lengths are u16)
constexpr int kMaxOff = 1 << 13;  // farthest reference
constexpr int kMaxRef = 264;      // longest reference: 2 + 7 + 255
constexpr int kMaxLit = 32;       // longest literal run under one control byte
constexpr int kHashLog = 13;      // 8192 x u16 positions: 16 KiB of LDS per wavefront
constexpr int kStep = 64;         // positions examined per step (one wavefront)
constexpr int kLazy = 8;          // the match starts within this many positions behind the step's first hit
constexpr int kProbe = 35;        // cap of the hit measure that ranks the candidates
constexpr int kHeaderStored = 5, kHeaderCompressed = 7;

// the largest block the parse can write for n source bytes: literal runs cost one control byte per 32, a run that a match
// cuts short costs one more, and every match is at least one byte shorter than what it copies
LE_HD uint32_t block_bound(uint32_t n) { return n + n / kMaxLit + 4; }
// s3s_max_compressed_size's figure for one segment: every chunk with the header of a compressed one
LE_HD int64_t stream_bound(int64_t ulen) { return ulen <= 0 ? 0 : ulen + kHeaderCompressed * ((ulen + kChunk - 1) / kChunk); }

LE_HD uint32_t rd32(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}
LE_HD uint32_t hash3(const uint8_t* p) {
  const uint32_t v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
  return (v * 2654435761u) >> (32 - kHashLog);
}

// the hit measure of position p (p + 3 <= n) against table entry c: 0 = no hit, else 3 .. kProbe equal bytes
LE_HD int probe(const uint8_t* s, uint32_t n, uint32_t p, uint32_t c) {
  if (c >= p || p - c > (uint32_t)kMaxOff) return 0;
  if (s[c] != s[p] || s[c + 1] != s[p + 1] || s[c + 2] != s[p + 2]) return 0;
  const int lim = n - p < (uint32_t)kProbe ? (int)(n - p) : kProbe;
  int len = 3;
  while (len + 4 <= lim) {
    const uint32_t x = rd32(s + c + len) ^ rd32(s + p + len);
    if (x) return len + (__builtin_ctz(x) >> 3);
    len += 4;
  }
  while (len < lim && s[c + len] == s[p + len]) len++;
  return len;
}

// the rank of a candidate: the largest gain wins, the earliest position among equals (0 = not a candidate)
LE_HD int gain_key(int len, int lane, int k0) {
  if (len <= 0 || lane < k0 || lane >= k0 + kLazy) return 0;
  const int gain = len - (lane - k0);
  return gain > 0 ? gain * kStep + (kStep - 1 - lane) : 0;
}

// ---- where the bytes land --------------------------------------------------------------------------------------------
// a run of ll literals: a control byte in front of every 32
LE_HD uint32_t lit_cost(uint32_t ll) { return ll + (ll + kMaxLit - 1) / kMaxLit; }
LE_HD void put_literal(uint8_t* out, const uint8_t* lit, uint32_t ll, uint32_t i) {
  const uint32_t g = i / kMaxLit;
  if (i % kMaxLit == 0) out[g * (kMaxLit + 1)] = (uint8_t)((ll - i < (uint32_t)kMaxLit ? ll - i : (uint32_t)kMaxLit) - 1);
  out[1 + i + g] = lit[i];
}
// a match of ml >= 3 bytes: references of 264 bytes, then the rest; a rest of 1 or 2 takes 2 or 1 bytes from the piece before
LE_HD uint32_t match_pieces(uint32_t ml) { return (ml + kMaxRef - 1) / kMaxRef; }
LE_HD uint32_t piece_len(uint32_t ml, uint32_t j) {
  const uint32_t np = match_pieces(ml), r = ml - (np - 1) * kMaxRef;  // r = 1 .. 264
  if (j + 1 == np) return r < 3 ? 3 : r;
  if (j + 2 == np && r < 3) return kMaxRef - (3 - r);
  return kMaxRef;
}
LE_HD uint32_t piece_bytes(uint32_t len) { return len <= 8 ? 2 : 3; }
LE_HD uint32_t match_cost(uint32_t ml) {
  const uint32_t np = match_pieces(ml);
  return 3 * (np - 1) + piece_bytes(piece_len(ml, np - 1));  // every piece but the last is 261 bytes or longer
}
LE_HD void put_piece(uint8_t* out, uint32_t ml, uint32_t off, uint32_t j) {
  const uint32_t len = piece_len(ml, j) - 2, o = off - 1;
  uint8_t* d = out + 3 * j;
  if (len < 7) {
    d[0] = (uint8_t)(len << 5 | o >> 8);
    d[1] = (uint8_t)o;
  } else {
    d[0] = (uint8_t)(7u << 5 | o >> 8);
    d[1] = (uint8_t)(len - 7);
    d[2] = (uint8_t)o;
  }
}

// the chunk header, right-aligned in front of the payload: -> bytes of header + payload in the image, stored or not
LE_HD bool chunk_stored(uint32_t n, uint32_t c) { return c + 2 >= n; }
LE_HD uint32_t put_chunk_header(uint8_t* payload, uint32_t n, uint32_t c) {
  if (chunk_stored(n, c)) {
    uint8_t* h = payload - kHeaderStored;
    h[0] = 'Z', h[1] = 'V', h[2] = 0, h[3] = (uint8_t)(n >> 8), h[4] = (uint8_t)n;
    return kHeaderStored + n;
  }
  uint8_t* h = payload - kHeaderCompressed;
  h[0] = 'Z', h[1] = 'V', h[2] = 1, h[3] = (uint8_t)(c >> 8), h[4] = (uint8_t)c, h[5] = (uint8_t)(n >> 8), h[6] = (uint8_t)n;
  return kHeaderCompressed + c;
}

#ifndef S3S_LZF_DEVICE
// The step parse on one thread: s[0, n) (n <= kChunk) -> out[0, block_bound(n)), returns the block's bytes.  tab: 1 << kHashLog
// entries.  Statement by statement what parse_wave (lzf_compress.hip) does with 64 lanes.
static inline uint32_t compress_block(const uint8_t* s, uint32_t n, uint16_t* tab, uint8_t* out) {
  memset(tab, 0, sizeof(uint16_t) << kHashLog);
  uint32_t ip = 0, anchor = 0, op = 0;
  while (ip + 3 <= n) {
    uint32_t h[kStep], c[kStep];
    int len[kStep];
    const int nact = n - 2 - ip < (uint32_t)kStep ? (int)(n - 2 - ip) : kStep;
    int k0 = -1;
    for (int l = 0; l < nact; l++) {  // every lane reads the table before any lane writes it
      h[l] = hash3(s + ip + l);
      c[l] = tab[h[l]];
      len[l] = probe(s, n, ip + (uint32_t)l, c[l]);
      if (len[l] > 0 && k0 < 0) k0 = l;
    }
    int k = -1;
    if (k0 >= 0) {
      int key = 0;
      for (int l = k0; l < nact && l < k0 + kLazy; l++) {
        const int q = gain_key(len[l], l, k0);
        key = q > key ? q : key;
      }
      k = kStep - 1 - (key & (kStep - 1));
    }
    for (int l = 0; l < nact && (k < 0 || l <= k); l++) tab[h[l]] = (uint16_t)(ip + (uint32_t)l);  // the latest position wins
    if (k < 0) {
      ip += kStep;
      continue;
    }
    uint32_t m = ip + (uint32_t)k, cc = c[k], ml = 3;
    while (m + ml < n && s[m + ml] == s[cc + ml]) ml++;
    for (int back = 0; back < kStep && m > anchor && cc > 0 && s[m - 1] == s[cc - 1]; back++) m--, cc--, ml++;
    const uint32_t ll = m - anchor;
    for (uint32_t i = 0; i < ll; i++) put_literal(out + op, s + anchor, ll, i);
    op += lit_cost(ll);
    for (uint32_t j = 0; j < match_pieces(ml); j++) put_piece(out + op, ml, m - cc, j);
    op += match_cost(ml);
    anchor = ip = m + ml;
  }
  const uint32_t ll = n - anchor;
  for (uint32_t i = 0; i < ll; i++) put_literal(out + op, s + anchor, ll, i);
  return op + lit_cost(ll);
}
#endif

}  // namespace s3s_lzf_enc
