// zstd_encode_core.h — Zstandard block WRITER (RFC 8878), written once for the device and for the host.
//
// Map side of S3S_CODEC_ZSTD (S3S_OPT_ZSTD_COMPRESS, ABI 11).  Not libzstd's output: a decode-compatible stream — any frame
// libzstd's decoder accepts and decodes to the partition's bytes is a valid map output.  One frame per
// non-empty segment, blocks of at most kBlock bytes, every block compressed with no history before its own first byte, every
// offset written as Offset_Value = offset + 3 (no repeat codes, so no frame state crosses a block), predefined LL / OF / ML
// tables, literals Raw / RLE / Huffman (code lengths <= 11, direct or FSE-compressed weights, 1 or 4 streams).
//
// The stages behind the parse take ARBITRARY sequence arrays (packed by seq_pack) and the literal bytes:
//   huf_build       histogram -> length-limited code, weights, the smaller of the two weight descriptions
//   lit_plan        Raw / RLE / Huffman, size format, stream offsets; writes the section's header (+ description, jump table)
//   huf_encode_stream   one of the 1 or 4 streams (independent: one lane each on the device)
//   seq_encode      sequence count, mode byte, the FSE bit stream (serial per block: one lane)
// Compiled by hipcc (S3S_ZSTD_DEVICE: zstd_compress.hip spreads the histogram, the bit sums, the streams and the parse over a
// workgroup) and by g++ (tests/model/zstd_encode_model.cpp: the same code on one thread, checked against libzstd's decoder on
// the CPU, under ASan with exact-size buffers, before it ever reaches a GPU).  parse_block below is the host statement of
// the device's 64-positions-per-step parse: both produce the same sequences, so the GPU's frames equal the model's.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef S3S_ZSTD_DEVICE
#define ZE_HD __device__ inline
#else
#define ZE_HD static inline
#endif

namespace s3s_zstd_enc {

constexpr int kBlock = 1 << 17;        // Block_Maximum_Size; also the window the frame header declares
constexpr int kFrameHeader = 14;       // magic | FHD (8-byte Frame_Content_Size) | window descriptor | FCS
constexpr int kHufMaxBits = 11;
constexpr int kHashLog = 13;           // 8192 x u32 positions
constexpr int kMinMatch = 4;
constexpr int kLazy = 8, kProbe = 32; // see parse_block
constexpr int kStep = 64;              // positions the parse examines per step (one wavefront)
constexpr int kMaxSeq = kBlock / kMinMatch;
constexpr int kSeqLog = 6, kOfLog = 5, kWtLog = 6;  // accuracy logs: predefined LL / ML, predefined OF, Huffman weights

// a sequence: literal length (<= 2^17) | match length << 18 | offset << 36
ZE_HD uint64_t seq_pack(uint32_t ll, uint32_t ml, uint32_t off) { return (uint64_t)ll | (uint64_t)ml << 18 | (uint64_t)off << 36; }
ZE_HD uint32_t seq_ll(uint64_t s) { return (uint32_t)s & 0x3ffffu; }
ZE_HD uint32_t seq_ml(uint64_t s) { return (uint32_t)(s >> 18) & 0x3ffffu; }
ZE_HD uint32_t seq_off(uint64_t s) { return (uint32_t)(s >> 36); }

ZE_HD int highbit(uint32_t x) { return 31 - __builtin_clz(x); }
ZE_HD uint32_t rd32(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}
ZE_HD uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - kHashLog); }

// ---- bits: fields are added from bit 0 up, bytes leave in ascending order (the reader of a "backward" stream starts at the end)
struct BitW {
  uint8_t* p;
  uint8_t* end;
  uint64_t acc;
  int nb, ovf;
};
ZE_HD void bw_init(BitW& w, uint8_t* p, uint8_t* end) {
  w.p = p;
  w.end = end;
  w.acc = 0;
  w.nb = w.ovf = 0;
}
ZE_HD void bw_add(BitW& w, uint32_t v, int n) {  // n <= 31; at most 57 bits between two flushes
  w.acc |= (uint64_t)(v & ((1u << n) - 1u)) << w.nb;
  w.nb += n;
}
ZE_HD void bw_flush(BitW& w) {
  const int nbytes = w.nb >> 3;
  if (w.end - w.p < nbytes) {
    w.ovf = 1;
  } else {
    for (int i = 0; i < nbytes; i++) w.p[i] = (uint8_t)(w.acc >> (8 * i));
    w.p += nbytes;
  }
  w.acc = nbytes >= 8 ? 0 : w.acc >> (8 * nbytes);
  w.nb &= 7;
}
ZE_HD void bw_close(BitW& w, bool marker) {  // marker: the closing 1-bit of a stream that is read backwards
  if (marker) bw_add(w, 1, 1);
  bw_flush(w);
  if (w.nb > 0) {
    if (w.p >= w.end) w.ovf = 1;
    else *w.p++ = (uint8_t)w.acc;
    w.nb = 0;
    w.acc = 0;
  }
}

// ---- FSE encoding table of one normalised distribution (accuracy log <= 6, at most 53 symbols)
struct FseCT {
  uint16_t state[64];
  int32_t dfs[56];   // deltaFindState
  uint32_t dnb[56];  // deltaNbBits
  int32_t log;
};

struct Work {
  FseCT ll, of, ml, wt;
  uint8_t tsym[64];
  uint16_t cumul[64];
  uint32_t hist[256];   // of the block's literals
  uint32_t cnt[256];    // the counts the tree is built from (halved until it is at most kHufMaxBits deep)
  uint8_t order[256];   // present symbols, ascending by count
  uint32_t nodew[512];  // tree: node weights, then node depths
  uint16_t parent[512];
  uint8_t nbits[256];
  uint16_t code[256];
  uint8_t weights[256];
  uint8_t wdesc[136];   // header byte + weight description
  int32_t wdesc_len;    // 0: the code has no description (Huffman cannot be used)
  int32_t maxbits, maxsym, nsym;
  uint32_t sbits[4];    // code bits of the four quarters of the literals
};

ZE_HD void fse_build(FseCT& t, const int16_t* norm, int nsym, int log, uint8_t* tsym, uint16_t* cumul) {
  const int size = 1 << log, mask = size - 1, step = (size >> 1) + (size >> 3) + 3;
  int high = size - 1;
  cumul[0] = 0;
  for (int s = 0; s < nsym; s++) {
    if (norm[s] == -1) {
      cumul[s + 1] = (uint16_t)(cumul[s] + 1);
      tsym[high--] = (uint8_t)s;
    } else {
      cumul[s + 1] = (uint16_t)(cumul[s] + norm[s]);
    }
  }
  int pos = 0;
  for (int s = 0; s < nsym; s++)
    for (int i = 0; i < norm[s]; i++) {
      tsym[pos] = (uint8_t)s;
      pos = (pos + step) & mask;
      while (pos > high) pos = (pos + step) & mask;
    }
  for (int u = 0; u < size; u++) {
    const int s = tsym[u];
    t.state[cumul[s]++] = (uint16_t)(size + u);
  }
  int total = 0;
  for (int s = 0; s < nsym; s++) {
    const int n = norm[s];
    if (n == 0) {
      t.dnb[s] = ((uint32_t)(log + 1) << 16) - (1u << log);
      t.dfs[s] = 0;
    } else if (n == -1 || n == 1) {
      t.dnb[s] = ((uint32_t)log << 16) - (1u << log);
      t.dfs[s] = total - 1;
      total++;
    } else {
      const int max_out = log - highbit((uint32_t)n - 1);
      t.dnb[s] = ((uint32_t)max_out << 16) - ((uint32_t)n << max_out);
      t.dfs[s] = total - n;
      total += n;
    }
  }
  t.log = log;
}
ZE_HD uint32_t fse_init(const FseCT& t, int sym) {  // a state that holds sym (the cheapest to reach)
  const uint32_t nb = (t.dnb[sym] + (1u << 15)) >> 16;
  const uint32_t value = (nb << 16) - t.dnb[sym];
  return t.state[(int)(value >> nb) + t.dfs[sym]];
}
ZE_HD uint32_t fse_enc(const FseCT& t, BitW& w, uint32_t st, int sym) {  // the state before `st` that holds sym; writes the step
  const uint32_t nb = (st + t.dnb[sym]) >> 16;
  bw_add(w, st, (int)nb);
  return t.state[(int)(st >> nb) + t.dfs[sym]];
}

// predefined distributions (RFC 8878 3.1.1.3.2.2)
ZE_HD void build_predefined(Work& w) {
  static const int8_t LL[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
  static const int8_t OF[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
  static const int8_t ML[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
  int16_t norm[56];
  for (int i = 0; i < 36; i++) norm[i] = LL[i];
  fse_build(w.ll, norm, 36, kSeqLog, w.tsym, w.cumul);
  for (int i = 0; i < 29; i++) norm[i] = OF[i];
  fse_build(w.of, norm, 29, kOfLog, w.tsym, w.cumul);
  for (int i = 0; i < 53; i++) norm[i] = ML[i];
  fse_build(w.ml, norm, 53, kSeqLog, w.tsym, w.cumul);
}

// ---- literals -----------------------------------------------------------------------------------------------------------
// the table description of a normalised distribution (RFC 8878 4.1.1; no "less than one" probabilities here)
ZE_HD void write_ncount(BitW& b, const int16_t* norm, int log) {
  bw_add(b, (uint32_t)(log - 5), 4);
  int remaining = (1 << log) + 1, threshold = 1 << log, nbits = log + 1, sym = 0;
  bool prev0 = false;
  while (remaining > 1) {
    if (prev0) {
      int z = 0;
      while (norm[sym + z] == 0) z++;
      sym += z;
      while (z >= 3) {
        bw_add(b, 3, 2);
        z -= 3;
        bw_flush(b);
      }
      bw_add(b, (uint32_t)z, 2);
    }
    const int count = norm[sym++];
    const int value = count + 1, mx = (2 * threshold - 1) - remaining;
    if (value < mx) bw_add(b, (uint32_t)value, nbits - 1);
    else bw_add(b, (uint32_t)(value >= threshold ? value + mx : value), nbits);
    bw_flush(b);
    remaining -= count;
    prev0 = count == 0;
    while (remaining < threshold) {
      nbits--;
      threshold >>= 1;
    }
  }
}

// The FSE-compressed description of weights[0, ng) into w.wdesc + 1; returns its bytes, 0 when there is none (one distinct
// weight, or 128 bytes and more).  No weight gets more than half of the table, so every state reads at least one bit: the
// decoder finds the end of the stream where the state that holds the last-but-one weight cannot be updated.
ZE_HD int weights_fse(Work& w, int ng) {
  if (ng < 2) return 0;
  int count[13], distinct = 0, maxw = 0;
  for (int i = 0; i < 13; i++) count[i] = 0;
  for (int i = 0; i < ng; i++) count[w.weights[i]]++;
  for (int i = 0; i < 13; i++)
    if (count[i]) {
      distinct++;
      maxw = i;
    }
  if (distinct < 2) return 0;
  const int size = 1 << kWtLog, half = size >> 1;
  int16_t norm[13];
  int sum = 0;
  for (int i = 0; i < 13; i++) {
    int v = count[i] ? count[i] * size / ng : 0;
    if (count[i] && v < 1) v = 1;
    if (v > half) v = half;
    norm[i] = (int16_t)v;
    sum += v;
  }
  while (sum < size) {  // the most frequent weight that still has room takes what is missing
    int k = -1;
    for (int i = 0; i < 13; i++)
      if (count[i] && norm[i] < half && (k < 0 || count[i] > count[k])) k = i;
    const int give = size - sum < half - norm[k] ? size - sum : half - norm[k];
    norm[k] = (int16_t)(norm[k] + give);
    sum += give;
  }
  while (sum > size) {
    int k = 0;
    for (int i = 1; i < 13; i++)
      if (norm[i] > norm[k]) k = i;
    const int take = sum - size < norm[k] - 1 ? sum - size : norm[k] - 1;
    norm[k] = (int16_t)(norm[k] - take);
    sum -= take;
  }
  fse_build(w.wt, norm, maxw + 1, kWtLog, w.tsym, w.cumul);
  BitW b;
  bw_init(b, w.wdesc + 1, w.wdesc + 128);
  write_ncount(b, norm, kWtLog);
  bw_close(b, false);
  // two interleaved states: the even weights through state 0, the odd ones through state 1 (RFC 8878 4.2.1.2)
  uint32_t st[2];
  st[(ng - 1) & 1] = fse_init(w.wt, w.weights[ng - 1]);
  st[(ng - 2) & 1] = fse_init(w.wt, w.weights[ng - 2]);
  for (int k = ng - 1; k >= 2; k--) {
    st[k & 1] = fse_enc(w.wt, b, st[k & 1], w.weights[k - 2]);
    bw_flush(b);
  }
  bw_add(b, st[1], kWtLog);
  bw_add(b, st[0], kWtLog);
  bw_close(b, true);
  return b.ovf ? 0 : (int)(b.p - (w.wdesc + 1));
}

// w.hist -> code lengths (<= kHufMaxBits), codes, weights and their description.  Returns 0 when fewer than two byte values occur.
ZE_HD int huf_build(Work& w) {
  int m = 0, maxsym = 0;
  for (int s = 0; s < 256; s++) {
    w.cnt[s] = w.hist[s];
    w.nbits[s] = 0;
    w.weights[s] = 0;
    w.code[s] = 0;
    if (!w.hist[s]) continue;
    maxsym = s;
    int j = m++;
    while (j > 0 && w.hist[w.order[j - 1]] > w.hist[s]) {
      w.order[j] = w.order[j - 1];
      j--;
    }
    w.order[j] = (uint8_t)s;
  }
  w.nsym = m;
  w.maxsym = maxsym;
  w.wdesc_len = 0;
  if (m < 2) return 0;
  int maxd;
  for (;;) {
    // leaves 0..m-1 in ascending weight, internal nodes m..2m-2 in the order they are made (ascending too): two queues
    for (int i = 0; i < m; i++) w.nodew[i] = w.cnt[w.order[i]];
    int li = 0, ni = m, nn = m;
    while (nn < 2 * m - 1) {
      int pick[2];
      for (int k = 0; k < 2; k++) pick[k] = (li < m && (ni >= nn || w.nodew[li] <= w.nodew[ni])) ? li++ : ni++;
      w.nodew[nn] = w.nodew[pick[0]] + w.nodew[pick[1]];
      w.parent[pick[0]] = w.parent[pick[1]] = (uint16_t)nn;
      nn++;
    }
    w.nodew[2 * m - 2] = 0;
    for (int i = 2 * m - 3; i >= 0; i--) w.nodew[i] = w.nodew[w.parent[i]] + 1;  // depths
    maxd = 0;
    for (int i = 0; i < m; i++) maxd = (int)w.nodew[i] > maxd ? (int)w.nodew[i] : maxd;
    if (maxd <= kHufMaxBits) break;
    for (int i = 0; i < m; i++) w.cnt[w.order[i]] = (w.cnt[w.order[i]] + 1) >> 1;  // (keeps the order)
  }
  w.maxbits = maxd;
  for (int i = 0; i < m; i++) {
    const int s = w.order[i];
    w.nbits[s] = (uint8_t)w.nodew[i];
    w.weights[s] = (uint8_t)(maxd + 1 - (int)w.nodew[i]);
  }
  // symbols of one weight take consecutive codes, smaller weights (longer codes) first
  uint32_t at = 0;
  for (int wv = 1; wv <= maxd; wv++)
    for (int s = 0; s <= maxsym; s++)
      if (w.weights[s] == wv) {
        w.code[s] = (uint16_t)(at >> (wv - 1));
        at += 1u << (wv - 1);
      }
  // the description covers symbols 0 .. maxsym - 1 (the last weight is implied): direct (4 bits each, at most 128) or FSE
  const int ng = maxsym;
  const int fse = weights_fse(w, ng);
  const int direct = ng <= 128 ? (ng + 1) / 2 : 0;
  if (fse && (!direct || fse < direct)) {
    w.wdesc[0] = (uint8_t)fse;
    w.wdesc_len = 1 + fse;
  } else if (direct) {
    w.wdesc[0] = (uint8_t)(127 + ng);
    for (int i = 0; i < direct; i++)
      w.wdesc[1 + i] = (uint8_t)(w.weights[2 * i] << 4 | (2 * i + 1 < ng ? w.weights[2 * i + 1] : 0));
    w.wdesc_len = 1 + direct;
  }
  return 1;
}

// the quarter k of nl literals: [lo, hi)
ZE_HD void stream_range(uint32_t nl, int k, uint32_t* lo, uint32_t* hi) {
  const uint32_t q = (nl + 3) / 4;
  *lo = (uint32_t)k * q < nl ? (uint32_t)k * q : nl;
  *hi = k == 3 ? nl : ((uint32_t)(k + 1) * q < nl ? (uint32_t)(k + 1) * q : nl);
}

struct LitPlan {
  int32_t mode;        // 0 Raw, 1 RLE, 2 Huffman
  int32_t single;      // Huffman: one stream
  uint32_t data;       // where the literal bytes / the first stream start in the section
  uint32_t total;      // bytes of the section
  uint32_t soff[4], sbytes[4];  // Huffman: the streams (offsets in the section)
};

// Decides the form of the literals section of nl literals (w.hist / huf_build / w.sbits are in place when nl > 0 and two byte
// values occur) and writes everything in front of the literal bytes / streams to out[0, cap).  Returns 0 when cap is too small.
ZE_HD int lit_plan(const Work& w, uint32_t nl, uint8_t first, LitPlan& P, uint8_t* out, uint32_t cap) {
  const uint32_t rh = nl < 32 ? 1 : nl < 4096 ? 2 : 3;
  P.mode = (nl > 0 && w.nsym == 1) ? 1 : 0;
  P.single = 0;
  P.data = rh;
  P.total = P.mode == 1 ? rh + 1 : rh + nl;
  if (w.nsym >= 2 && w.wdesc_len > 0) {
    const int single = nl < 256;
    const uint32_t lh = 3 + (nl >= 1024) + (nl >= 16384);
    uint32_t csize = (uint32_t)w.wdesc_len;
    if (single) {
      P.sbytes[0] = (w.sbits[0] + w.sbits[1] + w.sbits[2] + w.sbits[3]) / 8 + 1;
      P.soff[0] = lh + csize;
      csize += P.sbytes[0];
    } else {
      csize += 6;
      for (int k = 0; k < 4; k++) {
        P.sbytes[k] = w.sbits[k] / 8 + 1;
        P.soff[k] = lh + csize;
        csize += P.sbytes[k];
      }
    }
    if (lh + csize < P.total) {
      P.mode = 2;
      P.single = single;
      P.data = P.soff[0];
      P.total = lh + csize;
      if (P.total > cap) return 0;
      const int sf = single ? 0 : (int)lh - 2;  // 3-byte header with 4 streams: 1; 4 bytes: 2; 5 bytes: 3
      const int bits = sf < 2 ? 10 : sf == 2 ? 14 : 18;
      const uint64_t h = 2u | (uint64_t)sf << 2 | (uint64_t)nl << 4 | (uint64_t)csize << (4 + bits);
      for (uint32_t i = 0; i < lh; i++) out[i] = (uint8_t)(h >> (8 * i));
      for (int i = 0; i < w.wdesc_len; i++) out[lh + i] = w.wdesc[i];
      if (!single)
        for (int k = 0; k < 3; k++) {
          out[lh + w.wdesc_len + 2 * k] = (uint8_t)P.sbytes[k];
          out[lh + w.wdesc_len + 2 * k + 1] = (uint8_t)(P.sbytes[k] >> 8);
        }
      return 1;
    }
  }
  if (P.total > cap) return 0;
  const uint32_t h = rh == 1 ? ((uint32_t)P.mode | nl << 3) : ((uint32_t)P.mode | (rh == 2 ? 1u : 3u) << 2 | nl << 4);
  for (uint32_t i = 0; i < rh; i++) out[i] = (uint8_t)(h >> (8 * i));
  if (P.mode == 1) out[rh] = first;
  return 1;
}

// one Huffman stream: the last symbol first, nbytes = bits / 8 + 1 (lit_plan)
ZE_HD void huf_encode_stream(const Work& w, const uint8_t* lits, uint32_t n, uint8_t* out, uint32_t nbytes) {
  BitW b;
  bw_init(b, out, out + nbytes);
  for (uint32_t i = n; i-- > 0;) {
    const int s = lits[i];
    bw_add(b, w.code[s], w.nbits[s]);
    if (b.nb >= 32) bw_flush(b);
  }
  bw_close(b, true);
}

// ---- sequences ----------------------------------------------------------------------------------------------------------
ZE_HD int ll_code(uint32_t ll, uint32_t* extra, int* nbits) {
  static const uint32_t B[36] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40,
                                 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
  static const uint8_t N[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
  int c = ll < 16 ? (int)ll : 35;
  while (B[c] > ll) c--;
  *extra = ll - B[c];
  *nbits = N[c];
  return c;
}
ZE_HD int ml_code(uint32_t ml, uint32_t* extra, int* nbits) {
  static const uint32_t B[53] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29,
                                 30, 31, 32, 33, 34, 35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195,
                                 16387, 32771, 65539};
  static const uint8_t N[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
  int c = ml < 35 ? (int)ml - 3 : 52;
  while (B[c] > ml) c--;
  *extra = ml - B[c];
  *nbits = N[c];
  return c;
}

// The sequences section of nseq sequences (match length >= 3, 1 <= offset < 2^17) into out[0, cap): count, mode byte 0
// (predefined tables), bit stream.  Returns its bytes, 0 when cap is too small.
ZE_HD uint32_t seq_encode(const Work& w, const uint64_t* seqs, uint32_t nseq, uint8_t* out, uint32_t cap) {
  if (nseq == 0) {
    if (cap < 1) return 0;
    out[0] = 0;
    return 1;
  }
  if (cap < 4) return 0;
  uint32_t h = 0;
  if (nseq < 128) {
    out[h++] = (uint8_t)nseq;
  } else if (nseq < 0x7F00) {
    out[h++] = (uint8_t)(128 + (nseq >> 8));
    out[h++] = (uint8_t)nseq;
  } else {
    out[h++] = 0xFF;
    out[h++] = (uint8_t)(nseq - 0x7F00);
    out[h++] = (uint8_t)((nseq - 0x7F00) >> 8);
  }
  out[h++] = 0;
  BitW b;
  bw_init(b, out + h, out + cap);
  uint32_t sl = 0, so = 0, sm = 0;
  for (uint32_t i = nseq; i-- > 0;) {
    const uint64_t s = seqs[i];
    uint32_t lx, mx;
    int ln, mn;
    const int lc = ll_code(seq_ll(s), &lx, &ln), mc = ml_code(seq_ml(s), &mx, &mn);
    const uint32_t ov = seq_off(s) + 3;
    const int oc = highbit(ov);
    if (i == nseq - 1) {
      sm = fse_init(w.ml, mc);
      so = fse_init(w.of, oc);
      sl = fse_init(w.ll, lc);
    } else {
      so = fse_enc(w.of, b, so, oc);
      sm = fse_enc(w.ml, b, sm, mc);
      sl = fse_enc(w.ll, b, sl, lc);
      bw_flush(b);
    }
    bw_add(b, lx, ln);
    bw_add(b, mx, mn);
    bw_flush(b);
    bw_add(b, ov - (1u << oc), oc);
    bw_flush(b);
  }
  bw_add(b, sm, kSeqLog);
  bw_add(b, so, kOfLog);
  bw_add(b, sl, kSeqLog);
  bw_close(b, true);
  return b.ovf ? 0 : (uint32_t)(b.p - out);
}

// ---- block and frame headers ----------------------------------------------------------------------------------------------
enum { kBlockRaw = 0, kBlockRle = 1, kBlockCompressed = 2 };
ZE_HD void put_block_header(uint8_t* p, bool last, int type, uint32_t size) {
  const uint32_t v = (last ? 1u : 0u) | (uint32_t)type << 1 | size << 3;
  p[0] = (uint8_t)v;
  p[1] = (uint8_t)(v >> 8);
  p[2] = (uint8_t)(v >> 16);
}
// byte i of the frame header of a frame of `content` bytes: no dictionary id, no checksum, window = kBlock
ZE_HD uint8_t frame_header_byte(int i, uint64_t content) {
  const uint64_t lo = 0x38C0FD2FB528ull;  // 28 B5 2F FD | FHD 0xC0 (8-byte content size) | window descriptor 0x38 (2^17)
  return i < 6 ? (uint8_t)(lo >> (8 * i)) : (uint8_t)(content >> (8 * (i - 6)));
}

#ifndef S3S_ZSTD_DEVICE
// ---- host: the whole writer on one thread ---------------------------------------------------------------------------------
// The content of a Compressed_Block from sequences + literals into out[0, cap): returns its bytes, 0 when it does not fit.
static inline uint32_t encode_block_body(Work& w, const uint64_t* seqs, uint32_t nseq, const uint8_t* lits, uint32_t nl,
                                         uint8_t* out, uint32_t cap) {
  for (int s = 0; s < 256; s++) w.hist[s] = 0;
  for (uint32_t i = 0; i < nl; i++) w.hist[lits[i]]++;
  if (huf_build(w))
    for (int k = 0; k < 4; k++) {
      uint32_t lo, hi, bits = 0;
      stream_range(nl, k, &lo, &hi);
      for (uint32_t i = lo; i < hi; i++) bits += w.nbits[lits[i]];
      w.sbits[k] = bits;
    }
  LitPlan P;
  if (!lit_plan(w, nl, nl ? lits[0] : 0, P, out, cap)) return 0;
  if (P.mode == 0) {
    memcpy(out + P.data, lits, nl);
  } else if (P.mode == 2) {
    if (P.single) {
      huf_encode_stream(w, lits, nl, out + P.soff[0], P.sbytes[0]);
    } else {
      for (int k = 0; k < 4; k++) {
        uint32_t lo, hi;
        stream_range(nl, k, &lo, &hi);
        huf_encode_stream(w, lits + lo, hi - lo, out + P.soff[k], P.sbytes[k]);
      }
    }
  }
  const uint32_t sq = seq_encode(w, seqs, nseq, out + P.total, cap - P.total);
  return sq ? P.total + sq : 0;
}

// The device's parse, restated: 64 positions per step look their 4 bytes up in the table as it was before the step; the first
// one that finds them starts a match (extended forwards to the block's end, backwards by at most 64 bytes into the pending
// literals); the positions up to it enter the table.  seqs[kMaxSeq], lits[n].
static inline void parse_block(const uint8_t* src, uint32_t n, uint32_t* tab, uint64_t* seqs, uint32_t* nseq_out, uint8_t* lits,
                               uint32_t* nl_out) {
  for (int i = 0; i < (1 << kHashLog); i++) tab[i] = 0;
  uint32_t ip = 0, anchor = 0, nseq = 0, nl = 0;
  while (ip + 4 <= n && nseq < (uint32_t)kMaxSeq) {
    // every position that finds its 4 bytes measures the match (kProbe more bytes at most); of those within kLazy positions
    // behind the first, the one that gains most (length minus the literals it leaves in front) starts the match
    int k = -1, k0 = -1, best = 0;
    uint32_t cand = 0;
    for (int lane = 0; lane < kStep && (k0 < 0 || lane < k0 + kLazy); lane++) {
      const uint32_t p = ip + (uint32_t)lane;
      if (p + 4 > n) break;
      const uint32_t v = rd32(src + p), c = tab[hash4(v)];
      if (!c || rd32(src + c - 1) != v) continue;
      if (k0 < 0) k0 = lane;
      int len = 4;
      while (len < 4 + kProbe && p + len < n && src[p + len] == src[c - 1 + len]) len++;
      if (len - (lane - k0) > best) {
        best = len - (lane - k0);
        k = lane;
        cand = c - 1;
      }
    }
    for (int lane = 0; lane <= (k < 0 ? kStep - 1 : k); lane++) {
      const uint32_t p = ip + (uint32_t)lane;
      if (p + 4 > n) break;
      uint32_t& e = tab[hash4(rd32(src + p))];
      e = e > p + 1 ? e : p + 1;
    }
    if (k < 0) {
      ip += kStep;
      continue;
    }
    uint32_t m = ip + (uint32_t)k, c = cand, ml = 4;
    while (m + ml < n && src[m + ml] == src[c + ml]) ml++;
    const uint32_t end = m + ml;
    int back = 0;
    while (back < kStep && m - back > anchor && c - back > 0 && src[m - back - 1] == src[c - back - 1]) back++;
    m -= back;
    c -= back;
    ml += back;
    memcpy(lits + nl, src + anchor, m - anchor);
    nl += m - anchor;
    seqs[nseq++] = seq_pack(m - anchor, ml, m - c);
    anchor = ip = end;
  }
  memcpy(lits + nl, src + anchor, n - anchor);
  nl += n - anchor;
  *nseq_out = nseq;
  *nl_out = nl;
}

// One block (header included) into out[0, 3 + n): RLE when all bytes are equal, Raw when the compressed form is not smaller.
// seqs == nullptr: parse here (scratch: tab[1 << kHashLog], pseq[kMaxSeq], plit[n]).  Returns the bytes written.
static inline uint32_t encode_block(Work& w, const uint8_t* src, uint32_t n, bool last, const uint64_t* seqs, uint32_t nseq,
                                    const uint8_t* lits, uint32_t nl, uint32_t* tab, uint64_t* pseq, uint8_t* plit, uint8_t* out) {
  bool equal = true;
  for (uint32_t i = 1; i < n && equal; i++) equal = src[i] == src[0];
  if (equal && !seqs) {
    put_block_header(out, last, kBlockRle, n);
    out[3] = src[0];
    return 4;
  }
  if (!seqs) {
    parse_block(src, n, tab, pseq, &nseq, plit, &nl);
    seqs = pseq;
    lits = plit;
  }
  const uint32_t body = n > 1 ? encode_block_body(w, seqs, nseq, lits, nl, out + 3, n - 1) : 0;
  if (body) {
    put_block_header(out, last, kBlockCompressed, body);
    return 3 + body;
  }
  put_block_header(out, last, kBlockRaw, n);
  memcpy(out + 3, src, n);
  return 3 + n;
}
#endif

}  // namespace s3s_zstd_enc
