// discover_core.h — what the frame-discovery kernels of the reduce side share: the LZ4Block header checks of
// LZ4BlockInputStream.refill() and the SnappyInputStream header test (lz4_decompress.hip, snappy_decompress.hip: the one-shot
// discovery; decode_stream_kernels.hip: the stream-mode discovery), the one-wavefront scan, and the stream-mode walks with the
// stop rule, which the single feed (decode_stream_kernels.hip) and the batched feed (decode_stream_batch.hip) both run.
#pragma once
#include "s3s_internal.h"

namespace s3s {
namespace {

constexpr int kTileBytes = 65536;
constexpr uint64_t kMagic = 0x6b636f6c42345a4cull;  // "LZ4Block" little-endian

__device__ __forceinline__ uint64_t ld64u(const uint8_t* p) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}
__device__ __forceinline__ uint32_t ld32u(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

struct Header {
  int32_t method, comp_len, orig_len;
  uint32_t check;
  bool ok;
};

// LZ4BlockInputStream.refill() header checks (magic excluded)
__device__ __forceinline__ Header parse_header(const uint8_t* h) {
  Header r;
  const uint32_t token = h[8];
  r.method = (int32_t)(token & 0xF0u);
  const int level = 10 + (int)(token & 0x0Fu);
  r.comp_len = (int32_t)ld32u(h + 9);
  r.orig_len = (int32_t)ld32u(h + 13);
  r.check = ld32u(h + 17);
  r.ok = (r.method == 0x10 || r.method == 0x20) && r.orig_len >= 0 && r.comp_len >= 0 &&
         r.orig_len <= (1 << level) && !(r.orig_len == 0 && r.comp_len != 0) &&
         !(r.orig_len != 0 && r.comp_len == 0) && !(r.method == 0x10 && r.orig_len != r.comp_len) &&
         !(r.orig_len == 0 && r.check != 0);
  return r;
}

__device__ __forceinline__ bool is_stream_header(const uint8_t* c) {
  return c[0] == 0x82 && c[1] == 'S' && c[2] == 'N' && c[3] == 'A' && c[4] == 'P' && c[5] == 'P' &&
         c[6] == 'Y' && c[7] == 0;
}

// generic exclusive scan of uint32 -> int64 (n+1 outputs): ONE wavefront, NO LDS — the decode kernels of
// the other task threads book the whole LDS of every CU (20 x 8 KiB rings), and a workgroup that needs
// any of it waits for one of their frames to finish (see scan_items_kernel in assemble.hip)
__device__ __forceinline__ void scan_u32_wave(const uint32_t* __restrict__ in, int64_t n, int64_t* __restrict__ out,
                                              int lane) {
  int64_t carry = 0;
  for (int64_t tile = 0; tile < n; tile += 4 * kWave) {
    const int64_t i0 = tile + 4 * lane;
    int64_t x[4];
#pragma unroll
    for (int k = 0; k < 4; k++) x[k] = i0 + k < n ? (int64_t)in[i0 + k] : 0;
    const int64_t mine = x[0] + x[1] + x[2] + x[3];
    int64_t inc = mine;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const int64_t y = __shfl_up(inc, d);
      if (lane >= d) inc += y;
    }
    int64_t off = carry + inc - mine;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (i0 + k < n) out[i0 + k] = off;
      off += x[k];
    }
    carry += __shfl(inc, kWave - 1);
  }
  if (lane == 0) out[n] = carry;
}

// ---- stream mode (s3s_dstream_feed*): the window comp[0, comp_len) may end inside a frame ---------------------------------
// walk_tile with the stop rule: a frame whose header or payload crosses comp_len ends the chain (*need = its length as far
// as the window shows it, the return value = where it starts) unless it crosses range_left too - then the RANGE ends
// inside it, which is the one-shot walk's "Stream ended prematurely".  A header is read only when all 21 bytes of it lie
// in front of comp_len.  Counts only: the frames are emitted by the one-shot tile_emit_kernel up to the stop offset.
__device__ int64_t walk_tile_stream(const uint8_t* comp, int64_t comp_len, int64_t range_left, int64_t pos, int64_t tile_end,
                                    int32_t* count_out, int64_t* need) {
  int32_t n = 0;
  *need = 0;
  while (pos < tile_end && pos < comp_len) {
    int64_t unit = kLz4FrameHeader;
    if (comp_len - pos >= kLz4FrameHeader) {
      const uint8_t* h = comp + pos;
      if (ld64u(h) != kMagic) return -1;
      const Header hd = parse_header(h);
      if (!hd.ok) return -1;
      unit += hd.comp_len;
    }
    if (unit > range_left - pos) return -1;
    if (unit > comp_len - pos) {
      *need = unit;
      break;
    }
    n++;
    pos += unit;
  }
  *count_out = n;
  return pos;
}

// ---- stream mode (s3s_dstream_feed*): pieces of partitions inside a window that may end inside a unit -------------------
// One piece [beg, end) of a partition that ends at pend >= end (pend > end: the window ends first).  A unit - a stream
// header, a length | chunk, a ZV chunk - is read only when it lies in front of `end`; one that does not fit in front of
// pend is the one-shot walk's corruption (-1), one that fits there but not in front of `end` ends the walk: *stop = where
// it starts, *need = its length as far as the piece shows it (the header's when the header is cut, then header + payload).
// mid: the piece starts inside a Snappy stream, so no stream header is expected at beg.  Returns the chunks in front of *stop.
// A Snappy chunk whose varint claims more than kBatchMaxBlock decoded bytes ends the walk with -2: no decoder takes it, and a
// caller must not be sent for a buffer of that size (need_dst) - an LZ4Block frame is bounded by parse_header, an LZF chunk by
// its 16-bit field, a Snappy varint by nothing.
struct PieceWalk {
  int64_t ip, end, pend, need;
  // 0: x more bytes are there; 1: the window ends first (need set); -1: the partition ends first
  __device__ __forceinline__ int want(int64_t x) {
    if (x > pend - ip) return -1;
    if (x > end - ip) {
      need = x;
      return 1;
    }
    return 0;
  }
};

__device__ int walk_piece_stream(const uint8_t* comp, int64_t beg, int64_t end, int64_t pend, bool mid, int chunk_format, bool emit,
                                 Frame* frames, uint32_t* frame_orig, int64_t* stop, int64_t* need) {
  PieceWalk w{beg, end, pend, 0};
  int n = 0;
  bool header_next = !mid && chunk_format != kChunkLzf;
  while (w.ip < end) {
    int r;
    Frame f;
    int64_t unit;
    if (chunk_format == kChunkLzf) {
      if ((r = w.want(5)) != 0) { if (r < 0) return -1; break; }
      if (comp[w.ip] != 'Z' || comp[w.ip + 1] != 'V' || comp[w.ip + 2] > 1) return -1;
      const int type = comp[w.ip + 2];
      const uint32_t len = (uint32_t)comp[w.ip + 3] << 8 | comp[w.ip + 4];
      const int head = type == 1 ? 7 : 5;
      uint32_t ulen = len;
      if (type == 1) {
        if ((r = w.want(7)) != 0) { if (r < 0) return -1; break; }
        ulen = (uint32_t)comp[w.ip + 5] << 8 | comp[w.ip + 6];
        if (len == 0 || ulen == 0) return -1;
      }
      unit = head + (int64_t)len;
      if ((r = w.want(unit)) != 0) { if (r < 0) return -1; break; }
      f = Frame{w.ip + head, (int32_t)len, (int32_t)ulen, 0u, type == 1 ? 2 : 0x10};
    } else {
      if (header_next) {
        if ((r = w.want(kSnappyStreamHeader)) != 0) { if (r < 0) return -1; break; }
        if (!is_stream_header(comp + w.ip)) return -1;
        w.ip += kSnappyStreamHeader;
        header_next = false;
        continue;
      }
      if ((r = w.want(4)) != 0) { if (r < 0) return -1; break; }
      const uint32_t cl = (uint32_t)comp[w.ip] << 24 | (uint32_t)comp[w.ip + 1] << 16 | (uint32_t)comp[w.ip + 2] << 8 |
                          (uint32_t)comp[w.ip + 3];
      if (cl == 0x82534e41u) {  // the next concatenated stream starts here
        header_next = true;
        continue;
      }
      if (cl == 0) return -1;
      unit = 4 + (int64_t)cl;
      if ((r = w.want(unit)) != 0) { if (r < 0) return -1; break; }
      uint32_t ulen = 0;
      int sh = 0;
      for (uint32_t i = 0;; i++, sh += 7) {
        if (i >= cl || sh > 28) return -1;
        const uint32_t b = comp[w.ip + 4 + i];
        ulen |= (b & 0x7fu) << sh;
        if (!(b & 0x80u)) break;
      }
      if (ulen > (uint32_t)kBatchMaxBlock) return -2;
      f = Frame{w.ip + 4, (int32_t)cl, (int32_t)ulen, 0u, 1};
    }
    if (emit) {
      frames[n] = f;
      frame_orig[n] = (uint32_t)f.orig_len;
    }
    n++;
    w.ip += unit;
  }
  *stop = w.ip;
  *need = w.need;
  return n;
}

// One lane per piece raises the window's status word, so the word must not depend on which lane comes last: corruption in any
// piece (-1) is S3S_E_BAD_FRAME whatever the other pieces say, a refused claim (-2) is written only over "no error".
__device__ __forceinline__ void raise_piece_status(int32_t* status, int n) {
  if (n == -2) atomicCAS(status, 0, S3S_E_UNSUPPORTED);
  else atomicExch(status, S3S_E_BAD_FRAME);
}

}  // namespace
}  // namespace s3s
