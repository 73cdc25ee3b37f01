// discover_core.h — what the frame-discovery kernels of the reduce side share: the LZ4Block header checks of
// LZ4BlockInputStream.refill() and the SnappyInputStream header test (lz4_decompress.hip, snappy_decompress.hip: the one-shot
// discovery; decode_stream_kernels.hip: the stream-mode discovery).
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

}  // namespace
}  // namespace s3s
