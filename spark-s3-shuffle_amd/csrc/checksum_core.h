// checksum_core.h — the constant tables and the GF(2) polynomial arithmetic the checksum kernels share (checksum.hip: segments,
// fold, combine; decode_stream_kernels.hip: the seed step).
#pragma once
#include "s3s_internal.h"

namespace s3s {
namespace {

constexpr uint32_t kAdlerMod = 65521u;

struct Tables {             // built on the host once per context (codec_api.hip): one set per CRC polynomial
  uint32_t slice[4][256];   // slice-by-4 tables of the reflected polynomial
  uint32_t pow_piece[256];  // x^(8*64*k) mod P
  uint32_t x2n[32];         // x^(2^k) mod P
  uint32_t poly, pad[3];    // 0xEDB88320 (CRC-32, IEEE 802.3: java.util.zip.CRC32) / 0x82F63B78 (CRC-32C, Castagnoli: java.util.zip.CRC32C)
};
constexpr uint32_t kPolyIeee = 0xEDB88320u, kPolyCastagnoli = 0x82F63B78u;

// a(x) * b(x) mod P in the reflected representation (zlib multmodp), branch-free
__device__ __forceinline__ uint32_t multmodp(uint32_t a, uint32_t b, uint32_t poly) {
  uint32_t p = 0;
#pragma unroll
  for (int i = 0; i < 32; i++) {
    p ^= (a & (0x80000000u >> i)) ? b : 0u;
    b = (b >> 1) ^ (poly & (0u - (b & 1u)));
  }
  return p;
}

// x^(8n) mod P; x2n[k] = x^(2^k), k < 32.  zlib wraps that table (x2n[k & 31]) because x^(2^32) = x modulo ITS polynomial, which
// is irreducible.  CRC-32C's is not - it is (x + 1) times a polynomial of degree 31, and x^(2^32) = x^2 there - so from
// n = 2^29 bytes on (a range of 512 MiB and more) the powers are squared on from the table's last entry instead.
__device__ __forceinline__ uint32_t x8n(const uint32_t* x2n, uint64_t n, uint32_t poly) {
  uint32_t p = 0x80000000u;
  for (int k = 3; n && k < 32; n >>= 1, k++)
    if (n & 1) p = multmodp(x2n[k], p, poly);
  if (n) {
    uint32_t sq = x2n[31];
    for (; n; n >>= 1) {
      sq = multmodp(sq, sq, poly);
      if (n & 1) p = multmodp(sq, p, poly);
    }
  }
  return p;
}

// A checksum continued: `own` is the checksum of a range of len bytes alone, `seed` the state (getValue()) in front of it; the
// state behind it.  The identities are written out at checksum_seed_kernel (decode_stream_kernels.hip), which keeps its own copy
// so that it stays what it was; the batched feed's seed step (decode_stream_batch.hip) calls this one.
template <int ALGO>
__device__ __forceinline__ int64_t checksum_continue(const Tables* __restrict__ tabs, uint64_t len, uint32_t seed, uint32_t own) {
  if (ALGO == S3S_CHECKSUM_ADLER32) {
    const uint64_t rem = len % kAdlerMod, a1 = seed & 0xffffu, b1 = seed >> 16, a2 = own & 0xffffu, b2 = own >> 16;
    const uint64_t a = (a1 + a2 + kAdlerMod - 1) % kAdlerMod;
    const uint64_t b = (rem * a1 + b1 + b2 + kAdlerMod - rem) % kAdlerMod;
    return (int64_t)(b << 16 | a);
  }
  return (int64_t)(uint64_t)(multmodp(x8n(tabs->x2n, len, tabs->poly), seed, tabs->poly) ^ own);
}

}  // namespace
}  // namespace s3s
