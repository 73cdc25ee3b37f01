// aes_ctr.hip — Spark IO encryption (AES/CTR/NoPadding) as a layer between the codec and the checksums.
//
// With spark.io.encryption.enabled a non-empty partition is stored as  IV (16 bytes) | codec bytes XOR key stream  and an
// empty one stays 0 bytes (aes_ctr_core.h).  One kernel does the pass in three forms:
//   kCtrInPlace    map side behind a codec: the gather left a 16-byte hole in front of every non-empty partition of the
//                  .data image (kItemIv); the hole gets the IV, the bytes behind it are XORed where they lie
//   kCtrFromPlain  map side, codec NONE: source partition -> IV | cipher text in the image, in one pass
//   kCtrDecrypt    reduce side: stored range -> the codec bytes alone (IVs dropped) in a workspace buffer; the IV is read
//                  from the stream
// "E" are the n + 1 offsets of the STORED partitions (the .index: device-side B_INDEX on the map side, where the host does
// not know the compressed sizes before the sync), "Q" the offsets of the plain side (kCtrFromPlain / kCtrDecrypt).
//
// Work split.  The stored bytes are cut into tiles of kCtrTile bytes, one workgroup each; a thread takes chunks of 16 stored
// bytes.  Partition starts have every residue mod 16, so key stream blocks are not aligned with memory: a thread does not
// own the 16 bytes of its chunk but the UNITS that START inside it - the IV of a partition that begins there, or the key
// stream block j of the partition the chunk lies in (stored bytes [E[p] + 16 + 16 j, + 16), cut at the partition's end).
// Every stored byte belongs to exactly one unit and every unit starts in exactly one chunk, so a chunk inside a partition
// costs ONE block encryption (not the two that its 16 bytes straddle), and a chunk that holds a partition boundary two.
// The workgroup finds the partitions of its tile by two binary searches over E (wave-uniform), a lane its own between them.
//
// S-box.  No LDS is booked: the codec kernels of other task threads fill the LDS of every CU, and a workgroup that asks for
// even 1 KiB waits for one of their blocks to finish (the reason scan_items and checksum.hip are LDS-free).
// The 256 S-box bytes are ONE register across the 64 lanes of a wavefront (lane k holds bytes 4 k .. 4 k + 3) and a lookup
// is one ds_bpermute_b32 - the LDS crossbar without an LDS allocation, no bank conflicts by construction (every lane names a
// lane, not an address) - plus a shift.  MixColumns is arithmetic on packed columns (xtime on four bytes at once), so a
// round is 16 lookups and ~60 vector ALU operations.  A T-table would save the MixColumns arithmetic but is 1 KiB: four
// registers across the wave and four lookups plus selects per byte, or an LDS allocation.  ds_bpermute reads only from
// ACTIVE lanes, so all 64 lanes of every wavefront stay in the block encryption (lanes without a unit encrypt a dummy
// counter); only the loads and stores around it are predicated.
//
// The round keys (at most 60 dwords) are kernel arguments: wave-uniform scalars, never in the device workspace.
// All offsets and block numbers are 64-bit.
#define S3S_AES_DEVICE
#include "aes_ctr_core.h"
#include "s3s_internal.h"

namespace s3s {
namespace {

constexpr int kCtrThreads = 256;
constexpr int kCtrChunks = 4;                                   // chunks of 16 stored bytes per thread
constexpr int kCtrTile = 16 * kCtrThreads * kCtrChunks;         // stored bytes per workgroup

struct LaneSbox {
  uint32_t word;  // S-box bytes 4 lane .. 4 lane + 3
  __device__ __forceinline__ uint32_t operator()(uint32_t x) const {
    const uint32_t w = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(x & 0xfcu), (int)word);  // lane x / 4
    return (w >> ((x & 3u) * 8u)) & 0xffu;
  }
};

// the last p in [lo, hi] with E[p] <= x (E[lo] <= x)
__device__ __forceinline__ int32_t last_start_le(const int64_t* __restrict__ E, int32_t lo, int32_t hi, int64_t x) {
  while (lo < hi) {
    const int32_t mid = (int32_t)(((int64_t)lo + hi + 1) >> 1);
    if (E[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

template <int NR, int MODE>
__global__ __launch_bounds__(kCtrThreads) void aes_ctr_kernel(const AesKeys keys, const uint8_t* __restrict__ in, uint8_t* out,
                                                              const int64_t* __restrict__ E, const int64_t* __restrict__ Q,
                                                              const uint8_t* __restrict__ ivs, int32_t n, int64_t e_limit) {
  const int64_t e_all = E[n];
  const int64_t hard_end = e_all < e_limit ? e_all : e_limit;  // (a map-side image that overflowed its capacity is not touched beyond it)
  const int64_t tile0 = E[0] + (int64_t)blockIdx.x * kCtrTile;
  if (tile0 >= hard_end) return;  // the whole workgroup
  const int64_t tile_end = tile0 + kCtrTile < hard_end ? tile0 + kCtrTile : hard_end;
  const LaneSbox sbox{s3s_aes::sbox_word(threadIdx.x & 63u)};
  const int32_t p_lo = last_start_le(E, 0, n - 1, tile0), p_hi = last_start_le(E, p_lo, n - 1, tile_end - 1);

  for (int k = 0; k < kCtrChunks; k++) {
    const int64_t x0 = tile0 + 16 * ((int64_t)threadIdx.x + (int64_t)kCtrThreads * k);
    const bool live = x0 < tile_end;
    const int64_t lim = x0 + 16 < tile_end ? x0 + 16 : tile_end;
    int32_t p = last_start_le(E, p_lo, p_hi, x0);  // live: E[p] <= x0 < E[p + 1]
    int64_t ep = E[p], en = E[p + 1];
    int64_t xs = x0 + ((16 - ((x0 - ep) & 15)) & 15);  // the first unit start of partition p at or behind x0
    for (;;) {
      // the partition ends in front of the unit and inside the chunk: the next non-empty one starts there with its IV
      // (en < lim <= E[n], so p + 1 < n)
      while (live && xs >= en && en < lim) {
        p++;
        ep = en;
        en = E[p + 1];
        if (en > ep) xs = ep;
      }
      const bool has = live && xs < lim;
      if (__builtin_amdgcn_ballot_w64(has) == 0) break;  // wave-uniform: every lane stays for the block encryption
      const int64_t j = xs - ep;  // 0: the IV; 16 (b + 1): key stream block b
      const int64_t part_end = en < hard_end ? en : hard_end;
      const int len = has ? (int)(part_end - xs < 16 ? part_end - xs : 16) : 0;
      uint32_t ivw[4] = {0, 0, 0, 0};
      const uint8_t* ivp = MODE == kCtrDecrypt ? in + ep : ivs + 16 * (int64_t)p;
      if (has) {
        __builtin_memcpy(ivw, ivp, 16);
#pragma unroll
        for (int w = 0; w < 4; w++) ivw[w] = __builtin_bswap32(ivw[w]);
      }
      uint32_t ks[4];
      s3s_aes::keystream_block(keys.rk, NR, ivw, (uint64_t)(j >> 4) - 1, ks, sbox);
      if (has) {
        if (j == 0) {
          if (MODE != kCtrDecrypt) {  // (the reduce side drops the IV)
            uint8_t* d = out + xs;
            for (int i = 0; i < len; i++) d[i] = ivp[i];
          }
        } else {
          const int64_t plain = MODE == kCtrInPlace ? 0 : Q[p] + (j - 16);
          const uint8_t* s = MODE == kCtrInPlace ? out + xs : MODE == kCtrFromPlain ? in + plain : in + xs;
          uint8_t* d = MODE == kCtrDecrypt ? out + plain : out + xs;
          if (len == 16) {
            uint32_t v[4];
            __builtin_memcpy(v, s, 16);
#pragma unroll
            for (int w = 0; w < 4; w++) v[w] ^= __builtin_bswap32(ks[w]);
            __builtin_memcpy(d, v, 16);
          } else {
            for (int i = 0; i < len; i++) d[i] = (uint8_t)(s[i] ^ (ks[i >> 2] >> (24 - 8 * (i & 3))));
          }
        }
      }
      xs += 16;
    }
  }
}

// item_size of the kItemIv records (the codec kernels pass the kind by)
__global__ __launch_bounds__(kCtrThreads) void seed_iv_items_kernel(const Item* __restrict__ items, int32_t n_items,
                                                                   uint32_t* __restrict__ item_size) {
  const int64_t i = (int64_t)blockIdx.x * kCtrThreads + threadIdx.x;
  if (i < n_items && (items[i].kind & 0xff) == kItemIv) item_size[i] = (uint32_t)s3s_aes::kBlock;
}

template <int NR>
void launch_mode(int mode, unsigned grid, hipStream_t st, const AesKeys& keys, const uint8_t* in, uint8_t* out, const int64_t* E,
                 const int64_t* Q, const uint8_t* ivs, int32_t n, int64_t e_limit) {
  if (mode == kCtrInPlace)
    hipLaunchKernelGGL((aes_ctr_kernel<NR, kCtrInPlace>), dim3(grid), dim3(kCtrThreads), 0, st, keys, in, out, E, Q, ivs, n, e_limit);
  else if (mode == kCtrFromPlain)
    hipLaunchKernelGGL((aes_ctr_kernel<NR, kCtrFromPlain>), dim3(grid), dim3(kCtrThreads), 0, st, keys, in, out, E, Q, ivs, n, e_limit);
  else
    hipLaunchKernelGGL((aes_ctr_kernel<NR, kCtrDecrypt>), dim3(grid), dim3(kCtrThreads), 0, st, keys, in, out, E, Q, ivs, n, e_limit);
}

}  // namespace

int aes_expand_key(const uint8_t* key, int key_bytes, AesKeys* keys) { return s3s_aes::expand_key(key, key_bytes, keys->rk); }

int64_t aes_ctr_max_bytes() { return (int64_t)0x7fffffff * kCtrTile; }

void launch_aes_ctr(int mode, const AesKeys& keys, int rounds, const uint8_t* d_in, uint8_t* d_out, const int64_t* d_stored_off,
                    const int64_t* d_plain_off, const uint8_t* d_ivs, int32_t n_parts, int64_t stored_bound, int64_t stored_limit,
                    hipStream_t st) {
  if (n_parts <= 0 || stored_bound <= 0) return;
  const unsigned grid = (unsigned)((stored_bound + kCtrTile - 1) / kCtrTile);
  if (rounds == 10) launch_mode<10>(mode, grid, st, keys, d_in, d_out, d_stored_off, d_plain_off, d_ivs, n_parts, stored_limit);
  else if (rounds == 12) launch_mode<12>(mode, grid, st, keys, d_in, d_out, d_stored_off, d_plain_off, d_ivs, n_parts, stored_limit);
  else launch_mode<14>(mode, grid, st, keys, d_in, d_out, d_stored_off, d_plain_off, d_ivs, n_parts, stored_limit);
}

void launch_seed_iv_items(const Item* d_items, int32_t n_items, uint32_t* d_item_size, hipStream_t st) {
  if (n_items <= 0) return;
  hipLaunchKernelGGL(seed_iv_items_kernel, dim3((unsigned)((n_items + kCtrThreads - 1) / kCtrThreads)), dim3(kCtrThreads), 0, st,
                     d_items, n_items, d_item_size);
}

}  // namespace s3s
