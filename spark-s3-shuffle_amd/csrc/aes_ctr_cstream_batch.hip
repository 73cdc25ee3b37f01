// aes_ctr_cstream_batch.hip — the AES-CTR pass of the streaming map side (aes_ctr_cstream.hip) over the outputs of ALL windows
// of a batched feed under IO encryption (s3s_cstream_feed_batch*, compress_stream.hip): ONE launch writes the
// IVs into the holes the cut gather left and XORs the key stream over d_dst[0, out_len) of every window, in place.  Work split,
// S-box, block encryption and predication are the single kernel's - the tile body is the same text
// (aes_ctr_cstream_tile.inc) - and what a window is comes from a PassWindow descriptor in the call's arena
// (compress_stream_batch_core.h) instead of kernel arguments.  In place only: S3S_CODEC_NONE is not batched.  A file of its
// own: the single kernel keeps the instructions it had.
#define S3S_AES_DEVICE
#include "aes_ctr_stream_core.h"
#include "compress_stream_batch_core.h"
#include "s3s_internal.h"

namespace s3s {
namespace {

constexpr int kCsThreads = 256;
constexpr int kCsChunks = 4;                               // as in aes_ctr_cstream.hip: chunks of 16 stored bytes per thread,
constexpr int kCsTileChunks = kCsThreads * kCsChunks;      // chunks per workgroup,
constexpr int kCsTile = 16 * kCsTileChunks;                // stored bytes per workgroup
static_assert(kCsTile == s3s_cs::kPassTile, "the host sizes the grid in these tiles");

struct LaneSbox {
  uint32_t word;  // S-box bytes 4 lane .. 4 lane + 3
  __device__ __forceinline__ uint32_t operator()(uint32_t x) const {
    const uint32_t w = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(x & 0xfcu), (int)word);  // lane x / 4
    return (w >> ((x & 3u) * 8u)) & 0xffu;
  }
};

// PassWindow as the kernel reads it: a pointer read from a descriptor names global memory, and saying so in its type keeps every
// access through it a global one (the single kernel's pointers are kernel arguments, which the compiler knows to be global)
#define S3S_GLOBAL __attribute__((address_space(1)))
struct PassWindowDev {
  S3S_GLOBAL uint8_t* out;
  const S3S_GLOBAL int64_t* E;
  const S3S_GLOBAL uint8_t* ivs;
  const S3S_GLOBAL int64_t* cut;
  int32_t n_pieces, tile0;
  int64_t front;
};
static_assert(sizeof(PassWindowDev) == sizeof(s3s_cs::PassWindow) && alignof(PassWindowDev) == alignof(s3s_cs::PassWindow), "one layout");

// The grid is the sum of the windows' tile counts (host bounds: out_len is the device's).  A workgroup finds its window through
// the tile -> window map, once (blockIdx is uniform: the descriptor arrives in scalar registers), reads THAT window's out_len
// from its cut words and is then a workgroup of the single kernel on tile blockIdx.x - tile0 of that output: it returns whole
// at or beyond out_len, and when out_len is 0 (the window's first unit did not fit its dst).
template <int NR>
__global__ __launch_bounds__(kCsThreads) void aes_ctr_cstream_batch_kernel(const AesKeys keys, const PassWindowDev* __restrict__ wins,
                                                                          const int32_t* __restrict__ tile_win, int32_t total_tiles) {
  if ((int32_t)blockIdx.x >= total_tiles) return;
  const PassWindowDev w = wins[tile_win[blockIdx.x]];
  constexpr int MODE = kCsInPlace;
  const uint8_t* src = nullptr;  // (kCsFromPlain only)
  const int64_t* Q = nullptr;
  uint8_t* out = (uint8_t*)w.out;
  const int64_t* __restrict__ E = (const int64_t*)w.E;
  const uint8_t* __restrict__ ivs = (const uint8_t*)w.ivs;
  const int32_t n = w.n_pieces;
  const int64_t front = w.front;
  const int64_t L = w.cut[s3s_cs::kCutOutLen];
#define S3S_CS_TILE (blockIdx.x - (uint32_t)w.tile0)
#include "aes_ctr_cstream_tile.inc"
#undef S3S_CS_TILE
}

}  // namespace

void launch_aes_ctr_cstream_batch(const AesKeys& keys, int rounds, const void* d_wins, const int32_t* d_tile_win, int32_t total_tiles,
                                  hipStream_t st) {
  if (total_tiles <= 0) return;
  const dim3 grid((unsigned)total_tiles), block(kCsThreads);
  const PassWindowDev* wins = static_cast<const PassWindowDev*>(d_wins);
  if (rounds == 10)
    hipLaunchKernelGGL((aes_ctr_cstream_batch_kernel<10>), grid, block, 0, st, keys, wins, d_tile_win, total_tiles);
  else if (rounds == 12)
    hipLaunchKernelGGL((aes_ctr_cstream_batch_kernel<12>), grid, block, 0, st, keys, wins, d_tile_win, total_tiles);
  else
    hipLaunchKernelGGL((aes_ctr_cstream_batch_kernel<14>), grid, block, 0, st, keys, wins, d_tile_win, total_tiles);
}

}  // namespace s3s
