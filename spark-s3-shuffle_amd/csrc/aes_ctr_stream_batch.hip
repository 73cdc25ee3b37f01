// aes_ctr_stream_batch.hip — the window form of the AES-CTR pass (aes_ctr_stream.hip) over the windows of ALL entries of a
// batched feed (s3s_dstream_feed_batch*, decode_stream.hip): one launch decrypts every window into its plain
// buffer and gathers its IVs.  Work split, S-box, block encryption and predication are the single kernel's - the tile body is
// the same text (aes_ctr_window_tile.inc) - and what a window is comes from an AesWindow descriptor in the call's
// arena instead of kernel arguments.  A file of its own: the single kernel keeps the instructions it had.
#define S3S_AES_DEVICE
#include "aes_ctr_stream_core.h"
#include "s3s_internal.h"

namespace s3s {
namespace {

constexpr int kWinThreads = 256;
constexpr int kWinChunks = 4;                                  // as in aes_ctr_stream.hip: chunks of 16 stored bytes per thread,
constexpr int kWinTileChunks = kWinThreads * kWinChunks;       // chunks per workgroup,
constexpr int kWinTile = 16 * kWinTileChunks;                  // stored bytes per workgroup

struct LaneSbox {
  uint32_t word;  // S-box bytes 4 lane .. 4 lane + 3
  __device__ __forceinline__ uint32_t operator()(uint32_t x) const {
    const uint32_t w = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(x & 0xfcu), (int)word);  // lane x / 4
    return (w >> ((x & 3u) * 8u)) & 0xffu;
  }
};

// AesWindow as the kernel reads it: a pointer read from a descriptor names global memory, and saying so in its type keeps every
// access through it a global one (the single kernel's pointers are kernel arguments, which the compiler knows to be global)
#define S3S_GLOBAL __attribute__((address_space(1)))
struct AesWindowDev {
  const S3S_GLOBAL uint8_t* in;
  S3S_GLOBAL uint8_t* out;
  const S3S_GLOBAL int64_t* E;
  const S3S_GLOBAL int64_t* Q;
  S3S_GLOBAL uint8_t* iv_out;
  int32_t m, tile0;
  int64_t front, L;
  AesWindowIv iv;
};
static_assert(sizeof(AesWindowDev) == sizeof(AesWindow) && alignof(AesWindowDev) == alignof(AesWindow), "one layout");

// The windows of all entries of a batched feed in one launch (s3s_dstream_feed_batch*, decode_stream.hip).  The grid is the sum
// of the windows' tile counts; a workgroup finds its window through the tile -> window map, once, as tile_speculate_batch_kernel
// does (blockIdx is uniform: the descriptor arrives in scalar registers), and is then a workgroup of the single kernel on tile
// blockIdx.x - tile0 of that window.  A window without a plain piece or a stored byte owns no tile.  The carried IVs travel in the
// descriptors - they are stored in the clear in the stream; the round keys stay kernel arguments.
template <int NR>
__global__ __launch_bounds__(kWinThreads) void aes_ctr_window_batch_kernel(const AesKeys keys, const AesWindowDev* __restrict__ wins,
                                                                           const int32_t* __restrict__ tile_win, int32_t total_tiles) {
  if ((int32_t)blockIdx.x >= total_tiles) return;
  const AesWindowDev w = wins[tile_win[blockIdx.x]];
  const AesWindowIv iv0 = w.iv;
  const uint8_t* __restrict__ in = (const uint8_t*)w.in;
  uint8_t* __restrict__ out = (uint8_t*)w.out;
  const int64_t* __restrict__ E = (const int64_t*)w.E;
  const int64_t* __restrict__ Q = (const int64_t*)w.Q;
  uint8_t* __restrict__ iv_out = (uint8_t*)w.iv_out;
  const int32_t n = w.m;
  const int64_t front = w.front, L = w.L;
#define S3S_WIN_TILE (blockIdx.x - (uint32_t)w.tile0)
#include "aes_ctr_window_tile.inc"
#undef S3S_WIN_TILE
}

}  // namespace

int32_t aes_ctr_window_tiles(int32_t n_pieces, int64_t front, int64_t window_len) {
  if (n_pieces <= 0 || window_len <= 0) return 0;
  return (int32_t)((s3s_aes::win_chunk_count(window_len, front) + kWinTileChunks - 1) / kWinTileChunks);
}

void launch_aes_ctr_window_batch(const AesKeys& keys, int rounds, const AesWindow* d_wins, const int32_t* d_tile_win, int32_t total_tiles,
                                 hipStream_t st) {
  if (total_tiles <= 0) return;
  const dim3 grid((unsigned)total_tiles), block(kWinThreads);
  if (rounds == 10)
    hipLaunchKernelGGL((aes_ctr_window_batch_kernel<10>), grid, block, 0, st, keys, reinterpret_cast<const AesWindowDev*>(d_wins), d_tile_win, total_tiles);
  else if (rounds == 12)
    hipLaunchKernelGGL((aes_ctr_window_batch_kernel<12>), grid, block, 0, st, keys, reinterpret_cast<const AesWindowDev*>(d_wins), d_tile_win, total_tiles);
  else
    hipLaunchKernelGGL((aes_ctr_window_batch_kernel<14>), grid, block, 0, st, keys, reinterpret_cast<const AesWindowDev*>(d_wins), d_tile_win, total_tiles);
}

}  // namespace s3s
