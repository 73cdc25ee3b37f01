// aes_ctr_stream.hip — the window form of the AES-CTR pass: the stored bytes of one window of a streamed range -> its plain
// bytes in the workspace, IVs dropped (s3s_dstream_open_encrypted, decode_stream.hip).
//
// aes_ctr.hip's kCtrDecrypt starts at partition starts and reads every IV from the stream.  A window starts in the middle of
// a partition - its IV came by in an earlier feed and is an argument here, its key stream stands at any residue of a block -
// and ends anywhere, inside an IV too.  Which units a 16-byte chunk owns is aes_ctr_stream_core.h (the host tests hold it
// against keystream(offset, len)); this file is the same work split, S-box and block encryption as aes_ctr.hip around it:
// tiles of kWinTile stored bytes per workgroup, no LDS booked (the S-box is one register across the wavefront, read with
// ds_bpermute), all 64 lanes in every block encryption with only the loads and stores predicated, the round keys kernel
// arguments, every offset and block number 64-bit.  A kernel of its own, not a fourth mode of aes_ctr_kernel: the one-shot
// entry points keep the instructions they had.
//
// The IVs that start (whole) in the window are gathered into d_iv_out[16 p ..]: the host copies them with the feed's first
// wait and keeps the one of the partition the feed leaves open.
//
// The kernel's body is aes_ctr_window_tile.inc: aes_ctr_stream_batch.hip runs the same statements over the windows of a batched
// feed, in a translation unit of its own.
#define S3S_AES_DEVICE
#include "aes_ctr_stream_core.h"
#include "s3s_internal.h"

namespace s3s {
namespace {

constexpr int kWinThreads = 256;
constexpr int kWinChunks = 4;                                  // chunks of 16 stored bytes per thread
constexpr int kWinTileChunks = kWinThreads * kWinChunks;       // chunks per workgroup
constexpr int kWinTile = 16 * kWinTileChunks;                  // stored bytes per workgroup

struct LaneSbox {
  uint32_t word;  // S-box bytes 4 lane .. 4 lane + 3
  __device__ __forceinline__ uint32_t operator()(uint32_t x) const {
    const uint32_t w = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(x & 0xfcu), (int)word);  // lane x / 4
    return (w >> ((x & 3u) * 8u)) & 0xffu;
  }
};

template <int NR>
__global__ __launch_bounds__(kWinThreads) void aes_ctr_window_kernel(const AesKeys keys, const AesWindowIv iv0, const uint8_t* __restrict__ in,
                                                                     uint8_t* __restrict__ out, const int64_t* __restrict__ E,
                                                                     const int64_t* __restrict__ Q, uint8_t* __restrict__ iv_out, int32_t n,
                                                                     int64_t front, int64_t L) {
#define S3S_WIN_TILE blockIdx.x
#include "aes_ctr_window_tile.inc"
#undef S3S_WIN_TILE
}

}  // namespace

void launch_aes_ctr_window(const AesKeys& keys, int rounds, const AesWindowIv& iv0, const uint8_t* d_in, uint8_t* d_out,
                           const int64_t* d_stored_off, const int64_t* d_plain_off, uint8_t* d_iv_out, int32_t n_pieces, int64_t front,
                           int64_t window_len, hipStream_t st) {
  if (n_pieces <= 0 || window_len <= 0) return;
  const int64_t chunks = s3s_aes::win_chunk_count(window_len, front);
  const dim3 grid((unsigned)((chunks + kWinTileChunks - 1) / kWinTileChunks)), block(kWinThreads);
  if (rounds == 10)
    hipLaunchKernelGGL((aes_ctr_window_kernel<10>), grid, block, 0, st, keys, iv0, d_in, d_out, d_stored_off, d_plain_off, d_iv_out, n_pieces, front, window_len);
  else if (rounds == 12)
    hipLaunchKernelGGL((aes_ctr_window_kernel<12>), grid, block, 0, st, keys, iv0, d_in, d_out, d_stored_off, d_plain_off, d_iv_out, n_pieces, front, window_len);
  else
    hipLaunchKernelGGL((aes_ctr_window_kernel<14>), grid, block, 0, st, keys, iv0, d_in, d_out, d_stored_off, d_plain_off, d_iv_out, n_pieces, front, window_len);
}

}  // namespace s3s
