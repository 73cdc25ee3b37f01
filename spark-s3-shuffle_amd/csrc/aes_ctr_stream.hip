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
  const int64_t tile0 = s3s_aes::win_chunk_start((int64_t)blockIdx.x * kWinTileChunks, front);
  if (tile0 >= L) return;  // the whole workgroup
  const int64_t tile_end = tile0 + kWinTile < L ? tile0 + kWinTile : L;
  const LaneSbox sbox{s3s_aes::sbox_word(threadIdx.x & 63u)};
  const int32_t p_lo = s3s_aes::win_last_start_le(E, 0, n - 1, tile0), p_hi = s3s_aes::win_last_start_le(E, p_lo, n - 1, tile_end - 1);

  for (int k = 0; k < kWinChunks; k++) {
    const int64_t x0 = tile0 + 16 * ((int64_t)threadIdx.x + (int64_t)kWinThreads * k);
    const bool live = x0 < tile_end;
    const int64_t lim = x0 + 16 < tile_end ? x0 + 16 : tile_end;
    s3s_aes::WinCursor c;
    s3s_aes::win_open(c, E, s3s_aes::win_last_start_le(E, p_lo, p_hi, x0), front, x0);
    for (;;) {
      s3s_aes::WinUnit u;
      const bool has = s3s_aes::win_next(c, E, n, L, lim, live, u);
      if (__builtin_amdgcn_ballot_w64(has) == 0) break;  // wave-uniform: every lane stays for the block encryption
      const bool carried = u.part == 0 && front > 0;      // piece 0's IV came by in an earlier feed
      const bool work = has && u.len > 0;
      uint32_t ivw[4] = {iv0.w[0], iv0.w[1], iv0.w[2], iv0.w[3]};
      const uint8_t* ivp = in + (carried ? 0 : E[u.part]);
      if (work && !carried) {
        __builtin_memcpy(ivw, ivp, 16);
#pragma unroll
        for (int w = 0; w < 4; w++) ivw[w] = __builtin_bswap32(ivw[w]);
      }
      uint32_t ks[4];
      s3s_aes::keystream_block(keys.rk, NR, ivw, (uint64_t)u.block, ks, sbox);
      if (work) {
        if (u.is_iv) {  // whole (len 16): gathered for the host, dropped from the plain bytes
          uint8_t* d = iv_out + 16 * (int64_t)u.part;
          for (int i = 0; i < 16; i++) d[i] = ivp[i];
        } else {
          const uint8_t* s = in + (u.start + u.skip);
          uint8_t* d = out + (Q[u.part] - (carried ? front - 16 : 0) + u.plain);
          if (u.len == 16) {
            uint32_t v[4];
            __builtin_memcpy(v, s, 16);
#pragma unroll
            for (int w = 0; w < 4; w++) v[w] ^= __builtin_bswap32(ks[w]);
            __builtin_memcpy(d, v, 16);
          } else {
            for (int i = 0; i < u.len; i++) {
              const int b = u.skip + i;
              d[i] = (uint8_t)(s[i] ^ (ks[b >> 2] >> (24 - 8 * (b & 3))));
            }
          }
        }
      }
    }
  }
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
