// aes_ctr_cstream.hip — the AES-CTR pass of the streaming map side under IO encryption (s3s_cstream_open_encrypted,
// compress_stream.hip): the output of ONE feed -> IV | cipher text, behind a cut that only the device knows.
//
// aes_ctr.hip's map-side modes start at partition starts and know the image's length on the host.  A feed's output starts in
// the middle of the open partition - `front` stored bytes of it were written by earlier feeds, its key stream stands at any
// residue of a block, its IV travels in entry 0 of the feed's IV array - and ends where cstream_cut_kernel cut the plan at the
// caller's capacity: the host launches this kernel without having seen out_len.  The geometry is the window form's
// (aes_ctr_stream_core.h, used as it is): the feed's output is the window, E the n + 1 piece offsets the cut kernel clamped
// (pieces behind the cut have length 0), chunks follow piece 0's key stream.  Two modes:
//   kCsInPlace    behind a codec: the cut gather left a 16-byte hole in front of every partition that starts in the output
//                 (kItemIv); the hole gets the IV, the bytes behind it are XORed where they lie.  out_len is read from the cut
//                 kernel's result words; the grid is sized from a host bound and workgroups at or beyond out_len return whole
//   kCsFromPlain  codec NONE: source window -> IV | cipher text, in one pass (the host knows the cut: none_cut_encrypted)
// Nothing at or beyond out_len is read-modified or written: the contract promises untouched bytes there.
//
// The rest is aes_ctr.hip's: tiles of kCsTile stored bytes per workgroup, no LDS booked (the S-box is one register across the
// wavefront, read with ds_bpermute), all 64 lanes in every block encryption with a wave-uniform ballot as the loop's exit and
// only the loads and stores predicated, the round keys kernel arguments, every offset and block number 64-bit.  A kernel of
// its own, not a mode of aes_ctr_kernel or aes_ctr_window_kernel: the one-shot and reduce-side kernels keep their instructions.
// The tile body is aes_ctr_cstream_tile.inc, the text the batched feed's kernel (aes_ctr_cstream_batch.hip) includes too.
#define S3S_AES_DEVICE
#include "aes_ctr_stream_core.h"
#include "compress_stream_core.h"
#include "s3s_internal.h"

namespace s3s {
namespace {

constexpr int kCsThreads = 256;
constexpr int kCsChunks = 4;                               // chunks of 16 stored bytes per thread
constexpr int kCsTileChunks = kCsThreads * kCsChunks;      // chunks per workgroup
constexpr int kCsTile = 16 * kCsTileChunks;                // stored bytes per workgroup

struct LaneSbox {
  uint32_t word;  // S-box bytes 4 lane .. 4 lane + 3
  __device__ __forceinline__ uint32_t operator()(uint32_t x) const {
    const uint32_t w = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(x & 0xfcu), (int)word);  // lane x / 4
    return (w >> ((x & 3u) * 8u)) & 0xffu;
  }
};

template <int NR, int MODE>
__global__ __launch_bounds__(kCsThreads) void aes_ctr_cstream_kernel(const AesKeys keys, const uint8_t* __restrict__ src, uint8_t* out,
                                                                    const int64_t* __restrict__ E, const int64_t* __restrict__ Q,
                                                                    const uint8_t* __restrict__ ivs, const int64_t* __restrict__ cut,
                                                                    int32_t n, int64_t front, int64_t host_len) {
  const int64_t L = MODE == kCsInPlace ? cut[s3s_cs::kCutOutLen] : host_len;
#define S3S_CS_TILE blockIdx.x
#include "aes_ctr_cstream_tile.inc"
#undef S3S_CS_TILE
}

template <int NR>
void launch_mode(int mode, unsigned grid, hipStream_t st, const AesKeys& keys, const uint8_t* src, uint8_t* out, const int64_t* E,
                 const int64_t* Q, const uint8_t* ivs, const int64_t* cut, int32_t n, int64_t front, int64_t host_len) {
  if (mode == kCsInPlace)
    hipLaunchKernelGGL((aes_ctr_cstream_kernel<NR, kCsInPlace>), dim3(grid), dim3(kCsThreads), 0, st, keys, src, out, E, Q, ivs, cut, n, front, host_len);
  else
    hipLaunchKernelGGL((aes_ctr_cstream_kernel<NR, kCsFromPlain>), dim3(grid), dim3(kCsThreads), 0, st, keys, src, out, E, Q, ivs, cut, n, front, host_len);
}

}  // namespace

void launch_aes_ctr_cstream(int mode, const AesKeys& keys, int rounds, const uint8_t* d_src, uint8_t* d_dst, const int64_t* d_piece_off,
                            const int64_t* d_plain_off, const uint8_t* d_ivs, const int64_t* d_cut, int32_t n_pieces, int64_t front,
                            int64_t out_bound, hipStream_t st) {
  if (n_pieces <= 0 || out_bound <= 0) return;
  const int64_t chunks = s3s_aes::win_chunk_count(out_bound, front);
  const unsigned grid = (unsigned)((chunks + kCsTileChunks - 1) / kCsTileChunks);
  if (rounds == 10) launch_mode<10>(mode, grid, st, keys, d_src, d_dst, d_piece_off, d_plain_off, d_ivs, d_cut, n_pieces, front, out_bound);
  else if (rounds == 12) launch_mode<12>(mode, grid, st, keys, d_src, d_dst, d_piece_off, d_plain_off, d_ivs, d_cut, n_pieces, front, out_bound);
  else launch_mode<14>(mode, grid, st, keys, d_src, d_dst, d_piece_off, d_plain_off, d_ivs, d_cut, n_pieces, front, out_bound);
}

}  // namespace s3s
