// decode_stream_kernels.hip — the device side of the streaming reduce side (s3s_dstream_feed*, decode_stream.hip): frame
// discovery that treats "the window ends inside a unit" as a place to stop, the cut of the frame table at the caller's output
// capacity, and the seed step of the per-partition checksums.  The decode kernels run on the cut table unchanged.
//
// These are the one-shot discovery walks (lz4_decompress.hip, snappy_decompress.hip) and the checksum combine (checksum.hip)
// with one rule added each; they live in a file of their own so that the kernels the one-shot entry points launch stay what
// they were, instruction for instruction.  The header checks, the stream-mode walks (walk_tile_stream, walk_piece_stream: the
// batched feed's kernels, decode_stream_batch.hip, run them too) and the polynomial arithmetic are shared (discover_core.h,
// checksum_core.h).
#include "s3s_internal.h"
#include "checksum_core.h"
#include "discover_core.h"

namespace s3s {
namespace {

// resolve_chain (lz4_decompress.hip) with the stop rule and the result words.  The speculation in front of it is the one-shot
// kernel: a tile that holds the cut frame has no speculative exit, so it is re-walked here.
__global__ __launch_bounds__(kWave) void tile_resolve_stream_kernel(
    const uint8_t* __restrict__ comp, int64_t comp_len, int64_t range_left, int32_t n_tiles,
    const int64_t* __restrict__ spec_entry, int64_t* __restrict__ spec_exit, int32_t* __restrict__ spec_count,
    int64_t* __restrict__ true_entry, int32_t* __restrict__ status, int64_t* __restrict__ result) {
  const int lane = threadIdx.x;
  int64_t e = 0, need = 0;
  int k = 0;
  while (k < n_tiles) {
    const int kk = k + lane;
    bool ok = false;
    if (kk < n_tiles) {
      const int64_t want = (lane == 0) ? e : spec_exit[kk - 1];
      ok = (spec_entry[kk] == want) && spec_exit[kk] >= 0;
    }
    const uint64_t bad = ~__ballot(ok);
    const int good = bad ? __builtin_ctzll(bad) : kWave;
    if (lane < good) true_entry[k + lane] = spec_entry[k + lane];
    if (good > 0) {
      e = spec_exit[k + good - 1];
      k += good;
      continue;
    }
    const int64_t t0 = (int64_t)k * kTileBytes;
    const int64_t t1 = (t0 + kTileBytes) < comp_len ? (t0 + kTileBytes) : comp_len;
    if (e >= t1) {
      if (lane == 0) {
        true_entry[k] = -1;
        spec_count[k] = 0;
        spec_exit[k] = e;
      }
    } else {
      int32_t cnt = 0;
      const int64_t ex = walk_tile_stream(comp, comp_len, range_left, e, t1, &cnt, &need);  // uniform
      if (ex < 0) {
        if (lane == 0) atomicExch(status, S3S_E_BAD_FRAME);
        return;
      }
      if (lane == 0) {
        true_entry[k] = e;
        spec_count[k] = cnt;
        spec_exit[k] = ex;
      }
      e = ex;
      if (need > 0) {  // the chain stops in tile k: no frame starts in the tiles behind it
        for (int j = k + 1 + lane; j < n_tiles; j += kWave) {
          true_entry[j] = -1;
          spec_count[j] = 0;
        }
        break;
      }
    }
    __threadfence();
    k += 1;
  }
  if (lane == 0) {
    result[0] = e;
    result[1] = need;
  }
}

// the cut of the frame table at the caller's output capacity (launch_frames_cut, s3s_internal.h).  frame_out is the
// exclusive scan of the decoded sizes (n_frames + 1 entries, ascending, frame_out[0] = 0 <= dst_capacity): exactly one
// index k has frame_out[k] <= dst_capacity < frame_out[k + 1], or is n_frames.
__global__ __launch_bounds__(256) void frames_cut_kernel(const Frame* __restrict__ frames, const uint32_t* __restrict__ frame_orig,
                                                         const int64_t* __restrict__ frame_out, int64_t n_frames,
                                                         int64_t dst_capacity, int64_t stop, int codec,
                                                         int64_t* __restrict__ result) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > n_frames) return;
  const int64_t o = frame_out[i];
  if (o > dst_capacity) return;
  if (i < n_frames && frame_out[i + 1] <= dst_capacity) return;
  int64_t consumed = stop, need = 0;
  if (i < n_frames) {
    const Frame f = frames[i];
    // bytes of the unit in front of its payload: LZ4Block header / Snappy chunk length / LZF chunk header (stored: 5, compressed: 7)
    const int head = codec == S3S_CODEC_LZ4 ? kLz4FrameHeader : codec == S3S_CODEC_SNAPPY ? 4 : (f.method == 2 ? 7 : 5);
    consumed = f.comp_off - head;
    need = (int64_t)frame_orig[i];
  }
  result[0] = i;
  result[1] = consumed;
  result[2] = o;
  result[3] = need;
}

// result (written for the LAST piece, the only one a window can cut): [0] = stop offset, [1] = need
__global__ void snappy_count_stream_kernel(const uint8_t* __restrict__ comp, const int64_t* __restrict__ piece_off, int32_t n_pieces,
                                           int32_t first_mid, int64_t last_pend, uint32_t* __restrict__ piece_nframes,
                                           int32_t* __restrict__ status, int64_t* __restrict__ result, int chunk_format) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pieces) return;
  const int64_t end = piece_off[p + 1];
  int64_t stop = end, need = 0;
  const int n = walk_piece_stream(comp, piece_off[p], end, p == n_pieces - 1 ? last_pend : end, p == 0 && first_mid != 0, chunk_format,
                                  false, nullptr, nullptr, &stop, &need);
  if (n < 0) raise_piece_status(status, n);
  piece_nframes[p] = n < 0 ? 0u : (uint32_t)n;
  if (p == n_pieces - 1) {
    result[0] = stop;
    result[1] = need;
  }
}

__global__ void snappy_emit_stream_kernel(const uint8_t* __restrict__ comp, const int64_t* __restrict__ piece_off, int32_t n_pieces,
                                          int32_t first_mid, int64_t last_pend, const int64_t* __restrict__ frame_base,
                                          Frame* __restrict__ frames, uint32_t* __restrict__ frame_orig, int32_t* __restrict__ status,
                                          int chunk_format) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pieces) return;
  const int64_t end = piece_off[p + 1], b = frame_base[p];
  int64_t stop, need;
  const int n = walk_piece_stream(comp, piece_off[p], end, p == n_pieces - 1 ? last_pend : end, p == 0 && first_mid != 0, chunk_format,
                                  true, frames + b, frame_orig + b, &stop, &need);
  if (n < 0) raise_piece_status(status, n);
}

// A checksum continued (s3s_checksum_ranges_seeded*, the carried state of s3s_dstream_feed*): the seed is the checksum of
// the bytes in front of range p, so it enters as one more leading term of the combine -
//   CRC      crc(X || Y) = crc(X) * x^(8 |Y|) mod P  xor  crc(Y)                      (zlib crc32_combine)
//   Adler32  A = A_X + A_Y - 1,  B = B_X + B_Y + |Y| (A_X - 1)       (mod 65521)      (zlib adler32_combine)
// One lane per range, behind the combine kernel; a range of no bytes keeps its seed.
template <int ALGO>
__global__ __launch_bounds__(kWave) void checksum_seed_kernel(const int64_t* __restrict__ offsets, int32_t n,
                                                             const Tables* __restrict__ tabs, const int64_t* __restrict__ seeds,
                                                             int64_t* __restrict__ out) {
  const int p = (int)(blockIdx.x * kWave + threadIdx.x);
  if (p >= n) return;
  const uint64_t len = (uint64_t)(offsets[p + 1] - offsets[p]);
  const uint32_t seed = (uint32_t)seeds[p], own = (uint32_t)out[p];
  if (ALGO == S3S_CHECKSUM_ADLER32) {
    const uint64_t rem = len % kAdlerMod, a1 = seed & 0xffffu, b1 = seed >> 16, a2 = own & 0xffffu, b2 = own >> 16;
    const uint64_t a = (a1 + a2 + kAdlerMod - 1) % kAdlerMod;
    const uint64_t b = (rem * a1 + b1 + b2 + kAdlerMod - rem) % kAdlerMod;
    out[p] = (int64_t)(b << 16 | a);
  } else {
    out[p] = (int64_t)(uint64_t)(multmodp(x8n(tabs->x2n, len, tabs->poly), seed, tabs->poly) ^ own);
  }
}

}  // namespace

void launch_lz4_discover_stream(const uint8_t* d_comp, int64_t comp_len, int64_t range_left, int32_t n_tiles,
                                int64_t* d_spec_entry, int64_t* d_spec_exit, int32_t* d_spec_count, int64_t* d_true_entry,
                                int64_t* d_frame_base, int32_t* d_status, int64_t* d_result, hipStream_t st) {
  if (n_tiles <= 0) return;
  launch_lz4_speculate(d_comp, comp_len, n_tiles, d_spec_entry, d_spec_exit, d_spec_count, st);
  hipLaunchKernelGGL(tile_resolve_stream_kernel, dim3(1), dim3(kWave), 0, st, d_comp, comp_len, range_left, n_tiles, d_spec_entry,
                     d_spec_exit, d_spec_count, d_true_entry, d_status, d_result);
  launch_scan_u32(reinterpret_cast<const uint32_t*>(d_spec_count), (int64_t)n_tiles, d_frame_base, st);
}

void launch_frames_cut(int codec, const Frame* d_frames, const uint32_t* d_frame_orig, const int64_t* d_frame_out, int64_t n_frames,
                       int64_t dst_capacity, int64_t stop, int64_t* d_result, hipStream_t st) {
  hipLaunchKernelGGL(frames_cut_kernel, dim3((unsigned)((n_frames + 256) / 256)), dim3(256), 0, st, d_frames, d_frame_orig,
                     d_frame_out, n_frames, dst_capacity, stop, codec, d_result);
}

void launch_snappy_count_frames_stream(const uint8_t* d_comp, const int64_t* d_piece_off, int32_t n_pieces, int32_t first_mid,
                                       int64_t last_pend, uint32_t* d_piece_nframes, int32_t* d_status, int64_t* d_result,
                                       hipStream_t st, int chunk_format) {
  if (n_pieces <= 0) return;
  hipLaunchKernelGGL(snappy_count_stream_kernel, dim3((unsigned)((n_pieces + 63) / 64)), dim3(64), 0, st, d_comp, d_piece_off,
                     n_pieces, first_mid, last_pend, d_piece_nframes, d_status, d_result, chunk_format);
}

void launch_snappy_emit_frames_stream(const uint8_t* d_comp, const int64_t* d_piece_off, int32_t n_pieces, int32_t first_mid,
                                      int64_t last_pend, const int64_t* d_frame_base, Frame* d_frames, uint32_t* d_frame_orig,
                                      int32_t* d_status, hipStream_t st, int chunk_format) {
  if (n_pieces <= 0) return;
  hipLaunchKernelGGL(snappy_emit_stream_kernel, dim3((unsigned)((n_pieces + 63) / 64)), dim3(64), 0, st, d_comp, d_piece_off,
                     n_pieces, first_mid, last_pend, d_frame_base, d_frames, d_frame_orig, d_status, chunk_format);
}

void launch_checksum_seed(int algo, const int64_t* d_offsets, int32_t n, const void* d_tables, const int64_t* d_seeds,
                          int64_t* d_out, hipStream_t st) {
  if (n <= 0) return;
  const Tables* tabs = static_cast<const Tables*>(d_tables) + (algo == S3S_CHECKSUM_CRC32C ? 1 : 0);
  const dim3 grid((unsigned)((n + kWave - 1) / kWave));
  if (algo == S3S_CHECKSUM_ADLER32)
    hipLaunchKernelGGL(checksum_seed_kernel<S3S_CHECKSUM_ADLER32>, grid, dim3(kWave), 0, st, d_offsets, n, tabs, d_seeds, d_out);
  else
    hipLaunchKernelGGL(checksum_seed_kernel<S3S_CHECKSUM_CRC32>, grid, dim3(kWave), 0, st, d_offsets, n, tabs, d_seeds, d_out);
}

}  // namespace s3s
