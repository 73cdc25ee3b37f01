// decode_stream_batch.hip — the device side of the batched feed (s3s_dstream_feed_batch*, decode_stream.hip): one window of
// each of several streams per call.  Every kernel here is a kernel of the single feed (decode_stream_kernels.hip) or of the
// batched one-shot call (lz4_decompress.hip, decode_api.hip) with the window found through a descriptor: an LzRange (the
// window's bytes, its discovery workspace, its status word, its frame table) and a StreamWin (what a window has beyond a
// range).  They live in a file of their own so that the kernels the single feed and the one-shot calls launch stay what they
// are, instruction for instruction; the walks and the arithmetic are shared (discover_core.h, checksum_core.h).
//
// Result words of a window (LzRange::result, kWinWords of them): [0] stop offset, [1] need, [2] frames in front of the stop
// (phase 1); [4] k, [5] consumed, [6] out_len, [7] decoded bytes of frame k (phase 2, the cut).
//
// No kernel reads a byte at or beyond its window's comp_len: the walks are the single feed's, the speculation is the one-shot
// kernel's (it tests comp_len - p >= 21 before every load).  No kernel but the decoders writes to a destination.
#include "s3s_internal.h"
#include "checksum_core.h"
#include "discover_core.h"

namespace s3s {
namespace {

// tile_resolve_stream_kernel, one wavefront per window, with the scan of the tile counts behind it (as
// tile_resolve_batch_kernel does for the one-shot batch).  The speculation in front of it is tile_speculate_batch_kernel.
__global__ __launch_bounds__(kWave) void tile_resolve_stream_batch_kernel(const LzRange* __restrict__ ranges,
                                                                         const StreamWin* __restrict__ wins, int32_t n_wins) {
  const int wi = blockIdx.x;
  if (wi >= n_wins) return;
  const LzRange r = ranges[wi];
  const int64_t range_left = wins[wi].range_left;
  const int lane = threadIdx.x;
  const uint8_t* __restrict__ comp = r.comp;
  const int64_t comp_len = r.comp_len;
  const int32_t n_tiles = r.n_tiles;
  int64_t e = 0, need = 0;
  int k = 0;
  while (k < n_tiles) {
    const int kk = k + lane;
    bool ok = false;
    if (kk < n_tiles) {
      const int64_t want = (lane == 0) ? e : r.spec_exit[kk - 1];
      ok = (r.spec_entry[kk] == want) && r.spec_exit[kk] >= 0;
    }
    const uint64_t bad = ~__ballot(ok);
    const int good = bad ? __builtin_ctzll(bad) : kWave;
    if (lane < good) r.true_entry[k + lane] = r.spec_entry[k + lane];
    if (good > 0) {
      e = r.spec_exit[k + good - 1];
      k += good;
      continue;
    }
    const int64_t t0 = (int64_t)k * kTileBytes;
    const int64_t t1 = (t0 + kTileBytes) < comp_len ? (t0 + kTileBytes) : comp_len;
    if (e >= t1) {
      if (lane == 0) {
        r.true_entry[k] = -1;
        r.spec_count[k] = 0;
        r.spec_exit[k] = e;
      }
    } else {
      int32_t cnt = 0;
      const int64_t ex = walk_tile_stream(comp, comp_len, range_left, e, t1, &cnt, &need);  // uniform
      if (ex < 0) {
        if (lane == 0) atomicExch(r.status, S3S_E_BAD_FRAME);
        return;
      }
      if (lane == 0) {
        r.true_entry[k] = e;
        r.spec_count[k] = cnt;
        r.spec_exit[k] = ex;
      }
      e = ex;
      if (need > 0) {  // the chain stops in tile k: no frame starts in the tiles behind it
        for (int j = k + 1 + lane; j < n_tiles; j += kWave) {
          r.true_entry[j] = -1;
          r.spec_count[j] = 0;
        }
        break;
      }
    }
    __threadfence();
    k += 1;
  }
  __threadfence();
  scan_u32_wave(reinterpret_cast<const uint32_t*>(r.spec_count), (int64_t)n_tiles, r.frame_base, lane);
  __threadfence();
  if (lane == 0) {
    r.result[0] = e;
    r.result[1] = need;
    r.result[2] = __builtin_nontemporal_load(&r.frame_base[n_tiles]);
  }
}

// raise_piece_status for a status word that is reached through a descriptor: the pointer is loaded from memory, so the compiler
// has to be told that it names global memory (the kernels of the single feed get theirs as a kernel argument).  The rule is
// the same: corruption (-1) is S3S_E_BAD_FRAME whatever the window's other pieces say, a refused claim (-2) is written only
// over "no error".
__device__ __forceinline__ void raise_window_status(int32_t* status, int n) {
  auto* g = (__attribute__((address_space(1))) int32_t*)status;
  if (n == -2) {
    int32_t none = 0;
    __hip_atomic_compare_exchange_strong(g, &none, (int32_t)S3S_E_UNSUPPORTED, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    __hip_atomic_exchange(g, (int32_t)S3S_E_BAD_FRAME, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// snappy_count_stream_kernel / snappy_emit_stream_kernel over the pieces of ALL windows: one lane per piece, the window through
// piece_win.  A window owns n_pieces + 1 consecutive offsets, so its offsets start at first_piece + its index.  The counts go
// to the window's spec_count, the status word and the result words are the window's own - the rule of raise_piece_status holds
// per window.
template <bool EMIT>
__global__ __launch_bounds__(kWave) void snappy_walk_stream_batch_kernel(const LzRange* __restrict__ ranges,
                                                                        const StreamWin* __restrict__ wins,
                                                                        const int64_t* __restrict__ piece_off,
                                                                        const int32_t* __restrict__ piece_win, int32_t total_pieces,
                                                                        int chunk_format) {
  const int g = blockIdx.x * kWave + threadIdx.x;
  if (g >= total_pieces) return;
  const int wi = piece_win[g];
  const LzRange r = ranges[wi];
  const StreamWin x = wins[wi];
  const int p = g - x.first_piece;
  if (p < 0 || p >= x.n_pieces) return;
  if (EMIT && (r.skip || r.n_frames <= 0)) return;
  const int64_t* off = piece_off + x.first_piece + wi;
  const int64_t end = off[p + 1];
  int64_t stop = end, need = 0;
  const int64_t b = EMIT ? r.frame_base[p] : 0;
  const int n = walk_piece_stream(r.comp, off[p], end, p == x.n_pieces - 1 ? x.last_pend : end, p == 0 && x.first_mid != 0, chunk_format,
                                  EMIT, EMIT ? r.frames + b : nullptr, EMIT ? r.frame_orig + b : nullptr, &stop, &need);
  if (n < 0) raise_window_status(r.status, n);
  if (!EMIT) {
    r.spec_count[p] = n < 0 ? 0 : n;
    if (p == x.n_pieces - 1) {
      r.result[0] = stop;
      r.result[1] = need;
    }
  }
}

// the scan of a window's piece counts: frame_base[n_pieces + 1], result[2] = its frames
__global__ __launch_bounds__(kWave) void piece_scan_batch_kernel(const LzRange* __restrict__ ranges, const StreamWin* __restrict__ wins,
                                                                int32_t n_wins) {
  const int wi = blockIdx.x;
  if (wi >= n_wins) return;
  const LzRange r = ranges[wi];
  const int32_t n = wins[wi].n_pieces;
  scan_u32_wave(reinterpret_cast<const uint32_t*>(r.spec_count), (int64_t)n, r.frame_base, threadIdx.x);
  __threadfence();
  if (threadIdx.x == 0) r.result[2] = __builtin_nontemporal_load(&r.frame_base[n]);
}

// frames_cut_kernel per window, behind the scan of the window's decoded sizes: one wavefront per window, kCutWaves windows per
// workgroup.  Exactly one index k of a window has frame_out[k] <= dst_capacity < frame_out[k + 1], or is n_frames.
constexpr int kCutWaves = 4;
__global__ __launch_bounds__(kCutWaves* kWave) void frames_cut_batch_kernel(const LzRange* __restrict__ ranges,
                                                                           const StreamWin* __restrict__ wins, int32_t n_wins,
                                                                           int codec) {
  const int wi = blockIdx.x * kCutWaves + (int)(threadIdx.x / kWave);
  const int lane = threadIdx.x % kWave;
  if (wi >= n_wins) return;
  const LzRange r = ranges[wi];
  if (r.skip || r.n_frames <= 0) return;
  const int64_t n = r.n_frames, cap = r.dst_capacity;
  scan_u32_wave(r.frame_orig, n, r.frame_out, lane);
  __threadfence();
  for (int64_t i = lane; i <= n; i += kWave) {
    const int64_t o = __builtin_nontemporal_load(&r.frame_out[i]);
    if (o > cap) break;  // ascending: nothing behind it fits either
    if (i < n && __builtin_nontemporal_load(&r.frame_out[i + 1]) <= cap) continue;
    int64_t consumed = wins[wi].stop, need = 0;
    if (i < n) {
      const Frame f = r.frames[i];
      // bytes of the unit in front of its payload: LZ4Block header / Snappy chunk length / LZF chunk header (stored: 5, compressed: 7)
      const int head = codec == S3S_CODEC_LZ4 ? kLz4FrameHeader : codec == S3S_CODEC_SNAPPY ? 4 : (f.method == 2 ? 7 : 5);
      consumed = f.comp_off - head;
      need = (int64_t)r.frame_orig[i];
    }
    r.result[4] = i;
    r.result[5] = consumed;
    r.result[6] = o;
    r.result[7] = need;
  }
}

// rebase_frames_kernel / LzRange::out_abs with the cut: payload offsets and output offsets of the frames in front of a
// window's k become absolute addresses; the frames at or behind k, and every frame of a window that left the batch (skip),
// become empty.  One lane per frame of the batch-wide table, the window by a search over first_frame.
__global__ __launch_bounds__(256) void frames_rebase_cut_kernel(const LzRange* __restrict__ ranges, const StreamWin* __restrict__ wins,
                                                                int32_t n_wins, int64_t total_frames) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total_frames) return;
  int lo = 0, hi = n_wins;  // the last window with first_frame <= i (a window of no frames shares its first_frame with the next)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (wins[mid].first_frame <= i) lo = mid; else hi = mid;
  }
  const LzRange r = ranges[lo];
  const int64_t j = i - wins[lo].first_frame;
  if (j >= r.n_frames) return;  // (cannot happen: the table is dense)
  const int64_t k = r.skip ? 0 : r.result[4];
  if (j >= k) {
    r.frames[j] = Frame{0, 0, 0, 0u, 0x10};
    r.out_abs[j] = r.dst_base;
    return;
  }
  r.frames[j].comp_off += (int64_t)reinterpret_cast<uintptr_t>(r.comp);
  r.out_abs[j] = r.frame_out[j] + r.dst_base;
}

// checksum_seed_kernel over the flattened piece table: one lane per piece, the piece's length from its window's offsets
template <int ALGO>
__global__ __launch_bounds__(kWave) void checksum_seed_batch_kernel(const int64_t* __restrict__ offsets, const int32_t* __restrict__ piece_win,
                                                                   int32_t total_pieces, const Tables* __restrict__ tabs,
                                                                   const int64_t* __restrict__ seeds, int64_t* __restrict__ out) {
  const int g = (int)(blockIdx.x * kWave + threadIdx.x);
  if (g >= total_pieces) return;
  const int64_t* o = offsets + g + piece_win[g];
  out[g] = checksum_continue<ALGO>(tabs, (uint64_t)(o[1] - o[0]), (uint32_t)seeds[g], (uint32_t)out[g]);
}

}  // namespace

void launch_lz4_resolve_stream_batch(const LzRange* d_ranges, const StreamWin* d_wins, int32_t n_wins, hipStream_t st) {
  if (n_wins <= 0) return;
  hipLaunchKernelGGL(tile_resolve_stream_batch_kernel, dim3((unsigned)n_wins), dim3(kWave), 0, st, d_ranges, d_wins, n_wins);
}

void launch_snappy_count_stream_batch(const LzRange* d_ranges, const StreamWin* d_wins, int32_t n_wins, const int64_t* d_piece_off,
                                      const int32_t* d_piece_win, int32_t total_pieces, int chunk_format, hipStream_t st) {
  if (n_wins <= 0 || total_pieces <= 0) return;
  hipLaunchKernelGGL(snappy_walk_stream_batch_kernel<false>, dim3((unsigned)((total_pieces + kWave - 1) / kWave)), dim3(kWave), 0, st,
                     d_ranges, d_wins, d_piece_off, d_piece_win, total_pieces, chunk_format);
  hipLaunchKernelGGL(piece_scan_batch_kernel, dim3((unsigned)n_wins), dim3(kWave), 0, st, d_ranges, d_wins, n_wins);
}

void launch_snappy_emit_stream_batch(const LzRange* d_ranges, const StreamWin* d_wins, int32_t n_wins, const int64_t* d_piece_off,
                                     const int32_t* d_piece_win, int32_t total_pieces, int chunk_format, hipStream_t st) {
  if (n_wins <= 0 || total_pieces <= 0) return;
  hipLaunchKernelGGL(snappy_walk_stream_batch_kernel<true>, dim3((unsigned)((total_pieces + kWave - 1) / kWave)), dim3(kWave), 0, st,
                     d_ranges, d_wins, d_piece_off, d_piece_win, total_pieces, chunk_format);
}

void launch_frames_cut_batch(int codec, const LzRange* d_ranges, const StreamWin* d_wins, int32_t n_wins, hipStream_t st) {
  if (n_wins <= 0) return;
  hipLaunchKernelGGL(frames_cut_batch_kernel, dim3((unsigned)((n_wins + kCutWaves - 1) / kCutWaves)), dim3(kCutWaves * kWave), 0, st,
                     d_ranges, d_wins, n_wins, codec);
}

void launch_frames_rebase_cut(const LzRange* d_ranges, const StreamWin* d_wins, int32_t n_wins, int64_t total_frames, hipStream_t st) {
  if (n_wins <= 0 || total_frames <= 0) return;
  hipLaunchKernelGGL(frames_rebase_cut_kernel, dim3((unsigned)((total_frames + 255) / 256)), dim3(256), 0, st, d_ranges, d_wins, n_wins,
                     total_frames);
}

void launch_checksum_seed_batch(int algo, const int64_t* d_offsets, const int32_t* d_piece_win, int32_t total_pieces,
                                const void* d_tables, const int64_t* d_seeds, int64_t* d_out, hipStream_t st) {
  if (total_pieces <= 0) return;
  const Tables* tabs = static_cast<const Tables*>(d_tables) + (algo == S3S_CHECKSUM_CRC32C ? 1 : 0);
  const dim3 grid((unsigned)((total_pieces + kWave - 1) / kWave));
  if (algo == S3S_CHECKSUM_ADLER32)
    hipLaunchKernelGGL(checksum_seed_batch_kernel<S3S_CHECKSUM_ADLER32>, grid, dim3(kWave), 0, st, d_offsets, d_piece_win, total_pieces,
                       tabs, d_seeds, d_out);
  else
    hipLaunchKernelGGL(checksum_seed_batch_kernel<S3S_CHECKSUM_CRC32>, grid, dim3(kWave), 0, st, d_offsets, d_piece_win, total_pieces,
                       tabs, d_seeds, d_out);
}

}  // namespace s3s
