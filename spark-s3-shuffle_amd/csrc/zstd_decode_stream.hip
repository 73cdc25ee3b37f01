// zstd_decode_stream.hip — the device side of a resumable Zstandard stream (s3s_dstream_open_zstd, decode_stream.hip,
// DESIGN.md 6l): the unit walk over the pieces of partitions inside a window, the resumable frame decoder in its size and
// execute modes, and the cut of the unit table at the caller's output capacity.  The decoder is zstd_stream_core.h (shared
// with its host model, tests/model/zstd_stream_model.cpp); the kernels of the one-shot paths are not touched.
//
// Launch shape: one wavefront per piece of a partition (a workgroup of 64 lanes).  The control flow is uniform; literal runs
// and matches are copied 64 bytes per step, the four Huffman streams of a block go to lanes 0..3 of the same wavefront.
// LDS per workgroup: Work (tables, ring, literal window) + HufWork, booked below - eight workgroups per CU.
#define S3S_ZSTD_DEVICE 1
#include "s3s_internal.h"
#include "zstd_stream_core.h"
#include "zstd_decode_stream.h"

namespace s3s {
namespace {

using namespace s3s_zstd;

static_assert(sizeof(Work) + sizeof(HufWork) <= 20 * 1024, "LDS budget of the resumable decoder: 8 workgroups per CU");

// One lane per piece raises the window's status word: corruption (-1) wins over a refusal (-2) whatever the order.
__device__ __forceinline__ void raise_status(int32_t* status, int n) {
  if (n == -2) atomicCAS(status, 0, S3S_E_UNSUPPORTED);
  else atomicExch(status, S3S_E_BAD_FRAME);
}

// result (written for the LAST piece, the only one a window can cut): [0] = stop offset, [1] = need
__global__ void zstd_walk_kernel(const uint8_t* __restrict__ comp, const int64_t* __restrict__ piece_off, int32_t n_pieces,
                                 int32_t first_open, int64_t last_pend, int64_t wmax, int emit, const int64_t* __restrict__ unit_base,
                                 uint32_t* __restrict__ piece_units, ZUnit* __restrict__ units, uint32_t* __restrict__ dsize,
                                 int32_t* __restrict__ status, int64_t* __restrict__ result) {
  const int p = (int)(blockIdx.x * kWave + threadIdx.x);  // (launched with kWave lanes per workgroup)
  if (p >= n_pieces) return;
  const int64_t end = piece_off[p + 1];
  int64_t stop = end, need = 0;
  const int64_t b = emit ? unit_base[p] : 0;
  const int n = walk_piece(comp, piece_off[p], end, p == n_pieces - 1 ? last_pend : end, p == 0 && first_open != 0, wmax, emit != 0,
                           emit ? units + b : nullptr, emit ? dsize + b : nullptr, (int32_t)b, &stop, &need);
  if (n < 0) raise_status(status, n);
  if (!emit) {
    piece_units[p] = n < 0 ? 0u : (uint32_t)n;
    if (p == n_pieces - 1) {
      result[0] = stop;
      result[1] = need;
    }
  }
}

__global__ __launch_bounds__(kWave) void zstd_stream_kernel(ZStreamRun a) {
  __shared__ Work w;
  __shared__ HufWork h;
  const int p = blockIdx.x;
  const Lanes L{(int)threadIdx.x, kWave};
  const int64_t b0 = a.unit_base[p], b1 = a.unit_base[p + 1];
  const int32_t u0 = (int32_t)b0, u1 = (int32_t)(b1 < a.k ? b1 : a.k);
  if (u1 <= u0) return;
  ZPieceRes res;
  const int rc = run_piece(w, h, a.comp, a.units, a.dsize, a.unit_out, u0, u1, a.execute != 0, p == 0 && a.resumed != 0, a.st_in,
                           a.st_out, a.dst, a.staging, a.hist_len, a.lit + (int64_t)p * a.lit_stride, L, &res);
  if (L.lane == 0) {
    if (rc != ZS_OK) atomicExch(a.status, S3S_E_BAD_FRAME);
    if (p == 0) a.result[0] = res.resumed_out;
  }
}

// The cut at the caller's output capacity.  unit_out is the exclusive scan of the decoded sizes (n_units + 1 entries): exactly
// one index k has unit_out[k] <= dst_capacity < unit_out[k + 1], or is n_units.  result = {k, consumed, out_len, need, open,
// frame unit, Window_Size, out start}: what is open behind unit k - 1 (frame unit -1: the frame that was open at the start).
__global__ __launch_bounds__(256) void zstd_units_cut_kernel(const uint8_t* __restrict__ comp, const ZUnit* __restrict__ units,
                                                             const uint32_t* __restrict__ dsize, const int64_t* __restrict__ unit_out,
                                                             int64_t n_units, int64_t dst_capacity, int64_t stop, int32_t first_open,
                                                             int64_t* __restrict__ result) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > n_units) return;
  const int64_t o = unit_out[i];
  if (o > dst_capacity) return;
  if (i < n_units && unit_out[i + 1] <= dst_capacity) return;
  int64_t open = first_open, fu = -1, window = 0, start = 0;
  if (i > 0) {
    const ZUnit u = units[i - 1];
    const int kind = u.kind & 15;
    open = kind == ZU_FRAME || (kind >= ZU_RAW && !(u.kind & ZU_LAST)) ? 1 : 0;
    if (kind == ZU_SKIP) open = 0;
    fu = open ? u.frame_unit : -1;
    if (open && fu >= 0) {
      FrameHdr fh;
      frame_header(comp + units[fu].off, units[fu].payload, &fh);
      window = fh.window;
      start = unit_out[fu];
    }
  }
  result[0] = i;
  result[1] = i < n_units ? units[i].off : stop;
  result[2] = o;
  result[3] = i < n_units ? (int64_t)dsize[i] : 0;
  result[4] = open;
  result[5] = fu;
  result[6] = window;
  result[7] = start;
}

}  // namespace

void launch_zstd_walk(const uint8_t* d_comp, const int64_t* d_piece_off, int32_t n_pieces, int32_t first_open, int64_t last_pend,
                      int64_t wmax, bool emit, const int64_t* d_unit_base, uint32_t* d_piece_units, void* d_units, uint32_t* d_dsize,
                      int32_t* d_status, int64_t* d_result, hipStream_t st) {
  if (n_pieces <= 0) return;
  hipLaunchKernelGGL(zstd_walk_kernel, dim3((unsigned)((n_pieces + kWave - 1) / kWave)), dim3(kWave), 0, st, d_comp, d_piece_off, n_pieces, first_open,
                     last_pend, wmax, emit ? 1 : 0, d_unit_base, d_piece_units, static_cast<ZUnit*>(d_units), d_dsize, d_status, d_result);
}

void launch_zstd_stream(const ZStreamRun& run, int32_t n_pieces, hipStream_t st) {
  if (n_pieces <= 0) return;
  hipLaunchKernelGGL(zstd_stream_kernel, dim3((unsigned)n_pieces), dim3(kWave), 0, st, run);
}

void launch_zstd_units_cut(const uint8_t* d_comp, const void* d_units, const uint32_t* d_dsize, const int64_t* d_unit_out, int64_t n_units,
                           int64_t dst_capacity, int64_t stop, int32_t first_open, int64_t* d_result, hipStream_t st) {
  hipLaunchKernelGGL(zstd_units_cut_kernel, dim3((unsigned)((n_units + 256) / 256)), dim3(256), 0, st, d_comp,
                     static_cast<const ZUnit*>(d_units), d_dsize, d_unit_out, n_units, dst_capacity, stop, first_open, d_result);
}

}  // namespace s3s
