// compress_stream_kernels.hip — the device side of the streaming map side (s3s_cstream_feed*, compress_stream.hip) that the
// one-shot call does not have: the cut of a window's plan at the caller's output capacity.  The codec kernels, the scan and
// the checksums run unchanged; the gather that reads the cut from device memory shares gather_item_body with
// gather_items_kernel (assemble_gather.h).
#include "s3s_internal.h"
#include "compress_stream_core.h"

namespace s3s {
namespace {

using s3s_cs::Mark;

#include "assemble_gather.h"

// item_off is the scan of the item sizes (n_items + 1 entries, ascending).  The feed takes the items [0, k): k - 1 is the
// largest index that ends a unit (marks[].last) and whose end offset item_off[k] is at most dst_capacity.
// ONE wavefront and NO LDS, for the reason scan_items_body gives (assemble.hip): the codec kernels of other contexts book every
// CU's LDS, and a workgroup that asks for any waits for one of their chunks.  256 items per step, 4 per lane, like that scan;
// the wave-wide maximum is five cross-lane steps at the end.  Every store is a per-lane vector store.
//   result[kCut*]                 k, consumed, out_len, need_dst, parts_closed
//   piece_off[n_pieces + 1]       where the pieces of partitions start in the output, clamped to out_len: the checksum ranges
//   lengths[n_pieces - 1]         image length of every partition the feed closes (open_img added to the first), else 0
__global__ __launch_bounds__(kWave) void cstream_cut_kernel(
    const Mark* __restrict__ marks, const int64_t* __restrict__ item_off, int32_t n_items, const int32_t* __restrict__ part_first,
    int32_t n_pieces, int64_t dst_capacity, int32_t first_last, int32_t ends0, int64_t open_img, int64_t* __restrict__ result,
    int64_t* __restrict__ piece_off, int64_t* __restrict__ lengths) {
  const int lane = threadIdx.x;
  int32_t best = -1;
  for (int32_t tile = 0; tile < n_items; tile += 4 * kWave) {
    if (item_off[tile] > dst_capacity) break;  // uniform: nothing behind this tile fits
    const int32_t i0 = tile + 4 * lane;
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (i0 + k < n_items && s3s_cs::cut_lane(marks[i0 + k], item_off[i0 + k + 1], dst_capacity)) best = i0 + k;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int32_t y = __shfl_xor(best, d);
    best = y > best ? y : best;
  }
  const int32_t k = best + 1;
  const int64_t out_len = item_off[k];
  const int32_t closed = best >= 0 ? marks[best].ends_after : ends0;
  if (lane == 0) {
    result[s3s_cs::kCutK] = k;
    result[s3s_cs::kCutConsumed] = best >= 0 ? marks[best].src_end : 0;
    result[s3s_cs::kCutOutLen] = out_len;
    result[s3s_cs::kCutNeedDst] = best < 0 && first_last >= 0 && ends0 == 0 ? item_off[first_last + 1] : 0;
    result[s3s_cs::kCutPartsClosed] = closed;
  }
  for (int32_t p = lane; p <= n_pieces; p += kWave) {
    const int64_t a = item_off[part_first[p]];
    const int64_t lo = a < out_len ? a : out_len;
    piece_off[p] = lo;
    if (p < n_pieces - 1) {
      const int64_t b = item_off[part_first[p + 1]];
      lengths[p] = p < closed ? (b < out_len ? b : out_len) - lo + (p == 0 ? open_img : 0) : 0;
    }
  }
}

// the streaming map side (compress_stream.hip): the items [0, cut[0]) of a window's plan, where cut[0] is what the cut kernel
// left in device memory - the host does not wait between the cut and this launch, so the grid covers every item of the plan
__global__ __launch_bounds__(kGatherThreads) void gather_items_cut_kernel(
    const uint8_t* __restrict__ src, const Item* __restrict__ items, const int64_t* __restrict__ cut,
    const uint8_t* __restrict__ slots, int64_t slot_stride, const uint32_t* __restrict__ item_size,
    const int64_t* __restrict__ item_off, uint8_t* __restrict__ dst, int64_t dst_capacity,
    int32_t* __restrict__ status) {
  gather_item_body(src, items, (int32_t)cut[0], slots, slot_stride, item_size, item_off, dst, dst_capacity, status, (int)blockIdx.x);
}

}  // namespace

void launch_gather_items_cut(const uint8_t* d_src, const Item* d_items, int32_t n_items, const int64_t* d_cut,
                             const uint8_t* d_slots, int64_t slot_stride, const uint32_t* d_item_size,
                             const int64_t* d_item_off, uint8_t* d_dst, int64_t dst_capacity,
                             int32_t* d_status, hipStream_t st) {
  if (n_items <= 0) return;
  hipLaunchKernelGGL(gather_items_cut_kernel, dim3((unsigned)n_items), dim3(kGatherThreads), 0, st,
                     d_src, d_items, d_cut, d_slots, slot_stride, d_item_size, d_item_off, d_dst,
                     dst_capacity, d_status);
}

void launch_cstream_cut(const void* d_marks, const int64_t* d_item_off, int32_t n_items, const int32_t* d_part_first, int32_t n_pieces,
                        int64_t dst_capacity, int32_t first_last, int32_t ends0, int64_t open_img, int64_t* d_result,
                        int64_t* d_piece_off, int64_t* d_lengths, hipStream_t st) {
  hipLaunchKernelGGL(cstream_cut_kernel, dim3(1), dim3(kWave), 0, st, static_cast<const Mark*>(d_marks), d_item_off, n_items,
                     d_part_first, n_pieces, dst_capacity, first_last, ends0, open_img, d_result, d_piece_off, d_lengths);
}

}  // namespace s3s
