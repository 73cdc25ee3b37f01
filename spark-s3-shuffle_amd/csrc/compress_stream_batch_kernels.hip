// compress_stream_batch_kernels.hip — the device side of the batched feed of the streaming map side (s3s_cstream_feed_batch*,
// compress_stream.hip) that is specific to a stream: the capacity cut of EVERY window of the call in one launch, and the
// gather that reads every window's cut from device memory in one launch.  The codec kernels run unchanged over the items of all
// windows (an item addresses its source as a signed offset from one base pointer), the scan and the checksums are the
// task-aware launches of the batched one-shot call (launch_scan_items_batch, launch_checksum_batch) and of the batched
// reduce-side feed (launch_checksum_seed_batch).  The layout of the call's arrays is compress_stream_batch_core.h.
#include "s3s_internal.h"
#include "compress_stream_batch_core.h"

namespace s3s {
namespace {

using s3s_cs::CutEntry;
using s3s_cs::Mark;

#include "assemble_gather.h"
#include "compress_stream_cut.inc"

// One wavefront per window, no LDS, per-lane vector stores only (compress_stream_cut.inc says why).  The window's descriptor
// is wave-uniform: a handful of scalar loads.
__global__ __launch_bounds__(kWave) void cstream_cut_batch_kernel(
    const CutEntry* __restrict__ cuts, int32_t n_entries, const Mark* __restrict__ marks, const int64_t* __restrict__ item_off,
    const int32_t* __restrict__ part_first, int64_t* __restrict__ result, int64_t* __restrict__ piece_off, int64_t* __restrict__ lengths) {
  const int e = blockIdx.x;
  if (e >= n_entries) return;
  const CutEntry c = cuts[e];
  cstream_cut_body(marks + c.first_item, item_off + c.first_item + e, c.n_items, part_first + c.first_pp, c.n_pieces, c.dst_capacity,
                   c.first_last, c.ends0, c.open_img, result + (size_t)s3s_cs::kCutWords * (size_t)e, piece_off + c.first_pp,
                   lengths + c.first_len);
}

// the entry that owns item g of the call: the last e with first_item(e) <= g (wave-uniform: scalar loads; see assemble.hip)
__device__ __forceinline__ int owner_entry(const TaskTail* __restrict__ tails, int32_t n_entries, int32_t g) {
  int lo = 0, hi = n_entries;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tails[mid].first_item <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// One workgroup per item of EVERY window of the call: the items [0, k) of a window go to that window's d_dst, k is what the
// cut kernel left in the window's result words (never more than the window's items), and nothing is written at or beyond the
// window's dst_capacity (gather_item_body raises the window's status word instead).
__global__ __launch_bounds__(kGatherThreads) void gather_items_cut_batch_kernel(
    const TaskTail* __restrict__ tails, int32_t n_entries, int32_t n_items_total, const uint8_t* __restrict__ src,
    const Item* __restrict__ items, const int64_t* __restrict__ result, const uint8_t* __restrict__ slots, int64_t slot_stride,
    const uint32_t* __restrict__ item_size, const int64_t* __restrict__ item_off, int32_t* __restrict__ status) {
  const int g = blockIdx.x;
  if (g >= n_items_total) return;
  const int e = owner_entry(tails, n_entries, g);
  const TaskTail t = tails[e];
  const int64_t k = result[(size_t)s3s_cs::kCutWords * (size_t)e + s3s_cs::kCutK];
  gather_item_body(src, items + t.first_item, (int32_t)(k < t.n_items ? k : t.n_items), slots, slot_stride, item_size + t.first_item,
                   item_off + t.first_item + e, t.dst, t.dst_capacity, status + e, g - t.first_item);
}

}  // namespace

void launch_cstream_cut_batch(const void* d_cuts, int32_t n_entries, const void* d_marks, const int64_t* d_item_off,
                              const int32_t* d_part_first, int64_t* d_result, int64_t* d_piece_off, int64_t* d_lengths, hipStream_t st) {
  if (n_entries <= 0) return;
  hipLaunchKernelGGL(cstream_cut_batch_kernel, dim3((unsigned)n_entries), dim3(kWave), 0, st, static_cast<const CutEntry*>(d_cuts), n_entries,
                     static_cast<const Mark*>(d_marks), d_item_off, d_part_first, d_result, d_piece_off, d_lengths);
}

void launch_gather_items_cut_batch(const TaskTail* d_tails, int32_t n_entries, int32_t n_items_total, const uint8_t* d_src,
                                   const Item* d_items, const int64_t* d_result, const uint8_t* d_slots, int64_t slot_stride,
                                   const uint32_t* d_item_size, const int64_t* d_item_off, int32_t* d_status, hipStream_t st) {
  if (n_entries <= 0 || n_items_total <= 0) return;
  hipLaunchKernelGGL(gather_items_cut_batch_kernel, dim3((unsigned)n_items_total), dim3(kGatherThreads), 0, st, d_tails, n_entries,
                     n_items_total, d_src, d_items, d_result, d_slots, slot_stride, d_item_size, d_item_off, d_status);
}

}  // namespace s3s
