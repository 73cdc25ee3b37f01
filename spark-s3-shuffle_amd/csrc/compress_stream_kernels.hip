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

#include "compress_stream_cut.inc"  // cstream_cut_body: shared with cstream_cut_batch_kernel (compress_stream_batch_kernels.hip)

// one window: the cut of its plan at dst_capacity (the body, and what it writes: compress_stream_cut.inc)
__global__ __launch_bounds__(kWave) void cstream_cut_kernel(
    const Mark* __restrict__ marks, const int64_t* __restrict__ item_off, int32_t n_items, const int32_t* __restrict__ part_first,
    int32_t n_pieces, int64_t dst_capacity, int32_t first_last, int32_t ends0, int64_t open_img, int64_t* __restrict__ result,
    int64_t* __restrict__ piece_off, int64_t* __restrict__ lengths) {
  cstream_cut_body(marks, item_off, n_items, part_first, n_pieces, dst_capacity, first_last, ends0, open_img, result, piece_off, lengths);
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
