// compress_stream_cut.inc — the body of the cut kernels: a window's plan cut at the caller's output capacity.  Included INSIDE
// namespace s3s { namespace { ... } } by compress_stream_kernels.hip (cstream_cut_kernel: one window) and by
// compress_stream_batch_kernels.hip (cstream_cut_batch_kernel: one wavefront per window of a batched feed), so that both cut a
// plan the same way.  Needs s3s_cs::Mark and cut_lane (compress_stream_core.h).
//
// item_off is the scan of the item sizes (n_items + 1 entries, ascending).  The feed takes the items [0, k): k - 1 is the
// largest index that ends a unit (marks[].last) and whose end offset item_off[k] is at most dst_capacity.
// ONE wavefront and NO LDS, for the reason scan_items_body gives (assemble.hip): the codec kernels of other contexts book every
// CU's LDS, and a workgroup that asks for any waits for one of their chunks.  256 items per step, 4 per lane, like that scan;
// the wave-wide maximum is five cross-lane steps at the end.  Every store is a per-lane vector store.
//   result[kCut*]                 k, consumed, out_len, need_dst, parts_closed
//   piece_off[n_pieces + 1]       where the pieces of partitions start in the output, clamped to out_len: the checksum ranges
//   lengths[n_pieces - 1]         image length of every partition the feed closes (open_img added to the first), else 0
__device__ __forceinline__ void cstream_cut_body(
    const s3s_cs::Mark* __restrict__ marks, const int64_t* __restrict__ item_off, int32_t n_items, const int32_t* __restrict__ part_first,
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
