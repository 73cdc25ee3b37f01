// stream_placement.h — where a context's stream goes among the runtime's hardware-queue pools, and how a batched map-side
// call packs its small arrays into one upload and one download.  No HIP in here: both are pure functions of their
// arguments and are tested on the CPU (tests/test_stream_placement_cpu.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace s3s {

// The HIP runtime maps the streams of a process onto hardware queues, and streams that share a queue run one after the
// other.  It keeps one pool of queues PER STREAM PRIORITY, each with its own cap (GPU_MAX_HW_QUEUES, default 4).  Contexts
// take the lowest free slot of their device (codec_api.hip) and the slot decides the pool:
//   slots 0 .. cap-1        lowest priority   nothing else of the library or the application lives there, and the first
//                                             `cap` contexts stay equal among themselves
//   the next cap-1 slots    normal priority   one queue is left to the application's own stream
//   the next cap-2 slots    highest priority  two queues are left to the copy lanes (host_batch.hip)
//   beyond                  normal priority   sharing is unavoidable
// A device with two priority levels has no pool below the normal one, a device with one level has only the normal pool;
// the pools that exist are filled in the same order.
enum StreamClass { kStreamLowest = 0, kStreamNormal = 1, kStreamHighest = 2, kStreamOverflow = 3 };

// queues of a pool that contexts may take
inline int stream_pool_share(int cls, int cap, int levels) {
  if (cap < 1) cap = 1;
  if (cap > 32) cap = 32;
  switch (cls) {
    case kStreamLowest: return levels >= 3 ? cap : 0;
    case kStreamNormal: return cap - 1;
    case kStreamHighest: return levels >= 2 && cap > 2 ? cap - 2 : 0;
  }
  return 0;
}

// order 1: lowest, normal, highest (the default).  order 2: normal, highest, lowest.  order 0: every stream normal, no pools.
inline int stream_class_ordered(int slot, int cap, int levels, int order) {
  if (order == 0) return kStreamNormal;
  static const int kOrders[2][3] = {{kStreamLowest, kStreamNormal, kStreamHighest}, {kStreamNormal, kStreamHighest, kStreamLowest}};
  int first = 0;
  for (int i = 0; i < 3; i++) {
    const int cls = kOrders[order == 2 ? 1 : 0][i];
    first += stream_pool_share(cls, cap, levels);
    if (slot < first) return cls;
  }
  return kStreamOverflow;
}

inline int stream_class(int slot, int cap, int levels) { return stream_class_ordered(slot, cap, levels, 1); }

// ---- batched map-side call: one arena, one upload, one download ---------------------------------------------------------
// [work counter (16 bytes) | tails | items | part_first | seg_start | status | index | sums], the same layout in the pinned
// staging block and on the device.  The upload is ONE copy of [0, up_end): the zeros of the codec grid's block counter and
// of the per-task status words travel with it, so the call queues no memset.  The download is ONE copy of
// [status, total) - or of [status, sums) without a checksum algorithm, the sums region is then not read.
// n_parts = partitions of all tasks; part_first, seg_start and index hold n_parts + n_tasks entries (one more per task).
// Every region starts on a 16-byte boundary.
struct PackedPlan {
  size_t work, tails, items, part_first, seg_start, status, up_end;  // uploaded: [0, up_end)
  size_t index, sums, total;                                         // downloaded: [status, total)
};

inline size_t plan_align(size_t x) { return (x + 15) & ~size_t(15); }

inline PackedPlan packed_plan(size_t n_tasks, size_t n_parts, size_t n_items, size_t tail_bytes, size_t item_bytes) {
  PackedPlan L;
  const size_t np1 = n_parts + n_tasks;
  L.work = 0;
  L.tails = 16;
  L.items = plan_align(L.tails + tail_bytes * n_tasks);
  L.part_first = plan_align(L.items + item_bytes * n_items);
  L.seg_start = plan_align(L.part_first + 4 * np1);
  L.status = plan_align(L.seg_start + 4 * np1);
  L.up_end = plan_align(L.status + 4 * n_tasks);
  L.index = L.up_end;
  L.sums = plan_align(L.index + 8 * np1);
  L.total = plan_align(L.sums + 8 * n_parts);
  return L;
}

}  // namespace s3s
