// Stand-alone driver of spark-s3-shuffle_amd/csrc/stream_placement.h (TEST INFRASTRUCTURE: tests/test_stream_placement_cpu.py
// builds it with -fsanitize=address,undefined and reads what it prints).
//   class <cap> <levels> <order> : stream_class of slots 0 .. 127, one number per slot
//   plan <tasks> <parts> <items> <tail_bytes> <item_bytes> : the offsets of packed_plan, in the order of the struct
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "stream_placement.h"

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "class")) {
    const int cap = atoi(argv[2]), levels = atoi(argv[3]), order = atoi(argv[4]);
    for (int slot = 0; slot < 128; slot++) {
      const int c = s3s::stream_class_ordered(slot, cap, levels, order);
      if (order == 1 && c != s3s::stream_class(slot, cap, levels)) return 2;  // the default order IS stream_class
      printf("%d ", c);
    }
    printf("\n");
    return 0;
  }
  if (argc == 7 && !strcmp(argv[1], "plan")) {
    const s3s::PackedPlan L = s3s::packed_plan(strtoull(argv[2], 0, 10), strtoull(argv[3], 0, 10), strtoull(argv[4], 0, 10),
                                               strtoull(argv[5], 0, 10), strtoull(argv[6], 0, 10));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", L.work, L.tails, L.items, L.part_first, L.seg_start, L.status, L.up_end, L.index,
           L.sums, L.total);
    return 0;
  }
  fprintf(stderr, "usage: class <cap> <levels> <order> | plan <tasks> <parts> <items> <tail_bytes> <item_bytes>\n");
  return 1;
}
