// Host build of the block-parallel Zstandard path (spark-s3-shuffle_amd/csrc/zstd_decode_core.h: scan_partition, decode_block,
// decode_partition<true>) with one "lane": TEST INFRASTRUCTURE — tests/test_zstd_block_parallel_model.py runs writer frames,
// crafted frames that must fall back and libzstd's frames through it before the same code runs on the GPU.  The order is the
// device's: scan the headers, decode every block of every candidate frame on its own, then the per-partition walk that steps
// over the frames that completed and decodes the others.  Two builds: a shared object for ctypes, and (ZB_MAIN,
// -fsanitize=address,undefined) a program with source and destination on the heap at exactly their sizes.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../spark-s3-shuffle_amd/csrc/zstd_decode_core.h"

using namespace s3s_zstd;

extern "C" {
// info[0] candidate frames entered by the scan, [1] of them with block headers that add up (eligible), [2] blocks in the table,
// [3] blocks that decoded on their own, [4] frames flagged dependent, [5] blocks of the frames that completed on the block path,
// [6] bytes written outside a block's own slot (must be 0), [7] the serial decoder's verdict of the same bytes.
// frame_dep[k] (k < max_frames): dependent flag of candidate frame k.  Returns the verdict of the full path.
int zb_decode(const uint8_t* src, int64_t size, uint8_t* dst, int64_t cap, int window_rule, int64_t* total, int64_t* info, int32_t* frame_dep,
              int32_t max_frames) {
  static thread_local Work w;
  static thread_local LitPipe lp;
  std::vector<uint8_t> lit(kMaxBlock + 64);
  Lanes L{0, 1};
  for (int i = 0; i < 8; i++) info[i] = 0;
  const int32_t frame_cap = (int32_t)(cap / (kMaxBlock + 1) + 1);
  const int64_t job_cap = 2 * cap / kMaxBlock + 2;
  std::vector<FrameEnt> frames((size_t)frame_cap);
  std::vector<BlockJob> jobs((size_t)job_cap);
  int64_t n_jobs = 0;
  auto reserve = [&](int32_t want) -> int64_t {
    if (want > job_cap - n_jobs) return -1;
    const int64_t at = n_jobs;
    n_jobs += want;
    return at;
  };
  const int32_t nf = scan_partition(src, size, cap, 0, window_rule != 0, frames.data(), frame_cap, 0, jobs.data(), reserve);
  info[0] = nf;
  for (int32_t k = 0; k < nf; k++) info[1] += frames[(size_t)k].dependent ? 0 : 1;
  info[2] = n_jobs;
  std::vector<uint8_t> shadow;
  for (int64_t j = 0; j < n_jobs; j++) {
    const BlockJob job = jobs[(size_t)j];
    if (job.expect <= 0) continue;
    FrameEnt& fe = frames[(size_t)job.frame];
    if (fe.dependent) continue;  // (the device may skip such a block too; it never has to)
    shadow.assign(dst, dst + cap);
    const int64_t stored = job.type == 1 ? 1 : job.bsize;
    const int rc = decode_block(w, lp, src + job.src_off, 3 + stored, dst + job.out_off, job.expect, lit.data(), 0, 0, L);
    for (int64_t i = 0; i < cap; i++)
      if ((i < job.out_off || i >= job.out_off + job.expect) && dst[i] != shadow[(size_t)i]) info[6]++;
    if (rc == ZS_OK) {
      fe.done++;
      info[3]++;
    } else {
      fe.dependent = 1;
    }
  }
  for (int32_t k = 0; k < nf; k++) {
    info[4] += frames[(size_t)k].dependent ? 1 : 0;
    if (k < max_frames) frame_dep[k] = frames[(size_t)k].dependent;
  }
  int32_t blocks = 0;
  const int rc = decode_partition<true>(w, lp, src, size, dst, cap, true, lit.data(), 0, L, total, nullptr, SkipCursor{frames.data(), nf, 0}, &blocks);
  info[5] = blocks;
  {  // what the serial decoder alone says (the verdict the full path must repeat)
    std::vector<uint8_t> other((size_t)(cap > 0 ? cap : 1));
    int64_t t2 = 0;
    info[7] = decode_partition(w, lp, src, size, other.data(), cap, true, lit.data(), 0, L, &t2);
    if (info[7] == ZS_OK && rc == ZS_OK && (t2 != *total || memcmp(other.data(), dst, (size_t)t2) != 0)) return -1000;  // the two paths disagree
  }
  return rc;
}
}

#ifdef ZB_MAIN
// cases file: u32 count, then per case i64 size | i64 content size (-1: the frame is invalid) | i32 window rule | i32 expected
// candidate frames | i32 expected dependent frames | i32 expected blocks on the block path | source bytes | content bytes
// Verdict only (tests/test_zstd_mutants_model.py): the three counts are -1, an i64 capacity follows them, and the counts are
// not compared - the verdict, the bytes, the serial decoder's agreement and "nothing outside a slot" are.
template <typename T>
static bool rd(FILE* f, T* v, size_t n = 1) { return fread(v, sizeof(T), n, f) == n; }
#define CHECK(c)                                                             \
  do {                                                                       \
    if (!(c)) {                                                              \
      fprintf(stderr, "case %u: %s (line %d)\n", cs, #c, __LINE__);          \
      return 1;                                                              \
    }                                                                        \
  } while (0)
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  uint32_t count = 0;
  if (!rd(in, &count)) return 2;
  for (uint32_t cs = 0; cs < count; cs++) {
    int64_t size, csize;
    int32_t rule, want_frames, want_dep, want_blocks;
    if (!rd(in, &size) || !rd(in, &csize) || !rd(in, &rule) || !rd(in, &want_frames) || !rd(in, &want_dep) || !rd(in, &want_blocks)) return 2;
    const bool verdict_only = want_frames == -1 && want_dep == -1 && want_blocks == -1;
    int64_t cap = csize < 0 ? 4 * kMaxBlock : csize;
    if (verdict_only && !rd(in, &cap)) return 2;
    uint8_t* src = (uint8_t*)malloc((size_t)(size > 0 ? size : 1));  // exactly their sizes: the sanitizer sees the first byte outside
    uint8_t* content = (uint8_t*)malloc((size_t)(csize > 0 ? csize : 1));
    uint8_t* dst = (uint8_t*)malloc((size_t)(cap > 0 ? cap : 1));
    if (!src || !content || !dst || !rd(in, src, (size_t)size) || (csize > 0 && !rd(in, content, (size_t)csize))) return 2;
    memset(dst, 0x5A, (size_t)cap);
    int64_t total = -1, info[8];
    int32_t dep[16];
    const int rc = zb_decode(src, size, dst, cap, rule, &total, info, dep, 16);
    CHECK(info[6] == 0);
    CHECK(rc == (int)info[7]);
    if (csize >= 0) {
      CHECK(rc == ZS_OK);
      CHECK(total == csize);
      CHECK(memcmp(dst, content, (size_t)csize) == 0);
    } else {
      CHECK(rc != ZS_OK);
    }
    if (!verdict_only) {
      CHECK(info[0] == want_frames);
      CHECK(info[4] == want_dep);
      CHECK(info[5] == want_blocks);
    }
    free(src);
    free(content);
    free(dst);
  }
  fclose(in);
  printf("%u cases ok\n", count);
  return 0;
}
#endif
