// Host build of the staged Zstandard path (spark-s3-shuffle_amd/csrc/zstd_decode_core.h: staged_scan_partition, the entropy
// stage, staged_place_partition, staged_block_copy, staged_execute_frame, decode_partition<true, true>) with one "lane": TEST
// INFRASTRUCTURE - tests/test_zstd_staged_model.py holds it against libzstd and the serial host model before the same code runs
// on the GPU.  The order is the device's: (the block path of 6j over a prefix of the frames when asked for,) scan, entropy of
// every block, place, copy of every block, execute per frame, then the per-partition walk that steps over what completed and
// decodes the rest.  Two builds: a shared object for ctypes, and (ZG_MAIN, -fsanitize=address,undefined) a program whose
// source, staging and destination are heap buffers of exactly their sizes.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../spark-s3-shuffle_amd/csrc/zstd_decode_core.h"

using namespace s3s_zstd;

extern "C" {
// info[0] frames the staged scan entered, [1] blocks in its table, [2] of those frames flagged dependent, [3] blocks of the
// frames the walk stepped over as staged (key 16), [4] the same for the block path of 6j (key 14), [5] the serial decoder's
// verdict of the same bytes, [6] bytes of literal staging handed out, [7] records handed out, [8] Treeless blocks in the
// table, [9] Repeat_Mode tables in the table.  frame_dep[k] (k < max_frames): dependent flag of staged frame k.
// budget_bytes: compressed bytes the staging is sized for (the call's: >= size; the partition alone: size).
// Returns the verdict of the full path, -1000 when the two paths disagree in their verdict or, both ZS_OK, in length or bytes.
int zg_decode(const uint8_t* src, int64_t size, uint8_t* dst, int64_t cap, int with_block_path, int64_t budget_bytes, int64_t* total,
              int64_t* info, int32_t* frame_dep, int32_t max_frames) {
  static thread_local Work w;
  static thread_local LitPipe lp;
  static thread_local SeqWork sw;
  static thread_local HufWork hw;
  std::vector<uint8_t> lit(kMaxBlock + 64);
  Lanes L{0, 1};
  for (int i = 0; i < 10; i++) info[i] = 0;
  // ---- the block path of 6j in front (key 13) ----
  const int32_t frame_cap13 = (int32_t)(cap / (kMaxBlock + 1) + 1);
  const int64_t job_cap = 2 * cap / kMaxBlock + 2;
  std::vector<FrameEnt> frames13((size_t)frame_cap13);
  std::vector<BlockJob> jobs((size_t)job_cap);
  int32_t nf13 = 0;
  int64_t ip0 = 0, op0 = 0;
  if (with_block_path) {
    int64_t n_jobs = 0;
    auto reserve13 = [&](int32_t want) -> int64_t {
      if (want > job_cap - n_jobs) return -1;
      const int64_t at = n_jobs;
      n_jobs += want;
      return at;
    };
    nf13 = scan_partition(src, size, cap, 0, true, frames13.data(), frame_cap13, 0, jobs.data(), reserve13);
    for (int64_t j = 0; j < n_jobs; j++) {
      const BlockJob job = jobs[(size_t)j];
      if (job.expect <= 0) continue;
      FrameEnt& fe = frames13[(size_t)job.frame];
      if (fe.dependent) continue;
      const int64_t stored = job.type == 1 ? 1 : job.bsize;
      if (decode_block(w, lp, src + job.src_off, 3 + stored, dst + job.out_off, job.expect, lit.data(), 0, 0, L) == ZS_OK) fe.done++;
      else fe.dependent = 1;
    }
    for (int32_t k = 0; k < nf13; k++) {  // the staged walk starts behind the frames whose headers added up
      const FrameEnt& fe = frames13[(size_t)k];
      if (fe.consumed <= 0) break;
      ip0 = fe.src_off + fe.consumed;
      op0 = fe.out_off + fe.fcs;
    }
  }
  // ---- staging: heap buffers of exactly their sizes ----
  const int64_t blk_cap = staged_block_cap(budget_bytes), lit_cap = staged_lit_cap(budget_bytes), rec_cap = staged_rec_cap(budget_bytes);
  StagedBlock* tab = (StagedBlock*)malloc(sizeof(StagedBlock) * (size_t)blk_cap);
  uint8_t* lit_pool = (uint8_t*)malloc((size_t)lit_cap);
  SeqRec* rec_pool = (SeqRec*)malloc(sizeof(SeqRec) * (size_t)rec_cap);
  FrameEnt* frames = (FrameEnt*)malloc(sizeof(FrameEnt) * kStagedFramesPerPart);
  int32_t* block_base = (int32_t*)malloc(sizeof(int32_t) * kStagedFramesPerPart);
  int32_t* comp_len = (int32_t*)malloc(sizeof(int32_t) * (size_t)blk_cap);
  if (!tab || !lit_pool || !rec_pool || !frames || !block_base || !comp_len) return -1001;
  int64_t used[3] = {0, 0, 0};
  const int64_t caps[3] = {blk_cap, lit_cap, rec_cap};
  auto reserve = [&](int which, int64_t want) -> int64_t {
    if (want > caps[which] - used[which]) return -1;
    const int64_t at = used[which];
    used[which] += want;
    return at;
  };
  const int32_t nf = staged_scan_partition(src, size, 0, ip0, op0, frames, block_base, kStagedFramesPerPart, 0, tab, reserve);
  info[0] = nf;
  info[1] = used[0];
  info[6] = used[1];
  info[7] = used[2];
  for (int64_t b = 0; b < used[0]; b++) {
    const StagedBlock& sb = tab[b];
    if (sb.type == 2 && sb.ltype == 3) info[8]++;
    if (sb.type == 2 && sb.nseq > 0) info[9] += (sb.def_ll != b) + (sb.def_of != b) + (sb.def_ml != b);
  }
  // ---- entropy: any order (here: backwards, so that nothing can lean on an earlier block's having run) ----
  for (int64_t b = used[0] - 1; b >= 0; b--) {
    int32_t out_len = 0;
    int rc = staged_block_literals(hw, src, tab, (int32_t)b, lit_pool, lit_cap, L);
    if (rc == ZS_OK && tab[b].type == 2) {
      rc = staged_block_sequences(sw, src, tab, (int32_t)b, rec_pool, rec_cap, &out_len, L);
      if (rc == ZS_OK) comp_len[b] = out_len;
    }
    if (rc != ZS_OK) frames[tab[b].frame].dependent = 1;
  }
  // ---- place, copy, execute ----
  staged_place_partition(frames, block_base, nf, tab, comp_len, cap, L);
  for (int64_t b = used[0] - 1; b >= 0; b--)
    if (!frames[tab[b].frame].dependent) staged_block_copy(src, dst, tab[b], rec_pool, lit_pool, L);
  for (int32_t f = 0; f < nf; f++) {
    if (frames[f].dependent) continue;
    if (staged_execute_frame(frames[f], tab + block_base[f], rec_pool, dst + frames[f].out_off, L) == ZS_OK) frames[f].done = frames[f].n_blocks;
    else frames[f].dependent = 1;
  }
  for (int32_t f = 0; f < nf; f++) {
    info[2] += frames[f].dependent ? 1 : 0;
    if (f < max_frames) frame_dep[f] = frames[f].dependent;
  }
  // ---- the walk behind: steps over what completed, decodes the rest ----
  int32_t blocks13 = 0, blocks_staged = 0;
  const int rc = decode_partition<true, true>(w, lp, src, size, dst, cap, true, lit.data(), 0, L, total, nullptr,
                                              SkipCursor{frames13.data(), nf13, 0}, &blocks13, SkipCursor{frames, nf, 0}, &blocks_staged);
  info[3] = blocks_staged;
  info[4] = blocks13;
  free(tab);
  free(lit_pool);
  free(rec_pool);
  free(frames);
  free(block_base);
  free(comp_len);
  {  // what the serial decoder alone says (the verdict the full path must repeat)
    uint8_t* other = (uint8_t*)malloc((size_t)(cap > 0 ? cap : 1));
    int64_t t2 = 0;
    info[5] = decode_partition(w, lp, src, size, other, cap, true, lit.data(), 0, L, &t2);
    const bool differ = info[5] != rc || (rc == ZS_OK && (t2 != *total || memcmp(other, dst, (size_t)t2) != 0));
    free(other);
    if (differ) return -1000;
  }
  return rc;
}
}

// The staging a call of comp_bytes compressed bytes gets: entries of the block table, bytes of literals, records.
extern "C" void zg_caps(int64_t comp_bytes, int64_t* caps) {
  caps[0] = staged_block_cap(comp_bytes);
  caps[1] = staged_lit_cap(comp_bytes);
  caps[2] = staged_rec_cap(comp_bytes);
}

#ifdef ZG_MAIN
// cases file: u32 count, then per case i64 size | i64 content size (-1: the partition is invalid) | i64 capacity | i32 block path in
// front | i32 expected staged frames | i32 expected dependent frames | i32 expected staged blocks | source bytes | content bytes
// Verdict only (tests/test_zstd_mutants_model.py): the three counts are -1 and are not compared - the verdict, the bytes and the
// serial decoder's agreement are.
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
    int64_t size, csize, cap;
    int32_t with13, want_frames, want_dep, want_blocks;
    if (!rd(in, &size) || !rd(in, &csize) || !rd(in, &cap) || !rd(in, &with13) || !rd(in, &want_frames) || !rd(in, &want_dep) || !rd(in, &want_blocks))
      return 2;
    uint8_t* src = (uint8_t*)malloc((size_t)(size > 0 ? size : 1));  // exactly their sizes: the sanitizer sees the first byte outside
    uint8_t* content = (uint8_t*)malloc((size_t)(csize > 0 ? csize : 1));
    uint8_t* dst = (uint8_t*)malloc((size_t)(cap > 0 ? cap : 1));
    if (!src || !content || !dst || !rd(in, src, (size_t)size) || (csize > 0 && !rd(in, content, (size_t)csize))) return 2;
    memset(dst, 0x5A, (size_t)cap);
    int64_t total = -1, info[10];
    int32_t dep[16];
    const int rc = zg_decode(src, size, dst, cap, with13, size, &total, info, dep, 16);
    CHECK(rc == (int)info[5]);
    if (csize >= 0) {
      CHECK(rc == ZS_OK);
      CHECK(total == csize);
      CHECK(memcmp(dst, content, (size_t)csize) == 0);
    } else {
      CHECK(rc != ZS_OK);
    }
    if (!(want_frames == -1 && want_dep == -1 && want_blocks == -1)) {
      CHECK(info[0] == want_frames);
      CHECK(info[2] == want_dep);
      CHECK(info[3] == want_blocks);
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
