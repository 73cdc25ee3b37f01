// The conformance corpus (tests/zstd_conformance.py) through the product's Zstandard decoder core under ASan / UBSan: TEST
// INFRASTRUCTURE (tests/test_zstd_conformance.py builds and runs it).  Every partition is decoded once, unchanged, from a heap
// copy of EXACTLY its size into a destination of EXACTLY its content's size (an invalid one: into 64 KiB), so that a read or a
// write one byte outside either stops the run with a sanitizer report; the result is compared with the expected content or the
// expected refusal.
//   usage: zstd_asan_corpus <case file>     records: u32 compressed size, u32 content size, i32 expected status, the bytes, the content
//          zstd_asan_corpus --cap <case file>   the same records with an i64 destination capacity behind the expected status
//                                               (tests/test_zstd_mutants_model.py: a mutant's capacity is part of the case)
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../spark-s3-shuffle_amd/csrc/zstd_decode_core.h"

using namespace s3s_zstd;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const bool with_cap = argc > 2 && !strcmp(argv[1], "--cap");
  FILE* f = fopen(argv[with_cap ? 2 : 1], "rb");
  if (!f) return 2;
  static Work w_size, w_dec;
  static LitPipe lp_size, lp_dec;
  std::vector<uint8_t> lit(kMaxBlock + 64);
  long n_cases = 0, n_wrong = 0;
  for (;;) {
    uint32_t n = 0, usize = 0;
    int32_t want = 0;
    int64_t given_cap = 0;
    if (fread(&n, 4, 1, f) != 1 || fread(&usize, 4, 1, f) != 1 || fread(&want, 4, 1, f) != 1) break;
    if (with_cap && fread(&given_cap, 8, 1, f) != 1) return 2;
    std::unique_ptr<uint8_t[]> comp(new uint8_t[n ? n : 1]);
    std::unique_ptr<uint8_t[]> content(new uint8_t[usize ? usize : 1]);
    if (n && fread(comp.get(), 1, n, f) != n) return 2;
    if (usize && fread(content.get(), 1, usize, f) != usize) return 2;
    const int64_t cap = with_cap ? given_cap : want == 0 ? (int64_t)usize : 65536;
    std::unique_ptr<uint8_t[]> dst(new uint8_t[cap ? cap : 1]);
    Lanes L{0, 1};
    int64_t total = -1, total2 = -1;
    int rc = decode_partition(w_size, lp_size, comp.get(), (int64_t)n, nullptr, 0, false, nullptr, 0, L, &total);
    if (rc == 0) rc = decode_partition(w_dec, lp_dec, comp.get(), (int64_t)n, dst.get(), cap, true, lit.data(), 0, L, &total2);
    bool ok = rc == want;
    if (ok && want == 0) ok = total == (int64_t)usize && total2 == total && memcmp(dst.get(), content.get(), usize) == 0;
    if (!ok) {
      printf("case %ld: status %d (expected %d), sizes %lld / %lld (expected %u)\n", n_cases, rc, (int)want, (long long)total, (long long)total2, usize);
      n_wrong++;
    }
    n_cases++;
  }
  fclose(f);
  printf("zstd_asan_corpus: %ld cases, %ld wrong\n", n_cases, n_wrong);
  return n_wrong ? 1 : 0;
}
