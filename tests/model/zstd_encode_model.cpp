// Host build of the product's Zstandard writer core (spark-s3-shuffle_amd/csrc/zstd_encode_core.h) on one thread:
// TEST INFRASTRUCTURE — tests/test_zstd_encode_model.py has libzstd's decoder and the host model of the product's own decoder
// read every frame written here before the same code runs on the GPU.  Two builds of this file: a shared object for ctypes,
// and (ZE_MAIN, -fsanitize=address) a program that reads a file of cases and writes their frames, every buffer a heap
// allocation of exactly the size the writer may use.
#include <stdio.h>

#include <vector>

#include "../../spark-s3-shuffle_amd/csrc/zstd_encode_core.h"

using namespace s3s_zstd_enc;

extern "C" {
int64_t ze_frame_bound(int64_t n) { return n <= 0 ? 0 : kFrameHeader + n + 3 * ((n + kBlock - 1) / kBlock); }

// one frame for src[0, n): the parse, blocks of kBlock.  Returns the frame's bytes (0 for n == 0), -1 when cap < ze_frame_bound(n).
int64_t ze_encode_frame(const uint8_t* src, int64_t n, uint8_t* out, int64_t cap) {
  if (n <= 0) return 0;
  if (cap < ze_frame_bound(n)) return -1;
  std::vector<Work> w(1);
  build_predefined(w[0]);
  std::vector<uint32_t> tab(1 << kHashLog);
  std::vector<uint64_t> seqs(kMaxSeq);
  for (int i = 0; i < kFrameHeader; i++) out[i] = frame_header_byte(i, (uint64_t)n);
  int64_t at = kFrameHeader;
  for (int64_t pos = 0; pos < n; pos += kBlock) {
    const uint32_t len = (uint32_t)(n - pos < kBlock ? n - pos : kBlock);
    std::vector<uint8_t> lits(len), blk(3 + (size_t)len);
    const uint32_t sz = encode_block(w[0], src + pos, len, pos + len == n, nullptr, 0, nullptr, 0, tab.data(), seqs.data(), lits.data(), blk.data());
    memcpy(out + at, blk.data(), sz);
    at += sz;
  }
  return at;
}

// the parse alone: seqs[kMaxSeq], lits[n]; returns the number of sequences, *nl the number of literals
int64_t ze_parse(const uint8_t* src, int64_t n, uint64_t* seqs, uint8_t* lits, int64_t* nl) {
  if (n <= 0 || n > kBlock) return -1;
  std::vector<uint32_t> tab(1 << kHashLog);
  uint32_t nseq = 0, nlit = 0;
  parse_block(src, (uint32_t)n, tab.data(), seqs, &nseq, lits, &nlit);
  *nl = nlit;
  return nseq;
}

// one frame of one block whose content (n bytes, 1 <= n <= kBlock) is what the GIVEN sequences and literals decode to
int64_t ze_encode_crafted(const uint8_t* content, int64_t n, const uint64_t* seqs, int64_t nseq, const uint8_t* lits, int64_t nl,
                          uint8_t* out, int64_t cap) {
  if (n <= 0 || n > kBlock || cap < ze_frame_bound(n)) return -1;
  std::vector<Work> w(1);
  build_predefined(w[0]);
  for (int i = 0; i < kFrameHeader; i++) out[i] = frame_header_byte(i, (uint64_t)n);
  static const uint64_t none = 0;
  std::vector<uint8_t> blk(3 + (size_t)n);
  const uint32_t sz = encode_block(w[0], content, (uint32_t)n, true, seqs ? seqs : &none, (uint32_t)nseq, lits, (uint32_t)nl, nullptr, nullptr,
                                   nullptr, blk.data());
  memcpy(out + kFrameHeader, blk.data(), sz);
  return kFrameHeader + sz;
}
}

#ifdef ZE_MAIN
// cases file: u32 count, then per case u32 kind (0 parse, 1 crafted) | u64 n | u64 nseq | u64 nl | content | seqs | lits;
// frames file: per case i64 size | bytes
template <typename T>
static bool rd(FILE* f, T* v, size_t n = 1) { return fread(v, sizeof(T), n, f) == n; }
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* outf = fopen(argv[2], "wb");
  if (!in || !outf) return 2;
  uint32_t count = 0;
  if (!rd(in, &count)) return 2;
  for (uint32_t c = 0; c < count; c++) {
    uint32_t kind;
    uint64_t n, nseq, nl;
    if (!rd(in, &kind) || !rd(in, &n) || !rd(in, &nseq) || !rd(in, &nl)) return 2;
    std::vector<uint8_t> content(n), lits(nl), frame((size_t)ze_frame_bound((int64_t)n));
    std::vector<uint64_t> seqs(nseq);
    if ((n && !rd(in, content.data(), n)) || (nseq && !rd(in, seqs.data(), nseq)) || (nl && !rd(in, lits.data(), nl))) return 2;
    const int64_t sz = kind == 0 ? ze_encode_frame(content.data(), (int64_t)n, frame.data(), (int64_t)frame.size())
                                 : ze_encode_crafted(content.data(), (int64_t)n, nseq ? seqs.data() : nullptr, (int64_t)nseq, lits.data(),
                                                     (int64_t)nl, frame.data(), (int64_t)frame.size());
    fwrite(&sz, sizeof sz, 1, outf);
    if (sz > 0) fwrite(frame.data(), 1, (size_t)sz, outf);
  }
  fclose(outf);
  fclose(in);
  return 0;
}
#endif
