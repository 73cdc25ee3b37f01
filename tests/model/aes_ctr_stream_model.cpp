// Host build of the window form of the AES-CTR pass (spark-s3-shuffle_amd/csrc/aes_ctr_stream_core.h): TEST INFRASTRUCTURE.
// acw_window walks the chunks of a window exactly as aes_ctr_window_kernel does - tile by tile, chunk by chunk, the units of a
// chunk from win_open / win_next - with the table S-box in place of the cross-lane one, and counts how often every stored byte
// was touched.  tests/test_aes_ctr_stream_cpu.py holds the result against keystream(offset, len) of aes_ctr_core.h.
// Two builds: a shared object for ctypes, and (ACW_MAIN, -fsanitize=address,undefined) a program that reads a file of cases and
// runs them with every buffer a heap allocation of exactly the window's size.
#include <stdio.h>

#include <vector>

#include "../../spark-s3-shuffle_amd/csrc/aes_ctr_stream_core.h"

using namespace s3s_aes;

extern "C" {
// in[0, L) with L = E[n]: the stored window;  out: Q[n] plain bytes;  iv_out: 16 n;  cover: L counters (IV bytes and key
// stream bytes alike);  tile_chunks: chunks per workgroup (the kernel's 1024; small values put tile ends everywhere).
// Returns the number of block encryptions that had a unit, -1 for a key of another length.
int64_t acw_window(const uint8_t* key, int key_bytes, const uint8_t* iv0, const uint8_t* in, const int64_t* E, const int64_t* Q, int32_t n,
                   int64_t front, int64_t tile_chunks, uint8_t* out, uint8_t* iv_out, uint8_t* cover) {
  std::vector<uint32_t> rk((size_t)4 * (size_t)(rounds_for_key(key_bytes) + 1));
  const int nr = expand_key(key, key_bytes, rk.data());
  if (nr == 0) return -1;
  const int64_t L = E[n];
  const uint32_t iv0w[4] = {load_be32(iv0), load_be32(iv0 + 4), load_be32(iv0 + 8), load_be32(iv0 + 12)};
  int64_t blocks = 0;
  const int64_t chunks = win_chunk_count(L, front);
  for (int64_t t0 = 0; t0 < chunks; t0 += tile_chunks) {
    const int64_t tile0 = win_chunk_start(t0, front);
    if (tile0 >= L) break;
    const int64_t tile_end = tile0 + 16 * tile_chunks < L ? tile0 + 16 * tile_chunks : L;
    const int32_t p_lo = win_last_start_le(E, 0, n - 1, tile0), p_hi = win_last_start_le(E, p_lo, n - 1, tile_end - 1);
    for (int64_t k = 0; k < tile_chunks; k++) {
      const int64_t x0 = tile0 + 16 * k;
      const bool live = x0 < tile_end;
      const int64_t lim = x0 + 16 < tile_end ? x0 + 16 : tile_end;
      WinCursor c;
      win_open(c, E, win_last_start_le(E, p_lo, p_hi, x0), front, x0);
      for (;;) {
        WinUnit u;
        if (!win_next(c, E, n, L, lim, live, u)) break;
        const bool carried = u.part == 0 && front > 0;
        if (u.len == 0) continue;
        blocks++;
        uint32_t ivw[4] = {iv0w[0], iv0w[1], iv0w[2], iv0w[3]};
        const uint8_t* ivp = in + (carried ? 0 : E[u.part]);
        if (!carried)
          for (int w = 0; w < 4; w++) ivw[w] = load_be32(ivp + 4 * w);
        if (u.is_iv) {
          for (int i = 0; i < 16; i++) {
            iv_out[16 * (int64_t)u.part + i] = ivp[i];
            cover[u.start + i]++;
          }
          continue;
        }
        uint32_t ks[4];
        keystream_block(rk.data(), nr, ivw, (uint64_t)u.block, ks, TableSbox{});
        const uint8_t* s = in + (u.start + u.skip);
        uint8_t* d = out + (Q[u.part] - (carried ? front - 16 : 0) + u.plain);
        for (int i = 0; i < u.len; i++) {
          const int b = u.skip + i;
          d[i] = (uint8_t)(s[i] ^ (ks[b >> 2] >> (24 - 8 * (b & 3))));
          cover[u.start + u.skip + i]++;
        }
      }
    }
  }
  return blocks;
}
}

#ifdef ACW_MAIN
// cases file: u32 count, then per case  u32 key_bytes | key | iv0[16] | i32 n | i64 front | i64 tile_chunks | E[n + 1] | Q[n + 1] |
// in[E[n]];  output per case: out[Q[n]] | iv_out[16 n] | cover[E[n]]
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* outf = fopen(argv[2], "wb");
  if (!in || !outf) return 2;
  uint32_t count = 0;
  if (fread(&count, sizeof count, 1, in) != 1) return 2;
  for (uint32_t cs = 0; cs < count; cs++) {
    uint32_t kb;
    int32_t n;
    int64_t front, tile_chunks;
    if (fread(&kb, sizeof kb, 1, in) != 1 || kb > 32) return 2;
    std::vector<uint8_t> key(kb), iv(kBlock);
    if (kb && fread(key.data(), 1, kb, in) != kb) return 2;
    if (fread(iv.data(), 1, kBlock, in) != (size_t)kBlock) return 2;
    if (fread(&n, sizeof n, 1, in) != 1 || n < 1 || fread(&front, sizeof front, 1, in) != 1 || fread(&tile_chunks, sizeof tile_chunks, 1, in) != 1) return 2;
    std::vector<int64_t> E((size_t)n + 1), Q((size_t)n + 1);
    if (fread(E.data(), 8, E.size(), in) != E.size() || fread(Q.data(), 8, Q.size(), in) != Q.size()) return 2;
    // exactly the window's size: a read or write one byte outside is a heap-buffer-overflow (sizes of 0 get no buffer at all)
    const size_t L = (size_t)E[(size_t)n], PL = (size_t)Q[(size_t)n];
    uint8_t* win = L ? new uint8_t[L] : nullptr;
    uint8_t* out = PL ? new uint8_t[PL]() : nullptr;
    uint8_t* cover = L ? new uint8_t[L]() : nullptr;
    std::vector<uint8_t> iv_out((size_t)16 * (size_t)n);
    if (L && fread(win, 1, L, in) != L) return 2;
    if (acw_window(key.data(), (int)kb, iv.data(), win, E.data(), Q.data(), n, front, tile_chunks, out, iv_out.data(), cover) < 0) return 3;
    if (PL) fwrite(out, 1, PL, outf);
    fwrite(iv_out.data(), 1, iv_out.size(), outf);
    if (L) fwrite(cover, 1, L, outf);
    delete[] win;
    delete[] out;
    delete[] cover;
  }
  fclose(outf);
  fclose(in);
  return 0;
}
#endif
