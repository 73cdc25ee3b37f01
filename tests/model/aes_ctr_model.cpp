// Host build of the product's AES-CTR core (spark-s3-shuffle_amd/csrc/aes_ctr_core.h): TEST INFRASTRUCTURE —
// tests/test_aes_ctr_model.py holds it against FIPS-197, SP 800-38A and libcrypto before the same code runs on the GPU, and
// tests/spark_crypto_ref.py builds the expected images of the GPU tests on it.  Two builds of this file: a shared object for
// ctypes, and (AC_MAIN, -fsanitize=address,undefined) a program that reads a file of cases and writes their key streams,
// every buffer a heap allocation of exactly the permitted size.
#include <stdio.h>

#include <vector>

#include "../../spark-s3-shuffle_amd/csrc/aes_ctr_core.h"

using namespace s3s_aes;

extern "C" {
// rk[0, 4 * (rounds + 1)); returns the rounds (10 / 12 / 14), 0 for a key that is not 16, 24 or 32 bytes
int ac_expand_key(const uint8_t* key, int key_bytes, uint32_t* rk) { return expand_key(key, key_bytes, rk); }

// out[0, 16) = AES_K(in[0, 16)); -1 for a key of another length
int ac_encrypt_block(const uint8_t* key, int key_bytes, const uint8_t* in, uint8_t* out) {
  std::vector<uint32_t> rk((size_t)4 * (size_t)(rounds_for_key(key_bytes) + 1));
  const int nr = expand_key(key, key_bytes, rk.data());
  if (nr == 0) return -1;
  const uint32_t s[4] = {load_be32(in), load_be32(in + 4), load_be32(in + 8), load_be32(in + 12)};
  uint32_t o[4];
  encrypt_block(rk.data(), nr, s, o, TableSbox{});
  for (int k = 0; k < 4; k++) store_be32(out + 4 * k, o[k]);
  return 0;
}

// ctr[0, 16) = (iv + j) mod 2^128, big-endian
void ac_counter_add(const uint8_t* iv, uint64_t j, uint8_t* ctr) {
  const uint32_t w[4] = {load_be32(iv), load_be32(iv + 4), load_be32(iv + 8), load_be32(iv + 12)};
  uint32_t c[4];
  counter_add(w, j, c);
  for (int k = 0; k < 4; k++) store_be32(ctr + 4 * k, c[k]);
}

// out[0, len) = key stream bytes [offset, offset + len); -1 for a key of another length
int ac_keystream(const uint8_t* key, int key_bytes, const uint8_t* iv, uint64_t offset, uint8_t* out, uint64_t len) {
  std::vector<uint32_t> rk((size_t)4 * (size_t)(rounds_for_key(key_bytes) + 1));
  const int nr = expand_key(key, key_bytes, rk.data());
  if (nr == 0) return -1;
  keystream(rk.data(), nr, iv, offset, out, len, TableSbox{});
  return 0;
}

// data[0, len) ^= key stream bytes [offset, offset + len)
int ac_xor(const uint8_t* key, int key_bytes, const uint8_t* iv, uint64_t offset, uint8_t* data, uint64_t len) {
  std::vector<uint8_t> ks((size_t)len);
  if (ac_keystream(key, key_bytes, iv, offset, ks.data(), len) != 0) return -1;
  for (uint64_t i = 0; i < len; i++) data[i] ^= ks[(size_t)i];
  return 0;
}
}

#ifdef AC_MAIN
// cases file: u32 count, then per case u32 key_bytes | key | iv[16] | u64 offset | u64 len;  output: per case the key stream
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* outf = fopen(argv[2], "wb");
  if (!in || !outf) return 2;
  uint32_t count = 0;
  if (fread(&count, sizeof count, 1, in) != 1) return 2;
  for (uint32_t c = 0; c < count; c++) {
    uint32_t kb;
    uint64_t offset, len;
    if (fread(&kb, sizeof kb, 1, in) != 1 || kb > 32) return 2;
    std::vector<uint8_t> key(kb), iv(kBlock);
    if (kb && fread(key.data(), 1, kb, in) != kb) return 2;
    if (fread(iv.data(), 1, kBlock, in) != (size_t)kBlock) return 2;
    if (fread(&offset, sizeof offset, 1, in) != 1 || fread(&len, sizeof len, 1, in) != 1) return 2;
    std::vector<uint8_t> out((size_t)len);
    if (ac_keystream(key.data(), (int)kb, iv.data(), offset, out.data(), len) != 0) return 3;
    if (len) fwrite(out.data(), 1, (size_t)len, outf);
  }
  fclose(outf);
  fclose(in);
  return 0;
}
#endif
