// aes_ctr_core.h — AES in counter mode as Spark's IO encryption uses it (AES/CTR/NoPadding), written once for the device
// and for the host.
//
// The layer (CryptoStreamUtils.createCryptoOutputStream, restated - parity unpinned): a non-empty partition is
//   IV (16 bytes) | codec bytes XOR key stream,   key stream block j = AES_K((IV as a 128-bit big-endian integer + j) mod 2^128)
// The carry of the counter runs through all 16 bytes (the JCE and OpenSSL both count this way).  Every block is independent, so
// the stream is seekable: keystream(offset, len) below starts anywhere.
//
// What is here: the key expansion for 128 / 192 / 256 bits (host only: the round keys reach the kernel as arguments), one
// block encryption, the counter add, and keystream().  The block encryption takes its S-box as a functor: the host looks a
// byte up in the table (TableSbox), the kernel (aes_ctr.hip) keeps the 256 bytes in ONE register across the 64 lanes of a
// wavefront and reads them through the cross-lane network.  Everything else - ShiftRows, MixColumns on packed columns, the
// round structure - is the same code on both sides.  A column is a big-endian uint32 (row 0 in bits 31..24), as in FIPS-197's
// word notation; the round keys are words of the same form.
//
// Compiled by hipcc (S3S_AES_DEVICE: aes_ctr.hip) and by g++ (tests/model/aes_ctr_model.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef S3S_AES_DEVICE
#define AC_HD __host__ __device__ inline
#define AC_MEMBER __host__ __device__ inline
#else
#define AC_HD static inline
#define AC_MEMBER inline
#endif

namespace s3s_aes {

constexpr int kBlock = 16;          // bytes of an AES block, of the IV and of a key stream block
constexpr int kMaxRoundKeys = 60;   // dwords: 4 x (14 + 1) for a 256-bit key

// number of rounds for a key of key_bytes (16, 24, 32), 0 for any other length
AC_HD int rounds_for_key(int key_bytes) { return key_bytes == 16 ? 10 : key_bytes == 24 ? 12 : key_bytes == 32 ? 14 : 0; }

AC_HD uint32_t sbox_at(uint32_t i) {
  constexpr uint8_t t[256] = {
      0x63, 0x7c, 0x77, 0x7b, 0xf2, 0x6b, 0x6f, 0xc5, 0x30, 0x01, 0x67, 0x2b, 0xfe, 0xd7, 0xab, 0x76,
      0xca, 0x82, 0xc9, 0x7d, 0xfa, 0x59, 0x47, 0xf0, 0xad, 0xd4, 0xa2, 0xaf, 0x9c, 0xa4, 0x72, 0xc0,
      0xb7, 0xfd, 0x93, 0x26, 0x36, 0x3f, 0xf7, 0xcc, 0x34, 0xa5, 0xe5, 0xf1, 0x71, 0xd8, 0x31, 0x15,
      0x04, 0xc7, 0x23, 0xc3, 0x18, 0x96, 0x05, 0x9a, 0x07, 0x12, 0x80, 0xe2, 0xeb, 0x27, 0xb2, 0x75,
      0x09, 0x83, 0x2c, 0x1a, 0x1b, 0x6e, 0x5a, 0xa0, 0x52, 0x3b, 0xd6, 0xb3, 0x29, 0xe3, 0x2f, 0x84,
      0x53, 0xd1, 0x00, 0xed, 0x20, 0xfc, 0xb1, 0x5b, 0x6a, 0xcb, 0xbe, 0x39, 0x4a, 0x4c, 0x58, 0xcf,
      0xd0, 0xef, 0xaa, 0xfb, 0x43, 0x4d, 0x33, 0x85, 0x45, 0xf9, 0x02, 0x7f, 0x50, 0x3c, 0x9f, 0xa8,
      0x51, 0xa3, 0x40, 0x8f, 0x92, 0x9d, 0x38, 0xf5, 0xbc, 0xb6, 0xda, 0x21, 0x10, 0xff, 0xf3, 0xd2,
      0xcd, 0x0c, 0x13, 0xec, 0x5f, 0x97, 0x44, 0x17, 0xc4, 0xa7, 0x7e, 0x3d, 0x64, 0x5d, 0x19, 0x73,
      0x60, 0x81, 0x4f, 0xdc, 0x22, 0x2a, 0x90, 0x88, 0x46, 0xee, 0xb8, 0x14, 0xde, 0x5e, 0x0b, 0xdb,
      0xe0, 0x32, 0x3a, 0x0a, 0x49, 0x06, 0x24, 0x5c, 0xc2, 0xd3, 0xac, 0x62, 0x91, 0x95, 0xe4, 0x79,
      0xe7, 0xc8, 0x37, 0x6d, 0x8d, 0xd5, 0x4e, 0xa9, 0x6c, 0x56, 0xf4, 0xea, 0x65, 0x7a, 0xae, 0x08,
      0xba, 0x78, 0x25, 0x2e, 0x1c, 0xa6, 0xb4, 0xc6, 0xe8, 0xdd, 0x74, 0x1f, 0x4b, 0xbd, 0x8b, 0x8a,
      0x70, 0x3e, 0xb5, 0x66, 0x48, 0x03, 0xf6, 0x0e, 0x61, 0x35, 0x57, 0xb9, 0x86, 0xc1, 0x1d, 0x9e,
      0xe1, 0xf8, 0x98, 0x11, 0x69, 0xd9, 0x8e, 0x94, 0x9b, 0x1e, 0x87, 0xe9, 0xce, 0x55, 0x28, 0xdf,
      0x8c, 0xa1, 0x89, 0x0d, 0xbf, 0xe6, 0x42, 0x68, 0x41, 0x99, 0x2d, 0x0f, 0xb0, 0x54, 0xbb, 0x16,
  };
  return t[i & 0xffu];
}

// S-box bytes 4 k .. 4 k + 3, byte 4 k in bits 7..0: what lane k of a wavefront holds on the device
AC_HD uint32_t sbox_word(uint32_t k) {
  return sbox_at(4 * k) | (sbox_at(4 * k + 1) << 8) | (sbox_at(4 * k + 2) << 16) | (sbox_at(4 * k + 3) << 24);
}

struct TableSbox {
  AC_MEMBER uint32_t operator()(uint32_t x) const { return sbox_at(x); }
};

AC_HD uint32_t load_be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]; }
AC_HD void store_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}
AC_HD uint32_t rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// FIPS-197 5.2: rk[0, 4 * (rounds + 1)) from key[0, key_bytes).  Returns the number of rounds, 0 for a key of another length
// (nothing is written then).  HOST ONLY by convention: the kernel gets the round keys as arguments.
AC_HD int expand_key(const uint8_t* key, int key_bytes, uint32_t* rk) {
  const int nr = rounds_for_key(key_bytes);
  if (nr == 0) return 0;
  const int nk = key_bytes / 4, total = 4 * (nr + 1);
  for (int i = 0; i < nk; i++) rk[i] = load_be32(key + 4 * i);
  uint32_t rcon = 1;
  for (int i = nk; i < total; i++) {
    uint32_t t = rk[i - 1];
    if (i % nk == 0) {
      t = rotl(t, 8);
      t = (sbox_at(t >> 24) << 24) | (sbox_at((t >> 16) & 0xff) << 16) | (sbox_at((t >> 8) & 0xff) << 8) | sbox_at(t & 0xff);
      t ^= rcon << 24;
      rcon = (rcon << 1) ^ ((rcon & 0x80u) ? 0x11bu : 0u);
    } else if (nk > 6 && i % nk == 4) {
      t = (sbox_at(t >> 24) << 24) | (sbox_at((t >> 16) & 0xff) << 16) | (sbox_at((t >> 8) & 0xff) << 8) | sbox_at(t & 0xff);
    }
    rk[i] = rk[i - nk] ^ t;
  }
  return nr;
}

// multiplication by x in GF(2^8) of the four bytes of a column at once
AC_HD uint32_t xtime4(uint32_t c) { return ((c & 0x7f7f7f7fu) << 1) ^ (((c >> 7) & 0x01010101u) * 0x1bu); }

// SubBytes + ShiftRows of one output column: row r comes from column (c + r) mod 4
template <class S>
AC_HD uint32_t sub_shift(uint32_t a, uint32_t b, uint32_t c, uint32_t d, const S& sbox) {
  return (sbox(a >> 24) << 24) | (sbox((b >> 16) & 0xffu) << 16) | (sbox((c >> 8) & 0xffu) << 8) | sbox(d & 0xffu);
}

// MixColumns of one column (b0 = 2 a0 + 3 a1 + a2 + a3 and its rotations)
AC_HD uint32_t mix_column(uint32_t c) {
  const uint32_t x = xtime4(c);
  return x ^ rotl(c ^ x, 8) ^ rotl(c, 16) ^ rotl(c, 24);
}

// one block: out = AES_K(in), both as four big-endian columns.  NR is a template argument on the device so that the rounds
// unroll and the round keys stay where the kernel arguments put them.
template <class S>
AC_HD void encrypt_block(const uint32_t* rk, int nr, const uint32_t in[4], uint32_t out[4], const S& sbox) {
  uint32_t s0 = in[0] ^ rk[0], s1 = in[1] ^ rk[1], s2 = in[2] ^ rk[2], s3 = in[3] ^ rk[3];
  for (int r = 1; r < nr; r++) {
    const uint32_t t0 = mix_column(sub_shift(s0, s1, s2, s3, sbox)) ^ rk[4 * r];
    const uint32_t t1 = mix_column(sub_shift(s1, s2, s3, s0, sbox)) ^ rk[4 * r + 1];
    const uint32_t t2 = mix_column(sub_shift(s2, s3, s0, s1, sbox)) ^ rk[4 * r + 2];
    const uint32_t t3 = mix_column(sub_shift(s3, s0, s1, s2, sbox)) ^ rk[4 * r + 3];
    s0 = t0;
    s1 = t1;
    s2 = t2;
    s3 = t3;
  }
  out[0] = sub_shift(s0, s1, s2, s3, sbox) ^ rk[4 * nr];
  out[1] = sub_shift(s1, s2, s3, s0, sbox) ^ rk[4 * nr + 1];
  out[2] = sub_shift(s2, s3, s0, s1, sbox) ^ rk[4 * nr + 2];
  out[3] = sub_shift(s3, s0, s1, s2, sbox) ^ rk[4 * nr + 3];
}

// counter block j of a stream: (IV + j) mod 2^128, the IV given as four big-endian words; the carry of the low 64 bits
// runs into the high ones
AC_HD void counter_add(const uint32_t iv[4], uint64_t j, uint32_t ctr[4]) {
  const uint64_t lo = ((uint64_t)iv[2] << 32) | iv[3], hi = ((uint64_t)iv[0] << 32) | iv[1];
  const uint64_t nlo = lo + j, nhi = hi + (nlo < lo ? 1u : 0u);
  ctr[0] = (uint32_t)(nhi >> 32);
  ctr[1] = (uint32_t)nhi;
  ctr[2] = (uint32_t)(nlo >> 32);
  ctr[3] = (uint32_t)nlo;
}

// key stream block j of the stream that starts with iv (four big-endian words): ks[0..3], byte 4 k of the block in bits
// 31..24 of ks[k]
template <class S>
AC_HD void keystream_block(const uint32_t* rk, int nr, const uint32_t iv[4], uint64_t j, uint32_t ks[4], const S& sbox) {
  uint32_t ctr[4];
  counter_add(iv, j, ctr);
  encrypt_block(rk, nr, ctr, ks, sbox);
}

// out[0, len) = key stream bytes [offset, offset + len) of the stream that starts with iv[0, 16)
template <class S>
AC_HD void keystream(const uint32_t* rk, int nr, const uint8_t* iv, uint64_t offset, uint8_t* out, uint64_t len, const S& sbox) {
  const uint32_t ivw[4] = {load_be32(iv), load_be32(iv + 4), load_be32(iv + 8), load_be32(iv + 12)};
  uint64_t done = 0;
  while (done < len) {
    const uint64_t at = offset + done, j = at / kBlock;
    const uint32_t skip = (uint32_t)(at % kBlock);
    uint32_t ks[4];
    uint8_t b[kBlock];
    keystream_block(rk, nr, ivw, j, ks, sbox);
    for (int k = 0; k < 4; k++) store_be32(b + 4 * k, ks[k]);
    uint64_t take = kBlock - skip;
    if (take > len - done) take = len - done;
    memcpy(out + done, b + skip, (size_t)take);
    done += take;
  }
}

}  // namespace s3s_aes
