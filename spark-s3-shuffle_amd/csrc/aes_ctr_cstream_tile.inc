// aes_ctr_cstream_tile.inc — one tile of the map-side stream's AES-CTR pass: the body of aes_ctr_cstream_kernel
// (aes_ctr_cstream.hip) and of aes_ctr_cstream_batch_kernel (aes_ctr_cstream_batch.hip), shared as TEXT so that both kernels
// are compiled from the same statements in their own context (an inlined function changed the single kernel's schedule, as it
// did for aes_ctr_window_tile.inc).  The including kernel provides:
//   keys, NR, MODE               the round keys (a kernel argument), the rounds, kCsInPlace / kCsFromPlain
//   src, out, E, Q, ivs, n       what launch_aes_ctr_cstream documents (s3s_internal.h); src and Q are read by kCsFromPlain only
//   front, L                     stored bytes of the open partition in front of the output; the output's length
//   S3S_CS_TILE                  the tile of THIS output the workgroup owns
  const int64_t tile0 = s3s_aes::win_chunk_start((int64_t)(S3S_CS_TILE) * kCsTileChunks, front);
  if (L <= 0 || tile0 >= L) return;  // the whole workgroup
  const int64_t tile_end = tile0 + kCsTile < L ? tile0 + kCsTile : L;
  const LaneSbox sbox{s3s_aes::sbox_word(threadIdx.x & 63u)};
  const int32_t p_lo = s3s_aes::win_last_start_le(E, 0, n - 1, tile0), p_hi = s3s_aes::win_last_start_le(E, p_lo, n - 1, tile_end - 1);

  for (int k = 0; k < kCsChunks; k++) {
    const int64_t x0 = tile0 + 16 * ((int64_t)threadIdx.x + (int64_t)kCsThreads * k);
    const bool live = x0 < tile_end;
    const int64_t lim = x0 + 16 < tile_end ? x0 + 16 : tile_end;
    s3s_aes::WinCursor c;
    s3s_aes::win_open(c, E, s3s_aes::win_last_start_le(E, p_lo, p_hi, x0), front, x0);
    for (;;) {
      s3s_aes::WinUnit u;
      const bool has = s3s_aes::win_next(c, E, n, L, lim, live, u);
      if (__builtin_amdgcn_ballot_w64(has) == 0) break;  // wave-uniform: every lane stays for the block encryption
      const bool work = has && u.len > 0;
      uint32_t ivw[4] = {0, 0, 0, 0};
      const uint8_t* ivp = ivs + 16 * (int64_t)u.part;  // (entry 0: the open partition's carried IV when front > 0)
      if (work) {
        __builtin_memcpy(ivw, ivp, 16);
#pragma unroll
        for (int w = 0; w < 4; w++) ivw[w] = __builtin_bswap32(ivw[w]);
      }
      uint32_t ks[4];
      s3s_aes::keystream_block(keys.rk, NR, ivw, (uint64_t)u.block, ks, sbox);
      if (work) {
        if (u.is_iv) {  // whole (len 16): into the hole
          uint8_t* d = out + u.start;
          for (int i = 0; i < 16; i++) d[i] = ivp[i];
        } else {
          uint8_t* d = out + (u.start + u.skip);
          const uint8_t* s = MODE == kCsInPlace ? d : src + (Q[u.part] - (u.part == 0 && front > 0 ? front - 16 : 0) + u.plain);
          if (u.len == 16) {
            uint32_t v[4];
            __builtin_memcpy(v, s, 16);
#pragma unroll
            for (int w = 0; w < 4; w++) v[w] ^= __builtin_bswap32(ks[w]);
            __builtin_memcpy(d, v, 16);
          } else {
            for (int i = 0; i < u.len; i++) {
              const int b = u.skip + i;
              d[i] = (uint8_t)(s[i] ^ (ks[b >> 2] >> (24 - 8 * (b & 3))));
            }
          }
        }
      }
    }
  }
