// aes_ctr_window_tile.inc — one tile of one window of the AES-CTR window pass: the statements shared by
// aes_ctr_window_kernel (aes_ctr_stream.hip, one window per launch) and aes_ctr_window_batch_kernel
// (aes_ctr_stream_batch.hip, the windows of a batched feed in one launch).  Included as the BODY of either kernel, which
// provides keys, iv0, in, out, E, Q, iv_out, n, front and L under these names and S3S_WIN_TILE, the workgroup's tile inside
// its window.  Text, not a function: the single kernel compiles to the instructions it had before the body was shared (an
// inlined function changed its schedule).
  const int64_t tile0 = s3s_aes::win_chunk_start((int64_t)S3S_WIN_TILE * kWinTileChunks, front);
  if (tile0 >= L) return;  // the whole workgroup
  const int64_t tile_end = tile0 + kWinTile < L ? tile0 + kWinTile : L;
  const LaneSbox sbox{s3s_aes::sbox_word(threadIdx.x & 63u)};
  const int32_t p_lo = s3s_aes::win_last_start_le(E, 0, n - 1, tile0), p_hi = s3s_aes::win_last_start_le(E, p_lo, n - 1, tile_end - 1);

  for (int k = 0; k < kWinChunks; k++) {
    const int64_t x0 = tile0 + 16 * ((int64_t)threadIdx.x + (int64_t)kWinThreads * k);
    const bool live = x0 < tile_end;
    const int64_t lim = x0 + 16 < tile_end ? x0 + 16 : tile_end;
    s3s_aes::WinCursor c;
    s3s_aes::win_open(c, E, s3s_aes::win_last_start_le(E, p_lo, p_hi, x0), front, x0);
    for (;;) {
      s3s_aes::WinUnit u;
      const bool has = s3s_aes::win_next(c, E, n, L, lim, live, u);
      if (__builtin_amdgcn_ballot_w64(has) == 0) break;  // wave-uniform: every lane stays for the block encryption
      const bool carried = u.part == 0 && front > 0;      // piece 0's IV came by in an earlier feed
      const bool work = has && u.len > 0;
      uint32_t ivw[4] = {iv0.w[0], iv0.w[1], iv0.w[2], iv0.w[3]};
      const uint8_t* ivp = in + (carried ? 0 : E[u.part]);
      if (work && !carried) {
        __builtin_memcpy(ivw, ivp, 16);
#pragma unroll
        for (int w = 0; w < 4; w++) ivw[w] = __builtin_bswap32(ivw[w]);
      }
      uint32_t ks[4];
      s3s_aes::keystream_block(keys.rk, NR, ivw, (uint64_t)u.block, ks, sbox);
      if (work) {
        if (u.is_iv) {  // whole (len 16): gathered for the host, dropped from the plain bytes
          uint8_t* d = iv_out + 16 * (int64_t)u.part;
          for (int i = 0; i < 16; i++) d[i] = ivp[i];
        } else {
          const uint8_t* s = in + (u.start + u.skip);
          uint8_t* d = out + (Q[u.part] - (carried ? front - 16 : 0) + u.plain);
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
