/* A stand-in for the stream entry points of libs3shuffle_codec on a box without a GPU (TEST INFRASTRUCTURE, linked next to
 * fake_codec.c by tests/test_decode_stream_cpu.py): s3s_dstream_* and s3s_checksum_ranges_seeded with a toy "codec" - a unit is
 * a byte, decoded = byte xor 0x5A, at most 7 bytes per feed - that records what it was given, so that the harness can tell
 * which Java array reached which argument.  Nothing of the product links or loads this file. */
#include <stdlib.h>
#include <string.h>

#include "s3shuffle_codec.h"

struct s3s_dstream {
  s3s_ctx* ctx;
  int codec, algo;
  int32_t nparts;
  int64_t off[8], ref[8], pos;
};

int s3s_dstream_open(s3s_ctx* ctx, int codec, int algo, const int64_t* po, const int64_t* rs, int32_t nparts, s3s_dstream** out) {
  if (!ctx || !out || !po || nparts < 0 || nparts > 7) return S3S_E_INVALID;
  *out = NULL;
  if (codec == S3S_CODEC_ZSTD) return S3S_E_UNSUPPORTED;
  s3s_dstream* s = (s3s_dstream*)calloc(1, sizeof *s);
  s->ctx = ctx;
  s->codec = codec;
  s->algo = algo;
  s->nparts = nparts;
  memcpy(s->off, po, sizeof(int64_t) * (size_t)(nparts + 1));
  if (rs) memcpy(s->ref, rs, sizeof(int64_t) * (size_t)nparts);
  *out = s;
  return S3S_OK;
}
int s3s_dstream_feed(s3s_dstream* s, const uint8_t* comp, int64_t n, uint8_t* dst, int64_t cap, s3s_dstream_result* r) {
  if (!s || !r) return S3S_E_INVALID;
  memset(r, 0, sizeof *r);
  r->bad_partition = -1;
  const int64_t total = s->off[s->nparts];
  if (n > total - s->pos) return S3S_E_INVALID;
  if (n > 0 && cap == 0) {
    r->need_dst = 1;
    return S3S_E_CAPACITY;
  }
  if (n == 0 && s->pos < total) {
    r->need_comp = 1;
    return S3S_OK;
  }
  int64_t k = n < cap ? n : cap;
  if (k > 7) k = 7;
  for (int64_t i = 0; i < k; i++) {
    if (comp[i] == 0xEE) { /* the toy's corrupt byte: "partition 1 has a wrong checksum" */
      r->bad_partition = 1;
      return S3S_E_CHECKSUM;
    }
    dst[i] = comp[i] ^ 0x5A;
  }
  s->pos += k;
  r->consumed = r->out_len = k;
  r->at_end = s->pos == total;
  return S3S_OK;
}
int64_t s3s_dstream_position(const s3s_dstream* s) { return s ? s->pos : S3S_E_INVALID; }
int s3s_dstream_close(s3s_dstream* s) {
  if (!s) return S3S_E_INVALID;
  const int rc = s->pos == s->off[s->nparts] ? S3S_OK : S3S_E_BAD_FRAME;
  free(s);
  return rc;
}
/* toy checksum continued: out[i] = seeds[i] + the sum of the range's bytes; without seeds the state starts at `algo` */
int s3s_checksum_ranges_seeded(s3s_ctx* c, int algo, const uint8_t* d, const int64_t* o, int32_t n, const int64_t* seeds, int64_t* out) {
  if (!c || !o || (n > 0 && !out)) return S3S_E_INVALID;
  for (int32_t i = 0; i < n; i++) {
    int64_t s = seeds ? seeds[i] : algo;
    for (int64_t j = o[i]; j < o[i + 1]; j++) s += d[j];
    out[i] = s;
  }
  return S3S_OK;
}
/* what the harness reads back to see which array reached which argument */
int64_t fake_stream_ref(const s3s_dstream* s, int i) { return s->ref[i]; }
int64_t fake_stream_off(const s3s_dstream* s, int i) { return s->off[i]; }
