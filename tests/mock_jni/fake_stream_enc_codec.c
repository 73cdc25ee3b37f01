/* A stand-in for s3s_dstream_open_encrypted on a box without a GPU (TEST INFRASTRUCTURE, linked next to fake_codec.c and
 * fake_stream_codec.c by tests/test_decode_stream_encrypted_cpu.py): the toy stream of fake_stream_codec.c behind the entry
 * point's own rule - the layer must be on - with a count of the calls that reached it, so that the harness can tell that the
 * native called THIS entry point and that a refused call never got to the library.  Nothing of the product links this file. */
#include <stddef.h>

#include "s3shuffle_codec.h"

static int g_layer_on = 0, g_opens = 0;

void fake_enc_layer(int on) { g_layer_on = on; }
int fake_enc_opens(void) { return g_opens; }

int s3s_dstream_open_encrypted(s3s_ctx* ctx, int codec, int algo, const int64_t* po, const int64_t* rs, int32_t nparts, s3s_dstream** out) {
  g_opens++;
  if (out) *out = NULL;
  if (!ctx || !out || !po) return S3S_E_INVALID;
  if (!g_layer_on) return S3S_E_INVALID;
  return s3s_dstream_open(ctx, codec, algo, po, rs, nparts, out);
}
