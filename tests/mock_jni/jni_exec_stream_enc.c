/* Executes dstreamOpenEncrypted of jni/s3s_jni.c against the mock JNIEnv of mock_jvm.h, the way S3GpuStreamingInputStream.open
 * calls it on a context with a key (TEST INFRASTRUCTURE; tests/test_decode_stream_encrypted_cpu.py builds and runs it with
 * fake_codec.c + fake_stream_codec.c + fake_stream_enc_codec.c under ASan / UBSan).  The native makes the argument checks of
 * dstreamOpen - a call they refuse never reaches the library - and after every call no array may still be pinned. */
#include <stdio.h>
#include <string.h>

#include "mock_jvm.h"
#include "s3shuffle_codec.h"

#define FN(name) Java_org_apache_spark_shuffle_gpu_S3SCodec_00024_##name
#define CHECK(x)                                            \
  do {                                                      \
    if (!(x)) {                                             \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
      fflush(stdout);                                       \
      return 1;                                             \
    }                                                       \
  } while (0)
#define CLEAN() CHECK(mj_outstanding() == 0)

jlong FN(create)(JNIEnv*, jclass, jint, jlong);
void FN(destroy)(JNIEnv*, jclass, jlong);
jobject FN(hostAlloc)(JNIEnv*, jclass, jlong);
void FN(hostFree)(JNIEnv*, jclass, jobject);
jint FN(dstreamOpen)(JNIEnv*, jclass, jlong, jint, jint, jlongArray, jlongArray, jint, jlongArray);
jint FN(dstreamOpenEncrypted)(JNIEnv*, jclass, jlong, jint, jint, jlongArray, jlongArray, jint, jlongArray);
jint FN(dstreamFeed)(JNIEnv*, jclass, jlong, jobject, jlong, jlong, jobject, jlong, jlongArray);
jlong FN(dstreamPosition)(JNIEnv*, jclass, jlong);
jint FN(dstreamClose)(JNIEnv*, jclass, jlong);
int64_t fake_stream_ref(const s3s_dstream* s, int i);
int64_t fake_stream_off(const s3s_dstream* s, int i);
void fake_enc_layer(int on);
int fake_enc_opens(void);

int main(void) {
  JNIEnv* e = &mj_env;
  const jlong h = FN(create)(e, NULL, 0, 0);
  CHECK(h != 0);
  jlongArray off = mj_longs(3), ref = mj_longs(2), os = mj_longs(1), out = mj_longs(6), none = mj_longs(0), one = mj_longs(1);
  mj_l(off)[0] = 0; mj_l(off)[1] = 25; mj_l(off)[2] = 52; /* stored offsets: 16 + 9, 16 + 11 */
  mj_l(ref)[0] = 333; mj_l(ref)[1] = 444;
  /* ---- the layer is off: the library's E_INVALID comes back, no stream ---- */
  mj_l(os)[0] = -7;
  CHECK(FN(dstreamOpenEncrypted)(e, NULL, h, S3S_CODEC_LZ4, S3S_CHECKSUM_CRC32, off, ref, 2, os) == S3S_E_INVALID);
  CHECK(mj_l(os)[0] == 0 && fake_enc_opens() == 1);
  CLEAN();
  fake_enc_layer(1);
  CHECK(FN(dstreamOpenEncrypted)(e, NULL, h, S3S_CODEC_ZSTD, S3S_CHECKSUM_CRC32, off, ref, 2, os) == S3S_E_UNSUPPORTED);
  CHECK(mj_l(os)[0] == 0 && fake_enc_opens() == 2);
  CLEAN();
  /* ---- the argument checks of dstreamOpen: arrays shorter than nparts says, no room for the handle - never the library ---- */
  CHECK(FN(dstreamOpenEncrypted)(e, NULL, h, S3S_CODEC_LZ4, S3S_CHECKSUM_CRC32, off, ref, 3, os) == S3S_E_INVALID);
  CHECK(FN(dstreamOpenEncrypted)(e, NULL, h, S3S_CODEC_LZ4, S3S_CHECKSUM_CRC32, off, one, 2, os) == S3S_E_INVALID);
  CHECK(FN(dstreamOpenEncrypted)(e, NULL, h, S3S_CODEC_LZ4, S3S_CHECKSUM_CRC32, one, NULL, 1, os) == S3S_E_INVALID);
  CHECK(FN(dstreamOpenEncrypted)(e, NULL, h, S3S_CODEC_LZ4, S3S_CHECKSUM_CRC32, off, ref, 2, none) == S3S_E_INVALID);
  CHECK(FN(dstreamOpenEncrypted)(e, NULL, h, S3S_CODEC_LZ4, S3S_CHECKSUM_CRC32, off, ref, 2, NULL) == S3S_E_INVALID);
  CHECK(fake_enc_opens() == 2);
  CLEAN();
  /* ---- open: THIS entry point is called; offsets and reference checksums reach their arguments; the stream comes back ---- */
  CHECK(FN(dstreamOpenEncrypted)(e, NULL, h, S3S_CODEC_LZ4, S3S_CHECKSUM_CRC32, off, ref, 2, os) == S3S_OK);
  CLEAN();
  CHECK(fake_enc_opens() == 3);
  const jlong st = mj_l(os)[0];
  CHECK(st != 0);
  const s3s_dstream* s = (const s3s_dstream*)(intptr_t)st;
  CHECK(fake_stream_off(s, 1) == 25 && fake_stream_off(s, 2) == 52 && fake_stream_ref(s, 0) == 333 && fake_stream_ref(s, 1) == 444);
  /* the stream is an ordinary one to the other natives */
  jobject comp = FN(hostAlloc)(e, NULL, 64), dst = FN(hostAlloc)(e, NULL, 64);
  CHECK(comp && dst);
  for (int i = 0; i < 64; i++) ((uint8_t*)comp->data)[i] = (uint8_t)(i + 1);
  CHECK(FN(dstreamFeed)(e, NULL, st, comp, 0, 52, dst, 64, out) == S3S_OK && mj_l(out)[0] == 7);
  CHECK(FN(dstreamPosition)(e, NULL, st) == 7);
  CHECK(FN(dstreamClose)(e, NULL, st) == S3S_E_BAD_FRAME);
  CLEAN();
  CHECK(FN(dstreamOpenEncrypted)(e, NULL, h, S3S_CODEC_NONE, S3S_CHECKSUM_NONE, off, NULL, 2, os) == S3S_OK); /* no reference checksums */
  CHECK(mj_l(os)[0] != 0 && FN(dstreamClose)(e, NULL, mj_l(os)[0]) == S3S_E_BAD_FRAME);
  /* the plain open does not go through it */
  CHECK(FN(dstreamOpen)(e, NULL, h, S3S_CODEC_NONE, S3S_CHECKSUM_NONE, off, NULL, 2, os) == S3S_OK && fake_enc_opens() == 4);
  CHECK(FN(dstreamClose)(e, NULL, mj_l(os)[0]) == S3S_E_BAD_FRAME);
  CLEAN();
  FN(hostFree)(e, NULL, comp);
  FN(hostFree)(e, NULL, dst);
  mj_free(comp); mj_free(dst);
  mj_free(off); mj_free(ref); mj_free(os); mj_free(out); mj_free(none); mj_free(one);
  FN(destroy)(e, NULL, h);
  CLEAN();
  printf("jni_exec_stream_enc ok\n");
  return 0;
}
