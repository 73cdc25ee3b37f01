/* Executes the stream natives of jni/s3s_jni.c (dstreamOpen / dstreamFeed / dstreamPosition / dstreamClose /
 * checksumRangesSeeded) against the mock JNIEnv of mock_jvm.h, the way S3GpuStreamingInputStream calls them (TEST
 * INFRASTRUCTURE; tests/test_decode_stream_cpu.py builds and runs it with fake_codec.c + fake_stream_codec.c under ASan / UBSan).
 * After every native call no array may still be pinned and no local reference may be left. */
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
jint FN(dstreamFeed)(JNIEnv*, jclass, jlong, jobject, jlong, jlong, jobject, jlong, jlongArray);
jlong FN(dstreamPosition)(JNIEnv*, jclass, jlong);
jint FN(dstreamClose)(JNIEnv*, jclass, jlong);
jint FN(checksumRangesSeeded)(JNIEnv*, jclass, jlong, jint, jobject, jlongArray, jint, jlongArray, jlongArray);
int64_t fake_stream_ref(const s3s_dstream* s, int i);
int64_t fake_stream_off(const s3s_dstream* s, int i);

int main(void) {
  JNIEnv* e = &mj_env;
  const jlong h = FN(create)(e, NULL, 0, 0);
  CHECK(h != 0);
  /* ---- open: offsets and reference checksums reach their arguments, the stream comes back through outStream ---- */
  jlongArray off = mj_longs(3), ref = mj_longs(2), os = mj_longs(1), out = mj_longs(6);
  mj_l(off)[0] = 0; mj_l(off)[1] = 9; mj_l(off)[2] = 20;
  mj_l(ref)[0] = 111; mj_l(ref)[1] = 222;
  CHECK(FN(dstreamOpen)(e, NULL, h, S3S_CODEC_ZSTD, S3S_CHECKSUM_CRC32, off, ref, 2, os) == S3S_E_UNSUPPORTED);
  CHECK(mj_l(os)[0] == 0);
  CLEAN();
  CHECK(FN(dstreamOpen)(e, NULL, h, S3S_CODEC_LZ4, S3S_CHECKSUM_CRC32, off, ref, 3, os) == S3S_E_INVALID); /* arrays shorter than nparts says */
  CLEAN();
  jlongArray none = mj_longs(0);
  CHECK(FN(dstreamOpen)(e, NULL, h, S3S_CODEC_LZ4, S3S_CHECKSUM_CRC32, off, ref, 2, none) == S3S_E_INVALID);
  CLEAN();
  CHECK(FN(dstreamOpen)(e, NULL, h, S3S_CODEC_LZ4, S3S_CHECKSUM_CRC32, off, ref, 2, os) == S3S_OK);
  CLEAN();
  const jlong st = mj_l(os)[0];
  CHECK(st != 0);
  const s3s_dstream* s = (const s3s_dstream*)(intptr_t)st;
  CHECK(fake_stream_off(s, 1) == 9 && fake_stream_off(s, 2) == 20 && fake_stream_ref(s, 0) == 111 && fake_stream_ref(s, 1) == 222);
  CHECK(FN(dstreamPosition)(e, NULL, st) == 0);
  /* ---- feed: the window is comp[compOff, compOff + compLen) of a direct buffer; all six result words are copied back ---- */
  jobject comp = FN(hostAlloc)(e, NULL, 64), dst = FN(hostAlloc)(e, NULL, 64);
  CHECK(comp && dst);
  uint8_t* cp = (uint8_t*)comp->data;
  uint8_t* dp = (uint8_t*)dst->data;
  for (int i = 0; i < 64; i++) cp[i] = (uint8_t)(i + 1);
  memset(dp, 0, 64);
  for (int i = 0; i < 6; i++) mj_l(out)[i] = -99;
  CHECK(FN(dstreamFeed)(e, NULL, st, comp, 30, 20, dst, 64, out) == S3S_OK);
  CLEAN();
  CHECK(mj_l(out)[0] == 7 && mj_l(out)[1] == 7 && mj_l(out)[2] == 0 && mj_l(out)[3] == 0 && mj_l(out)[4] == -1 && mj_l(out)[5] == 0);
  for (int i = 0; i < 7; i++) CHECK(dp[i] == ((30 + i + 1) ^ 0x5A)); /* compOff was applied */
  CHECK(FN(dstreamPosition)(e, NULL, st) == 7);
  CHECK(FN(dstreamFeed)(e, NULL, st, comp, 0, 13, dst, 0, out) == S3S_E_CAPACITY); /* need_dst comes back with the code */
  CLEAN();
  CHECK(mj_l(out)[0] == 0 && mj_l(out)[3] == 1);
  CHECK(FN(dstreamFeed)(e, NULL, st, comp, 0, 0, dst, 64, out) == S3S_OK); /* an empty window: need_comp */
  CHECK(mj_l(out)[0] == 0 && mj_l(out)[2] == 1);
  CHECK(FN(dstreamFeed)(e, NULL, st, comp, 0, 14, dst, 64, out) == S3S_E_INVALID); /* past the end of the range */
  CLEAN();
  jlongArray five = mj_longs(5);
  CHECK(FN(dstreamFeed)(e, NULL, st, comp, 0, 13, dst, 64, five) == S3S_E_INVALID); /* a result array that is too short is never written */
  CHECK(FN(dstreamFeed)(e, NULL, st, comp, -1, 13, dst, 64, out) == S3S_E_INVALID);
  /* a window or a capacity that reaches past its direct buffer (64 bytes each) never gets to the library */
  for (int i = 0; i < 6; i++) mj_l(out)[i] = -99;
  CHECK(FN(dstreamFeed)(e, NULL, st, comp, 60, 5, dst, 64, out) == S3S_E_INVALID);
  CHECK(FN(dstreamFeed)(e, NULL, st, comp, 65, 0, dst, 64, out) == S3S_E_INVALID);
  CHECK(FN(dstreamFeed)(e, NULL, st, comp, 0, -1, dst, 64, out) == S3S_E_INVALID);
  CHECK(FN(dstreamFeed)(e, NULL, st, comp, 0, 13, dst, 65, out) == S3S_E_INVALID);
  CHECK(FN(dstreamFeed)(e, NULL, st, comp, 0, 13, NULL, 64, out) == S3S_E_INVALID);
  CHECK(FN(dstreamFeed)(e, NULL, st, NULL, 0, 13, dst, 64, out) == S3S_E_INVALID);
  CHECK(mj_l(out)[0] == -99 && FN(dstreamPosition)(e, NULL, st) == 7);
  CLEAN();
  cp[3] = 0xEE;
  CHECK(FN(dstreamFeed)(e, NULL, st, comp, 0, 13, dst, 64, out) == S3S_E_CHECKSUM); /* bad_partition is copied back on an error */
  CLEAN();
  CHECK(mj_l(out)[4] == 1 && mj_l(out)[0] == 0 && mj_l(out)[1] == 0);
  cp[3] = 4;
  CHECK(FN(dstreamFeed)(e, NULL, st, comp, 0, 13, dst, 64, out) == S3S_OK && mj_l(out)[0] == 7 && mj_l(out)[5] == 0);
  CHECK(FN(dstreamClose)(e, NULL, st) == S3S_E_BAD_FRAME); /* closed 6 bytes before the end */
  CLEAN();
  CHECK(FN(dstreamOpen)(e, NULL, h, S3S_CODEC_NONE, S3S_CHECKSUM_NONE, off, NULL, 2, os) == S3S_OK); /* no reference checksums */
  const jlong st2 = mj_l(os)[0];
  int feeds = 0;
  for (jlong pos = 0; pos < 20; pos += mj_l(out)[0], feeds++) CHECK(FN(dstreamFeed)(e, NULL, st2, comp, pos, 20 - pos, dst, 64, out) == S3S_OK);
  CHECK(feeds == 3 && mj_l(out)[5] == 1 && FN(dstreamPosition)(e, NULL, st2) == 20);
  CHECK(FN(dstreamClose)(e, NULL, st2) == S3S_OK);
  CLEAN();
  /* ---- seeded checksums: seeds and offsets are inputs (not copied back), out is copied back ---- */
  jlongArray co = mj_longs(3), seeds = mj_longs(2), sums = mj_longs(2);
  mj_l(co)[0] = 0; mj_l(co)[1] = 2; mj_l(co)[2] = 3;
  mj_l(seeds)[0] = 1000; mj_l(seeds)[1] = 5;
  CHECK(FN(checksumRangesSeeded)(e, NULL, h, 2, comp, co, 2, seeds, sums) == S3S_OK);
  CLEAN();
  CHECK(mj_l(sums)[0] == 1000 + 1 + 2 && mj_l(sums)[1] == 5 + 3 && mj_l(seeds)[0] == 1000);
  CHECK(FN(checksumRangesSeeded)(e, NULL, h, 2, comp, co, 2, NULL, sums) == S3S_OK); /* seeds == null: fresh */
  CHECK(mj_l(sums)[0] == 2 + 1 + 2);
  jlongArray one = mj_longs(1);
  CHECK(FN(checksumRangesSeeded)(e, NULL, h, 2, comp, co, 2, one, sums) == S3S_E_INVALID); /* fewer seeds than ranges */
  CLEAN();
  CHECK(FN(checksumRangesSeeded)(e, NULL, h, 2, comp, co, 2, seeds, one) == S3S_E_INVALID); /* fewer results than ranges */
  CHECK(FN(checksumRangesSeeded)(e, NULL, h, 2, comp, co, 3, NULL, sums) == S3S_E_INVALID); /* fewer offsets than n + 1 */
  mj_l(co)[2] = 65;
  CHECK(FN(checksumRangesSeeded)(e, NULL, h, 2, comp, co, 2, seeds, sums) == S3S_E_INVALID); /* the last range ends behind the buffer */
  CLEAN();
  FN(hostFree)(e, NULL, comp);
  FN(hostFree)(e, NULL, dst);
  mj_free(comp); mj_free(dst);
  mj_free(off); mj_free(ref); mj_free(os); mj_free(out); mj_free(none); mj_free(five); mj_free(co); mj_free(seeds); mj_free(sums); mj_free(one);
  FN(destroy)(e, NULL, h);
  CLEAN();
  printf("jni_exec_stream ok\n");
  return 0;
}
