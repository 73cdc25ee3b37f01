/* s3s_jni.c — JNI translation unit between org.apache.spark.shuffle.gpu.S3SCodec (scala/…/S3SCodec.scala) and the
 * C-ABI in include/s3shuffle_codec.h.  Logic-free on purpose: every function pins its arrays, forwards to the
 * entry point of the same name and releases the arrays; error codes go back as the int result and are mapped to
 * the reference's exceptions by the Scala side.
 *
 * What it binds into:
 *   map side     S3ShuffleMapOutputWriter.commitAllPartitions      shuffle/S3ShuffleMapOutputWriter.scala:91-118
 *                S3ShuffleOutputStream.write (staging)             shuffle/S3ShuffleMapOutputWriter.scala:168-202
 *                S3SingleSpillShuffleMapOutputWriter.transferMapSpillFile
 *                                                                  shuffle/S3SingleSpillShuffleMapOutputWriter.scala:24-64
 *   reduce side  S3ShuffleReader.read (validation + wrapStream)    storage/S3ShuffleReader.scala:98-110
 *
 * Build (with a JDK):  cc -O2 -fPIC -shared -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -Iinclude \
 *                         jni/s3s_jni.c -Lspark-s3-shuffle_amd/lib -ls3shuffle_codec -Wl,-rpath,'$ORIGIN' -o libs3shuffle_jni.so
 *                      (the name spark.shuffle.s3.gpu.library defaults to; libs3shuffle_codec.so next to it)
 * This image has no JDK: tests/test_jni_shim.py compiles the file against tests/mock_jni/jni.h instead, so the
 * signatures stay in step with the header.
 *
 * Buffers: `src` / `dst` / `comp` are DIRECT ByteBuffers — page-locked ones from hostAlloc() (below) — so there is
 * no GetPrimitiveArrayCritical section around a GPU call.  long[] / int[] arguments are small (N + 1 entries). */
#include <jni.h>
#include <stddef.h>
#include <stdint.h>

#include "s3shuffle_codec.h"

#define CTX(h) ((s3s_ctx*)(intptr_t)(h))
/* S3SCodec is a Scala `object`: scalac puts its @native methods on the module class S3SCodec$ as INSTANCE methods (the static
 * forwarders in class S3SCodec are ordinary bytecode), so the JVM looks the natives up under the mangled name of S3SCodec$
 * ('$' is _00024) and passes the module instance where a static native would get the class. */
#define FN(name) Java_org_apache_spark_shuffle_gpu_S3SCodec_00024_##name

static jlong* pin(JNIEnv* e, jlongArray a) { return a ? (*e)->GetLongArrayElements(e, a, NULL) : NULL; }
static void unpin(JNIEnv* e, jlongArray a, jlong* p, jint mode) {
  if (a && p) (*e)->ReleaseLongArrayElements(e, a, p, mode);
}
static uint8_t* addr(JNIEnv* e, jobject buf) { return buf ? (uint8_t*)(*e)->GetDirectBufferAddress(e, buf) : NULL; }

/* ---- lifecycle, options, errors ---------------------------------------------------------------------------- */
JNIEXPORT jint JNICALL FN(abiVersion)(JNIEnv* e, jclass c) { (void)e; (void)c; return s3s_abi_version(); }
JNIEXPORT jint JNICALL FN(deviceCount)(JNIEnv* e, jclass c) { (void)e; (void)c; return s3s_device_count(); }
JNIEXPORT jlong JNICALL FN(create)(JNIEnv* e, jclass c, jint device, jlong scratch) {
  (void)e; (void)c;
  return (jlong)(intptr_t)s3s_create(device, scratch);
}
JNIEXPORT void JNICALL FN(destroy)(JNIEnv* e, jclass c, jlong h) { (void)e; (void)c; s3s_destroy(CTX(h)); }
JNIEXPORT jint JNICALL FN(setOption)(JNIEnv* e, jclass c, jlong h, jint key, jlong v) {
  (void)e; (void)c;
  return s3s_set_option(CTX(h), key, v);
}
JNIEXPORT jlong JNICALL FN(getOption)(JNIEnv* e, jclass c, jlong h, jint key) {
  (void)e; (void)c;
  return s3s_get_option(CTX(h), key);
}
JNIEXPORT jstring JNICALL FN(lastError)(JNIEnv* e, jclass c, jlong h) {
  (void)c;
  return (*e)->NewStringUTF(e, s3s_last_error(CTX(h)));
}

/* ---- Spark IO encryption: key and per-partition IVs (direct ByteBuffers: keyBytes / 16 * nIvs bytes are read) -------
 * The two library symbols are WEAK here: a libs3shuffle_codec.so from before the layer still loads, and the natives then
 * answer S3S_E_UNSUPPORTED - the answer S3SCodec uses to keep the JVM path under spark.io.encryption.enabled. */
extern int s3s_set_io_encryption(s3s_ctx* ctx, const uint8_t* key, int32_t key_bytes) __attribute__((weak));
extern int s3s_set_stream_ivs(s3s_ctx* ctx, const uint8_t* ivs, int64_t n_ivs) __attribute__((weak));
JNIEXPORT jint JNICALL FN(setIoEncryption)(JNIEnv* e, jclass c, jlong h, jobject key, jint keyBytes) {
  (void)c;
  if (!s3s_set_io_encryption) return S3S_E_UNSUPPORTED;
  return s3s_set_io_encryption(CTX(h), addr(e, key), keyBytes);
}
JNIEXPORT jint JNICALL FN(setStreamIvs)(JNIEnv* e, jclass c, jlong h, jobject ivs, jlong nIvs) {
  (void)c;
  if (!s3s_set_stream_ivs) return S3S_E_UNSUPPORTED;
  return s3s_set_stream_ivs(CTX(h), addr(e, ivs), nIvs);
}

/* ---- page-locked staging: the shim's direct ByteBuffers come from here, never from allocateDirect ------------ */
JNIEXPORT jobject JNICALL FN(hostAlloc)(JNIEnv* e, jclass c, jlong bytes) {
  (void)c;
  void* p = s3s_host_alloc(bytes);
  return p ? (*e)->NewDirectByteBuffer(e, p, bytes) : NULL;
}
JNIEXPORT void JNICALL FN(hostFree)(JNIEnv* e, jclass c, jobject buf) {
  (void)c;
  s3s_host_free(addr(e, buf));
}

/* ---- sizing -------------------------------------------------------------------------------------------------- */
JNIEXPORT jlong JNICALL FN(maxCompressedSize)(JNIEnv* e, jclass c, jlong h, jint codec, jlongArray srcOffsets, jint n) {
  (void)c;
  jlong* o = pin(e, srcOffsets);
  const jlong r = s3s_max_compressed_size(CTX(h), codec, (const int64_t*)o, n);
  unpin(e, srcOffsets, o, JNI_ABORT);
  return r;
}
JNIEXPORT jint JNICALL FN(decompressedSize)(JNIEnv* e, jclass c, jlong h, jint codec, jobject comp, jlong compLen,
                                            jlongArray outLen) {
  (void)c;
  jlong* ol = pin(e, outLen);
  const int rc = s3s_decompressed_size(CTX(h), codec, addr(e, comp), compLen, (int64_t*)ol);
  unpin(e, outLen, ol, 0);
  return rc;
}

/* ---- map side: compress + checksum of one map task (commitAllPartitions / transferMapSpillFile) ---------------- */
JNIEXPORT jint JNICALL FN(compressMapOutput)(JNIEnv* e, jclass c, jlong h, jint codec, jint algo, jobject src,
                                             jlongArray srcOffsets, jint n, jobject dst, jlong dstCap,
                                             jlongArray outIndex, jlongArray outChecksums, jlongArray outTotal) {
  (void)c;
  jlong *so = pin(e, srcOffsets), *oi = pin(e, outIndex), *oc = pin(e, outChecksums), *ot = pin(e, outTotal);
  const int rc = s3s_compress_map_output(CTX(h), codec, algo, addr(e, src), (const int64_t*)so, n, addr(e, dst), dstCap,
                                         (int64_t*)oi, (int64_t*)oc, (int64_t*)ot);
  unpin(e, srcOffsets, so, JNI_ABORT);
  unpin(e, outIndex, oi, 0);
  unpin(e, outChecksums, oc, 0);
  unpin(e, outTotal, ot, 0);
  return rc;
}

/* multi-spill map tasks: one codec stream per spill piece (UnsafeShuffleWriter / SortShuffleWriter merges) */
JNIEXPORT jint JNICALL FN(compressMapOutputSegments)(JNIEnv* e, jclass c, jlong h, jint codec, jint algo, jobject src,
                                                     jlongArray segOffsets, jint nSegs, jintArray partFirstSeg, jint n,
                                                     jobject dst, jlong dstCap, jlongArray outIndex,
                                                     jlongArray outChecksums, jlongArray outTotal) {
  (void)c;
  jlong *so = pin(e, segOffsets), *oi = pin(e, outIndex), *oc = pin(e, outChecksums), *ot = pin(e, outTotal);
  jint* pf = (*e)->GetIntArrayElements(e, partFirstSeg, NULL);
  const int rc = s3s_compress_map_output_segments(CTX(h), codec, algo, addr(e, src), (const int64_t*)so, nSegs,
                                                  (const int32_t*)pf, n, addr(e, dst), dstCap, (int64_t*)oi,
                                                  (int64_t*)oc, (int64_t*)ot);
  (*e)->ReleaseIntArrayElements(e, partFirstSeg, pf, JNI_ABORT);
  unpin(e, segOffsets, so, JNI_ABORT);
  unpin(e, outIndex, oi, 0);
  unpin(e, outChecksums, oc, 0);
  unpin(e, outTotal, ot, 0);
  return rc;
}

/* ---- checksum only (S3ShuffleHelper.createChecksumAlgorithm users) ------------------------------------------------ */
JNIEXPORT jint JNICALL FN(checksumRanges)(JNIEnv* e, jclass c, jlong h, jint algo, jobject data, jlongArray offsets,
                                          jint n, jlongArray out) {
  (void)c;
  jlong *of = pin(e, offsets), *o = pin(e, out);
  const int rc = s3s_checksum_ranges(CTX(h), algo, addr(e, data), (const int64_t*)of, n, (int64_t*)o);
  unpin(e, offsets, of, JNI_ABORT);
  unpin(e, out, o, 0);
  return rc;
}

/* ---- reduce side: verify + decompress one fetched block range (S3ShuffleReader.read) ------------------------------- */
JNIEXPORT jint JNICALL FN(decompressRange)(JNIEnv* e, jclass c, jlong h, jint codec, jint algo, jobject comp,
                                           jlong compLen, jlongArray partOffsets, jlongArray refChecksums, jint nparts,
                                           jobject dst, jlong dstCap, jlongArray outLen, jintArray outBadPartition) {
  (void)c;
  jlong *po = pin(e, partOffsets), *rs = pin(e, refChecksums), *ol = pin(e, outLen);
  jint* ob = (*e)->GetIntArrayElements(e, outBadPartition, NULL);
  const int rc = s3s_decompress_range(CTX(h), codec, algo, addr(e, comp), compLen, (const int64_t*)po,
                                      (const int64_t*)rs, nparts, addr(e, dst), dstCap, (int64_t*)ol, (int32_t*)ob);
  unpin(e, partOffsets, po, JNI_ABORT);
  unpin(e, refChecksums, rs, JNI_ABORT);
  unpin(e, outLen, ol, 0);
  (*e)->ReleaseIntArrayElements(e, outBadPartition, ob, 0);
  return rc;
}

/* ---- batched forms over host buffers: what S3GpuCommitQueue / the prefetcher hand over in ONE call ------------------
 * (s3s_compress_map_outputs_batch / s3s_decompress_ranges_batch pipeline upload, codec and download over the tasks).
 * Object arrays carry one entry per task: direct ByteBuffers and long[] of the same shapes as in the single-task calls. */
#include <stdarg.h>
#include <stdlib.h>

/* every per-task array of a batched call has one entry per task (NULL-terminated list; the one optional array of a
 * call is passed last, so a NULL there just ends the list) */
static int same_length(JNIEnv* e, jsize n, ...) {
  va_list ap;
  va_start(ap, n);
  int bad = 0;
  for (jarray a; (a = va_arg(ap, jarray)) != NULL;) bad |= (*e)->GetArrayLength(e, a) != n;
  va_end(ap);
  return bad;
}

/* stamp a status array with S3S_STATUS_NOT_RUN (the library does the same on entry; this covers the returns in front of it) */
static void not_run(JNIEnv* e, jintArray status) {
  const jsize m = (*e)->GetArrayLength(e, status);
  jint* st = (*e)->GetIntArrayElements(e, status, NULL);
  if (!st) return;
  for (jsize i = 0; i < m; i++) st[i] = S3S_STATUS_NOT_RUN;
  (*e)->ReleaseIntArrayElements(e, status, st, 0);
}

JNIEXPORT jint JNICALL FN(compressMapOutputsBatch)(JNIEnv* e, jclass c, jlong h, jint codec, jint algo, jobjectArray src,
                                                   jobjectArray srcOffsets, jobjectArray dst, jlongArray dstCap,
                                                   jobjectArray outIndex, jobjectArray outChecksums, jlongArray outTotal,
                                                   jintArray outStatus) {
  (void)c;
  if (!src || !srcOffsets || !dst || !dstCap || !outIndex || !outTotal || !outStatus) return S3S_E_INVALID;
  const jsize n = (*e)->GetArrayLength(e, src);
  not_run(e, outStatus); /* every early return below leaves "not run", never a zero that reads as OK (advisor r4) */
  if (same_length(e, n, srcOffsets, dst, dstCap, outIndex, outTotal, outStatus, outChecksums, NULL) != 0) return S3S_E_INVALID;
  if ((*e)->EnsureLocalCapacity(e, 3 * n + 8) != 0) return S3S_E_NOMEM; /* three array references per task stay live over the call */
  /* the inner arrays against the partition count srcOffsets[i] implies (advisor r3: a short outIndex[i] / outChecksums[i]
   * would let the library write past a pinned JVM array) - checked before anything is pinned */
  for (jsize i = 0; i < n; i++) {
    jlongArray so = (jlongArray)(*e)->GetObjectArrayElement(e, srcOffsets, i);
    jlongArray oi = (jlongArray)(*e)->GetObjectArrayElement(e, outIndex, i);
    jlongArray oc = outChecksums ? (jlongArray)(*e)->GetObjectArrayElement(e, outChecksums, i) : NULL;
    const jsize np1 = so ? (*e)->GetArrayLength(e, so) : 0;
    const int bad = so && (np1 < 1 || !oi || (*e)->GetArrayLength(e, oi) < np1 ||
                           (outChecksums && algo != S3S_CHECKSUM_NONE && np1 > 1 && (!oc || (*e)->GetArrayLength(e, oc) < np1 - 1)));
    if (so) (*e)->DeleteLocalRef(e, so);
    if (oi) (*e)->DeleteLocalRef(e, oi);
    if (oc) (*e)->DeleteLocalRef(e, oc);
    if (bad) return S3S_E_INVALID;
  }
  s3s_map_task* t = (s3s_map_task*)calloc((size_t)(n > 0 ? n : 1), sizeof *t);
  jlongArray* arrs = (jlongArray*)calloc((size_t)(n > 0 ? n : 1) * 3, sizeof *arrs);
  if (!t || !arrs) {
    free(t);
    free(arrs);
    return S3S_E_NOMEM;
  }
  jlong *cap = pin(e, dstCap), *tot = pin(e, outTotal);
  jint* st = (*e)->GetIntArrayElements(e, outStatus, NULL);
  for (jsize i = 0; i < n; i++) {
    jlongArray so = (jlongArray)(*e)->GetObjectArrayElement(e, srcOffsets, i);
    jlongArray oi = (jlongArray)(*e)->GetObjectArrayElement(e, outIndex, i);
    jlongArray oc = outChecksums ? (jlongArray)(*e)->GetObjectArrayElement(e, outChecksums, i) : NULL;
    arrs[3 * i] = so;
    arrs[3 * i + 1] = oi;
    arrs[3 * i + 2] = oc;
    jobject sb = (*e)->GetObjectArrayElement(e, src, i), db = (*e)->GetObjectArrayElement(e, dst, i);
    t[i].d_src = addr(e, sb); /* host addresses in the host-buffer batch */
    t[i].d_dst = addr(e, db);
    (*e)->DeleteLocalRef(e, sb);
    (*e)->DeleteLocalRef(e, db);
    t[i].src_offsets = (const int64_t*)pin(e, so);
    t[i].num_partitions = so ? (int32_t)((*e)->GetArrayLength(e, so) - 1) : -1; /* (a null entry: the library answers S3S_E_INVALID) */
    t[i].dst_capacity = cap[i];
    t[i].out_index = (int64_t*)pin(e, oi);
    t[i].out_checksums = (int64_t*)pin(e, oc);
  }
  for (jsize i = 0; i < n; i++) t[i].status = S3S_STATUS_NOT_RUN; /* (a return before the library's own stamp must not read as S3S_OK) */
  const int rc = s3s_compress_map_outputs_batch(CTX(h), codec, algo, t, (int32_t)n);
  for (jsize i = 0; i < n; i++) {
    tot[i] = t[i].out_total;
    st[i] = t[i].status;
    unpin(e, arrs[3 * i], (jlong*)t[i].src_offsets, JNI_ABORT);
    unpin(e, arrs[3 * i + 1], (jlong*)t[i].out_index, 0);
    unpin(e, arrs[3 * i + 2], (jlong*)t[i].out_checksums, 0);
    (*e)->DeleteLocalRef(e, arrs[3 * i]);
    (*e)->DeleteLocalRef(e, arrs[3 * i + 1]);
    if (arrs[3 * i + 2]) (*e)->DeleteLocalRef(e, arrs[3 * i + 2]);
  }
  unpin(e, dstCap, cap, JNI_ABORT);
  unpin(e, outTotal, tot, 0);
  (*e)->ReleaseIntArrayElements(e, outStatus, st, 0);
  free(arrs);
  free(t);
  return rc;
}

JNIEXPORT jint JNICALL FN(decompressRangesBatch)(JNIEnv* e, jclass c, jlong h, jint codec, jint algo, jobjectArray comp,
                                                 jlongArray compLen, jobjectArray partOffsets, jobjectArray refChecksums,
                                                 jobjectArray dst, jlongArray dstCap, jlongArray outLen,
                                                 jintArray outBadPartition, jintArray outStatus) {
  (void)c;
  if (!comp || !compLen || !partOffsets || !dst || !dstCap || !outLen || !outBadPartition || !outStatus) return S3S_E_INVALID;
  const jsize n = (*e)->GetArrayLength(e, comp);
  not_run(e, outStatus);
  if (same_length(e, n, compLen, partOffsets, dst, dstCap, outLen, outBadPartition, outStatus, refChecksums, NULL) != 0)
    return S3S_E_INVALID;
  if ((*e)->EnsureLocalCapacity(e, 2 * n + 8) != 0) return S3S_E_NOMEM;
  for (jsize i = 0; i < n; i++) { /* refChecksums[i] must cover the partitions partOffsets[i] names */
    jlongArray po = (jlongArray)(*e)->GetObjectArrayElement(e, partOffsets, i);
    jlongArray rs = refChecksums ? (jlongArray)(*e)->GetObjectArrayElement(e, refChecksums, i) : NULL;
    const jsize np1 = po ? (*e)->GetArrayLength(e, po) : 0;
    const int bad = po && (np1 < 1 || (refChecksums && algo != S3S_CHECKSUM_NONE && np1 > 1 && (!rs || (*e)->GetArrayLength(e, rs) < np1 - 1)));
    if (po) (*e)->DeleteLocalRef(e, po);
    if (rs) (*e)->DeleteLocalRef(e, rs);
    if (bad) return S3S_E_INVALID;
  }
  s3s_fetch_range* r = (s3s_fetch_range*)calloc((size_t)(n > 0 ? n : 1), sizeof *r);
  jlongArray* arrs = (jlongArray*)calloc((size_t)(n > 0 ? n : 1) * 2, sizeof *arrs);
  if (!r || !arrs) {
    free(r);
    free(arrs);
    return S3S_E_NOMEM;
  }
  jlong *cl = pin(e, compLen), *cap = pin(e, dstCap), *ol = pin(e, outLen);
  jint *bad = (*e)->GetIntArrayElements(e, outBadPartition, NULL), *st = (*e)->GetIntArrayElements(e, outStatus, NULL);
  for (jsize i = 0; i < n; i++) {
    jlongArray po = (jlongArray)(*e)->GetObjectArrayElement(e, partOffsets, i);
    jlongArray rs = refChecksums ? (jlongArray)(*e)->GetObjectArrayElement(e, refChecksums, i) : NULL;
    arrs[2 * i] = po;
    arrs[2 * i + 1] = rs;
    jobject cb = (*e)->GetObjectArrayElement(e, comp, i), db = (*e)->GetObjectArrayElement(e, dst, i);
    r[i].d_comp = addr(e, cb);
    r[i].d_dst = addr(e, db);
    (*e)->DeleteLocalRef(e, cb);
    (*e)->DeleteLocalRef(e, db);
    r[i].comp_len = cl[i];
    r[i].part_offsets = (const int64_t*)pin(e, po);
    r[i].ref_checksums = (const int64_t*)pin(e, rs);
    r[i].num_partitions = po ? (int32_t)((*e)->GetArrayLength(e, po) - 1) : -1;
    r[i].dst_capacity = cap[i];
  }
  for (jsize i = 0; i < n; i++) r[i].status = S3S_STATUS_NOT_RUN;
  const int rc = s3s_decompress_ranges_batch(CTX(h), codec, algo, r, (int32_t)n);
  for (jsize i = 0; i < n; i++) {
    ol[i] = r[i].out_len;
    bad[i] = r[i].bad_partition;
    st[i] = r[i].status;
    unpin(e, arrs[2 * i], (jlong*)r[i].part_offsets, JNI_ABORT);
    unpin(e, arrs[2 * i + 1], (jlong*)r[i].ref_checksums, JNI_ABORT);
    (*e)->DeleteLocalRef(e, arrs[2 * i]);
    if (arrs[2 * i + 1]) (*e)->DeleteLocalRef(e, arrs[2 * i + 1]);
  }
  unpin(e, compLen, cl, JNI_ABORT);
  unpin(e, dstCap, cap, JNI_ABORT);
  unpin(e, outLen, ol, 0);
  (*e)->ReleaseIntArrayElements(e, outBadPartition, bad, 0);
  (*e)->ReleaseIntArrayElements(e, outStatus, st, 0);
  free(arrs);
  free(r);
  return rc;
}

/* ---- streaming reduce side: a fetched range decoded window by window (s3s_dstream_*; S3GpuStreamingInputStream) -------
 * and the seeded checksums under it.  WEAK like the IO encryption symbols: against a libs3shuffle_codec.so from before the
 * streams the natives answer S3S_E_UNSUPPORTED, the answer S3GpuBlockDecoder uses to keep the JVM path for large ranges.
 * A stream travels as a jlong; the window is comp[compOff, compOff + compLen) of a direct buffer, so the caller presents
 * what a feed did not consume without moving it.  out = { consumed, out_len, need_comp, need_dst, bad_partition, at_end }. */
extern int s3s_dstream_open(s3s_ctx* ctx, int codec, int checksum_algo, const int64_t* part_offsets, const int64_t* ref_checksums,
                            int32_t nparts, s3s_dstream** out) __attribute__((weak));
extern int s3s_dstream_feed(s3s_dstream* s, const uint8_t* comp, int64_t comp_len, uint8_t* dst, int64_t dst_capacity,
                            s3s_dstream_result* r) __attribute__((weak));
extern int64_t s3s_dstream_position(const s3s_dstream* s) __attribute__((weak));
extern int s3s_dstream_close(s3s_dstream* s) __attribute__((weak));
extern int s3s_checksum_ranges_seeded(s3s_ctx* ctx, int checksum_algo, const uint8_t* data, const int64_t* offsets, int32_t n,
                                      const int64_t* seeds, int64_t* out) __attribute__((weak));
/* a range stored under IO encryption (offsets, windows and positions count the stored bytes, IVs included).  WEAK on its own:
 * a library that has the streams but not this entry point answers S3S_E_UNSUPPORTED, and the caller keeps the JVM stack. */
extern int s3s_dstream_open_encrypted(s3s_ctx* ctx, int codec, int checksum_algo, const int64_t* part_offsets, const int64_t* ref_checksums,
                                      int32_t nparts, s3s_dstream** out) __attribute__((weak));
#define STREAM(s) ((s3s_dstream*)(intptr_t)(s))

typedef int (*dstream_open_fn)(s3s_ctx*, int, int, const int64_t*, const int64_t*, int32_t, s3s_dstream**);

/* dstreamOpen and dstreamOpenEncrypted: the same arguments, the same checks */
static jint dstream_open(JNIEnv* e, dstream_open_fn open, jlong h, jint codec, jint algo, jlongArray partOffsets, jlongArray refChecksums,
                         jint nparts, jlongArray outStream) {
  if (!open) return S3S_E_UNSUPPORTED;
  if (!outStream || (*e)->GetArrayLength(e, outStream) < 1) return S3S_E_INVALID;
  if (partOffsets && (*e)->GetArrayLength(e, partOffsets) < nparts + 1) return S3S_E_INVALID; /* (the library reads nparts + 1 / nparts entries) */
  if (refChecksums && (*e)->GetArrayLength(e, refChecksums) < nparts) return S3S_E_INVALID;
  jlong *po = pin(e, partOffsets), *rs = pin(e, refChecksums), *os = pin(e, outStream);
  s3s_dstream* s = NULL;
  const int rc = open(CTX(h), codec, algo, (const int64_t*)po, (const int64_t*)rs, nparts, &s);
  os[0] = (jlong)(intptr_t)s;
  unpin(e, partOffsets, po, JNI_ABORT);
  unpin(e, refChecksums, rs, JNI_ABORT);
  unpin(e, outStream, os, 0);
  return rc;
}
JNIEXPORT jint JNICALL FN(dstreamOpen)(JNIEnv* e, jclass c, jlong h, jint codec, jint algo, jlongArray partOffsets,
                                       jlongArray refChecksums, jint nparts, jlongArray outStream) {
  (void)c;
  return dstream_open(e, s3s_dstream_open, h, codec, algo, partOffsets, refChecksums, nparts, outStream);
}
JNIEXPORT jint JNICALL FN(dstreamOpenEncrypted)(JNIEnv* e, jclass c, jlong h, jint codec, jint algo, jlongArray partOffsets,
                                                jlongArray refChecksums, jint nparts, jlongArray outStream) {
  (void)c;
  return dstream_open(e, s3s_dstream_open_encrypted, h, codec, algo, partOffsets, refChecksums, nparts, outStream);
}
JNIEXPORT jint JNICALL FN(dstreamFeed)(JNIEnv* e, jclass c, jlong stream, jobject comp, jlong compOff, jlong compLen,
                                       jobject dst, jlong dstCap, jlongArray out) {
  (void)c;
  if (!s3s_dstream_feed) return S3S_E_UNSUPPORTED;
  if (!out || (*e)->GetArrayLength(e, out) < 6 || compOff < 0 || compLen < 0 || dstCap < 0) return S3S_E_INVALID;
  /* the library copies compLen bytes in and up to dstCap bytes out: both must lie inside the buffers they name */
  if ((compLen > 0 || compOff > 0) && (!comp || compOff > (*e)->GetDirectBufferCapacity(e, comp) - compLen)) return S3S_E_INVALID;
  if (dstCap > 0 && (!dst || dstCap > (*e)->GetDirectBufferCapacity(e, dst))) return S3S_E_INVALID;
  uint8_t* cp = addr(e, comp);
  s3s_dstream_result r = {0, 0, 0, 0, -1, 0};
  const int rc = s3s_dstream_feed(STREAM(stream), cp ? cp + compOff : NULL, compLen, addr(e, dst), dstCap, &r);
  jlong* o = pin(e, out);
  o[0] = r.consumed;
  o[1] = r.out_len;
  o[2] = r.need_comp;
  o[3] = r.need_dst;
  o[4] = r.bad_partition;
  o[5] = r.at_end;
  unpin(e, out, o, 0);
  return rc;
}
JNIEXPORT jlong JNICALL FN(dstreamPosition)(JNIEnv* e, jclass c, jlong stream) {
  (void)e; (void)c;
  return s3s_dstream_position ? s3s_dstream_position(STREAM(stream)) : (jlong)S3S_E_UNSUPPORTED;
}
JNIEXPORT jint JNICALL FN(dstreamClose)(JNIEnv* e, jclass c, jlong stream) {
  (void)e; (void)c;
  return s3s_dstream_close ? s3s_dstream_close(STREAM(stream)) : S3S_E_UNSUPPORTED;
}
JNIEXPORT jint JNICALL FN(checksumRangesSeeded)(JNIEnv* e, jclass c, jlong h, jint algo, jobject data, jlongArray offsets,
                                                jint n, jlongArray seeds, jlongArray out) {
  (void)c;
  if (!s3s_checksum_ranges_seeded) return S3S_E_UNSUPPORTED;
  if (n < 0 || !offsets || (*e)->GetArrayLength(e, offsets) < n + 1 || !out || (*e)->GetArrayLength(e, out) < n) return S3S_E_INVALID;
  if (seeds && (*e)->GetArrayLength(e, seeds) < n) return S3S_E_INVALID;
  jlong *of = pin(e, offsets), *sd = pin(e, seeds), *o = pin(e, out);
  if (n > 0 && (of[n] < 0 || !data || of[n] > (*e)->GetDirectBufferCapacity(e, data))) { /* (the library checks the order) */
    unpin(e, offsets, of, JNI_ABORT);
    unpin(e, seeds, sd, JNI_ABORT);
    unpin(e, out, o, JNI_ABORT);
    return S3S_E_INVALID;
  }
  const int rc = s3s_checksum_ranges_seeded(CTX(h), algo, addr(e, data), (const int64_t*)of, n, (const int64_t*)sd, (int64_t*)o);
  unpin(e, offsets, of, JNI_ABORT);
  unpin(e, seeds, sd, JNI_ABORT);
  unpin(e, out, o, 0);
  return rc;
}
