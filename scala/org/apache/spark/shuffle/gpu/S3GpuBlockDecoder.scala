//
// S3GpuBlockDecoder — what S3ShuffleReader.read (storage/S3ShuffleReader.scala:98-110) calls instead of
//   new S3ChecksumValidationStream(blockId, stream, algo)  +  serializerManager.wrapStream(blockId, …)
// when the reduce side of the GPU path is on (dispatcher.gpuReadEnabled, scala/patches/0001-gpu-codec.patch: with GPU writers,
// or on its own over the objects of JVM writers - lz4 of any block size, snappy, zstd): the prefetched block range (one
// ShuffleBlockId or one ShuffleBlockBatchId = several contiguous partitions of one map output,
// S3ShuffleBlockIterator.scala:37-42) is verified per partition against the `.checksum` object and decoded in ONE
// library call; the deserializer then reads plain bytes.
//
// A range above 1 GiB compressed or decoded (one direct ByteBuffer has Int positions) does not fit that one call: it is
// decoded window by window through S3GpuStreamingInputStream (s3s_dstream_*: two page-locked buffers of
// spark.shuffle.s3.gpu.streamWindowBytes, any range size, the checksum verdict at the end of each partition) - lz4, snappy,
// lzf and uncompressed ranges; a Zstandard range of that size keeps the JVM stack.
//
// A range below spark.shuffle.s3.gpu.minBytes, or written with a codec the library does not have, takes the
// reference's JVM stack (`jvmPath`): checksum validation stream + the codec's own input stream.  The objects a GPU
// writer produced are ordinary LZ4Block / SnappyOutputStream streams, so either side may be the JVM.
//
// NOT COMPILED IN THIS IMAGE (no JDK / scalac).
//
package org.apache.spark.shuffle.gpu

import java.io.{EOFException, InputStream}
import java.nio.ByteBuffer
import java.util.concurrent.atomic.AtomicBoolean

import org.apache.spark.SparkEnv
import org.apache.spark.shuffle.helper.{S3ShuffleDispatcher, S3ShuffleHelper}
import org.apache.spark.storage.{BlockId, ShuffleBlockBatchId, ShuffleBlockId}

object S3GpuBlockDecoder {
  private def range(blockId: BlockId): (Int, Long, Int, Int) = blockId match {
    case ShuffleBlockId(s, m, r) => (s, m, r, r + 1)
    case ShuffleBlockBatchId(s, m, r0, r1) => (s, m, r0, r1)
    case other => throw new IllegalArgumentException(s"unexpected block $other")
  }

  /** Compressed length of the range from the cached `.index` (S3ShuffleHelper.scala:76-81). */
  def compressedLength(blockId: BlockId): Long = {
    val (shuffleId, mapId, r0, r1) = range(blockId)
    val lengths = S3ShuffleHelper.getPartitionLengths(shuffleId, mapId)
    lengths(r1) - lengths(r0)
  }

  /** True when `decode` should take this block (the reader keeps the JVM stack otherwise).  The codec is the one the stored
    * objects carry (dispatcher.gpuReadCodec: spark.shuffle.s3.gpu.codec for GPU writers, spark.io.compression.codec for JVM
    * writers).  Zstandard: one wavefront decodes one partition's frame at ~10 MB/s, so the library only pays when a range
    * holds MANY small frames - a batch range of at least spark.shuffle.s3.gpu.zstd.minPartitions partitions whose mean size
    * is at most spark.shuffle.s3.gpu.zstd.maxFrameBytes; everything else stays with zstd-jni on the task thread. */
  def accepts(blockId: BlockId): Boolean = {
    val d = S3ShuffleDispatcher.get
    d.gpuReadEnabled && S3SCodec.supportsDecode(d.gpuReadCodec) && {
      val n = compressedLength(blockId)
      val (_, _, r0, r1) = range(blockId)
      val zstdOk = d.gpuReadCodec != "zstd" ||
        (r1 - r0 >= d.gpuZstdMinPartitions && n / math.max(r1 - r0, 1) <= d.gpuZstdMaxFrameBytes)
      // above one buffer: streamed in bounded memory (S3GpuStreamingInputStream) - every codec but Zstandard
      n >= d.gpuMinBytes && (n <= S3GpuBuffers.MaxBuffer || d.gpuReadCodec != "zstd") && zstdOk
    }
  }

  /** `jvmPath(in)` = the reference's stream stack for the same block over `in`: used when a range above one buffer cannot
    * be streamed by the library (a library from before s3s_dstream_*, Zstandard) - over the block stream itself, or over the
    * staged bytes when only the DECODED size turned out to be above one buffer (nothing is fetched twice). */
  def decode(blockId: BlockId, stream: InputStream, jvmPath: InputStream => InputStream): InputStream = {
    val dispatcher = S3ShuffleDispatcher.get
    val (shuffleId, mapId, r0, r1) = range(blockId)
    val ctx = S3SCodec.forThread(S3SCodec.deviceFor(mapId, S3SCodec.devices()))
    val codec = S3SCodec.decodeCodecId(dispatcher.gpuReadCodec)
    val algo = S3SCodec.checksumId(dispatcher.checksumEnabled, dispatcher.checksumAlgorithm)
    // cumulative `.index` of the map output, relative to the range
    val lengths = S3ShuffleHelper.getPartitionLengths(shuffleId, mapId)
    val rel = Array.tabulate(r1 - r0 + 1)(i => lengths(r0 + i) - lengths(r0))
    val refs = if (algo == S3SCodec.CHECKSUM_NONE) null else S3ShuffleHelper.getChecksums(shuffleId, mapId).slice(r0, r1)
    val compLen = rel(r1 - r0)
    // `in` belongs to the stream that comes back; when none does, closing it gives a staged buffer back to the pool
    def streamed(in: InputStream): InputStream =
      try S3GpuStreamingInputStream.open(blockId.name, in, compLen, ctx, codec, algo, rel, refs, r0).getOrElse(jvmPath(in))
      catch { case t: Throwable => in.close(); throw t }
    if (compLen > S3GpuBuffers.MaxBuffer) return streamed(stream) // never staged whole: window by window from the block stream
    val comp = S3GpuBuffers.take(compLen)
    var compOwned = true
    try {
      S3GpuStreams.readFully(stream, comp, compLen) // the prefetcher's buffer -> page-locked staging
      val outLen = new Array[Long](1)
      S3SCodec.check(ctx, S3SCodec.decompressedSize(ctx, codec, comp, compLen, outLen), blockId.name)
      if (outLen(0) > S3GpuBuffers.MaxBuffer) { // decoded range above one buffer: streamed from the staged bytes
        compOwned = false
        return streamed(new S3GpuStreams.DirectBufferInputStream(comp, compLen))
      }
      val out = S3GpuBuffers.take(outLen(0))
      val bad = Array(-1)
      val rc =
        try S3SCodec.decompressRange(ctx, codec, algo, comp, compLen, rel, refs, r1 - r0, out, outLen(0), outLen, bad)
        catch { case t: Throwable => S3GpuBuffers.give(out); throw t }
      if (rc != S3SCodec.OK) S3GpuBuffers.give(out)
      S3SCodec.check(ctx, rc, blockId.name, if (bad(0) >= 0) r0 + bad(0) else -1)
      new S3GpuStreams.DirectBufferInputStream(out, outLen(0)) // gives `out` back to S3GpuBuffers on the first close()
    } finally {
      if (compOwned) S3GpuBuffers.give(comp)
      stream.close()
    }
  }
}

object S3GpuStreams {
  def readFully(in: InputStream, dst: ByteBuffer, n: Long): Unit = {
    val chunk = new Array[Byte](1 << 20)
    dst.clear()
    var left = n
    while (left > 0) {
      val k = in.read(chunk, 0, math.min(left, chunk.length.toLong).toInt)
      if (k < 0) throw new java.io.EOFException(s"block ended $left bytes early")
      dst.put(chunk, 0, k); left -= k
    }
  }

  /** Reads a pooled page-locked buffer; close() is idempotent (Spark closes shuffle streams more than once) and
    * returns the buffer to the pool exactly once. */
  final class DirectBufferInputStream(buf: ByteBuffer, n: Long) extends InputStream {
    require(n <= buf.capacity() && n <= Int.MaxValue)
    private val view = buf.duplicate()
    view.position(0); view.limit(n.toInt)
    private val closed = new AtomicBoolean(false)
    private def live: Boolean = !closed.get()
    override def read(): Int = if (live && view.hasRemaining) view.get() & 0xff else -1
    override def read(b: Array[Byte], off: Int, len: Int): Int =
      if (len == 0) 0
      else if (!live || !view.hasRemaining) -1
      else { val k = math.min(len, view.remaining()); view.get(b, off, k); k }
    override def available(): Int = if (live) view.remaining() else 0
    override def close(): Unit = if (closed.compareAndSet(false, true)) S3GpuBuffers.give(buf)
  }
}

// S3GpuStreamingInputStream — the reduce side of the GPU path for a block range of ANY size, in bounded memory.
//
// S3GpuBlockDecoder.decode stages the whole compressed range and the whole decoded range (one direct ByteBuffer each, at
// most S3GpuBuffers.MaxBuffer).  The reference never holds a block like that: storage/S3BufferedInputStreamAdaptor.scala:13-19
// buffers min(maxBufferSizeTask, block length), storage/S3ChecksumValidationStream.scala:54-86 validates a partition as its
// last byte streams past, and the codec input streams decode frame by frame.  This stream degrades the same way through the
// library's s3s_dstream_* entry points (include/s3shuffle_codec.h): it owns ONE compressed and ONE decoded page-locked buffer
// of spark.shuffle.s3.gpu.streamWindowBytes each, refills the compressed window from the prefetched block stream, feeds it,
// and hands out the decoded bytes of the whole units the window held; what a feed did not consume stays in the window.
//
//   need_comp  the window's first unit is longer than the window: the compressed buffer grows to need_comp (a 32 MiB LZ4
//              block needs 32 MiB + 21 bytes whatever the key says)
//   need_dst   the first unit's decoded bytes do not fit: the decoded buffer grows to need_dst
//   errors     S3SCodec.check maps them to the reference's exceptions: E_CHECKSUM -> the SparkException of
//              S3ChecksumValidationStream.scala:74-80 with the partition's number, E_BAD_FRAME -> IOException("Stream is
//              corrupted").  As in the reference, bytes of a partition that is still open have been handed to the deserializer
//              before its checksum is known: the exception comes from the read() that passes the partition's end.
//
// Threading: the library context belongs to the task thread (S3SCodec.forThread); read() runs on the thread that opened the
// stream - the task thread that iterates the block, as with the reference's streams.
// IO encryption: with a key set on the context (OPT_IO_ENCRYPTION_KEY_BITS > 0) the range is opened by dstreamOpenEncrypted:
// offsets, windows and positions count the stored bytes, a partition's 16-byte IV is a unit of its own that decodes to
// nothing, and a window that shows less than a whole IV gets need_comp = 16 - an ordinary "fetch more" to this reader.
// Out of scope here: Zstandard ranges (the open answers E_UNSUPPORTED: the caller keeps the JVM stack), a streaming map
// side, a batched feed of several streams.
object S3GpuStreamingInputStream {
  /** spark.shuffle.s3.gpu.streamWindowBytes: the size of the compressed and of the decoded buffer of one stream.  A feed costs
    * ~0.5 ms whatever it holds, so the default is the largest window measured: 64 MiB (profiles/decode_stream.md, host-64m:
    * 29 GB/s host to host on TeraSort LZ4, 16 MiB: 15; INTEGRATION.md 1d). */
  val DefaultWindowBytes: Long = 64L << 20

  def windowBytes: Long =
    math.min(math.max(SparkEnv.get.conf.getSizeAsBytes("spark.shuffle.s3.gpu.streamWindowBytes", DefaultWindowBytes), 64L << 10),
             S3GpuBuffers.MaxBuffer)

  /** None: the library cannot stream this range (E_UNSUPPORTED: no stream entry points, Zstandard, or a key on a library from
    * before dstreamOpenEncrypted) - the caller takes the JVM stack over `source`, which is untouched.  `firstPartition` is r0 of
    * the range (exception messages). */
  def open(blockName: String, source: InputStream, rangeLength: Long, ctx: Long, codec: Int, algo: Int, rel: Array[Long],
           refs: Array[Long], firstPartition: Int): Option[S3GpuStreamingInputStream] = {
    val handle = new Array[Long](1)
    val encrypted = S3SCodec.getOption(ctx, S3SCodec.OPT_IO_ENCRYPTION_KEY_BITS) > 0 // (E_INVALID, negative: a library without the layer)
    val rc =
      if (encrypted) S3SCodec.dstreamOpenEncrypted(ctx, codec, algo, rel, refs, rel.length - 1, handle)
      else S3SCodec.dstreamOpen(ctx, codec, algo, rel, refs, rel.length - 1, handle)
    if (rc == S3SCodec.E_UNSUPPORTED) None
    else {
      S3SCodec.check(ctx, rc, blockName)
      try Some(new S3GpuStreamingInputStream(blockName, source, rangeLength, ctx, handle(0), firstPartition, windowBytes))
      catch { case t: Throwable => S3SCodec.dstreamClose(handle(0)); throw t } // (no buffer for the window)
    }
  }
}

final class S3GpuStreamingInputStream private (blockName: String, source: InputStream, rangeLength: Long, ctx: Long,
                                               stream: Long, firstPartition: Int, window: Long) extends InputStream {
  // the pool hands out any buffer of AT LEAST the size asked for: the window and the capacity a feed is given are bounded by
  // the key (or by what one unit needs), never by the size of the buffer that happened to come back
  private var comp: ByteBuffer = S3GpuBuffers.take(window) // [compPos, compEnd) = the window: fetched, not yet consumed
  private var out: ByteBuffer =
    try S3GpuBuffers.take(window) catch { case t: Throwable => S3GpuBuffers.give(comp); throw t }
  private var outCap = window // dst_capacity of a feed: the key, or need_dst of a unit that decodes to more
  private var compPos = 0L
  private var compEnd = 0L
  private var fetched = 0L // bytes of the range read from `source`
  private var outPos = 0
  private var outEnd = 0
  private var atEnd = false
  private val closed = new AtomicBoolean(false)
  private val result = new Array[Long](6) // consumed, out_len, need_comp, need_dst, bad_partition, at_end
  private val chunk = new Array[Byte](1 << 20)

  /** moves the window to the front of a buffer of at least `atLeast` bytes and fills it from the source */
  private def refillWindow(atLeast: Long): Unit = {
    val have = compEnd - compPos
    if (atLeast > comp.capacity()) { // a unit longer than the window: grow (the old buffer goes back to the pool)
      val bigger = S3GpuBuffers.take(atLeast)
      val src = comp.duplicate(); src.position(compPos.toInt); src.limit(compEnd.toInt)
      bigger.clear(); bigger.put(src)
      S3GpuBuffers.give(comp); comp = bigger
    } else if (compPos > 0) {
      comp.position(compPos.toInt); comp.limit(compEnd.toInt); comp.compact()
    }
    compPos = 0; compEnd = have
    comp.clear(); comp.position(compEnd.toInt)
    val want = math.min(math.max(atLeast, window), comp.capacity().toLong)
    while (compEnd < want && fetched < rangeLength) {
      val k = source.read(chunk, 0, math.min(math.min(want - compEnd, rangeLength - fetched), chunk.length.toLong).toInt)
      if (k < 0) throw new EOFException(s"$blockName ended ${rangeLength - fetched} bytes early")
      comp.put(chunk, 0, k); compEnd += k; fetched += k
    }
  }

  /** one or more feeds until decoded bytes are there or the range has ended */
  private def refill(): Unit = {
    var need = 0L
    while (outPos == outEnd && !atEnd) {
      if (need > 0 || compEnd - compPos < window && fetched < rangeLength) refillWindow(need)
      val rc = S3SCodec.dstreamFeed(stream, comp, compPos, compEnd - compPos, out, outCap, result)
      if (rc == S3SCodec.E_CAPACITY) { // the first unit decodes to more than the capacity: need_dst from here on
        outCap = result(3)
        if (outCap > out.capacity()) { S3GpuBuffers.give(out); out = null; out = S3GpuBuffers.take(outCap) }
      } else {
        S3SCodec.check(ctx, rc, blockName, if (result(4) >= 0) firstPartition + result(4).toInt else -1)
        compPos += result(0)
        outPos = 0; outEnd = result(1).toInt
        atEnd = result(5) != 0
        need = if (result(0) == 0) result(2) else 0 // the window grows to need_comp and the feed is repeated
      }
    }
  }

  override def read(): Int = {
    if (closed.get()) return -1
    if (outPos == outEnd) refill()
    if (outPos == outEnd) -1 else { val b = out.get(outPos) & 0xff; outPos += 1; b }
  }

  override def read(b: Array[Byte], off: Int, len: Int): Int = {
    if (len == 0) return 0
    if (closed.get()) return -1
    if (outPos == outEnd) refill()
    if (outPos == outEnd) return -1
    val k = math.min(len, outEnd - outPos)
    val view = out.duplicate(); view.position(outPos); view.limit(outPos + k)
    view.get(b, off, k); outPos += k
    k
  }

  override def available(): Int = if (closed.get()) 0 else outEnd - outPos

  /** Idempotent (Spark closes shuffle streams more than once).  A stream closed before the end of its range is not an error
    * here - Spark abandons streams (limit, task kill) - so the code of dstreamClose is dropped; corruption and wrong checksums
    * have been raised by the read() that met them. */
  override def close(): Unit = if (closed.compareAndSet(false, true)) {
    try S3SCodec.dstreamClose(stream)
    finally {
      S3GpuBuffers.give(comp); if (out != null) S3GpuBuffers.give(out)
      source.close()
    }
  }
}
