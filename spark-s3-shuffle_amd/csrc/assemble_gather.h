// assemble_gather.h — the body of the gather kernels: one plan item copied to its place in the .data image.  Included INSIDE
// namespace s3s { namespace { ... } } by assemble.hip (gather_items_kernel, gather_items_batch_kernel) and by
// compress_stream_kernels.hip (gather_items_cut_kernel), so that every gather writes an item the same way.
constexpr int kGatherThreads = 256;

// n bytes global -> global; 16-byte stores on the destination's alignment.
__device__ __forceinline__ void copy_bytes(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src,
                                           int n, int tid) {
  int head = (int)((16u - (uint32_t)(uintptr_t)dst) & 15u);
  head = head < n ? head : n;
  if (tid < head) dst[tid] = src[tid];
  const int nvec = (n - head) >> 4;
  uint4* d16 = reinterpret_cast<uint4*>(dst + head);
  const uint8_t* s = src + head;
  for (int v = tid; v < nvec; v += kGatherThreads) {
    uint4 x;
    __builtin_memcpy(&x, s + 16 * v, 16);  // source alignment is arbitrary
    d16[v] = x;
  }
  const int done = head + 16 * nvec;
  if (tid < n - done) dst[done + tid] = src[done + tid];
}

__device__ __forceinline__ void gather_item_body(
    const uint8_t* __restrict__ src, const Item* __restrict__ items, int32_t n_items,
    const uint8_t* __restrict__ slots, int64_t slot_stride, const uint32_t* __restrict__ item_size,
    const int64_t* __restrict__ item_off, uint8_t* __restrict__ dst, int64_t dst_capacity,
    int32_t* __restrict__ status, int it) {
  if (it >= n_items) return;
  const Item item = items[it];
  const uint32_t sz = item_size[it];
  const int n = (int)(sz & ~kRawFlag);
  const int64_t off = item_off[it];
  const int tid = threadIdx.x;
  if (off + n > dst_capacity) {
    if (tid == 0) atomicExch(status, S3S_E_CAPACITY);
    return;
  }
  uint8_t* d = dst + off;
  const int kind = item.kind & 0xff;
  if (kind == kItemLz4End) {
    // LZ4BlockOutputStream.finish(): magic | RAW|level | 0 | 0 | 0
    if (tid < kLz4FrameHeader) {
      const uint64_t magic = 0x6b636f6c42345a4cull;
      uint32_t b = 0;
      if (tid < 8) b = (uint32_t)(magic >> (8 * tid));
      else if (tid == 8) b = 0x10u | ((uint32_t)(item.kind >> 8) & 0x0Fu);
      d[tid] = (uint8_t)b;
    }
    return;
  }
  if (kind == kItemSnappyHeader) {
    if (tid < kSnappyStreamHeader) {
      const uint64_t lo = 0x00595050414e5382ull;  // 0x82 'S' 'N' 'A' 'P' 'P' 'Y' 0x00
      uint32_t b;
      if (tid < 8) b = (uint32_t)(lo >> (8 * tid));
      else b = (tid == 11 || tid == 15) ? 1u : 0u;  // version = 1, compatible version = 1 (BE)
      d[tid] = (uint8_t)b;
    }
    return;
  }
  if (kind == kItemZstdHeader) {
    // 28 B5 2F FD | descriptor 0xC0 (8-byte Frame_Content_Size, no checksum, no dictionary) | window 2^17 | content size LE
    if (tid < kZstdFrameHeader) {
      const uint64_t lo = 0x38C0FD2FB528ull;
      d[tid] = tid < 6 ? (uint8_t)(lo >> (8 * tid)) : (uint8_t)((uint64_t)item.src_off >> (8 * (tid - 6)));
    }
    return;
  }
  if (kind == kItemSnappyChunkHead) {
    // a Snappy chunk above one fragment: i32 BE compressed length | varint32(len).  The fragments follow this item, so the
    // raw block is the preamble plus what the scan placed between the first fragment's start and the last one's end.
    if (tid < n) {
      const int nfrag = (item.len + kSnappyFragment - 1) / kSnappyFragment;
      const int vlen = n - 4;
      const uint32_t clen = (uint32_t)(item_off[it + 1 + nfrag] - item_off[it + 1]) + (uint32_t)vlen;
      uint32_t b;
      if (tid < 4) b = clen >> (8 * (3 - tid));
      else b = (((uint32_t)item.len >> (7 * (tid - 4))) & 0x7fu) | (tid - 4 + 1 < vlen ? 0x80u : 0u);
      d[tid] = (uint8_t)b;
    }
    return;
  }
  if (kind == kItemIv) return;  // 16 bytes the AES-CTR pass fills (aes_ctr.hip)
  const uint8_t* slot = slots + (size_t)item.chunk * (size_t)slot_stride;
  if (kind == kItemSnappyFrag) {  // a fragment's elements, behind the head item (and the fragments in front of it)
    copy_bytes(d, slot + kSlotHeader, n, tid);
    return;
  }
  if (kind == kItemZstdBlock) {  // 3-byte block header, then the content (a Raw_Block's content is the source)
    if (sz & kRawFlag) {
      copy_bytes(d, slot + (kSlotHeader - 3), 3, tid);
      copy_bytes(d + 3, src + item.src_off, n - 3, tid);
    } else {
      copy_bytes(d, slot + (kSlotHeader - 3), n, tid);
    }
    return;
  }
  if (kind == kItemLzfChunk) {  // 'Z' 'V' type | lengths, then the block (a stored chunk's bytes are the source)
    if (sz & kRawFlag) {
      copy_bytes(d, slot + (kSlotHeader - 5), 5, tid);
      copy_bytes(d + 5, src + item.src_off, n - 5, tid);
    } else {
      copy_bytes(d, slot + (kSlotHeader - 7), n, tid);
    }
    return;
  }
  if (kind == kItemLz4Chunk || kind == kItemLz4ChunkU32) {
    if (sz & kRawFlag) {
      copy_bytes(d, slot + (kSlotHeader - kLz4FrameHeader), kLz4FrameHeader, tid);
      copy_bytes(d + kLz4FrameHeader, src + item.src_off, n - kLz4FrameHeader, tid);
    } else {
      copy_bytes(d, slot + (kSlotHeader - kLz4FrameHeader), n, tid);
    }
  } else {  // kItemSnappyChunk: i32 BE length right-aligned in the slot header, then payload
    copy_bytes(d, slot + (kSlotHeader - 4), n, tid);
  }
}
