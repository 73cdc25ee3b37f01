// lzf_compress.hip — map side of S3S_CODEC_LZF (S3S_OPT_LZF_COMPRESS = 1): LZFOutputStream-shaped streams any LZF decoder reads.
//
// No reference counterpart as an implementation: on the JVM the partition bytes go through compress-lzf's LZFOutputStream
// (LZFCompressionCodec), whose bytes depend on a hash table carried from chunk to chunk.  A decode-compatible
// stream can be written block-parallel: chunks of 65 535 source bytes, each compressed with no history before
// its own first byte, so every chunk is independent work.
//
// One wavefront per chunk (one workgroup of 64 threads per plan item; 16 KiB of LDS for 8192 u16 positions: ten wavefronts
// per compute unit).  parse_wave examines 64 positions per step - the statement of the same step for one thread is
// compress_block in lzf_encode_core.h, the host model, and both give the same bytes.  Literals and references are written
// one lane each at closed-form places (lit_cost / match_cost); there is no serial byte loop.  The block goes to the chunk's
// slot, the 5- or 7-byte chunk header right-aligned in front of it; a chunk whose block is not two bytes shorter is marked
// stored (kRawFlag) and the gather copies its bytes from the source.  The item / slot / scan / gather / checksum pipeline
// around this kernel is the one LZ4, Snappy and Zstandard use.
#define S3S_LZF_DEVICE 1
#include "s3s_internal.h"
#include "lzf_encode_core.h"

namespace s3s {
namespace {

using namespace s3s_lzf_enc;

static_assert(kLzfChunk == kChunk, "one chunk size, stated twice");
static_assert(kLzfSlotPayload >= kChunk + kChunk / kMaxLit + 4, "a slot holds the largest block the parse can write");

// the position table: volatile, because table_insert reads back what the wavefront's other lanes may have overwritten, and
// in the LDS address space by type, so that the volatile accesses stay ds_ instructions
typedef __attribute__((address_space(3))) volatile uint16_t LdsU16;

// tab[h] = p for the lanes with ins set; where several lanes of the step share a slot the LATEST position has to win whatever
// order the hardware takes the lanes in: write, read back, and write again while an earlier position is what stayed.
__device__ __forceinline__ void table_insert(LdsU16* tab, uint32_t h, uint32_t p, bool ins) {
  bool pend = ins;
  while (__ballot(pend)) {
    if (pend) {
      tab[h] = (uint16_t)p;
      pend = tab[h] < (uint16_t)p;  // (entries of earlier steps are below every position of this one)
    }
  }
}

__device__ __forceinline__ uint32_t parse_wave(const uint8_t* __restrict__ s, uint32_t n, LdsU16* tab, uint8_t* __restrict__ out) {
  const uint32_t lane = threadIdx.x;
  uint32_t ip = 0, anchor = 0, op = 0;
  while (ip + 3 <= n) {
    const uint32_t p = ip + lane;
    const bool active = p + 3 <= n;
    uint32_t h = 0, c = 0;
    int len = 0;
    if (active) {
      h = hash3(s + p);
      c = tab[h];
      len = probe(s, n, p, c);
    }
    const uint64_t hits = __ballot(len > 0);
    int k = -1;
    if (hits) {
      int key = gain_key(len, (int)lane, __builtin_ctzll(hits));
#pragma unroll
      for (int d = 1; d < kStep; d <<= 1) {
        const int o = __shfl_xor(key, d);
        key = o > key ? o : key;
      }
      k = kStep - 1 - (key & (kStep - 1));
    }
    table_insert(tab, h, p, active && (k < 0 || (int)lane <= k));
    if (k < 0) {
      ip += kStep;
      continue;
    }
    uint32_t m = ip + (uint32_t)k, cc = (uint32_t)__shfl((int)c, k), ml = 3;
    for (;;) {
      const uint32_t j = ml + lane;
      const bool ok = m + j < n && s[m + j] == s[cc + j];
      const uint64_t bad = __ballot(!ok);
      if (bad) {
        ml += (uint32_t)__builtin_ctzll(bad);
        break;
      }
      ml += kStep;
    }
    const uint32_t end = m + ml;
    const bool okb = m > anchor + lane && cc > lane && s[m - lane - 1] == s[cc - lane - 1];
    const uint64_t badb = __ballot(!okb);
    const uint32_t back = badb ? (uint32_t)__builtin_ctzll(badb) : (uint32_t)kStep;
    m -= back;
    cc -= back;
    ml += back;
    const uint32_t ll = m - anchor;
    for (uint32_t i = lane; i < ll; i += kStep) put_literal(out + op, s + anchor, ll, i);
    op += lit_cost(ll);
    const uint32_t np = match_pieces(ml);
    for (uint32_t j = lane; j < np; j += kStep) put_piece(out + op, ml, m - cc, j);
    op += match_cost(ml);
    anchor = ip = end;
  }
  const uint32_t ll = n - anchor;
  for (uint32_t i = lane; i < ll; i += kStep) put_literal(out + op, s + anchor, ll, i);
  return op + lit_cost(ll);
}

__global__ __launch_bounds__(kStep) void lzf_compress_kernel(const uint8_t* __restrict__ src, const Item* __restrict__ items,
                                                             int32_t n_items, uint8_t* __restrict__ slots, int64_t slot_stride,
                                                             uint32_t* __restrict__ item_size) {
  __shared__ uint16_t tab[1 << kHashLog];
  const int32_t it = blockIdx.x;
  if (it >= n_items) return;
  const Item item = items[it];
  if ((item.kind & 0xff) != kItemLzfChunk) return;
  for (int i = threadIdx.x; i < (1 << kHashLog) / 2; i += kStep) reinterpret_cast<uint32_t*>(tab)[i] = 0;
  __syncthreads();
  const uint32_t n = (uint32_t)item.len;  // 1 .. kChunk
  uint8_t* payload = slots + (size_t)item.chunk * (size_t)slot_stride + kSlotHeader;
  const uint32_t c = parse_wave(src + item.src_off, n, (LdsU16*)tab, payload);
  if (threadIdx.x == 0) item_size[it] = put_chunk_header(payload, n, c) | (chunk_stored(n, c) ? kRawFlag : 0u);
}

}  // namespace

void launch_lzf_compress(const uint8_t* d_src, const Item* d_items, int32_t n_items, uint8_t* d_slots, int64_t slot_stride,
                         uint32_t* d_item_size, hipStream_t st) {
  if (n_items <= 0) return;
  hipLaunchKernelGGL(lzf_compress_kernel, dim3((unsigned)n_items), dim3(kStep), 0, st, d_src, d_items, n_items, d_slots, slot_stride,
                     d_item_size);
}

}  // namespace s3s
