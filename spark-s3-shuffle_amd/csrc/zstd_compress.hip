// zstd_compress.hip — map side of S3S_CODEC_ZSTD (S3S_OPT_ZSTD_COMPRESS = 1, ABI 11): Zstandard frames any decoder reads.
//
// No reference counterpart as an implementation: on the JVM the partition bytes go through zstd-jni's ZstdOutputStream
// (ZStdCompressionCodec, level 1).  libzstd's bytes cannot be reproduced by a block-parallel program; a
// decode-compatible stream can be written by one: one frame per non-empty segment, blocks of 128 KiB with no
// history before their own first byte, so every block is independent work.
//
// One workgroup of 256 threads takes one block at a time (persistent grid, block b of the call goes to workgroup
// b mod grid; the bytes written do not depend on that):
//   1. parse      wavefront 0: 64 positions per step against an 8192 x u32 table in LDS, sequences and literals to the
//                 workgroup's scratch in global memory (the statement of the same parse for one thread is parse_block in
//                 zstd_encode_core.h — the host model — and both give the same sequences)
//   2. literals   histogram (LDS atomics: sums, order-free) by all threads; code construction, weight description and the
//                 section's layout by one lane; code-bit sums of the four quarters by all threads; the 1 or 4 Huffman
//                 streams by one lane each, on four different wavefronts
//   3. sequences  one lane: the FSE state chain is serial per block
// The block leaves as Raw when the compressed form is not smaller (the gather copies the source), as RLE when all its
// bytes are equal.  The item / slot / scan / gather / checksum pipeline around this kernel is the one LZ4 and Snappy use.
#define S3S_ZSTD_DEVICE 1
#include "s3s_internal.h"
#include "zstd_encode_core.h"

namespace s3s {
namespace {

using namespace s3s_zstd_enc;

constexpr int kThreads = 256;

__device__ void parse_wave(const uint8_t* __restrict__ src, uint32_t n, uint32_t* tab, uint64_t* seqs, uint8_t* lits,
                           uint32_t* nseq_out, uint32_t* nl_out) {
  const uint32_t lane = threadIdx.x;
  uint32_t ip = 0, anchor = 0, nseq = 0, nl = 0;
  while (ip + 4 <= n && nseq < (uint32_t)kMaxSeq) {
    const uint32_t p = ip + lane;
    const bool active = p + 4 <= n;
    uint32_t h = 0, c = 0;
    int len = 0;
    if (active) {
      const uint32_t v = rd32(src + p);
      h = hash4(v);
      c = tab[h];
      if (c && rd32(src + c - 1) == v) {
        len = 4;
        while (len < 4 + kProbe && p + len < n && src[p + len] == src[c - 1 + len]) len++;
      }
    }
    const uint64_t hits = __ballot(len > 0);
    int k = -1;
    uint32_t cand = 0;
    if (hits) {
      const int k0 = __builtin_ctzll(hits);
      const int gain = (len > 0 && (int)lane >= k0 && (int)lane < k0 + kLazy) ? len - ((int)lane - k0) : 0;
      int key = gain > 0 ? gain * 64 + (63 - (int)lane) : 0;  // the largest gain, the earliest position among equals
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_xor(key, d);
        key = o > key ? o : key;
      }
      k = 63 - (key & 63);
      cand = (uint32_t)__shfl((int)(c - 1), k);
    }
    if (active && (k < 0 || (int)lane <= k)) atomicMax(&tab[h], p + 1);
    if (k < 0) {
      ip += kStep;
      continue;
    }
    uint32_t m = ip + (uint32_t)k, cc = cand, ml = 4;
    for (;;) {
      const uint32_t j = ml + lane;
      const bool ok = m + j < n && src[m + j] == src[cc + j];
      const uint64_t bad = __ballot(!ok);
      if (bad) {
        ml += (uint32_t)__builtin_ctzll(bad);
        break;
      }
      ml += 64;
    }
    const uint32_t end = m + ml;
    const bool okb = m > anchor + lane && cc > lane && src[m - lane - 1] == src[cc - lane - 1];
    const uint64_t badb = __ballot(!okb);
    const uint32_t back = badb ? (uint32_t)__builtin_ctzll(badb) : 64u;
    m -= back;
    cc -= back;
    ml += back;
    const uint32_t ll = m - anchor;
    for (uint32_t i = lane; i < ll; i += 64) lits[nl + i] = src[anchor + i];
    if (lane == 0) seqs[nseq] = seq_pack(ll, ml, m - cc);
    nl += ll;
    nseq++;
    anchor = ip = end;
  }
  for (uint32_t i = lane; i < n - anchor; i += 64) lits[nl + i] = src[anchor + i];
  nl += n - anchor;
  if (lane == 0) {
    *nseq_out = nseq;
    *nl_out = nl;
  }
}

struct Shared {
  uint32_t tab[1 << kHashLog];
  Work w;
  LitPlan plan;
  uint32_t nseq, nl, plan_ok;
};

__global__ __launch_bounds__(kThreads) void zstd_compress_kernel(const uint8_t* __restrict__ src, const Item* __restrict__ items,
                                                                 int32_t n_items, uint8_t* __restrict__ slots, int64_t slot_stride,
                                                                 uint32_t* __restrict__ item_size, uint8_t* __restrict__ scratch,
                                                                 int64_t scratch_stride) {
  __shared__ Shared sh;
  const int tid = threadIdx.x;
  uint64_t* seqs = reinterpret_cast<uint64_t*>(scratch + (int64_t)blockIdx.x * scratch_stride);
  uint8_t* lits = reinterpret_cast<uint8_t*>(seqs + kMaxSeq);
  if (tid == 0) build_predefined(sh.w);
  __syncthreads();
  for (int32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    const Item item = items[it];
    const int kind = item.kind & 0xff;
    if (kind == kItemZstdHeader) {
      if (tid == 0) item_size[it] = kFrameHeader;
      continue;
    }
    if (kind != kItemZstdBlock) continue;
    const uint8_t* s = src + item.src_off;
    const uint32_t n = (uint32_t)item.len;
    const bool last = (item.kind >> 8) & 1;
    uint8_t* slot = slots + (size_t)item.chunk * (size_t)slot_stride;
    uint8_t* out = slot + kSlotHeader;  // block content; the 3-byte block header sits right in front of it
    // all bytes equal: RLE_Block
    int differs = 0;
    const uint8_t b0 = s[0];
    for (uint32_t i = tid; i < n; i += kThreads) differs |= s[i] != b0;
    for (int i = tid; i < (1 << kHashLog); i += kThreads) sh.tab[i] = 0;
    for (int i = tid; i < 256; i += kThreads) sh.w.hist[i] = 0;
    if (!__syncthreads_or(differs)) {
      if (tid == 0) {
        put_block_header(out - 3, last, kBlockRle, n);
        out[0] = b0;
        item_size[it] = 4;
      }
      continue;
    }
    if (tid < 64) parse_wave(s, n, sh.tab, seqs, lits, &sh.nseq, &sh.nl);
    __threadfence_block();
    __syncthreads();
    const uint32_t nseq = sh.nseq, nl = sh.nl;
    for (uint32_t i = tid; i < nl; i += kThreads) atomicAdd(&sh.w.hist[lits[i]], 1u);
    __syncthreads();
    if (tid == 0) {
      huf_build(sh.w);
      for (int k = 0; k < 4; k++) sh.w.sbits[k] = 0;
    }
    __syncthreads();
    if (sh.w.nsym >= 2) {
      const uint32_t q = (nl + 3) / 4;
      uint32_t mine[4] = {0, 0, 0, 0};
      for (uint32_t i = tid; i < nl; i += kThreads) {
        const uint32_t k = i / q;
        mine[k > 3 ? 3 : k] += sh.w.nbits[lits[i]];
      }
      for (int k = 0; k < 4; k++)
        if (mine[k]) atomicAdd(&sh.w.sbits[k], mine[k]);
    }
    __syncthreads();
    const uint32_t cap = n - 1;  // a Compressed_Block must be smaller than the block (equal is refused by libzstd at 128 KiB)
    if (tid == 0) sh.plan_ok = (uint32_t)lit_plan(sh.w, nl, nl ? lits[0] : 0, sh.plan, out, cap);
    __syncthreads();
    uint32_t body = 0;
    if (sh.plan_ok) {
      if (sh.plan.mode == 0) {
        for (uint32_t i = tid; i < nl; i += kThreads) out[sh.plan.data + i] = lits[i];
      } else if (sh.plan.mode == 2 && (tid & 63) == 0) {
        const int k = tid >> 6;
        if (sh.plan.single) {
          if (k == 0) huf_encode_stream(sh.w, lits, nl, out + sh.plan.soff[0], sh.plan.sbytes[0]);
        } else {
          uint32_t lo, hi;
          stream_range(nl, k, &lo, &hi);
          huf_encode_stream(sh.w, lits + lo, hi - lo, out + sh.plan.soff[k], sh.plan.sbytes[k]);
        }
      }
      if (tid == 0) {
        const uint32_t sq = seq_encode(sh.w, seqs, nseq, out + sh.plan.total, cap - sh.plan.total);
        body = sq ? sh.plan.total + sq : 0;
      }
    }
    if (tid == 0) {
      if (body) {
        put_block_header(out - 3, last, kBlockCompressed, body);
        item_size[it] = 3 + body;
      } else {
        put_block_header(out - 3, last, kBlockRaw, n);
        item_size[it] = (3 + n) | kRawFlag;
      }
    }
    __syncthreads();  // the next block reuses the table, the histogram and the scratch
  }
}

}  // namespace

int64_t zstd_compress_scratch_stride() { return (int64_t)kMaxSeq * 8 + kBlock + 256; }

void launch_zstd_compress(const uint8_t* d_src, const Item* d_items, int32_t n_items, uint8_t* d_slots, int64_t slot_stride,
                          uint32_t* d_item_size, uint8_t* d_scratch, int32_t grid, hipStream_t st) {
  if (n_items <= 0) return;
  if (grid > n_items) grid = n_items;
  hipLaunchKernelGGL(zstd_compress_kernel, dim3((unsigned)grid), dim3(kThreads), 0, st, d_src, d_items, n_items, d_slots, slot_stride,
                     d_item_size, d_scratch, zstd_compress_scratch_stride());
}

}  // namespace s3s
