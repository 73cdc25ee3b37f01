// zstd_decode_blocks.h — what zstd_decompress.hip (the serial, one-frame-per-wavefront decoder and the orchestration of the
// reduce side) and zstd_decode_blocks.hip (the block-parallel path in front of it) share: the records of a
// partition, the body of the per-partition kernel, and the host interface of the block path.
#pragma once
#include "s3s_ctx.h"
#include "zstd_decode_core.h"

namespace s3s {

struct ZPart {       // one partition of one range
  const uint8_t* src;
  int64_t size;
  uint8_t* dst;      // pass 2: where its decoded bytes go
  int64_t cap;       // pass 2: bytes available there
  int64_t lit_off;   // pass 2: offset of its literals scratch: two buffers lit_stride apart (block k uses buffer k & 1)
  int64_t lit_stride;
};
struct ZRes {
  int64_t total;     // decoded bytes
  int64_t lit_need;  // scratch the partition needs in pass 2
  int32_t rc;        // ZS_OK / ZS_BAD / ZS_CAPACITY / ZS_UNSUPPORTED (= the S3S_E_* values)
  int32_t pad;
};

// ---- the block path's records (device memory, one arena per context) --------------------------------------------------------------
struct ZBlockCtrl {
  int32_t n_jobs;       // entries of the block table handed out by the scan
  int32_t blocks_done;  // blocks of the frames the per-partition kernel stepped over (S3S_OPT_ZSTD_DECODE_BLOCKS)
  int32_t pad[2];
};
struct ZScanPart {      // per partition: its slice of the frame table
  int32_t frame_base, frame_cap;
};
struct ZBlockPlan {     // one call's block path; on = false: nothing was launched, the serial kernel runs as it always did
  bool on = false;
  ZBlockCtrl* d_ctrl = nullptr;
  const ZScanPart* d_sp = nullptr;
  const int32_t* d_nframes = nullptr;
  const s3s_zstd::FrameEnt* d_frames = nullptr;
};

constexpr int kZstdThreads = 3 * kWave;

// Scan + block decode of the partitions h_parts[0, n_parts) (already uploaded to d_parts, destinations and capacities final).
// plan->on tells whether anything ran; an allocation that does not fit only switches the path off for the call.
int zstd_blocks_launch(s3s_ctx* ctx, const ZPart* h_parts, const ZPart* d_parts, int32_t n_parts, ZBlockPlan* plan);
// the per-partition kernel behind the block path: frames it completed are stepped over, every other frame is decoded as ever
void zstd_partitions_skip_launch(s3s_ctx* ctx, const ZPart* d_parts, int32_t n_parts, uint8_t* d_lit, ZRes* d_res, const ZBlockPlan& plan);

#ifdef __HIPCC__
// Three wavefronts per workgroup, two partitions (round 4).  Wavefronts 0 and 1 are the SEQUENCE sides of partitions 2b and
// 2b + 1: headers, FSE tables, the sequence loop and its copies.  Wavefront 2 is the LITERAL side of both: it walks the same
// headers and regenerates the Huffman-coded literals of a partition's NEXT block while its sequence wavefront executes this
// one (a level-1 TeraSort frame spent 8.5 of its 38 ms in Huffman streams on 4 of 64 lanes, and the rest never needed those
// lanes' results before the next block; one literal wavefront keeps up with two sequence sides).  They meet through four
// counters in LDS per partition (s3s_zstd::LitPipe) and two literal buffers per partition.  Registers: the sequence side
// needs 186 VGPRs when left alone; three wavefronts per SIMD (12 per CU = 4 workgroups = 8 partitions in flight, what the
// one-wavefront-per-partition kernel had) leave it 168.
// kSkip (zstd_partitions_skip_kernel): both sides step over the frames the block path completed.
// kStaged (zstd_decode_staged.hip, with kSkip): and over the frames the staged path completed, a second list per partition
// (sp2 / nframes2 / frames2, counted into *staged_done); the block path's list may then be absent (nframes == nullptr).
template <bool kSkip, bool kStaged = false>
__device__ __forceinline__ void zstd_partitions_body(const ZPart* __restrict__ parts, int32_t n, int execute, uint8_t* __restrict__ lit_base,
                                                     ZRes* __restrict__ res, const ZScanPart* __restrict__ sp, const int32_t* __restrict__ nframes,
                                                     const s3s_zstd::FrameEnt* __restrict__ frames, ZBlockCtrl* __restrict__ ctrl,
                                                     s3s_zstd::SkipCursor* scs, const ZScanPart* __restrict__ sp2 = nullptr,
                                                     const int32_t* __restrict__ nframes2 = nullptr,
                                                     const s3s_zstd::FrameEnt* __restrict__ frames2 = nullptr, int32_t* staged_done = nullptr,
                                                     s3s_zstd::SkipCursor* scs2 = nullptr) {
  __shared__ s3s_zstd::Work w[2];
  __shared__ s3s_zstd::LitPipe lp[2];
  __shared__ s3s_zstd::LitWalker ks[2];  // (the literal wavefront's own state: indexed by partition, so not in registers)
  const int p0 = 2 * (int)blockIdx.x;
  if (p0 >= n) return;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  s3s_zstd::Lanes L{(int)(threadIdx.x & (kWave - 1)), kWave};
  if (threadIdx.x < 2) lp[threadIdx.x].ready = lp[threadIdx.x].consumed = lp[threadIdx.x].err = lp[threadIdx.x].quit = 0;
  __syncthreads();
  if (wave == 2) {
    if (execute == 0) return;
    const int np = n - p0 < 2 ? n - p0 : 2;
    for (int t = 0; t < np; t++) {
      const ZPart zp = parts[p0 + t];
      ks[t].src = zp.src;
      ks[t].size = zp.size;
      ks[t].ip = 0;
      ks[t].lit_buf = lit_base ? lit_base + zp.lit_off : nullptr;
      ks[t].lit_stride = zp.lit_stride;
      ks[t].hblock = 0;
      ks[t].in_frame = ks[t].has_check = ks[t].have = 0;
      ks[t].done = zp.size > 0 ? 0 : 1;
      if (kSkip) {
        const bool have = !kStaged || nframes != nullptr;
        scs[t].f = have ? frames + sp[p0 + t].frame_base : nullptr;
        scs[t].n = have ? nframes[p0 + t] : 0;
        scs[t].at = 0;
      }
      if (kStaged) {
        scs2[t].f = frames2 + sp2[p0 + t].frame_base;
        scs2[t].n = nframes2[p0 + t];
        scs2[t].at = 0;
      }
    }
    s3s_zstd::literal_side<kSkip, kStaged>(lp, ks, np, L, scs, scs2);
    return;
  }
  const int p = p0 + wave;
  if (p >= n) return;
  __builtin_amdgcn_s_setprio(3);  // (the sequence side is the partition's critical path, the literal wavefront has slack: + 4.7 %)
  const ZPart zp = parts[p];
  int64_t total = 0, need = 0;
  int32_t blocks = 0, blocks2 = 0;
  int rc = s3s_zstd::ZS_OK;
  if (zp.size > 0) {
    if (kStaged) {
      const bool have = nframes != nullptr;
      rc = s3s_zstd::decode_partition<true, true>(w[wave], lp[wave], zp.src, zp.size, zp.dst, zp.cap, execute != 0,
                                                  lit_base ? lit_base + zp.lit_off : nullptr, zp.lit_stride, L, &total, &need,
                                                  s3s_zstd::SkipCursor{have ? frames + sp[p].frame_base : nullptr, have ? nframes[p] : 0, 0}, &blocks,
                                                  s3s_zstd::SkipCursor{frames2 + sp2[p].frame_base, nframes2[p], 0}, &blocks2);
    } else if (kSkip)
      rc = s3s_zstd::decode_partition<true>(w[wave], lp[wave], zp.src, zp.size, zp.dst, zp.cap, execute != 0,
                                            lit_base ? lit_base + zp.lit_off : nullptr, zp.lit_stride, L, &total, &need,
                                            s3s_zstd::SkipCursor{frames + sp[p].frame_base, nframes[p], 0}, &blocks);
    else
      rc = s3s_zstd::decode_partition(w[wave], lp[wave], zp.src, zp.size, zp.dst, zp.cap, execute != 0,
                                      lit_base ? lit_base + zp.lit_off : nullptr, zp.lit_stride, L, &total, &need);
  }
  s3s_zstd::pipe_set(&lp[wave].quit, 1, L);  // (a literal side still waiting for a buffer leaves)
  if (L.lane == 0) {
    ZRes r;
    r.total = total;
    r.lit_need = need;
    r.rc = rc;
    r.pad = 0;
    res[p] = r;
    if (kSkip && blocks > 0 && rc == s3s_zstd::ZS_OK) atomicAdd(&ctrl->blocks_done, blocks);
    if (kStaged && blocks2 > 0 && rc == s3s_zstd::ZS_OK) atomicAdd(staged_done, blocks2);
  }
}
#endif

}  // namespace s3s
