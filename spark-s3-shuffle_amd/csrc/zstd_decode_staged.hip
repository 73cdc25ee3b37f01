// zstd_decode_staged.hip — Zstandard frames with history across their blocks, decoded in stages.
//
// A frame of zstd-jni / libzstd's streaming API has no content size, a window of 512 KiB or more and matches that reach into
// earlier blocks, so the block path of 6j leaves it to the serial decoder: one wavefront, block after block, ~190 instructions
// per sequence.  Most of that chain is entropy decoding, which does not depend on earlier blocks at all once the block that
// defined a repeated table or tree is known - and that follows from the headers.  The kernels here, in stream order:
//   scan     one lane per partition: frame and block headers of the eligible frames, a table of blocks with their staging;
//   entropy  a persistent grid, one wavefront per workgroup, two jobs per block in any order: its Huffman literals into the
//            literal staging, its sequences into records (literal length, match length, raw offset value as positions);
//   place    one wavefront per partition: prefix sums of the decoded lengths - where every block and frame lands;
//   copy     the entropy grid's shape, a block per step: Raw / RLE blocks and all literal runs;
//   execute  one wavefront per frame: repeat offsets resolved, match sources checked, matches copied - the serial chain left;
//   verdict  the per-partition kernel behind them steps over the frames that completed and decodes every other frame exactly as
//            it always did, into the same place: their bytes and their error codes are the serial decoder's.
// Stage order is stream order.  No workgroup waits for another one, and a workgroup here is one wavefront: there is no wait at
// all in these kernels.  The functions are zstd_decode_core.h's, the ones the host model runs.
#define S3S_ZSTD_DEVICE 1
#include "zstd_decode_staged.h"

#include <vector>

namespace s3s {
namespace {

using s3s_zstd::FrameEnt;
using s3s_zstd::SeqRec;
using s3s_zstd::StagedBlock;

constexpr int kScanThreads = 64;
constexpr int64_t kMinStagedPartition = 12;  // a frame header (6 bytes at least) and two block headers

__global__ __launch_bounds__(kScanThreads) void zstd_staged_scan_kernel(const ZPart* __restrict__ parts, int32_t n, const ZScanPart* __restrict__ sp13,
                                                                        const int32_t* __restrict__ nframes13, const FrameEnt* __restrict__ frames13,
                                                                        const ZScanPart* __restrict__ sp, FrameEnt* __restrict__ frames,
                                                                        int32_t* __restrict__ block_base, int32_t* __restrict__ nframes,
                                                                        StagedBlock* __restrict__ tab, ZStagedCtrl* __restrict__ ctrl, int32_t blk_cap,
                                                                        int64_t lit_cap, int64_t rec_cap) {
  const int p = (int)(blockIdx.x * kScanThreads + threadIdx.x);
  if (p >= n) return;
  const ZScanPart s = sp[p];
  int32_t nf = 0;
  if (s.frame_cap > 0) {
    const ZPart zp = parts[p];
    int64_t ip0 = 0, op0 = 0;
    if (nframes13) {  // the block path of 6j claimed a prefix of the frames: behind the ones whose headers added up
      const FrameEnt* f13 = frames13 + sp13[p].frame_base;
      const int32_t n13 = nframes13[p];
      for (int32_t k = 0; k < n13; k++) {
        const FrameEnt fe = f13[k];
        if (fe.consumed <= 0) break;
        ip0 = fe.src_off + fe.consumed;
        op0 = fe.out_off + fe.fcs;
      }
    }
    auto reserve = [&](int which, int64_t want) -> int64_t {  // never past a table's size: a counter only moves when the entries exist
      if (which == 0) {
        int32_t old = __hip_atomic_load(&ctrl->n_blocks, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (;;) {
          if (want > (int64_t)(blk_cap - old)) return -1;
          if (__hip_atomic_compare_exchange_strong(&ctrl->n_blocks, &old, old + (int32_t)want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return old;
        }
      }
      int64_t* const ctr = which == 1 ? &ctrl->lit_used : &ctrl->rec_used;
      const int64_t cap = which == 1 ? lit_cap : rec_cap;
      int64_t old = __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (;;) {
        if (want > cap - old) return -1;
        if (__hip_atomic_compare_exchange_strong(ctr, &old, old + want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return old;
      }
    };
    if (ip0 >= 0 && ip0 < zp.size)
      nf = s3s_zstd::staged_scan_partition(zp.src, zp.size, p, ip0, op0, frames + s.frame_base, block_base + s.frame_base, s.frame_cap, s.frame_base, tab,
                                           reserve);
    for (int32_t k = nf; k < s.frame_cap; k++) frames[s.frame_base + k].n_blocks = 0;  // (slots the execute grid finds empty)
  }
  nframes[p] = nf;
}

union StagedLds {
  s3s_zstd::SeqWork sw;
  s3s_zstd::HufWork hw;
};

// Job j < n_blocks: the sequences of block j; job n_blocks + j: its Huffman literals.  Any failure flags the block's frame.
__global__ __launch_bounds__(kWave) void zstd_staged_entropy_kernel(const ZPart* __restrict__ parts, int32_t n_parts, FrameEnt* __restrict__ frames,
                                                                   int32_t n_frames, const StagedBlock* __restrict__ tab, int32_t* __restrict__ comp_len,
                                                                   const ZStagedCtrl* __restrict__ ctrl, int32_t blk_cap,
                                                                   uint8_t* __restrict__ lit_pool, int64_t lit_cap,
                                                                   SeqRec* __restrict__ rec_pool, int64_t rec_cap) {
  using namespace s3s_zstd;
  __shared__ StagedLds lds;
  int32_t n_blocks = (int32_t)ZS_UNI32(ctrl->n_blocks);
  n_blocks = n_blocks < blk_cap ? n_blocks : blk_cap;
  Lanes L{(int)threadIdx.x, kWave};
  for (int64_t j = blockIdx.x; j < 2 * (int64_t)n_blocks; j += gridDim.x) {
    const int32_t bi = (int32_t)(j < n_blocks ? j : j - n_blocks);
    const bool literals = j >= n_blocks;
    const StagedBlock blk = tab[bi];
    if (blk.type != 2 || blk.frame < 0 || blk.frame >= n_frames) continue;
    if (literals && blk.ltype < 2) continue;
    FrameEnt* fe = frames + blk.frame;
    const int32_t part = fe->part;
    if (part < 0 || part >= n_parts) continue;
    const uint8_t* psrc = parts[part].src;
    int rc;
    if (literals) {
      rc = staged_block_literals(lds.hw, psrc, tab, bi, lit_pool, lit_cap, L);
    } else {
      int32_t out_len = 0;
      rc = staged_block_sequences(lds.sw, psrc, tab, bi, rec_pool, rec_cap, &out_len, L);
      if (rc == ZS_OK && L.lane == 0) comp_len[bi] = out_len;  // (beside the table: other jobs of this grid read tab[bi])
    }
    if (rc != ZS_OK && L.lane == 0) __hip_atomic_store(&fe->dependent, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ZS_FENCE();  // (the tables in LDS are the next job's to overwrite)
  }
}

__global__ __launch_bounds__(kWave) void zstd_staged_place_kernel(const ZPart* __restrict__ parts, int32_t n, const ZScanPart* __restrict__ sp,
                                                                 const int32_t* __restrict__ nframes, FrameEnt* __restrict__ frames,
                                                                 const int32_t* __restrict__ block_base, StagedBlock* __restrict__ tab,
                                                                 const int32_t* __restrict__ comp_len) {
  const int p = (int)blockIdx.x;
  if (p >= n) return;
  const int32_t nf = nframes[p];
  if (nf <= 0) return;
  s3s_zstd::Lanes L{(int)threadIdx.x, kWave};
  const int32_t base = sp[p].frame_base;
  s3s_zstd::staged_place_partition(frames + base, block_base + base, nf, tab, comp_len, parts[p].cap, L);
}

__global__ __launch_bounds__(kWave) void zstd_staged_copy_kernel(const ZPart* __restrict__ parts, int32_t n_parts, const FrameEnt* __restrict__ frames,
                                                                int32_t n_frames, const StagedBlock* __restrict__ tab, const ZStagedCtrl* __restrict__ ctrl,
                                                                int32_t blk_cap, const uint8_t* __restrict__ lit_pool, const SeqRec* __restrict__ rec_pool) {
  using namespace s3s_zstd;
  int32_t n_blocks = (int32_t)ZS_UNI32(ctrl->n_blocks);
  n_blocks = n_blocks < blk_cap ? n_blocks : blk_cap;
  Lanes L{(int)threadIdx.x, kWave};
  for (int32_t bi = (int32_t)blockIdx.x; bi < n_blocks; bi += (int32_t)gridDim.x) {
    const StagedBlock blk = tab[bi];
    if (blk.frame < 0 || blk.frame >= n_frames) continue;
    const FrameEnt fe = frames[blk.frame];
    if (fe.dependent || fe.part < 0 || fe.part >= n_parts) continue;
    const ZPart zp = parts[fe.part];
    // (place put the frame, and with it every block, inside the partition's capacity)
    staged_block_copy(zp.src, zp.dst, blk, rec_pool, lit_pool, L);
  }
}

__global__ __launch_bounds__(kWave) void zstd_staged_execute_kernel(const ZPart* __restrict__ parts, int32_t n_parts, FrameEnt* __restrict__ frames,
                                                                   int32_t n_frames, const int32_t* __restrict__ block_base,
                                                                   const StagedBlock* __restrict__ tab, int32_t blk_cap, const SeqRec* __restrict__ rec_pool) {
  using namespace s3s_zstd;
  const int32_t f = (int32_t)blockIdx.x;
  if (f >= n_frames) return;
  const FrameEnt fe = frames[f];
  if (fe.n_blocks <= 0 || fe.dependent || fe.part < 0 || fe.part >= n_parts) return;
  const int32_t bb = block_base[f];
  if (bb < 0 || fe.n_blocks > blk_cap - bb) return;
  Lanes L{(int)threadIdx.x, kWave};
  const int rc = staged_execute_frame(fe, tab + bb, rec_pool, parts[fe.part].dst + fe.out_off, L);
  if (L.lane == 0) {
    if (rc == ZS_OK) frames[f].done = fe.n_blocks;
    else frames[f].dependent = 1;
  }
}

__global__ __launch_bounds__(kZstdThreads, 3) void zstd_partitions_staged_kernel(const ZPart* __restrict__ parts, int32_t n, int execute,
                                                                                uint8_t* __restrict__ lit_base, ZRes* __restrict__ res,
                                                                                const ZScanPart* __restrict__ sp13, const int32_t* __restrict__ nframes13,
                                                                                const FrameEnt* __restrict__ frames13, ZBlockCtrl* __restrict__ ctrl13,
                                                                                const ZScanPart* __restrict__ sp, const int32_t* __restrict__ nframes,
                                                                                const FrameEnt* __restrict__ frames, ZStagedCtrl* __restrict__ ctrl) {
  __shared__ s3s_zstd::SkipCursor scs[2], scs2[2];  // (the literal wavefront's place in its partitions' two frame lists)
  zstd_partitions_body<true, true>(parts, n, execute, lit_base, res, sp13, nframes13, frames13, ctrl13, scs, sp, nframes, frames, &ctrl->blocks_done, scs2);
}

}  // namespace

int zstd_staged_launch(s3s_ctx* ctx, const ZPart* h_parts, const ZPart* d_parts, int32_t n_parts, const ZBlockPlan& plan13, int64_t budget,
                       ZStagedPlan* plan) {
  plan->on = false;
  std::vector<ZScanPart> sps((size_t)n_parts);
  int64_t n_frames = 0, comp = 0;
  for (int32_t p = 0; p < n_parts; p++) {
    const bool live = h_parts[p].size >= kMinStagedPartition;
    sps[(size_t)p].frame_base = (int32_t)n_frames;
    sps[(size_t)p].frame_cap = live ? s3s_zstd::kStagedFramesPerPart : 0;
    if (live) {
      n_frames += s3s_zstd::kStagedFramesPerPart;
      comp += h_parts[p].size;
    }
    if (n_frames > 0x7fffff00ll) return S3S_OK;  // (beyond 32-bit tables: the serial path alone)
  }
  if (n_frames == 0) return S3S_OK;
  // The staging, from the compressed bytes alone; scaled down to the budget where it would pass it (the frames that then do
  // not fit stay with the serial decoder).
  int64_t blk_cap = s3s_zstd::staged_block_cap(comp), lit_cap = s3s_zstd::staged_lit_cap(comp), rec_cap = s3s_zstd::staged_rec_cap(comp);
  const int64_t want = (int64_t)sizeof(StagedBlock) * blk_cap + lit_cap + (int64_t)sizeof(SeqRec) * rec_cap;
  if (budget <= 0) return S3S_OK;
  if (want > budget) {
    const double f = (double)budget / (double)want;
    blk_cap = (int64_t)((double)blk_cap * f);
    lit_cap = (int64_t)((double)lit_cap * f);
    rec_cap = (int64_t)((double)rec_cap * f);
  }
  if (blk_cap > 0x3fffff00ll) blk_cap = 0x3fffff00ll;
  if (blk_cap < 2) return S3S_OK;
  auto al = [](size_t x) { return (x + 63) & ~size_t(63); };
  const size_t o_ctrl = 0, o_sp = al(sizeof(ZStagedCtrl)), o_nf = al(o_sp + sizeof(ZScanPart) * (size_t)n_parts), o_fr = al(o_nf + 4 * (size_t)n_parts),
               o_bb = al(o_fr + sizeof(FrameEnt) * (size_t)n_frames), o_tab = al(o_bb + 4 * (size_t)n_frames),
               o_len = al(o_tab + sizeof(StagedBlock) * (size_t)blk_cap), total = o_len + 4 * (size_t)blk_cap;
  const size_t o_rec = al((size_t)lit_cap + 64), pool_total = o_rec + sizeof(SeqRec) * (size_t)rec_cap + 64;
  int e = ensure(ctx, B_ZSTAGED, total);
  if (e == S3S_OK) e = ensure(ctx, B_ZSTAGED_POOL, pool_total);
  if (e == S3S_E_NOMEM) {  // not this call's verdict: the serial path needs none of it
    (void)hipGetLastError();
    ctx->err[0] = 0;
    return S3S_OK;
  }
  if (e != S3S_OK) return e;
  uint8_t* base = dev<uint8_t>(ctx, B_ZSTAGED);
  ZStagedCtrl* d_ctrl = reinterpret_cast<ZStagedCtrl*>(base + o_ctrl);
  ZScanPart* d_sp = reinterpret_cast<ZScanPart*>(base + o_sp);
  int32_t* d_nf = reinterpret_cast<int32_t*>(base + o_nf);
  FrameEnt* d_frames = reinterpret_cast<FrameEnt*>(base + o_fr);
  int32_t* d_bb = reinterpret_cast<int32_t*>(base + o_bb);
  StagedBlock* d_tab = reinterpret_cast<StagedBlock*>(base + o_tab);
  int32_t* d_len = reinterpret_cast<int32_t*>(base + o_len);
  uint8_t* d_lit = dev<uint8_t>(ctx, B_ZSTAGED_POOL);
  SeqRec* d_rec = reinterpret_cast<SeqRec*>(d_lit + o_rec);
  HIP_TRY(ctx, hipMemsetAsync(d_ctrl, 0, sizeof(ZStagedCtrl), ctx->stream));
  // (pageable source: the copy is staged by the runtime before the call returns)
  HIP_TRY(ctx, hipMemcpyAsync(d_sp, sps.data(), sizeof(ZScanPart) * (size_t)n_parts, hipMemcpyHostToDevice, ctx->stream));
  const bool with13 = plan13.on;
  hipLaunchKernelGGL(zstd_staged_scan_kernel, dim3((unsigned)((n_parts + kScanThreads - 1) / kScanThreads)), dim3(kScanThreads), 0, ctx->stream, d_parts,
                     n_parts, with13 ? plan13.d_sp : nullptr, with13 ? plan13.d_nframes : nullptr, with13 ? plan13.d_frames : nullptr, d_sp, d_frames, d_bb,
                     d_nf, d_tab, d_ctrl, (int32_t)blk_cap, lit_cap, rec_cap);
  HIP_TRY(ctx, hipGetLastError());
  const int64_t max_grid = kStagedGrid;
  const unsigned grid2 = (unsigned)(2 * blk_cap < max_grid ? 2 * blk_cap : max_grid);
  const unsigned grid1 = (unsigned)(blk_cap < max_grid ? blk_cap : max_grid);
  hipLaunchKernelGGL(zstd_staged_entropy_kernel, dim3(grid2), dim3(kWave), 0, ctx->stream, d_parts, n_parts, d_frames, (int32_t)n_frames, d_tab, d_len,
                     d_ctrl, (int32_t)blk_cap, d_lit, lit_cap, d_rec, rec_cap);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(zstd_staged_place_kernel, dim3((unsigned)n_parts), dim3(kWave), 0, ctx->stream, d_parts, n_parts, d_sp, d_nf, d_frames, d_bb, d_tab,
                     d_len);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(zstd_staged_copy_kernel, dim3(grid1), dim3(kWave), 0, ctx->stream, d_parts, n_parts, d_frames, (int32_t)n_frames, d_tab, d_ctrl,
                     (int32_t)blk_cap, d_lit, d_rec);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(zstd_staged_execute_kernel, dim3((unsigned)n_frames), dim3(kWave), 0, ctx->stream, d_parts, n_parts, d_frames, (int32_t)n_frames, d_bb,
                     d_tab, (int32_t)blk_cap, d_rec);
  HIP_TRY(ctx, hipGetLastError());
  plan->on = true;
  plan->d_ctrl = d_ctrl;
  plan->d_sp = d_sp;
  plan->d_nframes = d_nf;
  plan->d_frames = d_frames;
  return S3S_OK;
}

void zstd_partitions_staged_launch(s3s_ctx* ctx, const ZPart* d_parts, int32_t n_parts, uint8_t* d_lit, ZRes* d_res, const ZBlockPlan& plan13,
                                   const ZStagedPlan& plan) {
  const bool with13 = plan13.on;
  hipLaunchKernelGGL(zstd_partitions_staged_kernel, dim3((unsigned)((n_parts + 1) / 2)), dim3(kZstdThreads), 0, ctx->stream, d_parts, n_parts, 1, d_lit,
                     d_res, with13 ? plan13.d_sp : nullptr, with13 ? plan13.d_nframes : nullptr, with13 ? plan13.d_frames : nullptr,
                     with13 ? plan13.d_ctrl : nullptr, plan.d_sp, plan.d_nframes, plan.d_frames, plan.d_ctrl);
}

}  // namespace s3s
