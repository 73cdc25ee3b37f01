// zstd_decode_blocks.hip — block-independent Zstandard frames, one workgroup per block.
//
// The frames the map side writes (zstd_compress.hip, S3S_OPT_ZSTD_COMPRESS) are blocks of 128 KiB that never look in front of
// their own first byte; the serial decoder (zstd_decompress.hip: one frame, one sequence wavefront) walks them one after the
// other all the same, which makes a 128 MiB partition a four-second chain.  Here the chain is cut:
//   scan     one lane per partition reads the frame headers and, for the frames whose header promises a window of at most
//            one block, the 3-byte block headers: a table of blocks with their source and output positions;
//   decode   a persistent grid of the serial kernel's workgroups (two sequence wavefronts, one literal wavefront, the same
//            LDS): every sequence wavefront takes blocks of the table, each with the state of a frame's first block;
//   verdict  a block that turns out to need history - or fails in any way - flags its FRAME dependent.  The per-partition
//            kernel runs behind the grid, steps over the frames that completed and decodes all others exactly as it always
//            did, into the same place: their bytes and their error codes are the serial decoder's.
// Nothing here waits for another workgroup; the only waits are the bounded ones between a workgroup's own wavefronts.
#define S3S_ZSTD_DEVICE 1
#include "zstd_decode_blocks.h"

#include <vector>

namespace s3s {
namespace {

using s3s_zstd::BlockJob;
using s3s_zstd::FrameEnt;

constexpr int kScanThreads = 64;
constexpr int64_t kLitStride = (s3s_zstd::kMaxBlock + 64 + 15) & ~15;  // one literal buffer of the grid: a block's largest literals section
constexpr int kBlockGridPerCu = 4;  // resident workgroups per CU of the serial kernel's shape (LDS: 4 x 39 KiB of 160 KiB)

// the smallest output a candidate frame has: two blocks
constexpr int64_t kMinCandidate = s3s_zstd::kMaxBlock + 1;
// A call whose non-empty partitions fill at least half of the serial kernel's resident places (2 per workgroup) keeps the
// machine busy one frame per wavefront, with the literal side a block ahead; cutting its short frames into blocks only adds
// table builds and hand-overs.  Measured (profiles/zstd_block_parallel.md): 1 GiB of TeraSort frames, 1 600 frames of ~6
// blocks 20.4 ms serial / 33.0 ms block path, 800 frames of ~11 blocks 34.1 / 28.5 - the crossover lies between, so such a
// call takes the block path only for frames of at least kBusyMinBlocks blocks.  Smaller calls keep the format's floor of two.
constexpr int32_t kBusyMinBlocks = 10;

__global__ __launch_bounds__(kScanThreads) void zstd_block_scan_kernel(const ZPart* __restrict__ parts, int32_t n, const ZScanPart* __restrict__ sp,
                                                                       FrameEnt* __restrict__ frames, BlockJob* __restrict__ jobs, int32_t job_cap,
                                                                       ZBlockCtrl* __restrict__ ctrl, int32_t* __restrict__ nframes, int32_t min_blocks) {
  const int p = (int)(blockIdx.x * kScanThreads + threadIdx.x);
  if (p >= n) return;
  const ZScanPart s = sp[p];
  int32_t nf = 0;
  if (s.frame_cap > 0) {
    const ZPart zp = parts[p];
    auto reserve = [&](int32_t want) -> int64_t {  // never past job_cap: the counter only moves when the entries exist
      int32_t old = __hip_atomic_load(&ctrl->n_jobs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (;;) {
        if (want > job_cap - old) return -1;
        if (__hip_atomic_compare_exchange_strong(&ctrl->n_jobs, &old, old + want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
          return old;
      }
    };
    nf = s3s_zstd::scan_partition(zp.src, zp.size, zp.cap, p, true, frames + s.frame_base, s.frame_cap, s.frame_base, jobs, reserve, min_blocks);
  }
  nframes[p] = nf;
}

// The literal side of the block grid: for hand-over i of slot t (block t's i-th job) it regenerates the block's Huffman-coded
// literals into buffer i & 1 and says so through lp.ready = i + 1, for EVERY job, Huffman or not, decodable or not: lit_rc[i & 1]
// carries what it found.  A block always brings its own tree here (a treeless one is refused by both sides).
__device__ __forceinline__ void block_literal_side(s3s_zstd::LitPipe* lps, int32_t (*lit_rc)[2], const ZPart* __restrict__ parts,
                                                   const FrameEnt* __restrict__ frames, const BlockJob* __restrict__ jobs, int32_t n_jobs,
                                                   uint8_t* __restrict__ lit_wg, s3s_zstd::Lanes L) {
  using namespace s3s_zstd;
  const int32_t stride = 2 * (int32_t)gridDim.x;
  int32_t it[2] = {0, 0};
  bool live[2] = {true, true};
  int32_t idle = 0;
  for (;;) {
    bool any = false, progressed = false;
    for (int t = 0; t < 2; t++) {
      if (!live[t]) continue;
      const int32_t i = t == 0 ? it[0] : it[1];
      const int64_t j = (int64_t)(2 * (int32_t)blockIdx.x + t) + (int64_t)i * stride;
      if (j >= n_jobs) { live[t] = false; continue; }
      any = true;
      LitPipe& lp = lps[t];
      if (pipe_get(&lp.quit)) { live[t] = false; continue; }
      if (pipe_get(&lp.consumed) < i - 1) continue;  // buffer i & 1 still holds hand-over i - 2
      const BlockJob job = jobs[j];
      int rc = ZS_OK;
      if (job.expect > 0 && job.type == 2) {
        const FrameEnt* fe = frames + job.frame;
        if (__hip_atomic_load(&fe->dependent, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
          rc = ZS_BAD;  // (its frame is the serial decoder's already)
        } else {
          const uint8_t* b = parts[fe->part].src + job.src_off + 3;
          LitHdr lh;
          rc = literals_header(b, job.bsize, &lh);
          if (rc == ZS_OK && lh.ltype >= 2) {
            lp.h.have_huf = 0;
            rc = lh.ltype == 3 || lh.regen > kLitStride - 64
                     ? (int)ZS_BAD
                     : block_literals(lp.h, lh, b + lh.lh, lh.lcomp, lit_wg + (int64_t)(2 * t + (i & 1)) * kLitStride, L);
          }
        }
      }
      if (L.lane == 0) lit_rc[t][i & 1] = rc;
      if (t == 0) it[0]++; else it[1]++;
      pipe_set(&lp.ready, i + 1, L);
      progressed = true;
    }
    if (!any) return;
    if (progressed) {
      idle = 0;
    } else {
      if (++idle >= kPipeSpins) {  // (see kPipeSpins: never in a working machine)
        for (int t = 0; t < 2; t++)
          if (live[t]) pipe_set(&lps[t].err, ZS_BAD, L);
        return;
      }
      __builtin_amdgcn_s_sleep(8);
    }
  }
}

// One workgroup of the serial kernel's shape on a persistent grid: sequence wavefront t takes the jobs 2 * block + t,
// + 2 * grid, ...; the literal wavefront serves both, up to one job ahead of each.
__global__ __launch_bounds__(kZstdThreads, 3) void zstd_block_decode_kernel(const ZPart* __restrict__ parts, FrameEnt* __restrict__ frames,
                                                                           const BlockJob* __restrict__ jobs, const ZBlockCtrl* __restrict__ ctrl,
                                                                           uint8_t* __restrict__ lit_base) {
  using namespace s3s_zstd;
  __shared__ Work w[2];
  __shared__ LitPipe lp[2];
  __shared__ int32_t lit_rc[2][2];
  const int32_t n_jobs = (int32_t)ZS_UNI32(ctrl->n_jobs);
  if (2 * (int32_t)blockIdx.x >= n_jobs) return;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  Lanes L{(int)(threadIdx.x & (kWave - 1)), kWave};
  if (threadIdx.x < 2) lp[threadIdx.x].ready = lp[threadIdx.x].consumed = lp[threadIdx.x].err = lp[threadIdx.x].quit = 0;
  __syncthreads();
  uint8_t* const lit_wg = lit_base + (int64_t)blockIdx.x * 4 * kLitStride;
  if (wave == 2) {
    block_literal_side(lp, lit_rc, parts, frames, jobs, n_jobs, lit_wg, L);
    return;
  }
  __builtin_amdgcn_s_setprio(3);
  const int32_t stride = 2 * (int32_t)gridDim.x;
  int32_t i = 0;
  for (int64_t j = 2 * (int32_t)blockIdx.x + wave; j < n_jobs; j += stride, i++) {
    const BlockJob job = jobs[j];
    FrameEnt* fe = frames + job.frame;
    int rc = ZS_BAD;
    if (job.expect > 0 && !ZS_UNI32(__hip_atomic_load(&fe->dependent, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
      const ZPart zp = parts[fe->part];
      const int64_t stored = job.type == 1 ? 1 : job.bsize;
      // (the scan placed the block inside the partition and its output inside the partition's capacity)
      rc = decode_block(w[wave], lp[wave], zp.src + job.src_off, 3 + stored, zp.dst + job.out_off, job.expect,
                        lit_wg + (int64_t)(2 * wave) * kLitStride, kLitStride, i, L);
    }
    // the literal side hands over every job: wait for this one's (it may still be writing the buffer), then give the buffer back
    const int wrc = pipe_wait_ready(lp[wave], i + 1);
    if (wrc != ZS_OK || lit_rc[wave][i & 1] != ZS_OK) rc = ZS_BAD;
    pipe_set(&lp[wave].consumed, i + 1, L);
    if (L.lane == 0 && job.expect > 0) {
      if (rc == ZS_OK) atomicAdd(&fe->done, 1);
      else __hip_atomic_store(&fe->dependent, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  pipe_set(&lp[wave].quit, 1, L);
}

__global__ __launch_bounds__(kZstdThreads, 3) void zstd_partitions_skip_kernel(const ZPart* __restrict__ parts, int32_t n, int execute,
                                                                              uint8_t* __restrict__ lit_base, ZRes* __restrict__ res,
                                                                              const ZScanPart* __restrict__ sp, const int32_t* __restrict__ nframes,
                                                                              const FrameEnt* __restrict__ frames, ZBlockCtrl* __restrict__ ctrl) {
  __shared__ s3s_zstd::SkipCursor scs[2];  // (the literal wavefront's place in its partitions' frame lists)
  zstd_partitions_body<true>(parts, n, execute, lit_base, res, sp, nframes, frames, ctrl, scs);
}

}  // namespace

int zstd_blocks_launch(s3s_ctx* ctx, const ZPart* h_parts, const ZPart* d_parts, int32_t n_parts, ZBlockPlan* plan) {
  plan->on = false;
  // Bounds from what the host knows, the capacities: a candidate frame decodes to at least kMinCandidate bytes, and a frame of
  // n >= 2 blocks to more than (n - 1) blocks' worth, so a partition of capacity c holds at most c / kMinCandidate candidates
  // (one more entry for the frame the walk stops at) and at most 2 c / kMaxBlock of their blocks.
  std::vector<ZScanPart> sps((size_t)n_parts);
  int64_t n_frames = 0, n_jobs = 0, n_live = 0;
  for (int32_t p = 0; p < n_parts; p++) n_live += h_parts[p].size > 0 ? 1 : 0;
  const int32_t min_blocks = n_live >= (int64_t)ctx->cu_count * kBlockGridPerCu ? kBusyMinBlocks : 2;
  for (int32_t p = 0; p < n_parts; p++) {
    const int64_t c = h_parts[p].size > 0 ? h_parts[p].cap : 0;
    const int64_t fc = c > (int64_t)(min_blocks - 1) * s3s_zstd::kMaxBlock ? c / kMinCandidate + 1 : 0;
    sps[(size_t)p].frame_base = (int32_t)n_frames;
    sps[(size_t)p].frame_cap = (int32_t)fc;
    n_frames += fc;
    if (fc) n_jobs += 2 * c / s3s_zstd::kMaxBlock + 2;
    if (n_frames > 0x7fffff00ll || n_jobs > 0x7fffff00ll) return S3S_OK;  // (beyond 32-bit tables: the serial path alone)
  }
  if (n_frames == 0) return S3S_OK;  // no partition can hold such a frame: nothing is launched
  auto al = [](size_t x) { return (x + 63) & ~size_t(63); };
  const size_t o_ctrl = 0, o_sp = al(sizeof(ZBlockCtrl)), o_nf = al(o_sp + sizeof(ZScanPart) * (size_t)n_parts),
               o_fr = al(o_nf + 4 * (size_t)n_parts), o_jobs = al(o_fr + sizeof(FrameEnt) * (size_t)n_frames),
               total = o_jobs + sizeof(BlockJob) * (size_t)n_jobs;
  const int64_t want_grid = (n_jobs + 1) / 2, max_grid = (int64_t)ctx->cu_count * kBlockGridPerCu;
  const unsigned grid = (unsigned)(want_grid < max_grid ? want_grid : max_grid);
  int e = ensure(ctx, B_ZBLOCKS, total);
  if (e == S3S_OK) e = ensure(ctx, B_ZBLOCK_LIT, (size_t)grid * 4 * (size_t)kLitStride + 64);
  if (e == S3S_E_NOMEM) {  // not this call's verdict: the serial path needs none of it
    (void)hipGetLastError();
    ctx->err[0] = 0;
    return S3S_OK;
  }
  if (e != S3S_OK) return e;
  uint8_t* base = dev<uint8_t>(ctx, B_ZBLOCKS);
  ZBlockCtrl* d_ctrl = reinterpret_cast<ZBlockCtrl*>(base + o_ctrl);
  ZScanPart* d_sp = reinterpret_cast<ZScanPart*>(base + o_sp);
  int32_t* d_nf = reinterpret_cast<int32_t*>(base + o_nf);
  FrameEnt* d_frames = reinterpret_cast<FrameEnt*>(base + o_fr);
  BlockJob* d_jobs = reinterpret_cast<BlockJob*>(base + o_jobs);
  HIP_TRY(ctx, hipMemsetAsync(d_ctrl, 0, sizeof(ZBlockCtrl), ctx->stream));
  // (pageable source: the copy is staged by the runtime before the call returns)
  HIP_TRY(ctx, hipMemcpyAsync(d_sp, sps.data(), sizeof(ZScanPart) * (size_t)n_parts, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(zstd_block_scan_kernel, dim3((unsigned)((n_parts + kScanThreads - 1) / kScanThreads)), dim3(kScanThreads), 0, ctx->stream, d_parts,
                     n_parts, d_sp, d_frames, d_jobs, (int32_t)n_jobs, d_ctrl, d_nf, min_blocks);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(zstd_block_decode_kernel, dim3(grid), dim3(kZstdThreads), 0, ctx->stream, d_parts, d_frames, d_jobs, d_ctrl,
                     dev<uint8_t>(ctx, B_ZBLOCK_LIT));
  HIP_TRY(ctx, hipGetLastError());
  plan->on = true;
  plan->d_ctrl = d_ctrl;
  plan->d_sp = d_sp;
  plan->d_nframes = d_nf;
  plan->d_frames = d_frames;
  return S3S_OK;
}

void zstd_partitions_skip_launch(s3s_ctx* ctx, const ZPart* d_parts, int32_t n_parts, uint8_t* d_lit, ZRes* d_res, const ZBlockPlan& plan) {
  hipLaunchKernelGGL(zstd_partitions_skip_kernel, dim3((unsigned)((n_parts + 1) / 2)), dim3(kZstdThreads), 0, ctx->stream, d_parts, n_parts, 1, d_lit,
                     d_res, plan.d_sp, plan.d_nframes, plan.d_frames, plan.d_ctrl);
}

}  // namespace s3s
