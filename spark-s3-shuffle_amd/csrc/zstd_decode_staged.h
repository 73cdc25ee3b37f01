// zstd_decode_staged.h — host interface of the staged Zstandard path (zstd_decode_staged.hip) for the
// orchestration in zstd_decompress.hip.
#pragma once
#include "zstd_decode_blocks.h"

namespace s3s {

struct ZStagedCtrl {     // device memory, zeroed per call
  int32_t n_blocks;      // entries of the block table handed out by the scan
  int32_t blocks_done;   // blocks of the frames the per-partition kernel stepped over (S3S_OPT_ZSTD_DECODE_STAGED_BLOCKS)
  int64_t lit_used;      // bytes of the literal staging handed out
  int64_t rec_used;      // records handed out
};
struct ZStagedPlan {     // one call's staged path; on = false: nothing was launched
  bool on = false;
  ZStagedCtrl* d_ctrl = nullptr;
  const ZScanPart* d_sp = nullptr;
  const int32_t* d_nframes = nullptr;
  const s3s_zstd::FrameEnt* d_frames = nullptr;
};

// Workgroups (of one wavefront each) of the entropy and copy grids at the most: persistent, a job at a time each, however many
// blocks a call holds - 8 per compute unit of a 256-CU device.  No workgroup waits for another, so nothing depends on all of
// them being resident.  The host never learns how many blocks the scan found (that would be a wait), so every grid is sized
// from a CAPACITY: entropy and copy from the block table's (comp / 32 + 64 entries: only a call of less than 64 KiB of
// compressed data launches fewer than kStagedGrid), execute one workgroup per slot of the frame table (kStagedFramesPerPart per
// partition that can hold a frame).  A workgroup that finds no job or an empty slot returns at once.
constexpr int kStagedGrid = 2048;

// Scan, entropy, place, copy and execute over the partitions h_parts[0, n_parts) (already uploaded to d_parts, destinations and
// capacities final), behind the block path's kernels when plan13.on.  budget: bytes the staging may take (it is scaled down to
// it); an allocation that does not fit only switches the path off for the call.
int zstd_staged_launch(s3s_ctx* ctx, const ZPart* h_parts, const ZPart* d_parts, int32_t n_parts, const ZBlockPlan& plan13, int64_t budget,
                       ZStagedPlan* plan);
// the per-partition kernel behind both paths: frames either completed are stepped over, every other frame is decoded as ever
void zstd_partitions_staged_launch(s3s_ctx* ctx, const ZPart* d_parts, int32_t n_parts, uint8_t* d_lit, ZRes* d_res, const ZBlockPlan& plan13,
                                   const ZStagedPlan& plan);

}  // namespace s3s
