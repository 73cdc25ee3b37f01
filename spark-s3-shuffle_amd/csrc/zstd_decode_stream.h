// zstd_decode_stream.h — host interface of the resumable Zstandard kernels (zstd_decode_stream.hip) for the
// streaming reduce side (decode_stream.hip).
#pragma once
#include "zstd_stream_core.h"

namespace s3s {

// one launch of the resumable decoder: workgroup p runs the units [unit_base[p], min(unit_base[p + 1], k)) of piece p
struct ZStreamRun {
  const uint8_t* comp;                   // the window
  const s3s_zstd::ZUnit* units;
  uint32_t* dsize;                       // decoded size per unit: written by the size pass, demanded by the execute pass
  const int64_t* unit_out;               // exclusive scan of dsize (execute pass only)
  const int64_t* unit_base;              // first unit of every piece, n_pieces + 1 entries
  int64_t k;                             // units to run: all of them (size pass) or the capacity cut's
  int32_t execute, resumed;              // resumed: piece 0 starts inside the stream's open frame
  const s3s_zstd::ZStreamState* st_in;   // ... whose saved state this is
  s3s_zstd::ZStreamState* st_out;        // execute pass: where the frame left open behind unit k - 1 saves its state (or null)
  uint8_t* dst;
  uint8_t* staging;                      // [saved history hist_len | what the resumed frame decodes in this feed]
  int64_t hist_len;
  uint8_t* lit;                          // literal scratch, lit_stride bytes per piece
  int64_t lit_stride;
  int32_t* status;
  int64_t* result;                       // [0] = bytes the resumed frame produced (piece 0)
};

// The unit walk, one lane per piece (walk_piece): counts (emit = false: d_piece_units[p], d_result = {stop, need} of the last
// piece) or writes d_units / d_dsize at d_unit_base[p].  first_open: a frame is open at the window's start; last_pend: where
// the last piece's partition ends (>= the window's end); wmax: the largest Window_Size the stream takes.
void launch_zstd_walk(const uint8_t* d_comp, const int64_t* d_piece_off, int32_t n_pieces, int32_t first_open, int64_t last_pend,
                      int64_t wmax, bool emit, const int64_t* d_unit_base, uint32_t* d_piece_units, void* d_units, uint32_t* d_dsize,
                      int32_t* d_status, int64_t* d_result, hipStream_t st);
void launch_zstd_stream(const ZStreamRun& run, int32_t n_pieces, hipStream_t st);
// d_result = {k, consumed, out_len, need, open, frame unit, Window_Size, out start} (zstd_units_cut_kernel)
void launch_zstd_units_cut(const uint8_t* d_comp, const void* d_units, const uint32_t* d_dsize, const int64_t* d_unit_out, int64_t n_units,
                           int64_t dst_capacity, int64_t stop, int32_t first_open, int64_t* d_result, hipStream_t st);

}  // namespace s3s
