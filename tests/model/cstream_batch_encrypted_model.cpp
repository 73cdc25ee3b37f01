// cstream_batch_encrypted_model.cpp — the host arithmetic of the batched feed of the streaming map side UNDER IO ENCRYPTION
// (spark-s3-shuffle_amd/csrc/compress_stream_batch_core.h) as a stand-alone program: the slices of the call's
// IVs, which entries are windows of the batch, the plan records WITH IV records, the IVs, the pass descriptors and the
// tile -> window map in ONE arena of exactly Arena::total bytes, and, behind the "download", the check of every window's
// words and the per-entry commit with the IV bookkeeping.  tests/test_compress_stream_batch_encrypted_cpu.py builds it with
// -fsanitize=address,undefined, plays the kernels over a pipe - the encrypt pass from the descriptors and the map this
// program prints - and compares every entry's answer and every stream's state, its IV included, with the Python model of the
// contract (tests/cstream_units_encrypted.py).  The protocol is tests/model/cstream_batch_model.cpp's, extended; the body is
// that program's too (cstream_batch_model.h, run<true>).
//
// stdin:   codec bs fresh with_sums n_streams, then n_streams epochs (1: the context's current key setting, 0: an earlier one)
//          rounds:  "R n n_ivs", n_ivs x 32 hex digits (or "-"), then n lines  stream addr src_len cap n_ends end...
// stdout:  "V" = the IV count is not the sum of the slices (S3S_E_INVALID for the call, every stream unchanged);
//          per round with windows:  "P m N PP P L", m lines "W ..." and "I", "M", "F", "S", "E" as in cstream_batch_model.cpp (an
//          IV record prints as kind 2: sixteen bytes without a slot), then "T tiles", m lines "D E ivs cut n_pieces tile0 front
//          out" (E / ivs / cut: the element the pointer names in the call's piece offsets / IVs / result words), "Q" the
//          tile -> window map, "H" the call's IVs in hex; then it READS the downloaded words.  "X" = impossible words.
//          per entry:  "A status consumed out_len need_src need_dst parts_closed n length... sum... pos written open_bytes
//          open_img carry iv"
#include "cstream_batch_model.h"

int main() { return run<true>(); }
