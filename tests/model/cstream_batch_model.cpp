// cstream_batch_model.cpp — the host arithmetic of the batched feed of the streaming map side
// (spark-s3-shuffle_amd/csrc/compress_stream_batch_core.h) as a stand-alone program: which entries are windows of the batch,
// their places in the call's packed arrays, the plan records and descriptors in ONE arena of exactly Arena::total bytes, and,
// behind the "download", the check of every window's words and the per-entry take step - every rule a call of the function
// compress_stream.hip calls (the body, shared with cstream_batch_encrypted_model.cpp: cstream_batch_model.h).  tests/test_compress_stream_batch_cpu.py
// builds it with -fsanitize=address,undefined, plays the kernels over a pipe (the scan, the cut, the clamped piece offsets, the
// lengths, the seeded checksums - from the plan this program prints, by the indices the descriptors hold) and compares every
// entry's answer and every stream's state with the Python model of the contract (tests/cstream_units.py).
//
// stdin:   codec bs fresh with_sums n_streams
//          rounds:  "R n", then n lines  stream addr src_len cap n_ends end...      (n_ends < 0: no ends follow)
// stdout:  per round with windows:  "P m N PP P L", m lines "W e first_item n_items first_pp n_pieces first_piece first_len
//          first_last ends0 cap open_img", "I" N x (src_off len kind piece), "M" N x (src_end last ends_after), "F" PP
//          part_first, "S" P seeds, "E" P piece -> window; then it READS one line: m status words, 8 m result words, PP piece
//          offsets, L lengths, P sums.  "X" = the words were impossible (S3S_E_HIP, nothing committed).
//          per entry:  "A status consumed out_len need_src need_dst parts_closed n length... sum... pos written open_bytes
//          open_img carry"
#include "cstream_batch_model.h"

int main() { return run<false>(); }
