// lz4_compress_ring.hip — lz4_compress_ring_kernel (S3S_OPT_LZ4_VARIANT 11): the exact-window kernel of lz4_compress.hip built
// with the window block's input ring (lz4_window_engine.inc, S3S_LZ4_RING): same arguments, 16 KiB table at LDS offset 0, the
// 4 KiB ring behind it.  A build of its own, so that lz4_compress_l2_kernel<> stays what it is, instruction for instruction.
#define S3S_LZ4_RING 1
#include "lz4_compress.hip"
