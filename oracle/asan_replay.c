/* Replays, under AddressSanitizer / UBSan, every decode that the damaged-range model of tests/stream_damage.py asks of the
 * oracle (the model rests on these decoders surviving hostile bytes).  Stand-alone: built by `make asan_replay`, never loaded
 * into Python.  Input: records of [u32 codec][u32 capacity][u32 length][bytes] (codec | 0x100: a whole
 * partition through the stream decoder, else one unit), as `python tests/stream_damage.py --dump FILE`
 * writes them.  Source and destination are heap blocks of exactly their sizes, so a read or write outside either is reported. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "s3s_oracle.h"

int main(int argc, char** argv) {
  if (argc != 2) return fprintf(stderr, "usage: %s FILE\n", argv[0]), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return perror(argv[1]), 2;
  uint32_t h[3];
  long n = 0, ok = 0;
  while (fread(h, 4, 3, f) == 3) {
    uint8_t* src = malloc(h[2] ? h[2] : 1);
    uint8_t* dst = malloc(h[1] ? h[1] : 1);
    if (!src || !dst || fread(src, 1, h[2], f) != h[2]) return fprintf(stderr, "short record %ld\n", n), 2;
    int64_t r;
    switch (h[0]) {
      case S3O_CODEC_LZ4: r = s3o_lz4block_decompress_stream(src, h[2], dst, h[1]); break;
      case S3O_CODEC_SNAPPY: r = s3o_snappy_decompress_stream(src, h[2], dst, h[1]); break;
      case S3O_CODEC_LZ4 | 0x100: r = s3o_lz4block_decompress_stream(src, h[2], dst, h[1]); break;
      case S3O_CODEC_SNAPPY | 0x100: r = s3o_snappy_decompress_stream(src, h[2], dst, h[1]); break;
      case S3O_CODEC_LZF | 0x100: r = s3o_lzf_decompress_stream(src, h[2], dst, h[1]); break;
      case S3O_CODEC_LZF: r = s3o_lzf_decompress_block(src, (int)h[2], dst, (int)h[1]); break;
      default: return fprintf(stderr, "unknown codec %u in record %ld\n", h[0], n), 2;
    }
    ok += r >= 0;
    n++;
    free(src);
    free(dst);
  }
  fclose(f);
  printf("%ld decodes replayed, %ld accepted, %ld refused\n", n, ok, n - ok);
  return 0;
}
