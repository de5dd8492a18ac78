// Host check of the re-draw of a determinized fork (monsoon_amd/csrc/determinize.h det_swaps / det_source, the text the
// kernel compiles), built by tests/test_env_determinize_cpu.py as a stand-alone program.  Never loaded into Python.
//   determinize_check <in> <out>
// <in>: n little-endian uint32 seeds; <out>: for every seed, every k in 0..5 and every d in 0..12, in that order, the k + d
// bytes det_source(l) for l < k + d -- the index in A of the entry that place l receives.  The test compares them with
// numpy's (monsoon_amd/vec_env.py determinize_order).  Prints "ok n".
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "determinize.h"

int main(int argc, char** argv) {
  if (argc != 3) {
    printf("usage: determinize_check <in> <out>\n");
    return 2;
  }
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) {
    printf("FAIL cannot read %s\n", argv[1]);
    return 1;
  }
  std::vector<uint32_t> seeds;
  uint32_t buf[1024];
  size_t got;
  while ((got = fread(buf, sizeof(uint32_t), 1024, fi)) > 0) seeds.insert(seeds.end(), buf, buf + got);
  fclose(fi);
  std::vector<uint8_t> out;
  for (uint32_t seed : seeds)
    for (int k = 0; k <= msb::DET_HAND_MAX; k++)
      for (int d = 0; d <= msb::DET_DECK_MAX; d++) {
        int j[msb::DET_HAND_MAX];
        msb::det_swaps(seed, k, d, j);
        for (int i = 0; i < k; i++)
          if (j[i] < i || j[i] >= k + d) {
            printf("FAIL swap partner out of range: seed %u k %d d %d i %d j %d\n", seed, k, d, i, j[i]);
            return 1;
          }
        for (int l = 0; l < k + d; l++) out.push_back((uint8_t)msb::det_source(j, k, l));
      }
  FILE* fo = fopen(argv[2], "wb");
  if (!fo || fwrite(out.data(), 1, out.size(), fo) != out.size()) {
    printf("FAIL cannot write %s\n", argv[2]);
    return 1;
  }
  fclose(fo);
  printf("ok %zu\n", seeds.size());
  return 0;
}
