// Host check of the weight function of monsoon_rollout_sample (monsoon_amd/csrc/sample_weight.h weight24, the text the
// kernels compile), built by tests/test_rollout_sample_cpu.py twice: with -O2 -ffp-contract=off as the library is, and
// with the address and UB sanitizers.  Never loaded into Python.
//   sample_weight_check <in> <out>
// <in>: n little-endian doubles, the x of every point; <out>: n little-endian uint32, weight24(x).  The test compares them
// with numpy's (monsoon_amd/game_log.py sample_weights) bit for bit.  Prints "ok n" and the three fixed points the header
// of include/monsoon.h quotes.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "sample_weight.h"

int main(int argc, char** argv) {
  if (argc != 3) {
    printf("usage: sample_weight_check <in> <out>\n");
    return 2;
  }
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) {
    printf("FAIL cannot read %s\n", argv[1]);
    return 1;
  }
  std::vector<double> x;
  double buf[1024];
  size_t got;
  while ((got = fread(buf, sizeof(double), 1024, fi)) > 0) x.insert(x.end(), buf, buf + got);
  fclose(fi);
  std::vector<uint32_t> w(x.size());
  for (size_t i = 0; i < x.size(); i++) w[i] = msb::weight24(x[i]);
  FILE* fo = fopen(argv[2], "wb");
  if (!fo || fwrite(w.data(), sizeof(uint32_t), w.size(), fo) != w.size()) {
    printf("FAIL cannot write %s\n", argv[2]);
    return 1;
  }
  fclose(fo);
  if (msb::weight24(0.0) != msb::SAMPLE_ONE || msb::weight24(-32.5) != 0u || msb::weight24((double)NAN) != 0u || msb::weight24(-(double)INFINITY) != 0u) {
    printf("FAIL fixed points\n");
    return 1;
  }
  printf("ok %zu\n", x.size());
  return 0;
}
