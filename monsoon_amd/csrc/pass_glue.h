// pass_glue.h -- what a pass of the hot kernel's decision loop (kernels.h play_game) does around the rules core to hand
// the pass's actions to its candidate lanes.
//
// The legal set is wave-uniform (three mask words in scalar registers).  One uniform loop takes the lowest set bit of
// `rem` n_act times and hands action l to candidate l; the caller's `put` deposits it in lane l (a compare-select against
// the lane id).  Afterwards `rem` has lost exactly this pass's actions, so lane l of the pass that starts at `base` holds
// the (base + l)-th legal action in ascending order.  It replaces a per-lane walk of up to U - 1 steps on the vector unit
// plus a U-step loop of three-way branches on the scalar unit that dropped the pass's bits, both paid on every pass
// however few candidates it held (profiles/pass_overhead_ab.txt).  Plain C++ of the mask words: it
// also compiles on the host, where tests/test_pass_overhead_cpu.py checks it against a plain nth-set-bit walk under the
// address and UB sanitizers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MSB_PASS_FN __device__ inline __attribute__((always_inline))
#else
#define MSB_PASS_FN inline
#endif

namespace msbk {

// rem: the legal actions no pass has taken yet (bit a of word a / 64).  Calls put(l, action) for l = 0 .. n_act-1 in
// ascending action order and clears those bits; stops early if the set runs out.
template <class Put>
MSB_PASS_FN void pass_actions(uint64_t rem[3], const int n_act, Put put) {
  int l = 0;
  for (int w = 0; w < 3; w++) {
    uint64_t m = rem[w];
    while (m != 0 && l < n_act) {
      put(l, w * 64 + __builtin_ctzll(m));
      m &= m - 1;
      l++;
    }
    rem[w] = m;
  }
}

}  // namespace msbk
