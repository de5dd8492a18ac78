// The re-draw of a determinized fork (monsoon_env_load_determinized_dev, include/monsoon.h): which card of the hidden
// side's hand and deck ends at which place.  The k movable hand entries and the d deck entries, in record order, form
// A[0 .. L), L = k + d; a partial Fisher-Yates over the first k places -- for i < k: r = hash32(seed, i, 0xD7),
// j = i + ((r * (L - i)) >> 32), swap A[i], A[j] -- makes the hand a uniformly chosen k-subset of the hidden cards in
// uniform order, and leaves the rest of the deck a rearrangement of what is left.  hash32 is monsoon_amd/fitness.py's over
// three words: integer arithmetic only, so the device, host C++ and numpy (monsoon_amd/vec_env.py determinize_order) agree
// in every bit.
// det_swaps gives the k swap partners (the same for a whole wavefront), det_source the entry of A that ends at one place:
// a lane needs no other lane's result, so the kernel (env_determinize.hip) moves every entry with one load and one store.
// One text for the kernel and for the host check (tests/determinize_check.cpp).  No device intrinsics.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MSB_DET_HD __host__ __device__
#else
#define MSB_DET_HD
#endif

namespace msb {

constexpr int DET_HAND_MAX = 5, DET_DECK_MAX = 12;   // HAND_CAP, DECK_CAP of the standard record (state.h)
constexpr uint32_t DET_TAG = 0xD7u;

MSB_DET_HD inline uint32_t det_hash32(const uint32_t a, const uint32_t b, const uint32_t c) {
  const uint32_t v[3] = {a, b, c};
  uint32_t h = 0x9E3779B9u;
  for (int i = 0; i < 3; i++) {
    h ^= v[i] + 0x7F4A7C15u + (h << 6) + (h >> 2);
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
  }
  return h;
}

// j[i] for i < k: the place whose entry swap i exchanges with place i's; i <= j[i] < k + d.  0 <= k <= DET_HAND_MAX.
MSB_DET_HD inline void det_swaps(const uint32_t seed, const int k, const int d, int j[DET_HAND_MAX]) {
  const int L = k + d;
  for (int i = 0; i < DET_HAND_MAX; i++)   // (a constant bound: the device keeps j in registers)
    j[i] = i < k ? i + (int)(((uint64_t)det_hash32(seed, (uint32_t)i, DET_TAG) * (uint32_t)(L - i)) >> 32) : i;
}

// The index in A of the entry that place l holds after the k swaps: the swaps undone from the last to the first.
MSB_DET_HD inline int det_source(const int j[DET_HAND_MAX], const int k, const int l) {
  int s = l;
  for (int i = DET_HAND_MAX - 1; i >= 0; i--)
    if (i < k) s = s == i ? j[i] : (s == j[i] ? i : s);
  return s;
}

}  // namespace msb
