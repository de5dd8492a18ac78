// Host check of pass_actions (monsoon_amd/csrc/pass_glue.h) against a plain nth-set-bit walk, built with the address and
// UB sanitizers by tests/test_pass_overhead_cpu.py.  For every mask and every U in {4, 8, 16, 32, 64} the passes of a
// decision are replayed as play_game runs them: lane l of the pass starting at `base` must receive the (base + l)-th legal
// action in ascending order, lanes at or beyond n_act keep NONE_A, and `rem` must have lost exactly the actions handed out.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pass_glue.h"

static const int NONE_A = 1 << 20, BITS = 156;
static long long n_masks = 0, n_passes = 0;

static int nth_set_bit_ref(const uint64_t m[3], int k) {   // the plain reference: count the set bits one by one
  for (int a = 0; a < BITS; a++)
    if ((m[a >> 6] >> (a & 63)) & 1)
      if (k-- == 0) return a;
  return -1;
}

static void fail(const char* what, const uint64_t m[3], int u, int base, int l) {
  printf("FAIL %s: mask %016llx %016llx %016llx U %d base %d lane %d\n", what, (unsigned long long)m[0], (unsigned long long)m[1],
         (unsigned long long)m[2], u, base, l);
  exit(1);
}

static void check(const uint64_t mask[3]) {
  static const int us[5] = {4, 8, 16, 32, 64};
  int legal[BITS], n_legal = 0;
  for (int k = 0; k < BITS; k++) {
    const int a = nth_set_bit_ref(mask, k);
    if (a < 0) break;
    legal[n_legal++] = a;
  }
  for (int ui = 0; ui < 5; ui++) {
    const int U = us[ui];
    uint64_t rem[3] = {mask[0], mask[1], mask[2]};
    for (int base = 0; base < n_legal; base += U) {
      const int n_act = n_legal - base < U ? n_legal - base : U;
      int* lanes = (int*)malloc(sizeof(int) * U);   // (heap: an index at or beyond U is the sanitizer's to catch)
      for (int l = 0; l < U; l++) lanes[l] = NONE_A;
      msbk::pass_actions(rem, n_act, [&](const int l, const int act) { lanes[l] = act; });
      for (int l = 0; l < U; l++)
        if (lanes[l] != (l < n_act ? legal[base + l] : NONE_A)) fail("action", mask, U, base, l);
      free(lanes);
      uint64_t want[3] = {mask[0], mask[1], mask[2]};
      for (int k = 0; k < base + n_act; k++) want[legal[k] >> 6] &= ~(1ull << (legal[k] & 63));
      if (memcmp(want, rem, sizeof(want)) != 0) fail("rem", mask, U, base, -1);
      n_passes++;
    }
    if (rem[0] | rem[1] | rem[2]) fail("left over", mask, U, n_legal, -1);
  }
  n_masks++;
}

static void set(uint64_t m[3], int a) { m[a >> 6] |= 1ull << (a & 63); }

int main() {
  {   // every mask with at most three bits set in the 156-bit window
    uint64_t z[3] = {0, 0, 0};
    check(z);
    for (int a = 0; a < BITS; a++) {
      uint64_t m1[3] = {0, 0, 0};
      set(m1, a);
      check(m1);
      for (int b = a + 1; b < BITS; b++) {
        uint64_t m2[3] = {m1[0], m1[1], m1[2]};
        set(m2, b);
        check(m2);
        for (int c = b + 1; c < BITS; c++) {
          uint64_t m3[3] = {m2[0], m2[1], m2[2]};
          set(m3, c);
          check(m3);
        }
      }
    }
  }
  {   // 10 000 seeded random masks of every density
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < 10000; i++) {
      uint64_t m[3] = {0, 0, 0};
      const int per_mille = 1 + (i * 37) % 1000;
      for (int a = 0; a < BITS; a++) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;   // xorshift64
        if ((int)(x % 1000) < per_mille) set(m, a);
      }
      check(m);
    }
  }
  {   // {1}, all 156 bits, only bit 155
    uint64_t one[3] = {1, 0, 0}, all[3] = {~0ull, ~0ull, (1ull << (BITS - 128)) - 1}, last[3] = {0, 0, 1ull << (155 - 128)};
    check(one);
    check(all);
    check(last);
  }
  printf("ok %lld masks %lld passes\n", n_masks, n_passes);
  return 0;
}
