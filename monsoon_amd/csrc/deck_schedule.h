// Per-game decks of a deck schedule (monsoon_draw_schedule; monsoon_amd/decks.py DeckEvolutionConfig(per_game=True)).
//
// Every game draws from a stream of its own, Python's random.Random(s32 | generation << 32 | game_seed << 64 | tag << 96):
// CPython seeds an int with init_by_array(key), key = the int's 32-bit words, lowest first (_randommodule.c: random_seed,
// init_by_array), here always the four words {s32, generation, game_seed, tag} because tag != 0.  This file restates
// what utils.py:26-242 (monsoon_amd/decks.py: get_deck_configuration, generate_random_deck) calls on that stream, as
// Lib/random.py has it:
//   random()        (a >> 5, b >> 6) -> (a * 2^26 + b) / 2^53                               two outputs
//   _randbelow(n)   k = n.bit_length(); r = u32 >> (32 - k) until r < n                     one output per try
//   sample(pop, k)  setsize = 21, + 4 ** ceil(log(3k, 4)) = 64 for k in 6..12
//                   n <= setsize: j = randbelow(n - i); take pool[j]; pool[j] = pool[n - i - 1]    (pool path)
//                   else:         j = randbelow(n) until j is new; take pop[j]                     (set path)
// One text for the kernels (k_draw_schedule, and k_env_reseed_schedule for the vector env's episodes: lane 0 of the game's
// wavefront walks, the stream's first 624 outputs lie in LDS) and for the host check (tests/deck_schedule_check.cpp).  Plain pointers, no device intrinsics.
//
// A game may read the first 624 outputs of its stream (one twist); the draws of a deck pair took at most 90 in the host
// check's 72 000 games.  Reading past the window sets DsStream::over and yields 0, every loop below ends on it, and the caller reports
// the game: its 24 bytes are not a draw.
#pragma once
#include "mt19937.h"

namespace msb {

constexpr uint32_t DS_INIT_SEED = 19650218u;   // init_by_array starts from init_genrand(19650218), the same for every key
constexpr int DS_POOL_MAX = 128;
enum : int { DS_STATIC = 0, DS_EXPLORE = 1, DS_BALANCE = 2 };   // DS_STATIC: the exploit phase, the vector env's schedule only (k_env_reseed_schedule)

// init_by_array(key[4]) over mt = init_genrand(19650218): 624 + 623 dependent steps.  The previous word stays in a
// register, so a step waits for arithmetic only, never for the store before it.
MSB_HD inline void ds_key_mix(uint32_t* mt, const uint32_t* key4) {
  const uint32_t k0 = key4[0], k1 = key4[1] + 1u, k2 = key4[2] + 2u, k3 = key4[3] + 3u;   // init_key[j] + j
  uint32_t prev = mt[0];
  // first loop, max(N, key_length) = 624 steps: i = 1..623 with j = (i - 1) & 3, then i wraps (mt[0] = mt[623]) to i = 1, j = 3
  for (int i = 1; i < MT_N; i++) {
    const int j = (i - 1) & 3;
    prev = (mt[i] ^ ((prev ^ (prev >> 30)) * 1664525u)) + (j == 0 ? k0 : j == 1 ? k1 : j == 2 ? k2 : k3);
    mt[i] = prev;
  }
  prev = (mt[1] ^ ((prev ^ (prev >> 30)) * 1664525u)) + k3;
  mt[1] = prev;
  // second loop, N - 1 = 623 steps: i = 2..623, wrap, i = 1
  for (int i = 2; i < MT_N; i++) {
    prev = (mt[i] ^ ((prev ^ (prev >> 30)) * 1566083941u)) - (uint32_t)i;
    mt[i] = prev;
  }
  prev = (mt[1] ^ ((prev ^ (prev >> 30)) * 1566083941u)) - 1u;
  mt[1] = prev;
  mt[0] = 0x80000000u;
}

// The stream: a read-only window of 624 TEMPERED outputs and a cursor.
struct DsStream {
  const uint32_t* w;
  int pos;
  int over;   // outputs asked for past the window
};

MSB_HD MSB_INL uint32_t ds_u32(DsStream& s) {
  if (s.pos >= MT_N) {
    s.over++;
    return 0u;
  }
  return s.w[s.pos++];
}

MSB_HD MSB_INL double ds_random(DsStream& s) {
  const uint32_t a = ds_u32(s) >> 5, b = ds_u32(s) >> 6;
  return ((double)a * 67108864.0 + (double)b) * (1.0 / 9007199254740992.0);
}

MSB_HD MSB_INL uint32_t ds_randbelow(DsStream& s, uint32_t n) {   // n >= 1
  const int shift = __builtin_clz(n);   // 32 - n.bit_length()
  uint32_t r;
  do r = ds_u32(s) >> shift;
  while (r >= n);   // (past the window r = 0 < n)
  return r;
}

// random.sample(pop[0..n), k) -> out[0..k); 0 <= k <= n <= 128.  The pool path works in pop itself, as the reference
// works in its copy: the caller hands a copy it no longer needs.
MSB_HD inline void ds_sample(DsStream& s, uint8_t* pop, int n, int k, uint8_t* out) {
  const int setsize = k > 5 ? 21 + 64 : 21;
  if (n <= setsize) {
    for (int i = 0; i < k; i++) {
      const uint32_t j = ds_randbelow(s, (uint32_t)(n - i));
      out[i] = pop[j];
      pop[j] = pop[n - i - 1];
    }
  } else {
    uint64_t sel0 = 0, sel1 = 0;
    for (int i = 0; i < k; i++) {
      uint32_t j;
      bool seen;
      do {
        j = ds_randbelow(s, (uint32_t)n);
        seen = ((j < 64 ? sel0 >> j : sel1 >> (j - 64)) & 1u) != 0;
      } while (seen && !s.over);
      if (j < 64) sel0 |= 1ull << j;
      else sel1 |= 1ull << (j - 64);
      out[i] = pop[j];
    }
  }
}

// One game's pair -> out24 (P1's deck, then P2's).  arch: [2][12], pool: [2][DS_POOL_MAX] with pool_n[side] cards; both
// are scratch copies (see ds_sample).
//   explore: per side, P1 first: sample(archetype, n_preserve) then sample(pool, 12 - n_preserve); n_preserve = 12 is
//            the archetype itself, no draws (generate_random_deck's preserve_ratio == 1.0)
//   balance: random() < ratio for P1, then for P2; then sample(pool, 12) per side whose test failed, P1 first
//   static:  both archetypes, no draw: the stream is not read, n_preserve and the pools are ignored
MSB_HD inline void ds_walk(DsStream& s, int phase, int n_preserve, double ratio, uint8_t* arch, uint8_t* pool, const int32_t* pool_n,
                           uint8_t* out24) {
  bool keep[2] = {n_preserve >= 12, n_preserve >= 12};
  if (phase == DS_STATIC) {
    keep[0] = keep[1] = true;
  } else if (phase == DS_BALANCE) {
    n_preserve = 0;
    for (int side = 0; side < 2; side++) keep[side] = ds_random(s) < ratio;
  }
  for (int side = 0; side < 2; side++) {
    uint8_t* o = out24 + side * 12;
    uint8_t* a = arch + side * 12;
    if (keep[side]) {
      for (int i = 0; i < 12; i++) o[i] = a[i];
      continue;
    }
    ds_sample(s, a, 12, n_preserve, o);
    ds_sample(s, pool + side * DS_POOL_MAX, pool_n[side], 12 - n_preserve, o + n_preserve);
  }
}

}  // namespace msb
