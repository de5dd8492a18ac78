// coop_draw.h -- the weighted draw of a decision's REPLACE candidates (actions 148..151: Player.cycle = discard + draw(1),
// rules.h) resolved once by the whole wavefront, for the hot kernel's decision loop only (kernels.h play_game), on the
// standard record.  rules.h draw() keeps the serial definition; everything else uses only that.
//
// After discard() every REPLACE candidate of a decision draws from the same weights: reweight() made every deck card one
// step older, and the replaced card sits behind them with age 0 -- unless it is single-use and left the game, which gives
// one second form without that entry.  discard() takes no random number, so all of them compare against the same u: the
// first random_sample at the parent's cursor.  The drawn index therefore depends on the parent record alone (column 0),
// and a lane per deck entry finds it with two division sequences where a candidate lane runs n + 2 (idx + 1) of them:
//   * lanes 0 .. n hold the entries of the form with the returned card, lanes 16 .. 16 + n - 1 those of the form without;
//   * sum: 0.0 + w0 + w1 + ... left to right, the entries read lane by lane (v_readlane) in index order; an entry that is
//     not there adds +0.0, which leaves a positive sum as it is, bit for bit; the returned card's weight is added last;
//   * p = w / sum on all lanes at once; the cumulative sums travel the same way (acc0 = p0, then acc + p in index order),
//     each lane keeping the one of its own index; the last one is the final value of the chain;
//   * q = acc / last on all lanes at once; the drawn index is the first lane with !(q <= u).
// Every f64 operation has the operands, the order and the single rounding of draw() (no reciprocal, no reassociation; the
// library is built with -ffp-contract=off).  Whenever the serial path would not reach a plain successful draw -- a card at
// AGE_MAX (reweight faults), a full deck (deck_push_handle faults), nothing to draw from, no index found, a stream window
// that ends before the sample does -- the answer is "nothing resolved" (0) and the serial code runs and raises what it raises.
#pragma once

namespace msbk {
using namespace msb;

__device__ MSB_INL double lane_f64(const double v, const int l) {   // v of lane l (a constant) as a wave-uniform value
  const unsigned long long x = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), l);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// e: the current record (column 0, the same for every lane).  ra, rb: the two stream words a random_sample at its cursor
// reads; u_ok: both lie inside the record's stream window.  Returns the word rules.h cycle() reads (state.h DRAW_HINT_LDS):
// drawn index + 1 in byte 0 (the replaced card returns to the deck) and byte 1 (it does not), 0 = not resolved.  Call with
// the whole wave.
template <class E>
__device__ MSB_INL uint32_t coop_draw(const E& e, const int lane, const uint32_t ra, const uint32_t rb, const bool u_ok) {
  static_assert(DECK_CAP < 16, "one 16-lane row per form");
  const int lo = e.local();
  const int n = e.pl_deck_n(lo);
  const int i = lane & 15;
  const bool second = lane >= 16;
  const int age = i < DECK_CAP ? e.m.ld8(e.pl(lo, P_AGE + i)) : 0;
  // reweight() tests whole age words: the stale bytes behind the list in the last word it touches count as well
  const bool too_old = lane < ((n + 3) & ~3) && lane < DECK_CAP && age >= AGE_MAX;
  if (!u_ok || n > DECK_CAP || __ballot(too_old)) return 0u;
  const int cnt = second ? n : n + 1;
  const bool act = lane < 32 && i < cnt;
  const double w1 = e.m.wtab(0);   // "choice.weight = 1": what the returned card weighs
  const double w = i < n ? e.m.wtab(age + 1) : 0.0;
  double sum = 0.0;
  _Pragma("unroll") for (int t = 0; t < DECK_CAP; t++) sum = sum + lane_f64(w, t);
  const double den = second ? sum : sum + w1;
  const double p = (act ? (i < n ? w : w1) : 0.0) / (act ? den : 1.0);
  double acc_a = 0.0, acc_b = 0.0, mine = 0.0;
  _Pragma("unroll") for (int t = 0; t <= DECK_CAP; t++) {
    const double pa = lane_f64(p, t), pb = lane_f64(p, 16 + t);
    acc_a = t == 0 ? pa : acc_a + pa;
    acc_b = t == 0 ? pb : acc_b + pb;
    if (lane == t) mine = acc_a;
    if (lane == 16 + t) mine = acc_b;
  }
  const double last = second ? acc_b : acc_a;
  const double q = mine / (act ? last : 1.0);
  const double u = ((double)(ra >> 5) * 67108864.0 + (double)(rb >> 6)) / 9007199254740992.0;   // rng_random_sample
  const unsigned long long stop = __ballot(act && !(q <= u));
  const uint32_t sa = (uint32_t)stop & 0xffffu, sb = (uint32_t)(stop >> 16) & 0xffffu;
  const uint32_t ha = (sa && n < DECK_CAP) ? (uint32_t)__builtin_ctz(sa) + 1u : 0u;
  const uint32_t hb = sb ? (uint32_t)__builtin_ctz(sb) + 1u : 0u;
  return ha | (hb << 8);
}

}  // namespace msbk
