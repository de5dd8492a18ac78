// coop_features.h -- StateFeatures.get_feature_vector (observe.inc features()) computed by the whole wavefront, for the
// hot kernel's decision loop only (kernels.h play_game).  observe.inc keeps the serial definition that k_features, the API
// kernels, the host build and the oracle use; this form computes the same ten doubles bit for bit.
//
// With U candidate lanes a candidate has S = 64 / U sub-lanes: lane l serves candidate l % U as sub-lane l / U and reads
// that candidate's record through an accessor whose column is l % U (state.h SubColMem; Col0Mem for the "before" side).
// A wave64 instruction costs the same issue slots for U live lanes as for 64, so what moves sideways is free:
//   * board scan: the 20 tiles are dealt to the sub-lanes in runs of T tiles: a board row each where there are at least 5
//     sub-lanes (U = 8), half a row with at least 10 (U = 4), else ceil(20 / S); every sub-lane reads its tiles' entities at
//     once.  Integer partials (strength sums, unit-tile masks, structure counts) are sums over disjoint tiles and are reduced
//     with a butterfly over the candidate's sub-lanes: integer addition is order-free.
//   * threat / protection are f64 sums in ASCENDING TILE ORDER and stay exactly that.  The products are formed on the tile's
//     sub-lane; the accumulator TRAVELS: the sub-lane holding tiles 0 .. T-1 starts from +0.0 and adds its terms in order,
//     hands the pair of sums to the sub-lane holding the next run, and so on down to sub-lane 0.  A tile that contributes
//     nothing adds +0.0 instead of being skipped: x + (+0.0) == x bit for bit unless x is -0.0, and an accumulator that
//     starts at +0.0 never becomes -0.0 (round-to-nearest gives -0.0 only for (-0.0) + (-0.0)).
//   * divisions: the six independent quotients (mana / est, (P-O) / total, strength / cost of four hand cards) sit on six
//     sub-lanes and share ONE division sequence; they meet again through the candidate's feature slot in LDS.  Then
//     total_value (ordered, +0.0 for a skipped card as above), avg = total_value / 3.0 and nv = avg / 3.0: three division
//     sequences instead of nine.  playable / 3.0 for valid == 3 is one of four quotients the compiler rounds (0/3, 1/3,
//     2/3, 3/3: IEEE division of the same operands).
// Every f64 operation of features() is performed with the same operands and the same single rounding.
#pragma once

namespace msbk {
using namespace msb;

// f: this candidate's ten-feature slot in LDS: staging area for the quotients first, the ten results at the end (written by
// sub-lane 0 where `on`; the values never sit in registers together).  `on`: this lane's candidate takes part (false: the
// lane runs along on whatever its column holds and writes nothing).  Call with the whole wave (one barrier inside).
template <int U, class E>
__device__ MSB_INL void coop_features(const E& e, const int lane, const bool on, MSB_AS_LDS double* f) {
  MSB_SCOPE(PS_FEATURES);
  constexpr int S = 64 / U;             // sub-lanes per candidate
  // tiles per sub-lane: a whole board row where there are 5 sub-lanes to take one each, half a row with 10; else ceil(20 / S)
  constexpr int T = S >= 10 ? 2 : (S >= 5 ? 4 : (20 + S - 1) / S);
  constexpr int H = (20 + T - 1) / T;   // sub-lanes that hold tiles; sub-lane j holds run H-1-j, so that the sums end on sub-lane 0
  constexpr int NQ = 6, QR = (NQ + S - 1) / S;
  const int j = lane / U;
  const int lo = e.local();
  const int mana_i = e.pl_mana(lo);
  const double mana = mana_i != -1 ? (double)mana_i : 0.0;

  // ---- board scan ------------------------------------------------------------------------------------------------------
  int Pm = 0, Pa = 0;        // strengths of the mover's entities / of all entities
  uint32_t mm = 0, ma = 0;   // the same split; bits 0-19: tiles holding a unit, bits 20-: number of structures
  double term_p[T], term_t[T];
  const bool holds = on && j < H;
  const int t0 = holds ? T * (H - 1 - j) : 0;
  uint32_t slots = 0;        // T == 2, 4: the run's board bytes in one LDS read (OFF_BOARD and the run are aligned to it)
  if constexpr (T == 4) slots = e.m.ld32(OFF_BOARD + t0);
  if constexpr (T == 2) slots = (uint32_t)e.m.ld16(OFF_BOARD + t0);
  _Pragma("unroll") for (int i = 0; i < T; i++) {
    const int t = t0 + i;
    const int s = (T == 4 || T == 2) ? (int)((slots >> (8 * i)) & 0xff) : e.m.ld8(OFF_BOARD + (t < 20 ? t : 0));
    const bool occ = holds && t < 20 && s != SLOT_NONE;
    const msb_u32x4 g = e.m.ld128g(E::eg(occ ? s : 0));   // the whole entity in one LDS read (slot 0 where there is none)
    const int str = (int)(int16_t)(g[2] >> 16);
    const bool mine = (int)((g[0] >> 8) & EF_OWNER) == lo;
    const bool unit = ((g[3] >> 24) & EK_UNIT) != 0;
    // sums skip entries equal to -1 (the "empty" marker); a real strength of -1 is skipped too.  Skipped = a term of 0 / +0.0.
    const int sv = (occ && str != -1) ? str : 0;
    Pa += sv;
    Pm += mine ? sv : 0;
    const uint32_t mark = occ ? (unit ? 1u << t : 1u << 20) : 0u;
    ma += mark;
    mm += mine ? mark : 0u;
    const int row = (T == 4 || T == 2) ? t0 >> 2 : t >> 2;   // (a run of 2 or 4 lies in one row)
    const double term = (double)sv * E::fifth(mine ? 5 - row : row + 1);   // (5 - row) / 5.0 : (row + 1) / 5.0
    term_p[i] = mine ? term : 0.0;
    term_t[i] = (!mine && unit) ? term : 0.0;
  }
  _Pragma("unroll") for (int off = U; off < 64; off <<= 1) {
    Pm += __shfl_xor(Pm, off);
    Pa += __shfl_xor(Pa, off);
    mm += (uint32_t)__shfl_xor((int)mm, off);
    ma += (uint32_t)__shfl_xor((int)ma, off);
  }
  const int P = Pm, O = Pa - Pm;
  const uint32_t mw = mm, ow = ma - mm;
  double protection = 0.0, threat = 0.0;
  _Pragma("unroll") for (int h = 0; h < H; h++) {   // after hop h sub-lane H-1-h holds the sums over tiles 0 .. T*(h+1)-1
    if (h) {
      protection = __shfl_down(protection, U);
      threat = __shfl_down(threat, U);
    }
    _Pragma("unroll") for (int i = 0; i < T; i++) {
      protection = protection + term_p[i];
      threat = threat + term_t[i];
    }
  }
  const uint32_t mu = mw & 0xFFFFFu, ou = ow & 0xFFFFFu;
  const int nlu = __popc(mu), nru = __popc(ou), nls = (int)(mw >> 20), nrs = (int)(ow >> 20);
  const int min_l = nlu ? __builtin_ctz(mu) >> 2 : 4;
  const int max_r = nru ? (31 - __builtin_clz(ou)) >> 2 : 0;
  const int total = P + O;

  // ---- hand ------------------------------------------------------------------------------------------------------------
  const int hn = on ? e.pl_hand_n(lo) : 0;
  int playable = 0, valid = 0;
  uint32_t inst[4];
  _Pragma("unroll") for (int i = 0; i < 4; i++) {
    inst[i] = i < hn ? e.m.ld32(e.hand_ref(lo, i)) : 0u;   // {card, cost, flags, x}; cost 0 where there is no card
    const int cost = (int)((inst[i] >> 8) & 0xff);
    if (i < hn) valid++;
    if (cost > 0 && (double)cost <= mana) playable++;
  }

  // ---- the six independent quotients, one division sequence ------------------------------------------------------------
  double est = mana + 2.0;
  if (!(est > 3.0)) est = 3.0;     // max(3, m+2)
  if (!(est < 10.0)) est = 10.0;   // min(10, .)
  _Pragma("unroll") for (int r = 0; r < QR; r++) {
    const int q = r * S + j;
    double num = 0.0, den = 1.0;   // a quotient nobody asks for: +0.0
    if (q == 0) {
      num = mana;
      den = est;
    } else if (q == 1) {
      if (total != 0) {
        num = (double)(P - O);
        den = (double)total;
      }
    } else if (q < NQ) {
      const uint32_t w = q == 2 ? inst[0] : (q == 3 ? inst[1] : (q == 4 ? inst[2] : inst[3]));
      const int cost = (int)((w >> 8) & 0xff), fl = (int)((w >> 16) & 0xff);
      if (cost > 0) {
        num = (double)((fl & CF_SPELL) ? 0 : e.inst_strength((int)(w & 0xff), fl, (int)(w >> 24)));
        den = (double)cost;
      }
    }
    const double quot = num / den;
    if (on && q < NQ) f[q < 2 ? 2 * q : 1 + q] = quot;   // mana / est -> f[0], (P-O) / total -> f[2], the hand's -> f[3..6]
  }
  __syncthreads();

  // ---- the ten values (every lane alike; they count on sub-lane 0, where threat and protection are complete).  A staged
  // quotient is read before its slot gets its result. --------------------------------------------------------------------
  double f9;
  {
    double total_value = 0.0;
    total_value = total_value + f[3];
    total_value = total_value + f[4];
    total_value = total_value + f[5];
    total_value = total_value + f[6];
    // division by valid = 1, 2 or 4 is an exact scaling; only valid == 3 needs a real division
    const double rv = valid == 1 ? 1.0 : (valid == 2 ? 0.5 : 0.25);
    const double third = playable == 0 ? 0.0 / 3.0 : (playable == 1 ? 1.0 / 3.0 : (playable == 2 ? 2.0 / 3.0 : 3.0 / 3.0));
    const double playability = valid == 3 ? third : (double)playable * rv;
    const double tv3 = total_value / 3.0;
    const double avg = valid == 3 ? tv3 : total_value * rv;
    double nv = avg / 3.0;
    nv = nv < 0.0 ? 0.0 : (nv > 1.0 ? 1.0 : nv);
    f9 = valid == 0 ? 0.0 : (playability + nv) / 2.0;
  }
  const double r0 = 1.0 - f[0];
  const double q_adv = f[2];
  if (on && j == 0) {
    const int lh = e.pl_base(lo), rh = e.pl_base(lo ^ 1);
    const double player_health = lh != -1 ? (double)lh : 20.0;
    const double opponent_health = rh != -1 ? (double)rh : 20.0;
    f[0] = r0 < 0.0 ? 0.0 : (r0 > 1.0 ? 1.0 : r0);
    f[1] = player_health - opponent_health;
    f[2] = total == 0 ? 0.0 : q_adv;
    f[3] = (nlu == 0 && nru == 0) ? 0.0 : (double)(max_r - min_l) / 4.0;
    f[4] = (double)(P - O);
    f[5] = (double)(nlu - nru);
    f[6] = (double)(nls - nrs);
    f[7] = threat;
    f[8] = protection;
    f[9] = f9;
  }
}

// HeuristicAgent.score_action as observe.inc action_score_lds has it, with the "after" features read from LDS as well
// (wb[0..9] weights, wb[10..19] "before" features): the same operations in the same order.
__device__ MSB_INL double coop_score(const MSB_AS_LDS double* wb, const MSB_AS_LDS double* after) {
  double agent = 0.0, enemy = 0.0;
  for (int i = 0; i < 10; i++) {
    double d = after[i] - wb[10 + i];
    agent = __builtin_fma(wb[i], d, agent);
    enemy = __builtin_fma(wb[i], -d, enemy);
  }
  double eff = after[0] - wb[10];
  double pen = eff < -0.3 ? __builtin_fabs(eff) * 0.2 : 0.0;
  return enemy - agent - pen;
}

}  // namespace msbk
