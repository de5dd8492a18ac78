// env_after.h -- the afterstates of a vector-env slot (monsoon_env_afterstates_dev, include/monsoon.h): the hot kernel's
// look-ahead without its decision.  after_slot<U> composes the pieces play_game is made of (kernels.h PlayLds<U>,
// legal_set, pass_actions, MSB_EACH_GRANULE): load and stage the slot's record, legal set, draw hint, "before" features,
// then passes that clone the record, take their actions, step them and hand each successor out -- status, reward, winner,
// the ten features, the observation -- instead of scoring it.  There is no arg-max, no v_best, no commit and no refill,
// and nothing of the handle is written: the record and its meta row are only read, the stream is read through the two
// resident blocks.  What follows the staging is spelled as MSB_AFTER_STATE, which the replay of logged games expands
// per kept row as well (replay_log.h replay_game<U, true>).
// k_env_after (env_after.hip) gives every slot to one wavefront.
#pragma once
#include "env.h"

namespace msbk {

// How the observation of a successor is written (2 160 bytes each, the bulk of the output).  1: the whole wave writes one
// candidate's tensor at a time, lane l composing the words l, l + 64, ... from the candidate's column (SubColMem), so a
// store instruction covers 256 consecutive bytes.  0: every candidate lane runs Engine::observe on its own successor, eight
// lanes storing at a 2 160-byte stride (measured 6 - 7 % slower in this phase: DESIGN.md section 4).
#ifndef MSB_AFTER_OBS_COOP
#define MSB_AFTER_OBS_COOP 1
#endif

// Field f of the (card id, cost, strength, movement) row of a hand / deck card (observe.inc obs_card_row).
template <class E>
__device__ MSB_INL int32_t obs_row_field(const E& e, const int f, const int card, const int cost, const int fl, const int x) {
  if (f == 0) return e.card_int_id(card);
  if (f == 1) return cost;
  if (f == 2) return (card < NUM_CARDS && g_cards[card].kind == KIND_SPELL) ? -1 : e.inst_strength(card, fl, x);
  return e.card_is_unit(card) ? (card < NUM_CARDS ? g_cards[card].movement : 1) : -1;
}

// Word i of Engine::observe's tensor (observe.inc: plane-major, then y, then x), composed on its own.  ord[k] = the deck
// position of the k-th card in the observation's (cost, card id) order, stable.
template <class E>
__device__ MSB_INL int32_t obs_word(const E& e, const int i, const MSB_AS_LDS uint8_t* ord) {
  const int p = i / 20, t = i - p * 20;
  const int lo = e.local(), re = lo ^ 1;
  if (p < 6 || (p >= 16 && p < 22)) {   // the board planes of the local / remote side
    const int s = e.board_at(t);
    if (s == SLOT_NONE) return -1;
    const int base = p < 6 ? 0 : 16, q = p - base;
    if ((e.e_owner(s) == lo) != (base == 0)) return -1;
    if (e.e_is_unit(s)) {
      if (q == 0) return e.card_int_id(e.e_card(s));
      if (q == 1) return e.e_str(s);
      if (q == 2) return e.e_mov(s);
      if (q == 3)
        return (e.e_st(s, ST_VITALIZED) ? 1 : 0) | (e.e_st(s, ST_POISONED) ? 2 : 0) | (e.e_st(s, ST_CONFUSED) ? 4 : 0) |
               (e.e_st(s, ST_FROZEN) ? 8 : 0) | (e.e_st(s, ST_DISABLED) ? 16 : 0);
      return -1;
    }
    if (q == 4) return e.card_int_id(e.e_card(s));
    if (q == 5) return e.e_str(s);
    return -1;
  }
  if (p == 6) {   // hand (first four) + sentinel row
    if (t >= 16) return 32767;
    const int h = t >> 2;
    if (h >= e.pl_hand_n(lo)) return -1;
    return obs_row_field(e, t & 3, e.hand_card(lo, h), e.hand_cost(lo, h), e.hand_flags(lo, h), e.hand_x(lo, h));
  }
  if (p < 13) {   // deck, sorted, four cards per plane + sentinel row
    if (t >= 16) return 32768;
    const int k = (p - 7) * 4 + (t >> 2);
    if (k >= e.pl_deck_n(lo)) return -1;
    const int v = ord[k];
    return obs_row_field(e, t & 3, e.deck_card(lo, v), e.deck_cost(lo, v), e.deck_flags(lo, v), e.deck_x(lo, v));
  }
  if (p == 13) return e.pl_mana(lo);
  if (p == 14) return e.pl_base(lo);
  if (p == 15) return e.m.ld8(e.pl(lo, P_FACTION));
  if (p == 22) return e.pl_mana(re);
  if (p == 23) return e.pl_base(re);
  if (p == 24) return e.m.ld8(e.pl(re, P_FACTION));
  if (p == 25) return (lo == 0 ? 1 : -1) * 99999;
  // plane 26: ([None] * 4 + history)[-4:] + sentinel row
  if (t >= 16) return 32769;
  const int k = (t >> 2) - (4 - e.m.ld8(H_HIST_N));
  if (k < 0 || (t & 3) > 1) return -1;
  if ((t & 3) == 0) return e.m.ld8(H_HIST + 2 * k) ? -99999 : 99999;
  return e.card_int_id(e.m.ld8(H_HIST + 2 * k + 1));
}

// The order obs_word reads a record's deck in, by the whole wave: a lane per deck card finds its place in the stable
// (cost, card id) order of engine se_'s deck and writes ord_[place].  The first barrier lets the readers of the order
// before finish, the second publishes this one.  Spelled in place like MSB_EACH_GRANULE (after_slot per successor,
// replay_row per row: replay_log.h): as a function it moved after_slot's scalar registers about (scripts/isa_diff.sh).
#define MSB_OBS_DECK_ORDER(se_, lane_, ord_)                                                          \
  {                                                                                                   \
    const int lo = se_.local(), dn = se_.pl_deck_n(lo);                                               \
    __syncthreads();                                                                                  \
    for (int v = lane_; v < dn; v += 64) {                                                            \
      const int kc = se_.deck_cost(lo, v), kid = se_.deck_card(lo, v);                                \
      int r = 0;                                                                                      \
      for (int j = 0; j < dn; j++) {                                                                  \
        const int oc = se_.deck_cost(lo, j), oid = se_.deck_card(lo, j);                              \
        r += (oc < kc || (oc == kc && (oid < kid || (oid == kid && j < v)))) ? 1 : 0;                 \
      }                                                                                               \
      ord_[r] = (uint8_t)v;                                                                           \
    }                                                                                                 \
    __syncthreads();                                                                                  \
  }

// The look-ahead of the state column 0 holds, into entry row_ of o_ (a monsoon_env_after with K_ entries per row): game
// g_'s record with the stream window at rng_ attached, v_par_ its image in registers, ls_ its legal set (rem is used up).
// n_legal, the draw hint, the "before" features, then the passes; column 0 is a candidate's afterwards.  For the whole
// wave, where b, pe, ce and L are what after_slot calls so.  Spelled in place like MSB_EACH_GRANULE, for after_slot
// and replay_game (replay_log.h): as a function template it reordered k_env_after's code object (scripts/isa_diff.sh).
#if MSB_AFTER_OBS_COOP
#define MSB_AFTER_OBS_(o_, K_, row_, lane_)                                                                                                           \
      const unsigned long long part = __ballot(ok);   /* (candidates sit on lanes 0 .. U-1) */                                                        \
      MSB_AS_LDS uint8_t* ord = (MSB_AS_LDS uint8_t*)(uintptr_t)L::CF;   /* (the features have left CF, the stacks are empty) */                      \
      for (int c = 0; c < n_act; c++) {                                                                                                               \
        if (!((part >> c) & 1)) continue;   /* (uniform) */                                                                                           \
        typename L::SubEngine se;                                                                                                                     \
        se.m.set_col(c);                                                                                                                              \
        MSB_OBS_DECK_ORDER(se, lane_, ord)   /* (its first barrier: the order of the candidate before has been read) */                               \
        int32_t* out = o_.obs + (row_ * K_ + base + c) * MONSOON_OBS_INTS;                                                                            \
        for (int i = lane_; i < MONSOON_OBS_INTS; i += 64) out[i] = obs_word(se, i, ord);                                                             \
      }
#else
#define MSB_AFTER_OBS_(o_, K_, row_, lane_) if (ok) ce.observe(o_.obs + e * MONSOON_OBS_INTS);
#endif
#define MSB_AFTER_STATE(o_, K_, row_, g_, rng_, ls_, v_par_, lane_)                                                                                   \
  {                                                                                                                                                   \
  const int n_legal = ls_.n;                                                                                                                          \
  const int n_do = n_legal < K_ ? n_legal : K_;   /* the afterstates this call hands out */                                                           \
  if (lane_ == 0) o_.n_legal[row_] = n_legal;                                                                                                         \
  for (int k = n_do + lane_; k < K_; k += 64) (o_.action + row_ * K_)[k] = 255;                                                                       \
  L::draw_hint(pe, b, g_, rng_, ls_.mask[2], lane_);                                                                                                  \
  if (o_.before_features && !pe.observation_raises()) {   /* (uniform) */                                                                             \
    if constexpr (!L::COOP) {   /* (as play_game spells it) */                                                                                        \
      if (lane_ == 0) pe.features(L::wf() + 10);                                                                                                      \
    } else {                                                                                                                                          \
      int sl = lane_;   /* (opaque, as in play_game) */                                                                                               \
      asm volatile("" : "+v"(sl));                                                                                                                    \
      coop_features<U>(pe, sl, true, L::wf() + 10);                                                                                                   \
    }                                                                                                                                                 \
    __syncthreads();                                                                                                                                  \
    if (lane_ < 10) o_.before_features[row_ * 10 + lane_] = L::wf()[10 + lane_];                                                                      \
  }                                                                                                                                                   \
  __syncthreads();                                                                                                                                    \
                                                                                                                                                      \
  for (int base = 0; base < n_do; base += U) {                                                                                                        \
    const int n_act = n_do - base < U ? n_do - base : U;                                                                                              \
    {   /* clone: copy.deepcopy (stream window included) for the whole pass, lane l writes granule l of every column in use */                        \
      __syncthreads();                                                                                                                                \
      for (int col = 0; col < n_act; col++) MSB_EACH_GRANULE(L::GPL, lane_, *L::gran(col, gr_) = v_par_[j_])                                        \
      __syncthreads();                                                                                                                                \
    }                                                                                                                                                 \
    const bool active = lane_ < n_act;                                                                                                                \
    const size_t e = row_ * K_ + base + (active ? lane_ : 0);   /* this candidate's entry */                                                          \
    int a = 255;                                                                                                                                      \
    pass_actions(ls_.rem, n_act, [&](const int l, const int act) { a = lane_ == l ? act : a; });                                                      \
    int status = 0;                                                                                                                                   \
    if (active) {                                                                                                                                     \
      const int rd = ce.step(a);                                                                                                                      \
      const int f = ce.fault();                                                                                                                       \
      /* a step that raised leaves no reward and no winner: 0 and -2 (include/monsoon.h) */                                                           \
      int reward = 0, winner = -2;                                                                                                                    \
      if (!f) {                                                                                                                                       \
        reward = rd & 1;                                                                                                                              \
        if (ce.have_winner()) winner = ce.winner_of(ce.pl_base(0), ce.pl_base(1));                                                                    \
      }                                                                                                                                               \
      status = f ? f : (ce.observation_raises() ? FAULT_INT_CARD : 0);                                                                                \
      o_.action[e] = (uint8_t)a;                                                                                                                      \
      if (o_.status) o_.status[e] = (uint8_t)status;                                                                                                  \
      if (o_.reward) o_.reward[e] = (int8_t)reward;                                                                                                   \
      if (o_.winner) o_.winner[e] = (int8_t)winner;                                                                                                   \
    }                                                                                                                                                 \
    const bool ok = active && status == 0;   /* the successors that have features and an observation */                                               \
    if (o_.features) {   /* (uniform) */                                                                                                              \
      if constexpr (!L::COOP) {                                                                                                                       \
        double fa[10];                                                                                                                                \
        if (ok) L::cand_features(ce, fa, o_.features + e * 10);                                                                                       \
      } else {                                                                                                                                        \
        const unsigned long long part = __ballot(ok);   /* (candidates sit on lanes 0 .. U-1) */                                                      \
        if (part) {                                                                                                                                   \
          L::coop_cand_features(part, lane_, L::CF);   /* (the stacks are empty once the pass has stepped) */                                         \
          __syncthreads();                                                                                                                            \
          for (int i = lane_; i < U * 10; i += 64)                                                                                                    \
            if ((part >> (i / 10)) & 1) o_.features[(row_ * K_ + base) * 10 + i] = ((MSB_AS_LDS const double*)(uintptr_t)L::CF)[i];                   \
        }                                                                                                                                             \
      }                                                                                                                                               \
    }                                                                                                                                                 \
    if (o_.obs) {   /* (uniform) 2 160 bytes per successor: the bulk of what this call writes */                                                      \
      MSB_AFTER_OBS_(o_, K_, row_, lane_)                                                                                                             \
    }                                                                                                                                                 \
  }                                                                                                                                                   \
  }

// The afterstates of slot g by the calling wavefront; K = max_after.  Call with the whole wave.
template <int U>
__device__ MSB_INL void after_slot(const DevBuffers& b, const monsoon_env_after& o, const int K, const int g, const int lane) {
  typedef PlayLds<U, PLAY_LDS_COLUMNS_AFTER> L;
  const GameMeta meta = b.meta[g];
  uint8_t* const act_row = o.action + (size_t)g * K;
  if (meta.result != -2) {   // the episode ended before the agent could act: the next step reports it
    if (lane == 0) o.n_legal[g] = 0;
    for (int k = lane; k < K; k += 64) act_row[k] = 255;
    return;
  }
  const u32x4* grec = (const u32x4*)(b.state + (size_t)g * SW);
  u32x4 v_par[L::GPL];   // granules lane, lane + 64, ... of the slot's record
  _Pragma("unroll") for (int j_ = 0; j_ < L::GPL; j_++) v_par[j_] = u32x4{0u, 0u, 0u, 0u};
  MSB_EACH_GRANULE(L::GPL, lane, v_par[j_] = grec[gr_])
  typename L::ParEngine pe;
  typename L::CandEngine ce;
  // stage: the image of the record in column 0; with the stream window attached it is what the clones start from
  MSB_EACH_GRANULE(L::GPL, lane, *L::gran(0, gr_) = v_par[j_])
  __syncthreads();
  if (lane == 0) attach_rng(pe, b, g, meta.rng);
  __syncthreads();
  MSB_EACH_GRANULE(L::GPL, lane, v_par[j_] = *L::gran(0, gr_))

  LegalSet ls = legal_set(pe);
  MSB_AFTER_STATE(o, K, (size_t)g, g, meta.rng, ls, v_par, lane)
}

// k_env_after<U, W> at the build's default variant (env_after.hip).
struct EnvAfterOps : KernelOps {
  void (*launch)(int grid, int lds_bytes, hipStream_t stream, DevBuffers b, monsoon_env_after out, int n, int max_after);
};
const EnvAfterOps* monsoon_env_after_ops();

}  // namespace msbk
