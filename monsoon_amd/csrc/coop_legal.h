// coop_legal.h -- the legal set of a decision (rules.h legal_mask_v: Stormbound.legal_actions + Action.to_int) computed
// by the whole wavefront from tile and hand masks, for the record in candidate column 0 of the wavefront-per-game kernels
// (kernels.h legal_set), on the standard record.  rules.h legal_mask_v() keeps the serial definition and stays in use: the
// lane-per-game kernels, the host builds and the extended records compute it, and this form is tested against it.
//
// legal_mask_v() handles the hand cards one after the other on the scalar unit, all 64 lanes running the same chain: per
// card an LDS round trip for the entry and a scalar load of its card-table row, and for a targeted spell one LDS round
// trip per occupied tile, a point list packed six bits at a time and unpacked again into action bits through a three-way
// branch per bit.  The action bits of a card are a fixed function of a 20-bit tile mask, the card's slot in the hand,
// its kind and whether the mover can pay for it, so here
//   * lanes c < hand_n read their own hand entry and their card's table row (kind, target descriptor) at once and compare
//     cost and mana; three ballots give the affordable unit / structure cards, untargeted spells and targeted spells;
//   * lanes t < 20 read board byte t: a ballot gives the occupied tiles, from which the 16 PLACE offsets of a card follow
//     as in legal_mask_v, and the words are composed from the ballots by shifts;
//   * only where a targeted spell is affordable (uniform; USE is 8.7 % of all candidates, profiles/pass_stats.md) do the
//     tile lanes read their entity (one ds_read_b128 each, one round trip) and evaluate rules.h target_matches for each
//     such spell in turn (a uniform loop over the ballot's bits, the descriptor taken from the spell's lane): a ballot is
//     the `hit` tile mask, whose row-reversed copy shifted to 65 + 21 c is the spell's action bits.  No list is built.
// Action 155, the REPLACE bits and "nothing playable" follow legal_mask_v to the letter, including what it does with the
// fifth hand slot, whose USE bits run into 148..155 and past the end of the action space.
//
// The mask arithmetic is plain C++ of integers that also compiles on the host, where tests/coop_legal_check.cpp holds it
// against legal_mask() / get_targets() under the address and UB sanitizers (tests/test_coop_legal_cpu.py); the wave form
// itself is pinned by tests/test_coop_legal_gpu.py.  DESIGN.md section 4 has the measurements.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MSB_LEGAL_FN __device__ inline __attribute__((always_inline))
#else
#define MSB_LEGAL_FN inline
#endif

namespace msbk {

constexpr int LEGAL_ACTIONS = 156;   // actions 0 .. 155 (bit a of word a / 64); 155 = pass
constexpr int LEGAL_TILES = 20;      // tile y * 4 + x

// Rows 0..4 of a tile mask in reverse order: tile (x, y) -> bit (4 - y) * 4 + x, the order Action.to_int counts positions in.
MSB_LEGAL_FN uint32_t legal_rows_reversed(const uint32_t tiles) {
  return ((tiles >> 16) & 0xFu) | ((tiles >> 8) & 0xF0u) | (tiles & 0xF00u) | ((tiles << 8) & 0xF000u) | ((tiles << 16) & 0xF0000u);
}
// The 16 PLACE offsets (4 - y) * 4 + x of one card: the empty tiles of rows 4 .. max(front line, 1).  Row 0 is not
// enumerated by Action.to_int (games/stormbound.py:262-271).
MSB_LEGAL_FN uint32_t legal_place_offsets(const uint32_t empty, const int front) {
  const int first = front < 1 ? 1 : (front > 5 ? 5 : front);
  return legal_rows_reversed(empty & (0xFFFFFu << (4 * first)) & 0xFFFFFu) & 0xFFFFu;
}
// ... and whether row 0 is open to it as well: those tiles all count as action 155.
MSB_LEGAL_FN bool legal_place_row0(const uint32_t empty, const int front) { return front <= 0 && (empty & 0xFu) != 0; }

// m |= v << pos over the three words, v < 2^20; what lands at or beyond bit 192 falls away.
MSB_LEGAL_FN void legal_or_at(uint64_t m[3], const uint64_t v, const int pos) {
  const int w = pos >> 6, s = pos & 63;
  const uint64_t lo = v << s, hi = s ? v >> (64 - s) : 0ull;
  m[0] |= w == 0 ? lo : 0ull;
  m[1] |= w == 1 ? lo : (w == 0 ? hi : 0ull);
  m[2] |= w == 2 ? lo : (w == 1 ? hi : 0ull);
}
// The USE bits of the targeted spell in hand slot c for the `hit` tiles: 65 + 21 c + (4 - y) * 4 + x.
MSB_LEGAL_FN void legal_use_bits(uint64_t m[3], const uint32_t hit, const int c) { legal_or_at(m, legal_rows_reversed(hit), 65 + 21 * c); }

// The part of the three words that needs no entity: PLACE for the cards of `units` (bit c: hand slot c holds a unit or a
// structure the mover can pay for), USE without a target for those of `plain` (an untargeted spell), 155 where row 0 is
// open.  Returns whether anything became playable (legal_mask_v's any_play so far).
MSB_LEGAL_FN bool legal_compose(uint64_t m[3], const uint32_t place, const bool row0, const uint32_t units, const uint32_t plain) {
  m[0] = m[1] = m[2] = 0ull;
  for (int c = 0; c < 4; c++) m[0] |= ((units >> c) & 1u) ? (uint64_t)place << (16 * c) : 0ull;
  m[1] |= ((units >> 4) & 1u) ? (uint64_t)place : 0ull;   // 16 * 4 - 64: the fifth slot's offsets share bits with the spells' first
  bool any_play = units != 0u && (place != 0u || row0);
  if (units != 0u && row0) m[2] |= 1ull << (155 - 128);
  for (int c = 0; c < 5; c++)
    if ((plain >> c) & 1u) legal_or_at(m, 1ull, 64 + 21 * c);
  return any_play || plain != 0u;
}
// One targeted spell: its tiles, and 155 for a base among its targets (an invalid point to Action.to_int).
MSB_LEGAL_FN bool legal_add_targets(uint64_t m[3], const uint32_t hit, const int bases, const int c) {
  legal_use_bits(m, hit, c);
  if (bases) m[2] |= 1ull << (155 - 128);
  return hit != 0u || bases != 0;
}
// The REPLACE bits 148 + c of a mover who may still replace, "nothing playable -> pass", and the end of the action space.
MSB_LEGAL_FN void legal_finish(uint64_t m[3], const bool any_play, const bool replacable, const int hand_n) {
  if (replacable && hand_n > 0) m[2] |= ((1ull << (hand_n < 8 ? hand_n : 8)) - 1ull) << (148 - 128);
  if (!any_play) m[2] |= 1ull << (155 - 128);
  m[2] &= (1ull << (LEGAL_ACTIONS - 128)) - 1ull;
}

#if defined(__HIPCC__)
using namespace msb;

// The three words of legal_mask_v() for the current record -- candidate column 0, which E addresses without state (state.h
// Col0Mem) -- in a register vector, the same in every lane.  Call with the whole wave.  Out of line, as legal_mask_v is
// (rules.h MSB_A_LEGAL): inlined, the phase's temporaries cost the decision loops around it registers.
template <class E>
__device__ MSB_NOINLINE msb_u64x4 coop_legal_v() {
  const E e;
  int lane = (int)__builtin_amdgcn_workitem_id_x();   // (opaque: nothing derived from it is computed ahead of the phase and kept)
  asm volatile("" : "+v"(lane));
  uint64_t out[3];
  static_assert(HAND_CAP <= 5 && LEGAL_TILES + HAND_CAP <= 64, "a lane per hand slot and per tile; legal_compose counts five slots");
  const int lo = e.local(), pov = e.cp();
  const int hn = __builtin_amdgcn_readfirstlane(e.pl_hand_n(lo));
  const int front = __builtin_amdgcn_readfirstlane(e.pl_front(lo));
  const bool replacable = (__builtin_amdgcn_readfirstlane(e.m.ld8(e.pl(lo, P_FLAGS))) & 1) != 0;
  const int mana = e.pl_mana(lo);
  // tiles: lane t holds board byte t
  const int slot = e.board_at(lane < LEGAL_TILES ? lane : 0);
  const bool occupied = lane < LEGAL_TILES && slot != SLOT_NONE;
  // hand: lane c holds entry c {card, cost, flags, x} and its card's row of the table
  const bool held = lane < hn && lane < HAND_CAP;
  const uint32_t inst = e.m.ld32(e.hand_ref(lo, lane < HAND_CAP ? lane : 0));
  const int card = (int)(inst & 0xff);
  const CardInfo& ci = g_cards[card < NUM_CARDS ? card : 0];
  const bool spell = ci.kind == KIND_SPELL, targeted = ci.tgt.has != 0;
  const Tgt tgt = mk_tgt(ci.tgt);
  const bool pays = held && (int)((inst >> 8) & 0xff) <= mana;
  const uint32_t units = (uint32_t)__ballot(pays && !spell);
  const uint32_t plain = (uint32_t)__ballot(pays && spell && !targeted);
  uint32_t aimed = (uint32_t)__ballot(pays && spell && targeted);
  const uint32_t empty = ~(uint32_t)__ballot(occupied) & 0xFFFFFu;
  bool any_play = legal_compose(out, legal_place_offsets(empty, front), legal_place_row0(empty, front), units, plain);
  if (aimed) {   // (uniform)
    const msb_u32x4 g = e.m.ld128g(E::eg(occupied && slot < NUM_ENT ? slot : 0));   // the whole entity in one LDS read
    do {
      const int c = __builtin_ctz(aimed);
      aimed &= aimed - 1;
      const Tgt t = ((Tgt)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(tgt >> 32), c) << 32) |
                    (Tgt)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)tgt, c);
      const uint32_t hit = (uint32_t)__ballot(occupied && e.target_matches(g, pov, t));
      any_play |= legal_add_targets(out, hit, E::target_bases(t), c);
    } while (aimed);
  }
  legal_finish(out, any_play, replacable, hn);
  return msb_u64x4{out[0], out[1], out[2], 0ull};
}
#endif

}  // namespace msbk
