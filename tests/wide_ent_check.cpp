// Host check of the header word and the entity image (monsoon_amd/csrc/rules.h hdr_word / hw_*, ei_load / ei_*: move_enter,
// call_run_ability, h_runab, call_pop_trigger, h_move, call_entity_damage, call_destroy, call_unit_play, the tail of step_impl;
// state.h MSB_WIDE_ENT) against the -DMSB_WIDE_ENT=0 text of the same header.  tests/test_wide_ent_cpu.py compiles this file
// twice per record build (no flag, -DMSB_EXT=1, -DMSB_EXT=2) over FlatMem with the address and UB sanitizers -- once with
// -DWE_SIDE=0 -Dmsb=msb_bytes -DMSB_WIDE_ENT=0 (the per-field text; the namespace renamed, so the two texts of the core are two
// sets of symbols) and once with -DWE_SIDE=1 (the switch at its default, and main) -- links the two objects into a stand-alone
// program and runs it, never loaded into Python.  (The extended and large records build the per-field text on both sides: there
// the program holds a text against itself and pins that the switch changes nothing.)  On the standard record side 1 is built
// and run a second time with -DMSB_WIDE_ENT_HDR=1: the header word, which is not in the product (state.h), stays a text that
// compiles and computes the same.
//
// Every generated record is copied, one text runs on each copy, and the record bytes, the return value and the fault code must
// be identical, also where the call faults.  Nothing is skipped.  The inputs are whole step() calls on described records
// (scenario.inc scn_build), so that the handlers run inside run():
//   move     a unit on every tile of rows 1-4 x both owners x both sides to play x movement 0..3 x fixedly forward or not: the
//            side to play's own unit is PLAYED from its hand onto the tile (Unit.play: the ability call, the move of `movement`
//            steps), the other side's unit stands there and MOVES when the turn is passed to its owner (action 155: the flip,
//            PH_TURN_START, one step) -- x what stands ahead: nothing, a friend in the same column, a friend beside, an enemy
//            weaker, equal and stronger, an enemy structure, an enemy beside (the sidestep of a play), and nothing with both
//            bases at 1 and at the mover's strength (a base hit with the base surviving is the first case's);
//   turn     a unit on every tile of row 0 whose owner is passed the turn: the base hit at a turn's start, the base surviving,
//            falling, and left at exactly 0;
//   status   frozen, poisoned, vitalized, confused and disabled at 0, 1 and 2 on a mover at an edge and at an inner tile x
//            nothing, a weaker enemy, a stronger enemy and a friend ahead x a plain mover and one with a BEFORE_ATTACKING
//            ability x both sides to play, in PH_TURN_START (action 155) and in PH_PLAY (the side to play plays a unit into
//            ue21, which survives and commands the mover);
//   trigger  movers with BEFORE_MOVING, BEFORE_ATTACKING, AFTER_ATTACKING, ON_DEATH and AFTER_SURVIVING, played and moved,
//            against nothing, a weaker, an equal and a stronger enemy; plain movers, weaker, equal and stronger, against
//            targets with each of the five -- each with and without ST_DISABLED (but for the played mover, which carries no
//            statuses), both sides to play;
//   depth    call_move inside run() with H_DEPTH at MAX_DEPTH - 2, MAX_DEPTH - 1 and MAX_DEPTH (begin_step zeroes the byte, so
//            this one call is made behind it by both sides' export), plain movers and movers with an ability; and step() on
//            records that already carry a fault;
//   games    whole games of random legal actions from init_game on random decks: step() of the two texts on two copies, record
//            for record; fights, base hits, destroys with and without an ON_DEATH trigger and AFTER_SURVIVING triggers counted.
// Prints one "ok ..." line: per part the number of compared cases and their outcomes (clean / the fault code), and how often
// each thing the inputs are built for happened.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "rules.h"

#if !defined(MSB_COUNT_FRAMES)
#error "compile with -DMSB_COUNT_FRAMES: the games part reads the core's own counts of moves, fights and base hits"
#endif
#ifndef WE_SIDE
#error "compile with -DWE_SIDE=0 (the per-field text, -Dmsb=msb_bytes -DMSB_WIDE_ENT=0) and with -DWE_SIDE=1"
#endif

using namespace msb;
typedef Engine<FlatMem> Eng;

#define WE_CAT2(a, b) a##b
#define WE_CAT(a, b) WE_CAT2(a, b)
#define WE_FN(name) WE_CAT(WE_CAT(we, WE_SIDE), name)

#if WE_SIDE == 0
static_assert(MSB_WIDE_ENT == 0 && !MSB_WE_ANY, "side 0 is the per-field text");
#else
#if defined(MSB_EXT) && MSB_EXT
static_assert(MSB_WIDE_ENT == 1 && !MSB_WE_ANY, "the records with worlds keep the per-field text");
#else
static_assert(MSB_WIDE_ENT == 1 && MSB_WE_IMG, "side 1 is the text of the entity image (and, with -DMSB_WIDE_ENT_HDR=1, of the header word)");
#endif
#endif

static Eng over(uint8_t* st) {
  Eng e;
  e.m.p = st;
  return e;
}
extern "C" int WE_FN(_state_bytes)() { return STATE_BYTES; }
extern "C" int WE_FN(_step)(uint8_t* st, int action) {
  Eng e = over(st);
  return e.step(action);
}
// Unit.move of the unit on `tile`, inside run(), with the recursion guard's byte at `depth`
extern "C" int WE_FN(_move_at_depth)(uint8_t* st, int tile, int depth) {
  Eng e = over(st);
  Eng::Wk k{0, 0, 0, 0};
  e.begin_step();
  e.m.st8(H_DEPTH, depth);
  const int u = e.board_at(tile);
  e.set_path(u, false);
  e.call_move(k, u);
  e.run(k);
  return e.fault();
}

#if WE_SIDE == 1
extern "C" int we0_state_bytes();
extern "C" int we0_step(uint8_t* st, int action);
extern "C" int we0_move_at_depth(uint8_t* st, int tile, int depth);

static uint64_t rnd_x = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {   // xorshift64
  rnd_x ^= rnd_x << 13, rnd_x ^= rnd_x >> 7, rnd_x ^= rnd_x << 17;
  return (uint32_t)(rnd_x >> 32);
}

struct Rec {
  alignas(16) uint8_t st[STATE_BYTES];
};
static uint32_t g_mt[MT_N];
static uint32_t g_out[2][MT_N];   // the fixed stream: both copies of a record point at it

static void fail(const char* what, long long a, long long b, long long c, long long d) {
  printf("FAIL %s: %lld %lld %lld %lld\n", what, a, b, c, d);
  exit(1);
}

struct Tally {
  long long n, clean, by_code[32];
  void add(int fault) {
    n++;
    if (fault == 0) clean++;
    else by_code[fault & 31]++;
  }
  void print(const char* name) const {
    printf(" %s %lld %s_clean %lld", name, n, name, clean);
    for (int c = 0; c < 32; c++)
      if (by_code[c]) printf(" %s_fault%d %lld", name, c, by_code[c]);
  }
};
static Tally t_move, t_turn, t_status, t_trigger, t_depth, t_faulted, t_step;
// what happened, counted on the whole-word side's copy
static long long n_moved[4], n_blocked, n_fight, n_target_dead, n_mover_dead, n_both_dead, n_struct_hit, n_sidestep, n_base_survives, n_base_falls,
    n_base_zero, n_thaw, n_poison_dmg, n_vital_gain, n_confused_step, n_play_phase_move, n_mover_ran[8][2], n_target_ran[8][2], n_depth_guard,
    n_depth_clean, n_games, n_g_moves, n_g_fights, n_g_base_hits, n_g_destroy_plain, n_g_destroy_on_death, n_g_after_surviving;

static void compare(const char* what, const Rec& a, const Rec& b, int ra, int rb, long long i, long long j) {
  if (ra != rb) fail(what, i, j, ra, rb);
  if (memcmp(a.st, b.st, STATE_BYTES) != 0) {
    int at = 0;
    while (a.st[at] == b.st[at]) at++;
    printf("FAIL %s: case %lld %lld: byte %d is %d (fields) and %d (words)\n", what, i, j, at, a.st[at], b.st[at]);
    exit(1);
  }
}

// ---- described records ---------------------------------------------------------------------------------------------------
static std::vector<int> g_plain;          // units without an ability
static int g_plain_mov[4], g_trig_card[8];   // a plain unit per movement, a unit per trigger

static void find_cards() {
  for (int m = 0; m < 4; m++) g_plain_mov[m] = -1;
  for (int t = 0; t < 8; t++) g_trig_card[t] = -1;
  for (int i = 0; i < NUM_CARDS; i++) {
    const CardInfo& c = g_cards[i];
    if (c.kind != KIND_UNIT) continue;
    if (!c.has_ability) {
      g_plain.push_back(i);
      if (c.movement < 4 && g_plain_mov[c.movement] < 0) g_plain_mov[c.movement] = i;
    } else if (c.trigger >= 0 && c.trigger < 8 && g_trig_card[c.trigger] < 0 && c.movement >= 1) {
      g_trig_card[c.trigger] = i;
    }
  }
  for (int m = 0; m < 4; m++)
    if (g_plain_mov[m] < 0) fail("no plain unit of movement", m, 0, 0, 0);
  const int need[5] = {TR_BEFORE_MOVING, TR_BEFORE_ATTACKING, TR_AFTER_ATTACKING, TR_ON_DEATH, TR_AFTER_SURVIVING};
  for (int t = 0; t < 5; t++)
    if (g_trig_card[need[t]] < 0) fail("no unit with trigger", need[t], 0, 0, 0);
  if (g_plain.size() < 12) fail("too few plain units", (long long)g_plain.size(), 0, 0, 0);
}

struct Unit {
  int card, owner, str, mov, ff, st[5];
};
struct Desc {
  int toplay, phase, base[2];
  int hand_card, hand_ff;   // hand[0] of the side to play (-1: a filler)
  bool on[20];
  Unit u[20];
  void clear(int toplay_) {
    toplay = toplay_, phase = PH_PLAY, base[0] = base[1] = 10, hand_card = -1, hand_ff = 0;
    for (int t = 0; t < 20; t++) on[t] = false;
  }
  void put(int tile, int card, int owner, int str, int mov = 1, int ff = 0) {
    on[tile] = true;
    u[tile] = Unit{card, owner, str, mov, ff, {0, 0, 0, 0, 0}};
  }
};
static void push_card(std::vector<int32_t>& S, int card, int ff, int oid) {
  const int v[8] = {card, g_cards[card].cost, 0, ff, g_cards[card].kind == KIND_SPELL ? -1 : g_cards[card].strength, 0, 1 + oid, oid};
  S.insert(S.end(), v, v + 8);
}
static void build(Rec& r, const Desc& d) {
  std::vector<int32_t> S;
  const int hdr[5] = {d.toplay, d.toplay, d.phase, 0, 0};
  S.insert(S.end(), hdr, hdr + 5);
  for (int o = 0; o < 2; o++) {
    const int pl[7] = {d.base[o], 30, 5, o == d.toplay ? 1 : 3, 1, 1, 0};
    S.insert(S.end(), pl, pl + 7);
    int oid = 0, fi = 0;
    auto filler = [&]() {
      while (g_plain[fi] == d.hand_card) fi++;
      return g_plain[fi++];
    };
    S.push_back(4);
    for (int i = 0; i < 4; i++) {
      if (i == 0 && o == d.toplay && d.hand_card >= 0) push_card(S, d.hand_card, d.hand_ff, oid++);
      else push_card(S, filler(), 0, oid++);
    }
    S.push_back(6);
    for (int i = 0; i < 6; i++) push_card(S, filler(), 0, oid++);
  }
  for (int t = 0; t < 20; t++) {
    S.push_back(d.on[t] ? 1 : 0);
    if (!d.on[t]) continue;
    const Unit& u = d.u[t];
    const int v[17] = {u.card, u.owner, u.str, u.mov, u.ff, u.st[0], u.st[1], u.st[2], u.st[3], u.st[4], -1, 0, (int)(rnd() & 0xff), 0, 0, 0, 0};
    S.insert(S.end(), v, v + 17);
  }
  memset(r.st, 0, STATE_BYTES);
  Eng e = over(r.st);
  e.rng_attach(g_out[0], g_out[1], rnd() % 600);
  e.scn_build(S.data(), 7u);
  if (e.fault()) fail("scn_build faults", e.fault(), 0, 0, 0);
}
static int place_action(int tile) { return (4 - tile / 4) * 4 + (tile & 3); }   // hand[0] onto a tile of rows 1-4

// the ability log of the whole-word side: how often `card` ran
static int32_t g_trace[2 * 256];
static int ran(int card) {
  int n = 0;
  for (int i = 0; i < msb_trace_n; i++) n += g_trace[2 * i] == card;
  return n;
}
// both texts on copies of r; returns the whole-word side's record in `out`
static int both_step(const char* what, Tally& t, const Rec& r, int action, Rec& out, long long i, long long j) {
  Rec a = r;
  out = r;
  const int ra = we0_step(a.st, action);
  msb_trace_log = g_trace, msb_trace_n = 0, msb_trace_cap = 256;
  const int rb = we1_step(out.st, action);
  msb_trace_log = nullptr;
  compare(what, a, out, ra, rb, i, j);
  t.add(out.st[H_FAULT]);
  return rb;
}
static int str_of(const Rec& r, int slot) { return over(const_cast<uint8_t*>(r.st)).e_str(slot); }
static int pos_of(const Rec& r, int slot) { return r.st[Eng::ent(slot) + EO_POS]; }
// the slot a play created: the one that held no card before
static int new_slot(const Rec& before, const Rec& after) {
  for (int s = 0; s < NUM_ENT; s++)
    if (before.st[Eng::ent(s)] == CARD_NONE && after.st[Eng::ent(s)] != CARD_NONE) return s;
  return -1;
}

// One mover case.  `tile`, `ahead` in the coordinates the mover moves in: the board as it stands for a play, the flipped board
// for a unit that moves when the turn is passed (described through the flip: tile t of the flipped board is tile 19 - t now).
struct Seen {
  int mover, target, moved_rows, moved_cols, mover_str0, target_str0;
};
static Seen mover_case(const char* what, Tally& t, Desc d, bool play, int tile, int target_tile, long long i, long long j, Rec* keep = nullptr) {
  Rec r, out;
  if (!play) {   // describe through the flip
    Desc f = d;
    for (int q = 0; q < 20; q++) f.on[q] = d.on[19 - q], f.u[q] = d.u[19 - q];
    d = f;
  }
  build(r, d);
  const Eng e0 = over(r.st);
  Seen s{-1, -1, 0, 0, 0, 0};
  if (target_tile >= 0) s.target = e0.board_at(play ? target_tile : 19 - target_tile);
  if (!play) s.mover = e0.board_at(19 - tile);
  both_step(what, t, r, play ? place_action(tile) : 155, out, i, j);
  if (play) s.mover = new_slot(r, out);
  if (s.mover >= 0 && !out.st[H_FAULT]) {
    s.moved_rows = abs(pos_of(out, s.mover) / 4 - tile / 4);
    s.moved_cols = abs((pos_of(out, s.mover) & 3) - (tile & 3));
  }
  s.mover_str0 = play ? g_cards[d.hand_card].strength : (s.mover >= 0 ? str_of(r, s.mover) : 0);
  s.target_str0 = s.target >= 0 && s.target != SLOT_NONE ? str_of(r, s.target) : 0;
  if (keep) *keep = out;
  return s;
}

enum { A_NONE = 0, A_FRIEND, A_FRIEND_BESIDE, A_WEAKER, A_EQUAL, A_STRONGER, A_STRUCTURE, A_ENEMY_BESIDE, A_BASE_1, A_BASE_EQ, A_COUNT };

static void check_moves() {
  const int structure = C_B001;
  long long c = 0;
  for (int tile = 4; tile < 20; tile++)
    for (int owner = 0; owner < 2; owner++)
      for (int toplay = 0; toplay < 2; toplay++)
        for (int mov = 0; mov < 4; mov++)
          for (int ff = 0; ff < 2; ff++)
            for (int ahead = 0; ahead < A_COUNT; ahead++) {
              const bool play = owner == toplay;
              const int card = g_plain_mov[mov], str = g_cards[card].strength, x = tile & 3;
              const int at = tile - 4, beside = x < 3 ? tile + 1 : tile - 1;
              Desc d;
              d.clear(toplay);
              if (play) d.hand_card = card, d.hand_ff = ff;
              else d.put(tile, card, owner, str, mov, ff);
              int target = -1;
              switch (ahead) {
                case A_FRIEND: d.put(at, g_plain_mov[1], owner, 4), target = at; break;
                case A_FRIEND_BESIDE: d.put(beside, g_plain_mov[1], owner, 4); break;
                case A_WEAKER: d.put(at, g_plain_mov[1], owner ^ 1, str > 1 ? str - 1 : 1), target = at; break;
                case A_EQUAL: d.put(at, g_plain_mov[1], owner ^ 1, str), target = at; break;
                case A_STRONGER: d.put(at, g_plain_mov[1], owner ^ 1, str + 2), target = at; break;
                case A_STRUCTURE: d.put(at, structure, owner ^ 1, str + 2), target = at; break;
                case A_ENEMY_BESIDE: d.put(beside, g_plain_mov[1], owner ^ 1, 1), target = beside; break;
                case A_BASE_1: d.base[0] = d.base[1] = 1; break;
                case A_BASE_EQ: d.base[0] = d.base[1] = str; break;
                default: break;
              }
              Rec out;
              const Seen s = mover_case("move", t_move, d, play, tile, target, c++, ahead, &out);
              if (out.st[H_FAULT]) continue;
              const Eng e1 = over(out.st);
              const int b0 = e1.pl_base(0), b1 = e1.pl_base(1);
              if (b0 < d.base[0] || b1 < d.base[1]) {
                const int b = b0 < d.base[0] ? b0 : b1;
                (b > 0 ? n_base_survives : (b == 0 ? n_base_zero : n_base_falls))++;
              } else if (s.mover >= 0) {
                if (ahead == A_NONE && s.moved_cols == 0) n_moved[s.moved_rows < 3 ? s.moved_rows : 3]++;
                if (ahead == A_FRIEND && s.moved_rows == 0 && s.moved_cols == 0) n_blocked++;
                if (ahead == A_ENEMY_BESIDE && s.moved_cols) n_sidestep++;
              }
              if (s.target >= 0 && (ahead == A_WEAKER || ahead == A_EQUAL || ahead == A_STRONGER || ahead == A_STRUCTURE) && str_of(out, s.target) < s.target_str0) {
                const bool td = str_of(out, s.target) <= 0, md = s.mover >= 0 && str_of(out, s.mover) <= 0;
                n_fight++;
                n_struct_hit += ahead == A_STRUCTURE;
                n_target_dead += td && !md, n_mover_dead += md && !td, n_both_dead += td && md;
              }
            }
}

static void check_turn_base() {
  long long c = 0;
  for (int tile = 0; tile < 4; tile++)
    for (int toplay = 0; toplay < 2; toplay++)
      for (int base = 0; base < 3; base++) {
        Desc d;
        d.clear(toplay);
        const int str = 3;
        d.put(tile, g_plain_mov[1], toplay ^ 1, str);
        d.base[0] = d.base[1] = base == 0 ? 10 : (base == 1 ? 1 : str);
        Rec out;
        mover_case("turn", t_turn, d, false, tile, -1, c++, base, &out);
        const Eng e1 = over(out.st);
        const int b = e1.pl_base(toplay);   // the mover's enemy
        if (b < d.base[toplay]) (b > 0 ? n_base_survives : (b == 0 ? n_base_zero : n_base_falls))++;
      }
}

static void check_status() {
  const int ue21 = C_UE21;
  long long c = 0;
  for (int status = 0; status < 5; status++)
    for (int count = 0; count < 3; count++)
      for (int phase = 0; phase < 2; phase++)          // 0: PH_TURN_START through action 155; 1: PH_PLAY through ue21's command
        for (int where = 0; where < 2; where++)        // an edge column, an inner column
          for (int ahead = 0; ahead < 4; ahead++)      // nothing, a weaker enemy, a stronger enemy, a friend
            for (int kind = 0; kind < 2; kind++)       // a plain mover, one with a BEFORE_ATTACKING ability
              for (int toplay = 0; toplay < 2; toplay++) {
                const int card = kind ? g_trig_card[TR_BEFORE_ATTACKING] : g_plain_mov[1], str = 4;
                const int mover_owner = toplay ^ 1;
                Desc d;
                d.clear(toplay);
                Rec r, out;
                int mover = -1, start = -1;
                if (phase == 0) {
                  // flipped coordinates: the mover on row 2, what is ahead on row 1
                  const int tile = 2 * 4 + (where ? 1 : 0), at = tile - 4;
                  Desc f;
                  f.clear(toplay);
                  f.put(tile, card, mover_owner, str);
                  f.u[tile].st[status] = count;
                  if (ahead == 1) f.put(at, g_plain_mov[1], mover_owner ^ 1, 2);
                  if (ahead == 2) f.put(at, g_plain_mov[1], mover_owner ^ 1, 7);
                  if (ahead == 3) f.put(at, g_plain_mov[1], mover_owner, 2);
                  for (int q = 0; q < 20; q++) d.on[q] = f.on[19 - q], d.u[q] = f.u[19 - q];
                  build(r, d);
                  mover = over(r.st).board_at(19 - tile), start = tile;
                  both_step("status", t_status, r, 155, out, c++, status * 10 + count);
                } else {
                  // the side to play puts a weak unit under the other side's ue21 (2, 1), which survives and commands its units:
                  // the mover on row 1 moves towards the side to play's base, row 2 is ahead of it
                  const int tile = 1 * 4 + (where ? 1 : 0), at = tile + 4;
                  d.hand_card = g_plain_mov[1];
                  d.put(1 * 4 + 2, ue21, mover_owner, 8);
                  d.put(tile, card, mover_owner, str);
                  d.u[tile].st[status] = count;
                  if (ahead == 1) d.put(at, g_plain_mov[1], mover_owner ^ 1, 2);
                  if (ahead == 2) d.put(at, g_plain_mov[1], mover_owner ^ 1, 7);
                  if (ahead == 3) d.put(at, g_plain_mov[1], mover_owner, 2);
                  build(r, d);
                  mover = over(r.st).board_at(tile), start = tile;
                  both_step("status", t_status, r, place_action(2 * 4 + 2), out, c++, status * 10 + count);
                }
                if (out.st[H_FAULT]) continue;
                const int st0 = count, st1 = out.st[Eng::ent(mover) + EO_ST + status];
                const bool moved = pos_of(out, mover) != start;
                if (phase == 1 && (moved || ran(ue21))) n_play_phase_move += ran(ue21) > 0;
                if (status == ST_FROZEN && st1 < st0) n_thaw++;
                if (status == ST_POISONED && phase == 0 && count > 0 && str_of(out, mover) < str && ahead == 0) n_poison_dmg++;
                if (status == ST_VITALIZED && phase == 0 && count > 0 && str_of(out, mover) > str && ahead == 0) n_vital_gain++;
                if (status == ST_CONFUSED && count > 0 && st1 < st0 && (pos_of(out, mover) & 3) != (start & 3)) n_confused_step++;
              }
}

static void check_triggers() {
  const int trig[5] = {TR_BEFORE_MOVING, TR_BEFORE_ATTACKING, TR_AFTER_ATTACKING, TR_ON_DEATH, TR_AFTER_SURVIVING};
  long long c = 0;
  for (int ti = 0; ti < 5; ti++)
    for (int disabled = 0; disabled < 2; disabled++)
      for (int rel = 0; rel < 4; rel++)        // mover role: nothing ahead, a weaker, an equal, a stronger enemy; target role: (unused), the mover weaker, equal, stronger
        for (int play = 0; play < 2; play++)
          for (int toplay = 0; toplay < 2; toplay++)
            for (int role = 0; role < 2; role++) {   // 0: the mover carries the trigger; 1: the unit ahead does
              if (role == 0 && play && disabled) continue;   // a played unit carries no statuses: that record would be the enabled one again
              const int card = g_trig_card[trig[ti]], owner = play ? toplay : toplay ^ 1;
              const int tile = 2 * 4 + 1, at = tile - 4;
              Desc d;
              d.clear(toplay);
              const int mover_card = role == 0 ? card : g_plain_mov[1];
              const int mstr = g_cards[mover_card].strength;
              if (play) d.hand_card = mover_card;
              else d.put(tile, mover_card, owner, mstr);
              if (role == 0) {
                if (disabled) d.u[tile].st[ST_DISABLED] = 1;
                if (rel) d.put(at, g_plain_mov[1], owner ^ 1, rel == 1 ? (mstr > 1 ? mstr - 1 : 1) : (rel == 2 ? mstr : mstr + 3));
              } else {
                const int tstr = rel <= 1 ? mstr + 3 : (rel == 2 ? mstr : (mstr > 1 ? mstr - 1 : 1));
                d.put(at, card, owner ^ 1, tstr);
                if (disabled) d.u[at].st[ST_DISABLED] = 1;
              }
              const Seen s = mover_case("trigger", t_trigger, d, play != 0, tile, (role || rel) ? at : -1, c++, ti * 10 + rel);
              (void)s;
              (role == 0 ? n_mover_ran : n_target_ran)[trig[ti]][disabled] += ran(card);
            }
}

static void check_depth_and_fault() {
  long long c = 0;
  const int cards[3] = {g_plain_mov[1], g_trig_card[TR_BEFORE_MOVING], g_trig_card[TR_BEFORE_ATTACKING]};
  for (int ci = 0; ci < 3; ci++)
    for (int depth = MAX_DEPTH - 2; depth <= MAX_DEPTH; depth++)
      for (int toplay = 0; toplay < 2; toplay++)
        for (int ahead = 0; ahead < 3; ahead++) {
          Desc d;
          d.clear(toplay);
          const int tile = 2 * 4 + 2, str = 4;
          d.put(tile, cards[ci], toplay, str);
          if (ahead) d.put(tile - 4, g_trig_card[TR_ON_DEATH], toplay ^ 1, ahead == 1 ? 1 : 9);
          Rec r;
          build(r, d);
          Rec a = r, b = r;
          const int ra = we0_move_at_depth(a.st, tile, depth), rb = we1_move_at_depth(b.st, tile, depth);
          compare("depth", a, b, ra, rb, c++, depth);
          t_depth.add(rb);
          n_depth_guard += rb == FAULT_DEPTH;
          n_depth_clean += rb == 0 && depth == MAX_DEPTH - 1;
        }
  // a record that already carries a fault: a play, a REPLACE, the turn passed on
  const int actions[3] = {place_action(2 * 4 + 1), 148, 155};
  for (int code = 1; code < 30; code += 7)
    for (int ai = 0; ai < 3; ai++)
      for (int toplay = 0; toplay < 2; toplay++) {
        Desc d;
        d.clear(toplay);
        d.hand_card = g_plain_mov[2];
        d.put(1 * 4 + 1, g_plain_mov[1], toplay ^ 1, 2);
        Rec r, out;
        build(r, d);
        r.st[H_FAULT] = (uint8_t)code;
        both_step("faulted", t_faulted, r, actions[ai], out, c++, code);
      }
}

// ---- whole games: step() of the two texts on two copies --------------------------------------------------------------------
static void check_games(int games, int max_steps) {
  memset(msb_frame_count, 0, sizeof msb_frame_count);   // this side's counts (rules.h MSB_COUNT_FRAMES): moves begun, fights, base hits
  for (int gi = 0; gi < games; gi++) {
    uint32_t mt[MT_N];
    static uint32_t out[2][MT_N];
    mt_seed(mt, 3000u + (uint32_t)gi);
    int cur = 0;
    for (int w = 0; w < 2; w++) {
      mt_twist(mt);
      for (int i = 0; i < MT_N; i++) out[w][i] = mt_temper(mt[i]);
    }
    uint32_t pos = 0;
    Rec a;
    memset(a.st, 0, STATE_BYTES);
    uint8_t deck[2][DECK_SIZE];
    for (int o = 0; o < 2; o++)
      for (int i = 0; i < DECK_SIZE; i++) {
        bool again = true;
        while (again) {
          deck[o][i] = (uint8_t)(rnd() % NUM_CARDS);
          again = false;
          for (int k = 0; k < i; k++) again = again || deck[o][k] == deck[o][i];
        }
      }
    {
      Eng e = over(a.st);
      e.rng_attach(out[0], out[1], 0);
      e.init_game(deck[0], deck[1], (int)(rnd() % 4), (int)(rnd() % 4), 3000u + (uint32_t)gi);
      if (e.fault()) continue;
      pos = e.rng_pos();
    }
    n_games++;
    for (int s = 0; s < max_steps; s++) {
      Eng e = over(a.st);
      e.rng_attach(out[cur], out[cur ^ 1], pos);
      uint64_t mask[3];
      e.legal_mask(mask);
      int legal[156], nl = 0;
      for (int act = 0; act < 156; act++)
        if ((mask[act >> 6] >> (act & 63)) & 1) legal[nl++] = act;
      if (nl == 0) break;
      // plays before anything else two times in three: a game of passes and REPLACEs moves little
      int action = legal[rnd() % nl];
      if (legal[0] < 148 && rnd() % 3) {
        int np = 0;
        while (np < nl && legal[np] < 148) np++;
        action = legal[rnd() % np];
      }
      const Rec before = a;
      Rec b;
      const int ra = both_step("step", t_step, before, action, b, gi, s * 1000 + action);
      a = b;
      // what the step did, off the records: units that moved, lost strength, died; bases that were hit; the abilities that ran
      const Eng eb = over(const_cast<uint8_t*>(before.st)), ea = over(a.st);
      if (!a.st[H_FAULT]) {
        for (int sl = 0; sl < NUM_ENT; sl++) {
          if (before.st[Eng::ent(sl)] == CARD_NONE) continue;
          const int kind = before.st[Eng::ent(sl) + EO_KIND];
          const bool on_board0 = eb.board_at(pos_of(before, sl) % 20) == sl;
          if (!on_board0) continue;
          const bool on_board1 = ea.board_at(pos_of(a, sl) % 20) == sl;
          if (!on_board1 && str_of(a, sl) <= 0) ((((kind >> 2) & 15) - 1 == TR_ON_DEATH && (kind & EK_UNIT)) ? n_g_destroy_on_death : n_g_destroy_plain)++;
          if ((kind & EK_UNIT) && ((kind >> 2) & 15) - 1 == TR_AFTER_SURVIVING && str_of(a, sl) < str_of(before, sl) && str_of(a, sl) > 0 &&
              ran(before.st[Eng::ent(sl)]))
            n_g_after_surviving++;
        }
      }
      if (a.st[H_FAULT] || (ra & 2)) break;
      pos = over(a.st).rng_pos();
      if (pos >= (uint32_t)MT_N) {
        pos -= MT_N;
        over(a.st).rng_block_advance();
        const int old = cur;
        cur ^= 1;
        mt_twist(mt);
        for (int i = 0; i < MT_N; i++) out[old][i] = mt_temper(mt[i]);
      }
    }
  }
}

static void games_counts() {
  n_g_moves = msb_frame_count[32 + Eng::MV_ENTRY] + msb_frame_count[32 + Eng::MV_START];
  n_g_fights = msb_frame_count[51];
  n_g_base_hits = msb_frame_count[50];
}

int main() {
  if (we0_state_bytes() != STATE_BYTES) fail("the two sides are different record builds", we0_state_bytes(), STATE_BYTES, 0, 0);
  mt_seed(g_mt, 20240612u);
  for (int w = 0; w < 2; w++) {
    mt_twist(g_mt);
    for (int i = 0; i < MT_N; i++) g_out[w][i] = mt_temper(g_mt[i]);
  }
  find_cards();
  check_moves();
  check_turn_base();
  check_status();
  check_triggers();
  check_depth_and_fault();
  check_games(NUM_ENT > 64 ? 120 : (NUM_ENT > 24 ? 200 : 600), 160);
  games_counts();
  printf("ok");
  t_move.print("move");
  t_turn.print("turn");
  t_status.print("status");
  t_trigger.print("trigger");
  t_depth.print("depth");
  t_faulted.print("faulted");
  t_step.print("step");
  for (int i = 0; i < 4; i++) printf(" moved%d %lld", i, n_moved[i]);
  printf(" blocked %lld fight %lld target_dead %lld mover_dead %lld both_dead %lld struct_hit %lld sidestep %lld base_survives %lld base_falls %lld base_zero %lld",
         n_blocked, n_fight, n_target_dead, n_mover_dead, n_both_dead, n_struct_hit, n_sidestep, n_base_survives, n_base_falls, n_base_zero);
  printf(" thaw %lld poison_dmg %lld vital_gain %lld confused_step %lld play_phase_move %lld", n_thaw, n_poison_dmg, n_vital_gain, n_confused_step, n_play_phase_move);
  const int trig[5] = {TR_BEFORE_MOVING, TR_BEFORE_ATTACKING, TR_AFTER_ATTACKING, TR_ON_DEATH, TR_AFTER_SURVIVING};
  for (int t = 0; t < 5; t++)
    printf(" mover_ran%d %lld mover_ran%d_disabled %lld target_ran%d %lld target_ran%d_disabled %lld", trig[t], n_mover_ran[trig[t]][0], trig[t],
           n_mover_ran[trig[t]][1], trig[t], n_target_ran[trig[t]][0], trig[t], n_target_ran[trig[t]][1]);
  printf(" depth_guard %lld depth_quiet %lld games %lld g_moves %lld g_fights %lld g_base_hits %lld g_destroy_plain %lld g_destroy_on_death %lld g_after_surviving %lld\n",
         n_depth_guard, n_depth_clean, n_games, n_g_moves, n_g_fights, n_g_base_hits, n_g_destroy_plain, n_g_destroy_on_death, n_g_after_surviving);
  return 0;
}
#endif
