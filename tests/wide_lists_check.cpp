// Host check of the whole-word forms of a step's list and path bookkeeping (monsoon_amd/csrc/rules.h discard_wide,
// draw_take_wide, the hand entry read once per play, set_path_impl; state.h MSB_WIDE_LISTS, MSB_WIDE_PATH) against the
// -DMSB_WIDE_LISTS=0 -DMSB_WIDE_PATH=0 text of the same header.  tests/test_wide_lists_cpu.py compiles this file twice per
// record build (no flag, -DMSB_EXT=1, -DMSB_EXT=2) over FlatMem with the address and UB sanitizers -- once with
// -DWL_SIDE=0 -Dmsb=msb_loops -DMSB_WIDE_LISTS=0 -DMSB_WIDE_PATH=0 (the loops; the namespace renamed, so the two texts of the
// core are two sets of symbols) and once with -DWL_SIDE=1 (the switches at their defaults, and main) -- links the two
// objects into a stand-alone program and runs it, never loaded into Python.
//
// Every generated record is copied, one text runs on each copy, and the record bytes, the return value and the fault
// code must be identical, also where the call faults.  Nothing is skipped.  Over which inputs:
//   discard   (standard record) hand sizes 0..5 x every index x deck sizes 0..12 (a push at 11 and at 12, FAULT_CAP_DECK)
//             x single use or not x both players; an earlier equal card at every earlier index, plain, positioned
//             (CF_STR, CF_ALIAS) on either or both entries, and two equal spells; ages 0, 254 and 255 at every byte of
//             the three age words over random clean ages (the fault in word 0, 1 and 2 behind clean lower words), an age
//             at AGE_MAX behind the end of a shorter list; random records with random pad bytes and a fault from before;
//   draw      (standard record) draw(o, amount, hint): the hinted form at every index of every deck size 0..12 x hand
//             sizes 0..5 (FAULT_CAP_HAND, the empty deck), the unhinted search over random ages on a fixed stream, amount
//             1..4; an earlier equal card in the deck at every earlier index, plain, positioned, two equal spells;
//   set_path  (every record build) every tile x both owners x both sides to play x mov 0..5 (PATH_CAP and its fault) x
//             fixedly forward or not x confused 0..2 (x = 0, 3 and the inner columns; a fixed stream) x on_play or not, on
//             boards whose other tiles are empty, friend or enemy at random (an enemy left, right, both, neither; a
//             friend, an enemy, nothing or a base ahead), and one board on which the sidestep alternates, whose path is
//             asserted: the third step is decided by a hit in the destinations;
//   step      (every record build) whole games of random legal actions from init_game on random decks: step() of the two
//             texts on two copies, record for record -- the play's single read of its hand entry, REPLACE, the draws of
//             a turn's end.
// Prints one "ok ..." line: per function the number of compared cases and their outcomes (clean / the fault code).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rules.h"

#ifndef WL_SIDE
#error "compile with -DWL_SIDE=0 (the loops, -Dmsb=msb_loops -DMSB_WIDE_LISTS=0 -DMSB_WIDE_PATH=0) and with -DWL_SIDE=1"
#endif

using namespace msb;
typedef Engine<FlatMem> Eng;

#define WL_CAT2(a, b) a##b
#define WL_CAT(a, b) WL_CAT2(a, b)
#define WL_FN(name) WL_CAT(WL_CAT(wl, WL_SIDE), name)

#if WL_SIDE == 0
static_assert(MSB_WIDE_LISTS == 0 && MSB_WIDE_PATH == 0, "side 0 is the text of the loops");
#else
static_assert(MSB_WIDE_LISTS == 1 && MSB_WIDE_PATH == 1, "side 1 is the text of the whole words");
#endif

// ---- what each side exports: one call of one function on a record (the stream window is already attached) ----------
static Eng over(uint8_t* st) {
  Eng e;
  e.m.p = st;
  return e;
}
extern "C" int WL_FN(_state_bytes)() { return STATE_BYTES; }
extern "C" int WL_FN(_discard)(uint8_t* st, int o, int idx) {
  Eng e = over(st);
  e.discard(o, idx);
  return e.fault();
}
extern "C" int WL_FN(_draw)(uint8_t* st, int o, int amount, int hint) {
  Eng e = over(st);
  e.draw(o, amount, hint);
  return e.fault();
}
extern "C" int WL_FN(_set_path)(uint8_t* st, int ent, int on_play) {
  Eng e = over(st);
  e.set_path(ent, on_play != 0);
  return e.fault();
}
extern "C" int WL_FN(_step)(uint8_t* st, int action) {
  Eng e = over(st);
  return e.step(action);
}

#if WL_SIDE == 1
extern "C" int wl0_state_bytes();
extern "C" int wl0_discard(uint8_t* st, int o, int idx);
extern "C" int wl0_draw(uint8_t* st, int o, int amount, int hint);
extern "C" int wl0_set_path(uint8_t* st, int ent, int on_play);
extern "C" int wl0_step(uint8_t* st, int action);

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

// outcome counts of one function: clean, and per fault code
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
static Tally t_discard, t_draw, t_path, t_step;
static long long n_hand_remove[5], n_deck_remove[12], n_push_at[13], n_dup_hand, n_dup_deck, n_sidestep_seen, n_games, n_plays, n_replaces;

static void compare(const char* what, const Rec& a, const Rec& b, int ra, int rb, long long i, long long j) {
  if (ra != rb) fail(what, i, j, ra, rb);
  if (memcmp(a.st, b.st, STATE_BYTES) != 0) {
    int at = 0;
    while (a.st[at] == b.st[at]) at++;
    printf("FAIL %s: case %lld %lld: byte %d is %d (loops) and %d (words)\n", what, i, j, at, a.st[at], b.st[at]);
    exit(1);
  }
}

static int card_of_kind(int kind, int skip) {
  for (int i = 0; i < NUM_CARDS; i++)
    if (g_cards[i].kind == kind && skip-- == 0) return i;
  fail("no such card", kind, skip, 0, 0);
  return 0;
}

static uint32_t entry(int card, int flags, int x) { return (uint32_t)card | ((uint32_t)g_cards[card].cost << 8) | ((uint32_t)flags << 16) | ((uint32_t)x << 24); }

#if !(defined(MSB_EXT) && MSB_EXT)
// ---- discard and draw: the standard record -----------------------------------------------------------------------
// a record whose players hold hands and decks of distinct cards with random clean ages; everything else random bytes
// that no list function reads, the stream attached at a random cursor
static void list_record(Rec& r, int hn0, int dn0, int hn1, int dn1, bool noise) {
  for (int i = 0; i < STATE_BYTES; i++) r.st[i] = noise ? (uint8_t)rnd() : 0;
  Eng e = over(r.st);
  e.rng_attach(g_out[0], g_out[1], rnd() % 1200);
  e.m.st8(H_FAULT, 0);
  e.m.st8(H_TOPLAY, (int)(rnd() & 1));
  for (int o = 0; o < 2; o++) {
    const int hn = o ? hn1 : hn0, dn = o ? dn1 : dn0;
    e.m.st8(e.pl(o, P_HAND_N), hn);
    e.m.st8(e.pl(o, P_DECK_N), dn);
    const int first = (int)(rnd() % 40);
    for (int i = 0; i < HAND_CAP; i++) {
      const int c = (first + i) % NUM_CARDS;
      if (i < hn || !noise) e.m.st32(e.pl(o, P_HAND + 4 * i), i < hn ? entry(c, (rnd() & 1) ? CF_XBASE : 0, (int)(rnd() % 12)) : 0u);
    }
    for (int i = 0; i < DECK_CAP; i++) {
      const int c = (first + HAND_CAP + i) % NUM_CARDS;
      if (i < dn || !noise) e.m.st32(e.pl(o, P_DECK + 4 * i), i < dn ? entry(c, (rnd() & 1) ? CF_XBASE : 0, (int)(rnd() % 12)) : 0u);
      e.m.st8(e.pl(o, P_AGE + i), i < dn ? (int)(rnd() % 40) : 0);
    }
  }
}
static void set_flags(Rec& r, int ref, int flags) { r.st[ref + 2] = (uint8_t)flags; }
static void set_card(Rec& r, int ref, int card) {
  r.st[ref] = (uint8_t)card;
  r.st[ref + 1] = (uint8_t)g_cards[card].cost;
}

static void run_discard(const Rec& r, int o, int idx, long long i, long long j) {
  Rec a = r, b = r;
  const Eng e0 = over(const_cast<uint8_t*>(r.st));
  const int hn = e0.pl_hand_n(o), dn = e0.pl_deck_n(o);
  const int ra = wl0_discard(a.st, o, idx), rb = wl1_discard(b.st, o, idx);
  compare("discard", a, b, ra, rb, i, j);
  t_discard.add(rb);
  if (rb == 0 && hn > 0) {
    const Eng e1 = over(b.st);
    if (e1.pl_hand_n(o) != hn - 1) fail("discard hand_n", i, j, hn, e1.pl_hand_n(o));
    if (e1.pl_deck_n(o) == dn + 1) n_push_at[dn]++;
  }
  if (rb == FAULT_CAP_DECK && dn == DECK_CAP && !r.st[H_FAULT]) n_push_at[DECK_CAP]++;
}

static void check_discard() {
  const int unit_a = card_of_kind(KIND_UNIT, 0), spell = card_of_kind(KIND_SPELL, 0), structure = card_of_kind(KIND_STRUCT, 0);
  Rec r;
  long long c = 0;
  // every hand size, index, deck size, single use or not, both players
  for (int hn = 0; hn <= HAND_CAP; hn++)
    for (int idx = 0; idx < (hn ? hn : 1); idx++)
      for (int dn = 0; dn <= DECK_CAP; dn++)
        for (int single = 0; single < 2; single++)
          for (int o = 0; o < 2; o++) {
            list_record(r, hn, dn, (int)(rnd() % 6), (int)(rnd() % 13), (c & 1) != 0);
            const Eng e = over(r.st);
            if (single) set_flags(r, e.hand_ref(o, idx), CF_SINGLE_USE | CF_XBASE);
            run_discard(r, o, idx, c++, 0);
            if (hn) n_hand_remove[idx]++;
          }
  // an earlier equal card: plain, positioned on either or both entries, structures and units; two equal spells
  const int pos_flags[3] = {0, CF_STR, CF_ALIAS};
  for (int idx = 1; idx < HAND_CAP; idx++)
    for (int at = 0; at < idx; at++)
      for (int fa = 0; fa < 3; fa++)
        for (int fb = 0; fb < 3; fb++)
          for (int kind = 0; kind < 3; kind++) {
            list_record(r, HAND_CAP - (int)(rnd() % (HAND_CAP - idx)), (int)(rnd() % 12), 4, 8, false);
            const Eng e = over(r.st);
            const int o = (int)(rnd() & 1), card = kind == 0 ? unit_a : (kind == 1 ? structure : spell);
            set_card(r, e.hand_ref(o, at), card), set_flags(r, e.hand_ref(o, at), pos_flags[fa]);
            set_card(r, e.hand_ref(o, idx), card), set_flags(r, e.hand_ref(o, idx), pos_flags[fb]);
            if (at > 0 && (rnd() & 1)) set_card(r, e.hand_ref(o, at - 1), card);   // two earlier ones: the first decides
            run_discard(r, o, idx, c++, 1);
            if (kind != 2 && !fa && !fb) n_dup_hand++;   // (a plain earlier equal unit or structure is the one that leaves the hand)
          }
  // ages: 0, 254 and 255 at every byte of the three words, over clean random ages; an age at AGE_MAX behind the list's end
  for (int byte = 0; byte < DECK_CAP; byte++)
    for (int v = 0; v < 3; v++)
      for (int dn = 1; dn <= DECK_CAP; dn++) {
        list_record(r, 4, dn, 4, 8, false);
        const Eng e = over(r.st);
        const int o = (int)(rnd() & 1);
        for (int i = 0; i < dn; i++) r.st[e.pl(o, P_AGE + i)] = (uint8_t)(rnd() % 255);
        r.st[e.pl(o, P_AGE + byte)] = (uint8_t)(v == 0 ? 0 : (v == 1 ? 254 : 255));
        run_discard(r, o, (int)(rnd() % 4), c++, 2);
      }
  // random records: noise in the pad bytes and behind the lists, now and then a fault from before the call
  for (int t = 0; t < 20000; t++) {
    const int hn = 1 + (int)(rnd() % HAND_CAP);
    list_record(r, hn, (int)(rnd() % 13), hn, (int)(rnd() % 13), true);
    const Eng e = over(r.st);
    const int o = (int)(rnd() & 1), idx = (int)(rnd() % hn);
    if (rnd() % 4 == 0) set_card(r, e.hand_ref(o, (int)(rnd() % hn)), r.st[e.hand_ref(o, idx)]);
    if (rnd() % 8 == 0) set_flags(r, e.hand_ref(o, (int)(rnd() % hn)), (int)(rnd() & 0x3f));
    if (rnd() % 16 == 0) r.st[e.pl(o, P_AGE + (int)(rnd() % 12))] = 255;
    if (rnd() % 32 == 0) r.st[H_FAULT] = FAULT_PY_EXCEPTION;
    run_discard(r, o, idx, c++, 3);
  }
}

static void run_draw(const Rec& r, int o, int amount, int hint, long long i, long long j) {
  Rec a = r, b = r;
  const Eng e0 = over(const_cast<uint8_t*>(r.st));
  const int dn = e0.pl_deck_n(o);
  const int ra = wl0_draw(a.st, o, amount, hint), rb = wl1_draw(b.st, o, amount, hint);
  compare("draw", a, b, ra, rb, i, j);
  t_draw.add(rb);
  if (rb == 0 && hint > 0 && amount == 1 && dn == DECK_CAP) n_deck_remove[hint - 1]++;
}

static void check_draw() {
  const int unit_a = card_of_kind(KIND_UNIT, 0), spell = card_of_kind(KIND_SPELL, 0), structure = card_of_kind(KIND_STRUCT, 0);
  Rec r;
  long long c = 0;
  // the hinted form at every index of every deck size x hand size; hint 0 is the search itself (the empty deck raises)
  for (int dn = 0; dn <= DECK_CAP; dn++)
    for (int hn = 0; hn <= HAND_CAP; hn++)
      for (int hint = 0; hint <= dn; hint++)
        for (int o = 0; o < 2; o++) {
          list_record(r, hn, dn, hn, dn, (c & 1) != 0);
          run_draw(r, o, 1, hint, c++, 0);
        }
  // the unhinted search, several cards in one call (fill_hand at a turn's end), ages up to the table's end
  for (int t = 0; t < 6000; t++) {
    const int dn = (int)(rnd() % 13), hn = (int)(rnd() % 6);
    list_record(r, hn, dn, hn, dn, (t & 1) != 0);
    const Eng e = over(r.st);
    const int o = (int)(rnd() & 1);
    if (t % 3 == 0)
      for (int i = 0; i < dn; i++) r.st[e.pl(o, P_AGE + i)] = (uint8_t)rnd();
    if (rnd() % 32 == 0) r.st[H_FAULT] = FAULT_PY_EXCEPTION;
    run_draw(r, o, 1 + (int)(rnd() % 4), 0, c++, 1);
  }
  // an earlier equal card in the deck
  const int pos_flags[3] = {0, CF_STR, CF_ALIAS};
  for (int idx = 1; idx < DECK_CAP; idx++)
    for (int at = 0; at < idx; at++)
      for (int fa = 0; fa < 3; fa++)
        for (int fb = 0; fb < 3; fb++)
          for (int kind = 0; kind < 3; kind++) {
            list_record(r, (int)(rnd() % 5), idx + 1 + (int)(rnd() % (DECK_CAP - idx)), 4, 8, false);
            const Eng e = over(r.st);
            const int o = (int)(rnd() & 1), card = kind == 0 ? unit_a : (kind == 1 ? structure : spell);
            set_card(r, e.deck_ref(o, at), card), set_flags(r, e.deck_ref(o, at), pos_flags[fa]);
            set_card(r, e.deck_ref(o, idx), card), set_flags(r, e.deck_ref(o, idx), pos_flags[fb]);
            run_draw(r, o, 1, idx + 1, c++, 2);
            if (kind != 2 && !fa && !fb) n_dup_deck++;
          }
}
#endif

// ---- set_path: every record build ------------------------------------------------------------------------------------
static void put_unit(Eng& e, int tile, int slot, int owner, int mov, bool ff, int confused) {
  msb_u32x4 g = {(uint32_t)card_of_kind(KIND_UNIT, 0) | ((uint32_t)(owner | (ff ? EF_FF : 0)) << 8) | ((uint32_t)tile << 16) | ((uint32_t)mov << 24),
                 (uint32_t)confused << 16, 3u << 16, (uint32_t)EK_UNIT << 24};
  e.m.st128g(Eng::eg(slot), g);
  e.board_put(tile, slot);
}
static void path_record(Rec& r, int toplay) {
  memset(r.st, 0, STATE_BYTES);
  Eng e = over(r.st);
  e.rng_attach(g_out[0], g_out[1], rnd() % 1200);
  for (int t = 0; t < 20; t++) e.board_put(t, SLOT_NONE);
  for (int s = 0; s < NUM_ENT; s++) e.m.st8g(Eng::eg(s), EO_CARD, CARD_NONE);
  if (REM_LISTS)
    for (int s = 0; s < NUM_ENT; s++) e.m.st8(E_REM + s, REM_NONE);
  e.m.st8(H_TOPLAY, toplay);
}
static void run_set_path(const Rec& r, int slot, int on_play, long long i, long long j) {
  Rec a = r, b = r;
  const int ra = wl0_set_path(a.st, slot, on_play), rb = wl1_set_path(b.st, slot, on_play);
  compare("set_path", a, b, ra, rb, i, j);
  t_path.add(rb);
}
static void check_set_path() {
  Rec r;
  long long c = 0;
  for (int board = 0; board < 6; board++)
    for (int tile = 0; tile < 20; tile++)
      for (int owner = 0; owner < 2; owner++)
        for (int toplay = 0; toplay < 2; toplay++)
          for (int mov = 0; mov <= 5; mov++)
            for (int ff = 0; ff < 2; ff++)
              for (int confused = 0; confused <= 2; confused++)
                for (int on_play = 0; on_play < 2; on_play++) {
                  path_record(r, toplay);
                  Eng e = over(r.st);
                  // board 0: the unit alone; 1: every other tile an enemy; 2: every other tile a friend; 3..5: each tile empty, friend, enemy
                  int slot = 0;
                  for (int t = 0; t < 20; t++) {
                    if (t == tile) continue;
                    const int k = board == 0 ? 0 : (board == 1 ? 2 : (board == 2 ? 1 : (int)(rnd() % 3)));
                    if (k) put_unit(e, t, ++slot, k == 1 ? owner : owner ^ 1, 1, false, 0);
                  }
                  put_unit(e, tile, 0, owner, mov, ff != 0, confused);
                  run_set_path(r, 0, on_play, c++, board);
                }
  // the sidestep that alternates: the side to play's unit at (1, 3) with movement 4, enemies at (2, 3) and (3, 3), nothing ahead.
  // right to (2, 3); there the left tile is the unit's own, so right again to (3, 3); there the enemy on the left is already a
  // destination and nothing is on the right: ahead to (3, 2), and to (3, 1)
  for (int toplay = 0; toplay < 2; toplay++) {
    path_record(r, toplay);
    Eng e = over(r.st);
    put_unit(e, 3 * 4 + 2, 1, toplay ^ 1, 1, false, 0);
    put_unit(e, 3 * 4 + 3, 2, toplay ^ 1, 1, false, 0);
    put_unit(e, 3 * 4 + 1, 0, toplay, 4, false, 0);
    Rec b = r;
    run_set_path(r, 0, 1, c++, 100);
    if (wl1_set_path(b.st, 0, 1) != 0) fail("sidestep faults", toplay, 0, 0, 0);
    const Eng eb = over(b.st);
    const uint32_t want = (uint32_t)p_pack(P{2, 3}) | ((uint32_t)p_pack(P{3, 3}) << 8) | ((uint32_t)p_pack(P{3, 2}) << 16) | ((uint32_t)p_pack(P{3, 1}) << 24);
    if (eb.e_path(0) != want) fail("sidestep path", toplay, eb.e_path(0), want, 0);
    n_sidestep_seen++;
  }
}

// ---- whole games: step() of the two texts on two copies --------------------------------------------------------------
static void check_games(int games, int max_steps) {
  for (int gi = 0; gi < games; gi++) {
    uint32_t mt[MT_N];
    static uint32_t out[2][MT_N];
    mt_seed(mt, 1000u + (uint32_t)gi);
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
      e.init_game(deck[0], deck[1], (int)(rnd() % 4), (int)(rnd() % 4), 1000u + (uint32_t)gi);
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
      // plays and REPLACE before anything else half of the time: a game of passes checks little
      int action = legal[rnd() % nl];
      if (legal[0] < 152 && (rnd() & 1)) {
        int np = 0;
        while (np < nl && legal[np] < 152) np++;
        action = legal[rnd() % np];
      }
      Rec b = a;
      const int ra = wl0_step(a.st, action), rb = wl1_step(b.st, action);
      compare("step", a, b, ra, rb, gi, s * 1000 + action);
      const int f = over(b.st).fault();
      t_step.add(f);
      n_plays += action < 148;
      n_replaces += action >= 148 && action < 152;
      if (f || (rb & 2)) break;
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

int main() {
  if (wl0_state_bytes() != STATE_BYTES) fail("the two sides are different record builds", wl0_state_bytes(), STATE_BYTES, 0, 0);
  mt_seed(g_mt, 20240611u);
  for (int w = 0; w < 2; w++) {
    mt_twist(g_mt);
    for (int i = 0; i < MT_N; i++) g_out[w][i] = mt_temper(g_mt[i]);
  }
#if !(defined(MSB_EXT) && MSB_EXT)
  check_discard();
  check_draw();
#endif
  check_set_path();
  check_games(NUM_ENT > 64 ? 100 : (NUM_ENT > 24 ? 400 : 1500), 120);
  printf("ok");
  t_discard.print("discard");
  t_draw.print("draw");
  t_path.print("set_path");
  t_step.print("step");
  for (int i = 0; i < 5; i++) printf(" hand_remove%d %lld", i, n_hand_remove[i]);
  for (int i = 0; i < 12; i++) printf(" deck_remove%d %lld", i, n_deck_remove[i]);
  for (int i = 0; i <= 12; i++) printf(" push_at%d %lld", i, n_push_at[i]);
  printf(" dup_hand %lld dup_deck %lld sidestep_seen %lld games %lld plays %lld replaces %lld\n", n_dup_hand, n_dup_deck, n_sidestep_seen, n_games,
         n_plays, n_replaces);
  return 0;
}
#endif
