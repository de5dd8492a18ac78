// Host check of the mask arithmetic of monsoon_amd/csrc/coop_legal.h and of the factored target predicate (rules.h
// target_matches / target_bases / get_targets_hit) against the serial text: legal_mask() and get_targets() of the host
// build of the product core.  Built with the address and UB sanitizers by tests/test_coop_legal_cpu.py and run as a program.
//
// mirror() is coop_legal() with its lanes written as loops: one iteration per hand slot for the three ballots, one per
// tile for the occupied and the `hit` masks; everything else is the header's own functions.  It is compared with
// legal_mask() on
//   1. PLACE: every 20-bit empty mask x front line 0..6 and 255 for the offsets themselves against the plain loop of
//      legal_mask_v, and a board for every single-row pattern and a 1/32 sample of all masks x front line 0..5, under a hand
//      of five units costing 0..4 (slot 4 lands in the second word) with mana 0..5;
//   2. USE: every single-tile and 4 000 random multi-tile `hit` masks x hand slot 0..4 for the bits themselves against the
//      serial SETBIT loop over a point list, and boards holding a matching unit on exactly those tiles under a hand whose
//      slot c holds a targeted spell at cost == mana; random boards x synthetic descriptors of every filter kind (kind, side,
//      types, exclude types, non-hero, status, exclude status, strength limit, bases) x both points of view against get_targets();
//   3. every state of 300 random-policy games on decks that hold all targeted spells of the card table.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rules.h"
#include "coop_legal.h"

using namespace msb;
typedef Engine<FlatMem> Eng;

static uint64_t rnd_x = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {   // xorshift64
  rnd_x ^= rnd_x << 13, rnd_x ^= rnd_x >> 7, rnd_x ^= rnd_x << 17;
  return (uint32_t)(rnd_x >> 32);
}

struct Game {
  alignas(16) uint8_t st[STATE_BYTES];
  uint32_t mt[MT_N];
  uint32_t out[2][MT_N];
  int cur;
  uint32_t pos;
};
static void refill(Game& g, int which) {
  mt_twist(g.mt);
  for (int i = 0; i < MT_N; i++) g.out[which][i] = mt_temper(g.mt[i]);
}
static Eng engine(Game& g) {
  Eng e;
  e.m.p = g.st;
  e.rng_attach(g.out[g.cur], g.out[g.cur ^ 1], g.pos);
  return e;
}
static void commit_rng(Game& g, Eng& e) {
  g.pos = e.rng_pos();
  if (g.pos >= (uint32_t)MT_N) {
    g.pos -= MT_N;
    e.rng_block_advance();
    const int old = g.cur;
    g.cur ^= 1;
    refill(g, old);
  }
}
static void new_game(Game& g, uint32_t seed, const uint8_t* d0, const uint8_t* d1) {
  memset(&g, 0, sizeof(g));
  mt_seed(g.mt, seed);
  refill(g, 0);
  refill(g, 1);
  Eng e = engine(g);
  e.init_game(d0, d1, 0, 0, seed);
  commit_rng(g, e);
}

static void fail(const char* what, long long a, long long b, long long c) {
  printf("FAIL %s: %lld %lld %lld\n", what, a, b, c);
  exit(1);
}

// the tiles whose entity matches, a "lane" per tile
static uint32_t hit_by_tile(Eng& e, const int pov, const Tgt t) {
  uint32_t hit = 0;
  for (int tile = 0; tile < msbk::LEGAL_TILES; tile++) {
    const int slot = e.board_at(tile);
    if (slot != SLOT_NONE && e.target_matches(e.m.ld128g(Eng::eg(slot)), pov, t)) hit |= 1u << tile;
  }
  return hit;
}

static long long n_aimed_cards = 0;
static void mirror(Eng& e, uint64_t m[3]) {
  const int lo = e.local(), pov = e.cp();
  const int hn = e.pl_hand_n(lo), front = e.pl_front(lo), mana = e.pl_mana(lo);
  const bool replacable = (e.m.ld8(e.pl(lo, P_FLAGS)) & 1) != 0;
  uint32_t occ = 0, units = 0, plain = 0, aimed = 0;
  for (int t = 0; t < msbk::LEGAL_TILES; t++)
    if (e.board_at(t) != SLOT_NONE) occ |= 1u << t;
  for (int c = 0; c < hn && c < HAND_CAP; c++) {
    const uint32_t inst = e.m.ld32(e.hand_ref(lo, c));
    const CardInfo& ci = g_cards[inst & 0xff];
    if ((int)((inst >> 8) & 0xff) > mana) continue;
    if (ci.kind != KIND_SPELL) units |= 1u << c;
    else if (!ci.tgt.has) plain |= 1u << c;
    else aimed |= 1u << c;
  }
  const uint32_t empty = ~occ & 0xFFFFFu;
  bool any_play = msbk::legal_compose(m, msbk::legal_place_offsets(empty, front), msbk::legal_place_row0(empty, front), units, plain);
  for (int c = 0; c < HAND_CAP; c++)
    if ((aimed >> c) & 1u) {
      const Tgt t = mk_tgt(g_cards[e.hand_card(lo, c)].tgt);
      const uint32_t hit = hit_by_tile(e, pov, t);
      if (hit != e.get_targets_hit(pov, t)) fail("hit by tile", c, hit, e.get_targets_hit(pov, t));
      any_play |= msbk::legal_add_targets(m, hit, Eng::target_bases(t), c);
      n_aimed_cards++;
    }
  msbk::legal_finish(m, any_play, replacable, hn);
}
static void compare(Eng& e, const char* what, long long a, long long b) {
  uint64_t want[3], got[3];
  e.legal_mask(want);
  mirror(e, got);
  if (memcmp(want, got, sizeof(want)) != 0) {
    printf("want %016llx %016llx %016llx\n got %016llx %016llx %016llx\n", (unsigned long long)want[0], (unsigned long long)want[1],
           (unsigned long long)want[2], (unsigned long long)got[0], (unsigned long long)got[1], (unsigned long long)got[2]);
    fail(what, a, b, 0);
  }
}

// the serial text's way from a point list to bits (rules.h legal_mask_v, MSB_SETBIT)
static void serial_bits(const PList& l, const int c, uint64_t m[3], bool& any_play) {
  for (int i = 0; i < l.n(); i++) {
    const P p = l.at(i);
    const int a = p_valid(p) ? 65 + 21 * c + (4 - p.y) * 4 + p.x : 155;
    if (a < 64) m[0] |= 1ull << a;
    else if (a < 128) m[1] |= 1ull << (a - 64);
    else if (a < 156) m[2] |= 1ull << (a - 128);
    any_play = true;
  }
}

static void put_hand(Eng& e, const int lo, const int c, const int card, const int cost) {
  const int r = e.hand_ref(lo, c);
  e.m.st8(r, card);
  e.m.st8(r + 1, cost);
  e.m.st8(r + 2, CF_XBASE | (g_cards[card].kind == KIND_SPELL ? CF_SPELL : 0));
  e.m.st8(r + 3, g_cards[card].strength);
}
static void put_entity(Eng& e, const int tile, const int card, const bool unit, const int owner, const int str, const uint32_t st4, const int st5) {
  msb_u32x4 g = {(uint32_t)card | ((uint32_t)owner << 8) | ((uint32_t)tile << 16) | (1u << 24), st4,
                 (uint32_t)(st5 & 0xff) | ((uint32_t)(uint16_t)(int16_t)str << 16), unit ? (uint32_t)EK_UNIT << 24 : 0u};
  e.m.st128g(Eng::eg(tile), g);   // entity slot = tile
  e.board_put(tile, tile);
}
static void clear_board(Eng& e) {
  for (int t = 0; t < 20; t++) e.board_put(t, SLOT_NONE);
}

static int a_unit() {   // a unit of the card table without type tags
  for (int i = 0; i < NUM_CARDS; i++)
    if (g_cards[i].kind == KIND_UNIT) return i;
  return 0;
}

static long long check_place(Game& g) {
  long long n = 0;
  const int fronts[8] = {0, 1, 2, 3, 4, 5, 6, 255};
  for (uint32_t empty = 0; empty < (1u << 20); empty++)
    for (int fi = 0; fi < 8; fi++) {
      const int fl = fronts[fi];
      uint32_t place = 0;
      for (int y = 4; y >= 1; y--)
        if (y >= fl) place |= ((empty >> (4 * y)) & 0xFu) << ((4 - y) * 4);
      if (place != msbk::legal_place_offsets(empty, fl)) fail("place offsets", empty, fl, place);
      if ((fl <= 0 && (empty & 0xFu) != 0) != msbk::legal_place_row0(empty, fl)) fail("place row 0", empty, fl, 0);
      n++;
    }
  Eng e = engine(g);
  const int lo = e.local(), unit = a_unit();
  e.m.st8(e.pl(lo, P_HAND_N), 5);
  for (int c = 0; c < 5; c++) put_hand(e, lo, c, unit, c);
  for (uint32_t empty = 0; empty < (1u << 20); empty++) {
    bool single_row = false;
    for (int y = 0; y < 5; y++) {
      const uint32_t others = (empty | (0xFu << (4 * y))) & 0xFFFFFu;
      single_row |= others == (0xFu << (4 * y)) || others == 0xFFFFFu;
    }
    if (!single_row && ((empty * 2654435761u) >> 27) != 0) continue;
    for (int t = 0; t < 20; t++) e.board_put(t, (empty >> t) & 1 ? SLOT_NONE : t);
    for (int fl = 0; fl <= 5; fl++) {
      e.m.st8(e.pl(lo, P_FRONT), fl);
      e.m.st16(e.pl(lo, P_MANA), fl);
      e.m.st8(e.pl(lo, P_FLAGS), (empty >> 3) & 3);
      compare(e, "place board", empty, fl);
      n++;
    }
  }
  return n;
}

static long long check_use(Game& g) {
  long long n = 0;
  for (int k = 0; k < 20 + 4000 + 2; k++) {
    const uint32_t hit = k < 20 ? 1u << k : (k == 20 ? 0u : (k == 21 ? 0xFFFFFu : rnd() & rnd() & 0xFFFFFu));
    PList l;
    l.clear();
    for (int t = 0; t < 20; t++)
      if ((hit >> t) & 1) l.push(tile_p(t));
    for (int c = 0; c < 5; c++) {
      uint64_t want[3] = {0, 0, 0}, got[3] = {0, 0, 0};
      bool any = false;
      serial_bits(l, c, want, any);
      msbk::legal_use_bits(got, hit, c);
      got[2] &= (1ull << 28) - 1;   // (legal_finish cuts the action space off)
      if (memcmp(want, got, sizeof(want)) != 0) fail("use bits", hit, c, 0);
      n++;
    }
    // the same through the engine: a unit on each of the tiles, slot c holds s021 (any unit that is not confused)
    Eng e = engine(g);
    const int lo = e.local(), unit = a_unit();
    clear_board(e);
    for (int t = 0; t < 20; t++)
      if ((hit >> t) & 1) put_entity(e, t, unit, true, t & 1, 3, 0u, 0);
    e.m.st8(e.pl(lo, P_HAND_N), 5);
    e.m.st16(e.pl(lo, P_MANA), 2);
    for (int c = 0; c < 5; c++) {
      for (int j = 0; j < 5; j++) put_hand(e, lo, j, j == c ? C_S021 : unit, j == c ? 2 : 9);
      compare(e, "use board", hit, c);
      n++;
    }
  }
  return n;
}

static long long check_descriptors(Game& g) {
  long long n = 0;
  Eng e = engine(g);
  const int type_cards[6] = {a_unit(), TOKEN_UNIT_BASE + UT_HERO, TOKEN_UNIT_BASE + UT_KNIGHT, TOKEN_UNIT_BASE + UT_DRAGON, TOKEN_STRUCT, 40};
  for (int board = 0; board < 400; board++) {
    clear_board(e);
    const uint32_t occ = board == 0 ? 0u : (board == 1 ? 0xFFFFFu : rnd() & 0xFFFFFu);
    for (int t = 0; t < 20; t++)
      if ((occ >> t) & 1) {
        const int card = type_cards[rnd() % 6];
        const bool unit = card == TOKEN_STRUCT ? false : (card >= NUM_CARDS ? true : g_cards[card].kind == KIND_UNIT);
        uint32_t st4 = 0;
        for (int s = 0; s < 4; s++)
          if (rnd() % 4 == 0) st4 |= (1u + rnd() % 2) << (8 * s);
        put_entity(e, t, card, unit, rnd() & 1, (int)(rnd() % 14) - 2, st4, rnd() % 4 == 0 ? 1 : 0);
      }
    for (int d = 0; d < 64; d++) {
      Tgt t = mk_tgt((int)(rnd() % 3), (int)(rnd() % 3));
      if (rnd() % 3 == 0) t = tgt_types(t, 1 << (rnd() % 16));
      if (rnd() % 3 == 0) t = tgt_xtypes(t, 1 << (rnd() % 16));
      if (rnd() % 3 == 0) t = tgt_non_hero(t);
      if (rnd() % 3 == 0) t = tgt_status(t, 1 + rnd() % 31);
      if (rnd() % 3 == 0) t = tgt_xstatus(t, 1 + rnd() % 31);
      if (rnd() % 3 == 0) t = tgt_limit(t, (int)(rnd() % 12));
      if (rnd() % 3 == 0) t = tgt_base(t);
      for (int pov = 0; pov < 2; pov++) {
        const uint32_t hit = hit_by_tile(e, pov, t);
        if (hit != e.get_targets_hit(pov, t)) fail("descriptor hit", board, d, pov);
        const PList l = e.get_targets(pov, t, PK_NONE);
        uint32_t listed = 0;
        int bases = 0;
        for (int i = 0; i < l.n(); i++) {
          const P p = l.at(i);
          if (p_valid(p)) listed |= 1u << p_tile(p);
          else bases++;
        }
        const int tb = Eng::target_bases(t);
        if (listed != hit || bases != (tb & 1) + (tb >> 1)) fail("descriptor list", board, d, pov);
        for (int c = 0; c < 5; c++) {
          uint64_t want[3] = {0, 0, 0}, got[3] = {0, 0, 0};
          bool any = false;
          serial_bits(l, c, want, any);
          const bool any2 = msbk::legal_add_targets(got, hit, tb, c);
          got[2] &= (1ull << 28) - 1;
          if (memcmp(want, got, sizeof(want)) != 0 || any != any2) fail("descriptor bits", board, d, c);
          n++;
        }
      }
    }
  }
  return n;
}

static long long check_games(long long& aimed_states) {
  static Game g;
  long long n = 0;
  uint8_t pool[NUM_CARDS];
  int np = 0;
  for (int i = 0; i < NUM_CARDS; i++) {
    const bool spell_t = g_cards[i].kind == KIND_SPELL && g_cards[i].tgt.has;
    if (i != C_B005 && i != C_UA20 && g_cards[i].int_id >= 0 && !spell_t) pool[np++] = (uint8_t)i;
  }
  uint8_t aimed[16];
  int na = 0;
  for (int i = 0; i < NUM_CARDS; i++)
    if (g_cards[i].kind == KIND_SPELL && g_cards[i].tgt.has) aimed[na++] = (uint8_t)i;
  if (na < 1 || na > 8) fail("targeted spells of the table", na, 0, 0);
  for (int game = 0; game < 300; game++) {
    uint8_t d[2][DECK_SIZE];
    for (int o = 0; o < 2; o++) {
      for (int i = 0; i < na; i++) d[o][i] = aimed[i];
      for (int i = na; i < DECK_SIZE; i++) {   // distinct cards
        bool again;
        do {
          d[o][i] = pool[rnd() % np];
          again = false;
          for (int j = na; j < i; j++) again |= d[o][j] == d[o][i];
        } while (again);
      }
    }
    new_game(g, 1000 + game, d[0], d[1]);
    for (int step = 0; step < 160; step++) {
      Eng e = engine(g);
      if (e.fault() || e.have_winner()) break;
      const long long before = n_aimed_cards;
      compare(e, "game state", game, step);
      aimed_states += n_aimed_cards != before;
      n++;
      uint64_t m[3];
      e.legal_mask(m);
      int legal[156], nl = 0;
      for (int a = 0; a < 156; a++)
        if ((m[a >> 6] >> (a & 63)) & 1) legal[nl++] = a;
      if (nl == 0) fail("empty legal set", game, step, 0);
      e.step(legal[rnd() % nl]);
      if (e.fault()) break;
      commit_rng(g, e);
    }
  }
  return n;
}

int main() {
  static Game g;
  uint8_t deck[DECK_SIZE];
  for (int i = 0; i < DECK_SIZE; i++) deck[i] = (uint8_t)(24 + i);
  new_game(g, 7, deck, deck);
  const long long place = check_place(g);
  const long long use = check_use(g);
  const long long desc = check_descriptors(g);
  long long aimed_states = 0;
  const long long states = check_games(aimed_states);
  printf("ok %lld place %lld use %lld descriptor %lld states %lld aimed\n", place, use, desc, states, aimed_states);
  return 0;
}
