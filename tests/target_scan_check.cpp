// Host check of the target scans that read only the tiles their caller keeps (monsoon_amd/csrc/rules.h shape_mask,
// get_targets, shape_targets, shape_any, targets_any, target_has) against the -DMSB_TARGET_SCAN=0 text of the same header,
// the *_full forms, which this program calls directly.  Compiled once per record build (no flag, -DMSB_EXT=1,
// -DMSB_EXT=2) over FlatMem with the address and UB sanitizers into a stand-alone program by
// tests/test_target_scan_cpu.py and run, never loaded into Python.
//
// The boards are random: 0..20 entities (board 0 empty, board 1 full) on random tiles in random entity slots, both owners,
// units of every type tag and structures, strengths -2..11, every status alone and combined, both values of the side to play
// and of the current player.  The descriptors are those of the card table plus every literal combination
// the ability files build: kind x side x base, alone and with one of status / xstatus (each of the five), types / xtypes
// (each of the sixteen), non_hero, limit -1..12.  On every board:
//   mask      shape_mask against in_shape: 7 shapes x 20 centres (and the ring of off-board centres around them) x both
//             points of view x all 20 tiles;
//   targets   get_targets against get_targets_full, list for list: every descriptor x both points of view x exclusion of
//             none, of every tile in turn (rotating) and of each base point;
//   shape     shape_targets against shape_targets_full, list for list, and shape_any against its length: a rotating
//             window of the descriptors x 7 shapes x 20 centres x both points of view x exclusion of none, of the centre
//             and of another tile or a base point;
//   any/has   targets_any and target_has against the list's n() > 0 and has(p), p every tile, both base points and the
//             points around the board; and the two of them composed the way Spell.play asks (a position on the board, on
//             each base, and none).
// Prints one "ok ..." line with the number of compared cases per form and per shape; any mismatch prints the place and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "rules.h"

using namespace msb;
typedef Engine<FlatMem> Eng;

static_assert(MSB_TARGET_SCAN == 1, "the program compares the restricted forms with the *_full forms");

static uint64_t rnd_x = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {   // xorshift64
  rnd_x ^= rnd_x << 13, rnd_x ^= rnd_x >> 7, rnd_x ^= rnd_x << 17;
  return (uint32_t)(rnd_x >> 32);
}

struct Game {
  alignas(16) uint8_t st[STATE_BYTES];
  uint32_t mt[MT_N];
  uint32_t out[2][MT_N];
};
static Eng engine(Game& g) {
  Eng e;
  e.m.p = g.st;
  e.rng_attach(g.out[0], g.out[1], 0);
  return e;
}

static void fail(const char* what, long long a, long long b, long long c, long long d) {
  printf("FAIL %s: %lld %lld %lld %lld\n", what, a, b, c, d);
  exit(1);
}
static bool same(const PList& a, const PList& b) {
  if (a.n() != b.n()) return false;
  for (int i = 0; i < a.n(); i++)
    if (a.get(i) != b.get(i)) return false;
  return true;
}

static void put_entity(Eng& e, const int tile, const int slot, const int card, const bool unit, const int owner, const int str, const uint32_t st4,
                       const int st5) {
  msb_u32x4 g = {(uint32_t)card | ((uint32_t)owner << 8) | ((uint32_t)tile << 16) | (1u << 24), st4,
                 (uint32_t)(st5 & 0xff) | ((uint32_t)(uint16_t)(int16_t)str << 16), unit ? (uint32_t)EK_UNIT << 24 : 0u};
  e.m.st128g(Eng::eg(slot), g);
  e.board_put(tile, slot);
}
static int a_unit() {   // a unit of the card table
  for (int i = 0; i < NUM_CARDS; i++)
    if (g_cards[i].kind == KIND_UNIT) return i;
  return 0;
}

static void random_board(Eng& e, const int board) {
  for (int t = 0; t < 20; t++) e.board_put(t, SLOT_NONE);
  const int n = board == 0 ? 0 : (board == 1 ? 20 : (int)(rnd() % 21));
  int tiles[20], slots[20];
  for (int i = 0; i < 20; i++) tiles[i] = slots[i] = i;
  for (int i = 19; i > 0; i--) {
    int j = (int)(rnd() % (i + 1)), k = (int)(rnd() % (i + 1)), x;
    x = tiles[i], tiles[i] = tiles[j], tiles[j] = x;
    x = slots[i], slots[i] = slots[k], slots[k] = x;
  }
  for (int i = 0; i < n; i++) {
    const int kind = (int)(rnd() % 6);
    // a plain unit of the table, a token unit of any type tag (the hero and the dragon among them), a token structure
    const int card = kind == 0 ? a_unit() : (kind == 5 ? TOKEN_STRUCT : TOKEN_UNIT_BASE + (int)(rnd() % 16));
    uint32_t st4 = 0;
    int st5 = 0;
    const int mode = (int)(rnd() % 4);   // no status, one status, random ones
    if (mode == 1) {
      const int s = (int)(rnd() % 5);
      if (s < 4) st4 = (1u + rnd() % 3) << (8 * s);
      else st5 = 1;
    } else if (mode >= 2) {
      for (int s = 0; s < 4; s++)
        if (rnd() % 3 == 0) st4 |= (1u + rnd() % 2) << (8 * s);
      st5 = rnd() % 3 == 0 ? 1 : 0;
    }
    put_entity(e, tiles[i], slots[i] + (NUM_ENT > 24 ? (int)(rnd() % 2) * 20 : 0), card, card != TOKEN_STRUCT, (int)(rnd() & 1), (int)(rnd() % 14) - 2, st4, st5);
  }
  const int toplay = (int)(rnd() & 1);
  e.m.st8(H_TOPLAY, toplay);
  e.m.st8(H_CP, (int)(rnd() & 1));
  e.set_pl_front(0, (int)(rnd() % 5));
  e.set_pl_front(1, (int)(rnd() % 5));
}

static std::vector<Tgt> g_desc;
static size_t g_table_desc = 0;
static void descriptors() {
  for (int i = 0; i < NUM_CARDS; i++)
    if (g_cards[i].tgt.has) g_desc.push_back(mk_tgt(g_cards[i].tgt));
  g_table_desc = g_desc.size();
  for (int kind = 0; kind < 3; kind++)
    for (int side = 0; side < 3; side++)
      for (int base = 0; base < 2; base++) {
        Tgt b = mk_tgt(kind, side);
        if (base) b = tgt_base(b);
        g_desc.push_back(b);
        for (int s = 0; s < 5; s++) g_desc.push_back(tgt_status(b, 1 << s)), g_desc.push_back(tgt_xstatus(b, 1 << s));
        for (int k = 0; k < 16; k++) g_desc.push_back(tgt_types(b, 1 << k)), g_desc.push_back(tgt_xtypes(b, 1 << k));
        g_desc.push_back(tgt_non_hero(b));
        for (int lim = -1; lim <= 12; lim++) g_desc.push_back(tgt_limit(b, lim));
      }
}

static long long n_mask[7], n_shape[7], n_shape_any[7];
static long long n_targets, n_any, n_has, n_spell, n_scan_none, n_scan_many;

static const P BASES[2] = {P{-1, 5}, P{-1, -1}};

static void check_mask(Eng& e, const int board) {
  e.m.st8(H_TOPLAY, board & 1);   // the mask reads the side to play only: boards 0 and 1 hold both
  for (int shape = 0; shape < 7; shape++)
    for (int cy = -1; cy <= 5; cy++)
      for (int cx = -1; cx <= 4; cx++)
        for (int pov = 0; pov < 2; pov++) {
          const P c{cx, cy};
          const uint32_t mask = e.shape_mask(shape, c, pov);
          if (mask >> 20) fail("mask outside the board", board, shape, cx, cy);
          for (int t = 0; t < 20; t++) {
            if (((mask >> t) & 1u) != (uint32_t)e.in_shape(shape, c, pov, tile_p(t))) fail("shape_mask", shape, cx * 8 + cy, pov, t);
            if (p_valid(c)) n_mask[shape]++;
          }
        }
}

static void check_targets(Eng& e, const int board) {
  for (size_t d = 0; d < g_desc.size(); d++)
    for (int pov = 0; pov < 2; pov++) {
      const Tgt t = g_desc[d];
      const int ex[4] = {PK_NONE, p_pack(tile_p((int)((d + board) % 20))), p_pack(BASES[0]), p_pack(BASES[1])};
      for (int x = 0; x < 4; x++) {
        if (!same(e.get_targets(pov, t, ex[x]), e.get_targets_full(pov, t, ex[x]))) fail("get_targets", board, (long long)d, pov, x);
        n_targets++;
      }
      const PList l = e.get_targets_full(pov, t, PK_NONE);
      if (e.targets_any(pov, t) != (l.n() > 0)) fail("targets_any", board, (long long)d, pov, 0);
      n_any++;
      for (int y = -1; y <= 5; y++)
        for (int x = -1; x <= 4; x++) {
          const P p{x, y};
          if (e.target_has(pov, t, p) != l.has(p)) fail("target_has", board, (long long)d, pov, p_pack(p));
          n_has++;
        }
      // Spell.play (rules.h call_spell_play): with a position `position in targets`, without one an exception unless the list is empty
      for (int k = 0; k < 23; k++) {
        const bool has_pos = k < 22;
        const P position = k < 20 ? tile_p(k) : (k < 22 ? BASES[k - 20] : P{0, 0});
        const bool go_full = has_pos && l.has(position), exc_full = !has_pos && l.n() > 0;
        const bool go = has_pos && e.target_has(pov, t, position), exc = !has_pos && e.targets_any(pov, t);
        if (go != go_full || exc != exc_full) fail("spell play", board, (long long)d, pov, k);
        n_spell++;
      }
    }
}

static void check_shapes(Eng& e, const int board) {
  const int window = 32;
  for (int w = 0; w < window; w++) {
    // the card table's descriptors on every board, the literal ones in turn
    const size_t d = (size_t)w < g_table_desc && w < 8 ? (size_t)w : ((size_t)board * (window - 8) + w) % g_desc.size();
    const Tgt t = g_desc[d];
    for (int shape = 0; shape < 7; shape++)
      for (int centre = 0; centre < 20; centre++)
        for (int pov = 0; pov < 2; pov++) {
          const P c = tile_p(centre);
          const int other = (int)(rnd() % 22);
          const int ex[3] = {PK_NONE, p_pack(c), other < 20 ? p_pack(tile_p(other)) : p_pack(BASES[other - 20])};
          for (int x = 0; x < 3; x++) {
            const PList want = e.shape_targets_full(shape, c, pov, t, ex[x]);
            if (!same(e.shape_targets(shape, c, pov, t, ex[x]), want)) fail("shape_targets", board, (long long)d, shape * 100 + centre, pov * 10 + x);
            n_shape[shape]++;
            if (x == 0) {
              if (e.shape_any(shape, c, pov, t) != (want.n() > 0)) fail("shape_any", board, (long long)d, shape * 100 + centre, pov);
              n_shape_any[shape]++;
              n_scan_none += want.n() == 0;
              n_scan_many += want.n() > 1;
            }
          }
        }
  }
}

int main() {
  static Game g;
  memset(&g, 0, sizeof(g));
  Eng e = engine(g);
  descriptors();
  const int boards = 120;
  for (int board = 0; board < boards; board++) {
    random_board(e, board);
    if (board < 4) check_mask(e, board);   // (the mask reads the side to play only)
    check_targets(e, board);
    check_shapes(e, board);
  }
  printf("ok boards %d descriptors %d table_descriptors %d targets %lld any %lld has %lld spell %lld scan_none %lld scan_many %lld", boards,
         (int)g_desc.size(), (int)g_table_desc, n_targets, n_any, n_has, n_spell, n_scan_none, n_scan_many);
  for (int s = 0; s < 7; s++) printf(" mask%d %lld shape%d %lld shape_any%d %lld", s, n_mask[s], s, n_shape[s], s, n_shape_any[s]);
  printf("\n");
  return 0;
}
