// Host check of the short ability effects on whole words (monsoon_amd/csrc/rules.h ei_need_unit / ei_st_add / ei_st_remove /
// heal_vitalize: MSB_WIDE_AB_ST; gain_speed through set_path_known: MSB_WIDE_AB_SPEED; Pick / choice_tile / targets_pick /
// shape_pick / empty_front_pick: MSB_WIDE_AB_PICK; state.h) against the text with the three switches at 0.
// tests/test_wide_ab_cpu.py compiles this file twice over FlatMem with the address and UB sanitizers -- once with -DWA_SIDE=0
// -Dmsb=msb_fields -DMSB_WIDE_AB_ST=0 -DMSB_WIDE_AB_SPEED=0 -DMSB_WIDE_AB_PICK=0 (the per-field text; the namespace renamed, so
// the two texts of the core are two sets of symbols) and once with -DWA_SIDE=1 (and main) -- links the two objects into a
// stand-alone program and runs it, never loaded into Python.  Side 1 is built with all three parts (-DMSB_WIDE_AB_ST=1
// -DMSB_WIDE_AB_SPEED=1: two of them are switches the product does not build) and with the product's defaults.  On the extended
// and large records every switch is off on both sides: there the program pins that the switches change nothing.
//
// Every generated record is copied, one text runs on each copy, and the record bytes, the return value and the fault code must
// be identical, also where the call faults.  Nothing is skipped.  Parts:
//   effect   freeze, poison, vitalize, confuse, deconfuse, disable, heal-then-vitalize (the card's and the spells' form) and
//            b203's deconfuse-if-confused on: a unit with an ability, a unit without, a structure, both base ids and an empty
//            tile (-1) x the effect's own count at 0, 1, 254, 255 x the opposite status (poisoned for vitalize, vitalized for
//            poison) at 0, 1, 255 x strength 1, 9 and 32765 x a record without and with a fault x both sides to play;
//   speed    gain_speed(1..3) of a unit on every tile of rows 0-4 x both owners x both sides to play x movement 0..3 x
//            confused 0, 1, 2 x resolving or not x three boards (empty, and two with random other units around);
//   choice   choice_tile(hit, bases, asc) against choice_point(hit_list(hit, asc) + bases) for random 20-bit masks (the empty
//            and the full one among them) x both orders x bases 0..3 x every draw value 0..n-1 (the stream holds the value):
//            the same point, the same number of words drawn (side 1 only: both forms live in the text with the pick);
//   pick     targets_pick / shape_pick / empty_front_pick and the draw, on the records of the games below and on both
//            points of view: kinds x sides x base or not x an excluded tile or base, five shapes around every third tile;
//   games    whole games of random legal actions on N12M and on a deck of the touched cards (u007 u021 u061 u053 u051 u050 ua07
//            ud01 u055 s007 s012 ue03): step() of the two texts on two copies, record for record; how often each touched
//            card's ability ran is counted.
// Prints one "ok ..." line: per part the number of compared cases and their outcomes, and how often each thing happened.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "rules.h"

#ifndef WA_SIDE
#error "compile with -DWA_SIDE=0 (-Dmsb=msb_fields, the three MSB_WIDE_AB_* switches at 0) and with -DWA_SIDE=1"
#endif

using namespace msb;
typedef Engine<FlatMem> Eng;

#define WA_CAT2(a, b) a##b
#define WA_CAT(a, b) WA_CAT2(a, b)
#define WA_FN(name) WA_CAT(WA_CAT(wa, WA_SIDE), name)

#if WA_SIDE == 0
static_assert(!MSB_AB_ST && !MSB_AB_SPEED && !MSB_AB_PICK, "side 0 is the per-field text");
#elif defined(MSB_EXT) && MSB_EXT
static_assert(!MSB_AB_ST && !MSB_AB_SPEED && !MSB_AB_PICK, "the records with worlds keep the per-field text");
#else
static_assert(MSB_AB_PICK, "side 1 builds the pick (and, with -DMSB_WIDE_AB_ST=1 -DMSB_WIDE_AB_SPEED=1, the other two parts)");
#endif

enum { OP_FREEZE, OP_POISON, OP_VITALIZE, OP_CONFUSE, OP_DECONFUSE, OP_DISABLE, OP_HEAL_VIT, OP_HEAL_VIT_CHECKED, OP_DECONFUSE_IF, OP_COUNT };

static Eng over(uint8_t* st) {
  Eng e;
  e.m.p = st;
  return e;
}
extern "C" int WA_FN(_state_bytes)() { return STATE_BYTES; }
extern "C" int WA_FN(_parts)() { return (MSB_AB_ST ? 1 : 0) | (MSB_AB_SPEED ? 2 : 0) | (MSB_AB_PICK ? 4 : 0); }
extern "C" int WA_FN(_step)(uint8_t* st, int action) {
  Eng e = over(st);
  return e.step(action);
}
extern "C" int WA_FN(_effect)(uint8_t* st, int op, int who, int amount) {
  Eng e = over(st);
  int ret = 0;
  switch (op) {
    case OP_FREEZE: e.freeze(who); break;
    case OP_POISON: e.poison(who); break;
    case OP_VITALIZE: e.vitalize(who); break;
    case OP_CONFUSE: e.confuse(who); break;
    case OP_DECONFUSE: e.deconfuse(who); break;
    case OP_DISABLE: e.disable(who); break;
#if MSB_AB_ST
    case OP_HEAL_VIT: e.heal_vitalize(who, amount, false); break;
    case OP_HEAL_VIT_CHECKED: e.heal_vitalize(who, amount, true); break;
#else   // the two calls as the cards spell them (abilities.inc MSB_HEAL_VITALIZE / MSB_HEAL_VITALIZE_CHECKED)
    case OP_HEAL_VIT: e.heal(who, amount); e.vitalize(who); break;
    case OP_HEAL_VIT_CHECKED: e.heal(who, amount); if (!e.fault()) e.vitalize(who); break;
#endif
    case OP_DECONFUSE_IF: ret = e.deconfuse_if_confused(who) ? 1 : 0; break;
  }
  return ret * 256 + e.fault();
}
extern "C" int WA_FN(_gain_speed)(uint8_t* st, int who, int amount) {
  Eng e = over(st);
  e.gain_speed(who, amount);
  return e.fault();
}
// mode 0: targets_pick(pov, t, exclude); 1: shape_pick(shape, centre, pov, t); 2: empty_front_pick(pov as the order).
// Returns n * 256 + the packed point drawn (no draw and 255 where the list is empty).
extern "C" int WA_FN(_pick)(uint8_t* st, int mode, int shape, int centre, int pov, int kind, int side, int base, int exclude_pk) {
  Eng e = over(st);
  Tgt t = mk_tgt(kind, side);
  if (base) t = tgt_base(t);
  const Eng::Pick q = mode == 0 ? e.targets_pick(pov, t, exclude_pk) : (mode == 1 ? e.shape_pick(shape, tile_p(centre), pov, t) : e.empty_front_pick(pov));
  const int n = q.n();
  return n * 256 + (n > 0 ? p_pack(e.choice_tile(q)) : 255);
}

#if WA_SIDE == 1
extern "C" int wa0_state_bytes();
extern "C" int wa0_step(uint8_t* st, int action);
extern "C" int wa0_effect(uint8_t* st, int op, int who, int amount);
extern "C" int wa0_gain_speed(uint8_t* st, int who, int amount);
extern "C" int wa0_pick(uint8_t* st, int mode, int shape, int centre, int pov, int kind, int side, int base, int exclude_pk);

static uint64_t rnd_x = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {   // xorshift64
  rnd_x ^= rnd_x << 13, rnd_x ^= rnd_x >> 7, rnd_x ^= rnd_x << 17;
  return (uint32_t)(rnd_x >> 32);
}

struct Rec {
  alignas(16) uint8_t st[STATE_BYTES];
};
static uint32_t g_mt[MT_N];
static uint32_t g_out[2][MT_N];    // the fixed stream of the described records: both copies of a record point at it
static uint32_t g_draw[2][MT_N];   // a stream that holds one value everywhere: the next draw is that value

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
static Tally t_effect, t_speed, t_step;
static long long n_choice, n_choice_base, n_choice_empty, n_pick, n_pick_empty, n_pick_base, n_pick_drawn;
static long long n_sat, n_removed_at_zero, n_not_a_unit, n_vit_took_poison, n_poison_took_vit, n_fault_kept, n_no_ability, n_healed_structure, n_deconfused;
static long long n_speed_path[PATH_CAP + 1], n_speed_confused_draw, n_speed_resolving_long, n_speed_cap;
static long long n_games, n_ran[NUM_CARDS];

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
static std::vector<int> g_plain;   // units without an ability
static int g_ability_unit = -1;

static void find_cards() {
  for (int i = 0; i < NUM_CARDS; i++) {
    const CardInfo& c = g_cards[i];
    if (c.kind != KIND_UNIT) continue;
    if (!c.has_ability) g_plain.push_back(i);
    else if (g_ability_unit < 0) g_ability_unit = i;
  }
  if (g_plain.size() < 12 || g_ability_unit < 0) fail("too few units", (long long)g_plain.size(), g_ability_unit, 0, 0);
}

struct Unit {
  int card, owner, str, mov, ff, st[5], resolving;
};
struct Desc {
  int toplay, base[2];
  bool on[20];
  Unit u[20];
  void clear(int toplay_) {
    toplay = toplay_, base[0] = base[1] = 10;
    for (int t = 0; t < 20; t++) on[t] = false;
  }
  void put(int tile, int card, int owner, int str, int mov = 1) {
    on[tile] = true;
    u[tile] = Unit{card, owner, str, mov, 0, {0, 0, 0, 0, 0}, 0};
  }
};
static void push_card(std::vector<int32_t>& S, int card, int oid) {
  const int v[8] = {card, g_cards[card].cost, 0, 0, g_cards[card].kind == KIND_SPELL ? -1 : g_cards[card].strength, 0, 1 + oid, oid};
  S.insert(S.end(), v, v + 8);
}
static void build(Rec& r, const Desc& d) {
  std::vector<int32_t> S;
  const int hdr[5] = {d.toplay, d.toplay, PH_PLAY, 0, 0};
  S.insert(S.end(), hdr, hdr + 5);
  for (int o = 0; o < 2; o++) {
    const int pl[7] = {d.base[o], 30, 5, o == d.toplay ? 1 : 3, 1, 1, 0};
    S.insert(S.end(), pl, pl + 7);
    int oid = 0, fi = 0;
    S.push_back(4);
    for (int i = 0; i < 4; i++) push_card(S, g_plain[fi++], oid++);
    S.push_back(6);
    for (int i = 0; i < 6; i++) push_card(S, g_plain[fi++], oid++);
  }
  for (int t = 0; t < 20; t++) {
    S.push_back(d.on[t] ? 1 : 0);
    if (!d.on[t]) continue;
    const Unit& u = d.u[t];
    const int v[17] = {u.card, u.owner, u.str, u.mov, u.ff, u.st[0], u.st[1], u.st[2], u.st[3], u.st[4], -1, 0, (int)(rnd() & 0xff), u.resolving, 0, 0, 0};
    S.insert(S.end(), v, v + 17);
  }
  memset(r.st, 0, STATE_BYTES);
  Eng e = over(r.st);
  e.rng_attach(g_out[0], g_out[1], rnd() % 600);
  e.scn_build(S.data(), 7u);
  if (e.fault()) fail("scn_build faults", e.fault(), 0, 0, 0);
}

static int op_status(int op) {
  switch (op) {
    case OP_FREEZE: return ST_FROZEN;
    case OP_POISON: return ST_POISONED;
    case OP_DISABLE: return ST_DISABLED;
    case OP_CONFUSE: case OP_DECONFUSE: case OP_DECONFUSE_IF: return ST_CONFUSED;
    default: return ST_VITALIZED;
  }
}
static int op_opposite(int op) { return op == OP_POISON ? ST_VITALIZED : ((op == OP_VITALIZE || op == OP_HEAL_VIT || op == OP_HEAL_VIT_CHECKED) ? ST_POISONED : -1); }

static void check_effects() {
  const int counts[4] = {0, 1, 254, 255}, others[3] = {0, 1, 255}, strs[3] = {1, 9, 32765};
  long long c = 0;
  for (int op = 0; op < OP_COUNT; op++)
    for (int target = 0; target < 6; target++)   // unit with an ability, plain unit, structure, base 0, base 1, empty tile
      for (int ci = 0; ci < 4; ci++)
        for (int oi = 0; oi < 3; oi++)
          for (int si = 0; si < 3; si++)
            for (int fault0 = 0; fault0 < 2; fault0++)
              for (int toplay = 0; toplay < 2; toplay++) {
                const int tile = 2 * 4 + 1, s = op_status(op), os = op_opposite(op);
                Desc d;
                d.clear(toplay);
                if (target < 3) {
                  d.put(tile, target == 0 ? g_ability_unit : (target == 1 ? g_plain[0] : C_B001), toplay ^ (ci & 1), strs[si]);
                  d.u[tile].st[s] = counts[ci];
                  if (os >= 0) d.u[tile].st[os] = others[oi];
                }
                d.put(3 * 4 + 2, g_plain[1], toplay, 3);   // a bystander: its granule must not move
                Rec r;
                build(r, d);
                if (fault0) r.st[H_FAULT] = FAULT_CAPACITY;
                const int who = target < 3 ? over(r.st).board_at(tile) : (target == 5 ? -1 : AT_PLAYER + (target - 3));
                Rec a = r, b = r;
                const int amount = 5;
                const int ra = wa0_effect(a.st, op, who, amount), rb = wa1_effect(b.st, op, who, amount);
                compare("effect", a, b, ra, rb, c++, op * 100 + target * 10 + ci);
                t_effect.add(b.st[H_FAULT]);
                const int f = b.st[H_FAULT];
                if (fault0) {
                  n_fault_kept += f == FAULT_CAPACITY;
                  continue;
                }
                if (target >= 2) n_not_a_unit += f == FAULT_PY_EXCEPTION;
                if (target == 2 && (op == OP_HEAL_VIT || op == OP_HEAL_VIT_CHECKED)) n_healed_structure += over(b.st).e_str(who) != strs[si];
                if (target < 2) {
                  const uint8_t* e0 = r.st + Eng::ent(who);
                  const uint8_t* e1 = b.st + Eng::ent(who);
                  n_sat += f == FAULT_STATUS_SAT;
                  if (op == OP_DECONFUSE) n_removed_at_zero += f == FAULT_PY_EXCEPTION && counts[ci] == 0;
                  if (op == OP_DECONFUSE_IF) n_deconfused += e1[EO_ST + ST_CONFUSED] + 1 == e0[EO_ST + ST_CONFUSED];
                  if (op == OP_VITALIZE && others[oi] > 0) n_vit_took_poison += e1[EO_ST + ST_POISONED] + 1 == e0[EO_ST + ST_POISONED];
                  if (op == OP_POISON && others[oi] > 0) n_poison_took_vit += e1[EO_ST + ST_VITALIZED] + 1 == e0[EO_ST + ST_VITALIZED];
                  if (op == OP_DISABLE && target == 1) n_no_ability += f == 0 && e1[EO_ST + ST_DISABLED] == e0[EO_ST + ST_DISABLED];
                }
              }
}

static void check_speed() {
  long long c = 0;
  for (int tile = 0; tile < 20; tile++)
    for (int owner = 0; owner < 2; owner++)
      for (int toplay = 0; toplay < 2; toplay++)
        for (int mov = 0; mov < 4; mov++)
          for (int amount = 1; amount <= 3; amount++)
            for (int confused = 0; confused < 3; confused++)
              for (int resolving = 0; resolving < 2; resolving++)
                for (int board = 0; board < 3; board++) {
                  Desc d;
                  d.clear(toplay);
                  d.put(tile, g_plain[0], owner, 4, mov);
                  d.u[tile].st[ST_CONFUSED] = confused;
                  d.u[tile].resolving = resolving;
                  if (board)
                    for (int q = 0; q < 20; q++)
                      if (q != tile && rnd() % 3 == 0) d.put(q, rnd() % 4 ? g_plain[2] : C_B001, (int)(rnd() & 1), 3);
                  Rec r;
                  build(r, d);
                  const int who = over(r.st).board_at(tile);
                  Rec a = r, b = r;
                  const int ra = wa0_gain_speed(a.st, who, amount), rb = wa1_gain_speed(b.st, who, amount);
                  compare("speed", a, b, ra, rb, c++, tile * 100 + mov * 10 + amount);
                  t_speed.add(rb);
                  if (b.st[Eng::ent(who) + EO_MOV] != mov) fail("gain_speed left another movement", tile, mov, amount, b.st[Eng::ent(who) + EO_MOV]);
                  n_speed_cap += rb == FAULT_CAP_PATH;
                  if (rb) continue;
                  const int pn = b.st[Eng::ent(who) + EO_PATHN];
                  n_speed_path[pn <= PATH_CAP ? pn : PATH_CAP]++;
                  n_speed_confused_draw += over(b.st).rng_pos() != over(r.st).rng_pos();
                  n_speed_resolving_long += resolving && pn > 1;
                }
}

#if MSB_AB_PICK
static void check_choice() {
  for (int round = 0; round < 400; round++) {
    const uint32_t hit = round == 0 ? 0u : (round == 1 ? 0xFFFFFu : (rnd() & rnd() & 0xFFFFFu) | (round & 1 ? rnd() & 0xFFFFFu : 0u));
    for (int asc = 0; asc < 2; asc++)
      for (int bases = 0; bases < 4; bases++) {
        PList l = Eng::hit_list(hit, asc != 0);
        if (bases & 1) l.push(Eng::base_point(true, asc != 0));
        if (bases & 2) l.push(Eng::base_point(false, asc != 0));
        const int n = l.n();
        if (n == 0) {   // no caller draws over an empty list
          n_choice_empty++;
          continue;
        }
        for (int r = 0; r < n; r++) {
          for (int w = 0; w < 2; w++)
            for (int i = 0; i < MT_N; i++) g_draw[w][i] = (uint32_t)r;
          Rec a, b;
          memset(a.st, 0, STATE_BYTES);
          over(a.st).rng_attach(g_draw[0], g_draw[1], 3);
          b = a;
          Eng ea = over(a.st), eb = over(b.st);
          const P pa = ea.choice_point(l), pb = eb.choice_tile(hit, bases, asc != 0);
          if (p_pack(pa) != p_pack(pb) || p_pack(pa) != l.get(r)) fail("choice_tile", hit, asc * 10 + bases, r, p_pack(pb));
          compare("choice", a, b, 0, 0, hit, r);
          n_choice++;
          n_choice_base += !p_valid(pb);
        }
      }
  }
}
#endif

// the pick on one record: both texts on copies
static void pick_case(const Rec& r, int mode, int shape, int centre, int pov, int kind, int side, int base, int exclude_pk, long long i) {
  Rec a = r, b = r;
  const int ra = wa0_pick(a.st, mode, shape, centre, pov, kind, side, base, exclude_pk), rb = wa1_pick(b.st, mode, shape, centre, pov, kind, side, base, exclude_pk);
  compare("pick", a, b, ra, rb, i, mode * 1000 + shape * 100 + centre);
  n_pick++;
  n_pick_empty += (rb >> 8) == 0;
  n_pick_drawn += over(b.st).rng_pos() != over(const_cast<uint8_t*>(r.st)).rng_pos();
  if ((rb >> 8) > 0) n_pick_base += !p_valid(p_unpack(rb & 0xff));
}
static void check_picks_on(const Rec& r, long long i) {
  if (r.st[H_FAULT]) return;
  const int kinds[3] = {TK_ANY, TK_UNIT, TK_STRUCTURE}, sides[3] = {TS_ANY, TS_FRIENDLY, TS_ENEMY};
  const int shapes[5] = {SH_SIDE, SH_ROW, SH_COLUMN, SH_BORDERING, SH_SURROUNDING};
  for (int pov = 0; pov < 2; pov++) {
    for (int k = 0; k < 3; k++)
      for (int s = 0; s < 3; s++)
        for (int base = 0; base < 2; base++) {
          const int which = (int)(rnd() % 4);   // nothing, a tile, one base, the other
          const int excl = which == 0 ? PK_NONE : (which == 1 ? p_pack(tile_p((int)(rnd() % 20))) : p_pack(which == 2 ? P{-1, 5} : P{-1, -1}));
          pick_case(r, 0, 0, 0, pov, kinds[k], sides[s], base, excl, i);
          for (int sh = 0; sh < 5; sh++) pick_case(r, 1, shapes[sh], (int)((i + 3 * sh + 7 * k) % 20), pov, kinds[k], sides[s], base, PK_NONE, i);
        }
    pick_case(r, 2, 0, 0, pov, 0, 0, 0, PK_NONE, i);
  }
}

// ---- whole games: step() of the two texts on two copies --------------------------------------------------------------------
static int32_t g_trace[2 * 256];
static void check_games(const uint8_t* deck12, int games, int max_steps, uint32_t seed0) {
  for (int gi = 0; gi < games; gi++) {
    uint32_t mt[MT_N];
    static uint32_t out[2][MT_N];
    mt_seed(mt, seed0 + (uint32_t)gi);
    int cur = 0;
    for (int w = 0; w < 2; w++) {
      mt_twist(mt);
      for (int i = 0; i < MT_N; i++) out[w][i] = mt_temper(mt[i]);
    }
    uint32_t pos = 0;
    Rec a;
    memset(a.st, 0, STATE_BYTES);
    {
      Eng e = over(a.st);
      e.rng_attach(out[0], out[1], 0);
      e.init_game(deck12, deck12, (int)(rnd() % 4), (int)(rnd() % 4), seed0 + (uint32_t)gi);
      if (e.fault()) fail("init_game faults", e.fault(), gi, 0, 0);
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
      int action = legal[rnd() % nl];
      if (legal[0] < 148 && rnd() % 3) {   // plays before anything else two times in three
        int np = 0;
        while (np < nl && legal[np] < 148) np++;
        action = legal[rnd() % np];
      }
      if (s % 4 == 0) check_picks_on(a, (long long)gi * 1000 + s);
      Rec x = a, b = a;
      const int ra = wa0_step(x.st, action);
      msb_trace_log = g_trace, msb_trace_n = 0, msb_trace_cap = 256;
      const int rb = wa1_step(b.st, action);
      msb_trace_log = nullptr;
      compare("step", x, b, ra, rb, gi, s * 1000 + action);
      t_step.add(b.st[H_FAULT]);
      for (int i = 0; i < msb_trace_n; i++)
        if (g_trace[2 * i] >= 0 && g_trace[2 * i] < NUM_CARDS) n_ran[g_trace[2 * i]]++;
      a = b;
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

int main() {
  if (wa0_state_bytes() != STATE_BYTES) fail("the two sides are different record builds", wa0_state_bytes(), STATE_BYTES, 0, 0);
  mt_seed(g_mt, 20240613u);
  for (int w = 0; w < 2; w++) {
    mt_twist(g_mt);
    for (int i = 0; i < MT_N; i++) g_out[w][i] = mt_temper(g_mt[i]);
  }
  find_cards();
  check_effects();
  check_speed();
#if MSB_AB_PICK
  check_choice();
#endif
  const uint8_t n12m[12] = {C_U001, C_U007, C_U020, C_U021, C_U026, C_U053, C_U061, C_UA07, C_UE01, C_S001, C_S012, C_B002};
  const uint8_t touched[12] = {C_U007, C_U021, C_U061, C_U053, C_U051, C_U050, C_UA07, C_UD01, C_U055, C_S007, C_S012, C_UE03};
  const int games = NUM_ENT > 64 ? 40 : (NUM_ENT > 24 ? 80 : 250);
  check_games(n12m, games, 160, 5000u);
  check_games(touched, games, 160, 9000u);
  printf("ok parts %d", wa1_parts());
  t_effect.print("effect");
  t_speed.print("speed");
  t_step.print("step");
  printf(" choice %lld choice_base %lld choice_empty %lld pick %lld pick_empty %lld pick_base %lld pick_drawn %lld", n_choice, n_choice_base, n_choice_empty, n_pick,
         n_pick_empty, n_pick_base, n_pick_drawn);
  printf(" sat %lld removed_at_zero %lld not_a_unit %lld vit_took_poison %lld poison_took_vit %lld fault_kept %lld no_ability %lld healed_structure %lld deconfused %lld",
         n_sat, n_removed_at_zero, n_not_a_unit, n_vit_took_poison, n_poison_took_vit, n_fault_kept, n_no_ability, n_healed_structure, n_deconfused);
  for (int i = 0; i <= PATH_CAP; i++) printf(" speed_path%d %lld", i, n_speed_path[i]);
  printf(" speed_confused_draw %lld speed_resolving_long %lld speed_cap %lld games %lld", n_speed_confused_draw, n_speed_resolving_long, n_speed_cap, n_games);
  const int cards[16] = {C_U007, C_U021, C_U061, C_U053, C_U051, C_U050, C_UA07, C_UD01, C_U055, C_S007, C_S012, C_UE03, C_UE01, C_U001, C_B002, C_U026};
  const char* names[16] = {"u007", "u021", "u061", "u053", "u051", "u050", "ua07", "ud01", "u055", "s007", "s012", "ue03", "ue01", "u001", "b002", "u026"};
  for (int i = 0; i < 16; i++) printf(" ran_%s %lld", names[i], n_ran[cards[i]]);
  printf("\n");
  return 0;
}
#endif
