// Card abilities, included inside Engine<M> (rules.h).  One entry per card class of
// /root/reference/cards/<id>.py (activate_ability); `e` is the entity slot of `self`,
// `self.player` = e_owner(e); a Context without pov uses board.current_player (board.py:151-152).
//
// Two kinds of entries (ability_cases.inc):
//   * LEAF abilities (MSB_CARD / MSB_SPELL) call nothing that can call an ability back: one non-inlined function each.
//   * The others (MSB_CARD_K / MSB_SPELL_K) deal damage, destroy, command, force an attack or play a card: they work
//     on the work stack `k` (its pointer goes in and comes back by value).  A nested call in TAIL position is just
//     call_X(k, ..); a loop around nested calls becomes an F_EACH frame, a call with something behind it an F_AFTER
//     frame (below).
//
// The standard build refuses ua20 and b005 at reset (they need the extended record: larger deck, snapshot pool) --
// see card_unsupported() in monsoon_hip.hip.

MSB_HD MSB_INL PList sel_targets(int shape, P c, int pov, Tgt t) { return shape_targets(shape, c, pov, t, PK_NONE); }

// len(<selector>(.., target)) > 0
MSB_HD MSB_INL bool sel_any(int shape, P c, int pov, Tgt t) { return shape_any(shape, c, pov, t); }

// [tile for tile in <raw shape tiles> if board.at(tile) is None]
MSB_HD MSB_A_TILES PList empty_shape_tiles(int shape, P c, int pov) {
  PList raw = shape_tiles(shape, c, pov);
  PList out;
  out.clear();
  int m = raw.n();
  for (int i = 0; i < m; i++)
    if (at(raw.at(i)) == AT_NONE) out.push_raw(raw.get(i));
  return out;
}
// Player.get_within_front_line, player.py:101-111 (uses the player's ORDER, not local/remote)
MSB_HD MSB_A_TILES PList empty_within_front_line(int order) {
  PList out;
  out.clear();
  int fl = pl_front(order);
  if (order == 0) {
    for (int y = fl; y < 5; y++)
      for (int x = 0; x < 4; x++) {
        P p{x, y};
        if (at(p) == AT_NONE) out.push(p);
      }
  } else {
    for (int y = fl; y >= 0; y--)
      for (int x = 3; x >= 0; x--) {
        P p{x, y};
        if (p_valid(p) && at(p) == AT_NONE) out.push(p);
      }
  }
  return out;
}

// cards/b305.py:24-31: the units around the other b305 move to the same offsets around this one
MSB_HD MSB_INL void b305_relocate(P tp, P mypos, int dpov) {
  PList around = sel_targets(SH_SURROUNDING, tp, dpov, mk_tgt(TK_UNIT, TS_ANY));
  for (int k = 0; k < around.n() && !fault(); k++) {
    P tile = around.at(k);
    P to{tile.x - tp.x + mypos.x, tile.y - tp.y + mypos.y};
    if (p_valid(to)) {
      int u = at(tile);
      if (!need_unit(u)) break;
      teleport(u, to);
    }
  }
}

// cards/s203.py:14-30: the union over the friendly units of the enemy ANY (+ base) around them, in the iteration order
// of a CPython set of Points (pyset.h).  Out of line: its hash table is a local array and must not live in the
// registers of run().
MSB_HD MSB_NOINLINE PList s203_targets(int dpov) {
  PList fr = get_targets(dpov, mk_tgt(TK_UNIT, TS_FRIENDLY), PK_NONE);
  Tgt t = mk_tgt(TK_ANY, TS_ENEMY);
  t = tgt_base(t);
  uint8_t keys[24 * 10];
  int nk = 0;
  for (int i = 0; i < fr.n(); i++) {
    PList l = shape_targets(SH_SURROUNDING, fr.at(i), dpov, t, PK_NONE);
    for (int k = 0; k < l.n() && nk < (int)sizeof(keys); k++) {
      P p = l.at(k);
      keys[nk++] = (uint8_t)(p_valid(p) ? p_tile(p) : (p.y == 5 ? 20 : 21));
    }
  }
  uint8_t order[24];
  int m = pyset_list(keys, nk, order);
  PList out;
  out.clear();
  for (int i = 0; i < m; i++) {
    int id = order[i];
    out.push(id < 20 ? tile_p(id) : (id == 20 ? P{-1, 5} : P{-1, -1}));
  }
  return out;
}

// ------------------------------------------------------------------------------------------------------------------
// F_EACH: `for x in <list or count>: <nested call>; <something behind it>` of a card.  Frame {hdr: state, e (self),
// cur; w1: op | arg << 8 | i << 16 | n << 24 (list ops) or op | arg << 8 | remaining << 16 (count ops); six words:
// the list}.  state 0 = round i begins, 1 = its nested call has returned.
// ------------------------------------------------------------------------------------------------------------------
enum : int {
  EACH_DMG = 1,        // deal_damage(board.at(p), arg, source=self)                       u101 ud02 s013 s203 s302
  EACH_DMG_B004,       // the same, and destroy(self) behind the loop                       b004
  EACH_DMG_POISON,     // u = at(p); if u: u.deal_damage(5); u.poison()                     u401
  EACH_DMG_HEAL,       // dealt = at(p).deal_damage(3); self.heal(dealt)                    u405
  EACH_DMG_RAND,       // at(p).deal_damage(randint(4, 6))                                  s003
  EACH_DESTROY,        // at(p).destroy(source=self)                                        ue12
  EACH_COMMAND,        // at(p).command()                                                   ue21
  EACH_COMMAND_B203,   // deconfuse, then command                                           b203
  EACH_U018,           // arg unused; count: a random enemy (or its base) takes 2           u018
  EACH_UE01,           // arg = self.player; count: a random enemy unit takes 1             ue01
  EACH_U017,           // list = hand indices to play, arg = those already played, cur = self.player   u017
};
MSB_HD MSB_INL static bool each_counts(int op) { return op == EACH_U018 || op == EACH_UE01; }
MSB_HD MSB_INL void call_each(Wk& k, int op, int e, const PList& l, int n, int arg, int cur) {
  wk_push_list(k, l);
  wk_push(k, (uint32_t)op | ((uint32_t)(arg & 0xff) << 8) | (each_counts(op) ? (uint32_t)(n & 0xffff) << 16 : (uint32_t)(n & 0xff) << 24));
  wk_push(k, mk_hdr(F_EACH, 0, e, cur));
}
MSB_HD MSB_INL void h_each(Wk& k, const uint32_t hdr) {
  const int top = k.sp - 1;
  const int e = hdr_a(hdr);
  int cur = hdr_b(hdr);
  const uint32_t w1 = m.sk_ld(top - 1);
  const int op = (int)(w1 & 0xff);
  int arg = (int)((w1 >> 8) & 0xff);
  const bool counts = each_counts(op);
  int i = counts ? 0 : (int)((w1 >> 16) & 0xff);
  int n = counts ? (int)(w1 >> 16) : (int)(w1 >> 24);   // count ops: rounds left
  if (hdr_st(hdr) == 1) {   // behind the nested call of round i
    if (op == EACH_DMG_POISON) poison(cur);
    else if (op == EACH_DMG_HEAL) heal(e, (int)(int8_t)cur);
    if (fault()) return;
    if (counts) n--;
    else i++;
  }
  if (counts ? n <= 0 : i >= n) {
    k.sp = top - 7;
    if (op == EACH_DMG_B004) call_destroy(k, e, true);   // cards/b004.py:22
    return;
  }
  const PList l = wk_list(top - 2, n);
  bool skip = false;   // this round makes no call: straight on to the next one
  switch (op) {
    case EACH_DMG:
    case EACH_DMG_B004:
      call_damage(k, at(l.at(i)), arg, true);
      break;
    case EACH_DMG_POISON: {   // cards/u401.py:19-24
      const int u = at(l.at(i));
      if (u == AT_NONE) {
        skip = true;
      } else if (u >= AT_PLAYER) {
        set_fault(FAULT_UNSUPPORTED);   // the list holds units only
      } else {
        cur = u;
        call_damage(k, u, 5, true);
      }
    } break;
    case EACH_DMG_HEAL: {   // cards/u405.py:17-21
      const int who = at(l.at(i));
      if (who < 0 || who >= AT_PLAYER) {
        set_fault(who < 0 ? FAULT_PY_EXCEPTION : FAULT_UNSUPPORTED);
        break;
      }
      const int s = e_str(who);
      const int dealt = s - 3 < 0 ? s : 3;   // what Unit.deal_damage returns (unit.py:206-207)
      if (dealt < -128) set_fault(FAULT_UNSUPPORTED);
      cur = dealt & 0xff;
      call_damage(k, who, 3, true);
    } break;
    case EACH_DMG_RAND: {   // cards/s003.py:17-19
      const int t = at(l.at(i));
      if (t < 0) {
        set_fault(FAULT_PY_EXCEPTION);
        break;
      }
      const int dmg = rng_randint(4, 6);
      call_damage(k, t, dmg, true);
    } break;
    case EACH_DESTROY: {   // cards/ue12.py:17-19
      const int t = at(l.at(i));
      if (t < 0 || t >= AT_PLAYER) {
        set_fault(t < 0 ? FAULT_PY_EXCEPTION : FAULT_UNSUPPORTED);
        break;
      }
      call_destroy(k, t, true);
    } break;
    case EACH_COMMAND:   // cards/ue21.py:18-19
      call_command(k, at(l.at(i)));
      break;
    case EACH_COMMAND_B203: {   // cards/b203.py:17-21
      const int t = at(l.at(i));
      if (!deconfuse_if_confused(t)) break;
      if (fault()) break;
      call_command(k, t);
    } break;
    case EACH_U018: {   // cards/u018.py:22-25
      Tgt t = mk_tgt(TK_ANY, TS_ENEMY);
      t = tgt_base(t);
      const Pick q = targets_pick(cp(), t, PK_NONE);   // (the enemy base is always in it)
      call_damage(k, at(choice_tile(q)), 2, true);
    } break;
    case EACH_UE01: {   // cards/ue01.py:16-20
      const Pick q = targets_pick(arg, mk_tgt(TK_UNIT, TS_ENEMY), PK_NONE);
      if (q.n() > 0) call_damage(k, at(choice_tile(q)), 1, true);
      else skip = true;
    } break;
    case EACH_U017: {   // cards/u017.py:29-35
      const int me = cur;
      const int oi = l.get(i);
      int idx = oi;   // self.player.hand.index(card): spells compare by identity
      for (int q = 0; q < oi; q++)
        if (arg & (1 << q)) idx--;
      const CardInfo& ci = g_cards[hand_card(me, idx)];
      P pos{0, 0};
      bool has_pos = false;
      if (ci.tgt.has) {
        const Pick q = targets_pick(cp(), mk_tgt(ci.tgt), PK_NONE);
        if (q.n() == 0) {
          set_fault(FAULT_PY_EXCEPTION);   // random.choice([]) raises
          break;
        }
        pos = choice_tile(q);
        has_pos = true;
      }
      arg |= 1 << oi;
      call_player_play(k, me, idx, pos, has_pos);
    } break;
    default:
      set_fault(FAULT_UNSUPPORTED);
      break;
  }
  if (fault()) return;
  if (skip) {   // round i is over already
    if (counts) n--;
    else i++;
  }
  m.sk_st(top - 1, (uint32_t)op | ((uint32_t)(arg & 0xff) << 8) | (counts ? (uint32_t)(n & 0xffff) << 16 : ((uint32_t)(i & 0xff) << 16) | ((uint32_t)(n & 0xff) << 24)));
  m.sk_st(top, mk_hdr(F_EACH, skip ? 0 : 1, e, cur));
}

// F_AFTER: what a card does behind its one nested call.  Frame {hdr: op (as the state byte), e (self), t; w1: aux}.
enum : int {
  AFTER_U076 = 1,   // t = the target, aux = self.player: a dragon where the target died    cards/u076.py:22-25
  AFTER_U302,       // t = the target, aux = self.position (tile): push it if it survived   cards/u302.py:20-22
  AFTER_B305,       // aux = self.player: the returned card costs its original 3 again      cards/b305.py:33-36
};
MSB_HD MSB_INL void call_after(Wk& k, int op, int e, int t, int aux) {
  wk_push(k, (uint32_t)aux);
  wk_push(k, mk_hdr(F_AFTER, op, e, t));
}
MSB_HD MSB_INL void h_after(Wk& k, const uint32_t hdr) {
  const int top = k.sp - 1;
  const int op = hdr_st(hdr), t = hdr_b(hdr);
  const int aux = (int)m.sk_ld(top - 1);
  k.sp = top - 1;
  switch (op) {
    case AFTER_U076:
      if (e_str(t) <= 0) spawn_token_unit(aux, e_pos(t), 6, UT_DRAGON);
      break;
    case AFTER_U302:
      if (e_str(t) > 0) push_pull(t, tile_p(aux), true);
      break;
    case AFTER_B305: {
      const int dn = pl_deck_n(aux);
      if (dn == 0) {
        set_fault(FAULT_PY_EXCEPTION);   // deck[-1] on an empty list
        break;
      }
      m.st8(deck_ref(aux, dn - 1) + 1, 3);   // self.player.deck[-1].cost = self.original_cost
    } break;
    default:
      set_fault(FAULT_UNSUPPORTED);
      break;
  }
}

// One function per card.  ability_cases.inc holds the card bodies; the dummy switch makes a case-level `break` leave the card.
#define MSB_CARD_LOCALS                                                    \
    const int me = e_owner(e);                                             \
    const int dpov = cp();                                                 \
    const P mypos = e_pos(e);                                              \
    PList l;                                                               \
    (void)card; (void)me; (void)dpov; (void)mypos; (void)pos_pk; (void)src; (void)l;
#define MSB_SPELL_LOCALS                                                   \
    const int dpov = cp();                                                 \
    const P position = p_unpack(pos_pk);                                   \
    PList l;                                                               \
    (void)card; (void)me; (void)dpov; (void)position; (void)l;
#define MSB_CARD(id, ...)                                                  \
  MSB_HD MSB_A_CARD void ab_##id(int e, int pos_pk, bool src) {            \
    const int card = id;                                                   \
    MSB_CARD_LOCALS                                                        \
    switch (0) {                                                           \
      default: __VA_ARGS__                                                 \
    }                                                                      \
  }
#define MSB_CARD_K(id, ...)                                                \
  MSB_HD MSB_A_RARE int ab_##id(int sp_, int deep_, int e, int pos_pk, bool src) { \
    Wk k{sp_, 0, deep_, 0};                                                \
    const int card = id;                                                   \
    MSB_CARD_LOCALS                                                        \
    switch (0) {                                                           \
      default: __VA_ARGS__                                                 \
    }                                                                      \
    return k.sp;                                                           \
  }
#define MSB_SPELL(id, ...)                                                 \
  MSB_HD MSB_A_CARD void sp_##id(int me, int pos_pk) {                     \
    const int card = id;                                                   \
    MSB_SPELL_LOCALS                                                       \
    switch (0) {                                                           \
      default: __VA_ARGS__                                                 \
    }                                                                      \
  }
#define MSB_SPELL_K(id, ...)                                               \
  MSB_HD MSB_A_RARE int sp_##id(int sp_, int deep_, int me, int pos_pk) {  \
    Wk k{sp_, 0, deep_, 0};                                                \
    const int card = id;                                                   \
    MSB_SPELL_LOCALS                                                       \
    switch (0) {                                                           \
      default: __VA_ARGS__                                                 \
    }                                                                      \
    return k.sp;                                                           \
  }
// X.heal(amount); X.vitalize() on one entity (a card body is a macro argument and can hold no #if): on the image where
// MSB_WIDE_AB_ST is built (rules.h heal_vitalize), the two calls as the cards spell them where it is not
#if MSB_AB_ST
#define MSB_HEAL_VITALIZE(who, amount) heal_vitalize(who, amount, false)
#define MSB_HEAL_VITALIZE_CHECKED(who, amount) heal_vitalize(who, amount, true)
#else
#define MSB_HEAL_VITALIZE(who, amount) { int t = who; heal(t, amount); vitalize(t); }
#define MSB_HEAL_VITALIZE_CHECKED(who, amount) { int t = who; heal(t, amount); if (!fault()) vitalize(t); }
#endif
#include "ability_cases.inc"
#undef MSB_HEAL_VITALIZE
#undef MSB_HEAL_VITALIZE_CHECKED
#undef MSB_CARD
#undef MSB_CARD_K
#undef MSB_SPELL
#undef MSB_SPELL_K

// Dispatch.  On the device the lanes of a wave are grouped by card first (a "waterfall": take the first active
// lane's card as a wave-uniform value, serve the lanes holding it, repeat): the switch then runs on a scalar --
// scalar compares and branches, no nest of execution masks to keep alive across the card bodies.
MSB_HD MSB_INL void ability_entity_card(Wk& k, int card, int e, int pos_pk, bool src) {
  switch (card) {
#define MSB_CARD(id, ...) case id: ab_##id(e, pos_pk, src); break;
#define MSB_CARD_K(id, ...) case id: k.sp = ab_##id(k.sp, k.base - k.seg, e, pos_pk, src); break;
#define MSB_SPELL(id, ...)
#define MSB_SPELL_K(id, ...)
#include "ability_cases.inc"
#undef MSB_CARD
#undef MSB_CARD_K
#undef MSB_SPELL
#undef MSB_SPELL_K
    default:
      if (card_has_ability(card)) set_fault(FAULT_UNSUPPORTED);
      break;
  }
}
MSB_HD MSB_INL void ability_entity(Wk& k, int e, int pos_pk, bool src) {
  MSB_SCOPE(PS_ABILITY_ENTITY);
  const int card = e_card(e);
#if defined(__HIP_DEVICE_COMPILE__)
  int cv = card;
  asm volatile("" : "+v"(cv));   // an opaque copy: under `card == c0` the compiler would switch on the vector `card` again
  for (unsigned long long todo = __ballot(1); todo;) {   // wave-uniform loop: one round per distinct card
    const int leader = __builtin_ctzll(todo);
    const int c0 = __builtin_amdgcn_readlane(card, leader), c1 = __builtin_amdgcn_readlane(cv, leader);
    const bool mine = card == c0;
    todo &= ~__ballot(mine);
    if (mine) {
      int ev = e, pv = pos_pk;
      asm volatile("" : "+v"(ev), "+v"(pv));   // what a card derives from its arguments is computed under its own case
      ability_entity_card(k, c1, ev, pv, src);
    }
  }
#else
  ability_entity_card(k, card, e, pos_pk, src);
#endif
}

MSB_HD MSB_INL void ability_spell_card(Wk& k, int card, int me, int pos_pk) {
  switch (card) {
#define MSB_CARD(id, ...)
#define MSB_CARD_K(id, ...)
#define MSB_SPELL(id, ...) case id: sp_##id(me, pos_pk); break;
#define MSB_SPELL_K(id, ...) case id: k.sp = sp_##id(k.sp, k.base - k.seg, me, pos_pk); break;
#include "ability_cases.inc"
#undef MSB_CARD
#undef MSB_CARD_K
#undef MSB_SPELL
#undef MSB_SPELL_K
    default:
      set_fault(FAULT_UNSUPPORTED);
      break;
  }
}
MSB_HD MSB_INL void ability_spell(Wk& k, int card, int me, int pos_pk) {
  MSB_SCOPE(PS_ABILITY_SPELL);
#if defined(__HIP_DEVICE_COMPILE__)
  int cv = card;
  asm volatile("" : "+v"(cv));
  for (unsigned long long todo = __ballot(1); todo;) {
    const int leader = __builtin_ctzll(todo);
    const int c0 = __builtin_amdgcn_readlane(card, leader), c1 = __builtin_amdgcn_readlane(cv, leader);
    const bool mine = card == c0;
    todo &= ~__ballot(mine);
    if (mine) {
      int mv = me, pv = pos_pk;
      asm volatile("" : "+v"(mv), "+v"(pv));
      ability_spell_card(k, c1, mv, pv);
    }
  }
#else
  ability_spell_card(k, card, me, pos_pk);
#endif
}
