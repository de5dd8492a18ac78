// Card abilities as X-macro entries (included twice by abilities.inc: once to define one function per card, once to
// build the dispatching switch).  MSB_CARD: entity cards; `e` is the entity slot of `self`, `me` = self.player order,
// `dpov` = board.current_player, `mypos` = self.position, `l` a scratch list.  MSB_SPELL: spells; `me` = caster,
// `position` = target point.  A `break` at case level leaves the card.  The _K forms are the cards whose ability makes
// a nested call (damage, destroy, command, force_attack, play): they take the work stack `k` (abilities.inc).

MSB_CARD_K(C_B002, {  // cards/b002.py:13-21
      l = get_targets(dpov, mk_tgt(TK_ANY, TS_ENEMY), PK_NONE);
      if (l.n() > 0) {
        l = sorted_head(l, 0, true, 1);   // sort(key=(y, random()), reverse=True)[0]
        call_damage(k, at(l.at(0)), 8, true);
      }
    } break;
)
MSB_CARD_K(C_B004, {  // cards/b004.py:13-22
      Tgt t = mk_tgt(TK_ANY, TS_ENEMY);
      t = tgt_base(t);
      l = get_targets(dpov, t, PK_NONE);
      call_each(k, EACH_DMG_B004, e, l, l.n(), 4, 0);   // ... and destroy(self) behind the loop
    } break;
)
MSB_CARD(C_B005, {  // cards/b005.py:14-33 (extended record only)
      if (!REM_LISTS) {
        set_fault(FAULT_UNSUPPORTED);
        break;
      }
      l = sel_targets(SH_SURROUNDING, mypos, dpov, mk_tgt(TK_ANY, TS_FRIENDLY));
      int mine = m.ld8(E_REM + e);
      if (mine == REM_LOST) {
        set_fault(FAULT_CAP_REM);   // this copy's memory could not be kept when it was made (state.h)
        break;
      }
      if (mine == REM_NONE || rem_n(mine) == 0) {
        // self.ability_remembered == []: remember copies of the surrounding friendly entities (Card.copy: a deepcopy
        // that reaches the whole game through entity.player -- rules.h rem_copy_entity / world_snapshot)
        if (l.n() == 0) break;   // stays [] -> "remember" again next time
        int list = rem_alloc();
        if (fault()) break;
        int n = 0;
        for (int i = 0; i < l.n() && !fault(); i++) {
          int t = at(l.at(i));
          if (t < 0 || t >= AT_PLAYER) {
#if defined(MSB_FAULT_TRACE) && !defined(__HIPCC__)
            fprintf(stderr, "b005 remember: i=%d n=%d tile=(%d,%d) t=%d ctx=%d\n", i, l.n(), l.at(i).x, l.at(i).y, t, ctx());
#endif
            set_fault(FAULT_PY_EXCEPTION);
            break;
          }
          int c = rem_copy_entity(t);
          if (fault()) break;
          m.st8(rem_off(list) + 4 + n, c);
          n++;
        }
        m.st8(rem_off(list), n);
        m.st8(E_REM + e, list);
      } else {
        int n = rem_n(mine);
        int count = 0;
        for (int i = 0; i < n && !fault(); i++) {
          int r = rem_get(mine, i);
          P pos = e_pos(r);
          int cur = at(pos);
          bool ok = cur == AT_NONE;
          if (!ok && cur < AT_PLAYER) {
            // board.at(entity.position) == entity: same class family, card_id, player, position (unit.py:25-26,
            // structure.py:18-19); the position compared is the one the OBJECT on that tile records
            ok = e_is_unit(cur) == e_is_unit(r) && e_card(cur) == e_card(r) && e_owner(cur) == e_owner(r) &&
                 m.ld8g(eg(cur), EO_POS) == m.ld8g(eg(r), EO_POS);
          }
          if (ok) {
            board_set(pos, r);   // the remembered OBJECT itself enters the board (with its own memory and world)
            if (++count >= 3) break;
          }
        }
        m.st8(E_REM + e, REM_NONE);   // self.ability_remembered = []  (the list is collected at the next step)
      }
    } break;
)
MSB_CARD_K(C_B006, {  // cards/b006.py:14-38
      l = get_targets(dpov, mk_tgt(TK_UNIT, TS_FRIENDLY), PK_NONE);
      PList nv;
      nv.clear();
      for (int i = 0; i < l.n(); i++)
        if (e_st(at(l.at(i)), ST_VITALIZED) == 0) nv.push_raw(l.get(i));
      nv = shuffle(nv);
      for (int i = 0; i < nv.n() && i < 3 && !fault(); i++) vitalize(at(nv.at(i)));
      if (fault()) break;
      PList tiles;
      tiles.clear();
      l = shape_tiles(SH_FRONT, mypos, dpov);
      // Player.is_within_front_line (player.py:96-100) compares by the player's ORDER
      if (l.n() > 0 && at(l.at(0)) == AT_NONE && (me == 0 ? l.at(0).y >= pl_front(me) : l.at(0).y <= pl_front(me)))
        tiles.push(l.at(0));
      l = shape_tiles(SH_BEHIND, mypos, dpov);
      if (l.n() > 0 && at(l.at(0)) == AT_NONE) tiles.push(l.at(0));
      if (tiles.n() > 0) {
        // copy = self.copy(); copy.strength = 1; copy.play(choice(tiles))
        int c = new_entity(card, me, 1, 0, false);
        if (fault()) break;
        if (e_flags(e) & EF_SINGLE_USE) e_set_flag(c, EF_SINGLE_USE, true);
        call_structure_play(k, c, choice_point(tiles));
      }
    } break;
)
MSB_CARD_K(C_B305, {  // cards/b305.py:15-45
      l = get_targets(dpov, mk_tgt(TK_STRUCTURE, TS_FRIENDLY), PK_NONE);
      for (int i = 0; i < l.n(); i++)
        if (l.get(i) == p_pack(mypos)) {
          l.remove_at(i);
          break;
        }
      bool moved = false;
      for (int i = 0; i < l.n() && i < 8 && !fault(); i++) {
        P tp = l.at(i);
        int other = at(tp);
        if (other < 0) {
          set_fault(FAULT_PY_EXCEPTION);
          break;
        }
        if (e_card(other) != C_B305) continue;
        b305_relocate(tp, mypos, dpov);
        if (fault()) break;
        int victim = at(tp);
        if (victim < 0) {
          set_fault(FAULT_PY_EXCEPTION);
          break;
        }
        call_after(k, AFTER_B305, e, 0, me);   // behind the destroy: self.player.deck[-1].cost = self.original_cost
        call_destroy(k, victim, true);
        moved = true;
        break;
      }
      if (moved || fault()) break;
      if (!(e_flags(e) & EF_SINGLE_USE)) {
        int dn = pl_deck_n(me);
        if (dn == 0) {
          set_fault(FAULT_PY_EXCEPTION);   // pop from empty list
          break;
        }
        m.st8(pl(me, P_DECK_N), dn - 1);
      }
      // self.cost = 2; self.weight = 1; self.player.hand.append(self): the board object joins the hand
      push_new_instance(me, true, C_B305, 2, CF_ALIAS | ((e_flags(e) & EF_SINGLE_USE) ? CF_SINGLE_USE : 0), e);
      m.st8(H_OBSFAULT, m.ld8(H_OBSFAULT) | GF_ALIAS);
    } break;
)
MSB_CARD(C_B007, {  // cards/b007.py:12-18
      int opp = opponent_of(me);
      if (pl_base(me) == pl_base(opp)) break;
      int stronger = pl_base(me) > pl_base(opp) ? me : opp;
      player_deal_damage(stronger, 2);
      player_heal(opponent_of(stronger), 2);
    } break;
)
MSB_CARD_K(C_B008, {  // cards/b008.py:14-25
      if (pl_hand_n(me) > 0 && card_is_unit(hand_card(me, 0))) {
        int o = hand_ref(me, 0) + 2;
        m.st8(o, m.ld8(o) ^ CF_FF);
      }
      Tgt t = mk_tgt(TK_UNIT, TS_ANY);
      t = tgt_status(t, 1 << ST_CONFUSED);
      l = get_targets(dpov, t, PK_NONE);
      if (l.n() > 0) {
        l = sorted_head(l, 1, false, 1);  // sort(key=(strength, random()))[0]
        call_destroy(k, at(l.at(0)), true);
      }
    } break;
)
MSB_CARD(C_B009, {  // cards/b009.py:13-25
      l = get_targets(dpov, mk_tgt(TK_UNIT, TS_ENEMY), PK_NONE);
      if (l.n() > 0) {
        l = sorted_head(l, 0, true, 2);   // sort(key=(y, random()), reverse=True)[:2]
        l = shuffle(l);
        for (int i = 0; i < l.n() && !fault(); i++) confuse(at(l.at(i)));
      }
    } break;
)
MSB_CARD(C_B104, {  // cards/b104.py:12-20
      l = get_targets(dpov, mk_tgt(TK_UNIT, TS_ENEMY), PK_NONE);
      if (l.n() > 0) {
        l = sorted_head(l, 0, true, 1);
        freeze(at(l.at(0)));
      }
    } break;
)
MSB_CARD_K(C_B203, {  // cards/b203.py:12-21
      l = sel_targets(SH_FRONT, mypos, me, mk_tgt(TK_UNIT, TS_FRIENDLY));
      call_each(k, EACH_COMMAND_B203, e, l, l.n(), 0, 0);
    } break;
)
MSB_CARD_K(C_B304,  // cards/b304.py:12-13
      call_entity_damage(k, e, 3, false, true);
      break;
    // ------------------------------------------------------------------ units
)
MSB_CARD(C_U007, {  // cards/u007.py:13-22
      const Pick q = shape_pick(SH_SURROUNDING, mypos, me, mk_tgt(TK_UNIT, TS_ENEMY));
      if (q.n() > 0) MSB_HEAL_VITALIZE(at(choice_tile(q)), 5);
    } break;
)
MSB_CARD_K(C_U017, {  // cards/u017.py:18-35: play up to 8 mana of spells from hand, free, in shuffled order
      int hn = pl_hand_n(me);
      PList orig;   // hand indices of the eligible spells (reusing the packed list type)
      orig.clear();
      for (int i = 0; i < hn; i++) {
        int c = hand_card(me, i);
        if (c < NUM_CARDS && g_cards[c].kind == KIND_SPELL && hand_cost(me, i) <= 8) orig.push_raw(i);
      }
      int nc = orig.n();
      if (nc == 0) break;
      orig = shuffle(orig);   // random.shuffle(cards)
      int remaining = 8;
      PList pick;
      pick.clear();
      for (int i = 0; i < nc; i++) {
        int cost = hand_cost(me, orig.get(i));
        if (cost <= remaining) {
          pick.push_raw(orig.get(i));
          remaining -= cost;
        }
      }
      call_each(k, EACH_U017, e, pick, pick.n(), 0, me);   // for card in pick: self.player.play(hand.index(card), target)
    } break;
)
MSB_CARD_K(C_U018, {  // cards/u018.py:13-25
      l = sel_targets(SH_SURROUNDING, mypos, dpov, mk_tgt(TK_UNIT, TS_ANY));
      int types = 0, cnt = 0;
      for (int i = 0; i < l.n(); i++) {
        int b = 1 << card_first_type(e_card(at(l.at(i))));
        if (!(types & b)) {
          types |= b;
          cnt++;
        }
      }
      call_each(k, EACH_U018, e, l, cnt, 0, 0);   // cnt times: a random enemy, or its base, takes 2
    } break;
)
MSB_CARD(C_U021, {  // cards/u021.py:13-20
      const Pick q = targets_pick(dpov, mk_tgt(TK_UNIT, TS_FRIENDLY), p_pack(mypos));
      if (q.n() > 0) heal(at(choice_tile(q)), 5);
    } break;
)
MSB_CARD_K(C_U026, {  // cards/u026.py:13-17
      l = sel_targets(SH_BEHIND, mypos, dpov, mk_tgt(TK_ANY, TS_ENEMY));
      if (l.n() > 0) call_damage(k, at(l.at(0)), 6, true);
    } break;
)
MSB_CARD(C_U036,  // cards/u036.py:12-14
      if (pl_hand_n(me) == 0) heal(at(mypos), 12);
      break;
)
MSB_CARD(C_U040, {  // cards/u040.py:13-22
      if (src) {
        l = shape_tiles(SH_SURROUNDING, mypos, me);
        if (l.n() > 0) respawn(e, choice_point(l), 12);
      }
    } break;
)
MSB_CARD(C_U050,  // cards/u050.py:13-15
      if (mypos.y == 4) gain_speed(e, 3);
      break;
)
MSB_CARD(C_U051, {  // cards/u051.py:14-21
      if (!sel_any(SH_BORDERING, mypos, dpov, mk_tgt(TK_UNIT, TS_ANY)))
        gain_speed(e, 1);
      else
        heal(e, 2);
    } break;
)
MSB_CARD(C_U053, {  // cards/u053.py:14-24
      if (!sel_any(SH_SURROUNDING, mypos, dpov, mk_tgt(TK_UNIT, TS_ANY))) {
        gain_speed(e, 2);
      } else {
        if (!sel_any(SH_BORDERING, mypos, dpov, mk_tgt(TK_UNIT, TS_ANY))) gain_speed(e, 1);
      }
    } break;
)
MSB_CARD(C_U055, {  // cards/u055.py:12-19
      Tgt t = mk_tgt(TK_UNIT, TS_ENEMY);
      t = tgt_xstatus(t, 1 << ST_CONFUSED);
      l = sel_targets(SH_FRONT, mypos, dpov, t);
      for (int i = 0; i < l.n() && !fault(); i++) confuse(at(l.at(i)));
    } break;
)
MSB_CARD(C_U061, {  // cards/u061.py:12-22
      confuse(e);
      const Pick q = targets_pick(dpov, mk_tgt(TK_UNIT, TS_FRIENDLY), p_pack(mypos));
      if (q.n() > 0) confuse(at(choice_tile(q)));
      gain_speed(e, 2);
    } break;
)
MSB_CARD(C_U071, {  // cards/u071.py:12-24
      l = sel_targets(SH_BORDERING, mypos, me, mk_tgt(TK_UNIT, TS_ENEMY));
      PList nc;
      nc.clear();
      for (int i = 0; i < l.n(); i++)
        if (!e_confused(at(l.at(i)))) nc.push_raw(l.get(i));
      if (nc.n() > 0) {
        confuse(at(choice_point(nc)));
        l = shape_tiles(SH_FRONT, mypos, dpov);
        if (l.n() > 0 && at(l.at(0)) == AT_NONE) teleport(e, l.at(0));
      }
    } break;
)
MSB_CARD_K(C_U074, {  // cards/u074.py:12-19
      l = sel_targets(SH_FRONT, mypos, me, mk_tgt(TK_UNIT, TS_ENEMY));
      if (l.n() > 0) call_force_attack(k, e, l.at(0));
    } break;
)
MSB_CARD_K(C_U076, {  // cards/u076.py:14-25
      Tgt t = mk_tgt(TK_UNIT, TS_ANY);
      t = tgt_xtypes(t, 1 << UT_DRAGON);
      const Pick q = shape_pick(SH_SURROUNDING, mypos, dpov, t);
      if (q.n() > 0) {
        int target = at(choice_tile(q));
        call_after(k, AFTER_U076, e, target, me);   // behind the damage: a dragon where the target died
        call_damage(k, target, 6, true);
      }
    } break;
)
MSB_CARD_K(C_U101, {  // cards/u101.py:13-26
      P position = p_unpack(pos_pk);
      int t = at(position);
      if (p_is_base(position) || t < 0 || t >= AT_PLAYER || !e_is_unit(t) || !e_frozen(t)) break;
      Tgt tg = mk_tgt(TK_UNIT, TS_ENEMY);
      tg = tgt_status(tg, 1 << ST_FROZEN);
      l = sel_targets(SH_SURROUNDING, mypos, me, tg);
      call_each(k, EACH_DMG, e, l, l.n(), 8, 0);
    } break;
)
MSB_CARD(C_U103, {  // cards/u103.py:12-19
      l = sel_targets(SH_BORDERING, mypos, dpov, mk_tgt(TK_UNIT, TS_ENEMY));
      for (int i = 0; i < l.n() && !fault(); i++) freeze(at(l.at(i)));
    } break;
)
MSB_CARD(C_U106, {  // cards/u106.py:13-18
      if (sel_any(SH_BORDERING, mypos, dpov, mk_tgt(TK_STRUCTURE, TS_FRIENDLY)) || mypos.y == 4) heal(e, 7);
    } break;
)
MSB_CARD(C_U111, {  // cards/u111.py:13-21
      for (int k = 0; k < 10 && !fault(); k++) {
        const Pick q = shape_pick(SH_SURROUNDING, mypos, me, mk_tgt(TK_UNIT, TS_FRIENDLY));
        if (q.n() > 0) heal(at(choice_tile(q)), 1);
      }
    } break;
)
MSB_CARD(C_U117,  // cards/u117.py:11-12
      freeze(e);
      break;
)
MSB_CARD(C_U206,  // cards/u206.py:12-13
      player_deal_damage(me, 3);
      break;
)
MSB_CARD(C_U211, {  // cards/u211.py:14-19
      l = shape_tiles(SH_FRONT, mypos, dpov);
      if (l.n() > 0 && at(l.at(0)) == AT_NONE) {
        int s = rng_randint(1, 3);
        spawn_token_unit(me, l.at(0), s, UT_SATYR);
      }
    } break;
)
MSB_CARD(C_U216,  // cards/u216.py:12-13
      player_deal_damage(me, 2);
      break;
)
MSB_CARD(C_U217, {  // cards/u217.py:13-17
      l = empty_shape_tiles(SH_ROW, P{0, 4}, dpov);
      if (l.n() > 0) spawn_token_unit(me, choice_point(l), 5, UT_SATYR);
    } break;
)
MSB_CARD_K(C_U302, {  // cards/u302.py:12-22
      P position = p_unpack(pos_pk);
      int t = at(position);
      if (p_is_base(position) || t < 0 || t >= AT_PLAYER || !e_is_unit(t)) break;
      if (e_str(t) > e_str(e)) {
        call_after(k, AFTER_U302, e, t, p_tile(mypos));   // behind the damage: push the survivor
        call_entity_damage(k, t, 7, false, true);
      }
    } break;
)
MSB_CARD(C_U305, {  // cards/u305.py:13-21
      Tgt t = mk_tgt(TK_UNIT, TS_FRIENDLY);
      t = tgt_types(t, 1 << UT_CONSTRUCT);
      const Pick q = shape_pick(SH_BORDERING, mypos, dpov, t);
      if (q.n() > 0) {
        heal(at(choice_tile(q)), 4);
        heal(e, 4);
      }
    } break;
)
MSB_CARD_K(C_U306, {  // cards/u306.py:13-20
      const Pick q = targets_pick(dpov, mk_tgt(TK_ANY, TS_FRIENDLY), p_pack(mypos));
      if (q.n() > 0) call_damage(k, at(choice_tile(q)), 1, true);
    } break;
)
MSB_CARD(C_U310, {  // cards/u310.py:13-40  (raises UnboundLocalError when nothing is pushable)
      l = sel_targets(SH_BORDERING, mypos, dpov, mk_tgt(TK_UNIT, TS_ENEMY));
      int behind = -1, right = -1, left = -1, front = -1;
      for (int i = 0; i < l.n(); i++) {
        P t = l.at(i);
        if (behind < 0 && mypos.y + 1 == t.y) behind = i;
        if (right < 0 && mypos.x + 1 == t.x) right = i;
        if (left < 0 && mypos.x - 1 == t.x) left = i;
        if (front < 0 && mypos.y - 1 == t.y) front = i;
      }
      int target = -1;
      if (behind >= 0 && l.at(behind).y < 4 && at(P{l.at(behind).x, l.at(behind).y + 1}) == AT_NONE)
        target = behind;
      else if (left >= 0 && l.at(left).x > 0 && at(P{l.at(left).x - 1, l.at(left).y}) == AT_NONE)
        target = left;
      else if (right >= 0 && l.at(right).x < 3 && at(P{l.at(right).x + 1, l.at(right).y}) == AT_NONE)
        target = right;
      else if (front >= 0 && l.at(front).y > 0 && at(P{l.at(front).x, l.at(front).y - 1}) == AT_NONE)
        target = front;
      if (target < 0) {
        set_fault(FAULT_PY_EXCEPTION);
        break;
      }
      push_pull(at(l.at(target)), mypos, true);
    } break;
)
MSB_CARD(C_U313, {  // cards/u313.py:13-22
      const Pick q = shape_pick(SH_SURROUNDING, mypos, dpov, mk_tgt(TK_UNIT, TS_FRIENDLY));
      if (q.n() > 0) heal(at(choice_tile(q)), 5);
      heal(e, 5);
    } break;
)
MSB_CARD(C_U314, {  // cards/u314.py:12-19
      l = sel_targets(SH_FRONT, mypos, dpov, mk_tgt(TK_UNIT, TS_FRIENDLY));
      if (l.n() > 0) push_pull(at(l.at(0)), mypos, true);
    } break;
)
MSB_CARD(C_U316, {  // cards/u316.py:13-25
      l = sel_targets(SH_SURROUNDING, mypos, dpov, mk_tgt(TK_UNIT, TS_FRIENDLY));
      if (l.n() > 0) {
        l = shuffle(l);
        for (int i = 0; i < l.n() && i < 2 && !fault(); i++) vitalize(at(l.at(i)));
      }
      vitalize(e);
    } break;
)
MSB_CARD(C_U320, {  // cards/u320.py:13-20
      const Pick q = shape_pick(SH_SURROUNDING, mypos, me, mk_tgt(TK_UNIT, TS_FRIENDLY));
      if (q.n() > 0) heal(at(choice_tile(q)), 4);
    } break;
)
MSB_CARD_K(C_U401, {  // cards/u401.py:13-24
      l = sel_targets(SH_BORDERING, mypos, dpov, mk_tgt(TK_UNIT, TS_ANY));
      call_each(k, EACH_DMG_POISON, e, l, l.n(), 5, 0);
    } break;
)
MSB_CARD(C_U403, {  // cards/u403.py:14-25
      Tgt t = mk_tgt(TK_UNIT, TS_ANY);
      t = tgt_status(t, 1 << ST_POISONED);
      l = sel_targets(SH_SURROUNDING, mypos, dpov, t);
      for (int i = 0; i < l.n() && !fault(); i++) {
        PList tiles;
        tiles = empty_shape_tiles(SH_BORDERING, l.at(i), dpov);
        tiles = shuffle(tiles);
        for (int k = 0; k < tiles.n() && k < 4 && !fault(); k++) spawn_token_unit(me, tiles.at(k), 1, UT_TOAD);
      }
    } break;
)
MSB_CARD_K(C_U405, {  // cards/u405.py:13-21
      l = sel_targets(SH_BORDERING, mypos, dpov, mk_tgt(TK_UNIT, TS_ANY));
      call_each(k, EACH_DMG_HEAL, e, l, l.n(), 3, 0);
    } break;
)
MSB_CARD(C_U406, {  // cards/u406.py:13-20
      l = empty_shape_tiles(SH_BORDERING, mypos, dpov);
      if (l.n() > 0) {
        P tile = choice_point(l);
        spawn_token_unit(opponent_of(me), tile, 1, UT_RAVEN);
      }
    } break;
)
MSB_CARD(C_U411, {  // cards/u411.py:13-23
      l = get_targets(dpov, mk_tgt(TK_UNIT, TS_ENEMY), PK_NONE);
      if (l.n() > 0) {
        l = shuffle(l);
        for (int i = 0; i < l.n() && i < 3 && !fault(); i++) poison(at(l.at(i)));
      }
    } break;
)
MSB_CARD(C_UA03, {  // cards/ua03.py:12-16
      l = empty_shape_tiles(SH_ROW, mypos, dpov);
      l.push(mypos);
      teleport(e, choice_point(l));
    } break;
)
MSB_CARD_K(C_UA04, {  // cards/ua04.py:12-32
      PList lu, ru;
      lu = get_targets(dpov, mk_tgt(TK_UNIT, TS_FRIENDLY), PK_NONE);
      ru = get_targets(dpov, mk_tgt(TK_UNIT, TS_ENEMY), PK_NONE);
      if (lu.n() != ru.n()) {
        PList side = lu.n() > ru.n() ? lu : ru;
        int mn = 32767;
        for (int i = 0; i < side.n(); i++) {
          int s = e_str(at(side.at(i)));
          if (s < mn) mn = s;
        }
        l.clear();
        for (int i = 0; i < side.n(); i++)
          if (e_str(at(side.at(i))) == mn) l.push_raw(side.get(i));
        if (l.n() > 0) call_destroy(k, at(choice_point(l)), true);
      }
    } break;
)
MSB_CARD(C_UA05, {  // cards/ua05.py:13-19
      l = empty_shape_tiles(SH_SIDE, mypos, dpov);
      for (int i = 0; i < l.n() && !fault(); i++) spawn_token_unit(me, l.at(i), 4, UT_ANCIENT);
    } break;
)
MSB_CARD(C_UA07, {  // cards/ua07.py:11-22
      switch (rng_randint(0, 5)) {
        case 0: freeze(e); break;
        case 1: poison(e); break;
        case 2: vitalize(e); break;
        case 3: confuse(e); break;
        case 4: disable(e); break;
      }
    } break;
)
MSB_CARD(C_UA20, {  // cards/ua20.py:21-32 (needs the extended record's deck capacity)
      if (!sel_any(SH_FRONT, mypos, me, mk_tgt(TK_UNIT, TS_ENEMY))) {
        const int cand[4] = {C_B005, C_B006, C_B203, C_B305};
        int c = cand[rng_randint(0, 4)];
        // copy(); cost = 0; weight = 1; is_single_use = True; deck.append(card)
        // (inside a frozen world the deck is the snapshot's, which nothing ever reads again: only the draw counts)
        if (ctx() == 0) push_new_instance(me, false, c, 0, CF_SINGLE_USE | CF_XBASE, g_cards[c].strength);
      }
    } break;
)
MSB_CARD(C_UD01, {  // cards/ud01.py:13-20
      Tgt t = mk_tgt(TK_UNIT, TS_FRIENDLY);
      t = tgt_types(t, 1 << UT_DRAGON);
      const Pick q = targets_pick(me, t, PK_NONE);
      if (q.n() > 0) heal(at(choice_tile(q)), 7);
    } break;
)
MSB_CARD_K(C_UD02, {  // cards/ud02.py:13-20
      Tgt t = mk_tgt(TK_UNIT, TS_ANY);
      t = tgt_xtypes(t, 1 << UT_DRAGON);
      l = sel_targets(SH_FRONT, mypos, dpov, t);
      call_each(k, EACH_DMG, e, l, l.n(), 4, 0);
    } break;
)
MSB_CARD(C_UD31, {  // cards/ud31.py:13-25
      P position = p_unpack(pos_pk);
      int t = at(position);
      if (p_is_base(position) || t < 0 || t >= AT_PLAYER || !e_is_unit(t)) break;
      Tgt tg = mk_tgt(TK_UNIT, TS_FRIENDLY);
      tg = tgt_types(tg, 1 << UT_DRAGON);
      const Pick q = shape_pick(SH_SURROUNDING, mypos, me, tg);
      if (q.n() > 0) heal(at(choice_tile(q)), 2);
      heal(e, 2);
    } break;
)
MSB_CARD_K(C_UE01, {  // cards/ue01.py:12-20
      int n = e_dmg(e);
      if (n > 0xffff) set_fault(FAULT_UNSUPPORTED);
      l.clear();
      if (n > 0 && n <= 0xffff) call_each(k, EACH_UE01, e, l, n, me, 0);   // n times: a random enemy unit, if there is one, takes 1
    } break;
)
MSB_CARD(C_UE03, {  // cards/ue03.py:12-18
      l = empty_shape_tiles(SH_BORDERING, mypos, dpov);
      if (l.n() > 0) {
        P tile = choice_point(l);
        spawn_token_unit(me, tile, e_str(e), UT_ELDER);
      }
    } break;
)
MSB_CARD(C_UE04, {  // cards/ue04.py:13-18
      l = get_targets(me, mk_tgt(TK_UNIT, TS_ENEMY), PK_NONE);
      int cnt = 0;
      for (int i = 0; i < l.n(); i++)
        if (e_str(at(l.at(i))) > e_str(e)) cnt++;
      heal(e, cnt * 4);
    } break;
)
MSB_CARD(C_UE05, {  // cards/ue05.py:13-20
      Tgt t = mk_tgt(TK_UNIT, TS_FRIENDLY);
      t = tgt_limit(t, e_str(e) - 1);
      l = get_targets(me, t, p_pack(mypos));
      for (int i = 0; i < l.n() && i < 4; i++) e_set_str(at(l.at(i)), e_str(e));
    } break;
)
MSB_CARD(C_UE11,  // cards/ue11.py:12-13
      heal(e, 6);
      break;
)
MSB_CARD_K(C_UE12, {  // cards/ue12.py:12-19
      l = sel_targets(SH_FRONT, mypos, me, mk_tgt(TK_UNIT, TS_ENEMY));
      call_each(k, EACH_DESTROY, e, l, l.n(), 0, 0);
    } break;
)
MSB_CARD_K(C_UE21, {  // cards/ue21.py:12-19
      Tgt t = mk_tgt(TK_UNIT, TS_FRIENDLY);
      t = tgt_limit(t, e_str(e));
      l = get_targets(me, t, p_pack(mypos));
      call_each(k, EACH_COMMAND, e, l, l.n(), 0, 0);
    } break;
)
MSB_CARD(C_UE22, {  // cards/ue22.py:13-23
      l = get_targets(me, mk_tgt(TK_UNIT, TS_FRIENDLY), p_pack(mypos));
      if (l.n() > 0) {
        l = shuffle(l);
        for (int i = 0; i < l.n() && i < 2 && !fault(); i++) heal(at(l.at(i)), e_dmg(e));
      }
    } break;
)
MSB_CARD(C_UE31,  // cards/ue31.py:12-13
      e_set_str(e, 6);
      break;
)
MSB_CARD_K(C_UE32, {  // cards/ue32.py:13-23
      int damage = e_str(e) < 6 ? e_str(e) : 6;
      l = sel_targets(SH_FRONT, mypos, me, mk_tgt(TK_ANY, TS_ENEMY));
      if (l.n() > 0)
        call_damage(k, at(l.at(0)), damage, true);
      else
        player_deal_damage(opponent_of(me), damage);
    } break;
)
MSB_CARD(C_UE41,  // cards/ue41.py:11-12
      convert(e);
      break;
)
MSB_CARD(C_UE42, {  // cards/ue42.py:12-15
      int amount = e_dmg(e) < 2 ? e_dmg(e) : 2;
      int dealt = player_deal_damage(opponent_of(me), amount);
      heal(e, dealt);
    } break;
)
MSB_CARD(C_UP02, {  // cards/up02.py:13-22
      l = get_targets(dpov, mk_tgt(TK_UNIT, TS_FRIENDLY), PK_NONE);
      int types = 0;
      for (int i = 0; i < l.n(); i++) types |= card_types(e_card(at(l.at(i))));
      heal(e, 2 * __builtin_popcount(types));
    } break;
)
MSB_CARD(C_UP03, {  // cards/up03.py:13-28
      l = get_targets(dpov, mk_tgt(TK_UNIT, TS_FRIENDLY), PK_NONE);
      int types = 0;
      for (int i = 0; i < l.n(); i++) types |= card_types(e_card(at(l.at(i))));
      int amount = 3 * __builtin_popcount(types);
      l = sel_targets(SH_SURROUNDING, mypos, dpov, mk_tgt(TK_UNIT, TS_ENEMY));
      for (int i = 0; i < l.n(); i++) {  // Unit.reduce, unit.py:233-234
        int t = at(l.at(i));
        int s = e_str(t) - amount;
        e_set_str(t, s > 1 ? s : 1);
      }
    } break;
)

MSB_SPELL_K(C_S001,  // cards/s001.py:13-14
      call_damage(k, at(position), 9, true);
      break;
)
MSB_SPELL_K(C_S003, {  // cards/s003.py:14-19
      l = get_targets(dpov, mk_tgt(TK_ANY, TS_ENEMY), PK_NONE);
      call_each(k, EACH_DMG_RAND, 0xff, l, l.n(), 0, 0);   // each takes randint(4, 6), drawn when its turn comes
    } break;
)
MSB_SPELL(C_S004, {  // cards/s004.py:14-23
      l = empty_within_front_line(me);
      if (l.n() > 0) {
        l = shuffle(l);
        int amount = rng_randint(6, 7);
        for (int i = 0; i < l.n() && i < amount && !fault(); i++) spawn_token_unit(me, l.at(i), 1, UT_TOAD);
      }
    } break;
)
MSB_SPELL(C_S007, {  // cards/s007.py:13-16
      MSB_HEAL_VITALIZE_CHECKED(at(position), 7);
    } break;
)
MSB_SPELL(C_S012, {  // cards/s012.py:13-18
      const Pick q = empty_front_pick(me);
      if (q.n() > 0) spawn_token_unit(me, choice_tile(q), 5, UT_KNIGHT);
    } break;
)
MSB_SPELL_K(C_S013, {  // cards/s013.py:13-26
      PList picked;
      picked.clear();
      for (int ut = 0; ut < 16; ut++) {
        Tgt t = mk_tgt(TK_UNIT, TS_ANY);
        t = tgt_types(t, 1 << ut);
        l = get_targets(dpov, t, PK_NONE);
        PList units;
        units.clear();
        for (int i = 0; i < l.n(); i++)
          if (!picked.has(l.at(i))) units.push_raw(l.get(i));
        if (units.n() > 0) picked.push(choice_point(units));
      }
      call_each(k, EACH_DMG, 0xff, picked, picked.n(), 6, 0);
    } break;
)
MSB_SPELL(C_S021, {  // cards/s021.py:13-24
      confuse(at(position));
      if (fault()) break;
      Tgt t = mk_tgt(TK_UNIT, TS_FRIENDLY);
      t = tgt_types(t, 1 << UT_FELINE);
      l = get_targets(dpov, t, PK_NONE);
      if (l.n() > 0) {
        int mn = 32767;
        for (int i = 0; i < l.n(); i++) {
          int s = e_str(at(l.at(i)));
          if (s < mn) mn = s;
        }
        PList w;
        w.clear();
        for (int i = 0; i < l.n(); i++)
          if (e_str(at(l.at(i))) == mn) w.push_raw(l.get(i));
        heal(at(choice_point(w)), 5);
      }
    } break;
)
MSB_SPELL(C_S101, {  // cards/s101.py:14-22 (IndexError without a friendly unit)
      set_pl_mana(me, pl_mana(me) + 13);
      l = get_targets(dpov, mk_tgt(TK_UNIT, TS_FRIENDLY), PK_NONE);
      l = sorted_head(l, 1, false, 1);    // sort(key=(strength, random()))[0]; random() once per element
      if (l.n() == 0) {
        set_fault(FAULT_PY_EXCEPTION);
        break;
      }
      heal(at(l.at(0)), 6);
    } break;
)
MSB_SPELL_K(C_S104, {  // cards/s104.py:13-19
      int t = at(position);
      if (!need_unit(t)) break;
      if (e_frozen(t))
        call_entity_damage(k, t, 12, false, true);
      else
        freeze(t);
    } break;
)
MSB_SPELL(C_S105,  // cards/s105.py:13-14
      heal(at(position), 15);
      break;
)
MSB_SPELL_K(C_S203, {  // cards/s203.py:14-30
      l = s203_targets(dpov);
      call_each(k, EACH_DMG, 0xff, l, l.n(), 6, 0);
    } break;
)
MSB_SPELL_K(C_S302, {  // cards/s302.py:14-22
      Tgt t = mk_tgt(TK_ANY, TS_ENEMY);
      t = tgt_base(t);
      l = get_targets(dpov, t, PK_NONE);
      l = shuffle(l);
      call_each(k, EACH_DMG, 0xff, l, l.n() < 4 ? l.n() : 4, 4, 0);
    } break;
)
MSB_SPELL(C_S403, {  // cards/s403.py:13-22
      Tgt t = mk_tgt(TK_UNIT, TS_FRIENDLY);
      t = tgt_status(t, 1 << ST_POISONED);
      l = get_targets(dpov, t, PK_NONE);
      for (int i = 0; i < l.n() && !fault(); i++) {
        MSB_HEAL_VITALIZE_CHECKED(at(l.at(i)), 5);
      }
    } break;
)
