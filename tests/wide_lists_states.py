"""Described states for tests/test_wide_lists_gpu.py: what 64 N12M games do not give the whole-word forms of rules.h
(discard_wide, draw_take_wide).  Each state is described once (tests/scenario_lib.py) and built from that description by
the oracle's scn_build and by monsoon_debug_build, the way tests/test_coop_legal_gpu.py builds its states; each comes with
the actions to step from it.  reference() plays every (state, action) on the recursive oracle and asserts that the case
is what it is named after:
    age-*         a play and a REPLACE with an age of 254 / AGE_MAX in word 0, 1 and 2 of the mover's deck ages (clean
                  lower words): 254 ages on, AGE_MAX is FAULT_CAP_DECK
    hand5         a five-card hand: a play and a REPLACE of each index an action can name (0..3; index 4 has no action:
                  64 + 21 * 4 is REPLACE), the fifth entry moving down
    dup-*         an earlier equal card in the hand, plain (the earlier one leaves), positioned on either or both entries
                  (the reference raises), two equal spells (identity: the played one leaves); an earlier equal card in
                  the deck under a draw
    deck11/12     a play into a deck of eleven (it fills the deck) and of twelve (FAULT_CAP_DECK), from hands of 1..4
    draw-*        a REPLACE whose drawn card sits at the deck's first index and at its last: of a single-use card (the
                  deck's own last entry) and of an ordinary one (the card that has just returned, found by trying stream
                  positions on the oracle)"""
import numpy as np

W0 = np.random.RandomState(2024).uniform(0, 1, 10)
FAULT_PY_EXCEPTION, FAULT_UNSUPPORTED, FAULT_CAP_DECK = 1, 20, 23
AGE_MAX = 255

_cache = {}


def _meta():
    from monsoon_amd.cards import CARD_INDEX, CARD_META
    return CARD_INDEX, CARD_META


def plain_cards():
    """Card indices of the units and structures without an ability: what the lists hold here."""
    _, meta = _meta()
    return [i for i, m in enumerate(meta) if m["kind"] in (0, 1) and not m["has_ability"] and m["int_id"] >= 0]


def card(index, positioned=False, single=False, age=0):
    _, meta = _meta()
    m = meta[index]
    return dict(card=index, cost=0, single_use=single, ff=bool(m["ff"]), kind="spell" if m["kind"] == 2 else "other",
                strength=m["strength"], position=[0, 0] if positioned else None, age=age)


def _entity(index, owner, tile):
    _, meta = _meta()
    m = meta[index]
    return dict(card=index, owner=owner, strength=3, movement=m["movement"], ff=bool(m["ff"]), status=[0] * 5,
                position=[tile % 4, tile // 4], damage_taken=0, single_use=False)


def state(lo, hand, deck):
    """A PLAY-phase state with `lo` to move, mana for everything, front line 2, a few bodies on the board."""
    bodies = plain_cards()
    players = []
    for o in range(2):
        cards = [dict(c) for c in (hand if o == lo else [card(bodies[0]), card(bodies[1])])]
        pile = [dict(c) for c in (deck if o == lo else [card(b, age=k) for k, b in enumerate(bodies[2:8])])]
        for k, c in enumerate(cards + pile):
            c["oid"] = k
        players.append(dict(base=12, mana=9, max_mana=9, front=2 if o == lo else (4 if o == 0 else 0), replacable=True,
                            leftmost_movable=True, faction=0, hand=cards, deck=pile))
    board = [None] * 20
    for t in (1, 6, 8, 15, 18):
        board[t] = _entity(bodies[0], t % 2, t)
    return dict(local_order=lo, cp=lo, phase=1, resolving=False, history=[], players=players, tiles=board)


def states():
    """[(name, state, [action or ("play", hand index), ...], stream position or None = to be searched)]"""
    index, meta = _meta()
    b = plain_cards()
    assert len(b) >= 17, len(b)
    spell = next(i for i, m in enumerate(meta) if m["kind"] == 2 and not m["target"]["has"] and m["int_id"] >= 0)
    hand4 = [card(x) for x in b[:4]]
    out = []
    for w in range(3):
        for v in (AGE_MAX - 1, AGE_MAX):
            ages = [(7 * k + 3 * w) % 50 for k in range(10)]
            ages[4 * w + 1] = v
            out.append((f"age-word{w}-{v}", state(w % 2, hand4, [card(x, age=a) for x, a in zip(b[5:15], ages)]), [("play", w), 148 + w], 5))
    five = [card(x) for x in b[:5]]
    out.append(("hand5", state(1, five, [card(x, age=k) for k, x in enumerate(b[5:12])]), [("play", i) for i in range(4)] + [148, 149, 150, 151], 9))
    deck6 = [card(x, age=2 * k) for k, x in enumerate(b[6:12])]
    for fa in (False, True):
        for fb in (False, True):
            hand = [card(b[0], positioned=fa), card(b[1]), card(b[0], positioned=fb), card(b[2])]
            out.append((f"dup-hand-{int(fa)}{int(fb)}", state(int(fa), hand, deck6), [("play", 2), 150, ("play", 0)], 11))
    out.append(("dup-spells", state(0, [card(spell), card(b[1]), card(spell)], deck6), [("play", 2), 150], 13))
    # the heavy card at the deck's end is drawn; an equal card sits before it: plain (that one leaves the deck), positioned (raises)
    for fa in (False, True):
        deck = [card(b[8], positioned=fa, age=0), card(b[9], age=0), card(b[8], age=200)]
        out.append((f"dup-deck-{int(fa)}", state(1, hand4, deck), [148], 15))
    for hn in range(1, 5):
        for dn in (11, 12):
            out.append((f"deck{dn}-hand{hn}", state(hn % 2, [card(x) for x in b[:hn]], [card(x, age=k) for k, x in enumerate(b[5:5 + dn])]),
                        [("play", hn - 1)], 17))
    single = [card(b[0], single=True)] + [card(x) for x in b[1:4]]
    out.append(("draw-first-single", state(0, single, [card(x, age=200 if k == 0 else 0) for k, x in enumerate(b[5:11])]), [148], 19))
    out.append(("draw-last-single", state(1, single, [card(x, age=200 if k == 5 else 0) for k, x in enumerate(b[5:11])]), [148], 21))
    out.append(("draw-first", state(0, hand4, [card(x, age=200 if k == 0 else 0) for k, x in enumerate(b[5:11])]), [149], 23))
    out.append(("draw-last", state(1, hand4, [card(b[5], age=0)]), [150], None))
    return out


def _lists(canon, mover):
    """(hand cards, deck cards) of `mover` in a canonical record (monsoon_amd/csrc/canon.h)."""
    c = np.frombuffer(canon, dtype=np.uint8)
    n = 12
    for o in range(2):
        hn, dn = int(c[n + 9]), int(c[n + 10])
        hand = [int(c[n + 12 + 3 * i]) for i in range(hn)]
        deck = [int(c[n + 12 + 3 * hn + 11 * i]) for i in range(dn)]
        if o == mover:
            return hand, deck
        n += 12 + 3 * hn + 11 * dn


def _resolve(legal, a):
    if not isinstance(a, tuple):
        return a
    i = a[1]
    own = [x for x in legal if 16 * i <= x < 16 * i + 16 or (64 + 21 * i <= x < 64 + 21 * i + 20 and x < 148)]
    assert own, (a, legal)
    return own[0]


def reference(core="oracle"):
    """dict(names, enc, seeds, pos, rows): rows = [(state k, action, fault, hash after)], every case asserted to be what
    it is named after; and per state the oracle's decision (action, scores, hash after the commit)."""
    if core in _cache:
        return _cache[core]
    import oracle_lib
    import scenario_lib as S
    sts = states()
    assert len(sts) <= 64
    orc = oracle_lib.Oracle(1, core=core) if core != "oracle" else oracle_lib.Oracle(1)
    names, encs, seeds, poss, rows, decisions, facts = [], [], [], [], [], [], {}
    for k, (name, st, actions, pos) in enumerate(sts):
        enc, seed, lo = S.encode_state(st), 6000 + k, st["local_order"]

        def run(p, a):
            assert orc.scn_build(0, seed, p, enc) == 0, name
            before = _lists(orc.canon(0), lo)
            act = _resolve(orc.legal_actions(0), a)
            f = orc.step(0, act)[0]
            return act, f, orc.canon_hash(0), before, _lists(orc.canon(0), lo)

        if pos is None:   # draw-last: the stream position at which the REPLACE draws the card that has just returned
            for p in range(600):
                act, f, _, before, after = run(p, actions[0])
                if not f and after[0][-1] == before[0][act - 148]:
                    pos = p
                    break
            assert pos is not None, name
        for a in actions:
            act, f, h, before, after = run(pos, a)
            rows.append((k, act, f, h))
            facts[(name, a)] = (act, f, before, after)
        assert orc.scn_build(0, seed, pos, enc) == 0
        a, scores, _ = orc.decide(0, W0)
        f = orc.step(0, a)[0]
        decisions.append(dict(action=a, scores=scores, fault=f, hash=orc.canon_hash(0)))
        names.append(name), encs.append(enc), seeds.append(seed), poss.append(pos)
    _check(facts)
    _cache[core] = dict(names=names, enc=encs, seeds=seeds, pos=poss, rows=rows, decisions=decisions)
    return _cache[core]


def _check(facts):
    def removed(before, after):   # index of the hand entry that left, for a hand of distinct positions
        hand, new = before[0], after[0]
        return next(i for i in range(len(hand)) if i >= len(new) or hand[i] != new[i])

    for (name, a), (act, f, before, after) in facts.items():
        hand, deck = before
        if name.startswith("age-"):
            assert f == (FAULT_CAP_DECK if name.endswith(str(AGE_MAX)) else 0), (name, a, f)
        elif name == "hand5":
            assert f == 0 and len(hand) == 5 and len(after[0]) == (4 if act < 148 else 5), (name, a, f)
            if act < 148:
                assert removed(before, after) == a[1] and after[0][3] == hand[4], (name, a)
            else:
                assert after[0][:4] == hand[:act - 148] + hand[act - 147:], (name, a)
        elif name.startswith("dup-hand-"):
            positioned = name[-2:] != "00"
            later = (isinstance(a, tuple) and a[1] == 2) or a == 150
            if later and positioned:
                assert f == (FAULT_UNSUPPORTED if name[-2:] == "11" else FAULT_PY_EXCEPTION), (name, a, f)
            else:
                assert f == 0 and after[1][-1] == hand[0], (name, a, f)   # the card returns to the deck's end
                if later:
                    assert after[0][:2] == hand[1:3], (name, a, after[0])   # the EARLIER equal entry left
        elif name == "dup-spells":
            assert f == 0 and after[0][:2] == hand[:2], (name, a, after[0])   # identity: the played one left
        elif name.startswith("dup-deck-"):
            if name.endswith("1"):
                assert f == FAULT_PY_EXCEPTION, (name, f)
            else:
                assert f == 0 and after[0][-1] == deck[2] and after[1][0] == deck[1], (name, after)   # deck[0] left, not deck[2]
        elif name.startswith("deck11"):
            assert f == 0 and len(deck) == 11 and len(after[1]) == 12, (name, f)
        elif name.startswith("deck12"):
            assert f == FAULT_CAP_DECK and len(deck) == 12, (name, f)
        elif name.startswith("draw-first"):
            assert f == 0 and after[0][-1] == deck[0], (name, f)
        elif name == "draw-last-single":
            assert f == 0 and after[0][-1] == deck[-1] and len(after[1]) == len(deck) - 1, (name, f)
        elif name == "draw-last":
            assert f == 0 and after[0][-1] == hand[act - 148] and after[1] == deck, (name, f)
        else:
            raise AssertionError(name)
