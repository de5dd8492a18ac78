"""Described states for tests/test_wide_ent_gpu.py: what the 64 N12M games do not give the move handler of rules.h (h_move on
the entity image, state.h MSB_WIDE_ENT).  Each state is described once (tests/scenario_lib.py) and built from that description
by the oracle's scn_build and by monsoon_debug_build, as tests/wide_lists_states.py builds its states; each comes with the
actions to step from it.  reference() plays every (state, action) on the recursive oracle and asserts that the case is what it
is named after:
    before-attacking-*   a unit with a BEFORE_ATTACKING ability placed under an enemy, weaker and stronger than itself, and
                         with ST_DISABLED impossible on a played unit, the same unit standing on the board, disabled and not,
                         when the turn is passed to its owner: the enemy ahead is struck
    after-attacking-*    a unit with an AFTER_ATTACKING ability placed under a weaker enemy: it stands where the enemy stood
    confused-*           a confused unit, in an edge and in an inner column, once and twice confused, when the turn is passed to
                         its owner: it has left its column and is confused once less
    quiet-two-*          a plain unit of movement two placed with nothing on the two tiles ahead: it stands two rows on and
                         the board is otherwise as it was (no committed placement of the 64 games does that)
    depth-guard-*        the boards of tests/golden/deep_scenarios.json.gz (recorded on the reference) that the standard record
                         holds and on which one Player.play ends in RecursionError: the step is FAULT_DEPTH, raised where
                         move_enter / call_run_ability find H_DEPTH at MAX_DEPTH"""
import gzip
import json
import os

import numpy as np

W0 = np.random.RandomState(2024).uniform(0, 1, 10)
TR_BEFORE_ATTACKING, TR_AFTER_ATTACKING = 2, 3
ST_CONFUSED, ST_DISABLED = 2, 3
FAULT_DEPTH = 18
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_cache = {}


def _meta():
    from monsoon_amd.cards import CARD_META
    return CARD_META


def plain_units():
    return [i for i, m in enumerate(_meta()) if m["kind"] == 0 and not m["has_ability"] and m["int_id"] >= 0]


def with_trigger(trigger):
    return next(i for i, m in enumerate(_meta()) if m["kind"] == 0 and m["trigger"] == trigger and m["movement"] >= 1 and m["int_id"] >= 0)


def card(index, age=0):
    m = _meta()[index]
    return dict(card=index, cost=1, single_use=False, ff=bool(m["ff"]), kind="other", strength=m["strength"], position=None, age=age)


def entity(index, owner, tile, strength, status=None):
    m = _meta()[index]
    return dict(card=index, owner=owner, strength=strength, movement=m["movement"], ff=bool(m["ff"]), status=list(status or [0] * 5),
                position=[tile % 4, tile // 4], damage_taken=0, single_use=False)


def state(lo, first_card, tiles, mana=9):
    """A PLAY-phase state with `lo` to move and `first_card` first in its hand, front line 2; mana for everything, or none:
    then passing the turn on is the one legal action besides REPLACE."""
    b = plain_units()
    players = []
    for o in range(2):
        hand = [card(first_card if o == lo else b[0]), card(b[1]), card(b[2])]
        deck = [card(x, age=k) for k, x in enumerate(b[3:9])]
        for k, c in enumerate(hand + deck):
            c["oid"] = k
        players.append(dict(base=12, mana=mana, max_mana=9, front=2 if o == lo else (4 if o == 0 else 0), replacable=True,
                            leftmost_movable=True, faction=0, hand=hand, deck=deck))
    board = [None] * 20
    for t, e in tiles.items():
        board[t] = e
    return dict(local_order=lo, cp=lo, phase=1, resolving=False, history=[], players=players, tiles=board)


PLACE_TILE, AHEAD = 3 * 4 + 1, 2 * 4 + 1     # hand[0] onto (1, 3); the enemy on (1, 2)
PLACE = (4 - 3) * 4 + 1                      # the action: card 0, tile offset (4 - y) * 4 + x


def states():
    """[(name, state, [action, ...], (seed, stream position) or None = numbered)]"""
    b = plain_units()
    two = next(i for i in b if _meta()[i]["movement"] == 2)
    ba, aa = with_trigger(TR_BEFORE_ATTACKING), with_trigger(TR_AFTER_ATTACKING)
    ba_str = _meta()[ba]["strength"]
    out = []
    for lo in (0, 1):
        out.append((f"quiet-two-{lo}", state(lo, two, {}), [PLACE]))
        out.append((f"before-attacking-weak-{lo}", state(lo, ba, {AHEAD: entity(b[0], 1 - lo, AHEAD, 1)}), [PLACE]))
        out.append((f"before-attacking-strong-{lo}", state(lo, ba, {AHEAD: entity(b[0], 1 - lo, AHEAD, ba_str + 4)}), [PLACE]))
        out.append((f"after-attacking-weak-{lo}", state(lo, aa, {AHEAD: entity(b[0], 1 - lo, AHEAD, 1)}), [PLACE]))
        # the turn is passed to 1 - lo, the board flips: tile t is tile 19 - t for the unit that then moves towards row 0
        for disabled in (0, 1):
            st = [0, 0, 0, disabled, 0]
            tiles = {19 - PLACE_TILE: entity(ba, 1 - lo, 19 - PLACE_TILE, ba_str, st), 19 - AHEAD: entity(b[0], lo, 19 - AHEAD, ba_str + 4)}
            out.append((f"before-attacking-moved-{disabled}-{lo}", state(lo, b[4], tiles, mana=0), [155]))
        for x in (0, 1):
            for confused in (1, 2):
                t = 2 * 4 + x
                tiles = {19 - t: entity(b[0], 1 - lo, 19 - t, 3, [0, 0, confused, 0, 0])}
                out.append((f"confused-{x}-{confused}-{lo}", state(lo, b[4], tiles, mana=0), [155]))
    out = [x + (None,) for x in out]
    # the recorded boards at the guard: the fixture names a position "class:family:seed:turn:action"
    with gzip.open(os.path.join(GOLD, "deep_scenarios.json.gz"), "rt") as f:
        cases = json.load(f)
    for case in cases:
        rec = case["records"][-1]
        if case["tier"] == 0 and rec["raised"] and rec["op"] == "Player.play" and len(case["records"]) == 1:
            st = rec["before"]
            out.append((f"depth-guard-{len(out)}", st, [int(case["test"].split(":")[-1])], (st["seed"], st["stream_pos"])))
    assert sum(name.startswith("depth-guard") for name, _, _, _ in out) >= 2
    return out


def _board(canon):
    import wide_ent_trace as E
    return E.parse(canon)[3]


def reference(core="oracle"):
    """dict(names, enc, seeds, pos, rows, decisions): rows = [(state k, action, fault, hash after)], every case asserted to be
    what it is named after; and per state the oracle's decision (action, scores, fault, hash after the commit)."""
    if core in _cache:
        return _cache[core]
    import oracle_lib
    import scenario_lib as S
    sts = states()
    assert len(sts) <= 64
    orc = oracle_lib.Oracle(1, core=core) if core != "oracle" else oracle_lib.Oracle(1)
    names, encs, seeds, poss, rows, decisions = [], [], [], [], [], []
    for k, (name, st, actions, stream) in enumerate(sts):
        enc = S.encode_state(st)
        seed, pos = stream if stream is not None else (7000 + k, 3 + 2 * k)
        for a in actions:
            assert orc.scn_build(0, seed, pos, enc) == 0, name
            assert a in orc.legal_actions(0), (name, a)
            before = _board(orc.canon(0))
            f = orc.step(0, a)[0]
            rows.append((k, a, f, orc.canon_hash(0)))
            _check(name, f, before, _board(orc.canon(0)))
        assert orc.scn_build(0, seed, pos, enc) == 0
        a, scores, _ = orc.decide(0, W0)
        f = orc.step(0, a)[0]
        decisions.append(dict(action=a, scores=scores, fault=f, hash=orc.canon_hash(0)))
        names.append(name), encs.append(enc), seeds.append(seed), poss.append(pos)
    _cache[core] = dict(names=names, enc=encs, seeds=seeds, pos=poss, rows=rows, decisions=decisions)
    return _cache[core]


def _check(name, fault, before, after):
    if name.startswith("depth-guard"):
        assert fault == FAULT_DEPTH, (name, fault)
        return
    assert fault == 0, (name, fault)
    meta = _meta()
    if name.startswith("quiet-two"):
        to = PLACE_TILE - 8
        assert to not in before and after[to]["owner"] == int(name[-1]) and meta[after[to]["card"]]["movement"] == 2, (name, after)
        assert {t: e for t, e in after.items() if t != to} == before, (name, after)
        return
    if name.startswith("before-attacking-moved"):
        # flipped: the mover stood on PLACE_TILE, the enemy on AHEAD
        enemy0, enemy1 = before[19 - AHEAD], after.get(AHEAD)
        assert enemy1 is None or enemy1["strength"] < enemy0["strength"] or enemy1["card"] != enemy0["card"], (name, enemy0, enemy1)
    elif name.startswith("before-attacking"):
        enemy0, enemy1 = before[AHEAD], after.get(AHEAD)
        assert meta[with_trigger(TR_BEFORE_ATTACKING)]["trigger"] == TR_BEFORE_ATTACKING
        assert enemy1 is None or enemy1["strength"] < enemy0["strength"] or enemy1["card"] != enemy0["card"], (name, enemy0, enemy1)
    elif name.startswith("after-attacking"):
        aa = with_trigger(TR_AFTER_ATTACKING)
        assert after.get(AHEAD) is not None and after[AHEAD]["card"] == aa and PLACE_TILE not in after, (name, after)
    elif name.startswith("confused"):
        x, confused = int(name.split("-")[1]), int(name.split("-")[2])
        t = 2 * 4 + x
        moved = [(tt, e) for tt, e in after.items() if e["status"][ST_CONFUSED] == confused - 1 and tt // 4 == 2 and tt % 4 != x]
        assert t not in after and len(moved) == 1, (name, after)
    else:
        raise AssertionError(name)
