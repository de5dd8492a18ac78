"""What the games of tests/test_wide_ent_gpu.py give the move, damage and destroy handlers of rules.h (h_move, call_entity_damage,
call_destroy, call_unit_play: the entity image, state.h MSB_WIDE_ENT).

The games and their line are those of tests/wide_lists_trace.py (64 N12M games x 40 decisions, 16 random-deck games x 20 for
the extended and large builds): trace() is that module's, computed once for both test files.  reached() replays the committed
actions on the recursive oracle and reads its canonical record (monsoon_amd/csrc/canon.h) before and after every step:
    quiet[k]      a unit placed with nothing on the k tiles ahead of it, found k tiles further on, the board otherwise
                  as it was (k = 1, 2)
    kill_target   a unit placed under an enemy: the enemy is gone, the unit is on the board
    kill_mover    ... the enemy is still there, weaker, the unit is not on the board
    kill_both     ... neither is on the board
    base_hit      the turn passed on with a unit of the next player on the row next to the passer's base, and that base lower after
    thaw          the turn passed on to a frozen unit, which stands where it stood with one freeze less
    poisoned      the turn passed on to a poisoned unit that is not frozen (it is damaged, then moves)
    vitalized     the turn passed on to a vitalized unit that is not frozen (it gains strength, then moves)"""
import numpy as np

import oracle_lib
import wide_lists_trace as T
from monsoon_amd.cards import CARD_META

W0, W1 = T.W0, T.W1
trace, legal_counts = T.trace, T.legal_counts
NUM_CARDS = len(CARD_META)
_cache = {}


def parse(canon):
    """(mover, [base of player 0, of player 1], [hand cards of player 0, of player 1], {tile: dict(card, owner, strength, status)})"""
    b = np.frombuffer(canon, dtype=np.uint8)
    mover, n, bases, hands = int(b[1]), 12, [], []
    for _ in range(2):
        bases.append(int(np.frombuffer(bytes(b[n:n + 2]), dtype=np.int16)[0]))
        hn, dn = int(b[n + 9]), int(b[n + 10])
        hands.append([int(b[n + 12 + 3 * i]) for i in range(hn)])
        n += 12 + 3 * hn + 11 * dn
    board = {}
    for t in range(20):
        if b[n] == 0xFF:
            n += 1
            continue
        board[t] = dict(card=int(b[n]), owner=int(b[n + 1]) & 1, strength=int(np.frombuffer(bytes(b[n + 2:n + 4]), dtype=np.int16)[0]),
                        status=[int(x) for x in b[n + 6:n + 11]])
        n += 11
    return mover, bases, hands, board


def _classify(a, before, after, r):
    mover, bases0, hands, b0 = before
    _, bases1, _, b1 = after
    if a < 64:
        card, at = hands[mover][a // 16], a % 16
        x, y = at % 4, 4 - at // 4          # the mover's own point of view: its units walk towards row 0
        tile = 4 * y + x
        if card >= NUM_CARDS or CARD_META[card]["kind"] != 0 or CARD_META[card]["movement"] < 1:
            return
        mine = [t for t, e in b1.items() if e["card"] == card and e["owner"] == mover and not (t in b0 and b0[t]["card"] == card and b0[t]["owner"] == mover)]
        ahead = b0.get(tile - 4) if y > 0 else None
        if ahead is None:
            for k in (1, 2):
                to = tile - 4 * k
                if to >= 0 and mine == [to] and all(tile - 4 * j not in b0 for j in range(1, k + 1)) and \
                        {t: e for t, e in b1.items() if t != to} == b0 and CARD_META[card]["movement"] >= k:
                    r["quiet"][k] += 1
        elif ahead["owner"] != mover:
            there = b1.get(tile - 4)
            enemy_there = there is not None and there["card"] == ahead["card"] and there["owner"] != mover
            if mine and not enemy_there:
                r["kill_target"] += 1
            elif not mine and enemy_there and there["strength"] < ahead["strength"]:
                r["kill_mover"] += 1
            elif not mine and there is None:
                r["kill_both"] += 1
    elif a == 155:
        nxt = 1 - mover
        for t, e in b0.items():
            if e["owner"] != nxt or not (e["card"] >= NUM_CARDS or CARD_META[e["card"]]["kind"] == 0):
                continue
            frozen, poisoned, _, _, vitalized = e["status"]
            stays = b1.get(19 - t)   # the board is flipped for the next player
            if frozen and stays is not None and stays["card"] == e["card"] and stays["status"][0] == frozen - 1:
                r["thaw"] += 1
            if not frozen:
                r["poisoned"] += poisoned > 0
                r["vitalized"] += vitalized > 0
                r["base_hit"] += t >= 16 and bases1[mover] < bases0[mover]


def reached(ext=False):
    if ext in _cache:
        return _cache[ext]
    t = trace(ext)
    decisions, n = t["action"].shape
    orc = oracle_lib.Oracle(n, extended=ext)
    r = dict(quiet=[0, 0, 0], kill_target=0, kill_mover=0, kill_both=0, base_hit=0, thaw=0, poisoned=0, vitalized=0)
    for i in range(n):
        assert orc.reset(i, t["seeds"][i], t["decks"][i, 0], t["decks"][i, 1]) == 0
        for d in range(decisions):
            if not t["live"][d, i]:
                break
            a = int(t["action"][d, i])
            before = parse(orc.canon(i))
            if orc.step(i, a)[0]:
                break
            assert orc.canon_hash(i) == int(t["hash"][d, i])
            _classify(a, before, parse(orc.canon(i)), r)
    _cache[ext] = r
    return r


def check_reached():
    """The N12M games hold committed quiet moves of one tile, fights that kill the target, the mover and both, base hits at a
    turn's start, frozen units that thaw and poisoned and vitalized movers.  No committed placement walks two tiles and leaves
    the board otherwise as it was (quiet[2] is counted and stays 0): tests/wide_ent_states.py describes that move (quiet-two-*),
    which the oracle is asserted to play that way and the device steps and decides."""
    r = reached(False)
    assert r["quiet"][1] > 0, r
    assert r["kill_target"] > 0 and r["kill_mover"] > 0 and r["kill_both"] > 0 and r["base_hit"] > 0, r
    assert r["thaw"] > 0 and r["poisoned"] > 0 and r["vitalized"] > 0, r
