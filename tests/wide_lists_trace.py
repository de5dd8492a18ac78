"""The oracle's line of the games tests/test_wide_lists_gpu.py plays, and which list and path bookkeeping they reach.

64 N12M games x 40 decisions (W0 on the first player's side, W1 on the other; tests/pass_overhead_trace.py's layout: per
decision round and game the chosen action, the 156 scores, the best score, the state hash after the commit), and 16
random-deck games x 20 decisions for the extended and large builds.

trace() reads the oracle's own states (its canonical record, monsoon_amd/csrc/canon.h) before and after every committed
decision and counts what the whole-word forms of rules.h (discard_wide, draw_take_wide, set_path_impl) were given:
    remove[i]     a play or a REPLACE of hand index i, over every legal action of the decision (the look-ahead steps them all)
    deck11        a legal play with eleven cards in the mover's deck (the played card fills it)
    draw_first    a committed REPLACE whose drawn card sat at deck index 0 (of the deck as Player.discard left it)
    draw_last     one whose drawn card sat at the last index
    sidestep      a legal placement of a unit that moves, with an enemy beside its tile and nothing or a friend ahead
                  (Unit.set_path turns to the side)"""
import numpy as np

import oracle_lib
from c5_games import c5_games
from monsoon_amd.cards import CARD_META, deck_indices

W0 = np.random.RandomState(2024).uniform(0, 1, 10)
W1 = np.random.RandomState(7).uniform(0, 1, 10)
SEEDS = list(range(64))
DECISIONS = 40
RANDOM_DECISIONS = 20
NUM_CARDS = len(CARD_META)

_cache = {}


def parse(canon):
    """(mover, [(hand cards, deck cards) of player 0, of player 1], {tile: (card index, owner)}) of a canonical record."""
    b = np.frombuffer(canon, dtype=np.uint8)
    mover, n, lists = int(b[1]), 12, []
    for _ in range(2):
        hn, dn = int(b[n + 9]), int(b[n + 10])
        hand = [int(b[n + 12 + 3 * i]) for i in range(hn)]
        deck = [int(b[n + 12 + 3 * hn + 11 * i]) for i in range(dn)]
        lists.append((hand, deck))
        n += 12 + 3 * hn + 11 * dn
    board = {}
    for t in range(20):
        if b[n] == 0xFF:
            n += 1
            continue
        board[t] = (int(b[n]), int(b[n + 1]) & 1)
        n += 11
    return mover, lists, board


# the first 16 games of the C5 family (tests/c5_games.py: random decks of the observable cards, the extended-record cards among
# them) that last the 20 decisions without an exception on the extended and on the large build (trace() asserts it)
RANDOM_INDICES = [0, 1, 2, 4, 5, 6, 7, 8, 10, 11, 14, 15, 16, 17, 18, 19]


def random_games():
    """(seeds, uint8[16][2][12] deck pairs) of the random-deck games."""
    m, pairs = c5_games(RANDOM_INDICES)
    return [int(s) for s in m["seed"]], pairs


def _classify(act, mover, hand, deck, board, reached):
    if act < 148:
        place = act < 64
        idx, at = (act // 16, act % 16) if place else divmod(act - 64, 21)
        if at >= 20:
            return
        reached["remove"][idx] += 1
        reached["deck11"] += len(deck) == 11
        meta = CARD_META[hand[idx]] if hand[idx] < NUM_CARDS else None
        if place and meta is not None and meta["kind"] == 0 and meta["movement"] >= 1 and not meta.get("ff", False):
            x, y = at % 4, 4 - at // 4   # the mover's own point of view: its units walk towards row 0
            ahead = board.get((y - 1) * 4 + x) if y > 0 else None
            beside = [board.get(y * 4 + x + d) for d in (-1, 1) if 0 <= x + d <= 3]
            if y > 0 and (ahead is None or ahead[1] == mover) and any(e is not None and e[1] != mover for e in beside):
                reached["sidestep"] += 1
    elif act < 152:
        reached["remove"][act - 148] += 1


def trace(ext=False):
    """dict over [decisions][games]: action, scores[..][156], best, hash, live, clean; "reached" as the module says."""
    if ext in _cache:
        return _cache[ext]
    standard = ext is False
    n, decisions = (len(SEEDS), DECISIONS) if standard else (len(RANDOM_INDICES), RANDOM_DECISIONS)
    seeds, decks = (SEEDS, np.broadcast_to(deck_indices("N12M"), (n, 2, 12))) if standard else random_games()
    orc = oracle_lib.Oracle(n, extended=ext)
    for i in range(n):
        assert orc.reset(i, seeds[i], decks[i, 0], decks[i, 1]) == 0
    t = dict(action=np.full((decisions, n), 255, dtype=np.uint8), scores=np.full((decisions, n, 156), np.nan), best=np.full((decisions, n), np.nan),
             hash=np.zeros((decisions, n), dtype=np.uint64), live=np.zeros((decisions, n), dtype=bool), clean=np.ones((decisions, n), dtype=bool))
    reached = dict(remove=[0] * 5, deck11=0, draw_first=0, draw_last=0, sidestep=0)
    dead, faulted = [False] * n, [False] * n
    for r in range(decisions):
        for i in range(n):
            if not dead[i] and orc.have_winner(i):
                dead[i] = True
            if not dead[i]:
                mover, lists, board = parse(orc.canon(i))
                hand, deck = lists[mover]
                a, sc, _ = orc.decide(i, W0 if orc.to_play(i) == 0 else W1)
                t["action"][r, i], t["scores"][r, i], t["best"][r, i], t["live"][r, i] = a, sc, sc[a], True
                for act in np.nonzero(~np.isnan(sc))[0]:
                    _classify(int(act), mover, hand, deck, board, reached)
                if orc.step(i, a)[0]:   # an exception while applying the action ends the game as a draw
                    dead[i] = faulted[i] = True
                elif 148 <= a < 152 and standard:
                    # N12M holds no single-use card and no card twice: the replaced card went to the deck's end, and the
                    # drawn card, now the last of the hand, names its index there
                    after = parse(orc.canon(i))[1][mover][0]
                    at = (deck + [hand[a - 148]]).index(after[-1])
                    reached["draw_first"] += at == 0
                    reached["draw_last"] += at == len(deck)
            t["hash"][r, i] = orc.canon_hash(i)
            t["clean"][r, i] = not faulted[i]
    for v in t.values():
        v.setflags(write=False)
    assert standard or (t["live"].all() and t["clean"].all())
    t["reached"], t["decks"], t["seeds"] = reached, decks, seeds
    _cache[ext] = t
    return t


def legal_counts(t):
    return (~np.isnan(t["scores"])).sum(axis=2)[t["live"]]


def check_reached():
    """The N12M games give the whole-word forms a removal at each of the four hand indices a game knows, a REPLACE that draws
    the deck's first entry and a path that turns to the side.  They hold no play into a deck of eleven (no side plays three
    cards in a turn within 40 decisions) and no REPLACE that draws the last entry (the card just returned: weight 1 among
    weights above 100): deck11 and draw_last are counted and stay 0, and tests/wide_lists_states.py describes states that
    hold both, which the oracle is asserted to play that way and the device steps (tests/test_wide_lists_gpu.py)."""
    r = trace(False)["reached"]
    assert all(r["remove"][i] > 0 for i in range(4)), r
    assert r["draw_first"] > 0 and r["sidestep"] > 0, r
