"""The oracle's line of the games tests/test_target_scan_gpu.py plays, and which target scans of the rules core they reach.

Two decks, 64 games x 40 decisions each, W0 on the first player's side and W1 on the other: N12M (the benchmark's), and
a deck made only of cards whose ability code scans for targets (TOUCHED; on the extended build two of them give way to
the extended-record cards ua20 and b005).  Per decision round and game: the chosen action, the 156 scores, the state
hash after the commit (tests/pass_overhead_trace.py's layout).

reached() reads the oracle's own states (its canonical record, monsoon_amd/csrc/canon.h) before every decision and says,
for every legal action the look-ahead steps, which kind of scan its step begins with and how many tiles that scan hits:
    shape_list    a unit whose ON_PLAY ability lists a selector's targets (u026 BEHIND, u103 BORDERING, u055 FRONT)
    shape_any     one that only asks whether there are any (u053 SURROUNDING then BORDERING, u106 BORDERING, u051)
    exclude       one that lists the board without itself (u021, u061, u306)
    spell_has     a targeted spell onto a tile (s001): `position in targets`
and which touched cards with a later trigger (ON_DEATH, BEFORE_ATTACKING, ...) stand on a board at all."""
import numpy as np

import oracle_lib
from monsoon_amd.cards import CARD_IDS, CARD_INDEX, CARD_META, deck_indices

W0 = np.random.RandomState(2024).uniform(0, 1, 10)
W1 = np.random.RandomState(7).uniform(0, 1, 10)
SEEDS = list(range(64))
DECISIONS = 40

# Every card but one is one whose ability goes through shape_targets / shape_any (u007 u313 SURROUNDING, u026 BEHIND, u055
# u074 FRONT, u053 SURROUNDING and BORDERING, u103 u106 BORDERING), get_targets with an excluded tile (u021 u306) or the
# membership form (s001, the targeted spell).  No card aims a target descriptor at SIDE, ROW or COLUMN.  s012 rides along:
# its empty-tile list stayed as it was (profiles/target_scan_ab.txt), the benchmark's deck holds it.
TOUCHED = ["u007", "u026", "u053", "u055", "u103", "u106", "u074", "u313", "u306", "u021", "s001", "s012"]
TOUCHED_EXT = ["ua20", "b005"] + TOUCHED[2:]   # FRONT as an emptiness question, SURROUNDING inside a frozen world

NUM_CARDS, TOKEN_STRUCT = len(CARD_META), 128
SH_FRONT, SH_BEHIND, SH_BORDERING, SH_SURROUNDING = 0, 1, 5, 6
K_ANY, K_UNIT, K_STRUCT = 0, 1, 2
S_ANY, S_FRIENDLY, S_ENEMY = 0, 1, 2
# ON_PLAY cards whose first scan is a selector around the tile they are placed on: (kind of scan, shape, target kind, side)
ON_PLAY_SHAPE = {"u026": ("shape_list", SH_BEHIND, K_ANY, S_ENEMY), "u103": ("shape_list", SH_BORDERING, K_UNIT, S_ENEMY),
                 "u053": ("shape_any", SH_SURROUNDING, K_UNIT, S_ANY), "u051": ("shape_any", SH_BORDERING, K_UNIT, S_ANY),
                 "u106": ("shape_any", SH_BORDERING, K_STRUCT, S_FRIENDLY)}
ON_PLAY_OTHER = {"u055": "shape_list", "u021": "exclude", "u061": "exclude", "u306": "exclude"}
LATER = ("u007", "u074", "u313", "ua20", "b005")

_cache = {}


def deck(name, ext=False):
    if name == "N12M":
        return deck_indices("N12M")
    return np.array([CARD_INDEX[c] for c in (TOUCHED_EXT if ext is True else TOUCHED)], dtype=np.uint8)


def parse(canon):
    """(local order, [hand card ids of player 0, of player 1], {tile: (card index, owner, strength)}) of a canonical record."""
    b = np.frombuffer(canon, dtype=np.uint8)
    local, n, hands = int(b[1]), 12, []
    for _ in range(2):
        hn, dn = int(b[n + 9]), int(b[n + 10])
        hands.append([CARD_IDS[int(b[n + 12 + 3 * i])] for i in range(hn)])
        n += 12 + 3 * hn + 11 * dn
    board = {}
    for t in range(20):
        if b[n] == 0xFF:
            n += 1
            continue
        board[t] = (int(b[n]), int(b[n + 1]) & 1, int(np.frombuffer(canon[n + 2:n + 4], dtype=np.int16)[0]))
        n += 11
    return local, hands, board


def in_shape(shape, c, p):
    """rules.h in_shape for the local point of view (the mover's), tiles as (x, y)."""
    dx, dy = p[0] - c[0], p[1] - c[1]
    if shape == SH_FRONT:
        return dx == 0 and p[1] < c[1]
    if shape == SH_BEHIND:
        return dx == 0 and p[1] > c[1]
    if shape == SH_BORDERING:
        return abs(dx) + abs(dy) == 1
    return (dx or dy) and abs(dx) <= 1 and abs(dy) <= 1


def hits(board, mover, shape, centre, kind, side):
    n = 0
    for t, (card, owner, strength) in board.items():
        struct = CARD_META[card]["kind"] == 1 if card < NUM_CARDS else card == TOKEN_STRUCT
        ok = strength > 0 and (kind == K_ANY or (kind == K_STRUCT) == struct)
        ok = ok and (side == S_ANY or (side == S_FRIENDLY) == (owner == mover))
        n += bool(ok and in_shape(shape, centre, (t % 4, t // 4)))
    return n


def trace(deck_name, ext=False):
    """dict over [DECISIONS][games]: action, scores[..][156], hash, live, clean; and "reached": {kind: [hit counts]},
    "on_board": the touched cards with a later trigger seen on a board."""
    key = (deck_name, ext)
    if key in _cache:
        return _cache[key]
    n = len(SEEDS)
    d = deck(deck_name, ext)
    orc = oracle_lib.Oracle(n, extended=ext)
    for i, s in enumerate(SEEDS):
        assert orc.reset(i, s, d, d) == 0
    t = dict(action=np.full((DECISIONS, n), 255, dtype=np.uint8), scores=np.full((DECISIONS, n, 156), np.nan),
             hash=np.zeros((DECISIONS, n), dtype=np.uint64), live=np.zeros((DECISIONS, n), dtype=bool), clean=np.ones((DECISIONS, n), dtype=bool))
    reached, on_board = {}, set()
    dead, faulted = [False] * n, [False] * n
    for r in range(DECISIONS):
        for i in range(n):
            if not dead[i] and orc.have_winner(i):
                dead[i] = True
            if not dead[i]:
                local, hands, board = parse(orc.canon(i))
                a, sc, _ = orc.decide(i, W0 if orc.to_play(i) == 0 else W1)
                t["action"][r, i], t["scores"][r, i], t["live"][r, i] = a, sc, True
                on_board.update(CARD_IDS[c] for c, _, _ in board.values() if c < NUM_CARDS and CARD_IDS[c] in LATER)
                for act in np.nonzero(~np.isnan(sc))[0]:
                    _classify(int(act), local, hands[local], board, reached)
                if orc.step(i, a)[0]:   # an exception while applying the action ends the game as a draw
                    dead[i] = faulted[i] = True
            t["hash"][r, i] = orc.canon_hash(i)
            t["clean"][r, i] = not faulted[i]
    for v in t.values():
        v.setflags(write=False)
    t["reached"], t["on_board"] = reached, on_board
    _cache[key] = t
    return t


def _classify(act, mover, hand, board, reached):
    if act < 64:
        cid, tile = hand[act // 16], (4 - (act % 16) // 4) * 4 + (act % 16) % 4
        if cid in ON_PLAY_SHAPE:
            kind, shape, tk, side = ON_PLAY_SHAPE[cid]
            reached.setdefault(kind, []).append(hits(board, mover, shape, (tile % 4, tile // 4), tk, side))
        elif cid in ON_PLAY_OTHER:
            reached.setdefault(ON_PLAY_OTHER[cid], []).append(-1)
    elif act < 148:
        c, i = divmod(act - 64, 21)
        if hand[c] == "s001" and i > 0:
            reached.setdefault("spell_has", []).append(1)


def legal_counts(t):
    return (~np.isnan(t["scores"])).sum(axis=2)[t["live"]]


def check_reached(ext):
    """Every converted kind of call site is reached in the two decks' games, the selector scans with a scan that hits
    nothing and one that hits more than one tile; the cards whose scans run on a later trigger stand on a board."""
    a, b = trace("N12M", ext), trace("touched", ext)
    kinds = {k: a["reached"].get(k, []) + b["reached"].get(k, []) for k in set(a["reached"]) | set(b["reached"])}
    for k in ("shape_list", "shape_any", "exclude", "spell_has"):
        assert len(kinds.get(k, [])) > 0, (k, {q: len(v) for q, v in kinds.items()})
    for k in ("shape_list", "shape_any"):
        counted = [v for v in kinds[k] if v >= 0]   # (-1: reached, its hits not counted here)
        assert min(counted) == 0 and max(counted) > 1, (k, sorted(set(counted)))
    later = a["on_board"] | b["on_board"]
    want = {"u007", "u074", "u313"} | ({"ua20", "b005"} if ext is True else set())
    assert want <= later, (want - later)
