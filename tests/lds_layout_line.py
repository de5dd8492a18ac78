"""The oracle's line of the 64 games tests/test_lds_layout_gpu.py plays on every hot-kernel variant, and the cases they hold.

Games 0..47 are N12M against N12M from reset (seeds 0..47); games 48..63 start from a described PLAY-phase state
(tests/scenario_lib.py, built by monsoon_debug_build on the device and by scn_build here) whose stream stands 1..16 words in
front of the end of its first block, so that their first committed draws run over it: the wavefront regenerates the block
with the candidate columns as its twist buffer and puts the record back into column 0.  W0 plays the first player, W1 the
second.  Per decision round and game: the chosen action, the number of legal actions, the canonical hash, to_play /
have_winner, the ten features (NaN where get_feature_vector raises) and the fault code of the game so far.  A game that has
a winner, or whose committed step raised, decides no more, as in tests/pass_overhead_trace.py."""
import numpy as np

import oracle_lib
import scenario_lib as S
from monsoon_amd.cards import CARD_INDEX, CARD_META, deck_indices

W0 = np.random.RandomState(2024).uniform(0, 1, 10)
W1 = np.random.RandomState(7).uniform(0, 1, 10)
N, N_RESET, DECISIONS = 64, 48, 40
SEEDS = list(range(N_RESET))
BLOCK = 624   # words of a stream block
UNIT, UNIT2, STRUCT, SPELL = "u025", "u001", "b001", "s012"   # plain cards and an untargeted spell

_cache = {}


def _card(cid, oid, age=0):
    m = CARD_META[CARD_INDEX[cid]]
    return dict(card=CARD_INDEX[cid], cost=m["cost"], single_use=False, ff=bool(m["ff"]), kind="spell" if m["kind"] == 2 else "other",
                strength=m["strength"], position=None, age=age, oid=oid)


def _entity(cid, owner, tile, strength):
    m = CARD_META[CARD_INDEX[cid]]
    return dict(card=CARD_INDEX[cid], owner=owner, strength=strength, movement=m["movement"], ff=bool(m["ff"]), status=[0] * 5,
                position=[tile % 4, tile // 4], damage_taken=0, single_use=False)


def scenario(k):
    """(seed, stream position, encoded state) of game N_RESET + k: four cards in hand, eight in the deck, a few plain entities
    on the board, mana enough for a card or two.  The first two are the decisions no reset game of these seeds holds, each with
    the mover's half of the board empty: game 48 four affordable units, the front line at 0 and a REPLACE left, 4 x 16 PLACE +
    4 REPLACE + PASS = 69 legal actions (three passes of U = 32, two of U = 64); game 49 the same hand with the front line
    at 3 and no REPLACE, 4 x 8 PLACE = exactly 32."""
    lo = k % 2
    wide = k < 2   # (the two counted states)
    players = []
    for o in range(2):
        mine = wide and o == lo
        hand = [_card(c, j) for j, c in enumerate((UNIT, UNIT2, STRUCT, UNIT) if mine else (UNIT, STRUCT, SPELL, UNIT2))]
        deck = [_card(c, 4 + j, age=j) for j, c in enumerate((UNIT2, UNIT, STRUCT, SPELL, UNIT, UNIT2, STRUCT, UNIT))]
        mana = 9 if mine else 3 + k % 4
        front = (0 if k == 0 else 3) if mine else (3 if o == 0 else 1)
        players.append(dict(base=12, mana=mana, max_mana=mana, front=front, replacable=not (mine and k == 1), leftmost_movable=True,
                            faction=0, hand=hand, deck=deck))
    board = [None] * 20
    if not wide:
        for t in (1 + k % 3, 6, 13, 18 - k % 2):
            board[t] = _entity(UNIT if t % 2 else STRUCT, 0 if t >= 10 else 1, t, 2 + (t + k) % 4)
    st = dict(local_order=lo, cp=lo, phase=1, resolving=False, history=[], players=players, tiles=board)
    return 7000 + k, BLOCK - 1 - k, S.encode_state(st)


def line(ext=False):
    """dict of read-only arrays over [DECISIONS][N]: action, n_legal, hash, status[..][2], features[..][10], fault, live, clean."""
    if ext in _cache:
        return _cache[ext]
    deck = deck_indices("N12M")
    orc = oracle_lib.Oracle(N, extended=ext)
    for i, s in enumerate(SEEDS):
        assert orc.reset(i, s, deck, deck) == 0
    for k in range(N - N_RESET):
        seed, pos, enc = scenario(k)
        assert orc.scn_build(N_RESET + k, seed, pos, enc) == 0, k
    t = dict(action=np.full((DECISIONS, N), 255, dtype=np.uint8), n_legal=np.zeros((DECISIONS, N), dtype=np.int32),
             hash=np.zeros((DECISIONS, N), dtype=np.uint64), status=np.zeros((DECISIONS, N, 2), dtype=np.int32),
             features=np.full((DECISIONS, N, 10), np.nan), fault=np.zeros((DECISIONS, N), dtype=np.uint8),
             live=np.zeros((DECISIONS, N), dtype=bool), clean=np.ones((DECISIONS, N), dtype=bool))
    dead, fault = [False] * N, [0] * N
    for r in range(DECISIONS):
        for i in range(N):
            if not dead[i] and orc.have_winner(i):
                dead[i] = True
            if not dead[i]:
                a, sc, _ = orc.decide(i, W0 if orc.to_play(i) == 0 else W1)
                t["action"][r, i], t["n_legal"][r, i], t["live"][r, i] = a, int((~np.isnan(sc)).sum()), True
                f = orc.step(i, a)[0]
                if f:   # an exception while applying the action ends the game as a draw
                    dead[i], fault[i] = True, f
            t["hash"][r, i] = orc.canon_hash(i)
            t["fault"][r, i] = fault[i]
            t["clean"][r, i] = not fault[i]
            if not fault[i]:
                t["status"][r, i] = (orc.to_play(i), int(orc.have_winner(i)))
                fv = orc.features(i)
                if fv is not None:
                    t["features"][r, i] = fv
    for v in t.values():
        v.setflags(write=False)
    _cache[ext] = t
    return t


def wanted(u):
    """The legal counts a variant of u candidate lanes must meet in these games: a single candidate (the first column alone),
    exactly u (the last column, one pass) and more than 2 u (several passes).  One combination cannot occur: more than 128
    legal actions at u = 64.  A hand slot contributes at most 21 actions (16 PLACE tiles, or a spell's 20 target tiles and
    its untargeted form share the slot's 21 USE ids), the hand has four playable slots, then 4 REPLACE and PASS: 89 at the
    most.  u = 64 meets the largest count these games hold instead, 69 (a second pass of five)."""
    return (1, u, 2 * u + 1) if u <= 32 else (1, 64, 65)


def check_cases(t, lanes):
    counts = t["n_legal"][t["live"]]
    have = set(int(c) for c in counts)
    assert max(have) <= 128
    for u in lanes:
        one, full, more = wanted(u)
        assert one in have and full in have, (u, sorted(have))
        assert any(c >= more for c in have), (u, sorted(have))
    # the scenario games decide all the way: their draws run over the end of the first block (the GPU test reads the cursor)
    assert t["live"][:, N_RESET:].sum() >= 30 * (N - N_RESET)
