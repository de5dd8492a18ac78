"""The oracle's line of the games tests/test_pass_overhead_gpu.py plays, and the cases it must contain.

N12M against N12M, W0 on the first player's side and a second RandomState vector on the other, DECISIONS decisions of
every game with the recursive oracle: per decision the chosen action, the 156 scores, the best score and the state hash
after the commit.  A game that has a winner, or whose committed step raised, decides no more (action 255, scores NaN)."""
import numpy as np

import oracle_lib
from monsoon_amd.cards import deck_indices

W0 = np.random.RandomState(2024).uniform(0, 1, 10)
W1 = np.random.RandomState(7).uniform(0, 1, 10)
SEEDS = list(range(64))
DECISIONS = 40

_cache = {}


def trace(ext=False):
    """dict of arrays over [DECISIONS][games]: action, scores[..][156], best, hash, live (decided), clean (hash defined)."""
    if ext in _cache:
        return _cache[ext]
    n = len(SEEDS)
    deck = deck_indices("N12M")
    orc = oracle_lib.Oracle(n, extended=ext)
    for i, s in enumerate(SEEDS):
        assert orc.reset(i, s, deck, deck) == 0
    t = dict(action=np.full((DECISIONS, n), 255, dtype=np.uint8), scores=np.full((DECISIONS, n, 156), np.nan),
             best=np.full((DECISIONS, n), np.nan), hash=np.zeros((DECISIONS, n), dtype=np.uint64),
             live=np.zeros((DECISIONS, n), dtype=bool), clean=np.ones((DECISIONS, n), dtype=bool))
    dead, faulted = [False] * n, [False] * n
    for r in range(DECISIONS):
        for i in range(n):
            if not dead[i] and orc.have_winner(i):
                dead[i] = True
            if not dead[i]:
                a, sc, _ = orc.decide(i, W0 if orc.to_play(i) == 0 else W1)
                t["action"][r, i], t["scores"][r, i], t["best"][r, i], t["live"][r, i] = a, sc, sc[a], True
                if orc.step(i, a)[0]:   # an exception while applying the action ends the game as a draw
                    dead[i] = faulted[i] = True
            t["hash"][r, i] = orc.canon_hash(i)
            t["clean"][r, i] = not faulted[i]
    for v in t.values():
        v.setflags(write=False)
    _cache[ext] = t
    return t


def legal_counts(t):
    return (~np.isnan(t["scores"])).sum(axis=2)[t["live"]]


def wanted_counts(u, counts):
    """The legal counts the issue names for lane count u, each replaced by the largest available below it where the
    games hold none; None where there is nothing at or below it."""
    have = sorted(set(int(c) for c in counts))
    out = {}
    for target in (1, u - 1, u, u + 1, 2 * u, 2 * u + 1):
        below = [c for c in have if c <= target]
        out[target] = below[-1] if below else None
    return out


def ties(t, u):
    """(decisions whose maximal score is shared by two candidates of one pass of u lanes -- the first maximum among them --,
    decisions whose maximal score is shared by candidates of two different passes)."""
    same = cross = 0
    for r, i in zip(*np.nonzero(t["live"])):
        sc = t["scores"][r, i]
        legal = np.nonzero(~np.isnan(sc))[0]
        top = np.nonzero(sc[legal] == sc[legal].max())[0]   # ranks of the maximal candidates in the ascending legal list
        if len(top) < 2:
            continue
        assert legal[top[0]] == t["action"][r, i]   # the smaller action id wins
        same += bool(top[1] // u == top[0] // u)
        cross += bool(top[-1] // u != top[0] // u)
    return same, cross
