"""The log of monsoon_rollout_logged (include/monsoon.h) by the CPU oracle: vs_expert_model.play(..., trace=True) gives the
actions and which of them were the bot's; the oracle's own decide gives the score of the action it chose and the legal
count of its mask.  Test infrastructure only.

ModelEngine has BatchEngine's rollout_logged / rollout_faults over it, so game_log.logged_rollout runs on the CPU."""
import numpy as np

import oracle_lib
import vs_expert_model as M
from monsoon_amd.engine import RolloutLog


class _Recording:
    """An Oracle whose decide() calls are written down: (score of the chosen action, legal actions) per decision."""

    def __init__(self, orc):
        self._orc, self.decisions = orc, []

    def __getattr__(self, name):
        return getattr(self._orc, name)

    def decide(self, i, w):
        a, scores, mask = self._orc.decide(i, w)
        self.decisions.append((scores[a], sum(bin(int(x)).count("1") for x in mask)))
        return a, scores, mask


def game_log(orc, seed, deck0, deck1, rows, weights, max_turns):
    """One game on slot 0 of `orc`: (vs_expert_model.play's dict, action uint8[k], score float64[k], n_legal int16[k], bot
    uint8[k]) over its k committed steps.  A raising bot's trailing 255 of the trace is not an entry."""
    rec = _Recording(orc)
    g = M.play(rec, 0, seed, deck0, deck1, rows, weights, max_turns, trace=True)
    k = g["steps"]
    action, bot = np.array(g["actions"][:k], dtype=np.uint8), np.array(g["bots"][:k], dtype=np.uint8)
    assert len(action) == k and len(g["actions"]) == k + int(g["bot_raised"])
    score, n_legal = np.full(k, np.nan), np.zeros(k, dtype=np.int16)
    assert int((bot == 0).sum()) == len(rec.decisions)
    if len(rec.decisions):
        score[bot == 0], n_legal[bot == 0] = zip(*rec.decisions)
    return g, action, score, n_legal, bot


class ModelEngine:
    """rollout_logged and rollout_faults of a BatchEngine on one record of the oracle (0 standard, 1 extended, 2 large)."""

    def __init__(self, tier=0):
        self.tier = tier
        self.orc = oracle_lib.Oracle(1, extended=tier)
        self.calls = []   # the number of matches of every call

    def rollout_logged(self, weights, matches, deck_pairs, max_turns, scores=True, n_legal=True):
        deck_pairs = np.asarray(deck_pairs, dtype=np.uint8).reshape(-1, 2, 12)
        n = len(matches)
        counts = np.zeros((len(weights), 3), dtype=np.int32)
        results = np.zeros(n, dtype=np.int8)
        log = RolloutLog.empty(n, max_turns, scores, n_legal)
        self.faults, self.finals = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint64)
        for k, m in enumerate(matches):
            d = deck_pairs[int(m["deck"])]
            g, a, s, nl, _ = game_log(self.orc, int(m["seed"]), d[0], d[1], (int(m["p1"]), int(m["p2"])), weights, max_turns)
            results[k], log.steps[k], self.faults[k], self.finals[k] = g["result"], g["steps"], g["reported"], g["final"]
            log.action[k, :len(a)] = a
            if scores:
                log.score[k, :len(a)] = s
            if n_legal:
                log.n_legal[k, :len(a)] = nl
            row, win = M.individual(int(m["p1"]), int(m["p2"]))
            if row >= 0:
                counts[row] += (g["result"] == win, g["result"] == -1, 1)
        self.calls.append(n)
        return counts, results, log.steps, log

    def rollout_faults(self, n):
        assert n == len(self.faults)
        return self.faults


def same_log(a, b):
    """Two RolloutLogs equal entry by entry: actions, legal counts, steps, and scores bit for bit where either holds a
    number (the padding NaN of the device is all ones, numpy's is not)."""
    if not (np.array_equal(a.action, b.action) and np.array_equal(a.steps, b.steps) and np.array_equal(a.n_legal, b.n_legal)):
        return False
    nan = np.isnan(a.score)
    return bool(np.array_equal(nan, np.isnan(b.score)) and np.array_equal(a.score[~nan].view(np.uint64), b.score[~nan].view(np.uint64)))
