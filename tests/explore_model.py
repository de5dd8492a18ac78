"""The contract of monsoon_rollout_explore (include/monsoon.h) over the CPU oracle: vs_expert_model.play's loop with the
exploration rule applied between the unchanged oracle's decide and step -- the legal list from the mask decide returns,
the draws from fitness.hash32, the taken action stepped.  Test infrastructure only.

    k = 0
    while not have_winner() and k < max_turns:
        if to_play() is the bot:  a = expert_action()
        else:
            g, scores, mask = decide(weights[row]); legal = sorted(mask)
            a = g
            if side's bit and (until_step <= 0 or k < until_step) and hash32(seed, match seed, k, 0) < threshold:
                a = legal[(hash32(seed, match seed, k, 1) * len(legal)) >> 32]
        step(a); k += 1

ModelEngine has BatchEngine's rollout_logged(..., explore=) / rollout_faults over it, so game_log.logged_rollout runs on
the CPU, ladder included."""
import numpy as np

import oracle_lib
import vs_expert_model as M
from monsoon_amd.engine import RolloutLog
from monsoon_amd.fitness import hash32


def legal_list(mask):
    return [x for x in range(156) if (int(mask[x >> 6]) >> (x & 63)) & 1]


def draw(explore, match_seed, k, n_legal):
    """(explores, rank) of the decision at committed step k by scalar hash32: the draw test only, like game_log.explore_draws."""
    explores = hash32(explore.seed, match_seed, k, 0) < explore.threshold
    return explores, (hash32(explore.seed, match_seed, k, 1) * n_legal) >> 32


def play(orc, i, seed, deck0, deck1, rows, weights, max_turns, explore=None):
    """One game on slot i of `orc`.  Returns vs_expert_model.play's dict (result, steps, fault, reported, bot_raised,
    decisions, lookahead, final) plus one list entry per committed step: action, score (the decision's best; NaN for the
    bot), n_legal (0 for the bot), greedy (255 for the bot), explored, taken_score (NaN for the bot), bot, side, and rank
    (the explored rank, -1 where the step did not explore) / greedy_rank (-1 for the bot)."""
    out = dict(result=-1, steps=0, fault=0, reported=0, bot_raised=False, decisions=0, lookahead=0)
    cols = ("action", "score", "n_legal", "greedy", "explored", "taken_score", "bot", "side", "rank", "greedy_rank")
    out.update({c: [] for c in cols})
    f = orc.reset(i, seed, deck0, deck1)
    if f:   # (the engine refuses the decks: no game)
        out.update(fault=f, reported=f, final=orc.canon_hash(i))
        return out
    steps = fault = 0
    while not orc.have_winner(i) and steps < max_turns:
        side = orc.to_play(i)
        row = rows[side]
        if row == M.EXPERT:
            a, fault = orc.expert_action(i)
            if fault:
                out["bot_raised"] = True
                break
            entry = (a, np.nan, 0, 255, 0, np.nan, 1, side, -1, -1)
        else:
            g, scores, mask = orc.decide(i, weights[row])
            legal = legal_list(mask)
            out["decisions"] += 1
            out["lookahead"] += len(legal)
            a, explored, rank = g, False, -1
            if explore is not None and explore.may_explore(side, steps):
                explored, r = draw(explore, seed, steps, len(legal))
                if explored:
                    a, rank = legal[r], r
            entry = (a, scores[g], len(legal), g, int(explored), scores[a], 0, side, rank, legal.index(g))
        fault = orc.step(i, a)[0]
        steps += 1
        if not fault and orc.observe(i) is None:
            fault = M.FAULT_INT_CARD
        for c, v in zip(cols, entry):
            out[c].append(v)
        if fault:
            break
    if not fault and orc.have_winner(i):
        out["result"] = M.result_of(orc, i)
    gf = orc.game_fault(i)   # a capacity code, if a look-ahead (or the stopping step) met one
    out.update(steps=steps, fault=fault, final=orc.canon_hash(i),
               reported=fault if fault >= M.CAPACITY_CODE else (gf if gf >= M.CAPACITY_CODE else fault))
    return out


class ModelEngine:
    """rollout_logged(..., explore=) and rollout_faults of a BatchEngine on one record of the oracle (0 standard, 1
    extended, 2 large).  games: the dict of every game of the last call."""

    def __init__(self, tier=0):
        self.tier = tier
        self.orc = oracle_lib.Oracle(1, extended=tier)
        self.calls = []   # (number of matches, their seeds) of every call

    def rollout_logged(self, weights, matches, deck_pairs, max_turns, scores=True, n_legal=True, explore=None):
        deck_pairs = np.asarray(deck_pairs, dtype=np.uint8).reshape(-1, 2, 12)
        n = len(matches)
        counts = np.zeros((len(weights), 3), dtype=np.int32)
        results = np.zeros(n, dtype=np.int8)
        log = RolloutLog.empty(n, max_turns, scores, n_legal, explore is not None)
        self.faults, self.finals, self.games = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint64), []
        for k, m in enumerate(matches):
            d = deck_pairs[int(m["deck"])]
            g = play(self.orc, 0, int(m["seed"]), d[0], d[1], (int(m["p1"]), int(m["p2"])), weights, max_turns, explore)
            self.games.append(g)
            ln = g["steps"]
            assert len(g["action"]) == ln
            results[k], log.steps[k], self.faults[k], self.finals[k] = g["result"], ln, g["reported"], g["final"]
            log.action[k, :ln] = g["action"]
            if scores:
                log.score[k, :ln] = g["score"]
            if n_legal:
                log.n_legal[k, :ln] = g["n_legal"]
            if explore is not None:
                log.greedy[k, :ln], log.explored[k, :ln], log.taken_score[k, :ln] = g["greedy"], g["explored"], g["taken_score"]
            row, win = M.individual(int(m["p1"]), int(m["p2"]))
            if row >= 0:
                counts[row] += (g["result"] == win, g["result"] == -1, 1)
        self.calls.append((n, np.array(matches["seed"])))
        return counts, results, log.steps, log

    def rollout_faults(self, n):
        assert n == len(self.faults)
        return self.faults


def _same_f64(a, b):
    """Bit for bit where either holds a number (the padding NaN of the device is all ones, numpy's is not)."""
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


def same_log(a, b):
    """Two RolloutLogs of exploring rollouts equal entry by entry: every integer array, and score / taken_score bit for bit."""
    ints = all(np.array_equal(getattr(a, c), getattr(b, c)) for c in ("action", "steps", "n_legal", "greedy", "explored"))
    return ints and _same_f64(a.score, b.score) and _same_f64(a.taken_score, b.taken_score)
