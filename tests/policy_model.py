"""The contract of monsoon_rollout_policies (include/monsoon.h) over the CPU oracle: sample_model.play's loop with the rule of
the weight row that moves, and with the weights written down on every decision that rule covers.  Test infrastructure only.

    k = 0
    while not have_winner() and k < max_turns:
        if to_play() is the bot:  a = expert_action()
        else:
            r = the mover's row; g, scores, mask = decide(weights[r]); legal = sorted(mask)
            a = g
            if side's bit and (until_step <= 0 or k < until_step) and thresholds[r] > 0:          # covered
                w = sample_weights(scores[legal], scores[g], inv_temperatures[r]); total = sum(w)
                taken = 2**24 if total else 0                                                     # the arg-max's weight
                if hash32(seed, match seed, k, 0) < thresholds[r] and total:
                    j = sample_rank(w, hash32(seed, match seed, k, 1)); a = legal[j]; taken = w[j]
        step(a); k += 1

ModelEngine has BatchEngine's rollout_logged(..., explore=) / rollout_faults over it, so game_log.logged_rollout runs on
the CPU, ladder included."""
import numpy as np

import explore_model as X
import oracle_lib
import sample_model as S
import vs_expert_model as M
from monsoon_amd import game_log
from monsoon_amd.engine import RolloutLog
from monsoon_amd.fitness import hash32

ONE = S.ONE


def play(orc, i, seed, deck0, deck1, rows, weights, max_turns, policies):
    """One game on slot i of `orc` under `policies` (an engine.Policies).  Returns sample_model.play's dict -- weight_total and
    taken_weight on every covered decision -- plus per committed step row (the mover's weight row, -1 for the bot), covered,
    and legal_scores (the scores of the ascending legal list, None for the bot)."""
    out = dict(result=-1, steps=0, fault=0, reported=0, bot_raised=False, decisions=0, lookahead=0)
    cols = ("action", "score", "n_legal", "greedy", "explored", "taken_score", "bot", "side", "rank", "greedy_rank", "weight_total",
            "taken_weight", "zero_weight", "tie", "min_weight", "row", "covered", "legal_scores")
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
            entry = (a, np.nan, 0, 255, 0, np.nan, 1, side, -1, -1, 0, 0, False, False, -1, -1, False, None)
        else:
            g, scores, mask = orc.decide(i, weights[row])
            legal = X.legal_list(mask)
            out["decisions"] += 1
            out["lookahead"] += len(legal)
            a, explored, rank, total, taken, zero, tie, low = g, False, -1, 0, 0, False, False, -1
            threshold = int(policies.thresholds[row])
            covered = bool(policies.may_explore(side, steps)) and threshold > 0
            if covered:
                w = game_log.sample_weights(np.asarray(scores)[legal], scores[g], policies.inv_temperatures[row])
                total = int(w.astype(np.uint64).sum())
                explored = hash32(policies.seed, seed, steps, 0) < threshold
                if total:
                    taken = ONE
                    zero, tie, low = bool((w == 0).any()), int((w == ONE).sum()) >= 2, int(w.min())
                    if explored:
                        rank = game_log.sample_rank(w, hash32(policies.seed, seed, steps, 1))
                        a, taken = legal[rank], int(w[rank])
            entry = (a, scores[g], len(legal), g, int(explored), scores[a], 0, side, rank, legal.index(g), total, taken, zero, tie, low, row,
                     covered, np.asarray(scores)[legal])
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
    extended, 2 large), for a Policies table.  games: the dict of every game of the last call."""

    def __init__(self, tier=0):
        self.tier = tier
        self.orc = oracle_lib.Oracle(1, extended=tier)

    def rollout_logged(self, weights, matches, deck_pairs, max_turns, scores=True, n_legal=True, explore=None):
        assert explore is not None and explore.per_individual and len(explore) == len(weights)
        deck_pairs = np.asarray(deck_pairs, dtype=np.uint8).reshape(-1, 2, 12)
        n = len(matches)
        counts = np.zeros((len(weights), 3), dtype=np.int32)
        results = np.zeros(n, dtype=np.int8)
        log = RolloutLog.empty(n, max_turns, scores, n_legal, sample=True)
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
            log.greedy[k, :ln], log.explored[k, :ln], log.taken_score[k, :ln] = g["greedy"], g["explored"], g["taken_score"]
            log.weight_total[k, :ln], log.taken_weight[k, :ln] = g["weight_total"], g["taken_weight"]
            row, win = M.individual(int(m["p1"]), int(m["p2"]))
            if row >= 0:
                counts[row] += (g["result"] == win, g["result"] == -1, 1)
        return counts, results, log.steps, log

    def rollout_faults(self, n):
        assert n == len(self.faults)
        return self.faults


def sides_of(games, shape):
    """(to_play int8[n][T], bot bool[n][T]) of the model's games, as game_log.step_sides reports a device log's."""
    to_play, bot = np.full(shape, -1, dtype=np.int8), np.zeros(shape, dtype=bool)
    for i, g in enumerate(games):
        to_play[i, :g["steps"]], bot[i, :g["steps"]] = g["side"], np.array(g["bot"], dtype=bool)
    return to_play, bot
