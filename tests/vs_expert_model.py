"""The contract of monsoon_rollout_vs_expert (include/monsoon.h) as a few lines of Python over the CPU oracle: a rollout in
which a side whose weight row is EXPERT (-1) is the reference's scripted bot.  Test infrastructure only.

    steps = 0
    while not have_winner() and steps < max_turns:
        if to_play() is the bot:  a = expert_action()      (raises -> a draw with that code, nothing is stepped)
        else:                     a = decide(weights[row])
        step(a); steps += 1                                (faults, or the observation raises -> a draw with that code)

vs_expert_rollout_fn is the FitnessEvaluator `rollout_fn` stand-in built on it (tests/oracle_rollout.py knows no bot)."""
import numpy as np

import oracle_lib
from vec_env_model import bases

EXPERT = -1
FAULT_INT_CARD = 2
CAPACITY_CODE = 16


def result_of(orc, i):
    """The one result rule: FIRST wins iff SECOND's base < 0 <= FIRST's base, SECOND likewise, else a draw."""
    b0, b1 = bases(orc.canon(i))
    return 0 if (b1 < 0 <= b0) else 1 if (b0 < 0 <= b1) else -1


def play(orc, i, seed, deck0, deck1, rows, weights, max_turns, trace=False):
    """One game on slot i of `orc`.  rows = (p1, p2): weight rows, EXPERT = the bot.  Returns a dict: result (-1 / 0 / 1),
    steps (all committed steps), fault (the code that stopped the game, 0 = none), reported (what monsoon_rollout_faults
    reports: a capacity code a look-ahead met takes precedence over a reference exception), bot_raised, decisions,
    lookahead, final (canonical hash); with trace also actions / bots / hashes per step (a raising bot leaves a last entry
    of action 255) and shashes per heuristic decision (hash of the scores over the sorted legal list)."""
    out = dict(result=-1, steps=0, fault=0, reported=0, bot_raised=False, decisions=0, lookahead=0, actions=[], bots=[], hashes=[], shashes=[])
    f = orc.reset(i, seed, deck0, deck1)
    if f:   # (the engine refuses the decks: no game)
        out.update(fault=f, reported=f, final=orc.canon_hash(i))
        return out
    steps = fault = 0
    while not orc.have_winner(i) and steps < max_turns:
        row = rows[orc.to_play(i)]
        if row == EXPERT:
            a, fault = orc.expert_action(i)
            if fault:
                out["bot_raised"] = True
                if trace:
                    out["actions"].append(255), out["bots"].append(1), out["hashes"].append(0)
                break
        else:
            a, scores, mask = orc.decide(i, weights[row])
            out["decisions"] += 1
            legal = [x for x in range(156) if (int(mask[x >> 6]) >> (x & 63)) & 1]
            out["lookahead"] += len(legal)
            if trace:
                out["shashes"].append(oracle_lib.fnv1a64(scores[legal].tobytes()))
        fault = orc.step(i, a)[0]
        steps += 1
        if not fault and orc.observe(i) is None:
            fault = FAULT_INT_CARD
        if trace:
            out["actions"].append(a), out["bots"].append(int(row == EXPERT)), out["hashes"].append(0 if fault else orc.canon_hash(i))
        if fault:
            break
    if not fault and orc.have_winner(i):
        out["result"] = result_of(orc, i)
    gf = orc.game_fault(i)   # a capacity code, if a look-ahead (or the stopping step) met one
    out.update(steps=steps, fault=fault, reported=fault if fault >= CAPACITY_CODE else (gf if gf >= CAPACITY_CODE else fault),
               final=orc.canon_hash(i))
    return out


def individual(p1, p2):
    """(row of the match's individual, the result that is its win), row -1 for the bot against itself."""
    return (p1, 0) if p1 >= 0 else (p2, 1)


def rollout_tier(weights, matches, deck_pairs, max_turns, tier, core=None):
    """(counts, results, steps, faults, finals) of a schedule on one record of the oracle (0 standard, 1 extended, 2 large)."""
    orc = oracle_lib.Oracle(1, extended=tier, core=core)
    deck_pairs = np.asarray(deck_pairs, dtype=np.uint8).reshape(-1, 2, 12)
    n = len(matches)
    counts = np.zeros((len(weights), 3), dtype=np.int64)
    results, steps = np.zeros(n, dtype=np.int8), np.zeros(n, dtype=np.int32)
    faults, finals = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint64)
    for k, m in enumerate(matches):
        d = deck_pairs[int(m["deck"])]
        g = play(orc, 0, int(m["seed"]), d[0], d[1], (int(m["p1"]), int(m["p2"])), weights, max_turns)
        results[k], steps[k], faults[k], finals[k] = g["result"], g["steps"], g["reported"], g["final"]
        row, win = individual(int(m["p1"]), int(m["p2"]))
        if row >= 0:
            counts[row] += (g["result"] == win, g["result"] == -1, 1)
    return counts, results, steps, faults, finals


def vs_expert_rollout_fn(weights, matches, deck_pairs, max_turns, want_results=False, want_faults=False):
    """The product's rollout (fitness._hip_rollout) on the CPU for schedules with the bot: every game on the smallest
    record its decks need, record-limited games replayed on the next larger one (fitness.tiered_rollout)."""
    from monsoon_amd.fitness import tiered_rollout
    matches = np.asarray(matches)
    counts, results, steps, faults, _, _ = tiered_rollout(
        lambda tier, sub, sub_pairs: rollout_tier(weights, sub, sub_pairs, max_turns, tier)[:4], len(weights), matches, deck_pairs)
    if want_faults:
        return counts, results, steps, faults
    return (counts, results, steps) if want_results else counts
