"""Game logs: what a rollout played, step by step (monsoon_rollout_logged, BatchEngine.rollout_logged).

logged_rollout plays a schedule over the record tiers as fitness.tiered_rollout does and keeps every game's log;
FitnessEvaluator.logged_games is its entry over an evaluator's own engines; replay plays logged games again through the
step interface and yields the (state, action) pairs a learner wants.
"""
import numpy as np

from .engine import RolloutLog
from .fitness import _ladder, bot_plays


def logged_rollout(engine_for_tier, weights, matches, deck_pairs, max_turns):
    """A schedule played on the smallest record each game needs, with its log.  engine_for_tier(tier) is the engine of a
    record (0 standard, 1 extended, 2 large): anything with BatchEngine's rollout_logged and rollout_faults.  The rule is
    fitness.tiered_rollout's, the same function (fitness._ladder): a deck pair holding ua20 / b005 starts on the extended
    record, a game that ends on a limit of its record (fitness.record_limited) is played again on the next larger one, and
    its rows -- the log's among them -- are replaced.  An engine is handed only the deck pairs its sub-schedule names.
    Returns (counts[n_rows][3], results, steps, faults, log)."""
    log = RolloutLog.empty(len(matches), max_turns)

    def play(t, sub, sub_pairs):
        eng = engine_for_tier(t)
        c, r, s, lg = eng.rollout_logged(weights, sub, sub_pairs, max_turns)
        return c, r, s, eng.rollout_faults(len(sub)), lg
    return _ladder(play, len(weights), matches, deck_pairs, put=log.put)[:4] + (log,)


def replay(engine, matches, deck_pairs, log):
    """Logged, bot-free games played again in lock-step through engine.reset / legal_mask / step (a generator).  Before
    every step it yields (live, to_play, legal_mask, observation, action): live bool[n] = the games that still have an
    entry, to_play int[n], legal_mask uint64[n][3], observation int32[n][27][5][4] and action uint8[n] (255 where not
    live) -- the (state, action) pairs of every decision.  A game past its last entry gets no further step.  The
    generator's return value (StopIteration.value, or `hashes = yield from replay(...)`) is the final state_hash().

    ValueError: a logged action that is not legal where it is replayed, and a match with the scripted bot on a side --
    the bot's choice draws from the game's own stream (expert_action consumes it), which step alone does not reproduce,
    so such a game cannot be replayed from its actions."""
    matches = np.asarray(matches)
    if bot_plays(matches):
        raise ValueError("replay: a match with the scripted bot cannot be replayed from its actions (the bot draws from the game's stream)")
    deck_pairs = np.asarray(deck_pairs, dtype=np.uint8).reshape(-1, 2, 12)
    n = len(matches)
    if log.action.shape[0] != n:
        raise ValueError("replay: one log row per match")
    engine.reset(matches["seed"], deck_pairs[matches["deck"]])
    steps = np.asarray(log.steps)
    for k in range(int(steps.max()) if n else 0):
        live = steps > k
        action = np.where(live, log.action[:, k], 255).astype(np.uint8)
        mask = engine.legal_mask()
        ok = (mask[np.arange(n), np.minimum(action, 155) >> 6] >> (np.minimum(action, 155) & 63).astype(np.uint64)) & np.uint64(1)
        bad = np.nonzero(live & ((ok == 0) | (action > 155)))[0]
        if len(bad):
            raise ValueError(f"replay: action {int(action[bad[0]])} of game {int(bad[0])} is not legal at its step {k}")
        yield live, engine.status()[:, 0], mask, engine.observe()[0], action
        engine.step(action)
    return engine.state_hash()
