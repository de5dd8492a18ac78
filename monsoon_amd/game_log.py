"""Game logs: what a rollout played, step by step (monsoon_rollout_logged, BatchEngine.rollout_logged).

logged_rollout plays a schedule over the record tiers as fitness.tiered_rollout does and keeps every game's log;
FitnessEvaluator.logged_games is its entry over an evaluator's own engines; replay plays logged games again through the
step interface and yields the (state, action) pairs a learner wants; dataset / dataset_batches / step_sides play them
again on the device (monsoon_replay_logged_dev), games with the scripted bot included, into torch tensors of rows; with a
candidate column (CANDIDATE_COLUMNS) every row also carries the afterstates of its state (monsoon_replay_logged_after_dev),
which candidates / candidate_mask hand to vec_env.select_actions and to a learner over afterstate features.  A rollout
with an engine.Explore rule logs games that leave the champion's line; its log keeps the arg-max of every decision
(greedy) and which decisions explored, explore_draws recomputes the draws, and dataset hands both out as row columns
(LOG_COLUMNS).  A rollout with an engine.Policies table (a rule per individual) logs the softmax weights of every decision
its rule covers; behaviour_prob turns them into the probability the behaviour policy gave each committed action.
"""
import numpy as np

from . import _lib
from .engine import RolloutLog
from .fitness import _ladder, bot_plays, hash32_array


def explore_draws(explore, match_seeds, k, n_legal):
    """The draws of monsoon_rollout_explore for decisions at committed-step index k of matches with the seeds match_seeds
    over n_legal legal actions (broadcastable integer arrays): (explores bool, rank int64) -- explores = draw0 <
    explore.threshold, rank = the position in the ascending legal list that an exploring decision commits.  Only the draw
    is tested: whether the side may explore and the step limit (Explore.may_explore) are the caller's to apply."""
    seeds, k, n_legal = np.broadcast_arrays(np.asarray(match_seeds, dtype=np.uint64), np.asarray(k, dtype=np.uint64), np.asarray(n_legal, dtype=np.uint64))
    draw0, draw1 = hash32_array(explore.seed, seeds, k, 0), hash32_array(explore.seed, seeds, k, 1)
    return draw0 < np.uint32(explore.threshold), ((draw1.astype(np.uint64) * n_legal) >> np.uint64(32)).astype(np.int64)


# c_k = the double nearest 1 / k!, k = 0 .. 10 (monsoon_amd/csrc/sample_weight.h)
_INV_FACTORIAL = (1.0, 1.0, 1.0 / 2, 1.0 / 6, 1.0 / 24, 1.0 / 120, 1.0 / 720, 1.0 / 5040, 1.0 / 40320, 1.0 / 362880, 1.0 / 3628800)
SAMPLE_ONE = 1 << 24   # the weight of a decision's arg-max and of every action tied with it


def sample_weights(scores, best, inv_temperature):
    """The weights of monsoon_rollout_sample (include/monsoon.h), the numpy statement of the device's arithmetic, bit for
    bit: x = (scores - best) * inv_temperature, two operations each rounded once, then weight24(x) = floor(exp(x) * 2**24)
    by range reduction, a degree-10 polynomial in Horner form, ldexp and floor -- plain *, +, - only, which numpy never
    fuses.  scores, best, inv_temperature broadcast to any shape; returns uint32 of that shape, 0 where x is NaN, -inf or
    < -32.  (x > 0 does not occur for a decision's scores against its best score.)"""
    scores, best, inv_t = np.broadcast_arrays(np.asarray(scores, dtype=np.float64), np.asarray(best, dtype=np.float64),
                                              np.asarray(inv_temperature, dtype=np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        x = (scores - best) * inv_t
        live = x >= -32.0   # (False for a NaN)
        x = np.where(live, x, 0.0)
        n = np.floor(x * float.fromhex("0x1.71547652b82fep+0") + 0.5)
        r = (x - n * float.fromhex("0x1.62e42feep-1")) - n * float.fromhex("0x1.a39ef35793c76p-33")
        p = np.full(x.shape, _INV_FACTORIAL[10])
        for k in range(9, -1, -1):
            p = p * r + _INV_FACTORIAL[k]
        w = np.floor(np.ldexp(p, n.astype(np.int32) + 24))
    return np.where(live, w, 0.0).astype(np.uint32)


def sample_rank(weights, draw1):
    """j* of monsoon_rollout_sample over the weights of one decision's ascending legal list (uint32[n_legal]) and its
    draw1: r = (draw1 * total) >> 32, the smallest j whose inclusive prefix sum exceeds r (so an action of weight 0 is never
    taken, and r equal to a prefix goes to the next action).  -1 where the weights sum to 0."""
    prefix = np.cumsum(np.asarray(weights, dtype=np.uint64))
    total = int(prefix[-1]) if len(prefix) else 0
    if total == 0:
        return -1
    return int(np.searchsorted(prefix, (int(draw1) * total) >> 32, side="right"))


def logged_rollout(engine_for_tier, weights, matches, deck_pairs, max_turns, explore=None):
    """A schedule played on the smallest record each game needs, with its log.  engine_for_tier(tier) is the engine of a
    record (0 standard, 1 extended, 2 large): anything with BatchEngine's rollout_logged and rollout_faults.  The rule is
    fitness.tiered_rollout's, the same function (fitness._ladder): a deck pair that cards.needs_extended_each names (ua20 / b005, a unit or structure card twice) starts on the extended
    record, a game that ends on a limit of its record (fitness.record_limited) is played again on the next larger one, and
    its rows -- the log's among them -- are replaced.  An engine is handed only the deck pairs its sub-schedule names.
    explore = an engine.Explore: every tier plays with that rule (the draws are keyed by the match's seed and the step, so a
    game played again on a larger record explores as it did on the smaller one) and the log carries greedy, explored and
    taken_score; the counts then describe explored games, not fitness.  A rule with a temperature (the sampling rule) goes
    through the tiers the same way, and the log carries weight_total and taken_weight too.  An engine.Policies (a rule per
    row of `weights`, monsoon_rollout_policies) likewise: a sub-schedule keeps its row indices, so every tier reads the same table.
    Returns (counts[n_rows][3], results, steps, faults, log)."""
    log = RolloutLog.empty(len(matches), max_turns, explore=explore is not None,
                           sample=explore is not None and getattr(explore, "samples", False))
    how = {} if explore is None else {"explore": explore}

    def play(t, sub, sub_pairs):
        eng = engine_for_tier(t)
        c, r, s, lg = eng.rollout_logged(weights, sub, sub_pairs, max_turns, **how)
        return c, r, s, eng.rollout_faults(len(sub)), lg
    return _ladder(play, len(weights), matches, deck_pairs, put=log.put)[:4] + (log,)


def behaviour_prob(policies, matches, log, sides):
    """float64[n][max_turns]: the probability with which the behaviour policy of a rollout under `policies` (an
    engine.Policies) committed each logged action.  sides = (to_play, bot) as step_sides returns them.  A decision of weight
    row r (p1 of its match when FIRST played, p2 when SECOND did) that the rule covers -- the side's bit, the step limit,
    thresholds[r] > 0 -- with weight_total > 0 has, with eps_r = thresholds[r] / 2**32,
        mu = (1 - eps_r) * [action == greedy] + eps_r * taken_weight / weight_total,
    sampled or not (include/monsoon.h monsoon_rollout_policies).  Every other decision committed its arg-max: 1.0.  Steps of
    the scripted bot, entries the replay did not reach and the padding are NaN."""
    if not getattr(policies, "per_individual", False) or log.weight_total is None or log.taken_weight is None or log.greedy is None:
        raise ValueError("behaviour_prob needs an engine.Policies and the log of a rollout under it")
    to_play, bot = (np.asarray(a) for a in sides)
    matches = np.asarray(matches)
    if to_play.shape != log.action.shape or bot.shape != log.action.shape or len(matches) != len(to_play):
        raise ValueError("behaviour_prob: sides has the shape of the log, one row per match")
    k = np.arange(log.action.shape[1])[None, :]
    decision = (to_play >= 0) & ~bot.astype(bool) & (k < np.asarray(log.steps)[:, None])
    row = np.where(to_play == 0, matches["p1"][:, None], matches["p2"][:, None])
    row = np.where(decision, row, 0)   # (a bot's -1 indexes nothing)
    if decision.any() and not (0 <= row[decision].min() and row[decision].max() < len(policies)):
        raise ValueError("behaviour_prob: a match names a row outside the Policies table")
    threshold = policies.thresholds[row]
    covered = decision & policies.may_explore(np.maximum(to_play, 0), k) & (threshold > 0) & (log.weight_total > 0)
    eps = threshold.astype(np.float64) / 2.0**32
    ratio = np.zeros(log.action.shape)
    np.divide(log.taken_weight, log.weight_total, out=ratio, where=covered)
    out = np.full(log.action.shape, np.nan)
    out[decision] = 1.0
    out[covered] = ((1.0 - eps) * (log.action == log.greedy) + eps * ratio)[covered]
    return out


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


# ---- replay on the device: (observation, action) rows as torch tensors -----------------------------------------------
# name -> (torch dtype, shape of a row): the columns of monsoon_replay_rows.  state_hash holds the bits of the uint64 that
# state_hash() reports (view it as uint64 on the host: t.cpu().numpy().view(numpy.uint64)).
COLUMNS = {"obs": ("int32", (27, 5, 4)), "legal": ("uint8", (156,)), "obs_raises": ("uint8", ()), "to_play": ("uint8", ()),
           "action": ("uint8", ()), "bot": ("uint8", ()), "game": ("int32", ()), "step": ("int32", ()), "state_hash": ("int64", ())}
ROW_BYTES = {"obs": 2160, "legal": 156, "obs_raises": 1, "to_play": 1, "action": 1, "bot": 1, "game": 4, "step": 4, "state_hash": 8}
# ... those gathered on the host from the arrays of an exploring rollout's log at the kept entries (no replay involved):
# greedy is the teacher's label of a row whose action was explored, explored marks such rows
# ; weight_total and taken_weight are a sampling rollout's or a Policies rollout's (the log's uint32 values, as int64 tensors)
LOG_COLUMNS = {"greedy": ("uint8", ()), "explored": ("uint8", ()), "weight_total": ("int64", ()), "taken_weight": ("int64", ())}
# ... and of monsoon_replay_after, "K" = max_after: the candidates the row's choice was made among, entry k the k-th legal
# action in ascending order.  Naming one of them turns the look-ahead on; _CANDIDATE_BASE comes along, as action does.
CANDIDATE_COLUMNS = {"n_legal": ("int32", ()), "chosen": ("int16", ()), "after_action": ("uint8", ("K",)), "after_status": ("uint8", ("K",)),
                     "after_reward": ("int8", ("K",)), "after_winner": ("int8", ("K",)), "after_features": ("float64", ("K", 10)),
                     "before_features": ("float64", (10,)), "after_obs": ("int32", ("K", 27, 5, 4))}
_CANDIDATE_BASE = ("n_legal", "after_action", "after_status")   # what it takes to read any other candidate column
_AFTER_FIELD = {"n_legal": "n_legal", "chosen": "chosen", "after_action": "action", "after_status": "status", "after_reward": "reward",
                "after_winner": "winner", "after_features": "features", "before_features": "before_features", "after_obs": "obs"}


def kept_counts(steps, keep=None):
    """int64[n]: the rows each game gets -- its entries k < steps[g], those with keep[g][k] != 0 if a mask is given."""
    steps = np.asarray(steps, dtype=np.int64)
    if keep is None:
        return steps.copy()
    keep = np.asarray(keep)
    if keep.ndim != 2 or keep.shape[0] != len(steps) or (len(steps) and int(steps.max()) > keep.shape[1]):
        raise ValueError("keep: one row per game, at least as long as the game")
    return ((keep != 0) & (np.arange(keep.shape[1])[None, :] < steps[:, None])).sum(axis=1).astype(np.int64)


def row_bases(steps, keep=None):
    """(base int64[n], S): rows are in match order, then entry order -- game g's first kept entry is row base[g], S rows in all."""
    counts = kept_counts(steps, keep)
    ends = np.cumsum(counts)
    return ends - counts, int(ends[-1]) if len(ends) else 0


def batch_cuts(counts, max_rows):
    """[(g0, g1), ...]: the games cut into runs of whole consecutive games, each as long as max_rows rows allow (greedy).
    ValueError if one game alone has more rows than max_rows."""
    cuts, g0, rows = [], 0, 0
    for g, c in enumerate(np.asarray(counts, dtype=np.int64).tolist()):
        if c > max_rows:
            raise ValueError(f"dataset_batches: game {g} alone has {c} rows, max_rows is {max_rows}")
        if rows + c > max_rows:
            cuts.append((g0, g))
            g0, rows = g, 0
        rows += c
    if g0 < len(counts):
        cuts.append((g0, len(counts)))
    return cuts


def outcome(results, game, to_play):
    """+1 / 0 / -1 per row, from the side to play: results[n] is the rollout's (-1 a draw, 0 FIRST won, 1 SECOND won), game
    the rows' match index (an index array of the results' library), to_play their side.  Works on numpy arrays and on
    torch tensors alike; the caller casts the result."""
    r = results[game]
    return (r >= 0) * (1 - 2 * (r != to_play))


def _want(columns):
    columns = tuple(columns)
    bad = [c for c in columns if c not in COLUMNS and c not in CANDIDATE_COLUMNS and c not in LOG_COLUMNS]
    if bad:
        raise ValueError(f"unknown column(s) {bad}: choose from {tuple(COLUMNS) + tuple(CANDIDATE_COLUMNS) + tuple(LOG_COLUMNS)}")
    if "action" not in columns:
        columns += ("action",)
    if any(c in CANDIDATE_COLUMNS for c in columns):
        columns += tuple(c for c in _CANDIDATE_BASE if c not in columns)
    return columns


def _max_after(names, max_after):
    """K of a call over the columns `names`: 0 without a candidate column, else max_after, which must be an integer in 1..156."""
    if not any(c in CANDIDATE_COLUMNS for c in names):
        return 0
    if isinstance(max_after, bool) or not isinstance(max_after, (int, np.integer)) or not 1 <= max_after <= 156:
        raise ValueError("a candidate column needs max_after, an integer in 1..156")
    return int(max_after)


def _tensors(engine, names, cap, max_after=0):
    import torch
    dev = torch.device("cuda", engine.device)
    out = {}
    for c in names:
        dt, shape = COLUMNS[c] if c in COLUMNS else LOG_COLUMNS[c] if c in LOG_COLUMNS else CANDIDATE_COLUMNS[c]
        shape = tuple(max_after if d == "K" else d for d in shape)
        out[c] = torch.empty((max(int(cap), 1),) + shape, dtype=getattr(torch, dt), device=dev)
    return out


def _replay_into(engine, tensors, matches, deck_pairs, action, steps, keep, max_after=0):
    """One monsoon_replay_logged_dev / _after_dev call into the first rows of `tensors`: (rows, status, replayed, fault)."""
    import torch
    torch.cuda.current_stream(tensors["action"].device).synchronize()   # the library works on the handle's stream
    rows = _lib.ReplayRows(**{c: t.data_ptr() for c, t in tensors.items() if c in COLUMNS})
    after = None
    if max_after:
        after = _lib.ReplayAfter(**{_AFTER_FIELD[c]: t.data_ptr() for c, t in tensors.items() if c in CANDIDATE_COLUMNS})
    return engine.replay_logged(matches, deck_pairs, action, steps, rows, tensors["action"].shape[0], keep, after, max_after)


def _log_columns(log, names):
    """The LOG_COLUMNS among `names`; ValueError where the log does not have their arrays."""
    want = [c for c in names if c in LOG_COLUMNS]
    missing = [c for c in want if getattr(log, c, None) is None]
    if missing:
        raise ValueError(f"column(s) {missing} need the log of a rollout with an Explore rule (rollout_logged(..., explore=); "
                         "weight_total / taken_weight: one with a temperature or a Policies table)")
    return want


def _gather_log(tensors, log, want, steps, keep, a=0, b=None):
    """Fill the LOG_COLUMNS `want` of `tensors` from the arrays of games [a, b) of `log` at the kept entries, in row order
    (match order, then entry order)."""
    import torch
    if not want:
        return
    steps = np.asarray(steps, dtype=np.int64)
    sel = np.arange(log.action.shape[1])[None, :] < steps[:, None]
    if keep is not None:
        sel &= np.asarray(keep)[:, :sel.shape[1]] != 0
    for c in want:
        vals = np.ascontiguousarray(getattr(log, c)[a:b][sel], dtype=LOG_COLUMNS[c][0])   # (boolean indexing is row-major: the documented row order)
        tensors[c][:len(vals)] = torch.as_tensor(vals, device=tensors[c].device)


def _columns_for(columns, results):
    names = _want(columns)
    if results is not None:
        names += tuple(c for c in ("game", "to_play") if c not in names)
    return names


def candidates(d):
    """The candidate columns of dataset rows as the dict VecEnv.afterstates returns, a row for a slot: action, status,
    n_legal, and whichever of reward, winner, features, obs the rows carry -- so vec_env.select_actions(candidates(d),
    values) picks per row among its legal actions as it does per slot.  Views, no copy; works on CPU tensors too."""
    if "after_action" not in d:
        raise ValueError("candidates: the rows carry no candidate column (dataset(..., columns=(..., 'after_features'), max_after=K))")
    names = {"action": "after_action", "status": "after_status", "n_legal": "n_legal", "reward": "after_reward", "winner": "after_winner",
             "features": "after_features", "obs": "after_obs"}
    return {k: d[c] for k, c in names.items() if c in d}


def candidate_mask(d):
    """bool [S][K]: the entries of the rows' candidates that exist (k < min(n_legal, K)) and have features and an
    observation (status == 0) -- what a loss over after_features / after_obs is masked with.  Pure torch."""
    import torch
    c = candidates(d)
    k = c["action"].shape[1]
    return (torch.arange(k, device=c["action"].device)[None, :] < c["n_legal"][:, None]) & (c["status"] == 0)


def _hand_out(tensors, columns, n_rows, results, status, replayed, fault):
    import torch
    out = {c: tensors[c][:n_rows] for c in _want(columns)}
    if results is not None:
        res = torch.as_tensor(np.ascontiguousarray(results, dtype=np.int8), device=tensors["action"].device)
        out["outcome"] = outcome(res, tensors["game"][:n_rows].long(), tensors["to_play"][:n_rows]).to(torch.int8)
    out.update(status=status, replayed=replayed, fault=fault)
    return out


def dataset(engine, matches, deck_pairs, log, keep=None, columns=tuple(COLUMNS), results=None, max_after=64):
    """The (state, action) rows of logged games as torch CUDA tensors, replayed on the device by `engine` (games with the
    scripted bot included: its expert_action runs again and consumes the stream as it did).  One row per entry k <
    log.steps[g] (with keep uint8 / bool [n][T]: per entry with keep[g][k]), in match order, then entry order, holding the
    state BEFORE the step: a dict of the chosen `columns` (COLUMNS; action always) plus the host arrays status uint8[n]
    (_lib.REPLAY_*: 0 = replayed to its last entry), replayed int32[n] and fault uint8[n].  The rows of a game that
    stopped early read action 255 from the stop on; their other columns are unspecified.  results int8[n] (the rollout's)
    adds outcome int8[S]: +1 / 0 / -1 from the side to play.

    Over the log of a rollout with an Explore rule the names of LOG_COLUMNS are accepted too: greedy uint8[S], the arg-max
    action of the row's decision (255 on a bot step) -- the teacher's label where `action` was explored -- and explored
    uint8[S]; both are gathered on the host from the log's arrays at the kept entries, in row order.  The replay itself
    takes an explored action as it takes any legal one.

    A name of CANDIDATE_COLUMNS in `columns` turns the look-ahead on (monsoon_replay_logged_after_dev): the row also carries
    the successor of every legal action of its state, K = max_after (1..156) entries, entry k the k-th legal action in
    ascending order, in the meaning of VecEnv.afterstates -- n_legal int32[S] (the full count, also beyond K), chosen
    int16[S] (the rank of `action` in that order, -1 for a PASS outside the legal set), after_action / after_status uint8
    [S][K], after_reward / after_winner int8[S][K], after_features float64[S][K][10], before_features float64[S][10] (zeros
    where the row's observation raises), after_obs int32[S][K][27][5][4].  n_legal, after_action and after_status come
    along, as action does; entries k >= min(n_legal, K) read after_action 255 and are otherwise unspecified, as are the
    features and observation of an entry with after_status != 0 (candidate_mask).  Per row that is 80 * K bytes of
    after_features and 2 160 * K of after_obs (K = 64: 5 KB and 138 KB), so ask for after_obs through dataset_batches.
    Without such a name max_after is not read and the call is what it was.

    torch has to be imported before the engine is created, for the reason VecEnv.__init__ gives (it has to load its own
    ROCm runtime first): `import torch` before the first BatchEngine(...) of the process."""
    import torch
    if not torch.cuda.is_available():
        raise _lib.MonsoonError("dataset: torch sees no device -- import torch before the first BatchEngine is created")
    matches = np.asarray(matches)
    if log.action.shape[0] != len(matches):
        raise ValueError("dataset: one log row per match")
    _, total = row_bases(log.steps, keep)
    names = _columns_for(columns, results)
    k_after = _max_after(names, max_after)
    from_log = _log_columns(log, names)
    tensors = _tensors(engine, names, total, k_after)
    n_rows, status, replayed, fault = _replay_into(engine, tensors, matches, deck_pairs, log.action, log.steps, keep, k_after)
    _gather_log(tensors, log, from_log, log.steps, keep)
    return _hand_out(tensors, columns, n_rows, results, status, replayed, fault)


def dataset_batches(engine, matches, deck_pairs, log, max_rows, keep=None, columns=tuple(COLUMNS), results=None, max_after=64):
    """dataset over a log too large for one set of tensors (65 536 games are about 30 GB of observations): a generator over
    runs of whole consecutive games whose rows fit max_rows (batch_cuts), each item dataset's dict for that run plus
    games = (g0, g1); game holds the index into the whole schedule.  ONE set of tensors is allocated and every item is a
    view of it: the next item overwrites the one before, so use or copy an item before asking for the next.
    Candidate columns and max_after as in dataset.  ValueError if one game alone has more than max_rows rows."""
    import torch
    if not torch.cuda.is_available():
        raise _lib.MonsoonError("dataset_batches: torch sees no device -- import torch before the first BatchEngine is created")
    matches = np.asarray(matches)
    counts = kept_counts(log.steps, keep)
    cuts = batch_cuts(counts, max_rows)
    cap = max((int(counts[a:b].sum()) for a, b in cuts), default=0)
    names = _columns_for(columns, results)
    k_after = _max_after(names, max_after)
    from_log = _log_columns(log, names)
    tensors = _tensors(engine, names, cap, k_after)
    for a, b in cuts:
        keep_ab = None if keep is None else np.asarray(keep)[a:b]
        n_rows, status, replayed, fault = _replay_into(engine, tensors, matches[a:b], deck_pairs, log.action[a:b], log.steps[a:b], keep_ab, k_after)
        _gather_log(tensors, log, from_log, log.steps[a:b], keep_ab, a, b)
        if "game" in tensors:
            tensors["game"][:n_rows] += a
        item = _hand_out(tensors, columns, n_rows, results, status, replayed, fault)
        item["games"] = (a, b)
        yield item


def step_sides(engine, matches, deck_pairs, log):
    """(to_play int8[n][T], bot bool[n][T]) on the host: who played entry k of game g (-1 behind the game's last replayed
    entry) and whether it was the scripted bot -- from a columns-only replay without observations.  What a keep mask is
    built from: the winner's decisions only, no bot steps, every 4th entry, ..."""
    d = dataset(engine, matches, deck_pairs, log, columns=("to_play", "bot", "game", "step"))
    cols = {c: d[c].cpu().numpy() for c in ("to_play", "bot", "game", "step", "action")}
    to_play = np.full(log.action.shape, -1, dtype=np.int8)
    bot = np.zeros(log.action.shape, dtype=bool)
    reached = cols["action"] != 255
    g, k = cols["game"][reached], cols["step"][reached]
    to_play[g, k] = cols["to_play"][reached]
    bot[g, k] = cols["bot"][reached] != 0
    return to_play, bot
