"""FitnessEvaluator -- Seam F: evaluate_population(population, generation) -> List[float]
(mirror of evo/fitness.py:18-259, the only call the GA driver makes into the hot path,
evo/evolution.py:88).

The reference's rollout loop is dead code (StormboundAdapter.is_terminal is always True,
evo/game_adapter.py:339-342 -> every game is scored as a player-1 win in 0 steps); it is kept as
mode="as_written".  mode="rollout" plays the games for real under the contract of SURVEY.md §8c:
    while not have_winner() and steps < max_turns: a = agent[to_play].select_action(); apply(a)
    P1 wins iff P2's base < 0 <= P1's base; P2 wins iff P1's base < 0 <= P2's base; else draw;
    a faulting committed step ends the game as a draw (evo/fitness.py:170-174, 208-210).
All games of a generation form one schedule of (p1, p2, seed, deck) entries which the HIP engine
plays monsoon_config.max_games at a time.  With torch.distributed initialised the schedule is
sharded by row individual, one process per GPU, and the per-individual {wins, draws, games}
counters are summed with one all_reduce (RCCL over xGMI on GPUs; gloo in the CPU tests).
"""
import time

import numpy as np

from .engine import MATCH_DTYPE  # noqa: F401  (defined once, next to the C ABI; engine.py needs no torch either)


def hash32(*vals):
    """Deterministic game seed from (generation, i, j, game) -- the reference uses Game(seed=None)
    (evo/fitness.py:144-145), i.e. OS entropy; a reproducible build needs an explicit seed."""
    h = 0x9E3779B9
    for v in vals:
        h ^= (int(v) + 0x7F4A7C15 + ((h << 6) & 0xFFFFFFFF) + (h >> 2)) & 0xFFFFFFFF
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        h ^= h >> 16
    return h


def hash32_array(*vals):
    """hash32 over broadcastable integer arrays (same values as the scalar form, element by element)."""
    M = np.uint64(0xFFFFFFFF)
    vals = np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in vals])
    h = np.full(vals[0].shape, 0x9E3779B9, dtype=np.uint64)
    for v in vals:
        h = h ^ ((v + np.uint64(0x7F4A7C15) + ((h << np.uint64(6)) & M) + (h >> np.uint64(2))) & M)
        h = (h * np.uint64(0x85EBCA6B)) & M
        h = h ^ (h >> np.uint64(13))
        h = (h * np.uint64(0xC2B2AE35)) & M
        h = h ^ (h >> np.uint64(16))
    return h.astype(np.uint32)


def round_robin_schedule(n_individuals, n_total_opponents, games_per_pairing, generation):
    """evo/fitness.py:53-59,133: every individual vs every other opponent (population + hall of fame)."""
    i, j, g = np.meshgrid(np.arange(n_individuals), np.arange(n_total_opponents), np.arange(games_per_pairing), indexing="ij")
    keep = (i != j).ravel()   # j < n_individuals and i == j is skipped; a hall-of-fame j is never < n_individuals when equal
    i, j, g = i.ravel()[keep], j.ravel()[keep], g.ravel()[keep]
    out = np.zeros(len(i), dtype=MATCH_DTYPE)
    out["p1"], out["p2"], out["seed"] = i, j, hash32_array(generation, i, j, g)
    return out


def ring_schedule(n_individuals, games_per_individual, generation):
    """individual i plays FIRST against (i+1+k) mod N, k = 0..games-1."""
    i, k = np.meshgrid(np.arange(n_individuals), np.arange(games_per_individual), indexing="ij")
    i, k = i.ravel(), k.ravel()
    out = np.zeros(len(i), dtype=MATCH_DTYPE)
    out["p1"], out["p2"], out["seed"] = i, (i + 1 + k) % n_individuals, hash32_array(generation, i, k)
    return out


EXPERT = -1   # MONSOON_PLAYER_EXPERT (include/monsoon.h): the reference's scripted bot as p1 / p2 of a match


def expert_schedule(n_individuals, games_per_individual, generation, sides="both"):
    """The absolute yardstick (play_vs_expert.py's tournament): individual i plays games_per_individual games against
    the scripted bot.  sides="both": game k has the individual FIRST for even k, SECOND for odd k; "first" / "second"
    fix it.  Seed hash32(generation, i, k, 0xE): a fourth word, so the games differ from the ring / round-robin ones."""
    if sides not in ("both", "first", "second"):
        raise ValueError("sides must be 'both', 'first' or 'second'")
    i, k = np.meshgrid(np.arange(n_individuals), np.arange(games_per_individual), indexing="ij")
    i, k = i.ravel(), k.ravel()
    first = (k % 2 == 0) if sides == "both" else np.full(len(k), sides == "first")
    out = np.zeros(len(i), dtype=MATCH_DTYPE)
    out["p1"], out["p2"] = np.where(first, i, EXPERT), np.where(first, EXPERT, i)
    out["seed"] = hash32_array(generation, i, k, 0xE)
    return out


def match_rows(matches):
    """Row of a match = the individual its counts belong to: p1 if it is one, else p2 (p1 is the scripted bot); -1 for a
    match of the bot against itself, which belongs to nobody.  Every piece of count bookkeeping goes through here."""
    return np.where(matches["p1"] >= 0, matches["p1"], matches["p2"])


def match_wins(matches, results):
    """bool[n]: the match's individual won -- FIRST won where it is p1, SECOND won where p1 is the bot."""
    return np.asarray(results) == np.where(matches["p1"] >= 0, 0, 1)


def bot_plays(matches):
    """True if the scripted bot is a side of any match: such a schedule is monsoon_rollout_vs_expert's."""
    return bool(((matches["p1"] < 0) | (matches["p2"] < 0)).any())


def mirrored_pair(deck):
    """One deck (12 card ids or a DECKS key) on both sides, as a one-pair table uint8[1][2][12]."""
    from .cards import deck_indices
    deck = deck_indices(deck)
    return np.stack([deck, deck])[None]


def _uncount(counts, matches, results):
    """Take the given matches, with the results they had, out of counts[n][3]."""
    rows = match_rows(matches)
    on = rows >= 0
    np.subtract.at(counts[:, 0], rows[on], match_wins(matches, results)[on])
    np.subtract.at(counts[:, 1], rows[on], (np.asarray(results) == -1)[on])
    np.subtract.at(counts[:, 2], rows[on], 1)


def shard_by_individual(matches, n_individuals, rank, world):
    """Contiguous blocks of row individuals per rank."""
    lo = (n_individuals * rank) // world
    hi = (n_individuals * (rank + 1)) // world
    rows = match_rows(matches)
    return matches[(rows >= lo) & (rows < hi)]


def fitness_from_counts(counts, games_per_individual):
    """wins + 0.5*draws, normalised (evo/fitness.py:111-113,160-166)."""
    counts = np.asarray(counts, dtype=np.float64)
    return [float((counts[i, 0] + 0.5 * counts[i, 1]) / games_per_individual) for i in range(len(counts))]


CAPACITY_CODE = 16   # fault codes >= this are limits of a build's record (csrc/msb_base.h), not reference behaviour
#                      (29, the work stack's word budget, among them: the same on every record, so the ladder ends by reporting it) ...
DEPTH_CODE = 18      # ... except the recursion guard: 40 nested abilities / moves.  Where that trips the reference's own
#                      recursion ends in RecursionError (raising the guard to 200 changes no game; the reference's trace of such
#                      a game is part of tests/golden/trace_heuristic_c5_big.npz), and the guard is the same on every record: such
#                      a game is a draw like any other exception, it is not replayed and not counted as a record limit


def record_limited(faults):
    """bool[n]: the games a LARGER record could play further (capacity codes other than the recursion guard)."""
    faults = np.asarray(faults)
    return (faults >= CAPACITY_CODE) & (faults != DEPTH_CODE)


def _replace_rows(counts, results, steps, faults, matches, idx, played, counted=True):
    """Rows idx of a rollout become `played` = (counts, results, steps, faults) of matches[idx]: the games are taken out
    of counts[n][3] with the results they had (counted False: they were not played before) and counted anew.  In place."""
    c, r, s, f = played
    if counted:
        _uncount(counts, matches[idx], results[idx])
    counts += np.asarray(c, dtype=counts.dtype)
    results[idx], steps[idx], faults[idx] = r, s, f


def replace_capacity_faulted(counts, results, steps, faults, matches, replay):
    """The two-record form for callers of the C ABI: the games of a rollout that hit a limit of the record (fault code
    >= 16: the reference's deep copies nest without bound, a record does not) are played again by `replay(sub_matches) ->
    (counts, results, steps, faults)` -- the same games on the build with the larger record -- and the rows of the first
    attempt replaced.  Returns the number of games replayed; the arrays are updated in place.

    Its rule is NOT the ladder's record_limited: it takes every code >= CAPACITY_CODE, the recursion guard's DEPTH_CODE
    (18) among them, which the ladder never replays (the guard is the same on every record: the replay ends as it did)."""
    bad = np.nonzero(faults >= CAPACITY_CODE)[0]
    if len(bad):
        _replace_rows(counts, results, steps, faults, matches, bad, replay(matches[bad]))
    return len(bad)


def _ladder(play, n_rows, matches, deck_pairs, concurrent=False, put=None):
    """The tier ladder, once: the tier of each game, the first pass, the climb and the replacement of rows.
    play(tier, sub_matches, sub_deck_pairs) -> (counts[n_rows][3], results, steps, faults), with a fifth item where put
    is given: a payload per row of the call, placed by put(rows, payload) (a replayed game's payload is that of the last
    tier that played it).  Returns (counts, results, steps, faults, replays, tier_sizes)."""
    from .cards import needs_extended_each
    matches = np.asarray(matches)
    deck_pairs = np.asarray(deck_pairs, dtype=np.uint8).reshape(-1, 2, 12)
    ext_pair = needs_extended_each(deck_pairs)

    def run(t, idx):   # a call is handed only the deck pairs its matches name
        used, inv = np.unique(matches["deck"][idx], return_inverse=True)
        sub = matches[idx].copy()
        sub["deck"] = inv
        return play(t, sub, deck_pairs[used])
    tier = ext_pair[matches["deck"]].astype(np.int8) if len(ext_pair) > 1 else np.full(len(matches), int(ext_pair[0]), dtype=np.int8)
    counts = np.zeros((n_rows, 3), dtype=np.int64)
    results = np.zeros(len(matches), dtype=np.int8)
    steps = np.zeros(len(matches), dtype=np.int32)
    faults = np.zeros(len(matches), dtype=np.uint8)
    first = [np.nonzero(tier == t)[0] for t in (0, 1)]
    todo = [(t, idx) for t, idx in enumerate(first) if len(idx)]
    if concurrent and len(todo) == 2:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=2) as pool:
            done = list(pool.map(lambda ti: run(*ti), todo))
    else:
        done = [run(t, idx) for t, idx in todo]

    def place(t, idx, played, counted):
        _replace_rows(counts, results, steps, faults, matches, idx, played[:4], counted)
        tier[idx] = t
        if put is not None:
            put(idx, played[4])
    for (t, idx), played in zip(todo, done):
        place(t, idx, played, False)
    replays = 0
    for t in (1, 2):   # standard -> extended -> large
        bad = np.nonzero(record_limited(faults) & (tier < t))[0]
        if len(bad):
            replays += len(bad)
            place(t, bad, run(t, bad), True)
    return counts, results, steps, faults, replays, [len(idx) for idx in first]


def tiered_rollout(play, n_rows, matches, deck_pairs, concurrent=False):
    """A schedule played on the smallest record each game needs (_ladder).  play(tier, sub_matches, sub_deck_pairs) ->
    (counts[n_rows][3], results, steps, faults) runs matches on one build (tier 0 standard, 1 extended, 2 large record);
    it is handed only the deck pairs its matches name (a build refuses a table holding a card it does not support).

    Tier per GAME, not per call: only a deck pair holding ua20 / b005, or a unit / structure card twice in one deck
    (cards.needs_extended_each: the rule of DESIGN.md §9), needs the extended record (2 400 bytes against
    752: the hot kernel runs half as many wavefronts with half as many candidate lanes on it), so a schedule of random
    109-card decks -- 37 % of whose games hold one of the two -- is split in two sub-schedules.  Then the ladder: games
    that hit a limit of their record (record_limited) are played again on the next larger one and their rows replaced
    (nested b005 memories are deep copies of the whole game, cards/b005.py:14-33, card.py:71-75: the reference's copies
    nest without bound, a record does not).  concurrent: the standard and the extended sub-schedule are played from two
    host threads (two handles, a stream each: the wavefronts of one fill the GPU while the other's batch drains or its
    host side works).  Returns (counts, results, steps, faults, replays, tier_sizes)."""
    return _ladder(play, n_rows, matches, deck_pairs, concurrent)


class FitnessEvaluator:
    def __init__(self, config, deck_config=None, rollout_fn=None, device=None, deck_draw_fn=None, strict=False, schedule_draw_fn=None):
        self.config = config
        self.deck_config = deck_config      # monsoon_amd.decks.DeckEvolutionConfig (utils.py:121-242) or None = config.deck both sides
        self.total_games = 0
        self.total_time = 0.0
        self.total_env_steps = 0        # this rank's own look-ahead steps and decisions (bench.py sums them over ranks itself) ...
        self.total_decisions = 0
        self.job_env_steps = 0          # ... and every rank's, summed in the evaluation's one all_reduce: what get_stats reports
        self.job_decisions = 0          #     (a single process: the same figures)
        self.hall_of_fame = []
        self.hall_of_fame_size = 5
        self.use_hall_of_fame = True
        self._rollout_fn = rollout_fn
        self._deck_draw_fn = deck_draw_fn   # test hook like rollout_fn: (pre-stream seeds, pool) -> uint8[n][2][12]
        self._schedule_draw_fn = schedule_draw_fn   # likewise for a per-game deck schedule: (schedule_params, game seeds) -> uint8[n][2][12]
        self._device = device
        self._engines = {}
        self.eval_times = []            # wall seconds of every evaluate_population call (the first one creates the engine)
        self.strict = strict            # True: a game left on a record limit raises instead of being scored as a draw
        self.depth_faults = 0           # games ended by the recursion guard (the reference's RecursionError), draws
        self.capacity_replays = 0       # games replayed on the large record
        self.capacity_faults = 0        # games not even the large record could hold (their fault code ends them as draws)
        self.tier_games = [0, 0]        # games first played on the standard / the extended record

    # -- device ------------------------------------------------------------------------------
    def _engine(self, tier):
        from .engine import BatchEngine
        if self._engines.get(tier) is None:
            dev = self._device
            if dev is None:
                import os
                dev = int(os.environ.get("LOCAL_RANK", "0"))
            # the large record is a replay tier for a few games per thousand: a small handle, its default variant
            games = self.config.max_concurrent_games if tier < 2 else min(self.config.max_concurrent_games, 2048)
            self._engines[tier] = BatchEngine(games, device=dev, lanes_per_game=self.config.lanes_per_game if tier == 0 else 0, extended=tier)
        return self._engines[tier]

    def warm_up(self):
        """Create the standard-record engine and launch once now instead of inside the first evaluate_population call; the
        extended / large engines are still created when a schedule first needs them."""
        if self._rollout_fn is None and self.config.mode == "rollout":
            eng = self._engine(0)
            # one decision of as many games as fill the GPU: loads the code objects and makes the runtime size the
            # launch-time buffers (work-stack overflow blocks, the queue's scratch) for a full grid -- 0.8 s the first time
            n = min(self.config.max_concurrent_games, 8192)
            m = np.zeros(n, dtype=MATCH_DTYPE)
            m["seed"] = np.arange(n)
            eng.rollout(np.zeros((1, 10)), m, mirrored_pair("N12M"), 1)
            eng.reset_stats()

    def _hip_rollout(self, weights, matches, deck_pairs, max_turns):
        import threading
        lock = threading.Lock()
        vs_expert = bot_plays(matches)

        def play(tier, sub, sub_pairs):
            eng = self._engine(tier)
            before = eng.stats()["lookahead_steps"]
            counts, results, steps = (eng.rollout_vs_expert if vs_expert else eng.rollout)(weights, sub, sub_pairs, max_turns, want_results=True)
            with lock:
                self.total_env_steps += eng.stats()["lookahead_steps"] - before
                self.total_decisions += int(steps.sum())
            return counts.astype(np.int64), results, steps, eng.rollout_faults(len(sub))

        counts, results, steps, faults, replays, sizes = tiered_rollout(play, len(weights), matches, deck_pairs,
                                                                        concurrent=self.config.concurrent_tiers)
        self.capacity_replays += replays
        left = int(record_limited(faults).sum())
        self.capacity_faults += left
        self.depth_faults += int((faults == DEPTH_CODE).sum())
        if left:
            msg = (f"{left} of {len(matches)} games still end on a limit of the largest record (fault codes "
                   f"{sorted(set(faults[record_limited(faults)].tolist()))}): scored as draws, parity with the reference unpinned for them"
                   f" (depth_faults so far: {self.depth_faults} games ended by the recursion guard, code {DEPTH_CODE}, the reference's"
                   " RecursionError: draws there too, not counted here)")
            if self.strict:
                raise RuntimeError(msg)
            import warnings
            warnings.warn(msg, RuntimeWarning, stacklevel=2)
        self.tier_games = [a + b for a, b in zip(self.tier_games, sizes)]
        self.last_rollout = (results, steps, faults)
        return counts

    def logged_games(self, weights, matches, deck_pairs=None, explore=None):
        """The games of a schedule with their logs, on this evaluator's engines (game_log.logged_rollout): what a
        champion played, step by step.  deck_pairs None: config.deck on both sides.  explore = an engine.Explore: the
        games leave the champion's line where its draws say so, and the log keeps the champion's choice (log.greedy).
        An engine.Policies (a rule per row of `weights`) passes through unchanged: sub-schedules keep their row indices.
        Returns (counts, results, steps, faults, log); the evaluator's statistics are left alone."""
        from .game_log import logged_rollout
        if deck_pairs is None:
            deck_pairs = mirrored_pair(self.config.deck)
        return logged_rollout(self._engine, np.asarray(weights, dtype=np.float64), np.asarray(matches), deck_pairs, self.config.max_turns, explore)

    def _deck_source(self):
        """Where this evaluator's decks come from: its DeckEvolutionConfig, else config.deck (a DECKS key or RANDOM_DECK)."""
        return self.config.deck if self.deck_config is None else self.deck_config

    @staticmethod
    def _seed_keyed(source):
        """True for a deck source whose per-game decks depend on the game's seed alone: configuration C5 and a per_game schedule."""
        from .cards import RANDOM_DECK
        return bool(getattr(source, "per_game", False)) or (isinstance(source, str) and source == RANDOM_DECK)

    def _decks_for(self, matches, generation, tag=1, source=None):
        """Deck pairs [n_decks][2][12] for a schedule; fills matches["deck"].  source (None: _deck_source(), the
        evaluator's own) is a deck for both sides as config.deck names one, RANDOM_DECK among them, or a
        DeckEvolutionConfig: utils.py:155-219 per GAME, as games/evolutionary_stormbound.py:52 draws them (one pair for
        the whole generation while the schedule is in its exploit phase).  tag: the stream tag of a per-game
        DeckEvolutionConfig (decks.TAG_POPULATION / TAG_EXPERT), unused otherwise."""
        from .cards import C5_STREAM_XOR, RANDOM_DECK, deck_indices, draw_random_decks_numpy, observable_pool
        if source is None:
            source = self._deck_source()
        if isinstance(source, str) and source == RANDOM_DECK:
            # configuration C5: two decks per game from the 109 observable cards, drawn by the game's own pre-stream
            pre = matches["seed"] ^ np.uint32(C5_STREAM_XOR)
            matches["deck"] = np.arange(len(matches))
            if self._deck_draw_fn is not None:
                return self._deck_draw_fn(pre, observable_pool())
            if self._rollout_fn is not None:   # CPU stand-in (tests): numpy itself
                return draw_random_decks_numpy(pre)
            return self._engine(0).draw_decks(pre, observable_pool())
        if not hasattr(source, "get_deck_configuration"):
            return mirrored_pair(source)
        if source.is_static(generation):
            d1, d2 = source.get_deck_configuration(generation)
            return np.stack([deck_indices(d1), deck_indices(d2)])[None]
        matches["deck"] = np.arange(len(matches))
        pairs = np.zeros((len(matches), 2, 12), dtype=np.uint8)
        if source.per_game:
            # every game draws from a stream of its own (decks.game_decks): on the device, unless a stand-in plays the games
            # or the schedule is one the device entry does not take (schedule_params is None: the host draw stays)
            params = source.schedule_params(generation, tag)
            if params is not None and self._schedule_draw_fn is not None:
                return self._schedule_draw_fn(params, matches["seed"])
            if params is not None and self._rollout_fn is None:
                return self._engine(0).draw_schedule(params, matches["seed"])
            for k, seed in enumerate(matches["seed"]):
                d1, d2 = source.game_decks(generation, seed, tag)
                pairs[k, 0], pairs[k, 1] = deck_indices(d1), deck_indices(d2)
            return pairs
        for k in range(len(matches)):
            d1, d2 = source.get_deck_configuration(generation)
            pairs[k, 0], pairs[k, 1] = deck_indices(d1), deck_indices(d2)
        return pairs

    @staticmethod
    def _dist():
        """torch.distributed if this process is a rank of an initialised job of more than one rank, else None.  A process
        that never imported torch.distributed cannot be one: it is not imported here (0.7 s the first time)."""
        import sys
        dist = sys.modules.get("torch.distributed")
        if dist is not None and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            return dist
        return None

    # -- Seam F ------------------------------------------------------------------------------
    def _play_schedule(self, matches, weights, n_rows, generation, tag, source, counted):
        """One schedule, evaluated: this rank's shard of it (by row individual, of n_rows), its decks from `source`
        (_decks_for) under stream tag `tag`, the rollout, and the one all-reduce.  Returns counts[len(weights)][3] of the
        whole job.  counted: the games' look-ahead steps and decisions go to the statistics -- total_* on this rank,
        job_* summed over ranks, riding as a last row of the counts tensor; else total_* end as they began."""
        source = self._deck_source() if source is None else source
        dist = self._dist()

        def shard(m):
            return m if dist is None else shard_by_individual(m, n_rows, dist.get_rank(), dist.get_world_size())
        if self._seed_keyed(source):
            # per-game decks that depend on the game's seed alone: every rank draws only the games it plays
            mine = shard(matches)
            if dist is not None:
                mine = mine.copy()
            deck_pairs = self._decks_for(mine, generation, tag, source) if len(mine) else np.zeros((1, 2, 12), dtype=np.uint8)
        else:
            # one pair for all, or a sequential stream (utils.py:155-219): drawn for the WHOLE schedule, so every rank sees the same decks
            deck_pairs = self._decks_for(matches, generation, tag, source)
            mine = shard(matches)
            if dist is not None and len(deck_pairs) > 1 and len(mine):   # keep only this rank's decks
                deck_pairs = deck_pairs[mine["deck"]]
                mine = mine.copy()
                mine["deck"] = np.arange(len(mine))
        fn = self._rollout_fn or self._hip_rollout
        counts = np.zeros((len(weights), 3), dtype=np.int64)
        before = self.total_env_steps, self.total_decisions   # the rollout, or its stand-in, adds its games to these
        if len(mine):
            counts += np.asarray(fn(weights, mine, deck_pairs, self.config.max_turns), dtype=np.int64)
        played = [self.total_env_steps - before[0], self.total_decisions - before[1], 0]
        if not counted:
            self.total_env_steps, self.total_decisions = before
            return counts if dist is None else self._all_reduce_counts(dist, counts)
        if dist is not None:
            # this rank's env-steps and decisions ride along as one more row: still one collective per evaluation
            counts, played = self._all_reduce_counts(dist, counts, played)
        self.job_env_steps += int(played[0])
        self.job_decisions += int(played[1])
        return counts

    def evaluate_population(self, population, generation=0):
        cfg = self.config
        n = len(population)
        opponents = list(population)
        if self.use_hall_of_fame and self.hall_of_fame:
            opponents.extend(self.hall_of_fame)
        n_total = len(opponents)
        start = time.time()
        if cfg.schedule == "ring":
            matches = ring_schedule(n, cfg.games_per_individual, generation)
            per_individual = cfg.games_per_individual
        else:
            matches = round_robin_schedule(n, n_total, cfg.games_per_pairing, generation)
            per_individual = (n_total - 1) * cfg.games_per_pairing
        if cfg.mode == "as_written":
            # _play_game returns 0 ("agent1 wins") without a step for every game
            counts = np.zeros((n_total, 3), dtype=np.int64)
            np.add.at(counts[:, 0], matches["p1"], 1)
            np.add.at(counts[:, 2], matches["p1"], 1)
        else:
            from .decks import TAG_POPULATION
            weights = np.stack([np.asarray(o.weights, dtype=np.float64) for o in opponents])
            counts = self._play_schedule(matches, weights, n, generation, TAG_POPULATION, None, True)
        self.total_games += len(matches)
        self.total_time += time.time() - start
        self.eval_times.append(time.time() - start)
        fitness = fitness_from_counts(counts[:n], per_individual)
        self._update_hall_of_fame(population, fitness)
        return fitness

    def evaluate_vs_expert(self, population, generation=0, games_per_individual=None, sides="both"):
        """The population against the reference's scripted bot (play_vs_expert.py; the success criterion of
        evo/EVOLUTIONARY_PLAN.md): individual i plays `games_per_individual` games (config.expert_eval_games by default)
        of expert_schedule; returns its score (wins + 0.5 * draws) / games.  self.last_vs_expert keeps the raw
        counts[n][3] = {wins, draws, games}.  Decks, tiers, sharding and the all-reduce are evaluate_population's; the hall
        of fame, the total_* statistics and a DeckEvolutionConfig's sequential stream are left alone, so the fitness
        evaluate_population returns does not depend on whether this was called.  In a random phase of a deck schedule the
        games play the schedule's own decks if it is a per_game=True one (stream tag 2), random109 decks otherwise."""
        from .cards import RANDOM_DECK
        from .decks import TAG_EXPERT
        n = len(population)
        games = int(self.config.expert_eval_games if games_per_individual is None else games_per_individual)
        if games <= 0:
            raise ValueError("games_per_individual must be positive")
        matches = expert_schedule(n, games, generation, sides)
        weights = np.stack([np.asarray(o.weights, dtype=np.float64) for o in population])
        # The random phase of a sequential DeckEvolutionConfig draws every game's decks from ONE stream: drawing from it
        # here would change the decks of the next evaluate_population.  These games take their decks as configuration C5
        # does instead, each from its own seed's pre-stream.  (A per_game=True schedule has no such stream: its games
        # play the schedule's own decks, drawn with the stream tag of this call.)
        dc = self.deck_config
        detour = dc is not None and not dc.is_static(generation) and not dc.per_game
        self.last_vs_expert = self._play_schedule(matches, weights, n, generation, TAG_EXPERT, RANDOM_DECK if detour else None, False)
        return fitness_from_counts(self.last_vs_expert, games)

    @staticmethod
    def _all_reduce_counts(dist, counts, extra=None):
        """counts[n][3] summed over ranks; with extra (three integers of this rank) appended as a last row of the same
        tensor, (summed counts, summed extra)."""
        import torch
        if extra is not None:
            counts = np.concatenate([np.asarray(counts, dtype=np.int64), np.asarray(extra, dtype=np.int64).reshape(1, 3)])
        t = torch.from_numpy(np.ascontiguousarray(counts))
        if dist.get_backend() == "nccl":   # RCCL: the tensor must live on this rank's GPU
            t = t.cuda()
        dist.all_reduce(t)   # sum over ranks; <= 48 KB at N = 4096
        out = t.cpu().numpy()
        return out if extra is None else (out[:-1], out[-1])

    # evo/fitness.py:247-259: copies of the five best of this generation
    def _update_hall_of_fame(self, population, fitness):
        ranked = sorted(zip(fitness, population), key=lambda p: p[0], reverse=True)
        self.hall_of_fame = [ind.copy() for _, ind in ranked[:self.hall_of_fame_size]]

    def get_stats(self):
        return {"total_games": self.total_games, "total_time": self.total_time,
                "avg_time_per_game": self.total_time / max(self.total_games, 1),
                "games_per_second": self.total_games / max(self.total_time, 1e-6),
                "env_steps": self.job_env_steps, "capacity_replays": self.capacity_replays, "capacity_faults": self.capacity_faults,
                "depth_faults": self.depth_faults,
                "env_steps_per_second": self.job_env_steps / max(self.total_time, 1e-6)}

    def kernel_time(self):
        """(ms, launches) of the hot kernel over every engine this evaluator has created (HIP events on their streams)."""
        ms, n = 0.0, 0
        for eng in self._engines.values():
            if eng is not None:
                a, b = eng.kernel_time()
                ms, n = ms + a, n + b
        return ms, n

    def reset_stats(self):
        self.total_games = 0
        self.total_time = 0.0
        self.total_env_steps = 0
        self.total_decisions = 0
        self.job_env_steps = 0
        self.job_decisions = 0
        for eng in self._engines.values():
            if eng is not None:
                eng.reset_stats()
