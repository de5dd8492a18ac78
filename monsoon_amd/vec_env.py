"""VecEnv: the device-resident vector environment (monsoon_env_reset / monsoon_env_step_dev) as torch tensors.

Seam G batched for a learner that lives on the GPU: n slots of games/abstract_game.py's interface (step, to_play,
legal_actions, reset, expert_agent as the opponent), each an endless sequence of episodes that restart in place.  One
`step` is three kernel launches on the handle's stream -- legality check, step, the scripted bot's turn, end of episode,
re-seed, re-init, observation and legal mask -- and no host round trip, so it can be captured into a CUDA graph.  The
opponent can also be the reference's HeuristicAgent with GA weights ("heuristic": seven launches per step).
`OpponentExplore` makes that opponent epsilon-greedy with an epsilon per slot (`reset(opponent_explore=...)`,
`set_opponent_explore` between steps, `opponent_explored` for the counts, `opponent_explore_draws` for the draws); with
`temperature=` its exploring decisions draw from the softmax over their scores, a temperature per slot.
`snapshot` / `restore` keep slots and put them back -- into the same slot (rewind) or into many (fork) -- on the device;
`determinize` is the restore of an information-set search: it draws again what the side to move cannot see.
Episode decks come from the reset decks, from a pool, or from a deck schedule (`reset(deck_schedule=...)`: the GA's
exploit / explore / balance curriculum, drawn on the device per episode; `set_deck_schedule` moves its generation).
torch is used for device memory and stream ordering only; there is no CPU fallback.
"""
import contextlib
import ctypes

import numpy as np

from ._lib import EnvAfter, EnvConfig, EnvViews, MonsoonError
from .engine import BatchEngine
from .fitness import hash32_array

OPPONENTS = {"none": 0, "expert": 1, "heuristic": 2}

# name -> (trailing shape, torch dtype name); the order of monsoon_env_views
_VIEWS = (("obs", (27, 5, 4), "int32"), ("legal", (156,), "bool"), ("obs_raises", (), "bool"), ("to_play", (), "uint8"),
          ("reward", (), "int8"), ("done", (), "bool"), ("winner", (), "int8"), ("truncated", (), "bool"), ("fault", (), "uint8"),
          ("illegal", (), "bool"), ("episode", (), "int32"), ("final_hash", (), "int64"))

# name -> (shape behind [n], with K = max_after; torch dtype name); the order of monsoon_env_after
_AFTER = (("n_legal", (), "int32"), ("action", ("K",), "uint8"), ("status", ("K",), "uint8"), ("reward", ("K",), "int8"),
          ("winner", ("K",), "int8"), ("features", ("K", 10), "float64"), ("obs", ("K", 27, 5, 4), "int32"),
          ("before_features", (10,), "float64"))


def select_actions(after, values):
    """The actions for VecEnv.step from a value per afterstate: values [n][K] (any real dtype) over the dict that
    VecEnv.afterstates returned -> uint8 [n].  Per slot the first maximum over the entries that exist (k < min(n_legal, K))
    and whose look-ahead raised nothing (status == 0); 155 (PASS, always accepted) where no entry is left; 255 (the slot is
    left alone, its pending end is reported by the step) where n_legal == 0.  A NaN value counts as -inf: its entry is taken
    only where no entry of the slot has a number.  Pure torch: works on CPU tensors too."""
    import torch
    action, status, n_legal = after["action"], after["status"], after["n_legal"]
    n, k = action.shape
    if values.shape != (n, k):
        raise ValueError(f"values must be [{n}][{k}], got {tuple(values.shape)}")
    ok = (torch.arange(k, device=action.device)[None, :] < n_legal[:, None]) & (status == 0)
    # first maximum: among the entries equal to the row's maximum, the lowest k (argmax's tie rule is not specified)
    v = values.to(torch.float64)
    v = torch.where(ok & ~torch.isnan(v), v, torch.full_like(v, float("-inf")))   # a NaN value ranks below every number
    best = ok & (v == v.max(dim=1, keepdim=True).values)
    idx = torch.arange(k, device=action.device)[None, :].expand(n, k)
    first = torch.where(best, idx, torch.full_like(idx, k)).min(dim=1).values.clamp(max=k - 1)
    out = action.gather(1, first[:, None])[:, 0]
    out = torch.where(best.any(dim=1), out, torch.full_like(out, 155))
    return torch.where(n_legal == 0, torch.full_like(out, 255), out)


class OpponentExplore:
    """The exploration rule of a VecEnv's heuristic opponents (monsoon_env_explore and its thresholds, include/monsoon.h):
    a decision of slot i's opponent at step index k of its episode (k < until_step where until_step > 0) commits a uniformly
    drawn legal action instead of its arg-max with probability eps[i].  eps is a scalar (every slot) or one value per slot;
    threshold = min(int(eps * 2**32), 0xFFFFFFFF) as engine.Explore's.  The draws are hash32(seed, episode seed, k, .):
    opponent_explore_draws recomputes them.
    temperature = a finite T > 0, a scalar (every slot) or one value per slot, selects the sampling rule instead
    (monsoon_env_set_opponent_sample): such a decision commits an action drawn from the softmax over its scores,
    exp((score - best) / T[i]) in 24-bit integer weights (game_log.sample_weights, game_log.sample_rank, as engine.Explore's
    temperature); inv_temperatures(n) = 1.0 / T is what the device multiplies by.  Actions tied for the best score share
    the probability equally.  temperature=None is the uniform rule, unchanged in every bit."""

    def __init__(self, eps, seed, until_step=0, temperature=None):
        e = np.asarray(eps, dtype=np.float64)
        if e.ndim > 1 or not ((e >= 0.0) & (e <= 1.0)).all():   # (a NaN fails it too)
            raise ValueError(f"OpponentExplore: eps is a scalar or [n] with every value in [0, 1], got {eps!r}")
        self.eps, self.seed, self.until_step = e, int(seed) & 0xFFFFFFFF, int(until_step)
        self.temperature = None
        if temperature is not None:
            t = np.asarray(temperature, dtype=np.float64)
            with np.errstate(divide="ignore", over="ignore"):
                ok = t.ndim <= 1 and bool(((t > 0.0) & np.isfinite(t) & np.isfinite(1.0 / np.where(t > 0.0, t, 1.0))).all())
            if not ok:   # (a NaN fails it too, and a subnormal T whose 1 / T is not finite)
                raise ValueError(f"OpponentExplore: temperature is a scalar or [n] with every value finite and > 0, got {temperature!r}")
            self.temperature = t

    @property
    def samples(self):
        """True for the sampling rule (a temperature), False for the uniform one."""
        return self.temperature is not None

    def inv_temperatures(self, n):
        """float64 [n]: 1.0 / T of slot i, what monsoon_env_set_opponent_sample takes and the device multiplies by."""
        if not self.samples:
            raise ValueError("OpponentExplore: inv_temperatures needs a temperature (the sampling rule)")
        if self.temperature.ndim == 1 and self.temperature.shape != (n,):
            raise ValueError(f"OpponentExplore: temperature holds {len(self.temperature)} values, the env {n} slots")
        return np.ascontiguousarray(1.0 / np.broadcast_to(self.temperature, (n,)), dtype=np.float64)

    def thresholds(self, n):
        """uint32 [n]: slot i's opponent explores iff its draw0 < thresholds[i]."""
        if self.eps.ndim == 1 and self.eps.shape != (n,):
            raise ValueError(f"OpponentExplore: eps holds {len(self.eps)} values, the env {n} slots")
        e = np.broadcast_to(self.eps, (n,))
        return np.minimum(np.floor(e * 2.0**32), float(0xFFFFFFFF)).astype(np.uint32)   # (eps * 2**32 is exact: int() of it floors)


def opponent_explore_draws(seed, episode_seeds, k):
    """The draws of the exploring opponent for decisions at step index k of episodes with the seeds episode_seeds
    (seed0[i] + episode[i] * seed_stride mod 2**32), broadcast together -> (draw0, draw1) uint32: the decision explores iff
    draw0 < the slot's threshold (and k is below until_step) and then commits legal action number (draw1 * n_legal) >> 32."""
    return hash32_array(seed, episode_seeds, k, 0), hash32_array(seed, episode_seeds, k, 1)


DETERMINIZE = {"stream": 1, "hand": 3}   # what -> MONSOON_DET_STREAM, MONSOON_DET_STREAM | MONSOON_DET_HAND


def determinize_order(seed, n_movable, n_deck):
    """The permutation VecEnv.determinize(what="hand") applies to the hidden side's cards for the seed `seed`
    (include/monsoon.h, monsoon_env_load_determinized_dev; csrc/determinize.h): with A = the n_movable movable hand entries
    in record order followed by the n_deck deck entries, the re-dealt list is A[order] -- order[:n_movable] is the new hand.
    An int64 array of n_movable + n_deck indices, recomputed on the host: r = hash32(seed, i, 0xD7),
    j = i + ((r * (L - i)) >> 32), swap places i and j, for i < n_movable."""
    k, d = int(n_movable), int(n_deck)
    if not (0 <= k <= 5 and 0 <= d <= 12):
        raise ValueError(f"a hand holds 0..5 cards and a deck 0..12, got {n_movable}, {n_deck}")
    order = np.arange(k + d, dtype=np.int64)
    if k:
        i = np.arange(k, dtype=np.uint64)
        r = hash32_array(int(seed) & 0xFFFFFFFF, i, 0xD7).astype(np.uint64)
        j = i + ((r * (np.uint64(k + d) - i)) >> np.uint64(32))
        for a, b in zip(range(k), j.astype(np.int64)):
            order[[a, b]] = order[[b, a]]
    return order


class EnvSnapshot:
    """Saved slots of a VecEnv (VecEnv.snapshot): data is a uint8 CUDA tensor [cap][entry_bytes], count the entries in
    use (the first `count` rows), extended the record build that wrote them, entry_bytes that build's entry size.  The
    entries are plain device bytes (include/monsoon.h, monsoon_env_save_dev): they load into any VecEnv of the same record
    build and library version."""

    def __init__(self, data, count, extended, entry_bytes):
        self.data = data
        self.count = int(count)
        self.extended = int(extended)
        self.entry_bytes = int(entry_bytes)

    @property
    def capacity(self):
        return int(self.data.shape[0])

    def __len__(self):
        return self.count


class VecEnv:
    """n game slots on one GPU.  reset() loads episode 0 of every slot; step(actions) advances every slot by the agent's
    action (and the bot's answer), restarts finished episodes and returns the view tensors.  snapshot() / restore() save
    slots and load them back, also one entry into many slots.  See include/monsoon.h (monsoon_env_*) for the contract and
    INTEGRATION.md for a trainer loop."""

    def __init__(self, max_slots, device=0, extended=0, lanes_per_game=0):
        """extended = 0 / 1 / 2 selects the record build (1: decks holding ua20 / b005, or a unit / structure card twice).  Raises MonsoonError when no
        gfx950 device is usable."""
        # torch ships a ROCm runtime of its own.  It has to be the first one the process loads: once libmonsoon_hip*.so has
        # pulled in the system's, a torch imported afterwards finds no device (torch.cuda.is_available() is False).  The
        # env's views are torch tensors, so torch is needed anyway: import it before the handle loads the library.
        import torch  # noqa: F401
        self.engine = BatchEngine(max_slots, device=device, lanes_per_game=lanes_per_game, extended=extended)
        self.device = device
        self.extended = extended
        self.n = 0
        self.views = None
        self._heuristic = False   # an opponent-2 env is loaded
        self._explore = False     # ... that was reset with an exploration rule
        self._samples = False     # ... of the sampling kind (OpponentExplore(temperature=)): the kind of the rule last set
        self._rows = None         # the rows last given to set_opponents / reset (None = row 0 for every slot)
        self._explored = None     # opponent_explored()'s tensor
        self._after = {}          # obs -> ((n, K), tensors, _lib.EnvAfter): the latest shape per obs flag, reused until it changes
        self._schedule = None     # the deck_schedule given to reset (a DeckEvolutionConfig or a dict) while a schedule-mode env is loaded
        self._decks = None        # decks()' tensor
        self._observers = {}      # (m, side) -> determinize's observer bytes for an int observer

    def close(self):
        if self.engine is not None:
            self.engine.close()
            self.engine = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    @property
    def stream(self):
        """The handle's stream as a torch stream: order your own work against it, or capture env.step on it."""
        import torch
        return torch.cuda.ExternalStream(self.engine.stream_ptr(), device=torch.device("cuda", self.device))

    def _alloc(self, n):
        import torch
        dev = torch.device("cuda", self.device)
        views = {}
        for name, shape, dt in _VIEWS:
            views[name] = torch.zeros((n,) + shape, dtype=getattr(torch, dt), device=dev)
        return views

    def reset(self, seed0, decks=None, factions=None, opponent="none", agent_side=0, max_steps=0, pool=None, seed_stride=0,
              opponent_weights=None, opponent_rows=None, deck_schedule=None, generation=None, opponent_explore=None):
        """Episode 0 of every slot: slot i plays seed0[i] with decks[i] ([n][2][12] or one [2][12] pair for all) and
        factions[i]; episode k then starts from seed0[i] + k * seed_stride (0 = n).  pool (12..128 card indices) draws
        fresh decks for every episode instead (decks must be None).  opponent "expert" puts the reference's scripted bot on
        the side that agent_side does not play; "heuristic" puts the reference's HeuristicAgent there, slot i playing row
        opponent_rows[i] (None = row 0) of opponent_weights ([10] or [k][10] float64, e.g. WeightVector.weights or a
        Population's individuals).  max_steps > 0 truncates episodes.  Returns the view tensors (a dict).

        deck_schedule (decks and pool must be None) draws the decks of every episode, episode 0 included, from a deck
        schedule on the device: a DeckEvolutionConfig(per_game=True) at `generation`, or a dict of the fields of
        monsoon_deck_schedule (DeckEvolutionConfig.env_schedule; a `generation` given here replaces the dict's; None = 0 for a
        config).  The episode that
        starts from seed s plays deck_schedule.game_decks(generation, s, decks.TAG_ENV) of the schedule in force when it
        starts; set_deck_schedule moves the generation between steps; decks() tells what every slot is playing.  Factions
        stay those of `factions` (episode 0 only, as ever).  Every faction's pool holds ua20 and Shadowfen's b005, so a
        schedule made from a config needs VecEnv(extended=1) once it draws (explore and balance phases): on the standard
        build the library refuses it (MONSOON_ERR_ARG) and MonsoonError is raised.  Whatever its pools hold, the standard
        build also refuses an explore generation that keeps some but not all of the archetype (0 < n_preserve < 12): the
        kept cards and the drawn ones may repeat a card, which only the extended record plays as the reference does
        (DESIGN.md §9), and the host never sees a deck drawn on the device.  The message names extended=1.

        opponent_explore (an OpponentExplore; opponent "heuristic" only) makes the opponents epsilon-greedy from the first
        decision on, and lets set_opponent_explore retune them between steps -- eps 0 everywhere arms the env for that and
        plays the plain opponent bit for bit until then.  Without it the env plays the plain opponent's kernel and
        set_opponent_explore raises.  An OpponentExplore with a temperature plays the sampling opponent's kernel instead;
        the library keeps one kind of rule per loaded heuristic env, so a reset that changes the kind on a VecEnv whose
        heuristic env holds a rule raises MonsoonError (open another VecEnv)."""
        if opponent not in OPPONENTS:
            raise ValueError(f"opponent must be one of {sorted(OPPONENTS)}")
        seed0 = np.ascontiguousarray(seed0, dtype=np.uint32)
        n = len(seed0)
        sched = None
        if deck_schedule is not None:
            if decks is not None or pool is not None:
                raise ValueError("deck_schedule draws every episode's decks: decks and pool must be None")
            sched = self._schedule_params(deck_schedule, generation)
        elif pool is None and decks is None:
            raise ValueError("decks are required without a pool or a deck_schedule")
        opp = None
        if opponent == "heuristic":
            if opponent_weights is None:
                raise ValueError('opponent="heuristic" needs opponent_weights ([10] or [k][10])')
            opp = self._opponents(opponent_weights, opponent_rows, n)
            if self._heuristic and self.n != n:
                raise ValueError(f"a VecEnv with a heuristic opponent keeps its {self.n} slots: open another VecEnv for {n}")
        elif opponent_weights is not None or opponent_rows is not None or opponent_explore is not None:
            raise ValueError('opponent_weights / opponent_rows / opponent_explore need opponent="heuristic"')
        thresholds = inv_t = None
        if opponent_explore is not None:
            if not isinstance(opponent_explore, OpponentExplore):
                raise ValueError("opponent_explore must be an OpponentExplore")
            thresholds = opponent_explore.thresholds(n)
            if opponent_explore.samples:
                inv_t = opponent_explore.inv_temperatures(n)
        cfg = EnvConfig()
        cfg.opponent = OPPONENTS[opponent]
        cfg.agent_side = int(agent_side)
        cfg.seed_stride = int(seed_stride) & 0xFFFFFFFF
        cfg.max_steps = int(max_steps)
        if pool is not None:
            pool = np.ascontiguousarray(pool, dtype=np.uint8)
            if not 12 <= len(pool) <= 128:
                raise ValueError("a pool holds 12..128 cards")
            cfg.pool_n = len(pool)
            ctypes.memmove(cfg.pool, pool.ctypes.data, len(pool))
        if self.views is None or self.n != n:
            self.engine.sync()
            self.views = self._alloc(n)
        self.n = n
        views = EnvViews(**{name: t.data_ptr() for name, t in self.views.items()})
        with self._after_torch_stream():
            if opp is not None:
                self.engine.env_set_opponents(opp[0], opp[1], n)
            if opp is not None:
                if thresholds is not None:
                    self._set_rule(opponent_explore.seed, opponent_explore.until_step, thresholds, inv_t)
                    self._samples = inv_t is not None
                elif self._explore:   # the loaded env holds the handle's rule: it cannot be cleared, silent is the same play
                    self._set_rule(0, 0, np.zeros(n, dtype=np.uint32), np.ones(n) if self._samples else None)
            self._heuristic = False
            self._schedule = None
            if sched is not None:
                self.engine.env_set_schedule(sched)
            self.engine.env_reset(cfg, views, seed0, decks, factions)
            self._heuristic = opp is not None
            if opp is not None:
                self._explore = thresholds is not None or self._explore
                self._rows = opp[1]
            self._schedule = deck_schedule
        return self.views

    @contextlib.contextmanager
    def _after_torch_stream(self):
        """The bracket of the synchronising setters (reset, set_opponents, set_deck_schedule): the env's stream waits for
        torch's current one -- the views may still be read by work queued there -- and torch's waits for the env's when the
        body is left, also by an exception.  Unconditional, unlike _on_env_stream's."""
        import torch
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        try:
            yield
        finally:
            torch.cuda.current_stream(self.device).wait_stream(self.stream)

    @staticmethod
    def _opponents(weights, rows, n):
        w = np.asarray(weights, dtype=np.float64)
        if w.ndim == 1:
            w = w[None]
        if w.ndim != 2 or w.shape[1] != 10 or len(w) == 0:
            raise ValueError(f"opponent weights must be [10] or [k][10], got {np.shape(weights)}")
        if rows is not None:
            rows = np.asarray(rows)
            if rows.shape != (n,) or not np.issubdtype(rows.dtype, np.integer):
                raise ValueError(f"opponent rows must be {n} integers, got {rows.shape} {rows.dtype}")
            if n and (rows.min() < 0 or rows.max() >= len(w)):
                raise ValueError(f"opponent rows must lie in [0, {len(w)})")
            rows = rows.astype(np.int32)
        return np.ascontiguousarray(w), rows

    def set_opponents(self, weights, rows=None):
        """A league update between steps: the heuristic opponents' weights ([10] or [k][10]; k at most the k given to
        reset) and each slot's row (None = row 0).  They apply from the next step; a captured step graph stays valid."""
        if not self._heuristic:
            raise MonsoonError('VecEnv.set_opponents needs reset(opponent="heuristic", ...) first')
        w, r = self._opponents(weights, rows, self.n)
        with self._after_torch_stream():
            self.engine.env_set_opponents(w, r, self.n)
        self._rows = r

    def _set_rule(self, seed, until_step, thresholds, inv_t):
        """The setter of the rule's kind: inv_t None = the uniform rule, else the sampling one."""
        if inv_t is None:
            self.engine.env_set_opponent_explore(seed, until_step, thresholds)
        else:
            self.engine.env_set_opponent_sample(seed, until_step, thresholds, inv_t)

    def eps_by_row(self, eps_rows):
        """A per-individual epsilon [k] -> the per-slot values [n] for OpponentExplore, through the rows last given to
        set_opponents / reset (slot i gets eps_rows[rows[i]]; no rows = row 0 for every slot).  It maps any per-individual
        vector: temperatures by row go through it too (OpponentExplore(eps_by_row(e), seed, temperature=eps_by_row(t)))."""
        e = np.asarray(eps_rows, dtype=np.float64)
        if e.ndim != 1 or len(e) == 0:
            raise ValueError(f"eps_rows must be [k], got {np.shape(eps_rows)}")
        rows = np.zeros(self.n, dtype=np.int64) if self._rows is None else np.asarray(self._rows, dtype=np.int64)
        if len(rows) and rows.max() >= len(e):
            raise ValueError(f"eps_rows holds {len(e)} values, the slots play rows up to {int(rows.max())}")
        return e[rows]

    def set_opponent_explore(self, opponent_explore):
        """Retune the exploring opponents between steps (monsoon_env_set_opponent_explore): the OpponentExplore's seed,
        until_step and per-slot epsilons (eps_by_row makes them from per-individual ones) apply from the next decision; a
        captured step graph stays valid.  Needs reset(opponent="heuristic", opponent_explore=...) first (MonsoonError).
        A sampling rule (OpponentExplore(temperature=)) retunes the temperatures too (monsoon_env_set_opponent_sample); the
        kind is the reset's -- the kernel was chosen there -- and a rule of the other kind raises MonsoonError before the
        library is touched.  Synchronises the env's stream."""
        if not (self._heuristic and self._explore):
            raise MonsoonError('VecEnv.set_opponent_explore needs reset(opponent="heuristic", opponent_explore=...) first')
        if not isinstance(opponent_explore, OpponentExplore):
            raise ValueError("opponent_explore must be an OpponentExplore")
        if opponent_explore.samples != self._samples:
            raise MonsoonError("VecEnv.set_opponent_explore: the env was reset with the " + ("sampling" if self._samples else "uniform") +
                               " rule; a rule " + ("without" if self._samples else "with") + " a temperature needs another reset")
        thresholds = opponent_explore.thresholds(self.n)
        inv_t = opponent_explore.inv_temperatures(self.n) if self._samples else None
        with self._after_torch_stream():
            self._set_rule(opponent_explore.seed, opponent_explore.until_step, thresholds, inv_t)

    def opponent_explored(self):
        """The decisions of every slot's opponent whose draw said "explore" (or "sample", under a rule with a temperature:
        the counter serves both kinds), since reset (monsoon_env_opponent_explored_dev):
        an int32 CUDA tensor [n], allocated on the first call per n and overwritten in place by every later one (a later
        call allocates nothing and can be captured).  Stream ordering as in step."""
        import torch
        if not (self._heuristic and self._explore):
            raise MonsoonError('VecEnv.opponent_explored needs reset(opponent="heuristic", opponent_explore=...) first')
        if self._explored is None or self._explored.shape[0] != self.n:
            self._explored = torch.zeros(self.n, dtype=torch.int32, device=torch.device("cuda", self.device))
        self._on_env_stream(lambda: self.engine.env_opponent_explored(self._explored.data_ptr()))
        return self._explored

    @staticmethod
    def _schedule_params(deck_schedule, generation):
        """The fields of monsoon_deck_schedule at `generation` from a DeckEvolutionConfig(per_game=True) or a dict of them."""
        if isinstance(deck_schedule, dict):
            return deck_schedule if generation is None else dict(deck_schedule, generation=int(generation))
        if not getattr(deck_schedule, "per_game", False):
            raise ValueError("deck_schedule must be a DeckEvolutionConfig(per_game=True) or a dict of monsoon_deck_schedule's fields")
        return deck_schedule.env_schedule(int(generation or 0))

    def set_deck_schedule(self, generation, deck_schedule=None):
        """Move a schedule-mode env to another generation (and, with deck_schedule, to another config or dict; None keeps
        the one given to reset) between steps: every episode that starts from the next step on draws from it, running
        episodes keep their decks, a captured step graph stays valid.  MonsoonError if the env was not reset with a
        deck_schedule.  Synchronises the env's stream."""
        if self._schedule is None:
            raise MonsoonError("VecEnv.set_deck_schedule needs reset(deck_schedule=...) first")
        new = self._schedule if deck_schedule is None else deck_schedule
        params = self._schedule_params(new, generation)
        with self._after_torch_stream():
            self.engine.env_set_schedule(params)
        self._schedule = new

    def decks(self):
        """The decks of every slot's current episode (monsoon_env_decks_dev): a uint8 CUDA tensor [n][2][12] of card
        indices, P1's deck first, in every deck mode.  Allocated on the first call per n and overwritten in place by every
        later one (a later call allocates nothing and can be captured).  Stream ordering as in step."""
        import torch
        if self.views is None:
            raise MonsoonError("VecEnv.decks before reset")
        if self._decks is None or self._decks.shape[0] != self.n:
            self._decks = torch.zeros((self.n, 2, 12), dtype=torch.uint8, device=torch.device("cuda", self.device))
        self._on_env_stream(lambda: self.engine.env_decks_dev(self._decks.data_ptr()))
        return self._decks

    def step(self, actions):
        """Advance every slot: actions is a uint8 CUDA tensor [n] (255 = leave the slot alone, 155 = PASS, any other
        action must be legal, else views["illegal"][i] is set and the slot is left untouched).  Asynchronous: returns the
        SAME view tensors reset() returned, overwritten in place on the env's stream (torch's current stream is made to
        wait for it); copy what you want to keep before the next step."""
        import torch
        if self.views is None:
            raise MonsoonError("VecEnv.step before reset")
        if not isinstance(actions, torch.Tensor) or actions.dtype != torch.uint8 or not actions.is_cuda or actions.shape != (self.n,):
            raise ValueError(f"actions must be a uint8 CUDA tensor of shape ({self.n},)")
        actions = actions.contiguous()
        self._on_env_stream(lambda: self.engine.env_step_dev(actions.data_ptr()))
        return self.views

    def afterstates(self, max_after=64, obs=True):
        """The successor of every legal action of every slot's current state (monsoon_env_afterstates_dev): one launch on
        the env's stream that changes nothing of the env.  Returns a dict of CUDA tensors with K = max_after entries per
        slot: n_legal [n] int32 (the full count, also beyond K), action / status [n][K] uint8, reward / winner [n][K] int8,
        features [n][K][10] float64, obs [n][K][27][5][4] int32 (obs=True only: 2 160 bytes per entry), before_features
        [n][10] float64.  Entry k is the k-th legal action in ascending order; entries k >= min(n_legal, K) hold action 255
        and are otherwise stale, entries with status != 0 have no features / obs (include/monsoon.h).  The tensors are
        allocated on the first call per (n, max_after, obs) and overwritten in place by every later one (a later call
        allocates nothing and can be captured).  One set is kept per obs flag: a call with another max_after, or after a
        reset to another n, replaces it, and the dict returned before must no longer be used.  Stream ordering as in step."""
        import torch
        if self.views is None:
            raise MonsoonError("VecEnv.afterstates before reset")
        if not isinstance(max_after, int) or not 1 <= max_after <= 156:
            raise ValueError("max_after must be an integer in 1..156")
        obs = bool(obs)
        if obs not in self._after or self._after[obs][0] != (self.n, max_after):
            # one set per obs flag: a call with another n or max_after replaces it (9.1 GB at 65 536 slots, K = 64 with obs)
            self._after.pop(obs, None)
            dev = torch.device("cuda", self.device)
            t = {}
            for name, shape, dt in _AFTER:
                if name == "obs" and not obs:
                    continue
                shape = tuple(max_after if d == "K" else d for d in shape)
                t[name] = torch.zeros((self.n,) + shape, dtype=getattr(torch, dt), device=dev)
            t["action"].fill_(255)
            self._after[obs] = ((self.n, max_after), t, EnvAfter(**{name: x.data_ptr() for name, x in t.items()}))
        _, tensors, struct = self._after[obs]
        self._on_env_stream(lambda: self.engine.env_afterstates_dev(struct, max_after))
        return tensors

    @property
    def entry_bytes(self):
        """The size of one saved slot (monsoon_env_entry_bytes); needs reset() first."""
        if self.views is None:
            raise MonsoonError("VecEnv.entry_bytes before reset")
        return self.engine.env_entry_bytes()

    def _index(self, t, name, m=None):
        """An int32 CUDA tensor [m] on this env's device (m None: any length) -> (contiguous tensor, length)."""
        import torch
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or not t.is_cuda or t.device.index != self.device or t.dim() != 1
                or (m is not None and t.shape[0] != m)):
            raise ValueError(f"{name} must be an int32 CUDA tensor of shape ({'m' if m is None else m},) on device {self.device}")
        return t.contiguous(), int(t.shape[0])

    def _on_env_stream(self, call):
        """call(), a launch on the env's stream, ordered against torch's current stream on both sides -- unless that IS the
        env's stream (a step captured on it): then nothing waits, which is what lets single-stream capture work."""
        import torch
        cur = torch.cuda.current_stream(self.device)
        env = self.stream
        if cur.cuda_stream != env.cuda_stream:
            env.wait_stream(cur)   # the call's inputs were written, its outputs may still be read, on torch's stream
        call()
        if cur.cuda_stream != env.cuda_stream:
            cur.wait_stream(env)

    def snapshot(self, slots=None, out=None):
        """Save slots (monsoon_env_save_dev): entry j = slot slots[j] (an int32 CUDA tensor [m]; None = every slot, in
        order).  Returns an EnvSnapshot of m entries.  out = an earlier snapshot of this env's build with room for m
        entries: it is overwritten and returned, nothing is allocated and the call can be captured.  A slot index outside
        [0, n) leaves an entry that never loads.  One launch on the env's stream that changes nothing of the env; stream
        ordering as in step."""
        import torch
        if self.views is None:
            raise MonsoonError("VecEnv.snapshot before reset")
        size = self.entry_bytes
        m = self.n
        if slots is not None:
            slots, m = self._index(slots, "slots")
        if out is None:
            data = torch.zeros((m, size), dtype=torch.uint8, device=torch.device("cuda", self.device))
            out = EnvSnapshot(data, m, int(self.extended), size)
        else:
            self._check_snapshot(out)
            if out.capacity < m:
                raise ValueError(f"out holds {out.capacity} entries, {m} are to be saved")
            out.count = m
        if m:
            self._on_env_stream(lambda: self.engine.env_save_dev(out.data.data_ptr(), 0 if slots is None else slots.data_ptr(), m))
        return out

    def _check_snapshot(self, snap):
        import torch
        if not isinstance(snap, EnvSnapshot):
            raise ValueError("not an EnvSnapshot")
        if snap.extended != int(self.extended) or snap.entry_bytes != self.entry_bytes:
            raise ValueError(f"the snapshot is of record build {snap.extended} with {snap.entry_bytes}-byte entries, this env of build "
                             f"{int(self.extended)} with {self.entry_bytes}")
        d = snap.data
        if (not isinstance(d, torch.Tensor) or d.dtype != torch.uint8 or not d.is_cuda or d.device.index != self.device or d.dim() != 2
                or d.shape[1] != snap.entry_bytes or not d.is_contiguous() or d.data_ptr() % 16 or not 0 <= snap.count <= d.shape[0]):
            raise ValueError(f"snapshot data must be a contiguous uint8 CUDA tensor [cap][{snap.entry_bytes}] on device {self.device}")

    def _check_loaded(self, loaded, m):
        import torch
        if loaded is not None:
            if (not isinstance(loaded, torch.Tensor) or loaded.dtype not in (torch.uint8, torch.bool) or not loaded.is_cuda
                    or loaded.device.index != self.device or loaded.shape != (m,) or not loaded.is_contiguous()):
                raise ValueError(f"loaded must be a contiguous uint8 or bool CUDA tensor of shape ({m},) on device {self.device}")

    def restore(self, snap, src=None, dst=None, loaded=None):
        """Load saved slots (monsoon_env_load_dev): for every j, slot dst[j] becomes entry src[j] of snap (int32 CUDA
        tensors of one length m; None = j: without dst m <= n, without both m = len(snap)).  The same src may appear many
        times -- the fork; the same dst twice is an error of the caller with an unspecified result.  A pair whose src is
        outside [0, len(snap)) or whose dst is outside [0, n), or whose entry was never written, is skipped: the slot and
        its views stay untouched.  loaded (a uint8 or bool CUDA tensor [m]) receives 1 per loaded pair, 0 per skipped one.
        A slot loaded from its own entry replays its future bit for bit; loaded elsewhere it follows the source until
        the episode ends and the destination's seed schedule after it, and plays the destination's opponent row.  Returns
        the view tensors: those of the loaded slots read as after a step that ended nothing (done 0, reward 0, winner -2,
        episode = the entry's count) in the restored state.  Two launches on the env's stream, no allocation: the call can be
        captured.  Stream ordering as in step.  ValueError for a snapshot of another build or entry size and for tensors
        of wrong dtype, device or shape; MonsoonError before reset."""
        import torch
        if self.views is None:
            raise MonsoonError("VecEnv.restore before reset")
        self._check_snapshot(snap)
        m = None
        if src is not None:
            src, m = self._index(src, "src")
        if dst is not None:
            dst, m = self._index(dst, "dst", m)
        if m is None:
            m = snap.count
        if dst is None and m > self.n:
            raise ValueError(f"{m} entries into {self.n} slots: give dst")
        if m > self.engine.max_games:
            raise ValueError(f"at most max_slots = {self.engine.max_games} pairs per call")
        self._check_loaded(loaded, m)
        if m:
            self._on_env_stream(lambda: self.engine.env_load_dev(snap.data.data_ptr(), snap.count, 0 if src is None else src.data_ptr(),
                                                                 0 if dst is None else dst.data_ptr(), m,
                                                                 0 if loaded is None else loaded.data_ptr()))
        return self.views

    def determinize(self, snap, seeds, src=None, dst=None, observer=None, what="hand", loaded=None):
        """restore() that draws again what an observer cannot see (monsoon_env_load_determinized_dev): the fork of an
        information-set search.  snap, src, dst and loaded are restore's, with restore's rules and skipped pairs.  seeds is
        a contiguous CUDA tensor [m] of 32-bit seeds, one per pair: int32 holding the uint32's bits (the seed s >= 2**31 is
        s - 2**32; torch.from_numpy(np.asarray(s, dtype=np.uint32).view(np.int32)) makes it), or torch.uint32 where torch has
        it.  The tensor is read on the device by every call, so a captured call sees the seeds written into it since.

        what="stream": the loaded slot's stream becomes numpy.random.RandomState(seeds[j]) at its start, so its draws,
        random picks and scripted-bot choices are a fresh sample and no longer the real game's.  what="hand" (standard
        record only) also re-deals the hidden side's hand uniformly from its hand and deck (determinize_order gives the
        permutation; b305's returned object stays).  The hidden side is the one that `observer` is not: None = the side to
        move in the entry's state, 0 / 1 = that side for every pair, or a uint8 CUDA tensor [m] of 0 / 1 / 255 (255 = the
        side to move; any other byte skips the pair).  An entry whose episode has ended or has its end pending loads as
        restore loads it.  With observer None the views of a loaded slot are those restore gives: what the side to move sees
        does not change.  Nothing of decks() changes.

        Returns the view tensors.  Three launches on the env's stream; with an int observer a tensor [m] is allocated on the
        first call per (m, observer) and kept, so a later call allocates nothing and can be captured.  Stream ordering as in
        step.  ValueError for what="hand" on VecEnv(extended != 0) (use what="stream") and for arguments of wrong type,
        dtype, device or shape; MonsoonError before reset."""
        import torch
        if what not in DETERMINIZE:
            raise ValueError(f"what must be one of {sorted(DETERMINIZE)}, got {what!r}")
        if what == "hand" and int(self.extended) != 0:
            raise ValueError(f'what="hand" re-deals the standard record\'s hand and deck entries; this VecEnv is of record build '
                             f'{int(self.extended)}, whose lists hold object ids: use what="stream"')
        if isinstance(observer, bool) or not (observer is None or isinstance(observer, (int, torch.Tensor))):
            raise ValueError("observer must be None, 0, 1 or a uint8 CUDA tensor")
        if isinstance(observer, int) and observer not in (0, 1):
            raise ValueError(f"observer must be None, 0, 1 or a uint8 CUDA tensor, got {observer}")
        if self.views is None:
            raise MonsoonError("VecEnv.determinize before reset")
        self._check_snapshot(snap)
        m = None
        if src is not None:
            src, m = self._index(src, "src")
        if dst is not None:
            dst, m = self._index(dst, "dst", m)
        if m is None:
            m = snap.count
        if dst is None and m > self.n:
            raise ValueError(f"{m} entries into {self.n} slots: give dst")
        if m > self.engine.max_games:
            raise ValueError(f"at most max_slots = {self.engine.max_games} pairs per call")
        seed_types = (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ())
        if (not isinstance(seeds, torch.Tensor) or seeds.dtype not in seed_types or not seeds.is_cuda or seeds.device.index != self.device
                or seeds.shape != (m,) or not seeds.is_contiguous()):
            raise ValueError(f"seeds must be a contiguous int32 (the uint32's bits) or uint32 CUDA tensor of shape ({m},) on device {self.device}")
        if isinstance(observer, torch.Tensor):
            if (observer.dtype != torch.uint8 or not observer.is_cuda or observer.device.index != self.device or observer.shape != (m,)
                    or not observer.is_contiguous()):
                raise ValueError(f"observer must be a contiguous uint8 CUDA tensor of shape ({m},) on device {self.device}")
        elif observer is not None:
            key = (m, observer)
            if key not in self._observers:
                self._observers[key] = torch.full((m,), observer, dtype=torch.uint8, device=torch.device("cuda", self.device))
            observer = self._observers[key]
        self._check_loaded(loaded, m)
        if m:
            self._on_env_stream(lambda: self.engine.env_load_determinized_dev(
                snap.data.data_ptr(), snap.count, 0 if src is None else src.data_ptr(), 0 if dst is None else dst.data_ptr(), m,
                seeds.data_ptr(), 0 if observer is None else observer.data_ptr(), DETERMINIZE[what], 0 if loaded is None else loaded.data_ptr()))
        return self.views

    def state_hash(self):
        """monsoon_state_hash of every slot's current state (synchronises)."""
        return self.engine.state_hash()


__all__ = ["VecEnv", "EnvSnapshot", "OpponentExplore", "opponent_explore_draws", "determinize_order", "DETERMINIZE", "OPPONENTS", "MonsoonError", "select_actions"]
