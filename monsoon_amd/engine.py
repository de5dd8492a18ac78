"""BatchEngine: numpy-facing wrapper of the C ABI (one handle = one GPU, a batch of games)."""
import ctypes

import numpy as np

from . import _lib
from ._lib import Config, Match, MonsoonError, Stats

MATCH_DTYPE = np.dtype([("p1", "<i4"), ("p2", "<i4"), ("seed", "<u4"), ("deck", "<u4")])   # monsoon_match
LOG_BUDGET = 256 << 20   # bytes of device log a batch of monsoon_rollout_logged may take (include/monsoon.h)


# The arrays of a logged rollout's log (csrc/host_layout.h LOG_COLUMN, in RolloutLog's order): name, dtype, the value behind
# a game's last step, bytes of device log per entry, and the entry point that introduces the array.
LOG_ARRAYS = (("action", np.uint8, 255, 1, "monsoon_rollout_logged"),
              ("score", np.float64, np.nan, 8, "monsoon_rollout_logged"),
              ("n_legal", np.int16, 0, 2, "monsoon_rollout_logged"),
              ("greedy", np.uint8, 255, 1, "monsoon_rollout_explore"),
              ("explored", np.uint8, 0, 1, "monsoon_rollout_explore"),
              ("taken_score", np.float64, np.nan, 8, "monsoon_rollout_explore"),
              ("weight_total", np.uint32, 0, 4, "monsoon_rollout_sample"),
              ("taken_weight", np.uint32, 0, 4, "monsoon_rollout_sample"))
# ... in the order in which each logs its predecessors' arrays too; monsoon_rollout_policies introduces none of its own
_LOG_ENTRIES = ("monsoon_rollout_logged", "monsoon_rollout_explore", "monsoon_rollout_sample", "monsoon_rollout_policies")


def _log_arrays(entry):
    """Names of the arrays a call of `entry` logs: the ones it introduces and its predecessors'."""
    return [name for name, *_, at in LOG_ARRAYS if _LOG_ENTRIES.index(at) <= _LOG_ENTRIES.index(entry)]


def _entry_bytes(**asked):
    """Bytes of device log one entry takes with the named arrays asked for (action always)."""
    return sum(size for name, _, _, size, _ in LOG_ARRAYS if name == "action" or asked.get(name))


def explore_entry_bytes(scores=True, n_legal=True, greedy=True, explored=True, taken_score=True):
    """Bytes of device log one entry of monsoon_rollout_explore takes, by the arrays asked for (action always): 1 .. 21."""
    return _entry_bytes(score=scores, n_legal=n_legal, greedy=greedy, explored=explored, taken_score=taken_score)


def sample_entry_bytes(scores=True, n_legal=True, greedy=True, explored=True, taken_score=True, weight_total=True, taken_weight=True):
    """Bytes of device log one entry of monsoon_rollout_sample takes, by the arrays asked for (action always): 1 .. 29."""
    return _entry_bytes(score=scores, n_legal=n_legal, greedy=greedy, explored=explored, taken_score=taken_score,
                        weight_total=weight_total, taken_weight=taken_weight)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class Explore:
    """The exploration rule of a logged rollout (monsoon_explore, include/monsoon.h): a heuristic decision of a side in
    `sides` ("first", "second", "both") at committed-step index k (k < until_step where until_step > 0) commits a
    uniformly drawn legal action instead of its arg-max with probability eps.  The draws are hash32(seed, match seed, k, .):
    game_log.explore_draws recomputes them.
    temperature = a finite T > 0 selects the sampling rule instead (monsoon_sample, monsoon_rollout_sample): such a decision
    commits an action drawn from the softmax over its scores, exp((score - best) / T) in 24-bit integer weights
    (game_log.sample_weights, game_log.sample_rank); inv_temperature = 1.0 / T is what the device multiplies by.  Actions
    tied for the best score share the probability equally.  temperature=None is the uniform rule, unchanged in every bit."""
    SIDES = {"first": 1, "second": 2, "both": 3}

    def __init__(self, eps, seed, sides="both", until_step=0, temperature=None):
        if not 0.0 <= eps <= 1.0:   # (a NaN fails it too)
            raise ValueError(f"Explore: eps must lie in [0, 1], got {eps!r}")
        if sides not in self.SIDES:
            raise ValueError(f"Explore: sides is one of {tuple(self.SIDES)}, got {sides!r}")
        self.temperature = self.inv_temperature = None
        if temperature is not None:
            if not 0.0 < temperature < float("inf"):   # (a NaN fails it too)
                raise ValueError(f"Explore: temperature must be finite and > 0, got {temperature!r}")
            self.temperature = float(temperature)
            self.inv_temperature = 1.0 / self.temperature
            if not self.inv_temperature < float("inf"):   # (a subnormal T)
                raise ValueError(f"Explore: 1 / temperature is not finite for {temperature!r}")
        self.eps, self.seed, self.sides, self.until_step = float(eps), int(seed) & 0xFFFFFFFF, sides, int(until_step)
        self.threshold = min(int(eps * 2**32), 0xFFFFFFFF)   # a decision explores iff draw0 < threshold
        self.side_bits = self.SIDES[sides]

    def may_explore(self, side, k):
        """The two conditions of the rule that are not the draw: the side's bit and the step limit (numpy or scalars)."""
        return (((self.side_bits >> side) & 1) != 0) & ((self.until_step <= 0) | (k < self.until_step))

    def c_struct(self):
        return _lib.Explore(self.seed, self.threshold, self.side_bits, self.until_step)

    @property
    def samples(self):
        """True for the sampling rule (a temperature), False for the uniform one."""
        return self.inv_temperature is not None

    def c_sample(self):
        """monsoon_sample of the sampling rule."""
        return _lib.Sample(self.c_struct(), self.inv_temperature)


class Policies:
    """An exploration rule per individual of a logged rollout (monsoon_policies, include/monsoon.h): a heuristic decision
    reads eps and temperature of the weight row that moves -- match p1 when FIRST is to play, p2 when SECOND is.  eps and
    temperature are array-likes with one entry per row of the weight table: eps in [0, 1] (0: the row plays greedily),
    temperature > 0, numpy.inf the uniform rule (inv_temperature 0.0: every legal action weighs the same).  seed, sides and
    until_step are call-wide, as on Explore.  The log carries weight_total and taken_weight on every decision the rule covers
    -- the side's bit, the step limit, eps > 0 -- sampled or not: game_log.behaviour_prob is the exact probability the
    behaviour policy gave every committed action."""
    SIDES = Explore.SIDES
    samples = True          # the log carries weight_total and taken_weight
    per_individual = True   # the rule is a table over the weight rows

    def __init__(self, eps, temperature, seed, sides="both", until_step=0):
        eps, temperature = np.asarray(eps, dtype=np.float64), np.asarray(temperature, dtype=np.float64)
        if eps.ndim != 1 or temperature.shape != eps.shape:
            raise ValueError(f"Policies: eps and temperature are one-dimensional and equally long, got shapes {eps.shape} and {temperature.shape}")
        if not ((eps >= 0.0) & (eps <= 1.0)).all():   # (a NaN fails it too)
            raise ValueError("Policies: every eps must lie in [0, 1]")
        if not (temperature > 0.0).all():   # (likewise)
            raise ValueError("Policies: every temperature must be > 0 (numpy.inf: the uniform rule)")
        if sides not in self.SIDES:
            raise ValueError(f"Policies: sides is one of {tuple(self.SIDES)}, got {sides!r}")
        with np.errstate(over="ignore"):
            inv = 1.0 / temperature
        if not np.isfinite(inv).all():   # (a subnormal T)
            raise ValueError("Policies: 1 / temperature is not finite for every row")
        self.eps, self.temperature, self._inv = eps.copy(), temperature.copy(), np.ascontiguousarray(inv)
        self._thresholds = np.minimum(np.floor(eps * 2.0**32), float(0xFFFFFFFF)).astype(np.uint32)   # (Explore.threshold per row: exact in float64)
        self.seed, self.sides, self.until_step = int(seed) & 0xFFFFFFFF, sides, int(until_step)
        self.side_bits = self.SIDES[sides]

    def __len__(self):
        return len(self._thresholds)

    @property
    def thresholds(self):
        """uint32[n_individuals]: row r's decisions leave the arg-max iff draw0 < thresholds[r]."""
        return self._thresholds

    @property
    def inv_temperatures(self):
        """float64[n_individuals]: 1 / temperature, what the device multiplies by (0.0 for numpy.inf)."""
        return self._inv

    may_explore = Explore.may_explore

    def c_struct(self):
        """monsoon_policies over this object's two tables (which it keeps alive)."""
        return _lib.Policies(self.seed, self.side_bits, self.until_step, _ptr(self._thresholds), _ptr(self._inv))


class RolloutLog:
    """What a logged rollout played (monsoon_rollout_logged): entry k of row i is game i's k-th committed step.
    action uint8[n][max_turns] (255 behind the last step), score float64[n][max_turns] or None (the decision's best score;
    NaN for a step of the scripted bot and behind the last step), n_legal int16[n][max_turns] or None (legal actions of
    the decision; 0 for a bot step and behind), steps int32[n] = the entries of each row.
    A rollout with an Explore rule (monsoon_rollout_explore) adds greedy uint8[n][max_turns] (the decision's arg-max action:
    the teacher's label where `action` was explored; 255 for a bot step and behind), explored uint8[n][max_turns] (1 = the
    decision's draw said "explore") and taken_score float64[n][max_turns] (score of the committed action; NaN for a bot
    step and behind); None otherwise.
    A rollout with a sampling rule (Explore(temperature=), monsoon_rollout_sample) adds to those weight_total
    uint32[n][max_turns] (the sum of the decision's 24-bit softmax weights) and taken_weight uint32[n][max_turns] (the weight
    of the committed action); both 0 for a bot step, a decision that did not sample, and behind; None otherwise.
    A rollout with a Policies table (monsoon_rollout_policies) has the same arrays; weight_total and taken_weight are there
    written on every decision the rule covers, sampled or not (game_log.behaviour_prob)."""

    def __init__(self, action, score, n_legal, steps, greedy=None, explored=None, taken_score=None, weight_total=None, taken_weight=None):
        self.action, self.score, self.n_legal, self.steps = action, score, n_legal, steps
        self.greedy, self.explored, self.taken_score = greedy, explored, taken_score
        self.weight_total, self.taken_weight = weight_total, taken_weight

    @classmethod
    def empty(cls, n, max_turns, scores=True, n_legal=True, explore=False, sample=False):
        """n rows of padding; explore: with the three arrays of an exploring rollout; sample: with those and the two of a
        sampling one."""
        asked = dict.fromkeys(_log_arrays(_LOG_ENTRIES[2 if sample else 1 if explore else 0]), True)
        asked.update(score=scores, n_legal=n_legal)
        arrays = {name: np.full((n, max_turns), pad, dtype=dtype) if asked.get(name) else None for name, dtype, pad, *_ in LOG_ARRAYS}
        return cls(steps=np.zeros(n, dtype=np.int32), **arrays)

    def taken_prob(self):
        """float64[n][max_turns]: taken_weight / weight_total, the probability the softmax gave the committed action GIVEN
        that the decision sampled; NaN where weight_total == 0 (a bot step, a decision that did not sample, behind the last
        step).  With eps < 1 the behaviour policy is the mixture include/monsoon.h spells out (monsoon_rollout_sample)."""
        if self.weight_total is None or self.taken_weight is None:
            raise ValueError("taken_prob needs the log of a rollout with a sampling rule (Explore(temperature=))")
        out = np.full(self.weight_total.shape, np.nan)
        np.divide(self.taken_weight, self.weight_total, out=out, where=self.weight_total != 0)
        return out

    def put(self, rows, other):
        """Rows `rows` become the rows of `other` (a log of len(rows) games with the same arrays)."""
        self.steps[rows] = other.steps
        for name, *_ in LOG_ARRAYS:
            if getattr(self, name) is not None:
                getattr(self, name)[rows] = getattr(other, name)


class BatchEngine:
    def __init__(self, max_games, device=0, lanes_per_game=0, stack_bytes=0, extended=False):
        """extended=True loads the build with the larger per-game record (decks holding ua20 / b005 or a unit / structure
        card twice: cards.needs_extended), extended=2 the
        one with the largest (254 entity slots; the replay tier of monsoon_amd/fitness.py).
        lanes_per_game selects a hot-kernel variant of the build (0 = default); a value the build does not hold is
        refused."""
        self.lib = _lib.load(extended)
        self.extended = extended
        self.h = ctypes.c_void_p()
        cfg = Config(device, max_games, lanes_per_game, stack_bytes)
        rc = self.lib.monsoon_create(ctypes.byref(cfg), ctypes.byref(self.h))
        if rc != _lib.OK:
            msg = self.lib.monsoon_last_error(self.h if self.h else None)
            if self.h:
                self.lib.monsoon_destroy(self.h)
            self.h = None
            raise MonsoonError(f"monsoon_create failed (status {rc}): {msg.decode() if msg else ''}")
        self.max_games = max_games
        self.device = device
        self.n = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.monsoon_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _ck(self, rc, what):
        _lib.check(self.h, rc, what, self.lib)

    # ---- Seam G, batched ------------------------------------------------------------------
    @staticmethod
    def _decks_factions(n, decks, factions):
        """decks as uint8[n][2][12] (one [2][12] pair stands for all n) and factions as uint8[n][2]; None stays None."""
        if decks is not None:
            decks = np.ascontiguousarray(decks, dtype=np.uint8)
            if decks.shape == (2, 12):
                decks = np.broadcast_to(decks, (n, 2, 12)).copy()
            if decks.shape != (n, 2, 12):
                raise ValueError(f"decks must be [n][2][12], got {decks.shape}")
        if factions is not None:
            factions = np.ascontiguousarray(factions, dtype=np.uint8).reshape(n, 2)
        return decks, factions

    def reset(self, seeds, decks, factions=None):
        seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
        n = len(seeds)
        decks, factions = self._decks_factions(n, decks, factions)
        self._ck(self.lib.monsoon_reset(self.h, n, _ptr(seeds), _ptr(decks), _ptr(factions)), "monsoon_reset")
        self.n = n

    def legal_mask(self):
        out = np.zeros((self.n, 3), dtype=np.uint64)
        self._ck(self.lib.monsoon_legal_mask(self.h, _ptr(out)), "monsoon_legal_mask")
        return out

    def legal_actions(self, i=0, mask=None):
        m = self.legal_mask()[i] if mask is None else mask
        return [a for a in range(156) if (int(m[a >> 6]) >> (a & 63)) & 1]

    def step(self, actions):
        actions = np.ascontiguousarray(actions, dtype=np.uint8)
        if actions.shape != (self.n,):
            raise ValueError("one action per game (255 = skip)")
        reward = np.zeros(self.n, dtype=np.int8)
        done = np.zeros(self.n, dtype=np.uint8)
        fault = np.zeros(self.n, dtype=np.uint8)
        self._ck(self.lib.monsoon_step(self.h, _ptr(actions), _ptr(reward), _ptr(done), _ptr(fault)), "monsoon_step")
        return reward, done, fault

    def expert_action(self):
        """Stormbound.expert_action for every game (consumes the games' streams)."""
        action = np.zeros(self.n, dtype=np.uint8)
        fault = np.zeros(self.n, dtype=np.uint8)
        self._ck(self.lib.monsoon_expert_action(self.h, _ptr(action), _ptr(fault)), "monsoon_expert_action")
        return action, fault

    def observe(self):
        out = np.zeros((self.n, 27, 5, 4), dtype=np.int32)
        raises = np.zeros(self.n, dtype=np.uint8)
        self._ck(self.lib.monsoon_observe(self.h, _ptr(out), _ptr(raises)), "monsoon_observe")
        return out, raises

    def game_faults(self):
        """Per-game fault code of the loaded batch (0 = none)."""
        out = np.zeros(self.n, dtype=np.uint8)
        self._ck(self.lib.monsoon_game_faults(self.h, _ptr(out)), "monsoon_game_faults")
        return out

    def observe_torch(self):
        """(n,27,5,4) int32 observation as a torch tensor ON THE GPU (no host copy), plus the raises mask.
        torch is used for device memory only."""
        import torch
        dev = torch.device("cuda", self.device)
        out = torch.empty((self.n, 27, 5, 4), dtype=torch.int32, device=dev)
        raises = torch.empty((self.n,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        self._ck(self.lib.monsoon_observe_dev(self.h, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(raises.data_ptr())),
                 "monsoon_observe_dev")
        return out, raises

    def features(self):
        out = np.zeros((self.n, 10), dtype=np.float64)
        self._ck(self.lib.monsoon_features(self.h, _ptr(out)), "monsoon_features")
        return out

    def status(self):
        out = np.zeros((self.n, 4), dtype=np.int32)
        self._ck(self.lib.monsoon_status(self.h, _ptr(out)), "monsoon_status")
        return out

    def export(self, i):
        buf = np.zeros(2048, dtype=np.uint8)
        ln = ctypes.c_int32()
        self._ck(self.lib.monsoon_state_export(self.h, i, _ptr(buf), ctypes.byref(ln)), "monsoon_state_export")
        return buf[:ln.value].tobytes()

    def variant(self):
        """(candidate lanes per game, waves per SIMD) of the hot kernel this handle runs."""
        u, w = ctypes.c_int32(), ctypes.c_int32()
        self._ck(self.lib.monsoon_variant(self.h, ctypes.byref(u), ctypes.byref(w)), "monsoon_variant")
        return u.value, w.value

    def save_state(self, i):
        """copy.deepcopy of game i (evo/game_adapter.py:280-287): the complete device state as an opaque blob."""
        buf = np.zeros(self.lib.monsoon_state_blob_bytes(), dtype=np.uint8)
        self._ck(self.lib.monsoon_state_save(self.h, i, _ptr(buf), len(buf)), "monsoon_state_save")
        return buf.tobytes()

    def load_state(self, i, blob):
        """Put a blob from save_state (any handle of the same build) into slot i; i == n appends a game."""
        buf = np.frombuffer(blob, dtype=np.uint8)
        self._ck(self.lib.monsoon_state_load(self.h, i, _ptr(buf), len(buf)), "monsoon_state_load")
        if i == self.n:
            self.n = i + 1

    def debug_build(self, i, seed, stream_pos, state):
        """Scenario tests: put game i into a described state (int32 stream, tests/scenario_lib.py); returns the fault code."""
        state = np.ascontiguousarray(state, dtype=np.int32)
        f = ctypes.c_int32()
        self._ck(self.lib.monsoon_debug_build(self.h, i, int(seed) & 0xFFFFFFFF, int(stream_pos), _ptr(state), len(state), ctypes.byref(f)),
                 "monsoon_debug_build")
        if i == self.n:
            self.n = i + 1
        return f.value

    def debug_op(self, i, op):
        """One engine call on game i; returns (fault code, [[card, position], ...] of the abilities that ran, in order)."""
        op = np.ascontiguousarray(op, dtype=np.int32)
        log = np.zeros(512, dtype=np.int32)
        f, n = ctypes.c_int32(), ctypes.c_int32()
        self._ck(self.lib.monsoon_debug_op(self.h, i, _ptr(op), len(op), ctypes.byref(f), _ptr(log), 256, ctypes.byref(n)), "monsoon_debug_op")
        return f.value, log[:2 * n.value].reshape(-1, 2).tolist()

    def debug_kat(self, kind, seed, n, inp=None):
        """Known-answer diagnostics (monsoon_debug_kat): 0 raw u32, 1 random(), 2 randint(0, inp[i]), 3 shuffle of range(12),
        4 scores of inp[n][30] = {weights, before, after}."""
        out = np.zeros((n, 12) if kind == 3 else n, dtype={0: np.uint32, 1: np.float64, 2: np.int32, 3: np.int32, 4: np.float64}[kind])
        if inp is not None:
            inp = np.ascontiguousarray(inp, dtype=np.int32 if kind == 2 else np.float64)
        self._ck(self.lib.monsoon_debug_kat(self.h, kind, int(seed) & 0xFFFFFFFF, n, _ptr(inp), _ptr(out)), "monsoon_debug_kat")
        return out

    def debug_sample_kat(self, scores, n_legal, best, inv_temperature, draw1):
        """monsoon_debug_sample_kat: the device's sampler on m caller-given decisions -- scores float64[m][156] (row i's first
        n_legal[i] entries are its legal list's scores), best float64[m], inv_temperature float64[m], draw1 uint32[m].
        Returns (rank int32[m] (-1 where total == 0), total uint32[m], weight uint32[m]): what game_log.sample_weights /
        sample_rank compute."""
        scores = np.ascontiguousarray(scores, dtype=np.float64).reshape(-1, 156)
        m = len(scores)
        n_legal, draw1 = np.ascontiguousarray(n_legal, dtype=np.int32), np.ascontiguousarray(draw1, dtype=np.uint32)
        best, inv_t = np.ascontiguousarray(best, dtype=np.float64), np.ascontiguousarray(inv_temperature, dtype=np.float64)
        if not (len(n_legal) == len(draw1) == len(best) == len(inv_t) == m):
            raise ValueError("debug_sample_kat: one entry per row of every argument")
        rank, total, weight = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint32)
        self._ck(self.lib.monsoon_debug_sample_kat(self.h, m, _ptr(scores), _ptr(n_legal), _ptr(best), _ptr(inv_t), _ptr(draw1), _ptr(rank),
                                                   _ptr(total), _ptr(weight)), "monsoon_debug_sample_kat")
        return rank, total, weight

    def debug_raw(self, i):
        buf = np.zeros(4096, dtype=np.uint8)
        ln = ctypes.c_int32()
        self._ck(self.lib.monsoon_debug_raw(self.h, i, _ptr(buf), ctypes.byref(ln)), "monsoon_debug_raw")
        return buf[:ln.value].copy()

    def state_hash(self):
        out = np.zeros(self.n, dtype=np.uint64)
        self._ck(self.lib.monsoon_state_hash(self.h, _ptr(out)), "monsoon_state_hash")
        return out

    # ---- vector env (monsoon_amd/vec_env.py drives these) ----------------------------------------
    def env_reset(self, config, views, seed0, decks=None, factions=None):
        """monsoon_env_reset: config = _lib.EnvConfig, views = _lib.EnvViews of device pointers; host seed0[n],
        decks[n][2][12] (None with a pool), factions[n][2] or None.  Synchronises."""
        seed0 = np.ascontiguousarray(seed0, dtype=np.uint32)
        n = len(seed0)
        decks, factions = self._decks_factions(n, decks, factions)
        self._ck(self.lib.monsoon_env_reset(self.h, ctypes.byref(config), ctypes.byref(views), n, _ptr(seed0), _ptr(decks),
                                            _ptr(factions)), "monsoon_env_reset")
        self.n = n

    def env_set_opponents(self, weights, rows, n):
        """monsoon_env_set_opponents: host weights[k][10] float64, rows[n] int32 or None (row 0 for every slot).  Synchronises."""
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.int32)
        self._ck(self.lib.monsoon_env_set_opponents(self.h, _ptr(weights), len(weights), _ptr(rows), int(n)), "monsoon_env_set_opponents")

    def env_set_opponent_explore(self, seed, until_step, thresholds):
        """monsoon_env_set_opponent_explore: the rule's seed and until_step, host thresholds[n] uint32 (slot i's opponent
        explores iff its draw0 < thresholds[i]); thresholds None clears the rule.  Synchronises."""
        if thresholds is None:
            self._ck(self.lib.monsoon_env_set_opponent_explore(self.h, None, None, 0), "monsoon_env_set_opponent_explore")
            return
        thresholds = np.ascontiguousarray(thresholds, dtype=np.uint32)
        ex = _lib.EnvExplore(int(seed) & 0xFFFFFFFF, int(until_step))
        self._ck(self.lib.monsoon_env_set_opponent_explore(self.h, ctypes.byref(ex), _ptr(thresholds), len(thresholds)),
                 "monsoon_env_set_opponent_explore")

    def env_set_opponent_sample(self, seed, until_step, thresholds, inv_temperatures):
        """monsoon_env_set_opponent_sample: monsoon_env_set_opponent_explore's rule whose decisions draw from the softmax
        over their scores, host inv_temperatures[n] float64 (1 / T of slot i, finite and > 0) beside the thresholds;
        thresholds None clears the rule.  Synchronises."""
        if thresholds is None:
            self._ck(self.lib.monsoon_env_set_opponent_sample(self.h, None, None, None, 0), "monsoon_env_set_opponent_sample")
            return
        thresholds = np.ascontiguousarray(thresholds, dtype=np.uint32)
        inv_temperatures = np.ascontiguousarray(inv_temperatures, dtype=np.float64)
        if inv_temperatures.shape != thresholds.shape:
            raise ValueError(f"inv_temperatures must be {thresholds.shape}, got {inv_temperatures.shape}")
        ex = _lib.EnvExplore(int(seed) & 0xFFFFFFFF, int(until_step))
        self._ck(self.lib.monsoon_env_set_opponent_sample(self.h, ctypes.byref(ex), _ptr(thresholds), _ptr(inv_temperatures), len(thresholds)),
                 "monsoon_env_set_opponent_sample")

    def env_opponent_explored(self, out_ptr):
        """monsoon_env_opponent_explored_dev: the explored decisions of every slot's opponent since the env's reset,
        uint32[n], into device memory at out_ptr (asynchronous on the handle's stream)."""
        self._ck(self.lib.monsoon_env_opponent_explored_dev(self.h, ctypes.c_void_p(out_ptr)), "monsoon_env_opponent_explored_dev")

    def debug_counters(self):
        """monsoon_debug_counters: the 192 raw counter words as uint64 (include/monsoon.h; synchronises)."""
        out = np.zeros(192, dtype=np.uint64)
        self._ck(self.lib.monsoon_debug_counters(self.h, _ptr(out)), "monsoon_debug_counters")
        return out

    def env_set_schedule(self, params):
        """monsoon_env_set_schedule: params = the fields of monsoon_deck_schedule (DeckEvolutionConfig.env_schedule, or a
        dict of the same fields; phase 0 = both archetypes, no draw), None clears the handle's schedule.  The schedule
        applies to every episode of a schedule-mode env that starts from the next step on.  Synchronises."""
        sc = None if params is None else self._deck_schedule(params)
        self._ck(self.lib.monsoon_env_set_schedule(self.h, None if sc is None else ctypes.byref(sc)), "monsoon_env_set_schedule")

    def env_decks_dev(self, out_ptr):
        """monsoon_env_decks_dev: the decks of every slot's current episode, uint8[n][2][12], into device memory at out_ptr
        (asynchronous on the handle's stream)."""
        self._ck(self.lib.monsoon_env_decks_dev(self.h, ctypes.c_void_p(out_ptr)), "monsoon_env_decks_dev")

    def env_reseed_time(self, enable=True):
        """monsoon_env_reseed_time: ms of the reseed kernel inside the last env step (0.0 if it was not timed); enable:
        whether later steps are timed (HIP events round that launch).  Synchronises."""
        ms = ctypes.c_double()
        self._ck(self.lib.monsoon_env_reseed_time(self.h, int(bool(enable)), ctypes.byref(ms)), "monsoon_env_reseed_time")
        return ms.value

    def env_step_dev(self, actions_ptr):
        """monsoon_env_step_dev on n bytes of device memory at actions_ptr (asynchronous on the handle's stream)."""
        self._ck(self.lib.monsoon_env_step_dev(self.h, ctypes.c_void_p(actions_ptr)), "monsoon_env_step_dev")

    def env_afterstates_dev(self, after, max_after):
        """monsoon_env_afterstates_dev: after = _lib.EnvAfter of device pointers with max_after entries per slot
        (asynchronous on the handle's stream; nothing of the handle changes)."""
        self._ck(self.lib.monsoon_env_afterstates_dev(self.h, ctypes.byref(after), int(max_after)), "monsoon_env_afterstates_dev")

    def env_entry_bytes(self):
        """monsoon_env_entry_bytes: the size of one saved slot of this record build (needs a loaded env)."""
        out = ctypes.c_int32()
        self._ck(self.lib.monsoon_env_entry_bytes(self.h, ctypes.byref(out)), "monsoon_env_entry_bytes")
        return int(out.value)

    def env_save_dev(self, entries_ptr, slots_ptr, m):
        """monsoon_env_save_dev: entry j at entries_ptr (device, 16-byte aligned) receives slot slots[j] (device int32[m] at
        slots_ptr, 0 = slot j).  Asynchronous on the handle's stream."""
        self._ck(self.lib.monsoon_env_save_dev(self.h, ctypes.c_void_p(entries_ptr), ctypes.c_void_p(slots_ptr or None), int(m)),
                 "monsoon_env_save_dev")

    def env_load_dev(self, entries_ptr, n_entries, src_ptr, dst_ptr, m, loaded_ptr):
        """monsoon_env_load_dev: slot dst[j] becomes entry src[j] for j < m (device int32[m] each, 0 = j); loaded_ptr =
        m device bytes or 0.  Asynchronous on the handle's stream."""
        self._ck(self.lib.monsoon_env_load_dev(self.h, ctypes.c_void_p(entries_ptr), int(n_entries), ctypes.c_void_p(src_ptr or None),
                                               ctypes.c_void_p(dst_ptr or None), int(m), ctypes.c_void_p(loaded_ptr or None)),
                 "monsoon_env_load_dev")

    def env_load_determinized_dev(self, entries_ptr, n_entries, src_ptr, dst_ptr, m, seeds_ptr, observers_ptr, what, loaded_ptr):
        """monsoon_env_load_determinized_dev: env_load_dev that draws again what the observer cannot see -- seeds_ptr =
        device uint32[m], observers_ptr = device uint8[m] or 0 (the side to move), what = 1 (the stream) or 3 (the stream
        and the hidden hand).  Asynchronous on the handle's stream."""
        self._ck(self.lib.monsoon_env_load_determinized_dev(self.h, ctypes.c_void_p(entries_ptr), int(n_entries), ctypes.c_void_p(src_ptr or None),
                                                            ctypes.c_void_p(dst_ptr or None), int(m), ctypes.c_void_p(seeds_ptr or None),
                                                            ctypes.c_void_p(observers_ptr or None), int(what),
                                                            ctypes.c_void_p(loaded_ptr or None)),
                 "monsoon_env_load_determinized_dev")

    def stream_ptr(self):
        """The hipStream_t the handle launches on (monsoon_stream), as an integer."""
        return self.lib.monsoon_stream(self.h) or 0

    # ---- Seam F ---------------------------------------------------------------------------
    def decide(self, weights, want_scores=False):
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if weights.shape == (10,):
            weights = np.broadcast_to(weights, (self.n, 2, 10)).copy()
        if weights.shape != (self.n, 2, 10):
            raise ValueError("weights must be [n][2][10]")
        action = np.zeros(self.n, dtype=np.uint8)
        best = np.zeros(self.n, dtype=np.float64)
        scores = np.zeros((self.n, 156), dtype=np.float64) if want_scores else None
        self._ck(self.lib.monsoon_decide(self.h, _ptr(weights), _ptr(action), _ptr(best), _ptr(scores)), "monsoon_decide")
        return (action, best, scores) if want_scores else (action, best)

    def rollout(self, weights, matches, deck_pairs, max_turns, want_results=False):
        return self._rollout("monsoon_rollout", weights, matches, deck_pairs, max_turns, want_results)

    def rollout_vs_expert(self, weights, matches, deck_pairs, max_turns, want_results=False):
        """monsoon_rollout_vs_expert: a rollout in which p1, p2 or both of a match may be monsoon_amd.EXPERT (-1), the
        reference's scripted bot.  counts[n][3] go to the row of the match's individual -- p1 if it is one (a win = FIRST
        won), else p2 (a win = SECOND won); results stay FIRST / SECOND, steps count both sides' committed steps."""
        return self._rollout("monsoon_rollout_vs_expert", weights, matches, deck_pairs, max_turns, want_results)

    def rollout_logged(self, weights, matches, deck_pairs, max_turns, scores=True, n_legal=True, explore=None):
        """monsoon_rollout_logged: rollout_vs_expert (the bot's rows included) that also writes down every committed step.
        Returns (counts, results, steps, log), log a RolloutLog whose score / n_legal are None where not asked for.
        explore = an Explore: monsoon_rollout_explore, the same call whose heuristic decisions may commit a drawn legal
        action; the log also carries greedy, explored and taken_score, and the counts describe the games that were played --
        they are not fitness.  An Explore with a temperature: monsoon_rollout_sample, whose decisions draw from the softmax
        over their scores; the log carries weight_total and taken_weight too (RolloutLog.taken_prob).  A Policies:
        monsoon_rollout_policies, the sampling call with the rule of the row that moves; its table has a row per row of
        `weights` (ValueError otherwise)."""
        sample = explore is not None and explore.samples
        table = getattr(explore, "per_individual", False)
        if table and len(explore) != len(weights):
            raise ValueError(f"rollout_logged: the Policies table has {len(explore)} rows, the weight table {len(weights)}")
        log = RolloutLog.empty(len(matches), max_turns, scores, n_legal, explore is not None, sample)
        entry = ("monsoon_rollout_logged" if explore is None else "monsoon_rollout_policies" if table else "monsoon_rollout_sample" if sample
                 else "monsoon_rollout_explore")
        return self._rollout(entry, weights, matches, deck_pairs, max_turns, True, log, explore) + (log,)

    @staticmethod
    def _rollout_args(weights, matches, deck_pairs):
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        deck_pairs = np.ascontiguousarray(deck_pairs, dtype=np.uint8).reshape(-1, 2, 12)
        m = np.ascontiguousarray(matches)
        if m.dtype != MATCH_DTYPE:
            arr = np.zeros(len(matches), dtype=MATCH_DTYPE)
            mm = np.asarray(matches)
            arr["p1"], arr["p2"], arr["seed"], arr["deck"] = mm[:, 0], mm[:, 1], mm[:, 2], mm[:, 3]
            m = arr
        return weights, m, deck_pairs

    def _rollout(self, entry, weights, matches, deck_pairs, max_turns, want_results, log=None, explore=None):
        """One rollout entry of the library.  log: the RolloutLog that monsoon_rollout_logged fills, one row per match (its
        steps are the call's steps); explore: the Explore of monsoon_rollout_explore, which fills the log's further arrays."""
        weights, m, deck_pairs = self._rollout_args(weights, matches, deck_pairs)
        n_ind = weights.shape[0]
        counts = np.zeros((n_ind, 3), dtype=np.int32)
        results = np.zeros(len(m), dtype=np.int8) if want_results else None
        steps = log.steps if log is not None else np.zeros(len(m), dtype=np.int32) if want_results else None
        extra, batch = (), self.max_games
        if log is not None:
            # the arrays each entry point introduces, as its struct of host pointers (_lib.RolloutLog / ExploreLog / SampleLog)
            c_logs = [struct(*(_ptr(getattr(log, name)) for name, *_, at in LOG_ARRAYS if at == e))
                      for e, struct in zip(_LOG_ENTRIES, (_lib.RolloutLog, _lib.ExploreLog, _lib.SampleLog))]
            extra = (ctypes.byref(c_logs[0]),)
            entry_bytes = 11   # a logged call's batches are cut by the log's budget too ...
            if explore is not None:   # ... an exploring or sampling call's by the arrays it asks for (include/monsoon.h)
                c_ex = explore.c_struct() if not explore.samples or getattr(explore, "per_individual", False) else explore.c_sample()
                extra += (ctypes.byref(c_ex),) + tuple(ctypes.byref(c) for c in c_logs[1:_LOG_ENTRIES.index(entry) + 1])
                entry_bytes = _entry_bytes(**{name: getattr(log, name) is not None for name in _log_arrays(entry)})
            batch = min(batch, max(1, LOG_BUDGET // (entry_bytes * max_turns)))
        self._ck(getattr(self.lib, entry)(self.h, _ptr(weights), n_ind, _ptr(m), len(m), _ptr(deck_pairs), len(deck_pairs),
                                          max_turns, _ptr(counts), _ptr(results), _ptr(steps), *extra), entry)
        self.n = len(m) - ((len(m) - 1) // batch) * batch   # the handle now holds the last batch of the schedule
        return (counts, results, steps) if want_results else counts

    def replay_logged(self, matches, deck_pairs, log_action, log_steps, rows, rows_cap, keep=None, after=None, max_after=0):
        """monsoon_replay_logged_dev: the logged games played again, one committed step per entry, the state before every
        kept entry written to row (kept entries before it) of `rows` -- a _lib.ReplayRows of DEVICE pointers with room for
        rows_cap rows.  log_action uint8[n][stride], log_steps int32[n], keep uint8[n][stride] or None (every entry).
        after = a _lib.ReplayAfter of DEVICE pointers with max_after entries per row (monsoon_replay_logged_after_dev): every
        kept entry's row also gets the afterstates of its state.
        Returns (rows written, status uint8[n] (_lib.REPLAY_*), replayed int32[n], fault uint8[n])."""
        _, m, deck_pairs = self._rollout_args(np.zeros((1, 10)), matches, deck_pairs)
        log_action = np.ascontiguousarray(log_action, dtype=np.uint8)
        log_steps = np.ascontiguousarray(log_steps, dtype=np.int32)
        if log_action.ndim != 2 or log_action.shape[0] != len(m) or log_steps.shape != (len(m),):
            raise ValueError("replay_logged: one log row and one step count per match")
        if keep is not None:
            keep = np.ascontiguousarray(keep, dtype=np.uint8)
            if keep.shape != log_action.shape:
                raise ValueError("replay_logged: keep has the shape of the log")
        status, replayed = np.zeros(len(m), dtype=np.uint8), np.zeros(len(m), dtype=np.int32)
        fault, n_rows = np.zeros(len(m), dtype=np.uint8), ctypes.c_int64(0)
        entry = "monsoon_replay_logged_dev" if after is None else "monsoon_replay_logged_after_dev"
        extra = () if after is None else (ctypes.byref(after), int(max_after))
        self._ck(getattr(self.lib, entry)(self.h, _ptr(m), len(m), _ptr(deck_pairs), len(deck_pairs), _ptr(log_action),
                                          log_action.shape[1], _ptr(log_steps), _ptr(keep), ctypes.byref(rows), int(rows_cap),
                                          ctypes.byref(n_rows), _ptr(status), _ptr(replayed), _ptr(fault), *extra), entry)
        self.n = len(m) - ((len(m) - 1) // self.max_games) * self.max_games   # the handle now holds the last batch
        return n_rows.value, status, replayed, fault

    def rollout_faults(self, n_matches):
        """Fault code of every game of the last rollout (>= 16: a limit of this build's record, see include/monsoon.h)."""
        out = np.zeros(n_matches, dtype=np.uint8)
        self._ck(self.lib.monsoon_rollout_faults(self.h, _ptr(out), n_matches), "monsoon_rollout_faults")
        return out

    def draw_decks(self, seeds, pool):
        """uint8[n][2][12]: RandomState(seed).choice(pool, 12, replace=False) twice per seed, drawn on the device
        (monsoon_draw_decks; configuration C5's per-game decks)."""
        seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
        pool = np.ascontiguousarray(pool, dtype=np.uint8)
        out = np.zeros((len(seeds), 2, 12), dtype=np.uint8)
        if len(seeds):
            self._ck(self.lib.monsoon_draw_decks(self.h, _ptr(seeds), len(seeds), _ptr(pool), len(pool), _ptr(out)), "monsoon_draw_decks")
        return out

    @staticmethod
    def _deck_schedule(params):
        """_lib.DeckSchedule (monsoon_deck_schedule) from a dict of its fields."""
        from ._lib import DeckSchedule
        arch = np.ascontiguousarray(params["archetype"], dtype=np.uint8)
        pool = np.ascontiguousarray(params["pool"], dtype=np.uint8)
        if arch.shape != (2, 12) or pool.shape != (2, 128):
            raise ValueError(f"archetype must be [2][12] and pool [2][128], got {arch.shape} and {pool.shape}")
        sc = DeckSchedule(int(params["seed"]), int(params["generation"]), int(params["tag"]), int(params["phase"]), int(params["n_preserve"]),
                          (ctypes.c_int32 * 2)(*[int(v) for v in params["pool_n"]]), float(params["balance_archetype_ratio"]))
        ctypes.memmove(sc.archetype, arch.ctypes.data, 24)
        ctypes.memmove(sc.pool, pool.ctypes.data, 256)
        return sc

    def draw_schedule(self, params, game_seeds):
        """uint8[n][2][12]: the per-game decks of a deck schedule, drawn on the device (monsoon_draw_schedule).  params:
        DeckEvolutionConfig.schedule_params(generation, tag), or a dict of the same fields; game_seeds: uint32[n].  Every
        pair equals DeckEvolutionConfig.game_decks(generation, game_seed, tag)."""
        game_seeds = np.ascontiguousarray(game_seeds, dtype=np.uint32)
        sc = self._deck_schedule(params)
        out = np.zeros((len(game_seeds), 2, 12), dtype=np.uint8)
        self._ck(self.lib.monsoon_draw_schedule(self.h, ctypes.byref(sc), _ptr(game_seeds), len(game_seeds), _ptr(out)), "monsoon_draw_schedule")
        return out

    def draw_schedule_time(self):
        """ms of the kernel inside the last draw_schedule call (HIP events; the call's copies are not in it)."""
        ms = ctypes.c_double()
        self._ck(self.lib.monsoon_draw_schedule_time(self.h, ctypes.byref(ms)), "monsoon_draw_schedule_time")
        return ms.value

    # ---- GA operators on the device (the host GA stays the default) -------------------------
    def ga_offspring(self, np_state, parents_w, parents_s, n_offspring, tau, tau_prime, min_sigma):
        """Population.generate_offspring on the device over numpy's global stream.  np_state: RandomState.get_state()
        (legacy tuple or dict).  Returns (weights[n][dim], sigmas[n][dim], parent[n], tries[n], new_state) with new_state
        in the form np.random.set_state accepts."""
        from ._lib import NpState
        if isinstance(np_state, dict):
            key, pos, hg, g = np_state["state"]["key"], np_state["state"]["pos"], np_state["has_gauss"], np_state["gauss"]
        else:
            _, key, pos, hg, g = np_state
        st = NpState()
        key = np.ascontiguousarray(key, dtype=np.uint32)   # kept alive across the memmove
        ctypes.memmove(st.key, key.ctypes.data, 624 * 4)
        st.pos, st.has_gauss, st.gauss = int(pos), int(hg), float(g)
        pw = np.ascontiguousarray(parents_w, dtype=np.float64)
        ps = np.ascontiguousarray(parents_s, dtype=np.float64)
        mu, dim = pw.shape
        ow, osg = np.zeros((n_offspring, dim)), np.zeros((n_offspring, dim))
        par, tries = np.zeros(n_offspring, dtype=np.int32), np.zeros(n_offspring, dtype=np.int64)
        self._ck(self.lib.monsoon_ga_offspring(self.h, ctypes.byref(st), _ptr(pw), _ptr(ps), mu, dim, n_offspring, float(tau), float(tau_prime),
                                               float(min_sigma), _ptr(ow), _ptr(osg), _ptr(par), _ptr(tries)), "monsoon_ga_offspring")
        new_key = np.ctypeslib.as_array(st.key).astype(np.uint32).copy()
        return ow, osg, par, tries, ("MT19937", new_key, int(st.pos), int(st.has_gauss), float(st.gauss))

    def ga_select(self, fitness):
        """Indices of all individuals by descending fitness, ties in original order (select_from_combined's sort)."""
        f = np.ascontiguousarray(fitness, dtype=np.float64)
        out = np.zeros(len(f), dtype=np.int32)
        self._ck(self.lib.monsoon_ga_select(self.h, _ptr(f), len(f), _ptr(out)), "monsoon_ga_select")
        return out

    # ---- device-resident rounds (bench) -------------------------------------------------------
    def upload_weights(self, weights):
        weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1, 10)
        self._ck(self.lib.monsoon_upload_weights(self.h, _ptr(weights), len(weights)), "monsoon_upload_weights")

    def assign_players(self, p1, p2):
        p1 = np.ascontiguousarray(p1, dtype=np.int32)
        p2 = np.ascontiguousarray(p2, dtype=np.int32)
        self._ck(self.lib.monsoon_assign_players(self.h, _ptr(p1), _ptr(p2)), "monsoon_assign_players")

    def decide_round(self):
        self._ck(self.lib.monsoon_decide_round_dev(self.h), "monsoon_decide_round_dev")

    def play_rounds(self, rounds):
        """`rounds` decisions of every loaded game in one launch (asynchronous; sync() waits)."""
        self._ck(self.lib.monsoon_play_rounds_dev(self.h, rounds), "monsoon_play_rounds_dev")

    def sync(self):
        self._ck(self.lib.monsoon_sync(self.h), "monsoon_sync")

    def stats(self):
        s = Stats()
        self._ck(self.lib.monsoon_get_stats(self.h, ctypes.byref(s)), "monsoon_get_stats")
        return {k: int(getattr(s, k)) for k, _ in Stats._fields_}

    def reset_stats(self):
        self._ck(self.lib.monsoon_reset_stats(self.h), "monsoon_reset_stats")

    def kernel_time(self):
        ms = ctypes.c_double()
        n = ctypes.c_int64()
        self._ck(self.lib.monsoon_kernel_time(self.h, ctypes.byref(ms), ctypes.byref(n)), "monsoon_kernel_time")
        return ms.value, n.value
