"""Python model of the vector env with epsilon-greedy heuristic opponents (include/monsoon.h,
monsoon_env_set_opponent_explore) over the CPU oracle (test helper): HeuristicVecEnvModel whose opponent turn applies the
exploration rule between the unchanged oracle's decide and step --

    g, _, mask = decide(weights[row]);  legal = sorted(mask);  k = the episode's committed steps;  s = the episode's seed
    a = g
    if (until_step <= 0 or k < until_step) and hash32(seed, s, k, 0) < thresholds[slot]:
        a = legal[(hash32(seed, s, k, 1) * len(legal)) >> 32]
    step(a)

-- counts the explored decisions per slot and writes every opponent decision down (Decision, below).  lockstep_case() is
the configuration the GPU lockstep test plays, computed once per process and shared with the CPU test that proves its
coverage; forked() is the model of an entry loaded into another slot."""
import collections
import functools

import numpy as np

from monsoon_amd.fitness import hash32
from vec_env_heuristic_model import FAULT_OPP_BOUND, OPP_BOUND, HeuristicVecEnvModel

# One decision of an opponent: the legal count, the explored rank (-1 = the arg-max was committed), the arg-max, the
# committed action, the episode's step index, whether the commit ended the episode, whether the decision belongs to an
# opening turn (the opponent plays before the agent ever acted in the episode), whether draw0 was below the slot's
# threshold at a step index that until_step excludes, and the model's slot.
Decision = collections.namedtuple("Decision", "n_legal r greedy taken k ended opening late_below slot")


def legal_list(mask):
    return [x for x in range(156) if (int(mask[x >> 6]) >> (x & 63)) & 1]


def thresholds_of(eps):
    """OpponentExplore's: min(int(eps * 2**32), 0xFFFFFFFF) per slot, by Python integers."""
    return np.array([min(int(float(e) * 2**32), 0xFFFFFFFF) for e in np.atleast_1d(eps)], dtype=np.uint32)


class ExploringVecEnvModel(HeuristicVecEnvModel):
    """thresholds: uint32 [n] over the WHOLE env, taken for the model's slots (like opponent_rows)."""

    def __init__(self, seed0, opponent_weights, opponent_rows=None, explore_seed=0, until_step=0, thresholds=None, slots=None, **kw):
        n_all = len(np.asarray(seed0))
        sl = np.arange(n_all) if slots is None else np.asarray(slots, dtype=np.int64)
        self.explored = np.zeros(len(sl), dtype=np.int64)
        self.decisions = []
        self._opening = False
        self.set_explore(explore_seed, until_step, np.zeros(n_all, dtype=np.uint32) if thresholds is None else thresholds, sl)
        super().__init__(seed0, opponent_weights, opponent_rows, slots=slots, **kw)

    def set_explore(self, seed, until_step, thresholds, slots=None):
        """A retune: applies from the next decision (as monsoon_env_set_opponent_explore between steps)."""
        self.explore_seed, self.until_step = int(seed) & 0xFFFFFFFF, int(until_step)
        self.thresholds = np.asarray(thresholds, dtype=np.uint32)[self.slots if slots is None else slots].astype(np.int64)

    def _start(self, j):
        self._opening = True
        try:
            super()._start(j)
        finally:
            self._opening = False

    def _bot_turn(self, j):
        turn = []
        w = self.weights[self.rows[j]]
        for _ in range(OPP_BOUND):
            if self.orc.to_play(j) == self.agent_side:
                return
            g, _, mask = self.orc.decide(j, w)
            g = int(g)
            if self.on_decide is not None:
                self.on_decide(j, g, mask)
            legal = legal_list(mask)
            k, s = int(self.steps[j]), self.seed(j)
            below = hash32(self.explore_seed, s, k, 0) < int(self.thresholds[j])
            in_time = self.until_step <= 0 or k < self.until_step
            a, r = g, -1
            if below and in_time:
                r = (hash32(self.explore_seed, s, k, 1) * len(legal)) >> 32
                a = legal[r]
                self.explored[j] += 1
            turn.append(a)
            fs, _, _ = self.orc.step(j, a)
            ended = self._after_step(j, a, fs)
            self.decisions.append(Decision(len(legal), r, g, a, k, bool(ended), self._opening, bool(below and not in_time), j))
            if ended:
                return
        if self.orc.to_play(j) != self.agent_side:
            self.bot_bound_hits += 1
            self.opp_bound_turns.append(turn)
            self._end(j, -1, FAULT_OPP_BOUND)


def random_legal(rs, legal):
    """A uniformly drawn legal action per slot (PASS where none is): the policy of the env tests, restated here so that
    this helper imports no GPU test module."""
    out = np.full(len(legal), 155, dtype=np.uint8)
    for j, row in enumerate(legal):
        ids = np.nonzero(row)[0]
        if len(ids):
            out[j] = ids[rs.randint(len(ids))]
    return out


def league(k=8):
    """k GA individuals: the committed population's initial and offspring weights."""
    import os
    pop = np.load(os.path.join(os.path.dirname(__file__), "golden", "population_seed42.npz"))
    return np.concatenate([pop["init_weights"], pop["off_weights"]])[:k].copy()


def mixed_decks(n):
    """Slot i plays one of four deck pairs of the named decks (the standard record holds them all)."""
    from monsoon_amd.cards import deck_indices
    names = ("N12M", "S12", "IRONCLAD", "N12M")
    pairs = [np.stack([deck_indices(names[a]), deck_indices(names[(a + 1) % 3])]) for a in range(4)]
    return np.stack([pairs[i % 4] for i in range(n)])


# The GPU lockstep configuration (tests/test_vec_env_explore_gpu.py), standard record: n slots, `steps` steps of a
# random-legal agent, max_steps 90, a league of 8 rows, epsilon by slot % 4, every (agent_side, until_step) below.  The
# seeds were chosen on the CPU (tests/test_vec_env_explore_cpu.py asserts what they were chosen for).
LOCKSTEP_N, LOCKSTEP_STEPS, LOCKSTEP_MAX_STEPS = 256, 120, 90
LOCKSTEP_EPS = (0.0, 0.1, 0.5, 1.0)
LOCKSTEP_CASES = ((0, 0), (1, 40), (0, 40), (1, 0))   # (agent_side, until_step)
LOCKSTEP_EXPLORE_SEED = 2024


def lockstep_config(agent_side, until_step, n=LOCKSTEP_N):
    seed0 = (np.arange(n, dtype=np.uint32) * 7919 + 11 + 1000 * agent_side + until_step).astype(np.uint32)
    w = league(8)
    rows = (np.arange(n) * 5) % len(w)
    eps = np.array([LOCKSTEP_EPS[i % 4] for i in range(n)])
    return dict(seed0=seed0, decks=mixed_decks(n), weights=w, rows=rows, eps=eps, thresholds=thresholds_of(eps),
                explore_seed=LOCKSTEP_EXPLORE_SEED + agent_side, until_step=until_step, agent_side=agent_side,
                max_steps=LOCKSTEP_MAX_STEPS, policy_seed=agent_side + until_step)


@functools.lru_cache(maxsize=None)
def lockstep_case(agent_side, until_step):
    """The model's run of one lockstep case: (config, reset views, reset hashes, [(actions, views, hashes, explored) per
    step], decisions)."""
    c = lockstep_config(agent_side, until_step)
    model = ExploringVecEnvModel(c["seed0"], c["weights"], c["rows"], explore_seed=c["explore_seed"], until_step=until_step,
                                 thresholds=c["thresholds"], decks=c["decks"], agent_side=agent_side, max_steps=c["max_steps"])
    views0 = {k: v.copy() for k, v in model.views.items()}
    hashes0, explored0 = model.hashes(), model.explored.copy()
    rs = np.random.RandomState(c["policy_seed"])
    trail = []
    for _ in range(LOCKSTEP_STEPS):
        a = random_legal(rs, model.views["legal"])
        v = model.step(a)
        trail.append((a, {k: x.copy() for k, x in v.items()}, model.hashes(), model.explored.copy()))
    return c, views0, hashes0, explored0, trail, list(model.decisions), model


def forked(spec, src_slot, prefix, dst_slot, dst_spec=None):
    """The one-slot model of: slot src_slot of the env `spec` plays the actions `prefix` from reset, is saved, and the entry
    is loaded into slot dst_slot of the env dst_spec (None = the same env).  spec: seed0, decks, weights, rows, thresholds,
    explore_seed, until_step, agent_side, max_steps.  From the load on the slot's configuration is the destination's --
    seed0, threshold, weight row -- while the episode in flight and the episode count are the carried ones."""
    import env_snapshot_model
    model = ExploringVecEnvModel(spec["seed0"], spec["weights"], spec["rows"], explore_seed=spec["explore_seed"],
                                 until_step=spec["until_step"], thresholds=spec["thresholds"], decks=spec["decks"],
                                 agent_side=spec["agent_side"], max_steps=spec["max_steps"], slots=[src_slot])
    for a in prefix:
        model.step([int(a)])
    d = spec if dst_spec is None else dst_spec
    env_snapshot_model._move(model, dict(seed0=d["seed0"], agent_side=d["agent_side"], max_steps=d["max_steps"],
                                         opponent_weights=d["weights"], opponent_rows=d["rows"]), dst_slot)
    model.set_explore(d["explore_seed"], d["until_step"], d["thresholds"], np.array([dst_slot]))
    return model
