"""Python model of the vector env with softmax heuristic opponents (include/monsoon.h, monsoon_env_set_opponent_sample)
over the CPU oracle (test helper): ExploringVecEnvModel whose opponent turn applies the sampling rule between the unchanged
oracle's decide and step --

    g, scores, mask = decide(weights[row]);  legal = sorted(mask);  k = the episode's committed steps;  s = the episode's seed
    a = g
    if (until_step <= 0 or k < until_step) and hash32(seed, s, k, 0) < thresholds[slot]:
        w = sample_weights(scores[legal], scores[g], inv_temperature[slot])
        if sum(w): a = legal[sample_rank(w, hash32(seed, s, k, 1))]
    step(a)

-- with the weights and the rank of monsoon_amd.game_log and the draws of monsoon_amd.fitness.hash32.  It counts the sampled
decisions per slot (`explored`, the counter both kinds of rule share) and writes every opponent decision down (Decision,
below).  lockstep_case() is a configuration the GPU lockstep test plays, computed once per process and shared with the CPU
test that proves its coverage; forked() is the model of an entry loaded into another slot."""
import collections
import functools

import numpy as np

import vec_env_explore_model as X
from monsoon_amd import game_log
from monsoon_amd.fitness import hash32
from vec_env_explore_model import league, legal_list, mixed_decks, random_legal, thresholds_of  # noqa: F401  (the tests' helpers)
from vec_env_heuristic_model import FAULT_OPP_BOUND, OPP_BOUND

ONE = 1 << 24

# One decision of an opponent: the legal count, the sampled rank in the ascending legal list (-1 = the draw did not say
# "sample", or the weights summed to 0), the arg-max's rank, the sum of the weights and the committed action's weight (0 where
# rank is -1), whether a legal action weighed 0, whether two weights were 2**24, the arg-max and the committed action ids, the
# episode's step index, whether the commit ended the episode, whether the decision belongs to an opening turn (the opponent
# plays before the agent ever acted in the episode), whether draw0 was below the slot's threshold at a step index that
# until_step excludes, and the model's slot.
Decision = collections.namedtuple(
    "Decision", "n_legal rank greedy_rank weight_total taken_weight zero_weight tie greedy taken k ended opening late_below slot")


class SamplingVecEnvModel(X.ExploringVecEnvModel):
    """thresholds uint32 [n] and inv_temperatures float64 [n] over the WHOLE env, taken for the model's slots."""

    def __init__(self, seed0, opponent_weights, opponent_rows=None, explore_seed=0, until_step=0, thresholds=None, inv_temperatures=None,
                 slots=None, **kw):
        n_all = len(np.asarray(seed0))
        sl = np.arange(n_all) if slots is None else np.asarray(slots, dtype=np.int64)
        self.inv_t = np.asarray(np.ones(n_all) if inv_temperatures is None else inv_temperatures, dtype=np.float64)[sl]
        super().__init__(seed0, opponent_weights, opponent_rows, explore_seed=explore_seed, until_step=until_step, thresholds=thresholds,
                         slots=slots, **kw)

    def set_sample(self, seed, until_step, thresholds, inv_temperatures, slots=None):
        """A retune: applies from the next decision (as monsoon_env_set_opponent_sample between steps)."""
        self.set_explore(seed, until_step, thresholds, slots)
        self.inv_t = np.asarray(inv_temperatures, dtype=np.float64)[self.slots if slots is None else slots]

    def _bot_turn(self, j):
        turn = []
        w = self.weights[self.rows[j]]
        for _ in range(OPP_BOUND):
            if self.orc.to_play(j) == self.agent_side:
                return
            g, scores, mask = self.orc.decide(j, w)
            g = int(g)
            if self.on_decide is not None:
                self.on_decide(j, g, mask)
            legal = legal_list(mask)
            k, s = int(self.steps[j]), self.seed(j)
            below = hash32(self.explore_seed, s, k, 0) < int(self.thresholds[j])
            in_time = self.until_step <= 0 or k < self.until_step
            a, rank, total, taken, zero, tie = g, -1, 0, 0, False, False
            if below and in_time:
                self.explored[j] += 1   # (the draw said "sample", whatever is drawn)
                wt = game_log.sample_weights(np.asarray(scores)[legal], scores[g], self.inv_t[j])
                total = int(wt.astype(np.uint64).sum())
                if total:
                    rank = game_log.sample_rank(wt, hash32(self.explore_seed, s, k, 1))
                    a, taken = legal[rank], int(wt[rank])
                    zero, tie = bool((wt == 0).any()), int((wt == ONE).sum()) >= 2
            turn.append(a)
            fs, _, _ = self.orc.step(j, a)
            ended = self._after_step(j, a, fs)
            self.decisions.append(Decision(len(legal), rank, legal.index(g), total, taken, zero, tie, g, a, k, bool(ended), self._opening,
                                           bool(below and not in_time), j))
            if ended:
                return
        if self.orc.to_play(j) != self.agent_side:
            self.bot_bound_hits += 1
            self.opp_bound_turns.append(turn)
            self._end(j, -1, FAULT_OPP_BOUND)


# The GPU lockstep configuration (tests/test_vec_env_sample_gpu.py), standard record: n slots, `steps` steps of a
# random-legal agent, max_steps 90, a league of 8 rows, epsilon by slot % 4 crossed with the temperature by (slot // 4) % 3 --
# three decades, so that a slot of every epsilon plays near-greedy, loosely and almost uniformly -- and every
# (agent_side, until_step) below.  The seeds were chosen on the CPU (tests/test_vec_env_sample_cpu.py asserts what they were
# chosen for).
LOCKSTEP_N, LOCKSTEP_STEPS, LOCKSTEP_MAX_STEPS = 256, 120, 90
LOCKSTEP_EPS = (0.0, 0.1, 0.5, 1.0)
LOCKSTEP_T = (0.02, 0.2, 2.0)
LOCKSTEP_CASES = ((0, 0), (1, 40))   # (agent_side, until_step)
LOCKSTEP_SAMPLE_SEED = 4242


def eps_of(n):
    return np.array([LOCKSTEP_EPS[i % 4] for i in range(n)])


def temperatures_of(n):
    return np.array([LOCKSTEP_T[(i // 4) % 3] for i in range(n)])


def lockstep_config(agent_side, until_step, n=LOCKSTEP_N):
    seed0 = (np.arange(n, dtype=np.uint32) * 7919 + 23 + 1000 * agent_side + until_step).astype(np.uint32)
    w = league(8)
    rows = (np.arange(n) * 5) % len(w)
    eps, temperature = eps_of(n), temperatures_of(n)
    return dict(seed0=seed0, decks=mixed_decks(n), weights=w, rows=rows, eps=eps, thresholds=thresholds_of(eps), temperature=temperature,
                inv_temperatures=1.0 / temperature, explore_seed=LOCKSTEP_SAMPLE_SEED + agent_side, until_step=until_step,
                agent_side=agent_side, max_steps=LOCKSTEP_MAX_STEPS, policy_seed=agent_side + until_step)


def open_model(spec, slots=None, **kw):
    """The model of the env `spec` (lockstep_config's keys) over `slots` (None = all)."""
    return SamplingVecEnvModel(spec["seed0"], spec["weights"], spec["rows"], explore_seed=spec["explore_seed"], until_step=spec["until_step"],
                               thresholds=spec["thresholds"], inv_temperatures=spec["inv_temperatures"], agent_side=spec["agent_side"],
                               max_steps=spec["max_steps"], slots=slots, **({"decks": spec["decks"]} if "decks" in spec else {}), **kw)


@functools.lru_cache(maxsize=None)
def lockstep_case(agent_side, until_step):
    """The model's run of one lockstep case: (config, reset views, reset hashes, reset explored, [(actions, views, hashes,
    explored) per step], decisions, model)."""
    c = lockstep_config(agent_side, until_step)
    model = open_model(c)
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
    """vec_env_explore_model.forked under the sampling rule: slot src_slot of the env `spec` plays the actions `prefix` from
    reset, is saved, and the entry is loaded into slot dst_slot of the env dst_spec (None = the same env).  From the load on
    the slot's configuration is the destination's -- seed0, threshold, inverse temperature, weight row -- while the episode
    in flight and the episode count are the carried ones."""
    import env_snapshot_model
    model = open_model(spec, slots=[src_slot])
    for a in prefix:
        model.step([int(a)])
    d = spec if dst_spec is None else dst_spec
    env_snapshot_model._move(model, dict(seed0=d["seed0"], agent_side=d["agent_side"], max_steps=d["max_steps"],
                                         opponent_weights=d["weights"], opponent_rows=d["rows"]), dst_slot)
    model.set_sample(d["explore_seed"], d["until_step"], d["thresholds"], d["inv_temperatures"], np.array([dst_slot]))
    return model
