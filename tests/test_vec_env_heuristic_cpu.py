"""CPU tests of the vector env's heuristic opponent (include/monsoon.h opponent 2, monsoon_env_set_opponents): the ABI is
exported, bound and declared, and the Python model the GPU tests compare against (tests/vec_env_heuristic_model.py) is
pinned to the reference's own HeuristicAgent traces and to the oracle's rollout loop."""
import os

import numpy as np
import pytest

from monsoon_amd.cards import deck_indices
from vec_env_heuristic_model import FAULT_OPP_BOUND, OPP_BOUND, HeuristicVecEnvModel

TRACES = ("trace_heuristic_N12M_2w.npz", "trace_heuristic_S12.npz", "trace_heuristic_IRONCLAD.npz")


def test_set_opponents_exported_bound_and_named():
    from monsoon_amd import _lib
    from monsoon_amd.vec_env import OPPONENTS
    for ext in (0, 1, 2):
        assert hasattr(_lib.load(ext), "monsoon_env_set_opponents"), ext
    assert "monsoon_env_set_opponents" in _lib.SIGNATURES
    assert OPPONENTS["heuristic"] == 2
    from monsoon_amd.engine import BatchEngine
    assert hasattr(BatchEngine, "env_set_opponents")


def test_fault_code_of_the_opponent_bound_is_declared():
    from conftest import REPO
    base = open(os.path.join(REPO, "monsoon_amd", "csrc", "msb_base.h")).read()
    header = open(os.path.join(REPO, "include", "monsoon.h")).read()
    assert f"FAULT_OPP_BOUND = {FAULT_OPP_BOUND}," in base and OPP_BOUND == 64
    assert "fault 28 (FAULT_OPP_BOUND" in header and "int monsoon_env_set_opponents(" in header


def test_heuristic_opponent_needs_weights_before_any_device_work():
    from monsoon_amd.vec_env import VecEnv
    env = VecEnv.__new__(VecEnv)   # no device: the checks come before anything reaches the library
    env.n, env.views, env._heuristic = 0, None, False
    deck = np.stack([deck_indices("N12M")] * 2)
    with pytest.raises(ValueError, match="opponent_weights"):
        env.reset(np.arange(4), deck, opponent="heuristic")
    with pytest.raises(ValueError, match=r"\[10\] or \[k\]\[10\]"):
        env.reset(np.arange(4), deck, opponent="heuristic", opponent_weights=np.zeros((2, 9)))
    with pytest.raises(ValueError, match="4 integers"):
        env.reset(np.arange(4), deck, opponent="heuristic", opponent_weights=np.zeros((2, 10)), opponent_rows=[0, 1])
    with pytest.raises(ValueError, match=r"\[0, 2\)"):
        env.reset(np.arange(4), deck, opponent="heuristic", opponent_weights=np.zeros((2, 10)), opponent_rows=[0, 1, 2, 0])
    with pytest.raises(ValueError, match="need opponent"):
        env.reset(np.arange(4), deck, opponent="expert", opponent_weights=np.zeros(10))


def replay_trace(g, agent_side):
    """Replays every game of a HeuristicAgent self-play trace through one model slot (stride 1: consecutive seeds are the
    slot's consecutive episodes): the agent plays the recorded actions of `agent_side`, a heuristic opponent with the other
    side's weights answers.  Returns [(episode log [(action, hash)], final views)] per game."""
    w = (g["w0"], g["w1"] if "w1" in g.files else g["w0"])
    deck = np.stack([g["deck"], g["deck1"] if "deck1" in g.files else g["deck"]])
    log = []
    env = HeuristicVecEnvModel([int(g["seeds"][0])], w[agent_side ^ 1], decks=deck[None], agent_side=agent_side, seed_stride=1,
                               max_steps=int(g["max_turns"]), on_commit=lambda j, ep, a, h: log.append((ep, a, h)))
    out = []
    for k in range(len(g["seeds"])):
        lo, hi = int(g["offsets"][k]), int(g["offsets"][k + 1])
        while True:
            t = lo + sum(1 for e, _, _ in log if e == k)
            assert t < hi, (k, t)
            v = env.step([int(g["action"][t])])
            if v["done"][0]:
                break
        out.append(([(a, h) for e, a, h in log if e == k], {name: np.array(x[0]) for name, x in v.items()}))
    return out


def opp_bound_cut(actions, agent_side):
    """Where the env's guard ends a trace game: the opponent's 64th decision of one turn that is not a PASS (None: never)."""
    side, run = 0, 0
    for t, a in enumerate(actions):
        if side != agent_side:
            run += 1
            if run == OPP_BOUND and a != 155:
                return t + 1
        if a == 155:
            side, run = side ^ 1, 0
    return None


def check_replay(g, games, agent_side):
    """Every recorded action and canonical hash of both sides, and the way each game ended.  Returns the games the
    opponent guard ended."""
    from vec_env_model import is_noop_use
    faults = g["fault"] if "fault" in g.files else np.zeros(len(g["seeds"]), dtype=np.uint8)
    cuts = 0
    for k, (mine, v) in enumerate(games):
        lo, hi = int(g["offsets"][k]), int(g["offsets"][k + 1])
        cut = opp_bound_cut(g["action"][lo:hi], agent_side)
        if cut is not None:   # the reference's agent repeats a no-op USE until max_turns: the env's guard ends the turn
            assert [a for a, _ in mine] == [int(x) for x in g["action"][lo:lo + cut]], k
            assert [h for _, h in mine] == [int(x) for x in g["hash"][lo:lo + cut]], k
            assert v["fault"] == FAULT_OPP_BOUND and v["winner"] == -1 and not v["truncated"], k
            assert all(is_noop_use(a) for a, _ in mine[-32:]), k
            cuts += 1
            continue
        assert [a for a, _ in mine] == [int(x) for x in g["action"][lo:hi]], k
        last = hi - 1 if faults[k] else hi
        assert [h for _, h in mine[:last - lo]] == [int(x) for x in g["hash"][lo:last]], k
        if faults[k]:
            assert v["fault"] != 0 and v["winner"] == -1, k
            continue
        assert v["fault"] == 0 and v["winner"] == g["result"][k], k
        assert bool(v["truncated"]) == (hi - lo == int(g["max_turns"]) and v["winner"] == -1), k
        assert v["episode"] == k + 1
    return cuts


@pytest.mark.parametrize("agent_side", [0, 1])
@pytest.mark.parametrize("fixture", TRACES)
def test_model_reproduces_heuristic_traces(oracle_mod, gold, fixture, agent_side):
    """Reference-anchored: against a heuristic opponent with the other side's weights, an agent that replays one side's
    recorded actions sees the other side's every recorded action and state; max_steps = max_turns truncates the episode
    exactly where the trace ends.  agent_side 1 has the opponent play the opening turn of every episode."""
    g = gold(fixture)
    if fixture.endswith("_2w.npz"):
        assert not np.array_equal(g["w0"], g["w1"])
    cuts = check_replay(g, replay_trace(g, agent_side), agent_side)
    # N12M_2w: 2 games end in a no-op USE loop of SECOND (w1) and 5 in one of FIRST (w0) that only max_turns stops
    assert cuts == ({0: 2, 1: 5}[agent_side] if fixture.endswith("_2w.npz") else 0)


@pytest.mark.parametrize("agent_side", [0, 1])
def test_model_equals_the_rollout_loop(oracle_mod, agent_side):
    """An agent playing Oracle.decide(w_a) against the heuristic opponent w_b is the oracle's rollout(w_a, w_b): same
    result, committed steps and final state, on 60 seeds of three deck pairs (max_steps = max_turns).  The rollout has
    no opponent guard: a seed whose opponent the guard stops is left out, and at least 20 are checked."""
    rs = np.random.RandomState(7 + agent_side)
    w_a, w_b = rs.uniform(0, 1, 10), rs.uniform(0, 1, 10)
    ref = oracle_mod.Oracle(1)
    max_turns = 150
    checked = 0
    for seed in range(60):
        names = (("N12M", "N12M"), ("S12", "N12M"), ("IRONCLAD", "S12"))[seed % 3]
        deck = np.stack([deck_indices(x) for x in names])
        episodes = []
        model = HeuristicVecEnvModel([seed], w_b, decks=deck[None], agent_side=agent_side, max_steps=max_turns,
                                     on_commit=lambda j, ep, a, h: episodes.append(ep))
        while True:
            v = model.step([model.orc.decide(0, w_a)[0]])
            if v["done"][0]:
                break
        if model.bot_bound_hits:
            assert v["fault"][0] == FAULT_OPP_BOUND
            continue
        ref.reset(0, seed, deck[0], deck[1])
        w1, w2 = (w_a, w_b) if agent_side == 0 else (w_b, w_a)
        r = ref.rollout(0, w1, w2, max_turns)
        assert int(v["winner"][0]) == r["result"], seed
        assert episodes.count(0) == r["steps"], seed
        assert (v["fault"][0] != 0) == (r["fault"] != 0), seed
        assert bool(v["truncated"][0]) == (r["steps"] == max_turns and r["result"] == -1 and r["fault"] == 0), seed
        assert int(v["final_hash"][0:1].view(np.uint64)[0]) == ref.canon_hash(0), seed
        checked += 1
    assert checked >= 20


def test_model_opponent_bound_is_a_no_op_use_loop(oracle_mod):
    """The guard's turns: wherever the model ends a turn with fault 28, its last 32 decisions are USE actions that do
    nothing (so the reference's loop would repeat them until max_turns)."""
    from vec_env_model import is_noop_use
    pop = np.load(os.path.join(os.path.dirname(__file__), "golden", "population_seed42.npz"))
    w = pop[pop.files[0]].reshape(-1, 10)[:8]
    n = 16
    model = HeuristicVecEnvModel(np.arange(n) + 500, w, opponent_rows=np.arange(n) % len(w),
                                 decks=np.stack([deck_indices("N12M"), deck_indices("S12")]), max_steps=400)
    rs = np.random.RandomState(3)
    for _ in range(60):
        acts = []
        for j in range(n):
            la = model.orc.legal_actions(j)
            acts.append(la[rs.randint(len(la))])
        model.step(acts)
    for turn in model.opp_bound_turns:
        assert len(turn) == OPP_BOUND and all(is_noop_use(a) for a in turn[-32:]), turn
