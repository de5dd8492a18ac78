"""CPU tests of the vector env's epsilon-greedy heuristic opponents (monsoon_env_set_opponent_explore, VecEnv
opponent_explore): the model of the contract (tests/vec_env_explore_model.py) against the plain heuristic model, the rule's
edges on the model, the two new exports, the host side of the Python layer, and the proof that the configuration the GPU
lockstep test plays contains every kind of explored decision the kernel treats differently."""
import os
import re

import numpy as np
import pytest

import vec_env_explore_model as M
from conftest import REPO
from monsoon_amd.fitness import hash32
from vec_env_heuristic_model import HeuristicVecEnvModel

NEW_SYMBOLS = ("monsoon_env_set_opponent_explore", "monsoon_env_opponent_explored_dev")


def test_library_exports_the_new_symbols():
    """As tests/test_abi.py checks exports: the loaded library has them, include/monsoon.h declares them, the binding
    knows them."""
    from monsoon_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "monsoon.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(monsoon_[a-z_0-9]+)\s*\(", text))
    for ext in (0, 1, 2):
        lib = _lib.load(ext)
        for name in NEW_SYMBOLS:
            assert hasattr(lib, name), (ext, name)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
    assert re.search(r"typedef struct \{\s*uint32_t seed;.*?int32_t\s+until_step;.*?\} monsoon_env_explore;", text, flags=re.S)
    assert [f[0] for f in _lib.EnvExplore._fields_] == ["seed", "until_step"]


def test_python_layer_thresholds_and_draws():
    from monsoon_amd.engine import Explore
    from monsoon_amd.vec_env import OpponentExplore, opponent_explore_draws
    ox = OpponentExplore([0.0, 0.1, 0.5, 1.0, 1e-12], seed=2**32 + 5, until_step=7)
    t = ox.thresholds(5)
    assert t.dtype == np.uint32 and ox.seed == 5 and ox.until_step == 7
    assert t.tolist() == [Explore(e, 0).threshold for e in (0.0, 0.1, 0.5, 1.0, 1e-12)] == M.thresholds_of(ox.eps).tolist()
    assert t[0] == 0 and t[3] == 0xFFFFFFFF
    assert OpponentExplore(0.25, 1).thresholds(3).tolist() == [2**30] * 3
    with pytest.raises(ValueError):
        ox.thresholds(4)
    for bad in (-0.1, 1.5, float("nan"), [[0.1]]):
        with pytest.raises(ValueError):
            OpponentExplore(bad, 1)
    seeds = np.array([0, 1, 0xFFFFFFFF, 123456789], dtype=np.uint32)
    for k in (0, 1, 39, 40, 65535):
        d0, d1 = opponent_explore_draws(77, seeds, k)
        assert d0.dtype == np.uint32 and d0.tolist() == [hash32(77, int(s), k, 0) for s in seeds]
        assert d1.tolist() == [hash32(77, int(s), k, 1) for s in seeds]


def _small(n, agent_side, **kw):
    seed0 = (np.arange(n, dtype=np.uint32) * 7919 + 5).astype(np.uint32)
    w = M.league(8)
    rows = (np.arange(n) * 3) % len(w)
    return dict(seed0=seed0, decks=M.mixed_decks(n), weights=w, rows=rows, agent_side=agent_side, max_steps=90, **kw)


def _open(c, slots=None):
    return M.ExploringVecEnvModel(c["seed0"], c["weights"], c["rows"], explore_seed=c["explore_seed"], until_step=c["until_step"],
                                  thresholds=c["thresholds"], decks=c["decks"], agent_side=c["agent_side"], max_steps=c["max_steps"],
                                  slots=slots)


def test_zero_thresholds_equal_the_plain_opponent():
    n, steps = 64, 150
    c = _small(n, 1, explore_seed=9, until_step=0, thresholds=np.zeros(n, dtype=np.uint32))
    a_model = _open(c)
    b_model = HeuristicVecEnvModel(c["seed0"], c["weights"], c["rows"], decks=c["decks"], agent_side=1, max_steps=90)
    rs = np.random.RandomState(1)
    for k in a_model.views:
        assert np.array_equal(a_model.views[k], b_model.views[k]), k
    for t in range(steps):
        a = M.random_legal(rs, b_model.views["legal"])
        va, vb = a_model.step(a), b_model.step(a)
        for k in vb:
            assert np.array_equal(va[k], vb[k]), (t, k)
        assert np.array_equal(a_model.hashes(), b_model.hashes()), t
    assert a_model.explored.sum() == 0 and all(d.r == -1 and d.taken == d.greedy for d in a_model.decisions)
    assert b_model.episode.sum() >= n // 2


def test_until_step_stops_exploration_at_exactly_that_index():
    n, until = 32, 12
    c = _small(n, 1, explore_seed=3, until_step=until, thresholds=np.full(n, 0xFFFFFFFF, dtype=np.uint32))
    model = _open(c)
    rs = np.random.RandomState(2)
    for _ in range(40):
        model.step(M.random_legal(rs, model.views["legal"]))
    ks = {True: set(), False: set()}
    for d in model.decisions:
        assert (d.r >= 0) == (d.k < until), d   # (threshold 2^32 - 1: all but one draw in 2^32 says "explore")
        ks[d.r >= 0].add(d.k)
        assert d.late_below == (d.k >= until), d
    assert until - 1 in ks[True] and until in ks[False] and max(ks[True]) == until - 1 and min(ks[False]) == until
    assert model.explored.sum() == sum(d.r >= 0 for d in model.decisions) > 0


def test_equal_seed0_shares_the_draws_and_other_seed0_parts():
    """Slots 0 and 1 are the same slot twice (seed0, decks, row, threshold): given the same actions they stay identical.
    An entry of slot 0 loaded into slots with other seed0 is in one state everywhere and then parts; loaded into two slots
    of equal seed0 it stays one."""
    n = 8
    c = _small(n, 0, explore_seed=21, until_step=0, thresholds=np.full(n, 1 << 31, dtype=np.uint32))
    c["seed0"][1] = c["seed0"][0]
    c["seed0"][5] = c["seed0"][4]
    c["decks"][1] = c["decks"][0]
    c["rows"][:] = 2
    twins = _open(c, slots=[0, 1])
    rs = np.random.RandomState(4)
    prefix = []
    for t in range(30):
        a = M.random_legal(rs, twins.views["legal"][:1])[0]
        prefix.append(int(a))
        v = twins.step([a, a])
        assert twins.hashes()[0] == twins.hashes()[1] and not v["illegal"].any(), t
        assert all(np.array_equal(x[0], x[1]) for x in v.values()), t
    assert twins.explored[0] == twins.explored[1] > 0
    prefix = prefix[:6]
    forks = [M.forked(c, 0, prefix, d) for d in range(2, n)]
    assert len({int(f.hashes()[0]) for f in forks}) == 1
    for t in range(10):
        a = M.random_legal(rs, forks[0].views["legal"])[0]
        for f in forks:
            f.step([a if f.views["legal"][0][a] or a == 155 else 155])
        assert forks[2].hashes()[0] == forks[3].hashes()[0], t   # slots 4 and 5: equal seed0
    assert len({int(f.hashes()[0]) for f in forks}) >= 2


def test_lockstep_configuration_covers_every_kind_of_explored_decision():
    """What the GPU lockstep test plays (vec_env_explore_model.lockstep_case, all of LOCKSTEP_CASES), on the model alone.
    With U = 8 candidate lanes per pass the kernel can only go wrong where the explored rank lands in another pass than the
    arg-max's, at the edges of a pass, or where the taken candidate decides what follows: each kind is there."""
    every, explored = [], []
    for case in M.LOCKSTEP_CASES:
        c, _, _, _, trail, decisions, model = M.lockstep_case(*case)
        assert len(trail) == M.LOCKSTEP_STEPS and model.m == M.LOCKSTEP_N
        assert model.explored.sum() == sum(d.r >= 0 for d in decisions)
        assert all(d.r == -1 for d in decisions if c["thresholds"][d.slot] == 0)
        every += decisions
        explored += [d for d in decisions if d.r >= 0]
    assert all(0 <= d.r < d.n_legal for d in explored)
    kinds = {
        "r == 0": [d for d in explored if d.r == 0],
        "r == n_legal - 1": [d for d in explored if d.r == d.n_legal - 1],
        "8 <= r < 16": [d for d in explored if 8 <= d.r < 16],
        "r >= 16": [d for d in explored if d.r >= 16],
        "r in a ragged last pass": [d for d in explored if d.n_legal % 8 != 0 and d.r >= d.n_legal - d.n_legal % 8],
        "taken == greedy": [d for d in explored if d.taken == d.greedy],
        "n_legal == 1": [d for d in explored if d.n_legal == 1],
        "an explored commit ends its episode": [d for d in explored if d.ended],
        "explored in an opening turn": [d for d in explored if d.opening],
        "k >= until_step with draw0 below the threshold": [d for d in every if d.late_below],
    }
    print({k: len(v) for k, v in kinds.items()})
    for name, hits in kinds.items():
        assert hits, name
    # the passes themselves: an explored rank in a later pass than the arg-max's, and in an earlier one
    def rank(d):
        return d.r // 8
    greedy_pass = [d for d in explored if d.taken != d.greedy]
    assert any(d.taken > d.greedy and rank(d) >= 1 for d in greedy_pass) and any(d.taken < d.greedy for d in greedy_pass)
