"""CPU tests of the afterstates (include/monsoon.h monsoon_env_afterstates_dev, VecEnv.afterstates / select_actions): the
Python model the GPU tests compare against (tests/env_afterstates_model.py) is pinned to the independent feature model
and to the oracle's own decision, select_actions is checked on hand-made tensors, and the ABI is declared and exported."""
import os

import numpy as np
import pytest

import heuristic_model
from env_afterstates_model import AfterstatesModel, History
from monsoon_amd.cards import deck_indices
from vec_env_model import VecEnvModel

PAIRS = [("N12M", "N12M"), ("N12V", "S12"), ("IRONCLAD", "SWARM"), ("S12", "N12M"), ("SWARM", "N12V")]


def _random_legal(rs, legal):
    u = rs.random_sample(legal.shape)
    u[~legal] = -1.0
    return u.argmax(axis=1).astype(np.uint8)


def _walk(opponent, agent_side, n, steps, seed):
    """A random walk of a VecEnvModel with its afterstates model: yields (t, model, afterstates model) before every step."""
    pairs = [np.stack([deck_indices(a), deck_indices(b)]) for a, b in PAIRS]
    decks = np.stack([pairs[i % len(pairs)] for i in range(n)])
    seed0 = (np.arange(n, dtype=np.uint32) * 104729 + seed).astype(np.uint32)
    hist = History()
    model = VecEnvModel(seed0, decks, opponent=opponent, agent_side=agent_side, max_steps=60, on_commit=hist)
    am = AfterstatesModel(model, hist)
    rs = np.random.RandomState(seed)
    for t in range(steps):
        yield t, model, am
        model.step(_random_legal(rs, model.views["legal"]))


@pytest.mark.parametrize("opponent,agent_side", [(0, 0), (1, 1)])
def test_model_features_are_the_independent_models(opponent, agent_side):
    """The successor features the model hands out equal heuristic_model.features(successor observation) bit for bit, and
    the entries are the ascending legal list of the slot's views."""
    checked = 0
    for t, model, am in _walk(opponent, agent_side, 6, 30, 5 + opponent):
        for j in range(model.m):
            s = am.slot(j, 156)
            if model.result[j] != -2:
                assert s["n_legal"] == 0
                continue
            assert [e["action"] for e in s["entries"]] == np.nonzero(model.views["legal"][j])[0].tolist()
            if s["before"] is not None:
                assert s["before"].tobytes() == heuristic_model.features(model.views["obs"][j]).tobytes()
            for e in s["entries"]:
                if e["status"] == 0:
                    assert e["features"].tobytes() == heuristic_model.features(e["obs"]).tobytes(), (t, j, e["action"])
                    checked += 1
    assert checked > 1000, checked


def test_first_maximum_of_the_models_scores_is_the_oracles_decision():
    """heuristic_model's score over (before_features, features), 0.0 where the look-ahead raised: its first maximum is
    Oracle.decide's action on the same state."""
    rs = np.random.RandomState(17)
    score = heuristic_model.ScoreCache()
    decisions = 0
    for t, model, am in _walk(0, 0, 5, 30, 23):
        for j in range(model.m):
            if model.result[j] != -2:
                continue
            w = rs.uniform(-1.0, 1.0, 10)
            s = am.slot(j, 156)
            am.rebuild(j)
            a, _, _ = am.orc.decide(0, w)
            scores = [score(w, s["before"], e["features"]) if (e["status"] == 0 and s["before"] is not None) else 0.0 for e in s["entries"]]
            assert s["entries"][heuristic_model.first_max(scores)]["action"] == a, (t, j)
            decisions += 1
    assert decisions > 100, decisions


def _after(n_legal, action, status):
    import torch
    return dict(n_legal=torch.tensor(n_legal, dtype=torch.int32), action=torch.tensor(action, dtype=torch.uint8),
                status=torch.tensor(status, dtype=torch.uint8))


def test_select_actions_on_hand_made_tensors():
    import torch
    from monsoon_amd.vec_env import select_actions
    after = _after(
        [3, 4, 6, 0, 2, 1],
        [[10, 20, 30, 255], [5, 6, 7, 8], [1, 2, 3, 4], [255, 255, 255, 255], [40, 155, 255, 255], [33, 255, 255, 255]],
        [[0, 0, 0, 9], [0, 2, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [17, 2, 0, 0], [0, 0, 0, 0]])
    values = torch.tensor([
        [1.0, 7.0, 7.0, 99.0],    # a tie: the first maximum; the stale entry beyond n_legal is not looked at
        [1.0, 50.0, 3.0, 3.0],    # the best entry's look-ahead raised: masked, then a tie of the rest
        [0.0, 0.0, 0.0, 5.0],     # n_legal > K: every one of the K entries counts
        [9.0, 9.0, 9.0, 9.0],     # n_legal == 0 (a pending end): 255
        [4.0, 8.0, 100.0, 100.0],  # every existing entry raised: PASS
        [-np.inf, 0.0, 0.0, 0.0]])  # a single entry valued -inf is still the maximum
    got = select_actions(after, values)
    assert got.dtype == torch.uint8 and got.tolist() == [20, 7, 4, 255, 155, 33]
    # integer and float32 values, and all-equal values: the first legal entry
    assert select_actions(after, torch.zeros(6, 4, dtype=torch.int64)).tolist() == [10, 5, 1, 255, 155, 33]
    assert select_actions(after, values.to(torch.float32)).tolist() == [20, 7, 4, 255, 155, 33]
    with pytest.raises(ValueError):
        select_actions(after, torch.zeros(6, 3))


def test_afterstates_symbol_declared_exported_and_bound():
    from conftest import REPO
    from monsoon_amd import _lib
    name = "monsoon_env_afterstates_dev"
    header = open(os.path.join(REPO, "include", "monsoon.h")).read()
    assert f"int {name}(monsoon_t* h, const monsoon_env_after* out, int32_t max_after);" in header
    for ext in (0, 1, 2):
        assert hasattr(_lib.load(ext), name), ext
    assert name in _lib.SIGNATURES
    assert _lib.ctypes.sizeof(_lib.EnvAfter) == 8 * 8   # eight device pointers

