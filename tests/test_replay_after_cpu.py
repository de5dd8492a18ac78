"""Rows that carry every legal action's afterstate (monsoon_replay_logged_after_dev, game_log's candidate columns), without
a device: the model the GPU tests compare with (tests/replay_after_model.py) pinned to the reference's own decisions, the
pure-torch helpers candidates / candidate_mask under vec_env.select_actions, and dataset's column handling."""
import os

import numpy as np
import pytest

import heuristic_model as HM
import replay_after_model as AM
import replay_model as RM
from monsoon_amd import _lib, game_log
from monsoon_amd.engine import MATCH_DTYPE
from monsoon_amd.vec_env import select_actions

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture_schedule(g):
    """(matches, deck pairs, action, steps) of a heuristic trace: weight row 0 on both sides, a deck pair per game where
    the fixture has them."""
    n = len(g["seeds"])
    if "decks" in g.files:
        pairs = g["decks"]
    else:
        pairs = np.stack([g["deck"], g["deck1"] if "deck1" in g.files else g["deck"]])[None]
    m = np.zeros(n, dtype=MATCH_DTYPE)
    m["seed"] = g["seeds"]
    if len(pairs) > 1:
        m["deck"] = np.arange(n)
    return (m, pairs) + RM.fixture_log(g)


def test_model_pinned_to_the_reference():
    """The first 4 games of trace_heuristic_S12, every row: the decision rebuilt from the model's candidates with the
    independent score is the reference's action, best score (bits) and legal count, and the scores are Oracle.decide's."""
    g = np.load(os.path.join(GOLD, "trace_heuristic_S12.npz"))
    m, pairs, action, steps = fixture_schedule(g)
    games, off, w0 = range(4), g["offsets"], g["w0"]
    score = HM.ScoreCache()
    seen = 0
    for r, i, k, row, orc in AM.rows(m, pairs, action, steps, 156, games):
        j = int(off[i]) + k
        assert r == j and row["n_legal"] == g["nlegal"][j] == len(row["entries"]), (i, k)
        status = [e["status"] for e in row["entries"]]
        best, s_best, s = AM.decision(w0, row["before"], status, [e["features"] for e in row["entries"]], score)
        assert row["entries"][best]["action"] == g["action"][j] == row["action"], (i, k)
        assert np.float64(s_best).tobytes() == g["best"][j].tobytes(), (i, k, s_best, g["best"][j])
        assert row["entries"][row["chosen"]]["action"] == g["action"][j], (i, k)
        a, scores, _ = orc.decide(0, w0)
        assert a == g["action"][j], (i, k)
        assert np.array(s).tobytes() == scores[[e["action"] for e in row["entries"]]].tobytes(), (i, k)
        seen += 1
    assert seen == off[4] == steps[:4].sum()   # no row is left out


def _rows():
    """Four hand-made rows, K = 3: all three entries; n_legal 2 (a stale third entry); a raised entry; n_legal 5 > K."""
    import torch
    return {"action": torch.tensor([9, 9, 9, 9], dtype=torch.uint8),
            "n_legal": torch.tensor([3, 2, 3, 5], dtype=torch.int32),
            "chosen": torch.tensor([1, 0, 2, 4], dtype=torch.int16),
            "after_action": torch.tensor([[4, 20, 155], [7, 155, 255], [1, 2, 3], [10, 11, 12]], dtype=torch.uint8),
            "after_status": torch.tensor([[0, 0, 0], [0, 0, 77], [0, 3, 0], [0, 2, 0]], dtype=torch.uint8),
            "after_reward": torch.zeros((4, 3), dtype=torch.int8), "after_winner": torch.full((4, 3), -2, dtype=torch.int8),
            "after_features": torch.arange(4 * 3 * 10, dtype=torch.float64).reshape(4, 3, 10),
            "before_features": torch.zeros((4, 10), dtype=torch.float64)}


def test_candidates_and_mask_under_select_actions():
    import torch
    d = _rows()
    c = game_log.candidates(d)
    assert set(c) == {"action", "status", "n_legal", "reward", "winner", "features"}   # (no after_obs in these rows)
    assert c["action"] is d["after_action"] and c["features"] is d["after_features"] and c["n_legal"] is d["n_legal"]
    mask = game_log.candidate_mask(d)
    assert mask.dtype == torch.bool
    assert mask.tolist() == [[True, True, True], [True, True, False], [True, False, True], [True, False, True]]
    nan = float("nan")
    values = torch.tensor([[1.0, 5.0, 5.0],     # the first maximum
                           [0.0, -1.0, 99.0],   # the best value sits beyond n_legal
                           [1.0, 99.0, nan],    # the best value sits on a raised entry, a NaN ranks below every number
                           [nan, 9.0, nan]])    # n_legal > K: only NaN values on the entries left
    assert select_actions(c, values).tolist() == [20, 7, 1, 10]
    d["after_obs"] = torch.zeros((4, 3, 27, 5, 4), dtype=torch.int32)
    assert game_log.candidates(d)["obs"] is d["after_obs"]
    with pytest.raises(ValueError):
        game_log.candidates({"action": d["action"]})
    with pytest.raises(ValueError):
        game_log.candidate_mask({"action": d["action"]})


def test_column_handling():
    plain = tuple(game_log.COLUMNS)
    assert game_log._want(plain) == plain and game_log._columns_for(plain, None) == plain   # the default means what it meant
    assert game_log._max_after(plain, 64) == 0 and game_log._max_after(plain, None) == 0
    assert game_log._want(("obs",)) == ("obs", "action")
    assert tuple(game_log.CANDIDATE_COLUMNS) == AM.AFTER_COLS
    assert not set(game_log.CANDIDATE_COLUMNS) & set(game_log.COLUMNS)
    names = game_log._want(("after_features",))
    assert names == ("after_features", "action", "n_legal", "after_action", "after_status")
    assert game_log._columns_for(("chosen", "n_legal"), np.zeros(1, np.int8)) == ("chosen", "n_legal", "action", "after_action", "after_status",
                                                                                   "game", "to_play")
    assert game_log._max_after(names, 64) == 64 and game_log._max_after(names, np.int64(1)) == 1 and game_log._max_after(names, 156) == 156
    for bad in (0, 157, -1, None, 8.0, True):
        with pytest.raises(ValueError):
            game_log._max_after(names, bad)
    for bad in (("after_value",), ("obs", "afterfeatures"), ("features",)):
        with pytest.raises(ValueError):
            game_log._want(bad)
    # the binding: monsoon_replay_after's fields in the header's order, the entry point in the table
    assert [f for f, _ in _lib.ReplayAfter._fields_] == ["n_legal", "chosen", "action", "status", "reward", "winner", "features",
                                                         "before_features", "obs"]
    res, args = _lib.SIGNATURES["monsoon_replay_logged_after_dev"]
    assert args[:-2] == _lib.SIGNATURES["monsoon_replay_logged_dev"][1] and len(args) == 17
