"""The model of monsoon_replay_logged_dev (tests/replay_model.py) pinned to the reference's fixtures, and the host logic
of game_log.dataset / dataset_batches (row bases, keep, batch cuts, outcome).  No GPU."""
import functools
import os
import re

import numpy as np
import pytest

import replay_model as RM
from monsoon_amd import _lib, game_log
from monsoon_amd.engine import MATCH_DTYPE

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fixture_call(name):
    """(g, matches, deck pairs, action, steps) of a reference trace as a replay call."""
    g = np.load(os.path.join(GOLD, name + ".npz"))
    n = len(g["seeds"])
    m = np.zeros(n, dtype=MATCH_DTYPE)
    m["seed"], m["deck"] = g["seeds"], np.arange(n)
    if name == "trace_live_expert":
        m["p1"] = m["p2"] = RM.EXPERT
    if "bot_side" in g.files:
        m["p1"] = np.where(g["bot_side"] == 1, 0, RM.EXPERT)
        m["p2"] = np.where(g["bot_side"] == 1, RM.EXPERT, 0)
    action, steps = RM.fixture_log(g)
    return g, m, np.stack([g["deck0"], g["deck1"]], axis=1), action, steps


@functools.lru_cache(maxsize=None)
def model_of(name):
    g, m, pairs, action, steps = fixture_call(name)
    return g, steps, RM.replay(m, pairs, action, steps)


@functools.lru_cache(maxsize=None)
def checked_of(name):
    """(rows checked against the reference, rows) of the model's replay of a fixture; raises where a row differs."""
    g, steps, out = model_of(name)
    return RM.check_fixture(g, out, game_log.row_bases(steps)[0], steps, bot_fixture=name == "trace_live_expert")


FIXTURES = ("trace_random_S12", "trace_live_expert", "trace_vs_expert", "trace_pool_up")


@pytest.mark.parametrize("name", FIXTURES)
def test_model_equals_the_reference(name):
    g, steps, out = model_of(name)
    base, total = game_log.row_bases(steps)
    assert total == int(steps.sum()) == len(out["action"]) and out["reached"].all()
    assert not out["status"].any() and np.array_equal(out["replayed"], steps)
    checked, rows = checked_of(name)
    print(f"{name}: {checked} of {rows} rows checked against the reference, {int(out['obs_raises'].sum())} rows with obs_raises")
    if name == "trace_pool_up":
        # every game ends on a step that raises or after which the observation does: the game's fault.  A ROW whose
        # observation raises is only ever a game's first: 10 of the 30 games are dealt an up01 / up02 / up03 card.
        assert out["fault"].all() and (out["fault"] == RM.FAULT_INT_CARD).sum() == 29
        assert out["obs_raises"].sum() == 10 and (out["step"][out["obs_raises"] != 0] == 0).all()
        assert not out["obs"][out["obs_raises"] != 0].any()
    else:
        assert not out["obs_raises"].any()
    if name == "trace_vs_expert":
        ok = g["fault"] == 0
        assert np.array_equal(out["final"][ok], g["final"][ok]) and np.array_equal(out["fault"] != 0, g["fault"] != 0)
    if name == "trace_random_S12":
        assert total == 2195 and len(steps) == 48
    if name == "trace_live_expert":
        assert total == 600 and len(steps) == 12


def test_the_fixtures_leave_more_than_95_percent_of_their_rows_checked():
    checked = rows = 0
    for name in FIXTURES:
        c, r = checked_of(name)
        checked, rows = checked + c, rows + r
    assert checked > 0.95 * rows, (checked, rows)


def test_model_stops():
    """The stop rules on trace_live_expert's log: another legal action where the bot plays, an illegal action in a bot-free
    log, an entry behind the end of a game that was won.  At entry 5 of game 3 the fixture's only legal action is the
    logged PASS, so the bot's entry that is replaced is the first one from 5 on with a second legal action: entry 6."""
    g, m, pairs, action, steps = fixture_call("trace_live_expert")
    assert RM.legal_bytes(g["legal"][g["offsets"][3] + 5]).sum() == 1
    k, other = RM.other_legal_entry(g, action, 3, 5)
    bad = action.copy()
    bad[3, k] = other
    out = RM.replay(m, pairs, bad, steps)
    base, _ = game_log.row_bases(steps)
    assert k == 6 and out["status"][3] == RM.BOT_DIFFERS and out["replayed"][3] == k and not np.delete(out["status"], 3).any()
    assert (out["action"][base[3] + k + 1:base[3] + steps[3]] == 255).all() and out["action"][base[3] + k] == other
    g, m, pairs, action, steps = fixture_call("trace_random_S12")
    off = g["offsets"]
    legal = RM.legal_bytes(g["legal"][off[2] + 4])
    bad = action.copy()
    bad[2, 4] = next(a for a in range(155) if not legal[a])
    out = RM.replay(m, pairs, bad, steps)
    assert out["status"][2] == RM.ILLEGAL and out["replayed"][2] == 4 and out["action"][game_log.row_bases(steps)[0][2] + 4] == 255
    won = next(i for i in range(len(steps)) if g["done"][off[i + 1] - 1] and not g["fault"][i])
    longer, more = np.concatenate([action, np.full((len(steps), 1), 255, np.uint8)], axis=1), steps.copy()
    longer[won, steps[won]] = 155
    more[won] += 1
    out = RM.replay(m, pairs, longer, more)
    assert out["status"][won] == RM.ENDED_EARLY and out["replayed"][won] == steps[won] and not np.delete(out["status"], won).any()


def test_row_bases_and_keep():
    steps = np.array([3, 0, 5, 2], dtype=np.int32)
    base, total = game_log.row_bases(steps)
    assert base.tolist() == [0, 3, 3, 8] and total == 10 and base.dtype == np.int64
    keep = np.zeros((4, 6), dtype=np.uint8)
    keep[:, ::2] = 1          # entries 0, 2, 4
    keep[3, 5] = 7            # behind game 3's last entry: not a row
    assert game_log.kept_counts(steps, keep).tolist() == [2, 0, 3, 1]
    base, total = game_log.row_bases(steps, keep)
    assert base.tolist() == [0, 2, 2, 5] and total == 6
    assert game_log.row_bases(np.zeros(0, dtype=np.int32)) [1] == 0
    with pytest.raises(ValueError):
        game_log.kept_counts(steps, keep[:, :4])   # shorter than the longest game
    with pytest.raises(ValueError):
        game_log.kept_counts(steps, keep[:3])
    # the model counts rows by the same rule
    m = np.zeros(2, dtype=MATCH_DTYPE)
    g, fm, pairs, action, fsteps = fixture_call("trace_pool_up")
    k = (np.arange(action.shape[1])[None, :] % 2 == 0).repeat(len(fsteps), axis=0)
    out = RM.replay(fm, pairs, action, fsteps, keep=k)
    full = model_of("trace_pool_up")[2]
    sel = full["step"] % 2 == 0
    assert len(m) == 2 and len(out["action"]) == int(sel.sum())
    for c in RM.COLS:
        assert np.array_equal(out[c], full[c][sel]), c


def test_batch_cuts():
    counts = [3, 0, 5, 2, 5, 1]
    assert game_log.batch_cuts(counts, 5) == [(0, 2), (2, 3), (3, 4), (4, 5), (5, 6)]
    assert game_log.batch_cuts(counts, 8) == [(0, 3), (3, 6)]
    assert game_log.batch_cuts(counts, 100) == [(0, 6)]
    assert game_log.batch_cuts([], 5) == []
    assert game_log.batch_cuts([0, 0], 5) == [(0, 2)]
    for cuts in (game_log.batch_cuts(counts, 5), game_log.batch_cuts(counts, 8)):   # whole consecutive games, all of them, within max_rows
        assert [a for a, _ in cuts] == [0] + [b for _, b in cuts[:-1]] and cuts[-1][1] == len(counts)
    with pytest.raises(ValueError, match="game 2 alone has 5 rows"):
        game_log.batch_cuts(counts, 4)


def test_outcome():
    results = np.array([0, 1, -1], dtype=np.int8)          # FIRST won, SECOND won, a draw
    game = np.array([0, 0, 1, 1, 2, 2])
    to_play = np.array([0, 1, 0, 1, 0, 1], dtype=np.uint8)
    assert game_log.outcome(results, game, to_play).astype(np.int8).tolist() == [1, -1, -1, 1, 0, 0]
    import torch
    t = game_log.outcome(torch.as_tensor(results), torch.as_tensor(game), torch.as_tensor(to_play)).to(torch.int8)
    assert t.tolist() == [1, -1, -1, 1, 0, 0]


def test_header_and_binding_agree():
    src = open(os.path.join(REPO, "include", "monsoon.h")).read()
    codes = dict(re.findall(r"#define MONSOON_REPLAY_(\w+)\s+(\d+)", src))
    assert {k: int(v) for k, v in codes.items()} == {"OK": _lib.REPLAY_OK, "ILLEGAL": _lib.REPLAY_ILLEGAL, "BOT_DIFFERS": _lib.REPLAY_BOT_DIFFERS,
                                                     "BOT_RAISED": _lib.REPLAY_BOT_RAISED, "ENDED_EARLY": _lib.REPLAY_ENDED_EARLY}
    assert (RM.OK, RM.ILLEGAL, RM.BOT_DIFFERS, RM.BOT_RAISED, RM.ENDED_EARLY) == tuple(range(5))
    body = re.search(r"typedef struct \{[^}]*\} monsoon_replay_rows;", src).group(0)
    fields = re.findall(r"\*\s+(\w+);", body)
    assert tuple(fields) == tuple(n for n, _ in _lib.ReplayRows._fields_) == RM.COLS == tuple(game_log.COLUMNS)
    assert "monsoon_replay_logged_dev" in _lib.SIGNATURES and len(_lib.SIGNATURES["monsoon_replay_logged_dev"][1]) == 15
    assert sum(game_log.ROW_BYTES.values()) == 2160 + 156 + 4 + 8 + 8
