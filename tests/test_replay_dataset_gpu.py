"""monsoon_replay_logged_dev / game_log.dataset on the device: the reference's fixtures replayed straight into rows, every
record build, a logged mixed schedule end to end against the model (tests/replay_model.py, pinned to the reference by
tests/test_replay_dataset_cpu.py), the existing generator game_log.replay, the stop rules, the refusals, and a
256-game batch.  No reference tree involved."""
import ctypes
import os

import numpy as np
import pytest

import replay_model as RM
from monsoon_amd import _lib, game_log
from monsoon_amd.cards import deck_indices
from monsoon_amd.engine import MATCH_DTYPE, BatchEngine, RolloutLog, _ptr
from test_replay_dataset_cpu import FIXTURES, fixture_call, model_of
from test_rollout_log_gpu import W2, _drain, _fixture_pairs, _n12m, _schedule

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _engine(max_games=64, build=0):
    """A handle for dataset: torch loads its runtime before the library does (VecEnv.__init__ says why)."""
    import torch
    assert torch.cuda.is_available()
    return BatchEngine(max_games, extended=build)


def _log(action, steps):
    return RolloutLog(np.ascontiguousarray(action), None, None, np.ascontiguousarray(steps, dtype=np.int32))


def _host(d, cols=RM.COLS):
    out = {c: d[c].cpu().numpy() for c in cols if c in d}
    if "state_hash" in out:
        out["state_hash"] = out["state_hash"].view(np.uint64)
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_fixtures_on_the_device(name):
    """The reference's traces as logs: legal masks, observations (by their fnv1a64) and state hashes of every row are the
    fixture's, the first two fixtures' every column is the model's, and the games are left in the fixture's last states."""
    g, m, pairs, action, steps = fixture_call(name)
    eng = _engine()
    d = game_log.dataset(eng, m, pairs, _log(action, steps))
    hashes = eng.state_hash()
    eng.close()
    assert not d["status"].any() and np.array_equal(d["replayed"], steps) and len(d["action"]) == steps.sum()
    rows = _host(d)
    base, _ = game_log.row_bases(steps)
    checked, total = RM.check_fixture(g, rows, base, steps, bot_fixture=name == "trace_live_expert")
    assert checked > 0.95 * total
    if name in FIXTURES[:2]:
        assert RM.same_rows(d, model_of(name)[2]) is None
    ok = (g["fault"] == 0) & (steps > 0)
    last = g["final"] if "final" in g.files else g["hash"][np.maximum(g["offsets"][1:] - 1, 0)]
    assert ok.any() or name == "trace_pool_up"
    assert np.array_equal(hashes[ok], last[ok]) and np.array_equal(d["fault"] != 0, g["fault"] != 0)
    if name == "trace_pool_up":   # (what tests/test_replay_dataset_cpu.py finds on the model)
        assert rows["obs_raises"].sum() == 10 and not rows["obs"][rows["obs_raises"] != 0].any()


@pytest.mark.parametrize("fixture,build", [("trace_heuristic_S12", 0), ("trace_heuristic_pool_ext", 1), ("trace_heuristic_c5_big", 2)])
def test_every_record_build(fixture, build):
    """The heuristic traces' actions as the log, on the build their decks need: the legal count of every row and the state
    of every row after the first are the reference's."""
    g = np.load(os.path.join(GOLD, fixture + ".npz"))
    n = len(g["seeds"])
    pairs = _fixture_pairs(g)
    m = np.zeros(n, dtype=MATCH_DTYPE)
    m["seed"] = g["seeds"]
    if len(pairs) > 1:
        m["deck"] = np.arange(n)
    action, steps = RM.fixture_log(g)
    eng = _engine(64, build)
    d = game_log.dataset(eng, m, pairs, _log(action, steps), columns=("legal", "state_hash", "game", "step"))
    eng.close()
    assert not d["status"].any() and np.array_equal(d["replayed"], steps) and set(d) >= {"legal", "state_hash", "game", "step", "action"}
    assert "obs" not in d
    rows = _host(d)
    assert np.array_equal(rows["action"], g["action"]) and np.array_equal(rows["legal"].sum(axis=1), g["nlegal"])
    later = rows["step"] > 0
    want = np.concatenate([np.zeros(1, np.uint64), g["hash"][:-1]])   # row j's state is the one after entry j - 1 of the same game
    on = later & (want != 0)
    assert on.sum() > 0.95 * len(on) and np.array_equal(rows["state_hash"][on], want[on])
    assert np.array_equal(rows["game"], np.repeat(np.arange(n), steps))


@pytest.fixture(scope="module")
def mixed():
    """96 matches, a third each bot-FIRST, bot-SECOND and plain, S12 and N12M alternating, logged on the device; the
    model's replay of that log."""
    n, T = 96, 200
    m = _schedule(n, seed0=1)
    m["deck"] = (np.arange(n) // 3) % 2
    pairs = np.stack([np.stack([deck_indices(d)] * 2) for d in ("S12", "N12M")])
    eng = _engine(64)
    _, results, steps, log = eng.rollout_logged(W2, m, pairs, T)
    d = game_log.dataset(eng, m, pairs, log, results=results)
    sides = game_log.step_sides(eng, m, pairs, log)
    eng.close()
    return dict(m=m, pairs=pairs, log=log, results=results, steps=steps, d=d, host=_host(d), sides=sides,
                model=RM.replay(m, pairs, log.action, steps))


def test_end_to_end_equals_the_model(mixed):
    d, model, steps = mixed["d"], mixed["model"], mixed["steps"]
    assert RM.same_rows(d, model) is None and model["reached"].all() and not d["status"].any()
    assert model["bot"].any() and not model["bot"].all() and len(model["action"]) == steps.sum()
    want = game_log.outcome(mixed["results"], model["game"], model["to_play"]).astype(np.int8)
    assert np.array_equal(d["outcome"].cpu().numpy(), want) and {-1, 1} <= set(np.unique(want).tolist())
    to_play, bot = mixed["sides"]
    assert to_play.shape == bot.shape == mixed["log"].action.shape
    assert np.array_equal(to_play[model["game"], model["step"]], model["to_play"]) and np.array_equal(bot[model["game"], model["step"]], model["bot"] != 0)
    assert (to_play == -1).sum() == to_play.size - steps.sum() and bot.sum() == model["bot"].sum()


def test_keep_batches_and_a_smaller_handle(mixed):
    m, pairs, log, model, host = mixed["m"], mixed["pairs"], mixed["log"], mixed["model"], mixed["host"]
    # every third entry, minus the bot's steps
    keep = (np.arange(log.action.shape[1])[None, :] % 3 == 0) & ~mixed["sides"][1]
    sel = (model["step"] % 3 == 0) & (model["bot"] == 0)
    eng = _engine(32)   # three batches
    d = game_log.dataset(eng, m, pairs, log, keep=keep)
    kept = _host(d)
    assert len(kept["action"]) == sel.sum() > 0 and np.array_equal(d["replayed"], mixed["steps"]) and not d["status"].any()
    for c in RM.COLS:
        assert np.array_equal(kept[c], model[c][sel]), c
    full = _host(game_log.dataset(eng, m, pairs, log))
    for c in RM.COLS:
        assert np.array_equal(full[c], host[c]), c
    ok = model["fault"][64:] == 0   # (behind a faulting step the oracle and the device hold different leftovers)
    assert eng.n == 32 and ok.sum() > 16 and np.array_equal(eng.state_hash()[ok], model["final"][64:][ok])
    # runs of whole games within 500 rows, one set of tensors
    parts, games, ptr = {c: [] for c in RM.COLS + ("outcome",)}, [], set()
    for item in game_log.dataset_batches(eng, m, pairs, log, 500, results=mixed["results"]):
        assert 0 < len(item["action"]) <= 500 and len(item["status"]) == item["games"][1] - item["games"][0]
        games.append(item["games"])
        ptr.add(item["obs"].data_ptr())
        for c in parts:
            parts[c].append(item[c].cpu().numpy())
    eng.close()
    assert len(games) > 5 and len(ptr) == 1 and games[0][0] == 0 and games[-1][1] == len(m)
    assert [a for a, _ in games[1:]] == [b for _, b in games[:-1]]
    for c in RM.COLS:
        got = np.concatenate(parts[c])
        assert np.array_equal(got.view(np.uint64) if c == "state_hash" else got, host[c]), c
    assert np.array_equal(np.concatenate(parts["outcome"]), mixed["d"]["outcome"].cpu().numpy())
    with pytest.raises(ValueError):
        next(game_log.dataset_batches(None, m, pairs, log, int(mixed["steps"].max()) - 1))


def test_against_the_step_interface():
    """64 bot-free S12 games: every item of game_log.replay -- to_play, legal mask, observation and action of the live
    games, step index by step index -- is the rows', and its final hashes are the states dataset leaves."""
    n = 64
    d12 = deck_indices("S12")
    pairs = np.stack([d12, d12])[None]
    m = _schedule(n, seed0=6, bot=False)
    eng, second = _engine(64), BatchEngine(64)
    _, _, steps, log = eng.rollout_logged(W2, m, pairs, 200)
    d = game_log.dataset(eng, m, pairs, log)
    hashes = eng.state_hash()
    items, finals = _drain(game_log.replay(second, m, pairs, log))
    eng.close()
    second.close()
    rows = _host(d)
    base, total = game_log.row_bases(steps)
    assert total == len(rows["action"]) and not d["status"].any() and len(items) == steps.max()
    for k, (live, to_play, mask, obs, action) in enumerate(items):
        r = base[live] + k
        assert np.array_equal(rows["step"][r], np.full(live.sum(), k)) and np.array_equal(rows["game"][r], np.nonzero(live)[0])
        assert np.array_equal(rows["to_play"][r], to_play[live]) and np.array_equal(rows["action"][r], action[live])
        assert np.array_equal(rows["obs"][r], obs[live])
        assert np.array_equal(rows["legal"][r], np.stack([RM.legal_bytes(x) for x in mask[live]]))
    ok = d["fault"] == 0
    assert ok.sum() >= 0.9 * n and np.array_equal(finals[ok], hashes[ok])


def test_stops():
    """BOT_DIFFERS, ILLEGAL and ENDED_EARLY, each in one game of a call whose other games are untouched.  At entry 5 of
    game 3 of trace_live_expert the only legal action is the logged PASS, so the replaced entry of the bot is the first one
    from 5 on that has a second legal action (entry 6, tests/test_replay_dataset_cpu.py)."""
    eng = _engine()
    g, m, pairs, action, steps = fixture_call("trace_live_expert")
    base, _ = game_log.row_bases(steps)
    clean = _host(game_log.dataset(eng, m, pairs, _log(action, steps)))
    k, other = RM.other_legal_entry(g, action, 3, 5)
    bad = action.copy()
    bad[3, k] = other
    d = game_log.dataset(eng, m, pairs, _log(bad, steps))
    rows = _host(d)
    assert d["status"][3] == _lib.REPLAY_BOT_DIFFERS and d["replayed"][3] == k and not np.delete(d["status"], 3).any()
    mine = slice(base[3], base[3] + steps[3])
    assert (rows["action"][mine][k + 1:] == 255).all() and rows["action"][mine][k] == other
    assert np.array_equal(np.delete(d["replayed"], 3), np.delete(steps, 3))
    for c in RM.COLS:   # the game's rows before the stop and every other game's rows
        same = np.ones(len(rows["action"]), bool)
        same[base[3] + k:base[3] + steps[3]] = False
        assert np.array_equal(rows[c][same], clean[c][same]), c
    assert RM.same_rows(d, RM.replay(m, pairs, bad, steps)) is None

    g, m, pairs, action, steps = fixture_call("trace_random_S12")
    base, _ = game_log.row_bases(steps)
    off = g["offsets"]
    legal = RM.legal_bytes(g["legal"][off[2] + 4])
    bad = action.copy()
    bad[2, 4] = next(a for a in range(155) if not legal[a])
    d = game_log.dataset(eng, m, pairs, _log(bad, steps), columns=("step",))
    assert d["status"][2] == _lib.REPLAY_ILLEGAL and d["replayed"][2] == 4 and not np.delete(d["status"], 2).any()
    assert (d["action"].cpu().numpy()[base[2] + 4:base[2] + steps[2]] == 255).all() and (d["action"].cpu().numpy()[:base[2] + 4] != 255).all()
    bad[2, 4] = 200   # not an action at all
    d = game_log.dataset(eng, m, pairs, _log(bad, steps), columns=())
    assert d["status"][2] == _lib.REPLAY_ILLEGAL and d["replayed"][2] == 4

    won = next(i for i in range(len(steps)) if g["done"][off[i + 1] - 1] and not g["fault"][i])
    longer, more = np.concatenate([action, np.full((len(steps), 1), 255, np.uint8)], axis=1), steps.copy()
    longer[won, steps[won]] = 155   # a PASS behind the end of a game that was won
    more[won] += 1
    d = game_log.dataset(eng, m, pairs, _log(longer, more), columns=("step",))
    eng.close()
    assert d["status"][won] == _lib.REPLAY_ENDED_EARLY and d["replayed"][won] == steps[won] and not np.delete(d["status"], won).any()
    a = d["action"].cpu().numpy()
    assert a[game_log.row_bases(more)[0][won] + steps[won]] == 255 and (a == 255).sum() == 1


def test_refusals():
    """S one more than rows_cap, a NULL rows, a NULL rows->action, log_steps > log_stride: MONSOON_ERR_ARG, the outputs
    untouched, and the handle plays on as a fresh one does."""
    import torch
    eng = _engine()
    g, m, pairs, action, steps = fixture_call("trace_pool_up")
    m, pairs, action = np.ascontiguousarray(m), np.ascontiguousarray(pairs), np.ascontiguousarray(action)
    total = int(steps.sum())
    act = torch.full((total,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    good = _lib.ReplayRows(action=act.data_ptr())
    too_long = steps.copy()
    too_long[1] = action.shape[1] + 1
    cases = [(ctypes.byref(good), total - 1, steps), (None, total, steps), (ctypes.byref(_lib.ReplayRows()), total, steps),
             (ctypes.byref(good), total + 1, too_long)]
    for rows, cap, st in cases:
        status, replayed, fault = np.full(len(m), 9, np.uint8), np.full(len(m), -9, np.int32), np.full(len(m), 9, np.uint8)
        n_rows = ctypes.c_int64(-9)
        rc = eng.lib.monsoon_replay_logged_dev(eng.h, _ptr(m), len(m), _ptr(pairs), len(pairs), _ptr(action), action.shape[1], _ptr(st), None,
                                               rows, cap, ctypes.byref(n_rows), _ptr(status), _ptr(replayed), _ptr(fault))
        assert rc == _lib.ERR_ARG and n_rows.value == -9
        assert (status == 9).all() and (replayed == -9).all() and (fault == 9).all() and (act == 7).all()
    free = _schedule(12, seed0=2, bot=False)
    fresh = BatchEngine(64)
    for x, y in zip(eng.rollout(W2, free, _n12m(), 50, want_results=True), fresh.rollout(W2, free, _n12m(), 50, want_results=True)):
        assert np.array_equal(x, y)
    # ... and so it does after a replay that ran
    n_rows, status, _, _ = eng.replay_logged(m, pairs, action, steps, good, total)
    assert n_rows == total and not status.any() and (act != 7).any() and (act != 255).all()
    for x, y in zip(eng.rollout(W2, free, _n12m(), 50, want_results=True), fresh.rollout(W2, free, _n12m(), 50, want_results=True)):
        assert np.array_equal(x, y)
    fresh.close()
    eng.close()


def test_a_full_handle():
    """256 N12M games on a 256-game handle (the persistent grid's pop counters at work), all columns."""
    n = 256
    m = _schedule(n, seed0=8)
    eng = _engine(256)
    _, results, steps, log = eng.rollout_logged(W2, m, _n12m(), 200)
    d = game_log.dataset(eng, m, _n12m(), log, results=results)
    hashes_after = eng.state_hash()
    eng.close()
    assert len(d["action"]) == log.steps.sum() == steps.sum() and d["obs"].shape == (steps.sum(), 27, 5, 4)
    a, game = d["action"].cpu().numpy(), d["game"].cpu().numpy()
    assert not (a[d["status"][game] == 0] == 255).any() and (d["status"] == 0).all()
    assert np.array_equal(game, np.repeat(np.arange(n), steps)) and np.array_equal(a, log.action[log.action != 255])
    assert len(hashes_after) == n and np.array_equal(d["replayed"], steps)


def test_more_games_than_resident_wavefronts():
    """8 192 games on one handle: more than the GPU holds wavefronts, so the games are popped from the range counters.  Every
    game is replayed to its last entry, the rows are in match and entry order, and every game without a fault is left in
    the state the rollout that wrote the log left it in."""
    n, T = 8192, 40
    m = _schedule(n, seed0=9)
    eng = _engine(n)
    _, _, steps, log = eng.rollout_logged(W2, m, _n12m(), T)
    played, faults = eng.state_hash(), eng.rollout_faults(n)
    for _ in range(2):   # (two launches in a row: the counter sets alternate)
        d = game_log.dataset(eng, m, _n12m(), log, columns=("game", "step", "to_play"))
        assert not d["status"].any() and np.array_equal(d["replayed"], steps) and len(d["action"]) == steps.sum()
        assert np.array_equal(d["game"].cpu().numpy(), np.repeat(np.arange(n), steps))
        assert np.array_equal(d["step"].cpu().numpy(), np.concatenate([np.arange(s) for s in steps]))
        assert np.array_equal(d["action"].cpu().numpy(), log.action[log.action != 255])
        ok = (faults == 0) & (d["fault"] == 0)
        assert ok.sum() > 0.9 * n and np.array_equal(eng.state_hash()[ok], played[ok])
    eng.close()
