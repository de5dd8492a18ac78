"""monsoon_replay_logged_after_dev / game_log's candidate columns on the device: the reference's heuristic traces replayed
into rows whose candidates give the reference's decisions back, on every record build; a logged mixed schedule against
the model (tests/replay_after_model.py, pinned to the reference by tests/test_replay_after_cpu.py) and against its own
log; the look-ahead leaving no trace in the replay; K; stops and refusals; dataset_batches.  No reference tree involved."""
import ctypes
import functools
import os

import numpy as np
import pytest

import heuristic_model as HM
import oracle_lib
import replay_after_model as AM
import replay_model as RM
from monsoon_amd import _lib, game_log
from monsoon_amd.cards import deck_indices
from monsoon_amd.engine import _ptr
from test_replay_after_cpu import fixture_schedule
from test_replay_dataset_cpu import fixture_call
from test_replay_dataset_gpu import _engine, _host, _log
from test_rollout_log_gpu import W2, _schedule

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALL = tuple(game_log.CANDIDATE_COLUMNS)
NO_OBS = tuple(c for c in ALL if c != "after_obs")
SCORE = HM.ScoreCache()


def _decisions(c, raises, weights_of_row, rows):
    """The heuristic decision of each of `rows` rebuilt from the device's candidate columns c (AM.host): (action, score,
    n_legal) arrays, and which rows hold a candidate that hit a limit of the record (status >= 16 other than 18)."""
    action, score = np.zeros(len(rows), np.uint8), np.zeros(len(rows))
    limited = np.zeros(len(rows), bool)
    for i, r in enumerate(rows):
        n = int(c["n_legal"][r])
        status = c["status"][r, :n]
        limited[i] = bool(((status >= 16) & (status != 18)).any())
        best, score[i], _ = AM.decision(weights_of_row(r), None if raises[r] else c["before_features"][r], status, c["features"][r], SCORE)
        action[i] = c["action"][r, best]
    return action, score, c["n_legal"][rows], limited


@functools.lru_cache(maxsize=None)
def _fixture_run(fixture, build, k):
    """A heuristic trace replayed with its candidates' features, K = k: (fixture, host columns, candidate columns)."""
    g = np.load(os.path.join(GOLD, fixture + ".npz"))
    m, pairs, action, steps = fixture_schedule(g)
    eng = _engine(64, build)
    d = game_log.dataset(eng, m, pairs, _log(action, steps), columns=("obs_raises",) + NO_OBS, max_after=k)
    eng.close()
    assert not d["status"].any() and np.array_equal(d["replayed"], steps) and len(d["action"]) == steps.sum()
    return g, _host(d, ("action", "obs_raises")), AM.host(d)


@pytest.mark.parametrize("fixture,build", [("trace_heuristic_S12", 0), ("trace_heuristic_pool_ext", 1), ("trace_heuristic_c5_big", 2)])
def test_candidates_give_the_reference_decisions(fixture, build):
    """Every row of the trace: the first maximum of the independent score over the device's afterstate features is the
    reference's action with the reference's best score, bit for bit, over the reference's number of legal actions, and
    chosen points at it.  A row with a candidate that hit a limit of the record is set aside (none on the standard one)."""
    g, rows, c = _fixture_run(fixture, build, 156)
    total = len(g["action"])
    assert np.array_equal(rows["action"], g["action"]) and np.array_equal(c["n_legal"], g["nlegal"])
    assert (c["chosen"] >= 0).all() and np.array_equal(c["action"][np.arange(total), c["chosen"]], g["action"])
    assert np.array_equal(c["action"] != 255, np.arange(156)[None, :] < c["n_legal"][:, None])
    action, score, n_legal, limited = _decisions(c, rows["obs_raises"], lambda r: g["w0"], np.arange(total))
    on = ~limited
    checked = int(on.sum())
    assert checked > 0.95 * total and (build or checked == total)
    assert np.array_equal(action[on], g["action"][on]) and np.array_equal(n_legal, g["nlegal"])
    assert np.array_equal(score[on].view(np.uint64), g["best"][on].view(np.uint64))


@pytest.mark.parametrize("k", [1, 8, 9])
def test_max_after_cuts_the_legal_list(k):
    """K = 1, one pass (8) and one candidate into the second pass (9) on the S12 trace (n_legal up to 68): the entries below
    min(n_legal, K) are the K = 156 run's, after_action reads 255 beyond, n_legal and chosen do not depend on K."""
    _, rows, full = _fixture_run("trace_heuristic_S12", 0, 156)
    _, rows_k, cut = _fixture_run("trace_heuristic_S12", 0, k)
    assert np.array_equal(rows_k["action"], rows["action"]) and np.array_equal(rows_k["obs_raises"], rows["obs_raises"])
    assert cut["action"].shape == (len(rows["action"]), k) and (full["n_legal"] > k).any() and (full["chosen"] >= k).any()
    shown = np.arange(k)[None, :] < full["n_legal"][:, None]
    assert (cut["action"][~shown] == 255).all() and (cut["action"][shown] != 255).all()
    head = {c: (v[:, :k] if v.ndim > 1 and c != "before_features" else v) for c, v in full.items()}
    assert AM.same_candidates(cut, head) is None


def _mixed_schedule(n, seed0):
    """n matches as test_replay_dataset_gpu's `mixed`: a third each bot-FIRST, bot-SECOND and plain over the two rows of W2,
    S12 and N12M alternating."""
    m = _schedule(n, seed0=seed0)
    m["deck"] = (np.arange(n) // 3) % 2
    return m, np.stack([np.stack([deck_indices(d)] * 2) for d in ("S12", "N12M")])


def test_against_the_model():
    """12 mixed matches logged on the device and replayed with every candidate column, K = 156: every specified entry of
    every row of four of the games -- bot FIRST, bot SECOND and plain on S12, bot FIRST on N12M, the bot's rows included --
    is the model's, floats by bit pattern.  Then every game of trace_pool_up, whose rows hold what those games do not: an
    observation that raises (before_features reads zeros, every candidate has status 2) and look-ahead steps that raise."""
    m, pairs = _mixed_schedule(12, 3)
    eng = _engine(16)
    _, _, steps, log = eng.rollout_logged(W2, m, pairs, 200)
    d = game_log.dataset(eng, m, pairs, log, columns=("bot", "to_play") + ALL, max_after=156)
    eng.close()
    assert not d["status"].any() and np.array_equal(d["replayed"], steps)
    c, rows = AM.host(d), _host(d, ("action", "bot", "to_play"))
    base, _ = game_log.row_bases(steps)
    games = range(4)
    seen = entries = bots = 0
    for r, g, k, want, _ in AM.rows(m, pairs, log.action, steps, 156, games):
        assert rows["action"][r] == want["action"] and rows["bot"][r] == want["bot"] and rows["to_play"][r] == want["to_play"], (g, k)
        entries += AM.compare_row(want, c, r, 156, (g, k))
        seen += 1
        bots += want["bot"]
    assert seen == steps[:4].sum() == base[4] and 0 < bots < seen and entries > 10 * seen

    g, m, pairs, action, steps = fixture_call("trace_pool_up")
    eng = _engine()
    d = game_log.dataset(eng, m, pairs, _log(action, steps), columns=("obs_raises",) + ALL, max_after=156)
    eng.close()
    c, raises = AM.host(d), d["obs_raises"].cpu().numpy()
    seen = raised = 0
    for r, g, k, want, _ in AM.rows(m, pairs, action, steps, 156, range(len(m))):
        assert (want["before"] is None) == bool(raises[r]), (g, k)
        AM.compare_row(want, c, r, 156, (g, k))
        seen += 1
        raised += sum(e["status"] != 0 for e in want["entries"])
    assert seen == steps.sum() and raises.sum() == 10 and raised > 100


@pytest.fixture(scope="module")
def runs():
    """48 mixed matches over the two rows of W2 logged on a handle of 16 games (three batches), max_turns 200, then replayed
    three times: without candidate columns, with them (K = 156, no observations), and with them under a keep mask of every
    third entry.  The handle's hashes after each."""
    n = 48
    m, pairs = _mixed_schedule(n, 4)   # (seeds whose game 41 draws 741 words in its 200 steps)
    eng = _engine(16)
    _, results, steps, log = eng.rollout_logged(W2, m, pairs, 200)
    keep = np.arange(log.action.shape[1])[None, :] % 3 == 0
    keep = np.broadcast_to(keep, log.action.shape).copy()
    plain = tuple(game_log.COLUMNS)
    out = dict(m=m, pairs=pairs, log=log, steps=steps, keep=keep)
    for name, cols, kp in (("plain", plain, None), ("after", plain + NO_OBS, None), ("kept", plain + NO_OBS, keep)):
        d = game_log.dataset(eng, m, pairs, log, keep=kp, columns=cols, max_after=156)
        out[name] = dict(d=d, rows=_host(d), c=AM.host(d) if name != "plain" else None, hashes=eng.state_hash(),
                         host={x: d[x] for x in ("status", "replayed", "fault")})
    # ... and in runs of whole games, one set of tensors
    total = int(steps.sum())
    max_rows = next(mr for mr in range(total // 3, total) if len(game_log.batch_cuts(steps, mr)) == 3)
    parts = []
    for item in game_log.dataset_batches(eng, m, pairs, log, max_rows, columns=("game", "step") + NO_OBS, max_after=156):
        parts.append((item["games"], _host(item, ("action", "game", "step")), AM.host(item)))
    eng.close()
    out["parts"] = parts
    return out


def test_against_the_log(runs):
    """Every row that is not the bot's: the decision rebuilt from the row's candidates and the weight row of the side to
    play is the logged action, with the logged score bit for bit, over the logged number of legal actions."""
    m, log, rows, c = runs["m"], runs["log"], runs["after"]["rows"], runs["after"]["c"]
    assert not runs["after"]["d"]["status"].any()
    mine = np.nonzero(rows["bot"] == 0)[0]
    assert 0 < len(mine) < len(rows["bot"])
    side_row = np.where(rows["to_play"] == 0, m["p1"][rows["game"]], m["p2"][rows["game"]])
    assert (side_row[mine] >= 0).all() and set(side_row[mine].tolist()) == {0, 1}
    action, score, n_legal, limited = _decisions(c, rows["obs_raises"], lambda r: W2[side_row[r]], mine)
    g, k = rows["game"][mine], rows["step"][mine]
    assert not limited.any()
    assert np.array_equal(action, log.action[g, k]) and np.array_equal(n_legal, log.n_legal[g, k])
    assert np.array_equal(score.view(np.uint64), log.score[g, k].view(np.uint64))
    assert np.array_equal(c["action"][mine, c["chosen"][mine]], log.action[g, k])


def test_the_lookahead_leaves_no_trace(runs):
    """The replay with candidate columns is the replay without: every plain column (state_hash included), status, replayed,
    fault and the states the handle is left in -- also under a keep mask, on the rows it keeps.  The schedule commits
    REPLACE actions (148..151), which draw, and holds a game whose stream runs into its third block."""
    m, pairs, log, steps = runs["m"], runs["pairs"], runs["log"], runs["steps"]
    a = log.action[np.arange(log.action.shape[1])[None, :] < steps[:, None]]
    assert ((a >= 148) & (a <= 151)).any()
    orc = oracle_lib.Oracle(1)
    used = [AM.stream_words(orc, m[g], pairs[int(m["deck"][g])], log.action[g], steps[g]) for g in range(len(m))]
    assert max(used) >= 624 + 64, max(used)   # a block holds 624 words: a refill, and rows behind it
    plain, after, kept = runs["plain"], runs["after"], runs["kept"]
    for run in (after, kept):
        for x in ("status", "replayed", "fault"):
            assert np.array_equal(run["host"][x], plain["host"][x]), x
        assert np.array_equal(run["hashes"], plain["hashes"])
    sel = plain["rows"]["step"] % 3 == 0
    assert len(kept["rows"]["action"]) == sel.sum() and len(after["rows"]["action"]) == steps.sum()
    for col in RM.COLS:
        assert np.array_equal(after["rows"][col], plain["rows"][col]), col
        assert np.array_equal(kept["rows"][col], plain["rows"][col][sel]), col
    assert AM.same_candidates(kept["c"], after["c"], rows_b=sel) is None


def test_dataset_batches_with_candidates(runs):
    parts, one, rows = runs["parts"], runs["after"]["c"], runs["after"]["rows"]
    assert len(parts) == 3 and parts[0][0][0] == 0 and parts[-1][0][1] == len(runs["m"])
    at = 0
    for (g0, g1), plain, c in parts:
        n = len(plain["action"])
        assert n == runs["steps"][g0:g1].sum() and np.array_equal(plain["game"], rows["game"][at:at + n])
        assert np.array_equal(plain["action"], rows["action"][at:at + n]) and np.array_equal(plain["step"], rows["step"][at:at + n])
        assert AM.same_candidates(c, one, rows_b=slice(at, at + n)) is None
        at += n
    assert at == len(rows["action"])


def test_a_stop_and_the_refusals():
    """A log whose entry 6 of game 3 names another legal action than the bot's stops there as it does without candidates:
    the game's rows behind that entry read action 255, every row before it and every other game's rows carry the clean
    run's candidates.  The refusals: MONSOON_ERR_ARG, nothing written, the loaded games untouched."""
    import torch
    eng = _engine()
    g, m, pairs, action, steps = fixture_call("trace_live_expert")
    base, total = game_log.row_bases(steps)
    cols = ("after_features", "before_features", "chosen")
    clean = game_log.dataset(eng, m, pairs, _log(action, steps), columns=cols, max_after=64)
    k, other = RM.other_legal_entry(g, action, 3, 5)
    bad = action.copy()
    bad[3, k] = other
    d = game_log.dataset(eng, m, pairs, _log(bad, steps), columns=cols, max_after=64)
    assert d["status"][3] == _lib.REPLAY_BOT_DIFFERS and d["replayed"][3] == k and not np.delete(d["status"], 3).any()
    a = d["action"].cpu().numpy()
    mine = slice(base[3], base[3] + steps[3])
    assert (a[mine][k + 1:] == 255).all() and a[mine][k] == other and (np.delete(a, np.arange(mine.start, mine.stop)) != 255).all()
    same = np.ones(total, bool)
    same[base[3] + k:base[3] + steps[3]] = False
    assert AM.same_candidates(AM.host(d), AM.host(clean), rows_a=same, rows_b=same) is None
    # the stopping row itself was written before the bot played: its candidates are those of the same state
    c, c0 = AM.host(d), AM.host(clean)
    assert c["n_legal"][base[3] + k] == c0["n_legal"][base[3] + k] and c["chosen"][base[3] + k] != c0["chosen"][base[3] + k]

    m, pairs, action = np.ascontiguousarray(m), np.ascontiguousarray(pairs), np.ascontiguousarray(action)
    hashes = eng.state_hash()
    K = 8
    act = torch.full((total,), 7, dtype=torch.uint8, device="cuda")
    buf = {c: torch.zeros((total + 1,) + tuple(K if x == "K" else x for x in shape), dtype=getattr(torch, dt), device="cuda")
           for c, (dt, shape) in game_log.CANDIDATE_COLUMNS.items() if c != "after_obs"}   # (a row to spare: a pointer may be moved)
    torch.cuda.synchronize()
    rows = _lib.ReplayRows(action=act.data_ptr())
    good = {game_log._AFTER_FIELD[c]: t.data_ptr() for c, t in buf.items()}
    cases = [(good, 0), (good, 157), (good, -1), ({**good, "n_legal": None}, K), ({**good, "action": None}, K),
             ({**good, "n_legal": good["n_legal"] + 2}, K), ({**good, "chosen": good["chosen"] + 1}, K),
             ({**good, "features": good["features"] + 4}, K), ({**good, "before_features": good["before_features"] + 4}, K),
             ({**good, "obs": good["n_legal"] + 2}, K)]
    for fields, k_after in cases:
        status, replayed, fault = np.full(len(m), 9, np.uint8), np.full(len(m), -9, np.int32), np.full(len(m), 9, np.uint8)
        n_rows = ctypes.c_int64(-9)
        rc = eng.lib.monsoon_replay_logged_after_dev(eng.h, _ptr(m), len(m), _ptr(pairs), len(pairs), _ptr(action), action.shape[1],
                                                     _ptr(steps), None, ctypes.byref(rows), total, ctypes.byref(n_rows), _ptr(status),
                                                     _ptr(replayed), _ptr(fault), ctypes.byref(_lib.ReplayAfter(**fields)), k_after)
        assert rc == _lib.ERR_ARG and n_rows.value == -9, (fields, k_after)
        assert (status == 9).all() and (replayed == -9).all() and (fault == 9).all() and (act == 7).all()
        assert all(not t.any() for t in buf.values()) and np.array_equal(eng.state_hash(), hashes)
    # after == NULL is monsoon_replay_logged_dev; and the good arguments run
    n_rows = ctypes.c_int64(-9)
    rc = eng.lib.monsoon_replay_logged_after_dev(eng.h, _ptr(m), len(m), _ptr(pairs), len(pairs), _ptr(action), action.shape[1], _ptr(steps),
                                                 None, ctypes.byref(rows), total, ctypes.byref(n_rows), None, None, None, None, 0)
    assert rc == 0 and n_rows.value == total and np.array_equal(act.cpu().numpy(), clean["action"].cpu().numpy())
    before = eng.stats()
    got = eng.replay_logged(m, pairs, action, steps, rows, total, None, _lib.ReplayAfter(**good), K)
    after = eng.stats()
    eng.close()
    assert got[0] == total and not got[1].any()
    n_legal = buf["n_legal"][:total].cpu().numpy()
    assert np.array_equal(n_legal, AM.host(clean)["n_legal"]) and not buf["n_legal"][total:].any()
    # monsoon_get_stats: the candidates stepped, and no decision
    assert after["lookahead_steps"] - before["lookahead_steps"] == np.minimum(n_legal, K).sum() > 0
    assert after["decisions"] == before["decisions"]
