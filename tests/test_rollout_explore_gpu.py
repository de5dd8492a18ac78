"""monsoon_rollout_explore on the device (k_play_explore): against monsoon_rollout_logged where nothing explores, and entry
by entry against the model over the CPU oracle (tests/explore_model.py) where decisions do -- on the three record builds,
with the places the kernel can go wrong counted from the model's own log."""
import ctypes

import numpy as np
import pytest

import explore_model as X
from monsoon_amd import EXPERT, _lib, game_log
from monsoon_amd.cards import C5_STREAM_XOR, CARD_INDEX, deck_indices, draw_random_decks_numpy, needs_extended_each
from monsoon_amd.engine import BatchEngine, Explore, RolloutLog, _ptr
from monsoon_amd.fitness import MATCH_DTYPE, hash32_array

pytestmark = pytest.mark.gpu

W0 = np.random.RandomState(2024).uniform(0, 1, 10)
W2 = np.stack([W0, np.random.RandomState(7).uniform(0, 1, 10)])   # two weight vectors
U = 8   # candidate lanes per pass of every build's default variant (variants.def)


def _schedule(n, seed0=0, bot=True):
    """n matches over the two rows of W2: a third each of bot-FIRST, bot-SECOND and plain; bot=False: the same seeds and rows
    without the bot."""
    m = np.zeros(n, dtype=MATCH_DTYPE)
    k = np.arange(n)
    row, third = k % 2, k % 3 if bot else np.full(n, 2)
    m["seed"] = hash32_array(seed0, k, 0xE)
    m["p1"] = np.where(third == 0, EXPERT, row)
    m["p2"] = np.where(third == 1, EXPERT, np.where(third == 0, row, 1 - row))
    return m


def _n12m():
    d = deck_indices("N12M")
    return np.stack([d, d])[None]


def _standard_set():
    """48 mixed matches: the even ones on N12M, the odd ones on random 109-card pairs the standard record holds."""
    n = 48
    m = _schedule(n, seed0=21)
    drawn = draw_random_decks_numpy(hash32_array(77, np.arange(4 * n)) ^ np.uint32(C5_STREAM_XOR))
    drawn = drawn[~needs_extended_each(drawn)][:n // 2]
    assert len(drawn) == n // 2
    pairs = np.concatenate([_n12m(), drawn])
    m["deck"] = np.where(np.arange(n) % 2 == 0, 0, 1 + np.arange(n) // 2)
    return m, pairs


def _engine(max_games=64, build=0):
    """A handle; torch loads its runtime before the library does (VecEnv.__init__ says why), for the sake of dataset."""
    import torch
    assert torch.cuda.is_available()
    return BatchEngine(max_games, extended=build)


def _device(build, cap, m, pairs, T, ex):
    eng = _engine(cap, build)
    assert eng.variant()[0] == U
    counts, results, steps, log = eng.rollout_logged(W2, m, pairs, T, explore=ex)
    out = dict(counts=counts, results=results, steps=steps, log=log, faults=eng.rollout_faults(len(m)), hashes=eng.state_hash(), n=eng.n,
               stats=eng.stats())
    eng.close()
    return out


def _model(build, m, pairs, T, ex):
    model = X.ModelEngine(build)
    counts, results, steps, log = model.rollout_logged(W2, m, pairs, T, explore=ex)
    return dict(counts=counts, results=results, steps=steps, log=log, faults=model.rollout_faults(len(m)), finals=model.finals,
                games=model.games)


def _assert_equals_model(dev, ref, last_batch_from=0):
    assert np.array_equal(dev["steps"], ref["steps"]) and np.array_equal(dev["results"], ref["results"])
    assert np.array_equal(dev["counts"], ref["counts"]) and np.array_equal(dev["faults"], ref["faults"])
    assert X.same_log(dev["log"], ref["log"])
    ok = ref["faults"][last_batch_from:] == 0   # (behind a faulting step the kernel and the oracle stop at different points)
    assert ok.sum() >= 0.7 * len(ok) and np.array_equal(dev["hashes"][ok], ref["finals"][last_batch_from:][ok])
    assert dev["stats"]["decisions"] == sum(g["decisions"] for g in ref["games"])
    assert dev["stats"]["lookahead_steps"] == sum(g["lookahead"] for g in ref["games"])


@pytest.fixture(scope="module")
def standard():
    """The standard set under Explore(0.25, 9), by the model and by a 64-game handle: computed once, read by several tests."""
    m, pairs = _standard_set()
    ex, T = Explore(0.25, 9), 200
    return m, pairs, ex, T, _model(0, m, pairs, T, ex), _device(0, 64, m, pairs, T, ex)


def test_nothing_changes_without_exploration():
    """64 mixed matches: explore=None and Explore(0, s) equal rollout_logged of the parent contract bit for bit -- log, counts,
    results, steps, faults, hashes, statistics -- and greedy = action, taken_score = score on decisions."""
    n, T = 64, 200
    m, pairs = _schedule(n), _n12m()
    eng = _engine()
    counts = np.zeros((2, 3), dtype=np.int32)
    results, steps, log = np.zeros(n, dtype=np.int8), np.zeros(n, dtype=np.int32), RolloutLog.empty(n, T)
    c_log = _lib.RolloutLog(_ptr(log.action), _ptr(log.score), _ptr(log.n_legal))
    args = (_ptr(np.ascontiguousarray(W2)), 2, _ptr(m), n, _ptr(np.ascontiguousarray(pairs)), 1, T)
    assert eng.lib.monsoon_rollout_logged(eng.h, *args, _ptr(counts), _ptr(results), _ptr(steps), ctypes.byref(c_log)) == _lib.OK
    eng.n = n
    parent = dict(counts=counts, results=results, steps=steps, faults=eng.rollout_faults(n), hashes=eng.state_hash(), stats=eng.stats())
    eng.close()
    assert (steps > 0).all() and (log.n_legal > 0).any() and np.isnan(log.score[log.action != 255]).any()
    none = _device(0, 64, m, pairs, T, None)
    zero = _device(0, 64, m, pairs, T, Explore(0.0, 1234))
    for got in (none, zero):
        for key in ("counts", "results", "steps", "faults", "hashes"):
            assert np.array_equal(got[key], parent[key]), key
        assert got["stats"] == parent["stats"]
        assert np.array_equal(got["log"].action, log.action) and np.array_equal(got["log"].n_legal, log.n_legal)
        assert np.array_equal(got["log"].score.view(np.uint64), log.score.view(np.uint64))   # the padding's bits too
    assert none["log"].greedy is None
    zl, decision = zero["log"], log.n_legal > 0
    assert np.array_equal(zl.greedy[decision], log.action[decision]) and (zl.greedy[~decision] == 255).all()
    assert not zl.explored.any()
    assert np.array_equal(zl.taken_score[decision].view(np.uint64), log.score[decision].view(np.uint64))
    assert np.isnan(zl.taken_score[~decision]).all()


def test_the_standard_set_reaches_every_place_the_kernel_can_go_wrong(standard):
    """From the model's log alone: the explored rank in the first pass, in a later pass, in a third or later pass, at the end
    of a partial last pass, equal to the greedy action's rank, in an earlier and in a later pass than the greedy action,
    and an explored decision immediately followed by a decision of the same side."""
    seen = dict.fromkeys(("first_pass", "later_pass", "third_pass", "last_of_partial", "is_greedy", "greedy_later", "greedy_earlier",
                          "same_side_next"), 0)
    for g in standard[4]["games"]:
        for k in range(g["steps"]):
            r, gr, nl = g["rank"][k], g["greedy_rank"][k], g["n_legal"][k]
            if r < 0:
                continue
            seen["first_pass"] += r < U
            seen["later_pass"] += r >= U
            seen["third_pass"] += r >= 2 * U
            seen["last_of_partial"] += r == nl - 1 and nl % U != 0
            seen["is_greedy"] += r == gr
            seen["greedy_later"] += gr // U > r // U
            seen["greedy_earlier"] += gr // U < r // U
            seen["same_side_next"] += k + 1 < g["steps"] and not g["bot"][k + 1] and g["side"][k + 1] == g["side"][k]
    assert all(v > 0 for v in seen.values()), seen


def test_device_log_equals_model_log_standard(standard):
    m, pairs, ex, T, ref, dev = standard
    _assert_equals_model(dev, ref)
    log = dev["log"]
    assert log.explored.any() and (log.greedy != log.action).any() and np.isnan(log.taken_score[log.action != 255]).any()
    differ = (log.explored != 0) & (log.greedy != log.action)
    assert (log.taken_score[differ] <= log.score[differ]).all()   # (the arg-max is the arg-max)


def test_device_log_equals_model_log_extended():
    """8 matches with ua20 / b005 on a side, on the extended build."""
    n, T = 8, 120
    m = _schedule(n, seed0=31)
    std = deck_indices("N12M")
    a, b = std.copy(), std.copy()
    a[0], b[1] = CARD_INDEX["ua20"], CARD_INDEX["b005"]
    pairs = np.stack([np.stack([a, b]), np.stack([b, a])])
    assert needs_extended_each(pairs).all()
    m["deck"] = np.arange(n) % 2
    ex = Explore(0.25, 10)
    ref = _model(1, m, pairs, T, ex)
    assert any((np.array(g["rank"]) >= U).any() for g in ref["games"])
    _assert_equals_model(_device(1, 64, m, pairs, T, ex), ref)


def test_device_log_equals_model_log_large():
    """4 matches on the large build."""
    n, T = 4, 120
    m, pairs = _schedule(n, seed0=32), _n12m()
    ex = Explore(0.25, 11)
    ref = _model(2, m, pairs, T, ex)
    assert any((np.array(g["rank"]) >= U).any() for g in ref["games"])
    _assert_equals_model(_device(2, 64, m, pairs, T, ex), ref)


def test_sides_and_step_limit():
    """Explore(1.0, s, sides="first", until_step=4): every explored entry is a FIRST decision with k < 4, every such decision
    explored, and the whole log is the model's."""
    n, T = 16, 200
    m, pairs = _schedule(n, seed0=33), _n12m()
    ex = Explore(1.0, 12, sides="first", until_step=4)
    ref = _model(0, m, pairs, T, ex)
    dev = _device(0, 64, m, pairs, T, ex)
    _assert_equals_model(dev, ref)
    log, found = dev["log"], 0
    for i, g in enumerate(ref["games"]):
        side, bot = np.array(g["side"]), np.array(g["bot"])
        where = np.nonzero(log.explored[i])[0]
        assert (where < 4).all() and (side[where] == 0).all() and not bot[where].any()
        may = (np.arange(g["steps"]) < 4) & (side == 0) & (bot == 0)
        assert np.array_equal(np.nonzero(may)[0], where)   # (no draw0 of these games is 0xFFFFFFFF)
        found += len(where)
    assert found > 0 and (log.explored.sum(axis=1) <= 4).all()


def test_batch_invariance(standard):
    """The 48-match exploring schedule on a 16-game handle (three batches) gives the 64-game handle's logs and results."""
    m, pairs, ex, T, ref, dev = standard
    small = _device(0, 16, m, pairs, T, ex)
    assert small["n"] == 16 and dev["n"] == 48
    for key in ("counts", "results", "steps", "faults"):
        assert np.array_equal(small[key], dev[key]), key
    assert X.same_log(small["log"], dev["log"])
    assert np.array_equal(small["hashes"], dev["hashes"][32:])   # the last batch


def test_dataset_carries_the_new_columns(standard):
    """game_log.dataset over the explored log, bot games included, under a keep mask that drops entries: every game replays
    to its end (an explored action is legal), the final hashes are the rollout's, and greedy / explored are the log's arrays
    gathered at the kept entries in row order."""
    m, pairs, ex, T, ref, dev = standard
    log = dev["log"]
    keep = np.ones(log.action.shape, dtype=np.uint8)
    keep[:, 1::3] = 0
    keep[5] = 0
    eng = _engine()
    d = game_log.dataset(eng, m, pairs, log, keep=keep, columns=("action", "game", "step", "greedy", "explored"))
    hashes = eng.state_hash()
    eng.close()
    assert not d["status"].any() and np.array_equal(d["replayed"], log.steps)
    assert np.array_equal(hashes, dev["hashes"])
    game, step = d["game"].cpu().numpy(), d["step"].cpu().numpy()
    assert len(game) == int(game_log.kept_counts(log.steps, keep).sum()) and not (game == 5).any() and not (step % 3 == 1).any()
    assert np.array_equal(d["action"].cpu().numpy(), log.action[game, step])
    assert np.array_equal(d["greedy"].cpu().numpy(), log.greedy[game, step])
    assert np.array_equal(d["explored"].cpu().numpy(), log.explored[game, step])
    assert d["explored"].any() and (d["greedy"] != d["action"]).any()
    plain = RolloutLog(log.action, log.score, log.n_legal, log.steps)
    with pytest.raises(ValueError, match="Explore rule"):
        game_log.dataset(None, m, pairs, plain, columns=("greedy",))


def test_bad_arguments_leave_the_games_untouched():
    """A sides bit above bit 1 is MONSOON_ERR_ARG: nothing is launched, the loaded games keep their states."""
    n, T = 16, 50
    m, pairs = _schedule(n, seed0=34), _n12m()
    eng = _engine()
    eng.rollout_logged(W2, m, pairs, T, explore=Explore(0.5, 3))
    before = eng.state_hash()
    counts = np.zeros((2, 3), dtype=np.int32)
    log = RolloutLog.empty(n, T, explore=True)
    c_log = _lib.RolloutLog(_ptr(log.action), _ptr(log.score), _ptr(log.n_legal))
    c_xlog = _lib.ExploreLog(_ptr(log.greedy), _ptr(log.explored), _ptr(log.taken_score))
    args = (_ptr(np.ascontiguousarray(W2)), 2, _ptr(m), n, _ptr(np.ascontiguousarray(pairs)), 1, T, _ptr(counts), None, None)
    for sides in (4, 7, 1 << 31):
        c_ex = _lib.Explore(3, 1 << 31, sides, 0)
        rc = eng.lib.monsoon_rollout_explore(eng.h, *args, ctypes.byref(c_log), ctypes.byref(c_ex), ctypes.byref(c_xlog))
        assert rc == _lib.ERR_ARG and not counts.any() and (log.action == 255).all()
    for bad_log in (None, ctypes.byref(_lib.RolloutLog(None, None, None))):   # what monsoon_rollout_logged refuses
        c_ex = _lib.Explore(3, 1 << 31, 3, 0)
        assert eng.lib.monsoon_rollout_explore(eng.h, *args, bad_log, ctypes.byref(c_ex), ctypes.byref(c_xlog)) == _lib.ERR_ARG
    assert np.array_equal(eng.state_hash(), before)
    c_ex = _lib.Explore(3, 1 << 31, 3, 0)   # and the handle plays on: NULL xlog, all three of its arrays NULL
    assert eng.lib.monsoon_rollout_explore(eng.h, *args, ctypes.byref(c_log), ctypes.byref(c_ex), None) == _lib.OK
    again = eng.rollout_logged(W2, m, pairs, T, explore=Explore(0.5, 3))
    assert np.array_equal(again[3].action, log.action) and counts[:, 2].sum() == n
    eng.close()
