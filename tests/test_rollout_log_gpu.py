"""monsoon_rollout_logged on the device: the whole-game launch (k_play_log) against the reference's traces at every
decision, against the unlogged rollouts it must not differ from, and against the model of its log
(tests/rollout_log_model.py, pinned to the reference by tests/test_rollout_log_cpu.py).  No reference tree involved."""
import ctypes
import os

import numpy as np
import pytest

import rollout_log_model as R
from monsoon_amd import EXPERT, _lib, game_log
from monsoon_amd.cards import C5_STREAM_XOR, deck_indices, draw_random_decks_numpy
from monsoon_amd.config import EvolutionaryConfig
from monsoon_amd.engine import BatchEngine, RolloutLog, _ptr
from monsoon_amd.fitness import MATCH_DTYPE, FitnessEvaluator, hash32_array

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W0 = np.random.RandomState(2024).uniform(0, 1, 10)
W2 = np.stack([W0, np.random.RandomState(7).uniform(0, 1, 10)])   # two weight vectors


def _padded(log, k, n):
    """Row k holds nothing but padding behind its n-th entry."""
    return bool((log.action[k, n:] == 255).all() and np.isnan(log.score[k, n:]).all() and not log.n_legal[k, n:].any())


def _fixture_pairs(g):
    if "decks" in g.files:
        return g["decks"]
    if "deck0" in g.files:
        return np.stack([g["deck0"], g["deck1"]], axis=1)
    return np.stack([g["deck"], g["deck1"] if "deck1" in g.files else g["deck"]])[None]


@pytest.mark.parametrize("fixture,build", [("trace_heuristic_S12", 0), ("trace_heuristic_IRONCLAD", 0), ("trace_heuristic_N12M", 0),
                                           ("trace_heuristic_pool", 0), ("trace_heuristic_pool_ext", 1), ("trace_heuristic_c5_big", 2),
                                           ("trace_heuristic_N12M_2w", 0)])
def test_whole_game_launch_equals_the_reference_at_every_decision(fixture, build):
    """One rollout_logged call per fixture: the action, the best score (bit for bit) and the legal count of every decision
    of every game are the reference's, the game is as long as the reference's, and the row is padding behind it."""
    g = np.load(os.path.join(GOLD, fixture + ".npz"))
    n = len(g["seeds"])
    pairs = _fixture_pairs(g)
    m = np.zeros(n, dtype=MATCH_DTYPE)
    m["seed"] = g["seeds"]
    if len(pairs) > 1:
        m["deck"] = np.arange(n)
    weights = g["w0"][None]
    if "w1" in g.files:   # per-side weights: FIRST plays row 0, SECOND row 1
        weights = np.stack([g["w0"], g["w1"]])
        m["p2"] = 1
    eng = BatchEngine(64, extended=build)
    _, results, steps, log = eng.rollout_logged(weights, m, pairs, int(g["max_turns"]))
    eng.close()
    lengths = np.diff(g["offsets"])
    assert np.array_equal(steps, lengths) and np.array_equal(log.steps, lengths) and np.array_equal(results, g["result"])
    for k in range(n):
        lo, hi, ln = int(g["offsets"][k]), int(g["offsets"][k + 1]), int(lengths[k])
        assert np.array_equal(log.action[k, :ln], g["action"][lo:hi]), k
        assert np.array_equal(log.score[k, :ln].view(np.uint64), g["best"][lo:hi].view(np.uint64)), k
        assert np.array_equal(log.n_legal[k, :ln], g["nlegal"][lo:hi]), k
        assert _padded(log, k, ln), k


def test_fixture_games_against_the_bot():
    """trace_vs_expert.npz, 40 games of the reference's own play: every action of either side, a NaN score and a legal count
    of 0 exactly on the bot's steps; results, steps and faults as test_vs_expert_gpu checks them."""
    g = np.load(os.path.join(GOLD, "trace_vs_expert.npz"))
    n = len(g["seeds"])
    m = np.zeros(n, dtype=MATCH_DTYPE)
    m["seed"], m["deck"] = g["seeds"], np.arange(n)
    m["p1"] = np.where(g["bot_side"] == 1, 0, EXPERT)
    m["p2"] = np.where(g["bot_side"] == 1, EXPERT, 0)
    eng = BatchEngine(64)
    counts, results, steps, log = eng.rollout_logged(g["w0"][None], m, _fixture_pairs(g), int(g["max_turns"]))
    faults, hashes = eng.rollout_faults(n), eng.state_hash()
    assert np.array_equal(results, g["result"]) and np.array_equal(steps, g["steps"]) and np.array_equal(faults != 0, g["fault"] != 0)
    ok = g["fault"] == 0
    assert ok.sum() == 37 and np.array_equal(hashes[ok], g["final"][ok])
    agent_wins = int((results == np.where(g["bot_side"] == 1, 0, 1)).sum())
    assert counts.tolist() == [[agent_wins, int((results == -1).sum()), n]]
    assert eng.stats()["decisions"] == int((g["bot"] == 0).sum())
    eng.close()
    assert np.array_equal(np.diff(g["offsets"]), steps)
    for k in range(n):
        lo, hi, ln = int(g["offsets"][k]), int(g["offsets"][k + 1]), int(steps[k])
        bot = g["bot"][lo:hi] == 1
        assert np.array_equal(log.action[k, :ln], g["action"][lo:hi]), k
        assert np.array_equal(np.isnan(log.score[k, :ln]), bot) and np.array_equal(log.n_legal[k, :ln] == 0, bot), k
        assert _padded(log, k, ln), k


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


def test_logging_changes_nothing_else():
    """600 matches in three batches of a 256-game handle, the last one partial, max_turns 60 so that some games truncate:
    counts, results, steps, faults, the last batch's hashes and the statistics of rollout_vs_expert; a row holds exactly
    steps[k] entries; and the bot-free schedule equals the plain rollout."""
    n, T = 600, 60
    m, pairs = _schedule(n), _n12m()
    plain, logged = BatchEngine(256), BatchEngine(256)
    a = plain.rollout_vs_expert(W2, m, pairs, T, want_results=True)
    b = logged.rollout_logged(W2, m, pairs, T)
    log = b[3]
    for x, y in zip(a, b[:3]):
        assert np.array_equal(x, y)
    assert np.array_equal(plain.rollout_faults(n), logged.rollout_faults(n))
    assert plain.n == logged.n == n - 512 and np.array_equal(plain.state_hash(), logged.state_hash())
    sa, sb = plain.stats(), logged.stats()
    assert (sa["decisions"], sa["lookahead_steps"]) == (sb["decisions"], sb["lookahead_steps"]) and sa["decisions"] > 0
    steps = b[2]
    assert np.array_equal((log.action != 255).sum(axis=1), steps) and np.array_equal(log.steps, steps)
    assert all((log.action[k, :steps[k]] != 255).all() for k in range(n))
    assert (steps == T).any() and (steps < T).any()   # truncated rows are full
    free = _schedule(n, bot=False)
    c = plain.rollout(W2, free, pairs, T, want_results=True)
    d = logged.rollout_logged(W2, free, pairs, T)
    for x, y in zip(c, d[:3]):
        assert np.array_equal(x, y)
    assert not np.isnan(d[3].score[:, 0]).any() and (d[3].n_legal[:, 0] > 0).all()
    plain.close()
    logged.close()


def test_whole_log_equals_the_model():
    """192 matches of the mixed schedule, S12 and N12M alternating: every entry and every padding byte of the log."""
    n, T = 192, 200
    m = _schedule(n, seed0=1)
    m["deck"] = (np.arange(n) // 3) % 2
    pairs = np.stack([np.stack([deck_indices(d)] * 2) for d in ("S12", "N12M")])
    eng = BatchEngine(256)
    counts, results, steps, log = eng.rollout_logged(W2, m, pairs, T)
    faults = eng.rollout_faults(n)
    eng.close()
    model = R.ModelEngine(0)
    ref = model.rollout_logged(W2, m, pairs, T)
    assert np.array_equal(counts, ref[0]) and np.array_equal(results, ref[1]) and np.array_equal(faults, model.rollout_faults(n))
    assert R.same_log(log, ref[3])
    assert np.isnan(log.score[log.action != 255]).any() and (log.n_legal > 0).any()


def test_edges():
    pairs = _n12m()
    eng = BatchEngine(64)
    model = R.ModelEngine(0)
    m = _schedule(12, seed0=2)
    for T, sub in ((1, m), (200, m[2:3]), (200, m[:1])):   # max_turns = 1; a schedule of one match (plain / with the bot)
        counts, results, steps, log = eng.rollout_logged(W2, sub, pairs, T)
        ref = model.rollout_logged(W2, sub, pairs, T)
        assert log.action.shape == (len(sub), T) and np.array_equal(counts, ref[0]) and np.array_equal(results, ref[1])
        assert R.same_log(log, ref[3])
    # action only
    full = eng.rollout_logged(W2, m, pairs, 50)
    only = eng.rollout_logged(W2, m, pairs, 50, scores=False, n_legal=False)
    assert only[3].score is None and only[3].n_legal is None and np.array_equal(only[3].action, full[3].action)
    assert np.array_equal(only[2], full[2]) and (only[3].action != 255).any()
    # NULL log / NULL action: refused, and the handle plays on
    c_m, c_w, c_p = np.ascontiguousarray(m), np.ascontiguousarray(W2), np.ascontiguousarray(pairs)
    counts = np.zeros((2, 3), dtype=np.int32)
    for c_log in (None, ctypes.byref(_lib.RolloutLog(None, None, None))):
        rc = eng.lib.monsoon_rollout_logged(eng.h, _ptr(c_w), 2, _ptr(c_m), len(m), _ptr(c_p), 1, 50, _ptr(counts), None, None, c_log)
        assert rc == _lib.ERR_ARG and not counts.any()
    free = _schedule(12, seed0=2, bot=False)
    fresh = BatchEngine(64)
    for x, y in zip(eng.rollout(W2, free, pairs, 50, want_results=True), fresh.rollout(W2, free, pairs, 50, want_results=True)):
        assert np.array_equal(x, y)
    fresh.close()
    eng.close()


def test_other_lane_counts_run_the_default_variants_kernel():
    """A lanes_per_game=4 handle logs through the build's default k_play_log: the same rows as a default handle."""
    pairs = _n12m()
    m = _schedule(300, seed0=5)
    out = []
    for lanes in (0, 4):
        eng = BatchEngine(128, lanes_per_game=lanes)
        counts, results, steps, log = eng.rollout_logged(W2, m, pairs, 200)
        out.append((counts, results, steps, log.action, log.n_legal, np.nan_to_num(log.score, nan=-1.0), eng.rollout_faults(len(m)),
                    eng.state_hash()))
        eng.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_log_budget_cuts_the_batch():
    """max_turns = 30000: 11 bytes x 30 000 entries per game let 813 games into the 256 MiB of a batch, so a 1024-game handle
    plays 1 024 matches in two batches; the rows are those of a 256-game handle's four."""
    n, T = 1024, 30000
    d = deck_indices("S12")
    pairs = np.stack([d, d])[None]
    m = _schedule(n, seed0=4, bot=False)
    out = []
    for cap in (1024, 256):
        eng = BatchEngine(cap)
        counts, results, steps, log = eng.rollout_logged(W2, m, pairs, T, scores=False, n_legal=False)
        out.append((counts, results, steps, log.action, eng.rollout_faults(n), eng.n))
        eng.close()
    assert out[0][5] == n - 813 and out[1][5] == 256
    for x, y in zip(out[0][:5], out[1][:5]):
        assert np.array_equal(x, y)
    steps, action = out[0][2], out[0][3]
    assert np.array_equal((action != 255).sum(axis=1), steps) and (steps > 0).all()


def _drain(gen):
    items = []
    while True:
        try:
            items.append(next(gen))
        except StopIteration as stop:
            return items, stop.value


def test_replay_on_a_second_handle():
    """64 bot-free S12 games logged, then played again from the log through reset / legal_mask / step: the same final
    states (where no step faulted: behind one the whole-game kernel and the step kernel stop at different points)."""
    n = 64
    d = deck_indices("S12")
    pairs = np.stack([d, d])[None]
    m = _schedule(n, seed0=6, bot=False)
    eng, second = BatchEngine(64), BatchEngine(64)
    _, _, steps, log = eng.rollout_logged(W2, m, pairs, 200)
    faults, hashes = eng.rollout_faults(n), eng.state_hash()
    items, finals = _drain(game_log.replay(second, m, pairs, log))
    ok = faults == 0
    assert ok.sum() >= 0.9 * n and np.array_equal(finals[ok], hashes[ok])
    assert sum(int(it[0].sum()) for it in items) == steps.sum() and len(items) == steps.max()
    live, to_play, mask, obs, action = items[0]
    assert live.all() and (to_play == 0).all() and obs.shape == (n, 27, 5, 4) and mask.shape == (n, 3)
    eng.close()
    second.close()


def test_tiers_on_the_device():
    """FitnessEvaluator.logged_games on 256 random 109-card-pair matches, a third each with the bot FIRST / SECOND: the log,
    results, steps, faults and counts of game_log.logged_rollout over the model's three records."""
    from monsoon_amd.cards import needs_extended_each
    n, T = 256, 100
    m = _schedule(n, seed0=3)
    m["deck"] = np.arange(n)
    pairs = draw_random_decks_numpy(m["seed"] ^ np.uint32(C5_STREAM_XOR))
    assert needs_extended_each(pairs).any() and not needs_extended_each(pairs).all()   # both first tiers
    ev = FitnessEvaluator(EvolutionaryConfig(max_turns=T, max_concurrent_games=512, deck="random109"))
    counts, results, steps, faults, log = ev.logged_games(W2, m, pairs)
    models = {}
    ref = game_log.logged_rollout(lambda t: models.setdefault(t, R.ModelEngine(t)), W2, m, pairs, T)
    assert np.array_equal(counts, ref[0]) and np.array_equal(results, ref[1]) and np.array_equal(steps, ref[2])
    assert np.array_equal(faults, ref[3]) and R.same_log(log, ref[4])
    assert isinstance(log, RolloutLog) and counts[:, 2].sum() == n
