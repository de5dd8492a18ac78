"""monsoon_rollout_vs_expert on the device against the model of its contract (tests/vs_expert_model.py, pinned to the
reference by tests/test_vs_expert_cpu.py).  No reference tree involved."""
import os
from concurrent.futures import ProcessPoolExecutor
import multiprocessing as mp

import numpy as np
import pytest

import vs_expert_model as M
from monsoon_amd import EXPERT, MonsoonError
from monsoon_amd.cards import C5_STREAM_XOR, deck_indices, draw_random_decks_numpy
from monsoon_amd.config import EvolutionaryConfig
from monsoon_amd.engine import BatchEngine
from monsoon_amd.fitness import MATCH_DTYPE, FitnessEvaluator, hash32_array

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W0 = np.random.RandomState(2024).uniform(0, 1, 10)
W2 = np.stack([W0, np.random.RandomState(7).uniform(0, 1, 10)])   # two weight vectors


def _chunk(args):
    weights, matches, deck_pairs, max_turns, tiered = args
    if tiered:
        return M.vs_expert_rollout_fn(weights, matches, deck_pairs, max_turns, want_faults=True) + (None,)
    return M.rollout_tier(weights, matches, deck_pairs, max_turns, 0)


def model(weights, matches, deck_pairs, max_turns, tiered=False, workers=16):
    """(counts, results, steps, faults, finals) by the model, the schedule split over fresh worker processes (finals is
    None with tiered=True: tiered_rollout over the three records, as FitnessEvaluator plays)."""
    parts = [p for p in np.array_split(np.arange(len(matches)), workers) if len(p)]
    with ProcessPoolExecutor(len(parts), mp_context=mp.get_context("spawn")) as ex:
        out = list(ex.map(_chunk, [(weights, matches[p], deck_pairs, max_turns, tiered) for p in parts]))
    counts = sum(o[0] for o in out)
    cat = lambda k: None if out[0][k] is None else np.concatenate([o[k] for o in out])   # noqa: E731
    return counts, cat(1), cat(2), cat(3), cat(4)


def _schedule(kind, n, seed0=0):
    """n matches over the two rows of W2: the bot SECOND, FIRST, or a third each of bot-FIRST, bot-SECOND and plain."""
    m = np.zeros(n, dtype=MATCH_DTYPE)
    k = np.arange(n)
    row = k % 2
    m["seed"] = hash32_array(seed0, k, 0xE)
    if kind == "second":
        m["p1"], m["p2"] = row, EXPERT
    elif kind == "first":
        m["p1"], m["p2"] = EXPERT, row
    else:
        third = k % 3
        m["p1"] = np.where(third == 0, EXPERT, row)
        m["p2"] = np.where(third == 1, EXPERT, np.where(third == 0, row, 1 - row))
    return m


def test_fixture_games_on_the_device():
    """Every game of trace_vs_expert.npz (the reference's own play): result, steps, fault and final hash.  The final hash
    of the three games that end on a step that raises is the model's (behind an exception the reference leaves a
    half-made move)."""
    g = np.load(os.path.join(GOLD, "trace_vs_expert.npz"))
    n = len(g["seeds"])
    m = np.zeros(n, dtype=MATCH_DTYPE)
    m["seed"], m["deck"] = g["seeds"], np.arange(n)
    m["p1"] = np.where(g["bot_side"] == 1, 0, EXPERT)
    m["p2"] = np.where(g["bot_side"] == 1, EXPERT, 0)
    pairs = np.stack([g["deck0"], g["deck1"]], axis=1)
    eng = BatchEngine(64)
    counts, results, steps = eng.rollout_vs_expert(g["w0"][None], m, pairs, int(g["max_turns"]), want_results=True)
    faults, hashes = eng.rollout_faults(n), eng.state_hash()
    assert np.array_equal(results, g["result"]) and np.array_equal(steps, g["steps"]) and np.array_equal(faults != 0, g["fault"] != 0)
    ok = g["fault"] == 0
    assert ok.sum() == 37 and np.array_equal(hashes[ok], g["final"][ok])
    ref = model(g["w0"][None], m, pairs, int(g["max_turns"]))
    assert np.array_equal(hashes[ok], ref[4][ok]) and np.array_equal(faults, ref[3]) and np.array_equal(counts, ref[0])
    agent_wins = int((results == np.where(g["bot_side"] == 1, 0, 1)).sum())
    assert counts.tolist() == [[agent_wins, int((results == -1).sum()), n]]
    st = eng.stats()
    assert st["decisions"] == int((g["bot"] == 0).sum())   # the heuristic agent's decisions only
    eng.close()


@pytest.mark.parametrize("deck", ["N12M", "S12"])
@pytest.mark.parametrize("kind", ["second", "first", "mixed"])
def test_2048_games_equal_the_model(deck, kind):
    n = 2048
    d = deck_indices(deck)
    pairs = np.stack([d, d])[None]
    m = _schedule(kind, n)
    eng = BatchEngine(4096)
    counts, results, steps = eng.rollout_vs_expert(W2, m, pairs, 200, want_results=True)
    faults, hashes = eng.rollout_faults(n), eng.state_hash()
    st = eng.stats()
    ref = model(W2, m, pairs, 200)
    assert np.array_equal(results, ref[1]) and np.array_equal(steps, ref[2]) and np.array_equal(faults, ref[3])
    assert np.array_equal(counts, ref[0]) and counts[:, 2].sum() == n
    ok = faults == 0   # (the state behind a step that raised is the core's partial state: the two cores stop at different points)
    assert np.array_equal(hashes[ok], ref[4][ok]) and ok.sum() > 0.9 * n
    assert st["decisions"] < int(steps.sum()) and st["lookahead_steps"] > 10 * st["decisions"]
    eng.close()


@pytest.mark.parametrize("kind", ["second", "first", "mixed"])
def test_random_109_card_pairs_through_the_evaluator(kind):
    """Per-game decks from the 109 observable cards: the extended tier and the ladder run (FitnessEvaluator._hip_rollout
    = tiered_rollout over the three handles), against the model doing the same over the oracle's three records."""
    n = 2048
    m = _schedule(kind, n, seed0=3)
    m["deck"] = np.arange(n)
    pairs = draw_random_decks_numpy(m["seed"] ^ np.uint32(C5_STREAM_XOR))
    ev = FitnessEvaluator(EvolutionaryConfig(max_turns=200, max_concurrent_games=4096, deck="random109"))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # games left on a limit of the largest record are compared like any other
        counts = ev._hip_rollout(W2, m, pairs, 200)
    results, steps, faults = ev.last_rollout
    ref = model(W2, m, pairs, 200, tiered=True)
    assert ev.tier_games[0] > 0 and ev.tier_games[1] > 0
    assert np.array_equal(results, ref[1]) and np.array_equal(steps, ref[2]) and np.array_equal(faults, ref[3])
    assert np.array_equal(counts, ref[0])


def test_evaluate_vs_expert_on_the_device():
    """The public entry: 8 individuals x 16 games with alternating sides = the model's scores and counts."""
    np.random.seed(3)
    from monsoon_amd.weights import WeightVector
    pop = [WeightVector(10) for _ in range(8)]
    cfg = EvolutionaryConfig(max_turns=100, max_concurrent_games=1024)
    ev = FitnessEvaluator(cfg)
    scores = ev.evaluate_vs_expert(pop, generation=1, games_per_individual=16)
    ref = FitnessEvaluator(cfg, rollout_fn=M.vs_expert_rollout_fn)
    assert scores == ref.evaluate_vs_expert(pop, generation=1, games_per_individual=16)
    assert np.array_equal(ev.last_vs_expert, ref.last_vs_expert) and (ev.last_vs_expert[:, 2] == 16).all()


def test_other_lane_counts_run_the_default_variants_kernel():
    """A lanes_per_game=4 handle plays its plain rollouts on k_play<4, 4> and the bot's on the build's default k_play_vs:
    the same rows as a default handle."""
    d = deck_indices("N12M")
    pairs = np.stack([d, d])[None]
    m = _schedule("mixed", 512, seed0=5)
    out = []
    for lanes in (0, 4):
        eng = BatchEngine(1024, lanes_per_game=lanes)
        counts, results, steps = eng.rollout_vs_expert(W2, m, pairs, 200, want_results=True)
        out.append((counts, results, steps, eng.rollout_faults(len(m)), eng.state_hash()))
        eng.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_bot_against_bot_is_the_expert_trace():
    """Both sides EXPERT, max_turns = the trace's length: final hash and steps of every game of trace_expert.npz that did
    not fault; no row of the counts is touched and no decision is made."""
    g = np.load(os.path.join(GOLD, "trace_expert.npz"))
    eng = BatchEngine(64)
    checked = 0
    lengths = np.diff(g["offsets"])
    for length in sorted(set(lengths.tolist())):   # one call per trace length (max_turns is per call)
        idx = np.nonzero((lengths == length) & (g["fault"] == 0))[0]
        if not len(idx):
            continue
        m = np.zeros(len(idx), dtype=MATCH_DTYPE)
        m["p1"] = m["p2"] = EXPERT
        m["seed"], m["deck"] = g["seeds"][idx], np.arange(len(idx))
        pairs = np.stack([g["deck0"][idx], g["deck1"][idx]], axis=1)
        counts, results, steps = eng.rollout_vs_expert(np.zeros((1, 10)), m, pairs, int(length), want_results=True)
        assert not counts.any() and (steps == length).all() and not eng.rollout_faults(len(idx)).any()
        last = g["hash"][g["offsets"][idx + 1] - 1]
        assert np.array_equal(eng.state_hash(), last)
        checked += len(idx)
    assert checked == 47 and eng.stats()["decisions"] == 0 and eng.stats()["lookahead_steps"] == 0
    eng.close()


def test_no_state_left_behind():
    """max_games + a small tail, twice on one handle (the persistent grid's pop counters), then a plain monsoon_rollout on
    the same handle equal to one on a fresh handle."""
    d = deck_indices("N12M")
    pairs = np.stack([d, d])[None]
    cap = 8192   # more than the resident wavefronts of the grid: the persistent form with its counters
    m = _schedule("mixed", cap + 37, seed0=9)
    eng = BatchEngine(cap)
    runs = []
    for _ in range(2):
        counts, results, steps = eng.rollout_vs_expert(W2, m, pairs, 40, want_results=True)
        runs.append((counts, results, steps, eng.rollout_faults(len(m)), eng.state_hash()))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    ref = model(W2, m, pairs, 40)
    assert np.array_equal(runs[0][1], ref[1]) and np.array_equal(runs[0][2], ref[2]) and np.array_equal(runs[0][0], ref[0])
    assert eng.n == 37 and np.array_equal(runs[0][4][runs[0][3][cap:] == 0], ref[4][cap:][ref[3][cap:] == 0])
    with pytest.raises(MonsoonError):   # the bot's row is still in place: only k_play_vs may play these games
        eng.play_rounds(1)
    plain = np.zeros(3000, dtype=MATCH_DTYPE)
    plain["p1"], plain["p2"], plain["seed"] = np.arange(3000) % 2, (np.arange(3000) + 1) % 2, np.arange(3000) + 77
    after = eng.rollout(W2, plain, pairs, 40, want_results=True) + (eng.rollout_faults(3000), eng.state_hash())
    fresh_eng = BatchEngine(cap)
    fresh = fresh_eng.rollout(W2, plain, pairs, 40, want_results=True) + (fresh_eng.rollout_faults(3000), fresh_eng.state_hash())
    for a, b in zip(after, fresh):
        assert np.array_equal(a, b)
    # ... and the vs-bot entry point plays a schedule without a bot exactly as monsoon_rollout does
    same = eng.rollout_vs_expert(W2, plain, pairs, 40, want_results=True) + (eng.rollout_faults(3000), eng.state_hash())
    for a, b in zip(same, fresh):
        assert np.array_equal(a, b)
    eng.close()
    fresh_eng.close()


def test_argument_checks():
    d = deck_indices("N12M")
    pairs = np.stack([d, d])[None]
    eng = BatchEngine(64)
    m = np.zeros(4, dtype=MATCH_DTYPE)
    m["p2"] = EXPERT
    with pytest.raises(MonsoonError):
        eng.rollout(W2, m, pairs, 10)          # monsoon_rollout keeps refusing the bot's row
    for bad in (-2, 2):
        m2 = m.copy()
        m2["p1"][1] = bad
        with pytest.raises(MonsoonError):
            eng.rollout_vs_expert(W2, m2, pairs, 10)
        m2 = m.copy()
        m2["p2"][3] = bad
        with pytest.raises(MonsoonError):
            eng.rollout_vs_expert(W2, m2, pairs, 10)
    assert eng.rollout_vs_expert(W2, m, pairs, 10)[:, 2].tolist() == [4, 0]
    assert eng.lib.monsoon_version() & 0xffff == 3
    eng.close()
