"""monsoon_draw_schedule (k_draw_schedule): the per-game decks of a deck schedule drawn on the device equal Python's own
random.Random through DeckEvolutionConfig.game_decks, on the cases of tests/deck_schedule_cases.py; argument errors;
independence of order; and Seam F end to end in the per-game mode against the CPU replay."""
import numpy as np
import pytest

import deck_schedule_cases as C
from monsoon_amd import MonsoonError
from monsoon_amd.cards import DECKS
from monsoon_amd.config import EvolutionaryConfig
from monsoon_amd.decks import DeckEvolutionConfig
from monsoon_amd.engine import BatchEngine
from monsoon_amd.fitness import FitnessEvaluator
from monsoon_amd.weights import WeightVector

pytestmark = pytest.mark.gpu

GAMES = 200   # per case


@pytest.fixture(scope="module")
def eng():
    e = BatchEngine(64)   # the draw needs no loaded games: the handle's capacity is no limit on n
    yield e
    e.close()


def _case(name):
    return next(i for i, c in enumerate(C.cases()) if c[0] == name)


def test_every_case_equals_game_decks(eng):
    for i, (name, params, _) in enumerate(C.cases()):
        seeds, want = C.expected(i, GAMES)
        got = eng.draw_schedule(params, seeds)
        bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
        assert len(bad) == 0, f"{name}: {len(bad)} of {GAMES} games differ, first at seed {int(seeds[bad[0]])}: {got[bad[0]].tolist()} != {want[bad[0]].tolist()}"


@pytest.mark.parametrize("n", [1, 65, 2000])
def test_one_game_one_more_than_a_wavefront_and_many(eng, n):
    """One workgroup per game: n = 1, n = 65 and n = 2 000 (far beyond the handle's 64 games), an explore generation that
    takes both sample paths' neighbour (6 from the pool) and a balance generation."""
    for name in ("explore-s0-keep6", "balance-s1-ratio0.7"):
        i = _case(name)
        seeds, want = C.expected(i, 2000)
        got = eng.draw_schedule(C.cases()[i][1], seeds[:n])
        assert got.shape == (n, 2, 12) and got.dtype == np.uint8
        assert np.array_equal(got, want[:n]), name


def test_argument_errors(eng):
    params = C.cases()[_case("explore-s0-keep6")][1]
    seeds = C.game_seeds(4)
    ok = eng.draw_schedule(params, seeds)
    pool11 = dict(params, pool_n=np.array([58, 11], dtype=np.int32))
    bad_pool = params["pool"].copy()
    bad_pool[1, 57] = 112   # NUM_CARDS
    bad_arch = params["archetype"].copy()
    bad_arch[0, 3] = 200
    for what, p, s in (("n = 0", params, seeds[:0]), ("pool of 11", pool11, seeds), ("card index in a pool", dict(params, pool=bad_pool), seeds),
                       ("card index in an archetype", dict(params, archetype=bad_arch), seeds), ("n_preserve 13", dict(params, n_preserve=13), seeds),
                       ("n_preserve -1", dict(params, n_preserve=-1), seeds), ("tag 0", dict(params, tag=0), seeds),
                       ("phase 0", dict(params, phase=0), seeds), ("pool of 129", dict(params, pool_n=np.array([129, 74], dtype=np.int32)), seeds)):
        try:
            eng.draw_schedule(p, s)
        except MonsoonError as e:
            assert "monsoon_draw_schedule" in str(e) and "status 1" in str(e), what
        else:
            pytest.fail(f"{what} was accepted")
    # an entry behind pool_n is no input, and a refused call leaves the handle usable
    loose = params["pool"].copy()
    loose[0, 58:] = 255
    assert np.array_equal(eng.draw_schedule(dict(params, pool=loose), seeds), ok)


def test_same_arguments_same_bytes_and_order_is_no_input(eng):
    for name in ("explore-s1-keep3", "balance-s0-ratio0.7", "synthetic-22-5"):
        i = _case(name)
        params = C.cases()[i][1]
        seeds, want = C.expected(i, GAMES)
        a = eng.draw_schedule(params, seeds)
        assert a.tobytes() == eng.draw_schedule(params, seeds).tobytes()
        assert np.array_equal(eng.draw_schedule(params, seeds[::-1].copy()), a[::-1])
        assert np.array_equal(eng.draw_schedule(params, np.repeat(seeds[:5], 3)), np.repeat(want[:5], 3, axis=0))   # nor is a neighbour
        assert eng.draw_schedule_time() > 0.0


def test_fitness_in_per_game_mode_equals_cpu_replay():
    """Seam F with a per_game=True schedule, one explore and one balance generation: the fitness of the HIP path (decks
    drawn by monsoon_draw_schedule, games on the device) equals the CPU replay's (decks by game_decks, games on the
    oracle); evaluate_vs_expert, which plays the schedule's decks under stream tag 2, likewise."""
    from oracle_rollout import oracle_rollout_fn
    import vs_expert_model as M
    from monsoon_amd.fitness import round_robin_schedule
    played = []   # (results, steps) of every call, device then CPU: at 60 turns most games are draws, their lengths still tell decks apart

    def cpu(w, m, d, t):
        m = np.asarray(m)
        counts, results, steps = (M.vs_expert_rollout_fn if ((m["p1"] < 0) | (m["p2"] < 0)).any() else oracle_rollout_fn)(w, m, d, t, want_results=True)
        played.append((results, steps))
        return counts
    np.random.seed(4)
    pop = [WeightVector(10) for _ in range(4)]
    cfg = EvolutionaryConfig(mu=4, lambda_=4, games_per_pairing=2, max_turns=60, max_concurrent_games=64)
    out, evs = [], []
    for fn in (None, cpu):
        dc = DeckEvolutionConfig(DECKS["IRONCLAD"], DECKS["SWARM"], exploit_generations=1, explore_generations=4, seed=5, per_game=True)
        ev = FitnessEvaluator(cfg, dc, rollout_fn=fn)
        res = []
        for call in (lambda: ev.evaluate_population(pop, 3), lambda: ev.evaluate_population(pop, 6),
                     lambda: ev.evaluate_vs_expert(pop, generation=3, games_per_individual=4),
                     lambda: ev.evaluate_vs_expert(pop, generation=6, games_per_individual=4)):
            res.append(call())
            if fn is None:
                played.append(ev.last_rollout[:2])
        res.append(ev.last_vs_expert.tolist())
        out.append(res)
        evs.append(ev)
    assert out[0] == out[1]
    assert len(played) == 8
    for k in range(4):
        assert np.array_equal(played[k][0], played[4 + k][0]) and np.array_equal(played[k][1], played[4 + k][1]), k
    for generation in (3, 6):   # and the decks themselves, device draw against host draw
        for tag in (1, 2):
            m = round_robin_schedule(4, 4, 2, generation)
            assert np.array_equal(evs[0]._decks_for(m.copy(), generation, tag), evs[1]._decks_for(m.copy(), generation, tag))
