"""Rollouts against the scripted bot, CPU side: the model of the contract (tests/vs_expert_model.py) against the reference's
own games, and the host logic (schedule, evaluate_vs_expert, count bookkeeping, sharding) over that model."""
import os
import socket

import numpy as np
import pytest

import oracle_lib
import vs_expert_model as M
from monsoon_amd.config import EvolutionaryConfig
from monsoon_amd.fitness import (EXPERT, MATCH_DTYPE, FitnessEvaluator, expert_schedule, match_rows, replace_capacity_faulted,
                                 ring_schedule, shard_by_individual, tiered_rollout)
from monsoon_amd.weights import WeightVector

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fixture():
    return np.load(os.path.join(GOLD, "trace_vs_expert.npz"))


@pytest.mark.parametrize("core", ["oracle", "product"])
def test_model_reproduces_the_reference(core):
    """trace_vs_expert.npz is the contract's loop played by the reference itself (HeuristicAgent against
    Stormbound.expert_action; scripts/gen_golden_vs_expert.py).  The model over either rules core reproduces every action,
    committed-state hash, score-vector hash, result, fault and step count of all 40 games.

    The fixture cannot hide a failure: it must hold a game won by the agent, one won by the bot and one ended by
    max_turns, the bot must commit at least 30 % of all steps, and no game is skipped.  Three of the eight pool games end
    on an exception of the reference (seeds 900, 901, 905: a committed step that raises); none of them is a raising
    expert_action -- these inputs produce none, and no other fixture holds one either (trace_expert.npz, next test), so
    that rule rests on the oracle's expert_action fault as the vector env's does.  The state behind a step that raised is
    not compared (the reference leaves a half-made move behind)."""
    g = _fixture()
    n = len(g["seeds"])
    assert n == 40 and int(g["max_turns"]) == 200
    orc = oracle_lib.Oracle(1, core=core)
    w = g["w0"][None]
    agent_won = bot_won = capped = bot_steps = all_steps = 0
    for k in range(n):
        bot = int(g["bot_side"][k])
        rows = (0, EXPERT) if bot == 1 else (EXPERT, 0)
        r = M.play(orc, 0, int(g["seeds"][k]), g["deck0"][k], g["deck1"][k], rows, w, 200, trace=True)
        lo, hi = int(g["offsets"][k]), int(g["offsets"][k + 1])
        slo, shi = int(g["soffsets"][k]), int(g["soffsets"][k + 1])
        assert r["actions"] == g["action"][lo:hi].tolist(), k
        assert r["bots"] == g["bot"][lo:hi].tolist(), k
        assert r["hashes"] == [int(x) for x in g["hash"][lo:hi]], k
        assert r["shashes"] == [int(x) for x in g["shash"][slo:shi]], k
        assert (r["result"], r["steps"], int(r["fault"] != 0)) == (int(g["result"][k]), int(g["steps"][k]), int(g["fault"][k])), k
        assert r["decisions"] == shi - slo
        if not g["fault"][k]:
            assert r["final"] == int(g["final"][k]), k
        agent_won += int(g["result"][k]) == 1 - bot
        bot_won += int(g["result"][k]) == bot
        capped += (not g["fault"][k]) and (not g["winner"][k]) and int(g["steps"][k]) == 200
        bot_steps += int(g["bot"][lo:hi].sum())
        all_steps += hi - lo
    assert agent_won >= 1 and bot_won >= 1 and capped >= 1, (agent_won, bot_won, capped)
    assert bot_steps >= 0.3 * all_steps, (bot_steps, all_steps)


def test_bot_against_bot_is_the_expert_trace():
    """Both rows EXPERT, max_turns = the trace's length: the model's bot side reproduces every game of trace_expert.npz, a
    fixture that predates it -- actions and hashes of the games that did not fault (47 of 48; the other one ends on a step
    that raises); a game in which the reference's bot itself raised (action 255) would have to raise at that step and
    without a step, but the fixture holds none."""
    g = np.load(os.path.join(GOLD, "trace_expert.npz"))
    orc = oracle_lib.Oracle(1)
    clean = raised = 0
    for k in range(len(g["seeds"])):
        lo, hi = int(g["offsets"][k]), int(g["offsets"][k + 1])
        r = M.play(orc, 0, int(g["seeds"][k]), g["deck0"][k], g["deck1"][k], (EXPERT, EXPERT), np.zeros((1, 10)), hi - lo, trace=True)
        assert r["decisions"] == 0 and r["lookahead"] == 0
        if not g["fault"][k]:
            assert r["actions"] == g["action"][lo:hi].tolist() and r["hashes"] == [int(x) for x in g["hash"][lo:hi]], k
            assert r["steps"] == hi - lo and r["fault"] == 0
            clean += 1
        elif g["action"][hi - 1] == 255:
            assert r["bot_raised"] and r["actions"] == g["action"][lo:hi].tolist() and r["steps"] == hi - lo - 1 and r["result"] == -1, k
            assert r["hashes"][:-1] == [int(x) for x in g["hash"][lo:hi - 1]], k
            raised += 1
    assert clean >= 30, (clean, raised)


def test_expert_schedule():
    m = expert_schedule(3, 4, generation=5)
    assert m.dtype == MATCH_DTYPE and len(m) == 12
    assert m["p1"].tolist() == [0, -1, 0, -1, 1, -1, 1, -1, 2, -1, 2, -1]
    assert m["p2"].tolist() == [-1, 0, -1, 0, -1, 1, -1, 1, -1, 2, -1, 2]
    assert match_rows(m).tolist() == [0] * 4 + [1] * 4 + [2] * 4
    first, second = expert_schedule(3, 4, 5, sides="first"), expert_schedule(3, 4, 5, sides="second")
    assert (first["p2"] == EXPERT).all() and (first["p1"] >= 0).all() and (second["p1"] == EXPERT).all() and (second["p2"] >= 0).all()
    assert np.array_equal(first["seed"], m["seed"]) and np.array_equal(second["seed"], m["seed"])
    ring = ring_schedule(3, 4, 5)
    assert len(set(m["seed"].tolist())) == 12 and not set(m["seed"].tolist()) & set(ring["seed"].tolist())
    assert not set(m["seed"].tolist()) & set(expert_schedule(3, 4, 6)["seed"].tolist())
    with pytest.raises(ValueError):
        expert_schedule(3, 4, 5, sides="left")
    # sharding goes by the match's individual, whichever side it plays
    parts = [shard_by_individual(m, 3, r, 2) for r in range(2)]
    assert sum(len(p) for p in parts) == 12 and match_rows(parts[0]).tolist() == [0] * 4 and match_rows(parts[1]).tolist() == [1] * 4 + [2] * 4


def _population(n=4):
    np.random.seed(11)
    return [WeightVector(10) for _ in range(n)]


def _config(**kw):
    return EvolutionaryConfig(mu=4, lambda_=4, schedule="ring", games_per_individual=2, max_turns=30, **kw)


def test_evaluate_vs_expert_is_the_model_game_by_game():
    """4 individuals x 6 games, sides alternating: scores and raw counts equal the model played game by game, and the
    counts land on the individual's row whichever side it plays."""
    pop = _population()
    ev = FitnessEvaluator(_config(), rollout_fn=M.vs_expert_rollout_fn)
    scores = ev.evaluate_vs_expert(pop, generation=2, games_per_individual=6)
    from monsoon_amd.cards import deck_indices
    deck = deck_indices("N12M")
    w = np.stack([p.weights for p in pop])
    sched = expert_schedule(4, 6, 2)
    orc = oracle_lib.Oracle(1)
    counts = np.zeros((4, 3), dtype=np.int64)
    per_side = {0: 0, 1: 0}
    for m in sched:
        r = M.play(orc, 0, int(m["seed"]), deck, deck, (int(m["p1"]), int(m["p2"])), w, 30)
        row, win = M.individual(int(m["p1"]), int(m["p2"]))
        counts[row] += (r["result"] == win, r["result"] == -1, 1)
        per_side[win] += 1
    assert per_side == {0: 12, 1: 12}
    assert np.array_equal(ev.last_vs_expert, counts) and (counts[:, 2] == 6).all()
    assert scores == [float((c[0] + 0.5 * c[1]) / 6) for c in counts]
    assert ev.evaluate_vs_expert(pop, 2, games_per_individual=6, sides="first") != [] and (ev.last_vs_expert[:, 2] == 6).all()


def _both(w, m, d, t):
    """A rollout_fn that serves both kinds of schedule."""
    from oracle_rollout import oracle_rollout_fn
    return (M.vs_expert_rollout_fn if (np.asarray(m)["p1"] < 0).any() or (np.asarray(m)["p2"] < 0).any() else oracle_rollout_fn)(w, m, d, t)


def _explore():
    """Generation 3 / 4 of this schedule are in its explore phase: a deck pair per game from one seeded stream."""
    from monsoon_amd.cards import DECKS
    from monsoon_amd.decks import DeckEvolutionConfig
    return DeckEvolutionConfig(DECKS["IRONCLAD"], DECKS["SWARM"], exploit_generations=1, explore_generations=6, seed=9)


def _two_generations(with_bot, deck_config, ev=None):
    """evaluate_population of generations 3 and 4, with an evaluate_vs_expert call in between or not: what the GA sees."""
    if ev is None:
        ev = FitnessEvaluator(_config(), deck_config() if deck_config else None, rollout_fn=_both)
    pop = _population()
    out = [ev.evaluate_population(pop, generation=3)]
    if with_bot:
        ev.evaluate_vs_expert(pop, generation=3, games_per_individual=2)
    out.append(ev.evaluate_population(pop, generation=4))
    return out, [h.weights.tolist() for h in ev.hall_of_fame], (ev.total_games, ev.total_env_steps, ev.total_decisions)


def test_evaluate_population_does_not_notice():
    """Hall of fame, statistics and a deck schedule's sequential stream are left alone: evaluate_population returns the
    same lists with an evaluate_vs_expert call in between as without one."""
    for deck_config in (None, _explore):
        assert _two_generations(True, deck_config) == _two_generations(False, deck_config)


def test_vs_expert_detour_changes_nothing_of_the_evaluator_or_its_config():
    """In a random phase of a sequential DeckEvolutionConfig the vs-bot games take configuration C5's per-seed decks, and
    the deck source is an argument: inside the deck_draw_fn and rollout_fn hooks the caller's config still names its own
    deck and the evaluator still holds its schedule (anything sharing the config reads it as it is), also after a hook
    that raises.  The decks are numpy's draw from seed ^ C5_STREAM_XOR, and what the GA sees is what an evaluator that
    never played the bot sees."""
    from monsoon_amd.cards import C5_STREAM_XOR, draw_random_decks_numpy
    cfg, dc = _config(), _explore()
    seen, played, boom = [], [], []

    def state():
        return cfg.deck, ev.deck_config is dc, ev.config is cfg

    def draw(pre, pool):
        seen.append((state(), np.array(pre)))
        if boom:
            raise RuntimeError(boom[0])
        return draw_random_decks_numpy(pre, pool)

    def roll(w, m, d, t):
        if (np.asarray(m)["p1"] < 0).any() or (np.asarray(m)["p2"] < 0).any():
            played.append((state(), np.array(m), np.array(d)))
            if boom:
                raise RuntimeError(boom[0])
        return _both(w, m, d, t)
    ev = FitnessEvaluator(cfg, dc, rollout_fn=roll, deck_draw_fn=draw)
    assert _two_generations(True, None, ev) == _two_generations(False, _explore)
    sched = expert_schedule(4, 2, 3)
    assert len(seen) == 1 and len(played) == 1
    assert seen[0][0] == ("N12M", True, True) and played[0][0] == ("N12M", True, True)
    assert np.array_equal(seen[0][1], sched["seed"] ^ np.uint32(C5_STREAM_XOR))
    assert np.array_equal(played[0][1]["seed"], sched["seed"]) and np.array_equal(played[0][1]["deck"], np.arange(8))
    assert np.array_equal(played[0][2], draw_random_decks_numpy(sched["seed"] ^ np.uint32(C5_STREAM_XOR)))
    for where in ("draw", "roll"):
        boom[:] = [where]
        ev = FitnessEvaluator(cfg, dc, rollout_fn=roll if where == "roll" else _both, deck_draw_fn=draw if where == "draw" else None)
        with pytest.raises(RuntimeError, match=where):
            ev.evaluate_vs_expert(_population(), generation=3, games_per_individual=2)
        assert state() == ("N12M", True, True)   # state() reads the evaluator in use


def test_record_limited_vs_bot_game_is_replayed_on_its_own_row():
    """A vs-bot game with the bot FIRST that tier 0 reports as stopped by a record limit (code 16) is played again on the
    next record and ITS INDIVIDUAL's row replaced -- indexing the bookkeeping by matches["p1"] would touch row -1."""
    w = np.stack([p.weights for p in _population()])
    from monsoon_amd.cards import deck_indices
    deck = deck_indices("N12M")
    sched = expert_schedule(4, 2, 0, sides="second")   # the bot FIRST in every game
    sched["deck"] = 0
    victim = 5
    calls = []

    def play(tier, sub, sub_pairs):
        c, r, s, f, _ = M.rollout_tier(w, sub, sub_pairs, 30, tier)
        calls.append((tier, sub["seed"].tolist()))
        if tier == 0:   # the stub: the victim ends as a draw on a limit of the standard record
            k = sub["seed"].tolist().index(int(sched["seed"][victim]))
            row = int(sub["p2"][k])
            c[row] -= (r[k] == 1, r[k] == -1, 0)
            c[row, 1] += 1
            r[k], f[k] = -1, 16
        return c, r, s, f
    counts, results, steps, faults, replays, _ = tiered_rollout(play, 4, sched, np.stack([deck, deck])[None])
    ref = M.rollout_tier(w, sched, np.stack([deck, deck])[None], 30, 0)
    assert replays == 1 and calls[1] == (1, [int(sched["seed"][victim])])
    assert np.array_equal(counts, ref[0]) and np.array_equal(results, ref[1]) and np.array_equal(steps, ref[2]) and not faults.any()
    assert (counts[:, 2] == 2).all()
    # the two-record form used by callers of the C ABI
    c0, r0, s0, f0 = play(0, sched, np.stack([deck, deck])[None])
    n = replace_capacity_faulted(c0, r0, s0, f0, sched, lambda sub: M.rollout_tier(w, sub, np.stack([deck, deck])[None], 30, 1)[:4])
    assert n == 1 and np.array_equal(c0, ref[0]) and np.array_equal(r0, ref[1])


def test_ga_driver_logs_vs_expert(tmp_path):
    """expert_eval_interval = 2: the driver evaluates the parents against the bot every second generation and logs it;
    with the default 0 the log has today's columns and the run is the same."""
    from oracle_rollout import oracle_rollout_fn
    from monsoon_amd.evolution import EvolutionEngine

    def fn(w, m, d, t):
        m = np.asarray(m)
        return (M.vs_expert_rollout_fn if ((m["p1"] < 0) | (m["p2"] < 0)).any() else oracle_rollout_fn)(w, m, d, t)

    def run(sub, **kw):
        np.random.seed(5)
        cfg = EvolutionaryConfig(mu=2, lambda_=2, generations=4, min_generations=4, schedule="ring", games_per_individual=2, max_turns=8,
                                 results_dir=str(tmp_path / sub), checkpoint_interval=100, **kw)
        eng = EvolutionEngine(cfg, rollout_fn=fn)
        eng.initialize()
        eng.run()
        with open(tmp_path / sub / "training_log.csv") as f:
            rows = [ln.rstrip("\n").split(",") for ln in f]
        return eng, rows
    plain, rows0 = run("off")
    eng, rows = run("on", expert_eval_interval=2, expert_eval_games=2)
    assert rows0[0][-1] == "env_steps_per_sec" and plain.vs_expert_log == []
    assert rows[0][-2:] == ["vs_expert_mean", "vs_expert_best"]
    assert [g for g, _, _ in eng.vs_expert_log] == [int(r[0]) for r in rows[1:] if r[-1] != ""] and len(eng.vs_expert_log) >= 1
    assert all(g % 2 == 0 and 0.0 <= mean <= best <= 1.0 for g, mean, best in eng.vs_expert_log)
    # the bot's games change nothing the GA sees
    assert [r[2:7] for r in rows0[1:]] == [r[2:7] for r in rows[1:]]
    assert [p.weights.tolist() for p in plain.population.get_parents()] == [p.weights.tolist() for p in eng.population.get_parents()]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch.distributed as dist
    import vs_expert_model
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    played = []

    def fn(w, m, d, t):
        played.append(len(m))
        return vs_expert_model.vs_expert_rollout_fn(w, m, d, t)
    ev = FitnessEvaluator(_config(), rollout_fn=fn)
    f = ev.evaluate_vs_expert(_population(), generation=3, games_per_individual=4)
    np.save(os.path.join(out_dir, f"vs{rank}.npy"), np.array(f))
    np.save(os.path.join(out_dir, f"counts{rank}.npy"), ev.last_vs_expert)
    np.save(os.path.join(out_dir, f"played{rank}.npy"), np.array(played))
    dist.destroy_process_group()


def test_sharded_vs_expert_matches_single_process(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    ev = FitnessEvaluator(_config(), rollout_fn=M.vs_expert_rollout_fn)
    single = ev.evaluate_vs_expert(_population(), generation=3, games_per_individual=4)
    for rank in range(2):
        assert np.array_equal(np.load(tmp_path / f"vs{rank}.npy"), np.array(single))
        assert np.array_equal(np.load(tmp_path / f"counts{rank}.npy"), ev.last_vs_expert)
        assert np.load(tmp_path / f"played{rank}.npy").tolist() == [8]   # 16 games, 8 per rank
