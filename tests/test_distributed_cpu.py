"""World-size-2 gloo test of the N>1 path: the schedule is sharded by row individual, each rank
plays its shard (oracle backend on CPU), and one all_reduce sums the per-individual counters.
The sharded result must equal the single-process one."""
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from monsoon_amd.config import EvolutionaryConfig
from monsoon_amd.fitness import FitnessEvaluator
from monsoon_amd.weights import WeightVector


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _population():
    np.random.seed(11)
    return [WeightVector(10) for _ in range(4)]


def _deck_schedule():
    from monsoon_amd.cards import DECKS
    from monsoon_amd.decks import DeckEvolutionConfig
    # generation 3 is in the explore phase: a different deck pair per game, drawn from one seeded stream
    return DeckEvolutionConfig(DECKS["IRONCLAD"], DECKS["SWARM"], exploit_generations=1, explore_generations=4, seed=9)


def _worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from oracle_rollout import oracle_rollout_fn
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = EvolutionaryConfig(mu=4, lambda_=4, schedule="ring", games_per_individual=2, max_turns=10)
    ev = FitnessEvaluator(cfg, rollout_fn=oracle_rollout_fn)
    f = ev.evaluate_population(_population(), generation=3)
    np.save(os.path.join(out_dir, f"fit{rank}.npy"), np.array(f))
    # with a deck schedule every rank draws the decks of the WHOLE schedule and keeps its shard's
    ev2 = FitnessEvaluator(cfg, _deck_schedule(), rollout_fn=oracle_rollout_fn)
    f2 = ev2.evaluate_population(_population(), generation=3)
    np.save(os.path.join(out_dir, f"fitdeck{rank}.npy"), np.array(f2))
    # configuration C5's per-game random decks depend on the game's seed alone: every rank draws only the decks of its shard
    from oracle_rollout import oracle_draw_decks
    drawn = []

    def draw(seeds, pool):
        drawn.append(len(seeds))
        return oracle_draw_decks(seeds, pool)
    cfg3 = EvolutionaryConfig(mu=4, lambda_=4, schedule="ring", games_per_individual=2, max_turns=10, deck="random109")
    f3 = FitnessEvaluator(cfg3, rollout_fn=oracle_rollout_fn, deck_draw_fn=draw).evaluate_population(_population(), generation=3)
    np.save(os.path.join(out_dir, f"fitrand{rank}.npy"), np.array(f3))
    np.save(os.path.join(out_dir, f"drawn{rank}.npy"), np.array(drawn))
    dist.destroy_process_group()


def test_sharded_evaluation_matches_single_process(tmp_path):
    from oracle_rollout import oracle_rollout_fn
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    f0 = np.load(tmp_path / "fit0.npy")
    f1 = np.load(tmp_path / "fit1.npy")
    cfg = EvolutionaryConfig(mu=4, lambda_=4, schedule="ring", games_per_individual=2, max_turns=10)
    single = FitnessEvaluator(cfg, rollout_fn=oracle_rollout_fn).evaluate_population(_population(), generation=3)
    assert np.array_equal(f0, f1)
    assert np.array_equal(f0, np.array(single))
    d0 = np.load(tmp_path / "fitdeck0.npy")
    d1 = np.load(tmp_path / "fitdeck1.npy")
    single_deck = FitnessEvaluator(cfg, _deck_schedule(), rollout_fn=oracle_rollout_fn).evaluate_population(_population(), generation=3)
    assert np.array_equal(d0, d1)
    assert np.array_equal(d0, np.array(single_deck))
    from oracle_rollout import oracle_draw_decks
    cfg3 = EvolutionaryConfig(mu=4, lambda_=4, schedule="ring", games_per_individual=2, max_turns=10, deck="random109")
    single_rand = FitnessEvaluator(cfg3, rollout_fn=oracle_rollout_fn, deck_draw_fn=oracle_draw_decks).evaluate_population(_population(), generation=3)
    r0, r1 = np.load(tmp_path / "fitrand0.npy"), np.load(tmp_path / "fitrand1.npy")
    assert np.array_equal(r0, r1) and np.array_equal(r0, np.array(single_rand))
    assert np.load(tmp_path / "drawn0.npy").tolist() == [4] and np.load(tmp_path / "drawn1.npy").tolist() == [4]   # 8 games, 4 per rank


def _run_bench(args, env_extra):
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.update(env_extra)
    p = subprocess.run([sys.executable, os.path.join(repo, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p.returncode, [json.loads(ln) for ln in lines], p.stderr


def test_bench_launcher_starts_the_ranks_itself():
    """`python bench.py --gpus 2` with no rendezvous in the environment starts two ranks (torch.distributed.run, one
    process per device) and reports the rank count the all-reduce saw.  CPU ranks: gloo backend and bench.py's
    stand-in engine (MONSOON_BENCH_FAKE, a test hook) -- what is exercised is the launcher and the rank plumbing."""
    env = {"MONSOON_BENCH_FAKE": "1", "MONSOON_BENCH_BACKEND": "gloo"}
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        assert k not in os.environ
    rc, lines, err = _run_bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--games", "64", "--no-cpu"], env)
    assert rc == 0, err[-2000:]
    assert len(lines) == 1   # rank 0 only
    line = lines[0]
    assert line["n_gpus"] == 2 and line["ranks"] == {"launched": 2, "in_all_reduce": 2, "backend": "gloo"}
    assert line["steps"] == 3 and line["scaling"] == "weak"
    assert line["value"] > 0 and abs(line["lookahead_per_decision"] - 17.0) < 1e-9   # both ranks' counters were summed


def test_bench_refuses_more_gpus_than_the_machine_has():
    """On a machine with fewer GPUs than --gpus (this container has none) the bench fails loudly instead of printing a
    line with a smaller n_gpus."""
    rc, lines, err = _run_bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu"], {})
    assert rc != 0 and lines == []
    assert "refusing" in err


def test_bench_dump_outputs(tmp_path):
    """--dump-outputs DIR: after the timed steps, the last step's outputs as float64 .npy files, the same from run to run,
    at most 64 MB in all (a larger batch is cut to a fixed sample of its rows); the stand-in's state shows that exactly
    --steps steps were timed.  CPU: bench.py's stand-in engine (MONSOON_BENCH_FAKE, a test hook)."""
    env = {"MONSOON_BENCH_FAKE": "1"}
    shapes = {"state_hash": (64, 2), "status": (64, 4), "features": (64, 10), "game_faults": (64,)}
    runs = []
    for k in range(2):
        out = tmp_path / f"run{k}"
        rc, lines, err = _run_bench(["--steps", "3", "--warmup", "1", "--games", "64", "--dump-outputs", str(out)], env)
        assert rc == 0, err[-2000:]
        assert len(lines) == 1 and lines[0]["steps"] == 3 and lines[0]["ms_per_step"] > 0
        assert sorted(os.listdir(out)) == sorted(f"{n}.npy" for n in shapes)
        runs.append({n: np.load(out / f"{n}.npy") for n in shapes})
        for n, shape in shapes.items():
            assert runs[-1][n].dtype == np.float64 and runs[-1][n].shape == shape, n
    for n in shapes:
        assert np.array_equal(runs[0][n], runs[1][n]), n
    h = np.arange(64, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(8 * 3)   # the stand-in's hash after 3 steps of 8 rounds
    assert np.array_equal(runs[0]["state_hash"].astype(np.uint64), np.stack([h >> np.uint64(32), h & np.uint64(0xFFFFFFFF)], axis=1))
    out = tmp_path / "big"
    rc, lines, err = _run_bench(["--steps", "1", "--warmup", "0", "--games", "600000", "--dump-outputs", str(out)], env)
    assert rc == 0, err[-2000:]
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 << 20
    rows = np.load(out / "sample_rows.npy")
    assert len(rows) > 400000 and np.all(np.diff(rows) > 0) and rows[-1] < 600000
    assert np.load(out / "features.npy").shape == (len(rows), 10)


def test_replace_capacity_faulted_rewrites_only_the_overflowing_rows():
    """Host logic of the replay tier (monsoon_amd/fitness.py): rows with a fault code >= 16 are replaced by the replay's,
    their first attempt's contribution to the per-individual counts is taken out, everything else is untouched."""
    import numpy as np
    from monsoon_amd.fitness import MATCH_DTYPE, replace_capacity_faulted
    m = np.zeros(6, dtype=MATCH_DTYPE)
    m["p1"] = [0, 0, 1, 1, 2, 2]
    m["p2"] = [1, 2, 0, 2, 0, 1]
    results = np.array([0, -1, 1, -1, 0, -1], dtype=np.int8)      # games 1 and 3 were cut short as draws ...
    steps = np.array([50, 7, 60, 9, 70, 200], dtype=np.int32)
    faults = np.array([0, 16, 0, 22, 1, 0], dtype=np.uint8)       # ... by capacity codes; code 1 is the reference's own exception
    counts = np.zeros((3, 3), dtype=np.int64)
    for k in range(6):
        counts[m["p1"][k], 0] += results[k] == 0
        counts[m["p1"][k], 1] += results[k] == -1
        counts[m["p1"][k], 2] += 1
    seen = {}

    def replay(sub):
        seen["sub"] = sub.copy()
        c = np.zeros((3, 3), dtype=np.int64)
        r = np.array([0, 1], dtype=np.int8)                        # replayed: game 1 is a win for p1 = 0, game 3 a loss for p1 = 1
        for j in range(2):
            c[sub["p1"][j], 0] += r[j] == 0
            c[sub["p1"][j], 1] += r[j] == -1
            c[sub["p1"][j], 2] += 1
        return c, r, np.array([120, 130], dtype=np.int32), np.array([0, 16], dtype=np.uint8)

    n = replace_capacity_faulted(counts, results, steps, faults, m, replay)
    assert n == 2 and list(seen["sub"]["p2"]) == [2, 2]
    assert results.tolist() == [0, 0, 1, 1, 0, -1] and steps.tolist() == [50, 120, 60, 130, 70, 200]
    assert faults.tolist() == [0, 0, 0, 16, 1, 0]                  # what not even the replay could hold stays flagged
    assert counts.tolist() == [[2, 0, 2], [0, 0, 2], [1, 1, 2]]
    assert replace_capacity_faulted(counts, results, steps, np.zeros(6, dtype=np.uint8), m, replay) == 0


# ---- the job shapes of tests/test_sharded_gpu.py without a GPU: world 2 and 3, gloo, every rank on the CPU oracle ---------------
# A clean job takes 4 s of wall time (either world size; most of it three Python starts) where these tests were written.  The
# launcher ends a job after five times CLEAN_JOB_SECONDS, a figure three times the measured one for a slower test machine.
CLEAN_JOB_SECONDS = 12


def _job(world, tmp_path_factory):
    import sharded_job as J
    out_dir = tmp_path_factory.mktemp(f"world{world}")
    _, ranks = J.run_job(world, "oracle", out_dir, CLEAN_JOB_SECONDS)
    return world, str(out_dir), ranks


@pytest.fixture(scope="module")
def job2(tmp_path_factory):
    """(world, out_dir, rank files) of the one two-rank job, which ran every scenario of tests/sharded_job.py and the GA loop."""
    return _job(2, tmp_path_factory)


@pytest.fixture(scope="module")
def job3(tmp_path_factory):
    return _job(3, tmp_path_factory)


@pytest.fixture(params=[2, 3])
def job(request):
    return request.getfixturevalue(f"job{request.param}")


def test_every_sharded_evaluation_equals_the_single_process_replay(job):
    """Ring with a fixed deck, configuration C5's decks, both modes of a deck schedule with the bot's games, and the rest
    below, each at world 2 and 3: fitness on every rank, every rank's block of games and deck pairs, the rows put back in
    schedule order and the counters summed over the ranks equal the single process's; get_stats' env-steps are the
    job's, on every rank, while total_env_steps stays the rank's own."""
    import sharded_job as J
    world, _, ranks = job
    for key in J.EVALUATIONS:
        total = J.check_evaluation(ranks, key)
        if not key.startswith("pg_vs"):
            assert total[J.COUNTERS.index("total_env_steps")] > 1000 and max(int(g[key + ".counters"][5]) for g in ranks) < total[5]


def test_round_robin_with_a_hall_of_fame_sharded(job):
    """4 individuals, 2 games per pairing, generations 1 and 2: the second one's 56 games hold 32 against the hall of fame
    (p2 >= 4; 28 games per rank at world 2).  Both generations' fitness and the hall's weights equal the replay's."""
    import sharded_job as J
    world, _, ranks = job
    m = np.concatenate([g["hall_gen2.matches"] for g in ranks])
    assert len(m) == 56 and int((m[:, 1] >= 4).sum()) == 32 and len(np.concatenate([g["hall_gen1.matches"] for g in ranks])) == 24
    assert [len(g["hall_gen2.matches"]) for g in ranks] == ([28, 28] if world == 2 else [14, 14, 28])
    for key in ("hall_gen1", "hall_gen2"):
        J.check_evaluation(ranks, key)
        assert all(g[key + ".hall"].shape == (4, 10) for g in ranks)
    assert len(set(J.reference()["hall_gen2.fitness"].tolist())) > 1


def test_mixed_tier_schedule_counts_sharded(job):
    """Configuration C5 on the 5 x 6 ring: every rank's shard has games on both records (sizes asserted from numpy's own
    draws), each rank runs the tier ladder and _uncount on its shard, and tier sizes, replays and faults add up to the
    single process's, with the two tiers played from two host threads and one after the other."""
    import sharded_job as J
    world, _, ranks = job
    assert J.c5_shards_by_numpy(world) == J.C5_SHARDS[world]
    for key in ("c5_on", "c5_off"):
        assert [(int(g[key + ".counters"][0] + g[key + ".counters"][1]), int(g[key + ".counters"][1])) for g in ranks] == J.C5_SHARDS[world]
        total = J.check_evaluation(ranks, key)
        assert total[:2].tolist() == [15, 15]
    assert all(np.array_equal(g["c5_on.results"], g["c5_off.results"]) and np.array_equal(g["c5_on.steps"], g["c5_off.steps"]) for g in ranks)


def test_rank_without_a_game_still_joins_the_reduce(job):
    """2 individuals: at world 3 rank 0 has no game, plays none, and returns the same fitness."""
    import sharded_job as J
    world, _, ranks = job
    J.check_evaluation(ranks, "empty")
    assert [len(g["empty.matches"]) for g in ranks] == ([6, 6] if world == 2 else [0, 6, 6])


def test_ga_loop_under_two_ranks_has_one_writer(job2):
    """EvolutionEngine as two ranks sharing one results_dir: one header and one row per generation in training_log.csv
    (every column but time and throughput equal to the single process's file), one checkpoint, one final_population.pkl
    equal to the single process's, one results_summary.txt; both ranks hold the single process's populations after
    every generation and return its best_fitness, best_weights and generations."""
    import sharded_job as J
    _, out_dir, ranks = job2
    ref = J.reference()
    J.check_ga_files(os.path.join(out_dir, "ga_off"), ref["ga_dir"])
    J.check_ga_runs([(ref, "ga_off"), (ranks[0], "ga_off"), (ranks[1], "ga_off")])
    own = [int(g["ga_off.stats"][2]) for g in ranks]
    assert all(int(g["ga_off.stats"][0]) == sum(own) == int(ref["ga_off.stats"][0]) for g in ranks) and min(own) > 0
