"""The multi-rank path on the device: FitnessEvaluator.evaluate_population / evaluate_vs_expert and the GA loop as ranks of a
torch.distributed job, every rank a fresh process that plays its shard through the HIP engine on device 0 (gloo: RCCL
cannot put two ranks on one device, so the nccl branch of _all_reduce_counts is not what runs here).

One job per world size (2 and 3) runs every scenario of tests/sharded_job.py and writes a file per rank; the tests
assert on those files.  The comparand is the single-process CPU replay in the parent (sharded_job.reference(): the
oracle libraries, numpy's and random.Random's own deck draws), never a device run -- except where a second device run
is the point: the GA loop alone on the device, made by rank 0 once its process group is gone.

Wall time of a clean job on an MI355X, measured with this module run alone: 2.7 s at world 2 (with the GA runs) and
3.3 s at world 3 (2.9 s a second time), nearly all of it the Python starts -- a rank's games take milliseconds.
CLEAN_JOB_SECONDS holds these figures; the launcher ends a job after five times as long (13.5 s and 16.5 s), which
leaves room for a busy shared machine, and after a job that it had to end or that lost a rank it starts no other."""
import os

import numpy as np
import pytest

import sharded_job as J

pytestmark = pytest.mark.gpu

CLEAN_JOB_SECONDS = {2: 2.7, 3: 3.3}
C = {name: k for k, name in enumerate(J.COUNTERS)}


def _job(world, tmp_path_factory):
    out_dir = tmp_path_factory.mktemp(f"hip_world{world}")
    _, ranks = J.run_job(world, "hip", out_dir, CLEAN_JOB_SECONDS[world])
    return world, str(out_dir), ranks


@pytest.fixture(scope="module")
def job2(tmp_path_factory):
    """(world, out_dir, rank files) of the one two-rank job."""
    return _job(2, tmp_path_factory)


@pytest.fixture(scope="module")
def job3(tmp_path_factory):
    return _job(3, tmp_path_factory)


@pytest.fixture(params=[2, 3])
def job(request):
    return request.getfixturevalue(f"job{request.param}")


def _sizes(ranks, key):
    return [len(g[key + ".matches"]) for g in ranks]


def test_ring_with_a_fixed_deck(job):
    """5 individuals x 6 N12M games, generation 3, shards of 12 / 18 and 6 / 12 / 12 games: the fitness on every rank is the
    CPU replay's, and the shards' rows (result, decisions, fault code), put back in schedule order, are the replay's."""
    world, _, ranks = job
    assert _sizes(ranks, "ring") == ([12, 18] if world == 2 else [6, 12, 12])
    J.check_evaluation(ranks, "ring")
    assert all(int(g["ring.counters"][C["engines"]]) == 1 and len(g["ring.drawn"]) == 0 for g in ranks)


def test_configuration_c5_decks(job):
    """deck="random109" on the same schedule.  By numpy alone every shard has games on both records; each rank drew on the
    device the decks of its own seeds -- numpy's pairs -- and no others; tier sizes, replays and faults summed over the
    ranks are those of a CPU tiered_rollout over the whole schedule; with the two tiers on two host threads and without."""
    world, _, ranks = job
    shards = J.c5_shards_by_numpy(world)
    assert shards == J.C5_SHARDS[world] and all(0 < ext < games for games, ext in shards)   # before any device result is looked at
    for key in ("c5_on", "c5_off"):
        assert _sizes(ranks, key) == [games for games, _ in shards]
        for g, (games, ext) in zip(ranks, shards):
            assert g[key + ".drawn"].tolist() == [games]
            assert g[key + ".counters"][:2].tolist() == [games - ext, ext] and int(g[key + ".counters"][C["engines"]]) >= 2
        total = J.check_evaluation(ranks, key)
        assert total[:2].tolist() == [15, 15]


def test_per_game_deck_schedule_and_the_bot(job):
    """DeckEvolutionConfig(per_game=True), an explore and a balance generation: each rank's pairs, drawn on the device for
    its own seeds only, are game_decks'; the fitness is the replay's; the bot's games (stream tag 2), 5 x 4 sharded 8 / 12
    and 4 / 8 / 8, equal tests/vs_expert_model.py in scores, raw counts and rows."""
    world, _, ranks = job
    for key in ("pg_explore", "pg_balance", "pg_vs_explore", "pg_vs_balance"):
        J.check_evaluation(ranks, key)
        assert all(g[key + ".drawn"].tolist() == [len(g[key + ".matches"])] for g in ranks), key
    assert _sizes(ranks, "pg_vs_explore") == _sizes(ranks, "pg_vs_balance") == ([8, 12] if world == 2 else [4, 8, 8])
    ref = J.reference()
    assert len(np.unique(ref["pg_balance.pairs"].reshape(-1, 24), axis=0)) > 1 and (ref["pg_vs_explore.matches"][:, :2] < 0).any()


def test_sequential_deck_schedule(job):
    """The default deck schedule: every rank draws the whole generation's 30 pairs on the host and hands its engine its
    shard's; the fitness is the replay's."""
    world, _, ranks = job
    J.check_evaluation(ranks, "seq")
    assert all(len(g["seq.drawn"]) == 0 and int(g["seq.decks_handed"]) == len(g["seq.matches"]) for g in ranks)
    assert len(np.unique(J.reference()["seq.pairs"].reshape(-1, 24), axis=0)) > 20


def test_round_robin_with_a_hall_of_fame(job):
    """4 individuals, 2 games per pairing, generations 1 and 2: 32 of the second one's 56 games are against the hall of fame
    (weight rows >= 4).  Both generations' fitness and the hall's weights equal the replay's on every rank."""
    world, _, ranks = job
    m = np.concatenate([g["hall_gen2.matches"] for g in ranks])
    assert len(m) == 56 and int((m[:, 1] >= 4).sum()) == 32
    assert _sizes(ranks, "hall_gen2") == ([28, 28] if world == 2 else [14, 14, 28])
    for key in ("hall_gen1", "hall_gen2"):
        J.check_evaluation(ranks, key)
        assert all(g[key + ".hall"].shape == (4, 10) for g in ranks)


def test_rank_without_a_game(job):
    """2 individuals over 3 ranks: rank 0 has no game, creates no engine, joins the reduce and returns the same fitness."""
    world, _, ranks = job
    J.check_evaluation(ranks, "empty")
    assert _sizes(ranks, "empty") == ([6, 6] if world == 2 else [0, 6, 6])
    assert [int(g["empty.counters"][C["engines"]]) for g in ranks] == ([1, 1] if world == 2 else [0, 1, 1])


def test_statistics_are_the_ranks_own_and_the_jobs(job):
    """total_env_steps / total_decisions stay a rank's own and add up to the CPU replay's count of the whole schedule
    (orc_rollout_schedule's look-ahead steps; the decisions of every game); get_stats' env_steps is that sum on every rank."""
    world, _, ranks = job
    ref = J.reference()
    for key in J.EVALUATIONS:
        own = np.array([g[key + ".counters"] for g in ranks])
        for name in ("total_env_steps", "total_decisions"):
            assert own[:, C[name]].sum() == ref[key + ".counters"][C[name]], (key, name, own[:, C[name]].tolist())
        assert (own[:, C["stats_env_steps"]] == ref[key + ".counters"][C["total_env_steps"]]).all(), key
        assert (own[:, C["job_decisions"]] == ref[key + ".counters"][C["total_decisions"]]).all(), key
    assert ref["ring.counters"][C["total_env_steps"]] > 10 * ref["ring.counters"][C["total_decisions"]] > 0


def test_ga_loop_on_the_device(job2):
    """EvolutionEngine as two ranks (LOCAL_RANK unset: both on device 0), host GA and ga_on_device: the populations after
    every generation are the same on both ranks and the same as those of the loop run alone on the device -- it is the
    same device, so ga_on_device too is bit for bit -- and, with the host GA, as those of the CPU replay of the whole
    run.  One writer: a log row per generation and one set of files, equal to the single run's."""
    _, out_dir, ranks = job2
    ref = J.reference()
    J.check_ga_runs([(ref, "ga_off"), (ranks[0], "single_ga_off"), (ranks[0], "ga_off"), (ranks[1], "ga_off")])
    J.check_ga_runs([(ranks[0], "single_ga_on"), (ranks[0], "ga_on"), (ranks[1], "ga_on")])
    assert len(set(ref["ga_off.fitness"].ravel().tolist())) > 2   # selection had something to go by
    J.check_ga_files(os.path.join(out_dir, "ga_off"), ref["ga_dir"])
    for key in ("ga_off", "ga_on"):
        J.check_ga_files(os.path.join(out_dir, key), os.path.join(out_dir, "single_" + key))
        own = [int(g[key + ".stats"][2]) for g in ranks]
        assert all(int(g[key + ".stats"][0]) == sum(own) == int(ranks[0]["single_" + key + ".stats"][0]) for g in ranks) and min(own) > 0
    assert int(ref["ga_off.stats"][0]) == int(ranks[0]["single_ga_off.stats"][0])
