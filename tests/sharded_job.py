"""Jobs of several torch.distributed ranks, for tests/test_distributed_cpu.py (backend "oracle": every rank plays on the
CPU oracle) and tests/test_sharded_gpu.py (backend "hip": every rank plays on device 0): the scenarios, what a rank
writes down, the launcher, and the comparand -- the single-process CPU replay in the parent (backend "replay").
Test infrastructure only.

A job runs every scenario of its world size in one process group (gloo); each rank writes what it observed to
<out_dir>/rank<k>.npz and the tests assert on those files.  The launcher ends a job that overruns its deadline or loses
a rank, and after such a job starts no other in the session."""
import datetime
import os
import socket
import time

import numpy as np

from monsoon_amd.config import EvolutionaryConfig
from monsoon_amd.fitness import DEPTH_CODE, MATCH_DTYPE, FitnessEvaluator, record_limited, tiered_rollout
from monsoon_amd.weights import WeightVector

MAX_TURNS, CAPACITY = 60, 256
C5_SHARDS = {2: [(12, 9), (18, 6)], 3: [(6, 3), (12, 7), (12, 5)]}   # (games, of them on the extended record) of the 5 x 6 ring, generation 3
COUNTERS = ("tier_standard", "tier_extended", "capacity_replays", "capacity_faults", "depth_faults", "total_env_steps", "total_decisions",
            "job_env_steps", "job_decisions", "stats_env_steps", "total_games", "engines")
SUMMED = COUNTERS[:7]   # a rank's own: they add up to the single process's over the ranks


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def population(n, seed=11):
    np.random.seed(seed)
    return [WeightVector(10) for _ in range(n)]


def ring_config(n=5, games=6, **kw):
    return EvolutionaryConfig(mu=n, lambda_=n, schedule="ring", games_per_individual=games, max_turns=MAX_TURNS, max_concurrent_games=CAPACITY, **kw)


def deck_schedule(per_game):
    """Generation 3 is in the explore phase, generation 6 in the balance phase."""
    from monsoon_amd.cards import DECKS
    from monsoon_amd.decks import DeckEvolutionConfig
    return DeckEvolutionConfig(DECKS["IRONCLAD"], DECKS["SWARM"], exploit_generations=1, explore_generations=4, seed=5, per_game=per_game)


def shard_bounds(n, world):
    return [((n * r) // world, (n * (r + 1)) // world) for r in range(world)]


def _with_bot(matches):
    return bool(((matches["p1"] < 0) | (matches["p2"] < 0)).any())


class CpuRollout:
    """fitness._hip_rollout on the CPU, bookkeeping included: tiered_rollout over oracle_rollout_tier (over the model of
    tests/vs_expert_model.py where the bot plays), so that the ladder and _uncount run, and the counters _hip_rollout
    keeps.  The env-steps and decisions go to the evaluator bound as .ev, as _hip_rollout's go to its own."""

    def __init__(self, concurrent=False):
        self.concurrent = concurrent
        self.ev = None
        self.tier_games, self.capacity_replays, self.capacity_faults, self.depth_faults = [0, 0], 0, 0, 0
        self.total_env_steps = self.total_decisions = 0
        self.last_rollout = None

    def __call__(self, weights, matches, deck_pairs, max_turns):
        import threading
        import vs_expert_model
        from oracle_rollout import oracle_rollout_tier
        matches = np.asarray(matches)
        bot = _with_bot(matches)
        lock = threading.Lock()
        to = self.ev if self.ev is not None else self

        def play(tier, sub, sub_pairs):
            if bot:
                c, r, s, f = vs_expert_model.rollout_tier(weights, sub, sub_pairs, max_turns, tier)[:4]
                look = 0
            else:
                c, r, s, f, look = oracle_rollout_tier(weights, sub, sub_pairs, max_turns, tier, want_lookahead=True)
            with lock:
                to.total_env_steps += look
                to.total_decisions += int(s.sum())
            return c, r, s, f
        counts, results, steps, faults, replays, sizes = tiered_rollout(play, len(weights), matches, deck_pairs, concurrent=self.concurrent)
        self.capacity_replays += replays
        self.capacity_faults += int(record_limited(faults).sum())
        self.depth_faults += int((faults == DEPTH_CODE).sum())
        self.tier_games = [a + b for a, b in zip(self.tier_games, sizes)]
        self.last_rollout = (results, steps, faults)
        return counts


class Probe:
    """One FitnessEvaluator of a backend, and a record of every rollout it was asked for:
    "hip"     FitnessEvaluator(cfg, deck_config, device=0): the code under test, nothing replaced (its _hip_rollout and
              the engine's two deck draws are wrapped to be written down);
    "oracle"  rollout_fn = CpuRollout: the ranks of the CPU tests;
    "replay"  the comparand: rollout_fn = oracle_rollout_fn / vs_expert_rollout_fn for counts and per-game rows, decks by
              numpy and DeckEvolutionConfig.game_decks (FitnessEvaluator's own host draws), a CpuRollout beside it for
              the counters."""

    def __init__(self, backend, cfg, deck_config=None):
        self.backend, self.calls = backend, []
        if backend == "hip":
            self.ev = self.src = FitnessEvaluator(cfg, deck_config, device=0)
            inner = self.ev._hip_rollout
        else:
            self.src = CpuRollout(cfg.concurrent_tiers)
            inner = self.src if backend == "oracle" else self._replay
            self.ev = self.src.ev = FitnessEvaluator(cfg, deck_config, rollout_fn=self._spy)
        self._inner = inner
        if backend == "hip":
            self.ev._hip_rollout = self._spy

    def _replay(self, weights, matches, deck_pairs, max_turns):
        import vs_expert_model
        from oracle_rollout import oracle_rollout_fn
        fn = vs_expert_model.vs_expert_rollout_fn if _with_bot(np.asarray(matches)) else oracle_rollout_fn
        counts, results, steps, faults = fn(weights, matches, deck_pairs, max_turns, want_results=True, want_faults=True)
        self.src(weights, matches, deck_pairs, max_turns)
        self.src.last_rollout = (results, steps, faults)
        return counts

    def _spy(self, weights, matches, deck_pairs, max_turns):
        counts = self._inner(weights, matches, deck_pairs, max_turns)
        self.calls.append((np.array(matches), np.array(deck_pairs, dtype=np.uint8).reshape(-1, 2, 12)) + tuple(np.array(x) for x in self.src.last_rollout))
        return counts

    def record(self, out, key, fitness):
        """What the last evaluate_* call did, under out[key + ".<field>"] (the counters run on over an evaluator's calls)."""
        ev, src = self.ev, self.src
        calls, self.calls = self.calls, []
        assert len(calls) <= 1, "one rollout per evaluation"
        if calls:
            m, d, results, steps, faults = calls[0]
        else:   # this rank had no game
            m, d = np.zeros(0, dtype=MATCH_DTYPE), np.zeros((0, 2, 12), dtype=np.uint8)
            results, steps, faults = np.zeros(0, dtype=np.int8), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8)
        out[key + ".fitness"] = np.asarray(fitness, dtype=np.float64)
        out[key + ".matches"] = np.stack([m["p1"], m["p2"], m["seed"]], axis=1).astype(np.int64)
        out[key + ".pairs"] = d[m["deck"]]              # the deck pair of every game played
        out[key + ".decks_handed"] = np.array(len(d))   # ... and the size of the table they came in
        out[key + ".results"], out[key + ".steps"], out[key + ".faults"] = results, steps, faults
        out[key + ".hall"] = np.stack([h.weights for h in ev.hall_of_fame]) if ev.hall_of_fame else np.zeros((0, 10))
        out[key + ".counters"] = np.array(list(src.tier_games) + [src.capacity_replays, src.capacity_faults, src.depth_faults, ev.total_env_steps,
                                          ev.total_decisions, ev.job_env_steps, ev.job_decisions, ev.get_stats()["env_steps"], ev.total_games,
                                          sum(e is not None for e in ev._engines.values())], dtype=np.int64)
        out[key + ".drawn"] = np.array(_DRAWN, dtype=np.int64)   # "hip": the sizes of the device draws of this call
        del _DRAWN[:]
        if hasattr(ev, "last_vs_expert"):
            out[key + ".vs_counts"] = np.asarray(ev.last_vs_expert)

    def close(self):
        for eng in self.ev._engines.values():
            if eng is not None:
                eng.close()


_DRAWN = []


def _watch_device_draws():
    """Write down the size of every monsoon_draw_decks / monsoon_draw_schedule call of this process."""
    from monsoon_amd.engine import BatchEngine
    if getattr(BatchEngine, "_watched", False):
        return
    for name, arg in (("draw_decks", 0), ("draw_schedule", 1)):
        def wrap(inner, arg):
            def fn(self, *a):
                _DRAWN.append(len(a[arg]))
                return inner(self, *a)
            return fn
        setattr(BatchEngine, name, wrap(getattr(BatchEngine, name), arg))
    BatchEngine._watched = True


# ---- scenarios: each one for every backend ---------------------------------------------------------------------------
def scn_ring(backend, out):
    """Ring, fixed deck: 5 individuals x 6 games, generation 3, N12M."""
    p = Probe(backend, ring_config())
    p.record(out, "ring", p.ev.evaluate_population(population(5), 3))
    p.close()


def scn_c5(backend, out):
    """Configuration C5's per-game decks on the same schedule: both records on every rank, the two tiers from two host
    threads and one after the other."""
    for tag, concurrent in (("c5_on", True), ("c5_off", False)):
        p = Probe(backend, ring_config(deck="random109", concurrent_tiers=concurrent))
        p.record(out, tag, p.ev.evaluate_population(population(5), 3))
        p.close()


def scn_per_game(backend, out):
    """A per_game=True deck schedule: an explore and a balance generation, then the bot's games (stream tag 2) on both."""
    p = Probe(backend, ring_config(), deck_schedule(per_game=True))
    pop = population(5)
    p.record(out, "pg_explore", p.ev.evaluate_population(pop, 3))
    p.record(out, "pg_balance", p.ev.evaluate_population(pop, 6))
    p.record(out, "pg_vs_explore", p.ev.evaluate_vs_expert(pop, generation=3, games_per_individual=4))
    p.record(out, "pg_vs_balance", p.ev.evaluate_vs_expert(pop, generation=6, games_per_individual=4))
    p.close()


def scn_sequential(backend, out):
    """The default deck schedule: one stream for the whole generation, drawn by every rank."""
    p = Probe(backend, ring_config(), deck_schedule(per_game=False))
    p.record(out, "seq", p.ev.evaluate_population(population(5), 3))
    p.close()


def scn_hall(backend, out):
    """Round robin over two generations: the second one's opponents include the hall of fame (p2 >= 4)."""
    p = Probe(backend, EvolutionaryConfig(mu=4, lambda_=4, games_per_pairing=2, max_turns=MAX_TURNS, max_concurrent_games=CAPACITY))
    pop = population(4)
    p.record(out, "hall_gen1", p.ev.evaluate_population(pop, 1))
    p.record(out, "hall_gen2", p.ev.evaluate_population(pop, 2))
    p.close()


def scn_empty(backend, out):
    """2 individuals: of 3 ranks, rank 0 has no game."""
    p = Probe(backend, ring_config(n=2))
    p.record(out, "empty", p.ev.evaluate_population(population(2), 3))
    p.close()


SCENARIOS = (scn_ring, scn_c5, scn_per_game, scn_sequential, scn_hall, scn_empty)
EVALUATIONS = ("ring", "c5_on", "c5_off", "pg_explore", "pg_balance", "pg_vs_explore", "pg_vs_balance", "seq", "hall_gen1", "hall_gen2", "empty")
INDIVIDUALS = {"hall_gen1": 4, "hall_gen2": 4, "empty": 2}   # 5 otherwise
GA_GENERATIONS = 3


def run_ga(backend, results_dir, on_device, out, key):
    """EvolutionEngine: mu = lambda = 4, ring with 4 games each, 3 generations, a checkpoint after the second; the Swarm deck
    S12, on which games get decided within 60 decisions, so that selection depends on the fitness.  Writes down the
    population after every generation and what run() returns."""
    from monsoon_amd.evolution import EvolutionEngine
    cfg = EvolutionaryConfig(mu=4, lambda_=4, generations=GA_GENERATIONS, schedule="ring", games_per_individual=4, max_turns=MAX_TURNS, deck="S12",
                             max_concurrent_games=CAPACITY, results_dir=results_dir, checkpoint_interval=2, seed=5, ga_on_device=on_device)
    eng = EvolutionEngine(cfg, rollout_fn=None if backend == "hip" else CpuRollout())
    snaps, log = [], eng._log_generation

    def spy(generation_time, vs_expert=None):
        pop = eng.population
        snaps.append((np.stack([i.weights for i in pop.individuals]), np.stack([i.sigmas for i in pop.individuals]), np.array(pop.fitness_scores)))
        return log(generation_time, vs_expert)
    eng._log_generation = spy
    eng.initialize()
    if backend != "hip":
        eng._rollout_fn.ev = eng.fitness_evaluator
    res = eng.run()
    out[key + ".weights"], out[key + ".sigmas"], out[key + ".fitness"] = (np.stack([s[k] for s in snaps]) for k in range(3))
    out[key + ".best_fitness"], out[key + ".best_weights"] = np.array(res["best_fitness"]), np.array(res["best_weights"])
    out[key + ".generations"] = np.array(res["generations"])
    out[key + ".stats"] = np.array([res["evaluation_stats"]["env_steps"], res["evaluation_stats"]["total_games"], eng.fitness_evaluator.total_env_steps])
    for e in eng.fitness_evaluator._engines.values():
        if e is not None:
            e.close()


def worker(rank, world, port, out_dir, backend, timeout_s):
    """One rank (a fresh process): every scenario, at world 2 the GA loop too, then -- rank 0 of a "hip" job, once the
    process group is gone and this is a single process again -- the same GA runs alone on the device."""
    import torch.distributed as dist
    os.environ.pop("LOCAL_RANK", None)   # EvolutionEngine's evaluator then takes device 0
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=timeout_s))
    if backend == "hip":
        _watch_device_draws()
    out = {}
    for scn in SCENARIOS:
        scn(backend, out)
    modes = (("ga_off", False), ("ga_on", True)) if backend == "hip" else (("ga_off", False),)
    if world == 2:
        for key, on_device in modes:
            run_ga(backend, os.path.join(out_dir, key), on_device, out, key)
    dist.barrier()
    dist.destroy_process_group()
    if world == 2 and rank == 0 and backend == "hip":
        assert FitnessEvaluator._dist() is None
        for key, on_device in modes:
            run_ga(backend, os.path.join(out_dir, "single_" + key), on_device, out, "single_" + key)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **out)


# ---- the launcher ----------------------------------------------------------------------------------------------------
_BROKEN = []   # why a job of this session was ended: nothing more is started after it


def run_job(world, backend, out_dir, clean_seconds):
    """Start `world` ranks (spawn: fresh processes) and join them against a deadline of five times a clean job's wall time
    (clean_seconds, measured: the room is for a busy shared machine).  A deadline or a rank that ends badly ends the
    others, raises, and bars every later job of the session.  Returns (wall seconds, [rank files' contents])."""
    import torch.multiprocessing as mp
    if _BROKEN:
        raise RuntimeError(f"not started, an earlier job of this session was ended: {_BROKEN[0]}")
    deadline = 5.0 * clean_seconds
    t0 = time.monotonic()
    ctx = mp.spawn(worker, args=(world, free_port(), str(out_dir), backend, deadline), nprocs=world, join=False)
    try:
        while not ctx.join(timeout=1.0):   # raises if a rank ended badly (and ends the others)
            if time.monotonic() - t0 > deadline:
                raise TimeoutError(f"world-{world} {backend} job still running after {deadline:.0f} s (5 x {clean_seconds} s)")
    except BaseException as e:
        _BROKEN.append(f"world {world}, {backend}: {type(e).__name__}: {str(e)[:300]}")
        for p in ctx.processes:
            if p.is_alive():
                p.terminate()
        for p in ctx.processes:
            p.join(10)
            if p.is_alive():
                p.kill()
        raise
    wall = time.monotonic() - t0
    print(f"world-{world} {backend} job: {wall:.1f} s wall, deadline {deadline:.0f} s")
    ranks = []
    for r in range(world):
        with np.load(os.path.join(str(out_dir), f"rank{r}.npz")) as z:
            ranks.append({k: z[k] for k in z.files})
    return wall, ranks


# ---- the comparand ---------------------------------------------------------------------------------------------------
_REFERENCE = {}


def reference():
    """The single-process CPU replay of every scenario and of the GA run (its files under reference()["ga_dir"]): computed
    once per session, shared by every test, never written to."""
    if not _REFERENCE:
        import atexit
        import shutil
        import tempfile
        out = {}
        for scn in SCENARIOS:
            scn("replay", out)
        d = tempfile.mkdtemp(prefix="monsoon_ga_single_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        run_ga("oracle", d, False, out, "ga_off")
        for v in out.values():
            v.setflags(write=False)
        out["ga_dir"] = d
        _REFERENCE.update(out)
    return _REFERENCE


def c5_shards_by_numpy(world):
    """[(games, games on the extended record)] per rank of the C5 scenario, from numpy's own draws alone."""
    from monsoon_amd.cards import C5_STREAM_XOR, draw_random_decks_numpy, needs_extended_each
    from monsoon_amd.fitness import ring_schedule
    m = ring_schedule(5, 6, 3)
    ext = needs_extended_each(draw_random_decks_numpy(m["seed"] ^ np.uint32(C5_STREAM_XOR)))
    return [(int(((m["p1"] >= lo) & (m["p1"] < hi)).sum()), int(ext[(m["p1"] >= lo) & (m["p1"] < hi)].sum())) for lo, hi in shard_bounds(5, world)]


# ---- checks shared by the CPU and the GPU tests ----------------------------------------------------------------------
def _rows(matches):
    return np.where(matches[:, 0] >= 0, matches[:, 0], matches[:, 1])


def check_evaluation(ranks, key):
    """One evaluate_* call of a job against the replay: fitness (and the hall of fame, and the bot's counts) on every
    rank; every rank played exactly its block of row individuals, in schedule order, with the replay's deck pairs handed
    over in a table of no other pairs (fixed deck: a table of one); the shards' rows put back in order are the replay's;
    the ranks' own counters add up to the single process's and the job-wide ones hold that sum on every rank."""
    ref = reference()
    world = len(ranks)
    n = INDIVIDUALS.get(key, 5)
    want = ref[key + ".matches"]
    at = 0
    for r, ((lo, hi), got) in enumerate(zip(shard_bounds(n, world), ranks)):
        assert np.array_equal(got[key + ".fitness"], ref[key + ".fitness"]), (key, r, got[key + ".fitness"], ref[key + ".fitness"])
        assert np.array_equal(got[key + ".hall"], ref[key + ".hall"]), (key, r)
        if key + ".vs_counts" in ref:
            assert np.array_equal(got[key + ".vs_counts"], ref[key + ".vs_counts"]), (key, r)
        size = int(((_rows(want) >= lo) & (_rows(want) < hi)).sum())
        m = got[key + ".matches"]
        assert np.array_equal(m, want[at:at + size]), (key, r, len(m), size)
        assert np.array_equal(got[key + ".pairs"], ref[key + ".pairs"][at:at + size]), (key, r)
        table = int(ref[key + ".decks_handed"])
        assert int(got[key + ".decks_handed"]) == (0 if size == 0 else 1 if table == 1 else size), (key, r)
        for f in ("results", "steps", "faults"):
            assert np.array_equal(got[f"{key}.{f}"], ref[f"{key}.{f}"][at:at + size]), (key, r, f, got[f"{key}.{f}"], ref[f"{key}.{f}"][at:at + size])
        at += size
    assert at == len(want)
    total = sum(g[key + ".counters"] for g in ranks)
    for k, name in enumerate(COUNTERS):
        if name in SUMMED:
            assert total[k] == ref[key + ".counters"][k], (key, name, [int(g[key + ".counters"][k]) for g in ranks], int(ref[key + ".counters"][k]))
    c = {name: k for k, name in enumerate(COUNTERS)}
    for r, g in enumerate(ranks):
        mine = g[key + ".counters"]
        assert mine[c["job_env_steps"]] == mine[c["stats_env_steps"]] == total[c["total_env_steps"]], (key, r)
        assert mine[c["job_decisions"]] == total[c["total_decisions"]], (key, r)
        assert mine[c["total_games"]] == ref[key + ".counters"][c["total_games"]], (key, r)
    return total


def check_ga_files(results_dir, single_dir=None):
    """One writer: a header and one row per generation in training_log.csv, one checkpoint (after generation 2), one
    final_population.pkl that loads, one results_summary.txt.  With single_dir (a single-process run's files) every log
    column but time and the two throughputs, the final population and the summary equal that run's."""
    import pickle

    def load(d):
        with open(os.path.join(d, "training_log.csv")) as f:
            rows = [ln.rstrip("\n").split(",") for ln in f]
        with open(os.path.join(d, "final_population.pkl"), "rb") as f:   # written by the run under test a moment ago
            final = pickle.load(f)
        with open(os.path.join(d, "results_summary.txt")) as f:
            return rows, final, f.read()
    rows, final, summary = load(results_dir)
    assert rows[0][0] == "generation" and [r[0] for r in rows[1:]] == [str(g) for g in range(1, GA_GENERATIONS + 1)], rows
    names = sorted(os.listdir(results_dir))
    assert len(names) == 4 and [n.startswith("checkpoint_gen2_") for n in names] == [True, False, False, False], names
    assert final["generation"] == GA_GENERATIONS and len(final["individuals"]) == 4
    if single_dir is not None:
        rows1, final1, summary1 = load(single_dir)
        keep = [k for k, name in enumerate(rows[0]) if name not in ("time", "games_per_sec", "env_steps_per_sec")]
        assert len(keep) == len(rows[0]) - 3 and [[r[k] for k in keep] for r in rows] == [[r[k] for k in keep] for r in rows1], (rows, rows1)
        assert final["fitness_scores"] == final1["fitness_scores"]
        for a, b in zip(final["individuals"], final1["individuals"]):
            assert np.array_equal(a.weights, b.weights) and np.array_equal(a.sigmas, b.sigmas)
        assert summary == summary1
    return rows


def check_ga_runs(runs):
    """Every run (dicts of a rank file or the reference, with the key prefix to look under) holds the same populations
    after every generation, bit for bit, and returned the same best individual and generation count."""
    (first, key0) = runs[0]
    assert first[key0 + ".weights"].shape == (GA_GENERATIONS, 4, 10)
    for got, key in runs[1:]:
        for f in ("weights", "sigmas", "fitness", "best_fitness", "best_weights", "generations"):
            assert np.array_equal(got[f"{key}.{f}"], first[f"{key0}.{f}"]), (key, f, got[f"{key}.{f}"], first[f"{key0}.{f}"])
