"""GPU tests of the vector env's schedule mode (monsoon_env_set_schedule / monsoon_env_decks_dev, VecEnv.reset(deck_schedule=...),
set_deck_schedule, decks(), monsoon_amd.game.EvolutionaryGame): every episode's decks are the pair the schedule in force
when it starts draws for its seed -- the stdlib's draw, through tests/vec_env_schedule_model.py -- in lockstep with the
model of the env contract; across a generation change, inside a captured step, after a restore; on the extended build with
a real faction schedule; and the argument errors.  An explore generation that keeps some but not all of the archetype can
draw a deck that lists a card twice, which only the extended record plays as the reference does: the
standard build refuses such a schedule (tests/test_dup_decks_gpu.py), so those cases run on VecEnv(extended=1)."""
import ctypes

import numpy as np
import pytest

from monsoon_amd.cards import DECKS, deck_indices
from monsoon_amd.decks import TAG_ENV, DeckEvolutionConfig
from test_vec_env_gpu import _first_legal, assert_views_equal, host_views, random_legal
from vec_env_schedule_model import FACTIONS, ScheduleVecEnvModel, schedule_decks, standard_schedule

pytestmark = pytest.mark.gpu

N = 70           # crosses a 64-lane block of the lane-per-slot kernels
MAX_STEPS = 12   # every slot rolls through several episodes in 40 steps


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _seed0(n, salt):
    s = (np.arange(n, dtype=np.uint64) * 2654435761 + 97 * salt + 5) & 0xFFFFFFFF
    s[:3] = (0, 0xFFFFFFFF, 0xFFFFFFF0)   # episode seeds that wrap
    return s.astype(np.uint32)


def _factions(n):
    return np.tile(np.array(FACTIONS, dtype=np.uint8), (n, 1))


def _word17(env):
    return int(env.engine.debug_counters()[17])


PARITY = [("static", dict(phase=0, n_preserve=5), "expert", 0),
          ("explore-keep9", dict(phase=1, n_preserve=9), "expert", 0),   # the set path: 3 of 56+
          ("explore-keep3", dict(phase=1, n_preserve=3), "expert", 0),   # the pool path: 9 drawn
          ("balance-0.7", dict(phase=2, ratio=0.7), "expert", 0),
          ("explore-none", dict(phase=1, n_preserve=6), "none", 0),
          ("balance-second", dict(phase=2, ratio=0.7), "expert", 1)]


@pytest.mark.parametrize("name,sched,opponent,agent_side", PARITY, ids=[p[0] for p in PARITY])
def test_parity_with_the_model(name, sched, opponent, agent_side):
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    salt = [p[0] for p in PARITY].index(name)
    params = standard_schedule(generation=40 + salt, **sched)
    seed0 = _seed0(N, salt)
    ext = int(sched["phase"] == 1)   # the explore draws can repeat a card: the extended record
    env = VecEnv(N, extended=ext)
    views = env.reset(seed0, factions=_factions(N), opponent=opponent, agent_side=agent_side, max_steps=MAX_STEPS, deck_schedule=params)
    model = ScheduleVecEnvModel(seed0, params, factions=_factions(N), opponent=int(opponent == "expert"), agent_side=agent_side,
                                max_steps=MAX_STEPS, extended=bool(ext))
    assert_views_equal(host_views(views), model.views, "reset")
    assert np.array_equal(env.state_hash(), model.hashes())
    assert np.array_equal(env.decks().cpu().numpy(), model.decks)
    rs = np.random.RandomState(salt)
    ends = 0
    for t in range(40):
        a = random_legal(rs, model.views["legal"])
        got = host_views(env.step(torch.from_numpy(a).cuda()))
        want = model.step(a)
        assert_views_equal(got, want, f"{name} step {t}")   # final_hash at every done included
        assert np.array_equal(env.state_hash(), model.hashes()), t
        ends += int(got["done"].sum())
    assert np.array_equal(env.decks().cpu().numpy(), model.decks)
    assert model.episode.min() >= 2 and ends >= 2 * N, (model.episode.min(), ends)
    if sched["phase"]:
        assert len({d.tobytes() for d in model.decks}) > N // 4   # the slots do play different pairs
    assert _word17(env) == 0
    env.close()


def test_decks_follow_the_schedule_across_a_generation_change():
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    first, second = standard_schedule(1, n_preserve=4, generation=33), standard_schedule(2, ratio=0.3, generation=71)
    seed0, stride = _seed0(N, 11), 1000003
    env = VecEnv(N, extended=1)
    views = env.reset(seed0, factions=_factions(N), opponent="expert", max_steps=MAX_STEPS, seed_stride=stride, deck_schedule=first)
    model = ScheduleVecEnvModel(seed0, first, factions=_factions(N), opponent=1, max_steps=MAX_STEPS, seed_stride=stride, extended=True)
    rs = np.random.RandomState(5)
    by_old = by_new = kept = 0
    for t in range(36):
        if t == 14:   # mid-run: another generation and another phase
            before = env.decks().cpu().numpy().copy()
            env.set_deck_schedule(second["generation"], second)
            model.params = second
            assert np.array_equal(env.decks().cpu().numpy(), before)   # running episodes keep their pair
        a = random_legal(rs, model.views["legal"])
        got = host_views(env.step(torch.from_numpy(a).cuda()))
        assert_views_equal(got, model.step(a), f"step {t}")
        decks = env.decks().cpu().numpy()
        for i in range(N):   # the specification, slot by slot: the schedule current when the episode started, its seed
            k = int(got["episode"][i])
            params, seed = model.drawn[i]
            assert seed == (int(seed0[i]) + k * stride) & 0xFFFFFFFF
            assert np.array_equal(decks[i], schedule_decks(params, seed)), (t, i, k)
            if t >= 14:
                by_new += params is second and bool(got["done"][i])
                kept += params is first
            else:
                by_old += bool(got["done"][i])
    assert by_old > N and by_new > N and kept > N // 2, (by_old, by_new, kept)   # both schedules drew; slots mid-episode kept their pair
    assert all(model.drawn[i][0] is second for i in range(N))
    assert _word17(env) == 0
    env.close()


def test_real_faction_schedule_needs_and_plays_the_extended_build():
    torch = _torch()
    from monsoon_amd import MonsoonError
    from monsoon_amd.vec_env import VecEnv
    dc = DeckEvolutionConfig(DECKS["IRONCLAD"], DECKS["SWARM"], exploit_generations=2, explore_generations=6, seed=77, per_game=True)
    n = 8
    seed0 = _seed0(n, 21)
    env = VecEnv(n, extended=1)
    for generation in (6, 9):   # explore, balance
        views = env.reset(seed0, factions=_factions(n), opponent="expert", max_steps=MAX_STEPS, deck_schedule=dc, generation=generation)
        for t in range(16):
            if t:
                views = env.step(_first_legal(torch, views["legal"]))
            decks, episode = env.decks().cpu().numpy(), views["episode"].cpu().numpy()
            for i in range(n):
                d1, d2 = dc.game_decks(generation, (int(seed0[i]) + int(episode[i]) * n) & 0xFFFFFFFF, TAG_ENV)
                assert np.array_equal(decks[i], np.stack([deck_indices(d1), deck_indices(d2)])), (generation, t, i)
        assert int(views["episode"].min().item()) >= 1
    assert _word17(env) == 0
    env.close()
    std = VecEnv(n)
    with pytest.raises(MonsoonError, match="not supported by this build"):   # every faction's pool holds ua20
        std.reset(seed0, factions=_factions(n), deck_schedule=dc, generation=6)
    std.reset(seed0, factions=_factions(n), deck_schedule=dc, generation=0)    # the exploit phase reads no pool
    assert np.array_equal(std.decks().cpu().numpy(), np.tile(np.stack([deck_indices("IRONCLAD"), deck_indices("SWARM")]), (n, 1, 1)))
    std.close()


def test_captured_step_sees_the_new_schedule():
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    first, second = standard_schedule(0, generation=1), standard_schedule(1, n_preserve=2, generation=44)
    seed0 = _seed0(N, 31)
    env = VecEnv(N, extended=1)
    views = env.reset(seed0, factions=_factions(N), opponent="expert", max_steps=MAX_STEPS, deck_schedule=first)
    model = ScheduleVecEnvModel(seed0, first, factions=_factions(N), opponent=1, max_steps=MAX_STEPS, extended=True)
    s = env.stream
    actions = torch.zeros(N, dtype=torch.uint8, device="cuda")
    with torch.cuda.stream(s):   # warm-up outside the graph
        actions.copy_(_first_legal(torch, views["legal"]))
        env.step(actions)
        decks = env.decks()
    torch.cuda.synchronize()
    model.step(_first_legal(torch, torch.from_numpy(model.views["legal"])).numpy())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        actions.copy_(_first_legal(torch, views["legal"]))
        env.step(actions)
        env.decks()
    for t in range(30):
        if t == 12:
            env.set_deck_schedule(second["generation"], second)
            model.params = second
        a = _first_legal(torch, torch.from_numpy(model.views["legal"])).numpy()
        g.replay()
        torch.cuda.synchronize()
        assert_views_equal(host_views(views), model.step(a), f"replay {t}")
        assert np.array_equal(decks.cpu().numpy(), model.decks), t
    assert all(model.drawn[i][0] is second for i in range(N))   # the generation change reached the replayed graph
    assert (model.decks != first["archetype"][None]).any(axis=(1, 2)).sum() > N // 2
    assert _word17(env) == 0
    env.close()


def test_evolutionary_game_is_episode_0_of_its_slot():
    torch = _torch()
    from monsoon_amd.game import EvolutionaryGame
    from monsoon_amd.vec_env import VecEnv
    dc = DeckEvolutionConfig(DECKS["IRONCLAD"], DECKS["SWARM"], exploit_generations=2, explore_generations=6, seed=123, per_game=True)
    n = 3
    seed0 = np.array([7, 0xFFFFFFFF, 424242], dtype=np.uint32)
    facs = np.tile(np.array([dc.player1_faction, dc.player2_faction], dtype=np.uint8), (n, 1))
    for generation in (1, 5, 10):   # exploit, explore, balance
        env = VecEnv(n, extended=1)
        views = env.reset(seed0, factions=facs, deck_schedule=dc, generation=generation)   # no opponent: the caller plays both sides
        # on the env's record build, which is the one a pair that repeats a card needs anyway
        games = [EvolutionaryGame(int(s), generation, dc, extended=1) for s in seed0]
        decks = env.decks().cpu().numpy()
        live = np.ones(n, dtype=bool)
        for i, g in enumerate(games):
            assert np.array_equal(decks[i], np.stack([deck_indices(g.player1_deck), deck_indices(g.player2_deck)]))
            assert (g.player1_deck, g.player2_deck) == dc.game_decks(generation, int(seed0[i]), TAG_ENV)
            assert np.array_equal(views["obs"][i].cpu().numpy(), g.reset()) and g.to_play() == int(views["to_play"][i])
        for t in range(25):
            legal = views["legal"].cpu().numpy()
            a = np.array([np.nonzero(legal[i])[0][(3 * t + i) % int(legal[i].sum())] if live[i] and legal[i].any() else 255 if not live[i] else 155
                          for i in range(n)], dtype=np.uint8)
            for i, g in enumerate(games):
                if live[i]:
                    assert sorted(g.legal_actions()) == np.nonzero(legal[i])[0].tolist()
            views = env.step(torch.from_numpy(a).cuda())
            got = host_views(views)
            for i, g in enumerate(games):
                if not live[i]:
                    continue
                obs, reward, done = g.step(int(a[i]))
                assert reward == 10 * int(got["reward"][i]) and done == bool(got["done"][i]), (generation, t, i)
                if done:
                    live[i] = False   # the env's slot moved on to episode 1; the game's last state is hashed instead
                    assert got["fault"][i] == 0 and got["episode"][i] == 1
                else:
                    assert np.array_equal(obs, got["obs"][i]), (generation, t, i)
        for g in games:
            g.close()
        env.close()
    # left to itself the game picks the build by its decks (cards.needs_extended): generation 5 draws ua20 for seed 424242,
    # a unit or structure twice in both decks and no ua20 for seed 7, neither for seed 3
    for seed, ext, ua20, repeat in ((424242, 1, True, False), (7, 1, False, True), (3, 0, False, False)):
        g = EvolutionaryGame(seed, 5, dc)
        assert int(g.env._eng.extended) == ext and ("ua20" in g.player1_deck + g.player2_deck) == ua20
        assert any(d.count(c) > 1 and c[0] != "s" for d in (g.player1_deck, g.player2_deck) for c in d) == repeat
        assert g.get_phase_info()["phase"] == "Explore"
        g.close()
    g = EvolutionaryGame(11)   # no config: the pair Stormbound plays
    assert (g.player1_deck, g.player2_deck) == ("IRONCLAD", "SWARM") and g.legal_actions()
    g.close()


def test_restored_slot_draws_with_the_destinations_seed():
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    params = standard_schedule(1, n_preserve=5, generation=37)
    n = 6
    seed0 = _seed0(n, 41)
    env = VecEnv(n, extended=1)
    views = env.reset(seed0, factions=_factions(n), opponent="expert", max_steps=MAX_STEPS, deck_schedule=params)
    views = env.step(_first_legal(torch, views["legal"]))
    src = int(torch.nonzero((views["episode"] == 0) & (views["winner"] == -2))[0])   # a slot in the middle of episode 0
    dst = (src + 3) % n
    snap = env.snapshot(torch.tensor([src], dtype=torch.int32, device="cuda"))
    env.restore(snap, dst=torch.tensor([dst], dtype=torch.int32, device="cuda"))
    pair = schedule_decks(params, int(seed0[src]))
    decks = env.decks().cpu().numpy()
    assert np.array_equal(decks[src], pair) and np.array_equal(decks[dst], pair)   # the entry's decks, until that episode ends
    for t in range(MAX_STEPS):
        assert np.array_equal(views["obs"][src].cpu().numpy(), views["obs"][dst].cpu().numpy())
        views = env.step(_first_legal(torch, views["legal"]))
        assert bool(views["done"][src]) == bool(views["done"][dst])
        if bool(views["done"][dst]):
            break
        assert np.array_equal(env.decks().cpu().numpy()[dst], pair)
    assert bool(views["done"][dst]) and int(views["episode"][dst]) == 1 and int(views["final_hash"][src]) == int(views["final_hash"][dst])
    decks = env.decks().cpu().numpy()
    assert np.array_equal(decks[dst], schedule_decks(params, (int(seed0[dst]) + n) & 0xFFFFFFFF))   # the destination's seed, episode 1
    assert np.array_equal(decks[src], schedule_decks(params, (int(seed0[src]) + n) & 0xFFFFFFFF))
    assert not np.array_equal(decks[dst], decks[src])
    env.close()


def test_reseed_time_is_off_by_default_and_reports_the_last_step():
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    n = 64
    env = VecEnv(n)
    views = env.reset(_seed0(n, 61), factions=_factions(n), opponent="expert", max_steps=MAX_STEPS, deck_schedule=standard_schedule(2))
    views = env.step(_first_legal(torch, views["legal"]))
    assert env.engine.env_reseed_time(True) == 0.0      # nothing was timed before it was asked for
    views = env.step(_first_legal(torch, views["legal"]))
    assert 0.0 < env.engine.env_reseed_time(False) < 50.0
    env.step(_first_legal(torch, views["legal"]))
    assert env.engine.env_reseed_time(False) == 0.0
    env.close()


def test_argument_errors():
    torch = _torch()
    from monsoon_amd import MonsoonError, _lib
    from monsoon_amd.engine import BatchEngine
    from monsoon_amd.vec_env import VecEnv
    n = 4
    seed0 = _seed0(n, 51)
    pair = np.stack([deck_indices("IRONCLAD"), deck_indices("SWARM")])
    params = standard_schedule(1, n_preserve=6)
    env = VecEnv(n, extended=1)
    with pytest.raises(ValueError, match="decks and pool must be None"):
        env.reset(seed0, pair, deck_schedule=params)
    with pytest.raises(ValueError, match="decks and pool must be None"):
        env.reset(seed0, pool=np.arange(20, dtype=np.uint8), deck_schedule=params)
    with pytest.raises(ValueError, match="per_game"):
        env.reset(seed0, deck_schedule=DeckEvolutionConfig(DECKS["IRONCLAD"], DECKS["SWARM"], seed=3))
    with pytest.raises(MonsoonError, match="before reset"):
        env.decks()
    env.reset(seed0, pair)
    with pytest.raises(MonsoonError, match="deck_schedule"):
        env.set_deck_schedule(3)
    assert np.array_equal(env.decks().cpu().numpy(), np.tile(pair, (n, 1, 1)))   # decks() works in every deck mode
    env.reset(seed0, deck_schedule=params)
    lib, h = env.engine.lib, env.engine.h
    assert lib.monsoon_env_set_schedule(h, None) == _lib.ERR_STATE   # a schedule-mode env is loaded
    assert b"schedule-mode env" in lib.monsoon_last_error(h)
    for bad in (dict(tag=0), dict(phase=3), dict(phase=-1), dict(n_preserve=13), dict(pool_n=np.array([11, 60], dtype=np.int32)),
                dict(pool_n=np.array([60, 129], dtype=np.int32)), dict(archetype=np.full((2, 12), 200, dtype=np.uint8))):
        with pytest.raises(MonsoonError, match="status 1"):
            env.engine.env_set_schedule(dict(params, **bad))
    env.engine.env_set_schedule(dict(params, phase=0, pool_n=np.zeros(2, dtype=np.int32)))   # phase 0 ignores the pools
    views = env.step(_first_legal(torch, env.views["legal"]))   # the refused schedules changed nothing
    assert not bool(views["illegal"].any().item())
    env.reset(seed0, pair)                                           # a fixed-deck env: the schedule may go
    assert lib.monsoon_env_set_schedule(h, None) == _lib.OK
    cfg, v = _lib.EnvConfig(), _lib.EnvViews(**{k: t.data_ptr() for k, t in env.views.items()})
    with pytest.raises(MonsoonError, match="status 1"):              # no decks, no pool, no schedule: as before
        env.engine.env_reset(cfg, v, seed0)
    env.close()
    eng = BatchEngine(4)
    buf = torch.zeros(4 * 24, dtype=torch.uint8, device="cuda")
    assert eng.lib.monsoon_env_decks_dev(eng.h, ctypes.c_void_p(buf.data_ptr())) == _lib.ERR_STATE   # no env
    eng.close()
