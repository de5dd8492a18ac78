"""GPU tests of the vector env on handles opened with a non-default lanes_per_game.  Such a handle's hot kernel (the rollout's)
has another U than the env's own kernels: k_env_opp and k_env_after exist at the build's default variant only and serve
every handle, and all of them index the one buffer of work-stack overflow blocks (DevBuffers::wk_ovf) with their own
U * OVF_WORDS per workgroup.  The buffer is sized by the rollout launch and by monsoon_env_reset, in whatever order the
caller mixes them; it only ever grows, and a block it outgrew stays allocated, so a launch captured earlier keeps a valid
one.  Every result is compared bit for bit: the env with the Python models over the CPU oracle (they do not depend on U),
the rollouts with tests/oracle_rollout.py.

N = 37 slots (at most 64): odd, three workgroups of the extended build's lane-per-game kernels (16 slots each) and five of
the large build's (8), the last one partly filled."""
import os

import numpy as np
import pytest

from env_afterstates_model import AfterstatesModel, History, compare_slot
from kernel_variants import BUILD_NAMES, variants
from oracle_rollout import oracle_rollout_tier
from test_vec_env_gpu import assert_views_equal, host_views, mixed_decks, random_legal
from test_vec_env_heuristic_gpu import league
from test_vec_env_large_gpu import games_decks
from vec_env_heuristic_model import HeuristicVecEnvModel
from vec_env_model import VecEnvModel

pytestmark = pytest.mark.gpu

N = 37
LANES = {0: (4, 64), 1: (4, 16), 2: (4,)}   # per build: lane counts it holds other than its default's
CASES = [(ext, u) for ext in (0, 1, 2) for u in LANES[ext]]
IDS = [f"{BUILD_NAMES[ext]}-{u}" for ext, u in CASES]


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _decks(ext):
    return mixed_decks(N) if ext == 0 else games_decks(N)   # the larger records: decks with b005 / ua20


def _open(ext, u):
    from monsoon_amd.vec_env import VecEnv
    held = [x for x, _ in variants(ext)]
    assert u in held and u != held[0], (u, held)
    env = VecEnv(N, extended=ext, lanes_per_game=u)
    assert env.engine.variant()[0] == u
    return env


def _heuristic(ext, env, seed, agent_side, hist=None):
    seed0 = (np.arange(N, dtype=np.uint32) * 7919 + seed).astype(np.uint32)
    w, rows, decks = league(2), np.arange(N) % 2, _decks(ext)
    views = env.reset(seed0, decks, opponent="heuristic", agent_side=agent_side, max_steps=40, opponent_weights=w, opponent_rows=rows)
    model = HeuristicVecEnvModel(seed0, w, rows, decks=decks, agent_side=agent_side, max_steps=40, extended=ext, on_commit=hist)
    assert_views_equal(host_views(views), model.views, "reset")
    assert np.array_equal(env.state_hash(), model.hashes())
    return model


def _lockstep(torch, env, model, steps, rs, ctx):
    ends = 0
    for t in range(steps):
        a = random_legal(rs, model.views["legal"])
        got = host_views(env.step(torch.from_numpy(a).cuda()))
        assert_views_equal(got, model.step(a), f"{ctx} step {t}")
        assert np.array_equal(env.state_hash(), model.hashes()), (ctx, t)
        ends += int(got["done"].sum())
    return ends


def _compare_afterstates(env, am, slots, ctx):
    h0 = env.state_hash()
    got = host_views(env.afterstates(156))
    assert np.array_equal(env.state_hash(), h0), ctx
    entries = most = 0
    for j in slots:
        want = am.slot(j, 156)
        entries += compare_slot(want, got, j, 156, (ctx, j))
        most = max(most, want["n_legal"])
    return entries, most


@pytest.mark.parametrize("ext,u", CASES, ids=IDS)
def test_heuristic_opponent_lockstep(ext, u):
    torch = _torch()
    env = _open(ext, u)
    model = _heuristic(ext, env, 3 + u, 1)
    ends = _lockstep(torch, env, model, 30, np.random.RandomState(u), "heuristic")
    assert ends > 0 and model.episode.max() >= 1
    env.close()


@pytest.mark.parametrize("ext,u", CASES, ids=IDS)
def test_afterstates(ext, u):
    torch = _torch()
    env = _open(ext, u)
    seed0 = (np.arange(N, dtype=np.uint32) * 104729 + 5 + u).astype(np.uint32)
    decks = _decks(ext)
    env.reset(seed0, decks, opponent="expert", agent_side=0, max_steps=50)
    hist = History()
    model = VecEnvModel(seed0, decks, opponent=1, agent_side=0, max_steps=50, extended=ext, on_commit=hist)
    _lockstep(torch, env, model, 6, np.random.RandomState(u + 1), "before")
    entries, most = _compare_afterstates(env, AfterstatesModel(model, hist, extended=ext), range(N), "afterstates")
    assert entries > 0 and most > 8   # (the model's count) more legal actions than k_env_after's eight candidate lanes: a second pass
    env.close()


def _rollout(ext, env, rep):
    """n matches through the env's own BatchEngine (the handle's variant U): this launch sizes the overflow blocks for
    grid x U.  Ends env mode."""
    rs = np.random.RandomState(50 + rep)
    weights = rs.uniform(0, 1, (3, 10))
    pairs = _decks(ext)[:6]
    m = np.zeros(N, dtype=[("p1", "<i4"), ("p2", "<i4"), ("seed", "<u4"), ("deck", "<u4")])
    m["seed"] = 4000 + 100 * rep + np.arange(N)
    m["p1"], m["p2"], m["deck"] = rs.randint(0, 3, N), rs.randint(0, 3, N), np.arange(N) % len(pairs)
    counts, results, steps = env.engine.rollout(weights, m, pairs, 60, want_results=True)
    faults = env.engine.rollout_faults(N)
    oc, ores, osteps, of = oracle_rollout_tier(weights, m, pairs, 60, ext)
    assert np.array_equal(results, ores) and np.array_equal(steps, osteps) and np.array_equal(counts, oc) and np.array_equal(faults, of)
    assert (steps > 0).all()


@pytest.mark.parametrize("ext,u", CASES, ids=IDS)
def test_env_rollout_env_on_one_handle(ext, u):
    """reset -> steps and afterstates -> a rollout on the same handle -> reset with the heuristic opponent -> steps and
    afterstates -> a second rollout -> steps again: whichever call sized the overflow blocks last, every kernel finds its
    own."""
    torch = _torch()
    from monsoon_amd import MonsoonError
    env = _open(ext, u)
    seed0 = (np.arange(N, dtype=np.uint32) * 31 + 77 + u).astype(np.uint32)
    decks = _decks(ext)
    env.reset(seed0, decks, opponent="expert", agent_side=1, max_steps=40)
    hist = History()
    model = VecEnvModel(seed0, decks, opponent=1, agent_side=1, max_steps=40, extended=ext, on_commit=hist)
    rs = np.random.RandomState(9 + u)
    _lockstep(torch, env, model, 5, rs, "first env")
    _compare_afterstates(env, AfterstatesModel(model, hist, extended=ext), range(0, N, 4), "first env")
    _rollout(ext, env, 0)
    with pytest.raises(MonsoonError):   # the rollout ended env mode
        env.step(torch.full((N,), 155, dtype=torch.uint8, device="cuda"))
    hist = History()
    model = _heuristic(ext, env, 11 + u, 0, hist)
    am = AfterstatesModel(model, hist, extended=ext)
    _lockstep(torch, env, model, 8, rs, "second env")
    assert _compare_afterstates(env, am, range(1, N, 4), "second env")[0] > 0
    _lockstep(torch, env, model, 8, rs, "second env, on")
    _rollout(ext, env, 1)
    model = _heuristic(ext, env, 13 + u, 1)
    ends = _lockstep(torch, env, model, 25, rs, "third env")
    assert ends > 0
    env.close()


def test_captured_step_survives_a_rollout_that_grows_the_overflow_blocks():
    """A step captured into a graph holds the overflow buffer of its capture.  A rollout at U = 64 on the same handle needs
    a larger one; after it and a reset with the same arguments the old graph replays on the block it was captured with,
    which the handle keeps: every replay equals an eager twin.

    That the rollout outgrows the buffer is arithmetic on the host code, not something the ABI shows: monsoon_create
    sizes it for max_games = 37 rounded up to the standard build's 64 API lanes (64 stepping lanes), this reset raises
    it to 37 afterstate workgroups x the default variant's 8 lanes = 296, and 37 matches are fewer than the resident
    grid, so the rollout launches a wavefront per game: 37 x 64 = 2 368 lanes.  The inputs of that sum are asserted."""
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    ext, u = 0, 64
    for knob in ("MONSOON_GRID", "MONSOON_PERSIST", "MONSOON_LANES"):   # development knobs that would change the grids
        assert knob not in os.environ, knob
    env, twin = _open(ext, u), VecEnv(N)
    assert env.engine.max_games == N == 37 and env.engine.variant()[0] == 64 and twin.engine.variant()[0] == 8
    seed0 = (np.arange(N, dtype=np.uint32) * 13 + 31).astype(np.uint32)
    decks = _decks(ext)
    kw = dict(opponent="expert", agent_side=0, max_steps=30)
    va = env.reset(seed0, decks, **kw)
    s = env.stream
    actions = torch.zeros(N, dtype=torch.uint8, device="cuda")

    def first_legal(v):
        return v["legal"].to(torch.uint8).argmax(dim=1).to(torch.uint8)

    with torch.cuda.stream(s):   # warm-up outside the graph
        actions.copy_(first_legal(va))
        env.step(actions)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        actions.copy_(first_legal(va))
        env.step(actions)
    g.replay()
    torch.cuda.synchronize()
    _rollout(ext, env, 2)   # N x 64 stepping lanes: more than the env ever asked for
    assert env.reset(seed0, decks, **kw) is va   # the same view tensors, the same workspace: what the graph points to
    vb = twin.reset(seed0, decks, **kw)
    for t in range(40):
        g.replay()
        vb = twin.step(first_legal(vb))
        torch.cuda.synchronize()
        assert_views_equal(host_views(va), host_views(vb), f"replay {t}")
        assert np.array_equal(env.state_hash(), twin.state_hash()), t
    assert int(host_views(va)["episode"].max()) >= 1
    env.close()
    twin.close()
