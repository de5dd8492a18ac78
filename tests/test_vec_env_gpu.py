"""GPU tests of the vector env (monsoon_env_reset / monsoon_env_step_dev, monsoon_amd/vec_env.py): every view and every
slot's state hash in lockstep with the Python model of the contract (tests/vec_env_model.py, over the CPU oracle), at
full size, with illegal / skipped actions, with per-episode pool decks on the extended build, captured into a graph, and
the error paths."""
import ctypes

import numpy as np
import pytest

from monsoon_amd.cards import DECKS, C5_STREAM_XOR, deck_indices, observable_pool
from vec_env_model import VecEnvModel, is_noop_use

pytestmark = pytest.mark.gpu

PAIRS = [("N12M", "N12M"), ("N12V", "S12"), ("IRONCLAD", "SWARM"), ("S12", "N12M"), ("SWARM", "N12V")]


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def mixed_decks(n):
    pairs = [np.stack([deck_indices(a), deck_indices(b)]) for a, b in PAIRS]
    return np.stack([pairs[i % len(pairs)] for i in range(n)])


def host_views(views, sel=None):
    out = {}
    for k, t in views.items():
        a = t.cpu().numpy()
        out[k] = a if sel is None else a[sel]
    return out


def random_legal(rs, legal):
    """numpy-seeded uniform choice among each row's legal actions."""
    u = rs.random_sample(legal.shape)
    u[~legal] = -1.0
    return u.argmax(axis=1).astype(np.uint8)


def assert_guard_only_on_endless_turns(model):
    """The bot guard (fault 27) fires only where the reference's bot would never hand the turn back: the bot of
    the model -- the reference's expert_action -- spent the end of that turn repeating actions that do nothing."""
    for turn in model.bot_bound_turns:
        assert len(turn) == 64 and all(is_noop_use(a) for a in turn[-32:]), turn


def assert_views_equal(got, want, ctx):
    """Every view equal.  final_hash only where the episode did not end on a fault: a step that raises leaves a partial
    state behind, and the oracle's recursive core and the product core stop at different points of it."""
    for k, w in want.items():
        g = got[k]
        if k == "final_hash":
            keep = want["fault"] == 0
            g, w = g[keep], w[keep]
        assert g.dtype == w.dtype or k == "obs", (ctx, k, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            bad = np.nonzero((g != w).reshape(len(w), -1).any(axis=1))[0] if len(w) else []
            raise AssertionError(f"{ctx}: view {k} differs in slots {bad[:8].tolist()} (of {len(bad)})")


@pytest.mark.parametrize("opponent,agent_side", [(0, 0), (1, 0), (1, 1)])
def test_lockstep_with_model(opponent, agent_side):
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    n, steps = 1024, 300
    seed0 = (np.arange(n, dtype=np.uint32) * 7919 + 11 + 1000 * opponent + 100 * agent_side).astype(np.uint32)
    decks = mixed_decks(n)
    env = VecEnv(n)
    opp = ("none", "expert")[opponent]
    views = env.reset(seed0, decks, opponent=opp, agent_side=agent_side, max_steps=120)
    model = VecEnvModel(seed0, decks, opponent=opponent, agent_side=agent_side, max_steps=120)
    assert_views_equal(host_views(views), model.views, "reset")
    assert np.array_equal(env.state_hash(), model.hashes())
    rs = np.random.RandomState(opponent * 10 + agent_side)
    trunc = 0
    for t in range(steps):
        a = random_legal(rs, model.views["legal"])
        views = env.step(torch.from_numpy(a).cuda())
        want = model.step(a)
        got = host_views(views)
        assert_views_equal(got, want, f"step {t}")
        assert np.array_equal(env.state_hash(), model.hashes()), t
        trunc += int(got["truncated"].sum())
    assert_guard_only_on_endless_turns(model)
    assert model.episode.min() >= 2 and trunc > 0, (model.episode.min(), trunc)
    if opponent:   # a live slot always waits for the agent
        live = model.result == -2
        assert (model.views["to_play"][live] == agent_side).all()
    env.close()


def _device_policy(torch, legal, gen):
    u = torch.rand(legal.shape, device=legal.device, generator=gen)
    u.masked_fill_(~legal, -1.0)
    return u.argmax(dim=1).to(torch.uint8)


def _full_run(torch, n, steps, seed0, decks, sel):
    from monsoon_amd.vec_env import VecEnv
    env = VecEnv(n)
    views = env.reset(seed0, decks, opponent="expert", agent_side=0, max_steps=150)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    w = torch.arange(1, 541, device="cuda", dtype=torch.int64)
    acc = torch.zeros(n, dtype=torch.int64, device="cuda")
    sel_t = torch.from_numpy(sel).cuda()
    trail = []
    for _ in range(steps):
        a = _device_policy(torch, views["legal"], gen)
        trail.append(a[sel_t].cpu().numpy())
        views = env.step(a)
        d = (views["obs"].view(n, -1).to(torch.int64) * w).sum(1) + views["final_hash"] + views["episode"].to(torch.int64) * 3 + \
            views["winner"].to(torch.int64) * 5 + views["legal"].to(torch.int64).sum(1) * 7 + views["reward"].to(torch.int64) * 11
        acc = acc * 1000003 + d
    torch.cuda.synchronize()
    out = (acc.cpu().numpy(), env.state_hash(), host_views(views, sel), trail)
    env.close()
    return out


def test_full_size_replay_and_determinism():
    torch = _torch()
    n, steps = 65536, 200
    seed0 = np.arange(n, dtype=np.uint32) + 500000
    decks = mixed_decks(n)
    sel = np.sort(np.random.RandomState(3).choice(n, 1024, replace=False))
    acc1, hash1, last1, trail = _full_run(torch, n, steps, seed0, decks, sel)
    model = VecEnvModel(seed0, decks, opponent=1, agent_side=0, max_steps=150, slots=sel)
    for t in range(steps):
        want = model.step(trail[t])
    assert_views_equal(last1, want, "full size, last step")
    assert np.array_equal(hash1[sel], model.hashes())
    assert_guard_only_on_endless_turns(model)
    acc2, hash2, _, trail2 = _full_run(torch, n, steps, seed0, decks, sel)
    assert np.array_equal(acc1, acc2) and np.array_equal(hash1, hash2)
    assert all(np.array_equal(x, y) for x, y in zip(trail, trail2))


def test_illegal_and_skip():
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    n = 256
    seed0 = np.arange(n, dtype=np.uint32) + 77
    decks = mixed_decks(n)
    env = VecEnv(n)
    views = env.reset(seed0, decks)
    model = VecEnvModel(seed0, decks)
    legal = host_views(views)["legal"]
    h0 = env.state_hash()
    a = np.zeros(n, dtype=np.uint8)
    for i in range(n):
        la = np.nonzero(legal[i])[0]
        kind = i % 5
        if kind == 0:
            a[i] = next(x for x in range(155) if not legal[i][x])   # not legal
        elif kind == 1:
            a[i] = 255                                                # skip
        elif kind == 2:
            a[i] = 155                                                # PASS: always accepted
        elif kind == 3:
            a[i] = la[0]
        else:
            a[i] = 200                                                # not an action at all
    got = host_views(env.step(torch.from_numpy(a).cuda()))
    want = model.step(a)
    assert_views_equal(got, want, "illegal / skip")
    h1 = env.state_hash()
    flagged = (np.arange(n) % 5 == 0) | (np.arange(n) % 5 == 4)
    assert np.array_equal(got["illegal"], flagged)
    untouched = flagged | (np.arange(n) % 5 == 1)
    assert np.array_equal(h1[untouched], h0[untouched])
    assert (h1[~untouched] != h0[~untouched]).all()
    assert np.array_equal(h1, model.hashes())
    env.close()


def test_pool_decks_extended_lockstep():
    torch = _torch()
    from monsoon_amd.engine import BatchEngine
    from monsoon_amd.vec_env import VecEnv
    n, steps = 512, 200
    pool = observable_pool()
    seed0 = np.arange(n, dtype=np.uint32) * 13 + 9000
    env = VecEnv(n, extended=1)
    views = env.reset(seed0, pool=pool, opponent="expert", agent_side=1, max_steps=100)
    model = VecEnvModel(seed0, pool=pool, opponent=1, agent_side=1, max_steps=100, extended=True)
    assert_views_equal(host_views(views), model.views, "reset")
    rs = np.random.RandomState(8)
    seeds = set(model.seed(j) for j in range(n))
    limit_ends = 0
    for t in range(steps):
        a = random_legal(rs, model.views["legal"])
        got = host_views(env.step(torch.from_numpy(a).cuda()))
        want = model.step(a)
        assert_views_equal(got, want, f"step {t}")
        assert np.array_equal(env.state_hash(), model.hashes()), t
        seeds.update(model.seed(j) for j in range(n))
        limit_ends += int((got["done"] & (got["fault"] >= 16)).sum())
    assert model.episode.min() >= 1
    # every episode's decks are monsoon_draw_decks of its seed (device draw vs numpy's, through the model)
    seeds = np.array(sorted(seeds), dtype=np.uint32)
    eng = BatchEngine(4, extended=1)
    from monsoon_amd.cards import draw_random_decks_numpy
    assert np.array_equal(eng.draw_decks(seeds ^ np.uint32(C5_STREAM_XOR), pool), draw_random_decks_numpy(seeds ^ np.uint32(C5_STREAM_XOR), pool))
    eng.close()
    env.close()
    print(f"episodes ended on a record limit: {limit_ends}")


def _first_legal(torch, legal):
    return legal.to(torch.uint8).argmax(dim=1).to(torch.uint8)


def _graph_is_a_chain(torch, graph):
    """hipGraphGetNodes / hipGraphGetEdges of the captured graph: every node has at most one edge in and one out."""
    hip = ctypes.CDLL("libamdhip64.so.7")   # the runtime torch and this library share (one soname per process)
    raw = ctypes.c_void_p(graph.raw_cuda_graph())
    nn = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(raw, None, ctypes.byref(nn)) == 0
    ne = ctypes.c_size_t(0)
    assert hip.hipGraphGetEdges(raw, None, None, ctypes.byref(ne)) == 0
    if ne.value:
        src = (ctypes.c_void_p * ne.value)()
        dst = (ctypes.c_void_p * ne.value)()
        assert hip.hipGraphGetEdges(raw, src, dst, ctypes.byref(ne)) == 0
        assert len(set(src)) == ne.value and len(set(dst)) == ne.value, "a node with two edges: a side branch"
    return nn.value, ne.value


def test_graph_capture_single_stream():
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    n = 4096
    seed0 = np.arange(n, dtype=np.uint32) + 31
    decks = mixed_decks(n)
    a_env, b_env = VecEnv(n), VecEnv(n)
    va = a_env.reset(seed0, decks, opponent="expert", agent_side=0, max_steps=60)
    vb = b_env.reset(seed0, decks, opponent="expert", agent_side=0, max_steps=60)
    s = a_env.stream
    actions = torch.zeros(n, dtype=torch.uint8, device="cuda")
    # warm-up outside the graph: one step of the first env and of its twin
    with torch.cuda.stream(s):
        actions.copy_(_first_legal(torch, va["legal"]))
        a_env.step(actions)
    b_env.step(_first_legal(torch, vb["legal"]))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g, stream=s):
        actions.copy_(_first_legal(torch, va["legal"]))
        a_env.step(actions)
    nodes, edges = _graph_is_a_chain(torch, g)
    assert nodes >= 4 and edges == nodes - 1, (nodes, edges)
    g.instantiate()
    for t in range(50):
        g.replay()
        wb = b_env.step(_first_legal(torch, vb["legal"]))
        torch.cuda.synchronize()
        assert_views_equal(host_views(va), host_views(wb), f"replay {t}")
        assert np.array_equal(a_env.state_hash(), b_env.state_hash()), t
    assert int(host_views(va)["episode"].max()) >= 1
    a_env.close()
    b_env.close()


def test_error_paths():
    torch = _torch()
    from monsoon_amd import MonsoonError, _lib
    from monsoon_amd.engine import BatchEngine
    from monsoon_amd.vec_env import VecEnv
    eng = BatchEngine(8)
    actions = torch.full((8,), 255, dtype=torch.uint8, device="cuda")
    assert eng.lib.monsoon_env_step_dev(eng.h, ctypes.c_void_p(actions.data_ptr())) == _lib.ERR_STATE
    eng.close()
    env = VecEnv(8)
    env.reset(np.arange(8, dtype=np.uint32), np.stack([deck_indices("N12M")] * 2))
    env.step(actions)
    torch.cuda.synchronize()
    env.engine.reset(np.arange(8, dtype=np.uint32), np.stack([deck_indices("N12M")] * 2))
    assert env.engine.lib.monsoon_env_step_dev(env.engine.h, ctypes.c_void_p(actions.data_ptr())) == _lib.ERR_STATE
    with pytest.raises(MonsoonError):
        env.step(actions)
    # the observable pool holds ua20 and b005: refused by the standard build at reset, accepted by the extended one
    with pytest.raises(MonsoonError, match="not supported"):
        env.reset(np.arange(8, dtype=np.uint32), pool=observable_pool())
    with pytest.raises(MonsoonError, match="not supported"):
        env.reset(np.arange(8, dtype=np.uint32), np.stack([deck_indices(DECKS["N12M"][:11] + ["b005"])] * 2))
    env.close()
    ext = VecEnv(8, extended=1)
    ext.reset(np.arange(8, dtype=np.uint32), pool=observable_pool())
    ext.step(actions)
    torch.cuda.synchronize()
    ext.close()
