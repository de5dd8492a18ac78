"""GPU tests of the vector env's epsilon-greedy heuristic opponents (k_env_opp_explore, monsoon_env_set_opponent_explore,
VecEnv opponent_explore): every view, state hash and explored counter in lockstep with the Python model
(tests/vec_env_explore_model.py, over the CPU oracle) on the three record builds, the armed-but-silent env against a plain
twin, retuning under a captured step, rewind and fork under exploration, and the error paths.  The standard-record lockstep
plays the configuration whose coverage tests/test_vec_env_explore_cpu.py proves on the model."""
import ctypes

import numpy as np
import pytest

import vec_env_explore_model as M
from monsoon_amd.cards import deck_indices, observable_pool
from test_vec_env_gpu import _first_legal, _graph_is_a_chain, assert_views_equal, host_views

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _explored(env):
    return env.opponent_explored().cpu().numpy().astype(np.int64)


def _eps(n):
    return np.array([M.LOCKSTEP_EPS[i % 4] for i in range(n)])


@pytest.mark.parametrize("agent_side,until_step", M.LOCKSTEP_CASES)
def test_lockstep_with_model(agent_side, until_step):
    torch = _torch()
    from monsoon_amd.vec_env import OpponentExplore, VecEnv
    c, views0, hashes0, explored0, trail, _, _ = M.lockstep_case(agent_side, until_step)
    n = len(c["seed0"])
    env = VecEnv(n)
    views = env.reset(c["seed0"], c["decks"], opponent="heuristic", agent_side=agent_side, max_steps=c["max_steps"],
                      opponent_weights=c["weights"], opponent_rows=c["rows"],
                      opponent_explore=OpponentExplore(c["eps"], c["explore_seed"], until_step))
    assert_views_equal(host_views(views), views0, "reset")
    assert np.array_equal(env.state_hash(), hashes0)
    assert np.array_equal(_explored(env), explored0)   # (agent_side 1: the opening turns explored already)
    for t, (a, want, hashes, explored) in enumerate(trail):
        got = host_views(env.step(torch.from_numpy(a).cuda()))
        assert_views_equal(got, want, f"step {t}")
        assert np.array_equal(env.state_hash(), hashes), t
        assert np.array_equal(_explored(env), explored), t
    assert explored.sum() > 0 and (explored[0::4] == 0).all()
    # every legal action is stepped exactly once, explored decision or not: word 16 is the sum of the decisions' legal counts
    out = env.engine.debug_counters()
    _, _, _, _, _, decisions, _ = M.lockstep_case(agent_side, until_step)
    assert (int(out[7]), int(out[16])) == (len(decisions), sum(d.n_legal for d in decisions))
    env.close()


@pytest.mark.parametrize("extended,n,steps,agent_side", [(1, 128, 80, 1), (2, 32, 60, 0)])
def test_pool_decks_lockstep_on_the_larger_records(extended, n, steps, agent_side):
    torch = _torch()
    from monsoon_amd.vec_env import OpponentExplore, VecEnv
    pool = observable_pool()
    seed0 = (np.arange(n, dtype=np.uint32) * 13 + 7000 + 100 * extended).astype(np.uint32)
    w = M.league(4)
    rows = np.arange(n) % 4
    eps = _eps(n)
    model = M.ExploringVecEnvModel(seed0, w, rows, explore_seed=55, until_step=0, thresholds=M.thresholds_of(eps), pool=pool,
                                   agent_side=agent_side, max_steps=100, extended=extended)
    env = VecEnv(n, extended=extended)
    views = env.reset(seed0, pool=pool, opponent="heuristic", agent_side=agent_side, max_steps=100, opponent_weights=w,
                      opponent_rows=rows, opponent_explore=OpponentExplore(eps, 55))
    assert_views_equal(host_views(views), model.views, "reset")
    assert np.array_equal(env.state_hash(), model.hashes())
    rs = np.random.RandomState(extended)
    for t in range(steps):
        a = M.random_legal(rs, model.views["legal"])
        got = host_views(env.step(torch.from_numpy(a).cuda()))
        assert_views_equal(got, model.step(a), f"step {t}")
        assert np.array_equal(env.state_hash(), model.hashes()), t
        assert np.array_equal(_explored(env), model.explored), t
    assert model.explored.sum() > 0 and model.episode.max() >= 1
    assert any(d.r >= 8 for d in model.decisions)   # (a rank beyond the first pass of the build's 8 candidate lanes)
    env.close()


def test_armed_but_silent_equals_the_plain_env():
    torch = _torch()
    from monsoon_amd.vec_env import OpponentExplore, VecEnv
    n = 256
    seed0 = (np.arange(n, dtype=np.uint32) * 7919 + 77).astype(np.uint32)
    decks, w = M.mixed_decks(n), M.league(8)
    rows = (np.arange(n) * 5) % 8
    kw = dict(opponent="heuristic", agent_side=1, max_steps=90, opponent_weights=w, opponent_rows=rows)
    armed, plain = VecEnv(n), VecEnv(n)
    va = armed.reset(seed0, decks, opponent_explore=OpponentExplore(0.0, 123), **kw)
    vp = plain.reset(seed0, decks, **kw)
    assert armed.engine.debug_counters()[7] == plain.engine.debug_counters()[7] > 0
    rs = np.random.RandomState(3)
    assert_views_equal(host_views(va), host_views(vp), "reset")
    for t in range(100):
        a = torch.from_numpy(M.random_legal(rs, host_views(vp)["legal"])).cuda()
        ga, gp = host_views(armed.step(a)), host_views(plain.step(a))
        assert_views_equal(ga, gp, f"step {t}")
        assert np.array_equal(ga["final_hash"], gp["final_hash"]) and np.array_equal(armed.state_hash(), plain.state_hash()), t
    assert (_explored(armed) == 0).all()
    assert np.array_equal(armed.engine.debug_counters()[[6, 7, 16]], plain.engine.debug_counters()[[6, 7, 16]])
    assert int(ga["episode"].max()) >= 1
    armed.close()
    plain.close()


def _capture_step(torch, env, views, actions):
    s = env.stream
    with torch.cuda.stream(s):
        actions.copy_(_first_legal(torch, views["legal"]))
        env.step(actions)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g, stream=s):
        actions.copy_(_first_legal(torch, views["legal"]))
        env.step(actions)
    return g


def test_retuning_under_a_captured_step():
    """A step captured while every threshold is 0 is retuned between replays: the graph holds the buffers' addresses, and
    the kernel reads the rule and the thresholds at every decision."""
    torch = _torch()
    from monsoon_amd.vec_env import OpponentExplore, VecEnv
    n = 1024
    seed0 = np.arange(n, dtype=np.uint32) + 41
    decks, w = M.mixed_decks(n), M.league(4)
    rows = np.arange(n) % 4
    kw = dict(opponent="heuristic", agent_side=1, max_steps=50, opponent_weights=w, opponent_rows=rows)
    a_env, b_env, c_env = VecEnv(n), VecEnv(n), VecEnv(n)
    va = a_env.reset(seed0, decks, opponent_explore=OpponentExplore(0.0, 1), **kw)
    vb = b_env.reset(seed0, decks, opponent_explore=OpponentExplore(0.0, 1), **kw)
    vc = c_env.reset(seed0, decks, **kw)
    act_a, act_c = (torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(2))   # (the graphs hold their addresses)
    g = _capture_step(torch, a_env, va, act_a)
    g_plain = _capture_step(torch, c_env, vc, act_c)
    b_env.step(_first_legal(torch, vb["legal"]))
    torch.cuda.synchronize()
    nodes, edges = _graph_is_a_chain(torch, g)
    assert (nodes, edges) == _graph_is_a_chain(torch, g_plain) and nodes >= 8 and edges == nodes - 1, (nodes, edges)
    g.instantiate()
    g_plain.instantiate()

    def replay(count, ctx):
        for t in range(count):
            g.replay()
            wb = b_env.step(_first_legal(torch, vb["legal"]))
            torch.cuda.synchronize()
            assert_views_equal(host_views(va), host_views(wb), f"{ctx} replay {t}")
            assert np.array_equal(a_env.state_hash(), b_env.state_hash()), (ctx, t)

    replay(10, "silent")
    assert (_explored(a_env) == 0).all() and (_explored(b_env) == 0).all()
    silent_hash = a_env.state_hash()
    for _ in range(10):   # the plain twin took the warm-up step of its capture only: ten steps behind
        c_env.step(_first_legal(torch, vc["legal"]))
    assert np.array_equal(silent_hash, c_env.state_hash())
    a_env.set_opponent_explore(OpponentExplore(0.5, 777))
    b_env.set_opponent_explore(OpponentExplore(0.5, 777))
    replay(15, "eps 0.5")
    ea, eb = _explored(a_env), _explored(b_env)
    assert np.array_equal(ea, eb) and ea.sum() > n
    for _ in range(15):
        c_env.step(_first_legal(torch, vc["legal"]))
    assert not np.array_equal(a_env.state_hash(), c_env.state_hash())   # (the retuned env left the plain twin's line)
    for e in (a_env, b_env, c_env):
        e.close()


def test_rewind_and_fork_under_exploration():
    torch = _torch()
    from monsoon_amd.vec_env import OpponentExplore, VecEnv
    n = 64
    seed0 = (np.arange(n, dtype=np.uint32) * 7919 + 901).astype(np.uint32)
    w = M.league(8)
    spec = dict(seed0=seed0, decks=M.mixed_decks(n), weights=w, rows=(np.arange(n) * 3) % 8, thresholds=M.thresholds_of(np.ones(n)),
                explore_seed=31, until_step=0, agent_side=0, max_steps=90)
    env = VecEnv(n)
    views = env.reset(seed0, spec["decks"], opponent="heuristic", agent_side=0, max_steps=90, opponent_weights=w,
                      opponent_rows=spec["rows"], opponent_explore=OpponentExplore(1.0, 31))
    rs = np.random.RandomState(6)

    def act():
        a = M.random_legal(rs, host_views(views)["legal"])
        env.step(torch.from_numpy(a).cuda())
        return a

    prefix = [act() for _ in range(5)]
    snap = env.snapshot()
    first = []
    for _ in range(20):
        a = act()
        first.append((a, env.state_hash(), host_views(views)))
    assert _explored(env).sum() > 0
    env.restore(snap)
    for t, (a, h, v) in enumerate(first):   # the rewind explores exactly as the first run did
        env.step(torch.from_numpy(a).cuda())
        assert np.array_equal(env.state_hash(), h), t
        assert_views_equal(host_views(views), v, f"rewind step {t}")
    # the fork: entry 0 into every slot; the slots' seed0 differ, so do their draws
    loaded = torch.zeros(n, dtype=torch.uint8, device="cuda")
    env.restore(snap, src=torch.zeros(n, dtype=torch.int32, device="cuda"), dst=torch.arange(n, dtype=torch.int32, device="cuda"),
                loaded=loaded)
    assert bool(loaded.all())
    forks = [M.forked(spec, 0, [p[0] for p in prefix], d) for d in range(n)]
    assert len(set(env.state_hash().tolist())) == 1
    for t in range(10):
        a = int(M.random_legal(rs, host_views(views)["legal"][:1])[0])   # slot 0's choice for every slot (illegal elsewhere: untouched)
        got = host_views(env.step(torch.full((n,), a, dtype=torch.uint8, device="cuda")))
        for f in forks:
            f.step([a])
        for k in ("legal", "to_play", "done", "illegal", "episode", "winner", "fault"):
            assert np.array_equal(got[k], np.concatenate([f.views[k] for f in forks])), (t, k)
        assert np.array_equal(env.state_hash(), np.array([f.hashes()[0] for f in forks], dtype=np.uint64)), t
    assert len(set(env.state_hash().tolist())) >= 2
    env.close()


def test_error_paths():
    torch = _torch()
    from monsoon_amd import MonsoonError, _lib
    from monsoon_amd.vec_env import OpponentExplore, VecEnv
    n = 8
    seed0 = np.arange(n, dtype=np.uint32)
    deck = np.stack([deck_indices("N12M")] * 2)
    w = M.league(4)
    env = VecEnv(n)
    lib, h = env.engine.lib, env.engine.h
    ex = _lib.EnvExplore(5, 0)
    th = np.zeros(n, dtype=np.uint32)
    ptr = th.ctypes.data_as(ctypes.c_void_p)
    out = torch.zeros(n, dtype=torch.int32, device="cuda")

    def set_rule(ex_, ptr_, n_):
        return lib.monsoon_env_set_opponent_explore(h, None if ex_ is None else ctypes.byref(ex_), ptr_, n_)

    # bad arguments, no env loaded
    assert set_rule(ex, None, n) == _lib.ERR_ARG
    assert set_rule(ex, ptr, 0) == _lib.ERR_ARG and set_rule(ex, ptr, -1) == _lib.ERR_ARG and set_rule(ex, ptr, n + 1) == _lib.ERR_ARG
    assert lib.monsoon_env_set_opponent_explore(None, ctypes.byref(ex), ptr, n) == _lib.ERR_ARG
    assert lib.monsoon_env_opponent_explored_dev(h, ctypes.c_void_p(out.data_ptr())) == _lib.ERR_STATE   # no env
    assert set_rule(None, None, 0) == _lib.OK   # clearing what is not there
    # an opponent-2 env reset WITHOUT a rule: no rule can be set, no counters read; Python says so before the library does
    env.reset(seed0, deck, opponent="heuristic", opponent_weights=w)
    assert set_rule(ex, ptr, n) == _lib.ERR_STATE
    assert lib.monsoon_env_opponent_explored_dev(h, ctypes.c_void_p(out.data_ptr())) == _lib.ERR_STATE
    with pytest.raises(MonsoonError):
        env.set_opponent_explore(OpponentExplore(0.5, 1))
    with pytest.raises(MonsoonError):
        env.opponent_explored()
    # opponents 0 and 1 ignore the rule: it is stored while such an env is loaded; a reset to opponent 2 with another n is refused
    env.reset(seed0, deck, opponent="expert")
    assert set_rule(ex, ptr, n - 1) == _lib.OK
    with pytest.raises(MonsoonError, match="monsoon_env_set_opponent_explore"):
        env.reset(seed0, deck, opponent="heuristic", opponent_weights=w)
    assert lib.monsoon_env_opponent_explored_dev(h, ctypes.c_void_p(out.data_ptr())) == _lib.ERR_STATE   # (the reset failed: no env)
    with pytest.raises(ValueError, match="opponent_explore"):
        env.reset(seed0, deck, opponent="expert", opponent_explore=OpponentExplore(0.5, 1))
    # an env reset WITH a rule: another n and a NULL rule are refused, the same n is accepted
    env.reset(seed0, deck, opponent="heuristic", opponent_weights=w, opponent_explore=OpponentExplore(0.5, 1))
    assert set_rule(ex, ptr, n - 1) == _lib.ERR_ARG
    assert set_rule(ex, None, n) == _lib.ERR_ARG
    assert set_rule(None, None, 0) == _lib.ERR_STATE
    assert set_rule(ex, ptr, n) == _lib.OK
    assert lib.monsoon_env_opponent_explored_dev(h, None) == _lib.ERR_ARG
    assert lib.monsoon_env_opponent_explored_dev(h, ctypes.c_void_p(out.data_ptr())) == _lib.OK
    with pytest.raises(ValueError):
        env.set_opponent_explore(OpponentExplore(np.zeros(n + 1), 1))
    env.step(torch.full((n,), 155, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    # a reset without opponent_explore on the armed VecEnv plays silent (the loaded env's rule cannot be cleared)
    env.reset(seed0, deck, opponent="heuristic", opponent_weights=w)
    for _ in range(5):
        env.step(torch.full((n,), 155, dtype=torch.uint8, device="cuda"))
    assert (env.opponent_explored().cpu().numpy() == 0).all()
    env.close()
