"""GPU tests of the vector env's softmax heuristic opponents (k_env_opp_sample, monsoon_env_set_opponent_sample, VecEnv
opponent_explore=OpponentExplore(temperature=)): every view, state hash and explored counter in lockstep with the Python
model (tests/vec_env_sample_model.py, over the CPU oracle) on the three record builds, the armed-but-silent env against a
plain twin, retuning epsilons and temperatures under a captured step, rewind and fork under sampling, and the error paths.
The standard-record lockstep plays the configuration whose coverage tests/test_vec_env_sample_cpu.py proves on the model."""
import ctypes

import numpy as np
import pytest

import vec_env_sample_model as M
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


def _rule(spec):
    from monsoon_amd.vec_env import OpponentExplore
    return OpponentExplore(spec["eps"], spec["explore_seed"], spec["until_step"], temperature=spec["temperature"])


def _assert_counters(env, decisions):
    """Word 7 counts the opponents' committed steps, word 16 n_legal per decision: a decision that sampled another action
    than its arg-max executed one step more than word 16 counts."""
    out = env.engine.debug_counters()
    assert (int(out[7]), int(out[16])) == (len(decisions), sum(d.n_legal for d in decisions))


@pytest.mark.parametrize("agent_side,until_step", M.LOCKSTEP_CASES)
def test_lockstep_with_model(agent_side, until_step):
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    c, views0, hashes0, explored0, trail, decisions, _ = M.lockstep_case(agent_side, until_step)
    n = len(c["seed0"])
    env = VecEnv(n)
    views = env.reset(c["seed0"], c["decks"], opponent="heuristic", agent_side=agent_side, max_steps=c["max_steps"],
                      opponent_weights=c["weights"], opponent_rows=c["rows"], opponent_explore=_rule(c))
    assert_views_equal(host_views(views), views0, "reset")
    assert np.array_equal(env.state_hash(), hashes0)
    assert np.array_equal(_explored(env), explored0)   # (agent_side 1: the opening turns sampled already)
    for t, (a, want, hashes, explored) in enumerate(trail):
        got = host_views(env.step(torch.from_numpy(a).cuda()))
        assert_views_equal(got, want, f"step {t}")
        assert np.array_equal(env.state_hash(), hashes), t
        assert np.array_equal(_explored(env), explored), t
    assert explored.sum() > 0 and (explored[0::4] == 0).all()
    assert any(d.rank >= 0 and d.taken != d.greedy for d in decisions)
    _assert_counters(env, decisions)
    env.close()


@pytest.mark.parametrize("extended,n,steps,agent_side", [(1, 128, 80, 1), (2, 32, 60, 0)])
def test_pool_decks_lockstep_on_the_larger_records(extended, n, steps, agent_side):
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    pool = observable_pool()
    w = M.league(4)
    eps, temperature = M.eps_of(n), M.temperatures_of(n)
    spec = dict(seed0=(np.arange(n, dtype=np.uint32) * 13 + 9000 + 100 * extended).astype(np.uint32), weights=w, rows=np.arange(n) % 4,
                eps=eps, thresholds=M.thresholds_of(eps), temperature=temperature, inv_temperatures=1.0 / temperature, explore_seed=66,
                until_step=0, agent_side=agent_side, max_steps=100)
    model = M.open_model(spec, pool=pool, extended=extended)
    env = VecEnv(n, extended=extended)
    views = env.reset(spec["seed0"], pool=pool, opponent="heuristic", agent_side=agent_side, max_steps=100, opponent_weights=w,
                      opponent_rows=spec["rows"], opponent_explore=_rule(spec))
    assert_views_equal(host_views(views), model.views, "reset")
    assert np.array_equal(env.state_hash(), model.hashes())
    rs = np.random.RandomState(extended)
    for t in range(steps):
        a = M.random_legal(rs, model.views["legal"])
        got = host_views(env.step(torch.from_numpy(a).cuda()))
        assert_views_equal(got, model.step(a), f"step {t}")
        assert np.array_equal(env.state_hash(), model.hashes()), t
        assert np.array_equal(_explored(env), model.explored), t
    moved = [d for d in model.decisions if d.rank >= 0 and d.taken != d.greedy]
    assert model.explored.sum() > len(moved) > 0 and model.episode.max() >= 1
    assert any(d.rank >= 8 for d in moved)   # (a rank beyond the first pass of the build's 8 candidate lanes)
    _assert_counters(env, model.decisions)
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
    va = armed.reset(seed0, decks, opponent_explore=OpponentExplore(0.0, 123, temperature=1.0), **kw)
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


def test_retuning_under_a_captured_step():
    """A step captured while every threshold is 0 is replayed, then epsilons AND temperatures are changed between replays:
    the graph holds the buffers' addresses, the kernel reads the rule, the thresholds and the inverse temperatures at every
    decision, and the replays follow the model."""
    torch = _torch()
    from monsoon_amd.vec_env import OpponentExplore, VecEnv
    n = 128
    w = M.league(4)
    spec = dict(seed0=np.arange(n, dtype=np.uint32) + 41, decks=M.mixed_decks(n), weights=w, rows=np.arange(n) % 4,
                thresholds=np.zeros(n, dtype=np.uint32), inv_temperatures=np.ones(n), explore_seed=1, until_step=0, agent_side=1, max_steps=50)
    model = M.open_model(spec)
    env = VecEnv(n)
    views = env.reset(spec["seed0"], spec["decks"], opponent="heuristic", agent_side=1, max_steps=50, opponent_weights=w,
                      opponent_rows=spec["rows"], opponent_explore=OpponentExplore(0.0, 1, temperature=1.0))
    actions = torch.zeros(n, dtype=torch.uint8, device="cuda")   # (the graph holds its address)
    s = env.stream
    with torch.cuda.stream(s):   # the warm-up step: played
        actions.copy_(_first_legal(torch, views["legal"]))
        env.step(actions)
    torch.cuda.synchronize()
    model.step(model.views["legal"].argmax(axis=1).astype(np.uint8))
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g, stream=s):   # the captured step: not played
        actions.copy_(_first_legal(torch, views["legal"]))
        env.step(actions)
    nodes, edges = _graph_is_a_chain(torch, g)
    assert nodes >= 8 and edges == nodes - 1, (nodes, edges)
    g.instantiate()

    def replay(count, ctx):
        for t in range(count):
            want = model.step(model.views["legal"].argmax(axis=1).astype(np.uint8))
            g.replay()
            torch.cuda.synchronize()
            assert_views_equal(host_views(views), want, f"{ctx} replay {t}")
            assert np.array_equal(env.state_hash(), model.hashes()), (ctx, t)
            assert np.array_equal(_explored(env), model.explored), (ctx, t)

    replay(5, "silent")
    assert model.explored.sum() == 0
    eps, temperature = M.eps_of(n), M.temperatures_of(n)
    env.set_opponent_explore(OpponentExplore(eps, 777, temperature=temperature))
    model.set_sample(777, 0, M.thresholds_of(eps), 1.0 / temperature)
    replay(12, "first retune")
    first = len(model.decisions)
    assert model.explored.sum() > 0 and any(d.rank >= 0 and d.taken != d.greedy for d in model.decisions)
    eps2, temperature2 = eps[::-1].copy(), np.full(n, 5.0)   # other epsilons, another seed, one loose temperature
    env.set_opponent_explore(OpponentExplore(eps2, 778, temperature=temperature2))
    model.set_sample(778, 0, M.thresholds_of(eps2), 1.0 / temperature2)
    replay(8, "second retune")
    assert any(d.rank >= 0 and d.taken != d.greedy for d in model.decisions[first:])
    env.close()


def test_rewind_and_fork_under_sampling():
    torch = _torch()
    from monsoon_amd.vec_env import OpponentExplore, VecEnv
    n = 64
    w = M.league(8)
    temperature = M.temperatures_of(n)
    spec = dict(seed0=(np.arange(n, dtype=np.uint32) * 7919 + 901).astype(np.uint32), decks=M.mixed_decks(n), weights=w,
                rows=(np.arange(n) * 3) % 8, thresholds=M.thresholds_of(np.ones(n)), inv_temperatures=1.0 / temperature, explore_seed=31,
                until_step=0, agent_side=0, max_steps=90)
    env = VecEnv(n)
    views = env.reset(spec["seed0"], spec["decks"], opponent="heuristic", agent_side=0, max_steps=90, opponent_weights=w,
                      opponent_rows=spec["rows"], opponent_explore=OpponentExplore(1.0, 31, temperature=temperature))
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
    for t, (a, h, v) in enumerate(first):   # the rewind samples exactly as the first run did
        env.step(torch.from_numpy(a).cuda())
        assert np.array_equal(env.state_hash(), h), t
        assert_views_equal(host_views(views), v, f"rewind step {t}")
    # the fork: entry 0 into every slot; the slots' seed0 and temperatures differ, so do their choices
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
    inv = np.ones(n)
    out = torch.zeros(n, dtype=torch.int32, device="cuda")

    def ptr(a):
        return None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def sample(ex_, th_, inv_, n_):
        return lib.monsoon_env_set_opponent_sample(h, None if ex_ is None else ctypes.byref(ex_), ptr(th_), ptr(inv_), n_)

    def uniform(ex_, th_, n_):
        return lib.monsoon_env_set_opponent_explore(h, None if ex_ is None else ctypes.byref(ex_), ptr(th_), n_)

    def explored_dev():
        return lib.monsoon_env_opponent_explored_dev(h, ctypes.c_void_p(out.data_ptr()))

    def bad_entries():
        for v in (float("nan"), float("inf"), -float("inf"), 0.0, -0.0, -1.0):
            for at in (0, n - 1):
                a = inv.copy()
                a[at] = v
                yield a

    # bad arguments, no env loaded
    assert lib.monsoon_env_set_opponent_sample(None, ctypes.byref(ex), ptr(th), ptr(inv), n) == _lib.ERR_ARG
    assert sample(ex, th, None, n) == _lib.ERR_ARG   # NULL inv_temperature
    assert sample(ex, None, inv, n) == _lib.ERR_ARG
    assert sample(ex, th, inv, 0) == _lib.ERR_ARG and sample(ex, th, inv, -1) == _lib.ERR_ARG and sample(ex, th, inv, n + 1) == _lib.ERR_ARG
    for a in bad_entries():
        assert sample(ex, th, a, n) == _lib.ERR_ARG, a
    assert explored_dev() == _lib.ERR_STATE   # no env
    assert sample(None, None, None, 0) == _lib.OK   # clearing what is not there
    # an opponent-2 env reset WITHOUT a rule: neither setter sets one, no counters are read
    env.reset(seed0, deck, opponent="heuristic", opponent_weights=w)
    assert sample(ex, th, inv, n) == _lib.ERR_STATE and uniform(ex, th, n) == _lib.ERR_STATE
    assert explored_dev() == _lib.ERR_STATE
    with pytest.raises(MonsoonError):
        env.set_opponent_explore(OpponentExplore(0.5, 1, temperature=1.0))
    with pytest.raises(MonsoonError):
        env.opponent_explored()   # before a rule
    # opponents 0 and 1 ignore the rule: either kind is stored, and replaces the other, while such an env is loaded
    env.reset(seed0, deck, opponent="expert")
    assert sample(ex, th, inv, n - 1) == _lib.OK
    with pytest.raises(MonsoonError, match="monsoon_env_set_opponent_sample"):   # the reset's n differs from the rule's
        env.reset(seed0, deck, opponent="heuristic", opponent_weights=w)
    assert uniform(ex, th, n) == _lib.OK and sample(ex, th, inv, n) == _lib.OK
    # an env reset WITH the sampling rule
    env.reset(seed0, deck, opponent="heuristic", opponent_weights=w, opponent_explore=OpponentExplore(0.5, 1, temperature=0.5))
    counters = env.engine.debug_counters()[[6, 7, 16]]
    hashes = env.state_hash()
    assert sample(ex, th, inv, n - 1) == _lib.ERR_ARG   # n mismatch
    assert sample(ex, th, None, n) == _lib.ERR_ARG and sample(ex, None, inv, n) == _lib.ERR_ARG
    for a in bad_entries():
        assert sample(ex, th, a, n) == _lib.ERR_ARG, a
    assert uniform(ex, th, n) == _lib.ERR_STATE   # the uniform setter under a sampling env
    assert sample(None, None, None, 0) == _lib.ERR_STATE and uniform(None, None, 0) == _lib.ERR_STATE   # clearing under a loaded env
    with pytest.raises(MonsoonError, match="sampling rule"):   # Python refuses the other kind before the library is touched
        env.set_opponent_explore(OpponentExplore(0.5, 1))
    with pytest.raises(ValueError):
        env.set_opponent_explore(OpponentExplore(0.5, 1, temperature=np.ones(n + 1)))
    assert sample(ex, th, inv, n) == _lib.OK
    assert explored_dev() == _lib.OK
    # nothing was launched by any of it: the counters and the states are where the reset left them
    assert np.array_equal(env.engine.debug_counters()[[6, 7, 16]], counters) and np.array_equal(env.state_hash(), hashes)
    env.step(torch.full((n,), 155, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    # a reset without opponent_explore on the armed VecEnv plays silent (the loaded env's rule cannot be cleared)
    env.reset(seed0, deck, opponent="heuristic", opponent_weights=w)
    for _ in range(5):
        env.step(torch.full((n,), 155, dtype=torch.uint8, device="cuda"))
    assert (env.opponent_explored().cpu().numpy() == 0).all()
    env.close()
    # the reverse: the sampling setter under an env reset with the uniform rule
    env = VecEnv(n)
    lib, h = env.engine.lib, env.engine.h
    env.reset(seed0, deck, opponent="heuristic", opponent_weights=w, opponent_explore=OpponentExplore(0.5, 1))
    assert sample(ex, th, inv, n) == _lib.ERR_STATE and uniform(ex, th, n) == _lib.OK
    assert sample(None, None, None, 0) == _lib.ERR_STATE and uniform(None, None, 0) == _lib.ERR_STATE
    with pytest.raises(MonsoonError, match="uniform rule"):
        env.set_opponent_explore(OpponentExplore(0.5, 1, temperature=1.0))
    assert explored_dev() == _lib.OK   # the counters serve both kinds
    env.close()
