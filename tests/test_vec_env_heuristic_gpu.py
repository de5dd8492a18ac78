"""GPU tests of the vector env's heuristic opponent (opponent 2: k_env_opp, monsoon_env_set_opponents, VecEnv
opponent="heuristic"): every view and state hash in lockstep with the Python model (tests/vec_env_heuristic_model.py, over
the CPU oracle), the reference's HeuristicAgent traces replayed on the device, full size, graph capture, league updates and
the error paths."""
import ctypes

import numpy as np
import pytest

from monsoon_amd.cards import deck_indices, observable_pool
from test_vec_env_gpu import _first_legal, _graph_is_a_chain, assert_views_equal, host_views, mixed_decks, random_legal
from vec_env_heuristic_model import FAULT_OPP_BOUND, OPP_BOUND, HeuristicVecEnvModel
from vec_env_model import is_noop_use

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def league(k=8):
    """k GA individuals: the committed population's initial and offspring weights."""
    import os
    pop = np.load(os.path.join(os.path.dirname(__file__), "golden", "population_seed42.npz"))
    return np.concatenate([pop["init_weights"], pop["off_weights"]])[:k].copy()


def assert_guard_only_on_endless_turns(model):
    for turn in model.opp_bound_turns:
        assert len(turn) == OPP_BOUND and all(is_noop_use(a) for a in turn[-32:]), turn


def lockstep(torch, env, model, n, steps, rs, ctx):
    trunc = opp_ends = 0
    for t in range(steps):
        a = random_legal(rs, model.views["legal"])
        got = host_views(env.step(torch.from_numpy(a).cuda()))
        want = model.step(a)
        assert_views_equal(got, want, f"{ctx} step {t}")
        assert np.array_equal(env.state_hash(), model.hashes()), (ctx, t)
        trunc += int(got["truncated"].sum())
        opp_ends += int((got["fault"] == FAULT_OPP_BOUND).sum())
    return trunc, opp_ends


@pytest.mark.parametrize("agent_side,max_steps", [(0, 0), (1, 0), (0, 90), (1, 90)])
def test_lockstep_with_model(agent_side, max_steps):
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    n, steps = 256, 200
    seed0 = (np.arange(n, dtype=np.uint32) * 7919 + 3 + 100 * agent_side + max_steps).astype(np.uint32)
    decks = mixed_decks(n)
    w = league(8)
    rows = (np.arange(n) * 5) % len(w)
    env = VecEnv(n)
    views = env.reset(seed0, decks, opponent="heuristic", agent_side=agent_side, max_steps=max_steps, opponent_weights=w,
                      opponent_rows=rows)
    model = HeuristicVecEnvModel(seed0, w, rows, decks=decks, agent_side=agent_side, max_steps=max_steps)
    assert_views_equal(host_views(views), model.views, "reset")
    assert np.array_equal(env.state_hash(), model.hashes())
    trunc, opp_ends = lockstep(torch, env, model, n, steps, np.random.RandomState(agent_side + max_steps), "fixed decks")
    assert_guard_only_on_endless_turns(model)
    assert opp_ends == model.bot_bound_hits
    assert model.episode.sum() >= n // 4, model.episode.sum()
    if max_steps:
        assert trunc > 0
    live = model.result == -2   # a live slot always waits for the agent
    assert (model.views["to_play"][live] == agent_side).all()
    # monsoon_debug_counters word 7: the opponent's committed steps
    out = (ctypes.c_ulonglong * 192)()
    assert env.engine.lib.monsoon_debug_counters(env.engine.h, out) == 0
    assert out[6] > 0 and out[7] > 0
    env.close()


def test_pool_decks_extended_lockstep():
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    n, steps = 256, 150
    pool = observable_pool()
    seed0 = np.arange(n, dtype=np.uint32) * 13 + 7000
    w = league(4)
    rows = np.arange(n) % 4
    env = VecEnv(n, extended=1)
    views = env.reset(seed0, pool=pool, opponent="heuristic", agent_side=1, max_steps=100, opponent_weights=w, opponent_rows=rows)
    model = HeuristicVecEnvModel(seed0, w, rows, pool=pool, agent_side=1, max_steps=100, extended=True)
    assert_views_equal(host_views(views), model.views, "reset")
    lockstep(torch, env, model, n, steps, np.random.RandomState(8), "pool")
    assert_guard_only_on_endless_turns(model)
    assert model.episode.min() >= 1
    env.close()


def _movers(actions):
    """The side that played each action of a trace game (PASS hands the turn over)."""
    side, out = 0, []
    for a in actions:
        out.append(side)
        if a == 155:
            side ^= 1
    return out


@pytest.mark.parametrize("agent_side", [0, 1])
@pytest.mark.parametrize("fixture", ["trace_heuristic_N12M_2w.npz", "trace_heuristic_S12.npz", "trace_heuristic_IRONCLAD.npz"])
def test_trace_replay_on_device(gold, fixture, agent_side):
    """The CPU model's reference-anchored replay, on the device: slot k plays game k; its agent replays the recorded
    actions of agent_side, and after every step the slot is in the recorded state just before its side's next action
    (or the episode ended where the trace, or the opponent guard, ends it)."""
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    g = gold(fixture)
    w = (g["w0"], g["w1"] if "w1" in g.files else g["w0"])
    deck = np.stack([g["deck"], g["deck1"] if "deck1" in g.files else g["deck"]])
    n = len(g["seeds"])
    env = VecEnv(n)
    env.reset(g["seeds"].astype(np.uint32), deck, opponent="heuristic", agent_side=agent_side,
                      max_steps=int(g["max_turns"]), opponent_weights=w[agent_side ^ 1])
    lo = g["offsets"][:-1].astype(int)
    hi = g["offsets"][1:].astype(int)
    movers = [_movers(g["action"][lo[k]:hi[k]]) for k in range(n)]

    def advance(k, start):
        """Where the slot stops after the opponent's turn from trace index `start`: ("agent", p) before the agent's next
        action p, ("end", None) at the end of the game, ("cut", q) where the guard ends the turn at action q."""
        run = 0
        for q in range(start, hi[k]):
            if movers[k][q - lo[k]] == agent_side:
                return "agent", q
            run += 1
            if run == OPP_BOUND and g["action"][q] != 155:
                return "cut", q
        return "end", None

    def final(got, k):
        return int(got["final_hash"][k:k + 1].view(np.uint64)[0])

    state = [advance(k, lo[k]) for k in range(n)]   # the opponent's opening turn (agent_side 1)
    h = env.state_hash()
    for k in range(n):
        if state[k][0] == "agent" and state[k][1] > lo[k]:
            assert int(h[k]) == int(g["hash"][state[k][1] - 1]), k
    finished = np.zeros(n, dtype=bool)
    for _ in range(int(g["max_turns"]) + 2):
        if finished.all():
            break
        a = np.array([int(g["action"][state[k][1]]) if state[k][0] == "agent" and not finished[k] else 255 for k in range(n)],
                     dtype=np.uint8)
        got = host_views(env.step(torch.from_numpy(a).cuda()))
        h = env.state_hash()
        for k in np.nonzero(~finished)[0]:
            kind, p = state[k]
            if kind == "cut":   # the guard ended the opponent's turn (reported at this step)
                assert got["done"][k] and got["fault"][k] == FAULT_OPP_BOUND and final(got, k) == int(g["hash"][p]), k
                finished[k] = True
                continue
            assert kind == "agent", k
            state[k] = advance(k, p + 1)
            kind, q = state[k]
            if kind == "cut":
                assert got["done"][k] and got["fault"][k] == FAULT_OPP_BOUND and final(got, k) == int(g["hash"][q]), k
                finished[k] = True
            elif kind == "end":   # a winner, or truncation at max_turns
                assert got["done"][k] and got["winner"][k] == g["result"][k] and got["fault"][k] == 0, k
                assert final(got, k) == int(g["hash"][hi[k] - 1]), k
                finished[k] = True
            else:
                assert not got["done"][k] and int(h[k]) == int(g["hash"][q - 1]), (k, q)
    assert finished.all()
    env.close()


def _full_run(torch, n, steps, seed0, decks, w, rows, sel):
    from monsoon_amd.vec_env import VecEnv
    env = VecEnv(n)
    views = env.reset(seed0, decks, opponent="heuristic", agent_side=1, max_steps=150, opponent_weights=w, opponent_rows=rows)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(99)
    sel_t = torch.from_numpy(sel).cuda()
    trail, finals, hashes = [], [], []
    for _ in range(steps):
        u = torch.rand(views["legal"].shape, device="cuda", generator=gen)
        u.masked_fill_(~views["legal"], -1.0)
        a = u.argmax(dim=1).to(torch.uint8)
        trail.append(a[sel_t].cpu().numpy())
        views = env.step(a)
        finals.append(views["final_hash"].cpu().numpy())
        hashes.append(env.state_hash())
    out = (trail, finals, hashes, host_views(views, sel))
    env.close()
    return out


def test_full_size_determinism_and_sample():
    torch = _torch()
    n, steps = 65536, 60
    seed0 = np.arange(n, dtype=np.uint32) + 300000
    decks = mixed_decks(n)
    w = league(8)
    rows = np.arange(n) % len(w)
    sel = np.sort(np.random.RandomState(4).choice(n, 128, replace=False))
    trail, finals, hashes, last = _full_run(torch, n, steps, seed0, decks, w, rows, sel)
    trail2, finals2, hashes2, _ = _full_run(torch, n, steps, seed0, decks, w, rows, sel)
    assert all(np.array_equal(x, y) for x, y in zip(finals, finals2))
    assert all(np.array_equal(x, y) for x, y in zip(hashes, hashes2))
    assert all(np.array_equal(x, y) for x, y in zip(trail, trail2))
    model = HeuristicVecEnvModel(seed0, w, rows, decks=decks, agent_side=1, max_steps=150, slots=sel)
    for t in range(steps):
        want = model.step(trail[t])
        assert np.array_equal(hashes[t][sel], model.hashes()), t
    assert_views_equal(last, want, "full size, last step")
    assert_guard_only_on_endless_turns(model)
    assert sum(int((f != 0).sum()) for f in finals) > 0


def test_graph_capture_replays_equal_eager():
    """A captured step (seven launches, one stream) replayed 40 times equals an eager twin step for step: the two
    k_env_opp launches of a step alternate their pop-counter sets, so every replay starts from cleared counters."""
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    n = 4096
    seed0 = np.arange(n, dtype=np.uint32) + 41
    decks = mixed_decks(n)
    w = league(4)
    rows = np.arange(n) % 4
    kw = dict(opponent="heuristic", agent_side=1, max_steps=50, opponent_weights=w, opponent_rows=rows)
    a_env, b_env = VecEnv(n), VecEnv(n)
    va = a_env.reset(seed0, decks, **kw)
    vb = b_env.reset(seed0, decks, **kw)
    s = a_env.stream
    actions = torch.zeros(n, dtype=torch.uint8, device="cuda")
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
    assert nodes >= 8 and edges == nodes - 1, (nodes, edges)
    g.instantiate()
    for t in range(40):
        g.replay()
        wb = b_env.step(_first_legal(torch, vb["legal"]))
        torch.cuda.synchronize()
        assert_views_equal(host_views(va), host_views(wb), f"replay {t}")
        assert np.array_equal(a_env.state_hash(), b_env.state_hash()), t
    assert int(host_views(va)["episode"].max()) >= 1
    a_env.close()
    b_env.close()


def test_league_update_between_steps():
    """set_opponents between steps: new weights and rows apply from the next step, as in the model; a twin model without
    the update leaves the env's line."""
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    n = 256
    seed0 = np.arange(n, dtype=np.uint32) + 1234
    decks = mixed_decks(n)
    w = league(8)
    rows = np.arange(n) % 4
    env = VecEnv(n)
    env.reset(seed0, decks, opponent="heuristic", agent_side=0, max_steps=120, opponent_weights=w, opponent_rows=rows)
    model = HeuristicVecEnvModel(seed0, w, rows, decks=decks, max_steps=120)
    stale = HeuristicVecEnvModel(seed0, w, rows, decks=decks, max_steps=120)
    rs = np.random.RandomState(5)
    diverged = False
    for t in range(80):
        if t == 20:
            rows2 = (np.arange(n) % 4) + 4   # the other half of the league ...
            w2 = w[::-1].copy()               # ... through a reordered table: rows2 now name the first four individuals
            env.set_opponents(w2, rows2)
            model.set_opponents(w2, rows2)
        a = random_legal(rs, model.views["legal"])
        got = host_views(env.step(torch.from_numpy(a).cuda()))
        want = model.step(a)
        assert_views_equal(got, want, f"step {t}")
        assert np.array_equal(env.state_hash(), model.hashes()), t
        if not diverged:   # until they part, the stale twin's slots are in the model's states: the same actions are legal
            stale.step(a)
            diverged = not np.array_equal(stale.hashes(), model.hashes())
            assert t >= 20 or not diverged, t
    assert diverged
    env.close()


def test_error_paths():
    torch = _torch()
    from monsoon_amd import MonsoonError, _lib
    from monsoon_amd.vec_env import VecEnv
    n = 8
    seed0 = np.arange(n, dtype=np.uint32)
    deck = np.stack([deck_indices("N12M")] * 2)
    w = league(4)
    env = VecEnv(n)
    # opponent 2 without monsoon_env_set_opponents: MONSOON_ERR_STATE
    from monsoon_amd._lib import EnvConfig, EnvViews
    cfg = EnvConfig()
    cfg.opponent = 2
    done = torch.zeros(n, dtype=torch.uint8, device="cuda")
    views = EnvViews(done=done.data_ptr())
    decks = np.ascontiguousarray(np.broadcast_to(deck, (n, 2, 12)))
    rc = env.engine.lib.monsoon_env_reset(env.engine.h, ctypes.byref(cfg), ctypes.byref(views), n,
                                          seed0.ctypes.data_as(ctypes.c_void_p), decks.ctypes.data_as(ctypes.c_void_p), None)
    assert rc == _lib.ERR_STATE
    with pytest.raises(ValueError, match="opponent_weights"):
        env.reset(seed0, deck, opponent="heuristic")
    # a row outside the table, an n other than reset's
    with pytest.raises(MonsoonError, match="row outside"):
        env.engine.env_set_opponents(w, np.full(n, 4, dtype=np.int32), n)
    env.engine.env_set_opponents(w, None, n - 1)
    with pytest.raises(MonsoonError, match="differs"):
        env.engine.env_reset(cfg, views, seed0, decks)
    env.reset(seed0, deck, opponent="heuristic", opponent_weights=w, opponent_rows=np.arange(n) % 4)
    with pytest.raises(MonsoonError, match="differs"):
        env.engine.env_set_opponents(w, None, n - 1)
    # more rows than at reset: refused while the env is loaded; fewer or as many: accepted
    with pytest.raises(MonsoonError, match="more weight rows"):
        env.engine.env_set_opponents(league(5), None, n)
    env.set_opponents(w[:2], np.arange(n) % 2)
    env.step(torch.full((n,), 155, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        env.set_opponents(w, np.arange(n + 1) % 4)
    env.close()
