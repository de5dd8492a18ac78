"""GPU tests of the afterstates (monsoon_env_afterstates_dev, VecEnv.afterstates / select_actions): every output in
lockstep with the Python model of the contract (tests/env_afterstates_model.py, over the CPU oracle) on the three record
builds, purity, consistency with the step that commits the action, truncation by max_after, the reference's agent rebuilt
from the afterstate features, graph capture, and the error paths.  All comparisons are exact (floats by bit pattern)."""
import ctypes

import numpy as np
import pytest

import heuristic_model
import oracle_lib
from env_afterstates_model import AfterstatesModel, History, compare_slot
from monsoon_amd.cards import CARD_IDS, DECKS, FAULT_CARDS, UNSUPPORTED, deck_indices
from test_vec_env_gpu import _graph_is_a_chain, host_views, mixed_decks, random_legal
from vec_env_model import FAULT_INT_CARD, VecEnvModel

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def pool107():
    """Every card of the standard record but the three whose int(card) raises."""
    return np.array([i for i, c in enumerate(CARD_IDS) if c not in UNSUPPORTED and c not in FAULT_CARDS], dtype=np.uint8)


def pool110():
    """... and with them: up01 / up02 / up03 make get_observation raise wherever they are visible."""
    return np.array([i for i, c in enumerate(CARD_IDS) if c not in UNSUPPORTED], dtype=np.uint8)


def n12m(n):
    """N12M against N12M; in every fourth slot SECOND's deck holds up01: FIRST's PASS hands over to an observation that raises."""
    plain = np.stack([deck_indices("N12M")] * 2)
    up01 = np.stack([deck_indices("N12M"), deck_indices(DECKS["N12M"][:11] + ["up01"])])
    return np.stack([up01 if i % 4 == 3 else plain for i in range(n)])


# name -> (extended, n slots, steps, share of the (slot, step) pairs whose afterstates are compared, reset arguments).
# The model replays a slot's episode once per legal action (O(steps^2) per slot): small envs.  "fault_cards": the 110-card
# pool with up01 / up02 / up03: episodes whose first observation raises end before the agent acts (n_legal = 0); "ext":
# b005 / ua20 forced into fixed decks on the extended record.
def _ext_decks(n):
    d = DECKS["N12M"]
    a = deck_indices(d[:10] + ["b005", "ua20"])
    return np.stack([np.stack([a, a])] * n)


LOCKSTEP = {
    "none_n12m": (0, 64, 40, 1.0, dict(decks="n12m", opponent=0, agent_side=0)),
    "expert0_pool": (0, 64, 40, 1.0, dict(pool="107", opponent=1, agent_side=0)),
    "expert1_fault_cards": (0, 64, 40, 1.0, dict(pool="110", opponent=1, agent_side=1)),
    "ext_b005_ua20": (1, 32, 30, 1.0, dict(decks="ext", opponent=0, agent_side=0)),
    "big_small": (2, 8, 16, 1.0, dict(decks="ext", opponent=1, agent_side=0)),
}


def _case_args(name):
    ext, n, steps, share, kw = LOCKSTEP[name]
    seed0 = (np.arange(n, dtype=np.uint32) * 2654435 + 97 + 1000 * sorted(LOCKSTEP).index(name)).astype(np.uint32)
    decks = {"n12m": n12m, "ext": _ext_decks}[kw["decks"]](n) if "decks" in kw else None
    pool = {"107": pool107, "110": pool110}[kw["pool"]]() if "pool" in kw else None
    return ext, n, steps, share, seed0, decks, pool, kw["opponent"], kw["agent_side"]


def lockstep_case(name, afterstates=None, step=None):
    """Drives the model of case `name` with a numpy-seeded random policy and compares the sampled afterstates with
    afterstates() -> host dict (None: the model alone, for fixing the seeds on a CPU).  Returns what the compared
    afterstates covered."""
    ext, n, steps, share, seed0, decks, pool, opponent, agent_side = _case_args(name)
    hist = History()
    model = VecEnvModel(seed0, decks, opponent=opponent, agent_side=agent_side, max_steps=50, pool=pool, extended=ext, on_commit=hist)
    am = AfterstatesModel(model, hist, extended=ext)
    rs = np.random.RandomState(sorted(LOCKSTEP).index(name))
    cov = dict(entries=0, step_fault=0, int_card=0, winner=0, passes=0, pending=0)
    for t in range(steps):
        got = afterstates() if afterstates else None
        for j in np.nonzero(rs.random_sample(n) < share)[0]:
            want = am.slot(j, 156)
            if got is not None:
                compare_slot(want, got, j, 156, (name, t, j))
            cov["entries"] += len(want["entries"])
            cov["step_fault"] += sum(e["status"] not in (0, FAULT_INT_CARD) for e in want["entries"])
            cov["int_card"] += sum(e["status"] == FAULT_INT_CARD for e in want["entries"])
            cov["winner"] += sum(e["winner"] != -2 for e in want["entries"])
            cov["passes"] += want["n_legal"] > 8
            cov["pending"] += model.result[j] != -2
        a = random_legal(rs, model.views["legal"])
        model.step(a)
        if step:
            step(a, model)
    return cov


@pytest.mark.parametrize("name", sorted(LOCKSTEP))
def test_lockstep_with_model(name):
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    ext, n, steps, share, seed0, decks, pool, opponent, agent_side = _case_args(name)
    env = VecEnv(n, extended=ext)
    env.reset(seed0, decks, opponent=("none", "expert")[opponent], agent_side=agent_side, max_steps=50, pool=pool)

    def afterstates():
        return host_views(env.afterstates(156))

    def step(a, model):
        env.step(torch.from_numpy(a).cuda())
        assert np.array_equal(env.state_hash(), model.hashes())

    cov = lockstep_case(name, afterstates, step)
    print(name, cov)
    env.close()
    # what the compared afterstates must include (checked on the CPU model when the seeds were fixed)
    assert cov["entries"] > 0 and cov["passes"] > 0, cov
    if name == "none_n12m":
        assert cov["winner"] > 0 and cov["int_card"] > 0, cov
    if name == "expert1_fault_cards":
        assert cov["pending"] > 0, cov
    if name in ("expert0_pool", "expert1_fault_cards"):
        assert cov["step_fault"] > 0, cov


def _twin_stream(torch, n, steps, seed0, decks, with_after):
    from monsoon_amd.vec_env import VecEnv, select_actions
    env = VecEnv(n)
    views = env.reset(seed0, decks, opponent="expert", agent_side=0, max_steps=80)
    acc = torch.zeros(n, dtype=torch.int64, device="cuda")
    for t in range(steps):
        if with_after:
            if t % 50 == 0:
                h0 = env.state_hash()
            after = env.afterstates(16, obs=(t % 2 == 0))
            if t % 50 == 0:
                assert np.array_equal(env.state_hash(), h0), t
            del after
        a = views["legal"].to(torch.uint8).argmax(dim=1).to(torch.uint8)   # the first legal action
        views = env.step(a)
        acc = acc * 1000003 + views["done"].to(torch.int64) + views["winner"].to(torch.int64) * 3 + views["final_hash"] * 5 + \
            views["episode"].to(torch.int64) * 7
    torch.cuda.synchronize()
    out = acc.cpu().numpy(), env.state_hash(), int(views["episode"].min())
    env.close()
    return out


def test_purity():
    """state_hash() is the same before and after the call, and an env that asks for afterstates every step produces the
    done / winner / final_hash / episode streams of a twin that never does (any change of a record, a stream cursor, a
    stream block or a meta row would move them apart)."""
    torch = _torch()
    n, steps = 65536, 300
    seed0 = np.arange(n, dtype=np.uint32) + 40000
    decks = mixed_decks(n)
    acc1, hash1, ep1 = _twin_stream(torch, n, steps, seed0, decks, True)
    acc2, hash2, ep2 = _twin_stream(torch, n, steps, seed0, decks, False)
    assert np.array_equal(acc1, acc2) and np.array_equal(hash1, hash2) and ep1 == ep2 and ep1 >= 1


def test_commit_consistency():
    """Opponent none: the observation of the action actually played is the observation the step then reports, wherever the
    episode went on; where it ended by a winner, the afterstate's winner is the step's."""
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    n, steps = 2048, 120
    seed0 = np.arange(n, dtype=np.uint32) * 3 + 7
    env = VecEnv(n)
    views = env.reset(seed0, mixed_decks(n))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    went_on = won = 0
    for t in range(steps):
        after = env.afterstates(156)
        k = (torch.rand(n, device="cuda", generator=gen) * after["n_legal"]).to(torch.int64).clamp(max=155)
        pending = after["n_legal"] == 0
        a = torch.where(pending, torch.full((n,), 255, dtype=torch.uint8, device="cuda"), after["action"].gather(1, k[:, None])[:, 0])
        obs_k = after["obs"][torch.arange(n, device="cuda"), k].clone()
        win_k = after["winner"].gather(1, k[:, None])[:, 0].clone()
        st_k = after["status"].gather(1, k[:, None])[:, 0].clone()
        views = env.step(a)
        assert not bool(views["illegal"].any())
        live = ~views["done"] & ~pending
        assert bool((st_k[live] == 0).all())
        assert torch.equal(obs_k[live], views["obs"][live]), t
        ended = views["done"] & ~pending & (views["fault"] == 0) & ~views["truncated"]
        assert torch.equal(win_k[ended], views["winner"][ended]), t
        assert bool((win_k[live] == -2).all())
        went_on += int(live.sum())
        won += int(ended.sum())
    assert went_on > 1000 and won > 50, (went_on, won)
    env.close()


@pytest.mark.parametrize("k", [1, 8, 9])
def test_truncation(k):
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    n = 1024
    env = VecEnv(n)
    views = env.reset(np.arange(n, dtype=np.uint32) + 321, mixed_decks(n))
    for _ in range(6):
        views = env.step(views["legal"].to(torch.uint8).argmax(dim=1).to(torch.uint8))
    full = host_views(env.afterstates(156))
    part = host_views(env.afterstates(k))
    assert np.array_equal(part["n_legal"], full["n_legal"]) and (full["n_legal"] > 9).any() and (full["n_legal"] < 8).any()
    assert np.array_equal(part["before_features"], full["before_features"])
    shown = np.arange(k)[None, :] < full["n_legal"][:, None]
    assert np.array_equal(part["action"], np.where(shown, full["action"][:, :k], 255))
    for name in ("status", "reward", "winner"):
        assert np.array_equal(part[name][shown], full[name][:, :k][shown]), name
    ok = shown & (full["status"][:, :k] == 0)
    assert np.array_equal(part["features"][ok].view(np.uint64), full["features"][:, :k][ok].view(np.uint64))
    assert np.array_equal(part["obs"][ok], full["obs"][:, :k][ok])
    env.close()


def test_against_the_agent():
    """Both sides driven by heuristic_model's score over the afterstate features (status != 0 or a raising "before"
    observation -> 0.0, first maximum): the committed-state hashes follow Oracle.rollout(trace=True)."""
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    n, max_turns = 16, 60
    rs = np.random.RandomState(77)
    w = rs.uniform(-1.0, 1.0, (2, 10))
    seed0 = np.arange(n, dtype=np.uint32) * 17 + 5
    decks = mixed_decks(n)
    orc = oracle_lib.Oracle(n)
    traces = []
    for i in range(n):
        orc.reset(i, seed0[i], decks[i, 0], decks[i, 1])
        traces.append(orc.rollout(i, w[0], w[1], max_turns, trace=True))
    env = VecEnv(n)
    views = env.reset(seed0, decks)
    score = heuristic_model.ScoreCache()
    followed = 0
    for t in range(max_turns):
        after = host_views(env.afterstates(156))
        to_play = views["to_play"].cpu().numpy()
        raises = views["obs_raises"].cpu().numpy()
        a = np.full(n, 255, dtype=np.uint8)
        for i in range(n):
            if t >= traces[i]["steps"]:
                continue   # the rollout of this game is over: the slot is left alone
            nl = int(after["n_legal"][i])
            s = [score(w[to_play[i]], after["before_features"][i], after["features"][i, k])
                 if (after["status"][i, k] == 0 and not raises[i]) else 0.0 for k in range(nl)]
            a[i] = after["action"][i, heuristic_model.first_max(s)]
            assert a[i] == traces[i]["actions"][t], (t, i)
        views = env.step(torch.from_numpy(a).cuda())
        h = env.state_hash()
        for i in range(n):
            if t < traces[i]["steps"] and not bool(views["done"][i]):
                assert h[i] == traces[i]["hashes"][t], (t, i)
                followed += 1
        if bool(views["done"].any()):   # a finished game's slot restarts: stop following it
            for i in np.nonzero(views["done"].cpu().numpy())[0]:
                traces[i]["steps"] = min(traces[i]["steps"], t + 1)
    assert followed > 300, followed
    env.close()


def test_graph_capture_single_stream():
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv, select_actions
    n = 4096
    seed0 = np.arange(n, dtype=np.uint32) + 31
    decks = mixed_decks(n)
    a_env, b_env = VecEnv(n), VecEnv(n)
    a_env.reset(seed0, decks, opponent="expert", agent_side=0, max_steps=60)
    b_env.reset(seed0, decks, opponent="expert", agent_side=0, max_steps=60)
    s = a_env.stream
    wts = torch.linspace(-1.0, 1.0, 10, dtype=torch.float64, device="cuda")

    def policy(after):   # a torch "network" over the successors' features and observations
        v = (after["features"] * wts).sum(dim=2) + (after["obs"][:, :, 1].sum(dim=(2, 3)) % 7).to(torch.float64)
        return select_actions(after, torch.nan_to_num(v))

    actions = torch.zeros(n, dtype=torch.uint8, device="cuda")
    with torch.cuda.stream(s):   # warm-up outside the graph: the afterstate tensors are allocated here
        actions.copy_(policy(a_env.afterstates(32)))
        va = a_env.step(actions)
    vb = b_env.step(policy(b_env.afterstates(32)))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g, stream=s):
        actions.copy_(policy(a_env.afterstates(32)))
        a_env.step(actions)
    nodes, edges = _graph_is_a_chain(torch, g)
    assert nodes >= 5 and edges == nodes - 1, (nodes, edges)
    g.instantiate()
    for t in range(40):
        g.replay()
        vb = b_env.step(policy(b_env.afterstates(32)))
        torch.cuda.synchronize()
        for k in va:
            assert torch.equal(va[k], vb[k]), (t, k)
        assert not bool(va["illegal"].any())
        assert np.array_equal(a_env.state_hash(), b_env.state_hash()), t
    assert int(va["episode"].max()) >= 1
    a_env.close()
    b_env.close()


def test_error_paths():
    torch = _torch()
    from monsoon_amd import MonsoonError, _lib
    from monsoon_amd.engine import BatchEngine
    from monsoon_amd.vec_env import VecEnv
    buf = torch.zeros(8 * 4 + 8 * 4, dtype=torch.uint8, device="cuda")
    out = _lib.EnvAfter(n_legal=buf.data_ptr(), action=buf.data_ptr() + 32)
    eng = BatchEngine(8)
    assert eng.lib.monsoon_env_afterstates_dev(eng.h, ctypes.byref(out), 4) == _lib.ERR_STATE   # no env loaded
    eng.close()
    env = VecEnv(8)
    with pytest.raises(MonsoonError):
        env.afterstates()                                     # before reset
    decks = np.stack([deck_indices("N12M")] * 2)
    env.reset(np.arange(8, dtype=np.uint32), decks)
    lib, h = env.engine.lib, env.engine.h
    assert lib.monsoon_env_afterstates_dev(h, ctypes.byref(out), 4) == _lib.OK
    torch.cuda.synchronize()
    assert (buf[:32].view(torch.int32) > 0).all() and (buf[32:] != 255).any()
    for bad in (0, -1, 157):
        assert lib.monsoon_env_afterstates_dev(h, ctypes.byref(out), bad) == _lib.ERR_ARG
    for bad in (0, 157, 2.0, None):
        with pytest.raises(ValueError):
            env.afterstates(bad)
    assert lib.monsoon_env_afterstates_dev(h, None, 4) == _lib.ERR_ARG
    assert lib.monsoon_env_afterstates_dev(h, ctypes.byref(_lib.EnvAfter(n_legal=buf.data_ptr())), 4) == _lib.ERR_ARG
    assert lib.monsoon_env_afterstates_dev(h, ctypes.byref(_lib.EnvAfter(action=buf.data_ptr())), 4) == _lib.ERR_ARG
    env.engine.reset(np.arange(8, dtype=np.uint32), decks)    # monsoon_reset ends env mode
    assert lib.monsoon_env_afterstates_dev(h, ctypes.byref(out), 4) == _lib.ERR_STATE
    with pytest.raises(MonsoonError):
        env.afterstates()
    env.close()
