"""GPU tests of the vector env on the large record build (VecEnv(extended=2): k_env_step, k_env_init, k_env_reseed,
k_env_view, k_env_opp<8,1>, k_env_after<8,1>, k_env_save, k_env_load of libmonsoon_hip_big): every view, state hash,
afterstate and saved byte against the Python models over the recursive core's large build (oracle_lib.Oracle(extended=2)).
All comparisons are exact: integers, observation words, f64 bit patterns, entry bytes.

N = 21 slots: a workgroup of the lane-per-game env kernels serves API_LANES = 8 slots on this build, so 21 slots are three
workgroups, the last with five live lanes -- the guard g >= n runs on three lanes and blocks 1 and 2 index their own
work-stack overflow blocks.  21 is odd too: the copy kernels' workgroups of four wavefronts end on a single entry."""
import ctypes

import numpy as np
import pytest

from c5_games import C5_OVERFLOWING, c5_games
from env_afterstates_model import AfterstatesModel, History, compare_slot
from env_snapshot_model import EnvSnapshotModel, build_entry, entry_layout
from monsoon_amd.cards import observable_pool
from test_vec_env_gpu import assert_guard_only_on_endless_turns, assert_views_equal, host_views, random_legal
from test_vec_env_heuristic_gpu import assert_guard_only_on_endless_turns as assert_opp_guard_only_on_endless_turns
from test_vec_env_heuristic_gpu import league
from vec_env_heuristic_model import HeuristicVecEnvModel
from vec_env_model import VecEnvModel

pytestmark = pytest.mark.gpu

N = 21
MAX_STEPS = 100
# record limits (msb_base.h): entity slots / trigger stack / status count / memory lists / deck / hand / path / strength.
# Stricter than "16 and above, not the recursion guard 18": the stream overrun (19), an unsupported card (20) and the
# env's own turn guards (27, 28) are no limits of the record either.
CAPACITY_CODES = (16, 17, 21, 22, 23, 24, 25, 26)

# Deck pairs of C5 games whose nested b005 memories outgrew the extended record in self-play (tests/c5_games.py; 2063 and
# 6149 outgrow the large record too and are left out).  Slot i plays pair i % 18 from seed GAMES_SEED0 + 7919 * i against
# the scripted bot with the random policy RandomState(GAMES_POLICY), whose draws for a slot depend on the slot's index
# alone.  The seeds of slots 7, 10 and 17 were searched on the CPU with the loop of large_games_case() below (480 seeds a
# slot, eight hits): with them the extended record ends the slot's episode on a record limit where the large one plays on.
GAMES = [k for k in C5_OVERFLOWING if k not in (2063, 6149)]
GAMES_SEED0, GAMES_POLICY = 17, 0
GAMES_SEED_OF = {7: 97000308 + 7 * 7919, 10: 12000053 + 10 * 7919, 17: 373001136 + 17 * 7919}


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _i32(torch, xs):
    return torch.tensor(list(xs), dtype=torch.int32, device="cuda")


def games_decks(n=N):
    _, pairs = c5_games(GAMES)
    return np.stack([pairs[i % len(GAMES)] for i in range(n)])


def games_seed0(n=N):
    seed0 = (np.arange(n, dtype=np.uint32) * 7919 + GAMES_SEED0).astype(np.uint32)
    for i, s in GAMES_SEED_OF.items():
        if i < n:
            seed0[i] = s
    return seed0


def lockstep(torch, env, model, steps, rs, ctx, trail=None):
    """Random-legal actions from the model's legal bytes; every view and every state hash equal at every step.  Returns
    (episodes ended, ended on a fault)."""
    ends = faults = 0
    for t in range(steps):
        a = random_legal(rs, model.views["legal"])
        if trail is not None:
            trail.append(a)
        got = host_views(env.step(torch.from_numpy(a).cuda()))
        want = model.step(a)
        assert_views_equal(got, want, f"{ctx} step {t}")
        assert np.array_equal(env.state_hash(), model.hashes()), (ctx, t)
        ends += int(got["done"].sum())
        faults += int((got["done"] & (got["fault"] != 0)).sum())
    return ends, faults


def test_pool_decks_lockstep_with_the_bot():
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    pool = observable_pool()
    assert len(pool) == 109
    seed0 = (np.arange(N, dtype=np.uint32) * 13 + 9000).astype(np.uint32)
    env = VecEnv(N, extended=2)
    views = env.reset(seed0, pool=pool, opponent="expert", agent_side=1, max_steps=MAX_STEPS)
    model = VecEnvModel(seed0, pool=pool, opponent=1, agent_side=1, max_steps=MAX_STEPS, extended=2)
    assert_views_equal(host_views(views), model.views, "reset")
    assert np.array_equal(env.state_hash(), model.hashes())
    ends, _ = lockstep(torch, env, model, 100, np.random.RandomState(8), "pool")
    assert_guard_only_on_endless_turns(model)
    # auto-reset: episodes ended and the slots went on into their next ones
    assert ends > 0 and model.episode.max() >= 1 and int(host_views(env.views)["episode"].max()) >= 1
    env.close()


def large_games_case():
    """The CPU side of the games that need the large record: the model over Oracle(extended=2) plays 100 random-legal
    steps; a twin over Oracle(extended=1) is given the same actions.  Until a slot's twin ends an episode the two are in
    the same state; a slot NEEDS the large record when its twin's first end is a record limit (CAPACITY_CODES) at a step
    where the large model's slot goes on, or ends without a fault.  Returns (actions of every step, slots that needed it)."""
    decks = games_decks()
    seed0 = games_seed0()
    kw = dict(opponent=1, agent_side=1, max_steps=MAX_STEPS)
    big = VecEnvModel(seed0, decks, extended=2, **kw)
    ext = VecEnvModel(seed0, decks, extended=1, **kw)
    rs = np.random.RandomState(GAMES_POLICY)
    together = np.array([big.hashes()[j] == ext.hashes()[j] and ext.result[j] == big.result[j] for j in range(N)])
    needed, trail = [], []
    for t in range(100):
        a = random_legal(rs, big.views["legal"])
        trail.append(a)
        vb = {k: v.copy() for k, v in big.step(a).items()}
        ve = ext.step(np.where(together, a, 255).astype(np.uint8))
        for j in np.nonzero(together)[0]:
            if ve["done"][j] or vb["done"][j] or big.hashes()[j] != ext.hashes()[j]:
                together[j] = False
                if ve["done"][j] and int(ve["fault"][j]) in CAPACITY_CODES and int(vb["fault"][j]) == 0:
                    needed.append(int(j))
    return trail, needed


def test_games_that_need_the_large_record():
    """Fixed deck pairs whose b005 memories nest: the wide trigger-source word, slot ids above 63 and nested worlds are
    live in the env kernels here and nowhere else."""
    trail, needed = large_games_case()
    assert len(needed) >= 2, needed   # on the CPU, before the device is touched: the extended record ends these slots
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    decks, seed0 = games_decks(), games_seed0()
    env = VecEnv(N, extended=2)
    views = env.reset(seed0, decks, opponent="expert", agent_side=1, max_steps=MAX_STEPS)
    model = VecEnvModel(seed0, decks, opponent=1, agent_side=1, max_steps=MAX_STEPS, extended=2)
    assert_views_equal(host_views(views), model.views, "reset")
    assert np.array_equal(env.state_hash(), model.hashes())
    mine = []
    ends, _ = lockstep(torch, env, model, len(trail), np.random.RandomState(GAMES_POLICY), "games", mine)
    assert all(np.array_equal(x, y) for x, y in zip(mine, trail))   # the run the precondition was shown for
    assert_guard_only_on_endless_turns(model)
    assert ends > 0 and model.episode.max() >= 1
    env.close()


class _Counted:
    """Counts what monsoon_debug_counters words 6 / 7 / 16 count, on the model: the agent's and the opponent's committed
    steps and the opponent's look-ahead transitions (one per legal action of every decision, oracle.cpp decide)."""

    def __init__(self):
        self.commits = self.agent = self.lookahead = 0

    def on_commit(self, j, episode, action, canon_hash):
        self.commits += 1

    def on_decide(self, j, action, mask):
        self.lookahead += sum(bin(int(x)).count("1") for x in mask)


@pytest.mark.parametrize("agent_side", [0, 1])
def test_heuristic_opponent_lockstep(agent_side):
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    steps = 60
    pool = observable_pool()
    seed0 = (np.arange(N, dtype=np.uint32) * 13 + 7000 + 500 * agent_side).astype(np.uint32)
    w = league(2)
    rows = np.arange(N) % 2
    cnt = _Counted()   # (the opening turns of agent_side 1 are played, and counted, inside the model's constructor)
    model = HeuristicVecEnvModel(seed0, w, rows, pool=pool, agent_side=agent_side, max_steps=MAX_STEPS, extended=2,
                                 on_commit=cnt.on_commit, on_decide=cnt.on_decide)
    env = VecEnv(N, extended=2)
    views = env.reset(seed0, pool=pool, opponent="heuristic", agent_side=agent_side, max_steps=MAX_STEPS, opponent_weights=w,
                      opponent_rows=rows)
    assert_views_equal(host_views(views), model.views, "reset")
    assert np.array_equal(env.state_hash(), model.hashes())
    rs = np.random.RandomState(8 + agent_side)
    ends = 0
    for t in range(steps):
        cnt.agent += int((model.result == -2).sum())   # the policy gives every live slot a legal action
        a = random_legal(rs, model.views["legal"])
        got = host_views(env.step(torch.from_numpy(a).cuda()))
        assert_views_equal(got, model.step(a), f"step {t}")
        assert np.array_equal(env.state_hash(), model.hashes()), t
        ends += int(got["done"].sum())
    assert_opp_guard_only_on_endless_turns(model)
    assert ends > 0 and model.episode.max() >= 1
    out = (ctypes.c_ulonglong * 192)()
    assert env.engine.lib.monsoon_debug_counters(env.engine.h, out) == 0
    print(f"agent steps {out[6]}, opponent steps {out[7]}, look-ahead transitions {out[16]}")
    assert (int(out[6]), int(out[7]), int(out[16])) == (cnt.agent, cnt.commits - cnt.agent, cnt.lookahead)
    env.close()


def test_afterstates_lockstep():
    """The deck pairs and seeds of the games case with opponent none (the caller acts for both sides, so b005 is played by
    either): a sample of (slot, step) pairs against AfterstatesModel, and purity of every call."""
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    decks, seed0 = games_decks(), games_seed0()
    env = VecEnv(N, extended=2)
    env.reset(seed0, decks, opponent="none", agent_side=0, max_steps=50)
    hist = History()
    model = VecEnvModel(seed0, decks, opponent=0, agent_side=0, max_steps=50, extended=2, on_commit=hist)
    am = AfterstatesModel(model, hist, extended=2)
    rs = np.random.RandomState(GAMES_POLICY + 1)
    entries = second_pass = 0   # counted on the model: 2 367 entries, 88 slots with a second pass for these seeds
    for t in range(24):
        h0 = env.state_hash()
        got = host_views(env.afterstates(156))
        assert np.array_equal(env.state_hash(), h0), t   # purity: the call changes no slot
        for j in np.nonzero(rs.random_sample(N) < 0.35)[0]:
            want = am.slot(j, 156)
            entries += compare_slot(want, got, j, 156, ("large", t, j))
            second_pass += want["n_legal"] > 8   # more legal actions than the eight candidate lanes of k_env_after<8,1>
        a = random_legal(rs, model.views["legal"])
        model.step(a)
        env.step(torch.from_numpy(a).cuda())
        assert np.array_equal(env.state_hash(), model.hashes()), t
    assert entries > 0 and second_pass > 0, (entries, second_pass)
    env.close()


# ---- snapshot, restore, fork ---------------------------------------------------------------------------------------------
def _spec(seed, **kw):
    seed0 = (np.arange(N, dtype=np.uint32) * 104729 + seed).astype(np.uint32)
    return dict(seed0=seed0, decks=games_decks(), extended=2, **kw)


def _open(spec):
    from monsoon_amd.vec_env import VecEnv
    env = VecEnv(N, extended=2)
    env.reset(spec["seed0"], spec["decks"], opponent=("none", "expert")[spec["opponent"]], agent_side=spec.get("agent_side", 0),
              max_steps=spec["max_steps"], seed_stride=spec.get("seed_stride", 0))
    return env


def _helper_lockstep(torch, env, helper, steps, rs, ctx):
    sel = np.array(helper.slots)
    ends = 0
    for t in range(steps):
        a = np.full(env.n, 255, dtype=np.uint8)
        a[sel] = random_legal(rs, helper.views()["legal"])
        got = host_views(env.step(torch.from_numpy(a).cuda()), sel)
        assert_views_equal(got, helper.step(a[sel]), f"{ctx} step {t}")
        assert np.array_equal(env.state_hash()[sel], helper.hashes()), (ctx, t)
        ends += int(got["done"].sum())
    return ends


def test_saved_entries_byte_for_byte():
    """Every byte of every saved entry: the header, the meta row, the decks, and all 989 body granules -- both passes of the
    copy loop, the 29-lane tail, the seams record | rng_mt | rng_out -- against the entry put together from
    monsoon_state_save's blob of the slot (k_blob: another kernel, word by word) and the model's episode count and decks."""
    torch = _torch()
    lay = entry_layout(2)
    spec = _spec(23, opponent=1, agent_side=0, max_steps=30)
    env = _open(spec)
    model = VecEnvModel(**spec)
    lockstep(torch, env, model, 35, np.random.RandomState(4), "before")   # past max_steps: later episodes, re-seeded streams
    assert model.episode.max() >= 1
    assert env.entry_bytes == lay["entry_bytes"] and (lay["passes"], lay["tail_granules"]) == (2, 349)
    order = [20, 3, 3, 0, 17, 8, 11]   # out of order, one slot twice, seven entries: no multiple of the four wavefronts
    version = env.engine.lib.monsoon_version()
    for slots in (None, order):
        snap = env.snapshot(None if slots is None else _i32(torch, slots))
        data = snap.data.cpu().numpy()
        assert data.shape == (N if slots is None else len(order), lay["entry_bytes"])
        for j, s in enumerate(range(N) if slots is None else slots):
            want = build_entry(2, version, model.episode[s], model.decks[s], env.engine.save_state(s))
            if not np.array_equal(data[j], want):
                bad = np.nonzero(data[j] != want)[0]
                raise AssertionError(f"entry {j} (slot {s}): {len(bad)} bytes differ, first at {bad[0]} (granule {(bad[0] - 80) // 16} of "
                                     f"the body; rng_mt starts at byte {lay['mt_at']}, rng_out at {lay['out_at']})")
        # the parts are not trivially equal: no stretch of the body that a pass, the tail or a seam covers is all zero
        for lo, hi in ((80, 80 + 640 * 16), (80 + 640 * 16, lay["entry_bytes"]), (lay["entry_bytes"] - 29 * 16, lay["entry_bytes"]),
                       (lay["mt_at"] - 16, lay["mt_at"] + 16), (lay["out_at"] - 16, lay["out_at"] + 16)):
            assert data[:, lo:hi].any(axis=1).all(), (lo, hi)
    env.close()


def test_rewind_replays_bit_for_bit():
    torch = _torch()
    spec = _spec(11, opponent=1, agent_side=0, max_steps=40)
    env = _open(spec)
    model = VecEnvModel(**spec)
    rs = np.random.RandomState(11)
    lockstep(torch, env, model, 25, rs, "before")
    snap = env.snapshot()
    views0, hash0 = host_views(env.views), env.state_hash()
    trail, first = [], []
    for t in range(30):
        a = random_legal(rs, model.views["legal"])
        got = host_views(env.step(torch.from_numpy(a).cuda()))
        assert_views_equal(got, model.step(a), f"step {25 + t}")
        trail.append(a)
        first.append(got)
    hash1 = env.state_hash()
    assert np.array_equal(hash1, model.hashes())
    assert sum(int(g["done"].sum()) for g in first) > 0 and not np.array_equal(hash0, hash1)
    loaded = torch.zeros(N, dtype=torch.uint8, device="cuda")
    got = host_views(env.restore(snap, loaded=loaded))
    assert loaded.cpu().numpy().tolist() == [1] * N
    want = dict(views0)
    for k, v in dict(reward=0, done=0, winner=-2, truncated=0, fault=0, illegal=0, final_hash=0).items():
        want[k] = np.full_like(views0[k], v)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), ("restored views", k)
    assert np.array_equal(env.state_hash(), hash0)
    for t in range(30):
        again = host_views(env.step(torch.from_numpy(trail[t]).cuda()))
        for k in again:
            assert np.array_equal(again[k], first[t][k]), ("replayed step", t, k)
    assert np.array_equal(env.state_hash(), hash1)
    env.close()


def test_fork_and_load_into_another_handle():
    torch = _torch()
    spec_a = _spec(17, opponent=0, max_steps=24)
    spec_b = _spec(99991, opponent=0, max_steps=20, seed_stride=1000)
    spec_b["decks"] = spec_b["decks"][::-1].copy()
    env_a, env_b = _open(spec_a), _open(spec_b)
    help_a, help_b = EnvSnapshotModel(spec_a), EnvSnapshotModel(spec_b, slots=[0, 6, 13, 20])
    rs = np.random.RandomState(2)
    _helper_lockstep(torch, env_a, help_a, 9, rs, "a")
    _helper_lockstep(torch, env_b, help_b, 3, rs, "b")
    roots = [5, 17, 12]
    snap, model_snap = env_a.snapshot(_i32(torch, roots)), help_a.snapshot(roots)
    # the fork: entry 0 into three slots, entry 2 into two; dst out of order and not contiguous; two pairs that are skipped
    src, dst = [0, 2, 0, 1, 2, 0, 7, -1], [19, 1, 2, 20, 9, 4, 6, 8]
    before, hash0 = host_views(env_a.views), env_a.state_hash()
    loaded = torch.full((8,), 9, dtype=torch.uint8, device="cuda")
    got = host_views(env_a.restore(snap, _i32(torch, src), _i32(torch, dst), loaded))
    assert loaded.cpu().numpy().tolist() == [1, 1, 1, 1, 1, 1, 0, 0]
    assert help_a.restore(model_snap, src, dst).tolist() == [1, 1, 1, 1, 1, 1, 0, 0]
    hash1 = env_a.state_hash()
    rest = np.setdiff1d(np.arange(N), dst[:6])
    for k in got:
        assert np.array_equal(got[k][rest], before[k][rest]), ("untouched slots", k)
    assert np.array_equal(hash1[rest], hash0[rest])
    for s, d in zip(src[:6], dst[:6]):
        assert hash1[d] == hash0[roots[s]]
    assert_views_equal(got, help_a.views(), "restored")
    assert np.array_equal(hash1, help_a.hashes())
    # the destination keeps its own configuration: across the end of the forked episode into the destination's schedule
    ends = _helper_lockstep(torch, env_a, help_a, 30, rs, "forks")
    assert ends > 0 and help_a.episodes()[dst[:6]].min() >= 1
    # the same entries into a second handle of the large build, with another stride and step limit
    torch.cuda.synchronize()
    loaded = torch.zeros(2, dtype=torch.uint8, device="cuda")
    env_b.restore(snap, _i32(torch, [1, 0]), _i32(torch, [13, 6]), loaded)
    assert loaded.cpu().numpy().tolist() == [1, 1]
    assert help_b.restore(model_snap, [1, 0], [13, 6]).tolist() == [1, 1]
    assert_views_equal(host_views(env_b.views, np.array(help_b.slots)), help_b.views(), "loaded into b")
    hb = env_b.state_hash()
    assert hb[13] == hash0[17] and hb[6] == hash0[5]
    _helper_lockstep(torch, env_b, help_b, 25, rs, "b after the load")
    assert help_b.episodes()[1:3].min() >= 1
    env_a.close()
    env_b.close()


def test_entries_of_another_build_are_refused():
    torch = _torch()
    from monsoon_amd import EnvSnapshot
    from monsoon_amd.vec_env import VecEnv
    n = 5
    seed0 = np.arange(n, dtype=np.uint32) + 9
    decks = games_decks(n)
    big, ext = VecEnv(n, extended=2), VecEnv(n, extended=1)
    big.reset(seed0, decks)
    ext.reset(seed0, decks)
    snap_big, snap_ext = big.snapshot(), ext.snapshot()
    assert (snap_big.extended, snap_ext.extended) == (2, 1)
    assert (snap_big.entry_bytes, snap_ext.entry_bytes) == (entry_layout(2)["entry_bytes"], entry_layout(1)["entry_bytes"])
    for env, other in ((big, snap_ext), (ext, snap_big)):
        with pytest.raises(ValueError, match="build"):
            env.restore(other)
        with pytest.raises(ValueError, match="build"):
            env.snapshot(out=other)
        with pytest.raises(ValueError):   # relabelled: the entry size still gives it away
            env.restore(EnvSnapshot(other.data, other.count, int(env.extended), other.entry_bytes))
    # the device's own check (the loaded byte): the other build's entries behind this build's stride.  The buffers hold
    # n entries of the LARGER size, so every read of either kernel stays inside them.
    size = snap_big.entry_bytes
    torch.cuda.synchronize()
    for env, foreign in ((big, snap_ext), (ext, snap_big)):
        buf = torch.zeros(n * size, dtype=torch.uint8, device="cuda")
        flat = foreign.data.reshape(-1)
        buf[:flat.numel()] = flat
        h0, v0 = env.state_hash(), host_views(env.views)
        loaded = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc = env.engine.lib.monsoon_env_load_dev(env.engine.h, ctypes.c_void_p(buf.data_ptr()), 1, None, None, 1, ctypes.c_void_p(loaded.data_ptr()))
        assert rc == 0
        env.engine.sync()
        assert loaded.cpu().numpy().tolist() == [0, 9, 9, 9, 9]   # entry 0 carries the other build's record size: skipped
        assert np.array_equal(env.state_hash(), h0)
        for k, v in host_views(env.views).items():
            assert np.array_equal(v, v0[k]), k
    big.close()
    ext.close()
