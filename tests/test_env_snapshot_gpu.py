"""GPU tests of saving and restoring vector-env slots (monsoon_env_save_dev / monsoon_env_load_dev, VecEnv.snapshot /
restore): a rewind replays bit for bit, a fork follows its source and then the destination's seed schedule and opponent
row -- against the helper model (tests/env_snapshot_model.py: a fresh model of the source slot replays the saved prefix,
no state is copied) -- on both record builds, with a pending end, captured into a graph, across handles, and the guard
rails.  n = 96 slots: 24 workgroups of four wavefronts, and the m of the partial calls (3, 8, 2) is no multiple of four;
an entry is 520 granules on the standard record, no multiple of 64.  Every index that reaches the device is valid or in
the documented skip range."""
import ctypes

import numpy as np
import pytest

from env_snapshot_model import EnvSnapshotModel
from monsoon_amd.cards import CARD_INDEX, DECKS, deck_indices
from test_vec_env_gpu import assert_views_equal, host_views, mixed_decks, random_legal
from test_vec_env_heuristic_gpu import league
from vec_env_model import VecEnvModel

pytestmark = pytest.mark.gpu

PER_CALL = dict(reward=0, done=0, winner=-2, truncated=0, fault=0, illegal=0, final_hash=0)


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _i32(torch, xs):
    return torch.tensor(list(xs), dtype=torch.int32, device="cuda")


def _same(a, b, ctx):
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (ctx, k)


def _rewind(torch, extended, n, decks, before, after, seed):
    """Case 1 / 4: `before` random-legal steps in lockstep with VecEnvModel, a snapshot, `after` recorded steps, a 1:1
    restore, the same `after` action tensors again: every view of every step and the final state hashes are identical."""
    from monsoon_amd.vec_env import VecEnv
    seed0 = (np.arange(n, dtype=np.uint32) * 7919 + seed).astype(np.uint32)
    env = VecEnv(n, extended=extended)
    views = env.reset(seed0, decks, opponent="expert", agent_side=0, max_steps=40)
    model = VecEnvModel(seed0, decks, opponent=1, agent_side=0, max_steps=40, extended=bool(extended))
    assert_views_equal(host_views(views), model.views, "reset")
    rs = np.random.RandomState(seed)
    for t in range(before):
        a = random_legal(rs, model.views["legal"])
        assert_views_equal(host_views(env.step(torch.from_numpy(a).cuda())), model.step(a), f"step {t}")
    assert np.array_equal(env.state_hash(), model.hashes())
    # slots in a later episode carry a stream that k_env_reseed wrote for another seed than the slot's first: the copy of
    # rng_mt and both rng_out blocks is what makes their replay right (the model shows the same on the CPU for these seeds)
    assert model.episode.max() > 0, model.episode
    snap = env.snapshot()
    assert len(snap) == n and snap.data.shape == (n, env.entry_bytes) and env.entry_bytes % 16 == 0
    views0, hash0 = host_views(views), env.state_hash()
    trail, first = [], []
    for t in range(after):
        a = random_legal(rs, model.views["legal"])
        got = host_views(env.step(torch.from_numpy(a).cuda()))
        assert_views_equal(got, model.step(a), f"step {before + t}")
        trail.append(a)
        first.append(got)
    hash1 = env.state_hash()
    assert np.array_equal(hash1, model.hashes())
    assert sum(int(g["done"].sum()) for g in first) > 0 and not np.array_equal(hash0, hash1)
    loaded = torch.zeros(n, dtype=torch.uint8, device="cuda")
    got = host_views(env.restore(snap, loaded=loaded))
    assert loaded.cpu().numpy().tolist() == [1] * n
    want = dict(views0)
    for k, v in PER_CALL.items():
        want[k] = np.full_like(views0[k], v)
    _same(got, want, "restored views")
    assert np.array_equal(env.state_hash(), hash0)
    for t in range(after):
        _same(host_views(env.step(torch.from_numpy(trail[t]).cuda())), first[t], f"replayed step {t}")
    assert np.array_equal(env.state_hash(), hash1)
    env.close()


def test_rewind_replays_bit_for_bit():
    n = 96
    _rewind(_torch(), 0, n, np.stack([deck_indices("N12M")] * 2), 30, 40, 11)


def test_rewind_extended_record():
    torch = _torch()
    deck = deck_indices(DECKS["N12M"][:10] + ["ua20", "b005"])
    _rewind(torch, 1, 16, np.stack([deck, deck]), 25, 25, 5)


def _lockstep(torch, env, helper, steps, rs, ctx):
    """Random-legal actions for the helper's slots, 255 (the slot is left alone) for the others; every view of the tracked
    slots and their state hashes equal the helper model's."""
    sel = np.array(helper.slots)
    ends = 0
    for t in range(steps):
        a = np.full(env.n, 255, dtype=np.uint8)
        a[sel] = random_legal(rs, helper.views()["legal"])
        got = host_views(env.step(torch.from_numpy(a).cuda()), sel)
        want = helper.step(a[sel])
        assert_views_equal(got, want, f"{ctx} step {t}")
        assert np.array_equal(env.state_hash()[sel], helper.hashes()), (ctx, t)
        ends += int(got["done"].sum())
    return ends


def test_fork_follows_source_then_destination_schedule():
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    n = 96
    seed0 = (np.arange(n, dtype=np.uint32) * 104729 + 17).astype(np.uint32)
    spec = dict(seed0=seed0, decks=mixed_decks(n), opponent=0, max_steps=24)
    env = VecEnv(n)
    env.reset(seed0, spec["decks"], opponent="none", max_steps=24)
    helper = EnvSnapshotModel(spec)
    rs = np.random.RandomState(2)
    _lockstep(torch, env, helper, 9, rs, "before")
    roots = [5, 17, 63]
    snap = env.snapshot(_i32(torch, roots))
    assert len(snap) == 3 and snap.data.shape == (3, env.entry_bytes)
    src, dst = [0, 0, 0, 1, 2, 2, 7, -1], [90, 1, 2, 3, 95, 4, 6, 8]
    before, hash0 = host_views(env.views), env.state_hash()
    loaded = torch.full((8,), 9, dtype=torch.uint8, device="cuda")
    got = host_views(env.restore(snap, _i32(torch, src), _i32(torch, dst), loaded))
    assert loaded.cpu().numpy().tolist() == [1, 1, 1, 1, 1, 1, 0, 0]
    assert helper.restore(helper.snapshot(roots), src, dst).tolist() == [1, 1, 1, 1, 1, 1, 0, 0]
    hash1 = env.state_hash()
    rest = np.setdiff1d(np.arange(n), dst[:6])   # slots 6 and 8 among them: untouched, bit for bit
    _same({k: v[rest] for k, v in got.items()}, {k: v[rest] for k, v in before.items()}, "untouched slots")
    assert np.array_equal(hash1[rest], hash0[rest])
    for s, d in zip(src[:6], dst[:6]):
        assert hash1[d] == hash0[roots[s]]
    assert_views_equal(got, helper.views(), "restored")
    assert np.array_equal(hash1, helper.hashes())
    # every fork plays its own actions: across the end of the forked episode (max_steps 24) into the destination's next ones
    ends = _lockstep(torch, env, helper, 50, rs, "forks")
    assert ends > 0 and helper.episodes()[dst[:6]].min() >= 2
    assert len(set(helper.hashes()[[5, 90, 1, 2]].tolist())) == 4
    env.close()


def test_fork_pool_decks_heuristic_plays_destination_row():
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    n = 96
    pool = np.array(sorted({CARD_INDEX[c] for d in DECKS.values() for c in d})[:40], dtype=np.uint8)
    assert len(pool) == 40
    seed0 = (np.arange(n, dtype=np.uint32) * 13 + 4000).astype(np.uint32)
    w = league(2)
    rows = np.arange(n) % 2
    spec = dict(seed0=seed0, pool=pool, agent_side=0, max_steps=30, opponent_weights=w, opponent_rows=rows)
    env = VecEnv(n)
    env.reset(seed0, pool=pool, opponent="heuristic", agent_side=0, max_steps=30, opponent_weights=w, opponent_rows=rows)
    helper = EnvSnapshotModel(spec, slots=[0, 1, 2, 3, 5])
    rs = np.random.RandomState(6)
    _lockstep(torch, env, helper, 6, rs, "before")
    snap = env.snapshot(_i32(torch, [0]))
    dst = [1, 3, 5]   # slots of the other weight row
    env.restore(snap, _i32(torch, [0, 0, 0]), _i32(torch, dst))
    assert helper.restore(helper.snapshot([0]), [0, 0, 0], dst).tolist() == [1, 1, 1]
    assert_views_equal(host_views(env.views, np.array(helper.slots)), helper.views(), "restored")
    # the forks play slot 0's actions: where they leave slot 0's line, the other opponent row did it
    parted = False
    for t in range(40):
        legal = helper.views()["legal"]
        a = random_legal(rs, legal)
        same = np.array_equal(helper.hashes()[[1, 3, 4]], np.repeat(helper.hashes()[0], 3))
        if same:
            a[[1, 3, 4]] = a[0]
        full = np.full(n, 255, dtype=np.uint8)
        full[helper.slots] = a
        got = host_views(env.step(torch.from_numpy(full).cuda()), np.array(helper.slots))
        assert_views_equal(got, helper.step(a), f"fork step {t}")
        h = env.state_hash()[helper.slots]
        assert np.array_equal(h, helper.hashes()), t
        assert h[1] == h[3] == h[4] or not same   # the three forks share row 1: one line while they get the same actions
        parted = parted or (same and h[1] != h[0])
    assert parted and helper.episodes().min() >= 1
    env.close()


# An episode that ends before the agent acts: the configuration of test_vec_env_gpu.test_pool_decks_extended_lockstep
# (pool decks on the extended record, agent_side 1, the scripted bot opens).  Episode 1 of its slot 37 -- seed 9481 + 512 --
# ends in the bot's opening turn with fault 1 (found on the CPU with VecEnvModel; the fixed-deck configuration of
# test_lockstep_with_model[1-1] has no such episode among the first 200 of its 1 024 slots).
PENDING_SEED = 9993


def test_pending_end_is_restored_pending():
    torch = _torch()
    from monsoon_amd.cards import observable_pool
    from monsoon_amd.vec_env import VecEnv
    n, src_slot, dst_slot = 96, 7, 20
    pool = observable_pool()
    seed0 = (np.arange(n, dtype=np.uint32) * 13 + 9000).astype(np.uint32)
    seed0[src_slot] = PENDING_SEED
    spec = dict(seed0=seed0, pool=pool, opponent=1, agent_side=1, max_steps=100, extended=True)
    env = VecEnv(n, extended=1)
    env.reset(seed0, pool=pool, opponent="expert", agent_side=1, max_steps=100)
    helper = EnvSnapshotModel(spec, slots=[src_slot, dst_slot, 2])
    assert helper.model[src_slot].result[0] != -2 and helper.model[dst_slot].result[0] == -2 and helper.model[2].result[0] == -2
    sel = np.array(helper.slots)
    assert_views_equal(host_views(env.views, sel), helper.views(), "reset")
    snap = env.snapshot(_i32(torch, [src_slot]))
    env.restore(snap, dst=_i32(torch, [dst_slot]))
    assert helper.restore(helper.snapshot([src_slot]), dst=[dst_slot]).tolist() == [1]
    got = host_views(env.views, sel)
    assert_views_equal(got, helper.views(), "restored")
    assert not got["done"].any() and env.state_hash()[dst_slot] == env.state_hash()[src_slot]
    a = np.full(n, 255, dtype=np.uint8)   # the end is reported whatever the action: none for the source, PASS for the copy
    a[dst_slot], a[2] = 155, 155
    got = host_views(env.step(torch.from_numpy(a).cuda()), sel)
    assert_views_equal(got, helper.step(a[sel]), "the pending end")
    assert got["done"][0] and got["done"][1] and not got["done"][2]
    for k in ("winner", "fault", "truncated", "final_hash", "episode"):
        assert got[k][0] == got[k][1], k
    _lockstep(torch, env, helper, 10, np.random.RandomState(1), "after")
    env.close()


def test_guard_rails():
    torch = _torch()
    from monsoon_amd import EnvSnapshot, MonsoonError, _lib
    from monsoon_amd.vec_env import VecEnv
    n = 96
    deck = np.stack([deck_indices("N12M")] * 2)
    seed0 = np.arange(n, dtype=np.uint32) + 9
    env = VecEnv(n)
    fresh = VecEnv(8)
    lib, h = env.engine.lib, env.engine.h
    size = ctypes.c_int32(-1)
    buf = torch.zeros(64 * 1024, dtype=torch.uint8, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    assert lib.monsoon_env_entry_bytes(h, ctypes.byref(size)) == _lib.ERR_STATE
    assert lib.monsoon_env_save_dev(h, p, None, 1) == _lib.ERR_STATE
    assert lib.monsoon_env_load_dev(h, p, 1, None, None, 1, None) == _lib.ERR_STATE
    with pytest.raises(MonsoonError):
        env.snapshot()
    env.reset(seed0, deck, opponent="expert", max_steps=40)
    for t in range(3):
        env.step(torch.full((n,), 155, dtype=torch.uint8, device="cuda"))
    assert lib.monsoon_env_entry_bytes(h, ctypes.byref(size)) == 0 and size.value == env.entry_bytes == 8320
    before, hash0 = host_views(env.views), env.state_hash()
    # a zero-filled snapshot loads nothing
    zero = EnvSnapshot(torch.zeros((n, env.entry_bytes), dtype=torch.uint8, device="cuda"), n, 0, env.entry_bytes)
    loaded = torch.ones(n, dtype=torch.bool, device="cuda")
    got = host_views(env.restore(zero, loaded=loaded))
    assert not loaded.cpu().numpy().any()
    _same(got, before, "zero-filled snapshot")
    assert np.array_equal(env.state_hash(), hash0)
    # an entry saved from a slot index outside [0, n) never loads either; its neighbours do
    snap = env.snapshot(_i32(torch, [4, n, -1, 7, 2]))
    assert snap.data[1, :16].cpu().numpy().tolist() == [0] * 16 and snap.data[2, :16].cpu().numpy().tolist() == [0] * 16
    loaded = torch.zeros(5, dtype=torch.uint8, device="cuda")
    env.restore(snap, dst=_i32(torch, [10, 11, 12, 13, 14]), loaded=loaded)
    assert loaded.cpu().numpy().tolist() == [1, 0, 0, 1, 1]
    h1 = env.state_hash()
    assert h1[10] == hash0[4] and h1[13] == hash0[7] and h1[14] == hash0[2] and h1[11] == hash0[11] and h1[12] == hash0[12]
    # another record build, another entry size
    ext = VecEnv(8, extended=1)
    ext.reset(np.arange(8, dtype=np.uint32), deck)
    other = ext.snapshot()
    assert other.extended == 1 and other.entry_bytes != env.entry_bytes
    with pytest.raises(ValueError, match="build"):
        env.restore(other)
    with pytest.raises(ValueError, match="build"):
        env.snapshot(out=other)
    with pytest.raises(ValueError):
        env.restore(EnvSnapshot(snap.data, 5, 0, env.entry_bytes - 16))
    ext.close()
    # before reset
    with pytest.raises(MonsoonError):
        fresh.restore(snap)
    with pytest.raises(MonsoonError):
        fresh.entry_bytes
    fresh.close()
    # dtype, device, shape
    good = _i32(torch, [0, 1])
    for bad in (good.to(torch.int64), good.cpu(), good.view(1, 2), [0, 1]):
        with pytest.raises(ValueError):
            env.restore(snap, src=bad, dst=good)
        with pytest.raises(ValueError):
            env.restore(snap, src=good, dst=bad)
        with pytest.raises(ValueError):
            env.snapshot(slots=bad)
    with pytest.raises(ValueError):
        env.restore(snap, src=good, dst=_i32(torch, [0, 1, 2]))
    with pytest.raises(ValueError):
        env.restore(snap, src=good, dst=good, loaded=torch.zeros(3, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        env.restore(snap, src=good, dst=good, loaded=torch.zeros(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        env.restore(snap, src=_i32(torch, range(n + 1)))   # more pairs than slots without dst
    with pytest.raises(ValueError):
        env.snapshot(out=EnvSnapshot(snap.data[:2], 2, 0, env.entry_bytes))   # room for 2, n to be saved
    # the C ABI's own argument checks
    assert lib.monsoon_env_save_dev(h, None, None, 1) == _lib.ERR_ARG
    assert lib.monsoon_env_save_dev(h, ctypes.c_void_p(buf.data_ptr() + 8), None, 1) == _lib.ERR_ARG
    assert lib.monsoon_env_save_dev(h, p, None, -1) == _lib.ERR_ARG
    assert lib.monsoon_env_save_dev(h, p, None, n + 1) == _lib.ERR_ARG
    assert lib.monsoon_env_load_dev(h, None, 1, None, None, 1, None) == _lib.ERR_ARG
    assert lib.monsoon_env_load_dev(h, ctypes.c_void_p(buf.data_ptr() + 4), 1, None, None, 1, None) == _lib.ERR_ARG
    assert lib.monsoon_env_load_dev(h, p, 1, None, None, -1, None) == _lib.ERR_ARG
    assert lib.monsoon_env_load_dev(h, p, 1, None, None, n + 1, None) == _lib.ERR_ARG
    assert np.array_equal(env.state_hash(), h1)
    env.engine.reset(np.arange(8, dtype=np.uint32), deck)   # monsoon_reset ends env mode
    assert lib.monsoon_env_save_dev(h, p, None, 1) == _lib.ERR_STATE
    env.close()


def test_captured_snapshot_steps_restore():
    """snapshot(out=), two steps and restore captured into one graph on the env's stream: every replay plays two steps and
    comes back to where it started."""
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    n = 96
    seed0 = np.arange(n, dtype=np.uint32) + 31
    env = VecEnv(n)
    views = env.reset(seed0, mixed_decks(n), opponent="expert", agent_side=0, max_steps=60)
    snap = env.snapshot()
    s = env.stream
    a = torch.full((n,), 155, dtype=torch.uint8, device="cuda")
    mid = torch.zeros(n, dtype=torch.int64, device="cuda")

    def body():
        env.snapshot(out=snap)
        env.step(a)
        env.step(a)
        mid.copy_(views["obs"].view(n, -1).to(torch.int64).sum(1))   # what the two steps left, kept for the host
        env.restore(snap)

    with torch.cuda.stream(s):   # warm-up outside the graph
        body()
    torch.cuda.synchronize()
    allocs = torch.cuda.memory_stats()["allocation.all.allocated"]
    with torch.cuda.stream(s):
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        env.snapshot(out=snap)
        env.restore(snap)
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before   # the two calls allocate nothing
    torch.cuda.synchronize()
    assert allocs == before
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        body()
    rs = np.random.RandomState(3)
    counters = (ctypes.c_ulonglong * 192)()
    for r in range(3):
        if r:   # move on between the replays, so that every replay saves another state
            env.step(torch.from_numpy(random_legal(rs, host_views(views)["legal"])).cuda())
        torch.cuda.synchronize()
        h0, v0 = env.state_hash(), host_views(views)
        assert env.engine.lib.monsoon_debug_counters(env.engine.h, counters) == 0
        steps0 = counters[6]
        a.copy_(torch.from_numpy(random_legal(rs, v0["legal"])))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(env.state_hash(), h0), r
        v1 = host_views(views)
        for k in ("obs", "legal", "to_play", "obs_raises", "episode"):
            assert np.array_equal(v1[k], v0[k]), (r, k)
        assert not v1["done"].any() and (v1["winner"] == -2).all()
        assert env.engine.lib.monsoon_debug_counters(env.engine.h, counters) == 0
        assert counters[6] >= steps0 + n, "the captured steps ran"   # the first step's action is legal in every slot
        assert not np.array_equal(mid.cpu().numpy(), v0["obs"].reshape(n, -1).astype(np.int64).sum(1))
    env.close()


def test_entries_load_into_another_handle():
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    na, nb = 96, 40
    spec_a = dict(seed0=(np.arange(na, dtype=np.uint32) * 31 + 5).astype(np.uint32), decks=mixed_decks(na), opponent=1, agent_side=0,
                  max_steps=40)
    spec_b = dict(seed0=(np.arange(nb, dtype=np.uint32) * 977 + 123456).astype(np.uint32), decks=mixed_decks(nb)[::-1].copy(), opponent=1,
                  agent_side=0, max_steps=35, seed_stride=1000)
    env_a, env_b = VecEnv(na), VecEnv(nb)
    env_a.reset(spec_a["seed0"], spec_a["decks"], opponent="expert", max_steps=40)
    env_b.reset(spec_b["seed0"], spec_b["decks"], opponent="expert", max_steps=35, seed_stride=1000)
    help_a = EnvSnapshotModel(spec_a, slots=[3, 50])
    help_b = EnvSnapshotModel(spec_b, slots=[0, 7, 39])
    rs = np.random.RandomState(12)
    _lockstep(torch, env_a, help_a, 12, rs, "a")
    _lockstep(torch, env_b, help_b, 3, rs, "b")
    snap = env_a.snapshot(_i32(torch, [3, 50]))
    torch.cuda.synchronize()   # the entries were written on env_a's stream
    loaded = torch.zeros(2, dtype=torch.uint8, device="cuda")
    env_b.restore(snap, _i32(torch, [1, 0]), _i32(torch, [7, 39]), loaded)
    assert loaded.cpu().numpy().tolist() == [1, 1]
    assert help_b.restore(help_a.snapshot([3, 50]), [1, 0], [7, 39]).tolist() == [1, 1]
    assert_views_equal(host_views(env_b.views, np.array(help_b.slots)), help_b.views(), "restored")
    hb, ha = env_b.state_hash(), env_a.state_hash()
    assert hb[7] == ha[50] and hb[39] == ha[3]
    _lockstep(torch, env_b, help_b, 20, rs, "b after the load")
    assert help_b.episodes()[1:].min() >= 1   # into env_b's seed schedule (stride 1000) and step limit
    env_a.close()
    env_b.close()
