"""GPU tests of determinized forks (monsoon_env_load_determinized_dev, VecEnv.determinize) against the byte model
(tests/env_determinize_model.py): a snapshot of every loaded slot equals the model's entry byte for byte -- on real states
and on entries patched to the edges of hand and deck -- what the side to move sees does not change, a determinized slot
plays as the model's entry loaded by the plain restore plays, skipped pairs and ended episodes, the extended and the large
build, and a captured call that reads new seeds on every replay.  Few slots everywhere; 200 pairs into 256 slots once, which
is more than the wavefronts of one workgroup of the copy kernel and 200 workgroups of the re-draw."""
import ctypes

import numpy as np
import pytest

import env_determinize_model as M
from env_snapshot_model import entry_layout
from monsoon_amd.cards import deck_indices
from test_vec_env_gpu import host_views

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _i32(torch, xs):
    return torch.tensor([int(x) for x in xs], dtype=torch.int32, device="cuda")


def _u8(torch, xs):
    return torch.tensor([int(x) for x in xs], dtype=torch.uint8, device="cuda")


def _seeds(torch, xs):
    """uint32 seeds as the int32 tensor VecEnv.determinize takes: the same bits."""
    return torch.from_numpy(np.array(xs, dtype=np.uint32).view(np.int32).copy()).cuda()


def _two_pairs(n):
    pairs = [np.stack([deck_indices("N12M"), deck_indices("N12M")]), np.stack([deck_indices("S12"), deck_indices("N12V")])]
    return np.stack([pairs[i % 2] for i in range(n)])


def _first_legal(views, live=None):
    legal = views["legal"].cpu().numpy()
    a = np.where(legal.any(axis=1), legal.argmax(axis=1), 155).astype(np.uint8)
    if live is not None:
        a[~live] = 255
    return a


def _six_states(torch, opponent="none", **kw):
    """Six slots of two deck pairs; slot i has played i first-legal actions."""
    from monsoon_amd.vec_env import VecEnv
    env = VecEnv(6)
    views = env.reset(np.arange(6, dtype=np.uint32) * 7919 + 3, _two_pairs(6), opponent=opponent, **kw)
    for t in range(5):
        env.step(torch.from_numpy(_first_legal(views, np.arange(6) > t)).cuda())
    return env


def _bytes(snap):
    return snap.data[:snap.count].cpu().numpy()


def _as_snapshot(torch, entries):
    from monsoon_amd.vec_env import EnvSnapshot
    e = np.ascontiguousarray(entries, dtype=np.uint8)
    return EnvSnapshot(torch.from_numpy(e).cuda(), len(e), 0, e.shape[1])


def _assert_entry(got, want, ctx):
    if not np.array_equal(got, want):
        at = np.nonzero(got != want)[0]
        out_at = len(want) - 2 * M.MT_N * 4
        parts = [("header", 0), ("meta", 16), ("decks", 48), ("record", 80), ("rng_mt", out_at - M.MT_N * 4), ("rng_out", out_at)]
        where = [name for name, start in parts if start <= at[0]][-1]
        raise AssertionError(f"{ctx}: {len(at)} bytes differ, the first at {int(at[0])} ({where}), the last at {int(at[-1])}")


def _big(n=256):
    from monsoon_amd.vec_env import VecEnv
    env = VecEnv(n)
    env.reset(np.arange(n, dtype=np.uint32) + 70000, np.stack([deck_indices("N12M")] * 2), opponent="none")
    return env


def test_loaded_slots_equal_the_model_byte_for_byte():
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    env = _six_states(torch)
    snap = env.snapshot()
    src_bytes = _bytes(snap)
    counts = set()
    for e in src_bytes:
        assert e[M.META_RESULT:M.META_RESULT + 1].view(np.int8)[0] == -2
        for side in (0, 1):
            counts.add((int(e[M.player_at(side) + M.P_HAND_N]), int(e[M.player_at(side) + M.P_DECK_N])))
    print("hand / deck counts of the six states:", sorted(counts))
    assert len({h for h, _ in counts}) >= 2 and all(h + d <= 12 for h, d in counts)
    big = _big()
    # a single pair, default observer and an int observer
    for observer, byte in ((None, 255), (1, 1), (0, 0)):
        loaded = torch.zeros(1, dtype=torch.uint8, device="cuda")
        big.determinize(snap, _seeds(torch, [4242]), src=_i32(torch, [2]), dst=_i32(torch, [5]), observer=observer, loaded=loaded)
        assert loaded.cpu().numpy().tolist() == [1]
        got = _bytes(big.snapshot(_i32(torch, [5])))[0]
        _assert_entry(got, M.determinize_entry(src_bytes[2], 4242, byte, "hand"), f"m = 1, observer {observer}")
    # 200 pairs forked from the six entries
    m = 200
    rs = np.random.RandomState(11)
    src = np.arange(m) % 6
    dst = (np.arange(m) * 7 + 3) % 256   # distinct slots
    observers = rs.choice([0, 1, 255], m)
    seeds = rs.randint(0, 2**32, m, dtype=np.uint64).astype(np.uint32)
    seeds[0], seeds[1], seeds[2] = 0, 0xFFFFFFFF, 0x7FFFFFFF
    changed = 0
    for what in ("hand", "stream"):
        loaded = torch.zeros(m, dtype=torch.uint8, device="cuda")
        big.determinize(snap, _seeds(torch, seeds), _i32(torch, src), _i32(torch, dst), _u8(torch, observers), what, loaded)
        assert loaded.cpu().numpy().tolist() == [1] * m
        got = _bytes(big.snapshot(_i32(torch, dst)))
        for j in range(m):
            want = M.determinize_entry(src_bytes[src[j]], int(seeds[j]), int(observers[j]), what)
            _assert_entry(got[j], want, f"{what} pair {j} (entry {src[j]}, observer {observers[j]}, seed {seeds[j]})")
            rec = slice(M.BODY_AT, entry_layout(0)["mt_at"])
            if what == "stream":
                assert np.array_equal(got[j][rec], src_bytes[src[j]][rec])
            else:
                changed += not np.array_equal(got[j][rec], src_bytes[src[j]][rec])
    assert changed > m // 2   # a hand of two or more among ten or more hidden cards rarely comes back as it was
    # the stream is the one a reset with that seed leaves: rng_mt and both blocks, while the cursor is still in block 0
    ref = VecEnv(3)
    ref.reset(seeds[:3].copy(), np.stack([deck_indices("N12M")] * 2), opponent="none")
    ref_bytes = _bytes(ref.snapshot())
    mt_at = entry_layout(0)["mt_at"]
    for j in range(3):
        rng = int(ref_bytes[j][M.META_RNG:M.META_RNG + 4].view("<u4")[0])
        assert rng >> 16 == 0 and 0 < (rng & 0xffff) < M.MT_N, hex(rng)
        assert np.array_equal(got[j][mt_at:], ref_bytes[j][mt_at:]), j
    for e in (env, big, ref):
        e.close()


def _patched(entry, side, hn, dn, flags=()):
    """The entry with player `side`'s hand and deck counts set; further entries are copies of that player's own cards."""
    e = entry.copy()
    pl = M.player_at(side)
    hn0, dn0 = int(e[pl + M.P_HAND_N]), int(e[pl + M.P_DECK_N])
    own = [e[pl + M.P_HAND + 4 * i:pl + M.P_HAND + 4 * i + 4].copy() for i in range(hn0)]
    own += [e[pl + M.P_DECK + 4 * i:pl + M.P_DECK + 4 * i + 4].copy() for i in range(dn0)]
    for i in range(hn0, hn):
        e[pl + M.P_HAND + 4 * i:pl + M.P_HAND + 4 * i + 4] = own[(3 * i + 1) % len(own)]
    for i in range(dn0, dn):
        e[pl + M.P_DECK + 4 * i:pl + M.P_DECK + 4 * i + 4] = own[(5 * i + 2) % len(own)]
    e[pl + M.P_HAND_N], e[pl + M.P_DECK_N] = hn, dn
    for p, f in flags:
        e[pl + M.P_HAND + 4 * p + 2] |= f
    return e


def test_edge_shapes_by_patched_entries():
    """Hands of 0, 1, 4, 5 and decks of 0, 1, 12, b305's two flags pinned at hand positions 0 and 2, an ended episode.  The
    patched block is always the one of the side that is NOT to move, and the observer is the mover (by default and by
    name): the views the load writes read the mover's hand only.  Bytes are compared; the slots are never stepped."""
    torch = _torch()
    env = _six_states(torch)
    base = _bytes(env.snapshot())
    shapes = [(0, 5, ()), (1, 0, ()), (1, 1, ()), (4, 12, ()), (5, 12, ()), (5, 0, ()), (0, 0, ()), (4, 1, ()), (0, 12, ()),
              (4, 8, ((0, M.CF_ALIAS),)), (5, 7, ((2, M.CF_STR),)), (5, 12, ((0, M.CF_ALIAS), (2, M.CF_STR))), (1, 6, ((0, M.CF_ALIAS),)),
              (3, 0, ((2, M.CF_STR),))]
    entries, observers = [], []
    for i, (hn, dn, flags) in enumerate(shapes):
        e = base[i % 6]
        mover = int(e[M.BODY_AT + M.H_TOPLAY])
        assert mover in (0, 1)
        entries.append(_patched(e, 1 - mover, hn, dn, flags))
        observers.append(255 if i % 2 else mover)
    ended = base[3].copy()
    ended[M.META_RESULT] = 1   # SECOND won: loaded verbatim
    entries.append(ended)
    observers.append(255)
    m = len(entries)
    snap = _as_snapshot(torch, np.stack(entries))
    big = _big(32)
    seeds = (np.arange(m, dtype=np.uint32) * 2654435761 + 17).astype(np.uint32)
    loaded = torch.zeros(m, dtype=torch.uint8, device="cuda")
    big.determinize(snap, _seeds(torch, seeds), dst=_i32(torch, np.arange(m) + 9), observer=_u8(torch, observers), what="hand", loaded=loaded)
    assert loaded.cpu().numpy().tolist() == [1] * m
    got = _bytes(big.snapshot(_i32(torch, np.arange(m) + 9)))
    for j in range(m):
        _assert_entry(got[j], M.determinize_entry(entries[j], int(seeds[j]), observers[j], "hand"), f"shape {j} {shapes[j] if j < len(shapes) else 'ended'}")
    assert np.array_equal(got[m - 1], ended)
    for j, (hn, dn, flags) in enumerate(shapes):   # the pinned entries stayed where they were
        pl = M.player_at(1 - int(entries[j][M.BODY_AT + M.H_TOPLAY]))
        for p, _ in flags:
            at = pl + M.P_HAND + 4 * p
            assert np.array_equal(got[j][at:at + 4], entries[j][at:at + 4]), (j, p)
    env.close()
    big.close()


def test_what_the_observer_sees_does_not_change():
    torch = _torch()
    env = _six_states(torch)
    snap = env.snapshot()
    big = _big(32)
    src, dst = _i32(torch, [0, 1, 2, 3, 4, 5, 3, 5]), _i32(torch, [20, 4, 9, 31, 0, 7, 8, 12])
    sel = dst.cpu().numpy()
    decks0 = big.decks().cpu().numpy().copy()
    plain = host_views(big.restore(snap, src, dst), sel)
    decks1 = big.decks().cpu().numpy().copy()
    for what in ("hand", "stream"):
        got = host_views(big.determinize(snap, _seeds(torch, np.arange(8) + 99), src, dst, what=what), sel)
        for k in plain:
            assert np.array_equal(got[k], plain[k]), (what, k)
        assert np.array_equal(big.decks().cpu().numpy(), decks1)   # determinize never changes decks()
    assert not np.array_equal(decks0, decks1)   # (the restore carried the entries' decks)
    assert np.array_equal(host_views(env.views)["obs"][[0, 1, 2, 3, 4, 5, 3, 5]], plain["obs"])
    env.close()
    big.close()


@pytest.mark.parametrize("opponent", ["expert", "heuristic"])
def test_plays_as_the_models_entry_loaded_by_restore(opponent):
    """Slot 1 receives the model's entry by the plain restore (which the snapshot tests pin to the oracle), slot 2 the same
    pair by determinize: 30 first-legal steps against the opponent give the same views, final_hash included.  All slots
    share seed0, so the episodes that follow the forked one are the same too."""
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    from test_vec_env_heuristic_gpu import league
    kw = dict(opponent_weights=league(1)) if opponent == "heuristic" else {}
    env = VecEnv(4)
    views = env.reset(np.full(4, 4711, dtype=np.uint32), _two_pairs(4)[1], opponent=opponent, agent_side=0, max_steps=40, seed_stride=13, **kw)
    for t in range(3):
        env.step(torch.from_numpy(_first_legal(views)).cuda())
    snap = env.snapshot(_i32(torch, [0]))
    entry = _bytes(snap)[0]
    assert entry[M.META_RESULT:M.META_RESULT + 1].view(np.int8)[0] == -2 and entry[M.BODY_AT + M.H_TOPLAY] == 0
    seed = 0x9E3779B9
    want = M.determinize_entry(entry, seed, 255, "hand")
    assert not np.array_equal(want[M.BODY_AT:entry_layout(0)["mt_at"]], entry[M.BODY_AT:entry_layout(0)["mt_at"]])   # the hidden hand moved
    env.restore(_as_snapshot(torch, want[None]), dst=_i32(torch, [1]))
    env.determinize(snap, _seeds(torch, [seed]), dst=_i32(torch, [2]), what="hand")
    ends = 0
    parted = False
    for t in range(30):
        v = host_views(views)
        for k in v:
            assert np.array_equal(v[k][1], v[k][2]), (t, k)
        parted = parted or not np.array_equal(v["obs"][0], v["obs"][1])
        ends += int(v["done"][1])
        a = _first_legal(views)
        assert a[1] == a[2]
        env.step(torch.from_numpy(a).cuda())
    h = env.state_hash()
    assert h[1] == h[2] and parted   # the fork left the true game's line: another stream, another hidden hand
    print(f"{opponent}: {ends} episode ends in 30 steps")
    env.close()


def test_skipped_pairs_leave_slot_and_views_untouched():
    torch = _torch()
    env = _six_states(torch)
    good = _bytes(env.snapshot())
    entries = np.concatenate([good, np.zeros((1, good.shape[1]), dtype=np.uint8)])   # entry 6 was never written
    snap = _as_snapshot(torch, entries)
    big = _big(32)
    before, views0 = _bytes(big.snapshot()), host_views(big.views)
    #        bad src    bad dst     zero  observer 7  good
    src = [-1, 7, 99,   0, 1,       6,    2,          3]
    dst = [1, 2, 3,     -1, 32,     4,    5,          6]
    obs = [255, 0, 1,   255, 255,   255,  7,          255]
    for what in ("stream", "hand"):
        loaded = torch.full((8,), 9, dtype=torch.uint8, device="cuda")
        big.determinize(snap, _seeds(torch, np.arange(8) + 5), _i32(torch, src), _i32(torch, dst), _u8(torch, obs), what, loaded)
        assert loaded.cpu().numpy().tolist() == [0, 0, 0, 0, 0, 0, 0, 1], what
        after, views1 = _bytes(big.snapshot()), host_views(big.views)
        rest = np.setdiff1d(np.arange(32), [6])
        assert np.array_equal(after[rest], before[rest]), what
        for k in views0:
            assert np.array_equal(views1[k][rest], views0[k][rest]), (what, k)
        _assert_entry(after[6], M.determinize_entry(good[3], 12, 255, what), what)
    env.close()
    big.close()


# tests/test_env_snapshot_gpu.py PENDING_SEED: on the extended record with pool decks and the scripted bot opening, episode
# 0 of this seed ends in the bot's opening turn, before the agent can act
def test_a_pending_end_loads_verbatim():
    torch = _torch()
    from monsoon_amd.cards import observable_pool
    from monsoon_amd.vec_env import VecEnv
    from test_env_snapshot_gpu import PENDING_SEED
    n = 8
    seed0 = (np.arange(n, dtype=np.uint32) * 13 + 9000).astype(np.uint32)
    seed0[3] = PENDING_SEED
    env = VecEnv(n, extended=1)
    env.reset(seed0, pool=observable_pool(), opponent="expert", agent_side=1, max_steps=100)
    snap = env.snapshot(_i32(torch, [3, 5]))
    e = _bytes(snap)
    assert e[0][M.META_RESULT:M.META_RESULT + 1].view(np.int8)[0] != -2 and e[1][M.META_RESULT:M.META_RESULT + 1].view(np.int8)[0] == -2
    env.determinize(snap, _seeds(torch, [77, 78]), dst=_i32(torch, [6, 7]), what="stream")
    got = _bytes(env.snapshot(_i32(torch, [6, 7])))
    assert np.array_equal(got[0], e[0])   # the pending end: verbatim, its stream too
    _assert_entry(got[1], M.determinize_entry(e[1], 78, 255, "stream", extended=1), "the running neighbour")
    a = np.full(n, 255, dtype=np.uint8)
    a[6] = 155
    v = host_views(env.step(torch.from_numpy(a).cuda()))
    assert v["done"][6] and v["done"][3] and not v["done"][7]   # the next step reports the end, as after a plain restore
    for k in ("winner", "fault", "truncated", "final_hash"):
        assert v[k][6] == v[k][3], k
    env.close()


@pytest.mark.parametrize("extended", [1, 2])
def test_extended_builds_take_the_stream_only(extended):
    torch = _torch()
    from monsoon_amd import _lib
    from monsoon_amd.vec_env import VecEnv
    n = 8
    env = VecEnv(n, extended=extended)
    views = env.reset(np.arange(n, dtype=np.uint32) + 40, np.stack([deck_indices("N12M")] * 2), opponent="none")
    for t in range(2):
        env.step(torch.from_numpy(_first_legal(views)).cuda())
    snap = env.snapshot()
    src = _bytes(snap)
    lay = entry_layout(extended)
    seeds = np.array([0, 0xFFFFFFFF, 5, 6], dtype=np.uint32)
    loaded = torch.zeros(4, dtype=torch.uint8, device="cuda")
    env.determinize(snap, _seeds(torch, seeds), _i32(torch, [0, 1, 2, 3]), _i32(torch, [7, 6, 5, 4]), _u8(torch, [0, 1, 255, 255]), "stream", loaded)
    assert loaded.cpu().numpy().tolist() == [1] * 4
    got = _bytes(env.snapshot(_i32(torch, [7, 6, 5, 4])))
    for j in range(4):
        _assert_entry(got[j], M.determinize_entry(src[j], int(seeds[j]), 255, "stream", extended=extended), f"build {extended} pair {j}")
        assert np.array_equal(got[j][M.BODY_AT:lay["mt_at"]], src[j][M.BODY_AT:lay["mt_at"]])
        assert not np.array_equal(got[j][lay["mt_at"]:], src[j][lay["mt_at"]:])
    with pytest.raises(ValueError, match='what="stream"'):
        env.determinize(snap, _seeds(torch, seeds), _i32(torch, [0, 1, 2, 3]), _i32(torch, [7, 6, 5, 4]))
    lib, h = env.engine.lib, env.engine.h
    all_seeds = _seeds(torch, np.arange(n))
    p, s = ctypes.c_void_p(snap.data.data_ptr()), ctypes.c_void_p(all_seeds.data_ptr())
    before = _bytes(env.snapshot())
    assert lib.monsoon_env_load_determinized_dev(h, p, n, None, None, n, s, None, 3, None) == _lib.ERR_ARG
    assert b"standard record" in lib.monsoon_last_error(h)
    with pytest.raises(_lib.MonsoonError, match="standard record"):
        env.engine.env_load_determinized_dev(snap.data.data_ptr(), n, 0, 0, n, s.value, 0, 3, 0)
    assert np.array_equal(_bytes(env.snapshot()), before)
    env.close()


def test_argument_checks_of_the_call_and_of_the_method():
    torch = _torch()
    from monsoon_amd import MonsoonError, _lib
    from monsoon_amd.vec_env import VecEnv
    n = 8
    env = VecEnv(n)
    lib, h = env.engine.lib, env.engine.h
    buf = torch.zeros(n * 8320 + 16, dtype=torch.uint8, device="cuda")
    seeds = _seeds(torch, np.arange(n))
    p, s = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(seeds.data_ptr())
    assert lib.monsoon_env_load_determinized_dev(h, p, n, None, None, 1, s, None, 1, None) == _lib.ERR_STATE
    env.reset(np.arange(n, dtype=np.uint32), _two_pairs(n), opponent="none")
    snap = env.snapshot()
    h0 = env.state_hash()
    for what in (0, 2, 4, 7, -1):
        assert lib.monsoon_env_load_determinized_dev(h, p, n, None, None, 1, s, None, what, None) == _lib.ERR_ARG, what
    assert lib.monsoon_env_load_determinized_dev(h, p, n, None, None, 1, None, None, 1, None) == _lib.ERR_ARG   # no seeds
    assert lib.monsoon_env_load_determinized_dev(h, None, n, None, None, 1, s, None, 1, None) == _lib.ERR_ARG
    assert lib.monsoon_env_load_determinized_dev(h, ctypes.c_void_p(buf.data_ptr() + 8), n, None, None, 1, s, None, 1, None) == _lib.ERR_ARG
    assert lib.monsoon_env_load_determinized_dev(h, p, n, None, None, -1, s, None, 1, None) == _lib.ERR_ARG
    assert lib.monsoon_env_load_determinized_dev(h, p, n, None, None, n + 1, s, None, 1, None) == _lib.ERR_ARG
    assert lib.monsoon_env_load_determinized_dev(h, p, n, None, None, 0, s, None, 3, None) == 0   # m = 0: nothing to do
    good = _i32(torch, [0, 1])
    two = _seeds(torch, [1, 2])
    for bad in (two.to(torch.int64), two.cpu(), two.view(1, 2), [1, 2], _seeds(torch, [1, 2, 3]), _seeds(torch, [1, 2, 3, 4])[::2], None):
        with pytest.raises(ValueError, match="seeds"):
            env.determinize(snap, bad, good, good)
    for bad in (_u8(torch, [0, 1, 0]), _u8(torch, [0, 1]).to(torch.int32), _u8(torch, [0, 1]).cpu()):
        with pytest.raises(ValueError, match="observer"):
            env.determinize(snap, two, good, good, observer=bad)
    with pytest.raises(ValueError):
        env.determinize(snap, two, good.to(torch.int64), good)
    with pytest.raises(ValueError):
        env.determinize(snap, two, good, good, loaded=torch.zeros(3, dtype=torch.uint8, device="cuda"))
    fresh = VecEnv(4)
    with pytest.raises(MonsoonError):
        fresh.determinize(snap, two, good, good)
    fresh.close()
    assert np.array_equal(env.state_hash(), h0)
    env.close()


def test_captured_determinize_reads_new_seeds_on_every_replay():
    """determinize + step captured on the env's stream: the seeds tensor is read on the device, so a replay after new seeds
    were written into it equals the uncaptured calls with those seeds."""
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    n = 16
    env = VecEnv(n)
    views = env.reset(np.arange(n, dtype=np.uint32) + 31, _two_pairs(n), opponent="expert", agent_side=0, max_steps=60)
    for t in range(2):
        env.step(torch.from_numpy(_first_legal(views)).cuda())
    snap = env.snapshot()
    s = env.stream
    a = torch.full((n,), 155, dtype=torch.uint8, device="cuda")   # PASS: the scripted bot answers from the slot's stream
    seeds = _seeds(torch, np.arange(n) + 1000)

    def body():
        env.determinize(snap, seeds, what="hand")
        env.step(a)

    with torch.cuda.stream(s):   # warm-up outside the graph
        body()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        env.determinize(snap, seeds, what="hand")
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before   # the call allocates nothing
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        body()
    hashes = []
    for r in range(2):
        new = np.arange(n) * 977 + 50000 * (r + 1)
        seeds.copy_(_seeds(torch, new))
        g.replay()
        torch.cuda.synchronize()
        h_graph, v_graph = env.state_hash(), host_views(views)
        env.determinize(snap, _seeds(torch, new), what="hand")
        env.step(a)
        torch.cuda.synchronize()
        assert np.array_equal(env.state_hash(), h_graph), r
        v = host_views(views)
        for k in v:
            assert np.array_equal(v[k], v_graph[k]), (r, k)
        hashes.append(h_graph)
    assert not np.array_equal(hashes[0], hashes[1])   # other seeds, other worlds
    env.close()
