"""CPU tests of saving and restoring vector-env slots (include/monsoon.h monsoon_env_entry_bytes / monsoon_env_save_dev /
monsoon_env_load_dev, VecEnv.snapshot / restore): the ABI is declared, exported by every built library and bound, and the
helper model the GPU tests compare against (tests/env_snapshot_model.py) is pinned to a straight VecEnvModel run."""
import ctypes
import inspect

import numpy as np
import pytest

from env_snapshot_model import EnvSnapshotModel, build_entry, entry_layout, replay
from monsoon_amd.cards import deck_indices
from test_abi import header_functions
from vec_env_model import VecEnvModel

NAMES = ("monsoon_env_entry_bytes", "monsoon_env_save_dev", "monsoon_env_load_dev")
PAIRS = [("N12M", "N12M"), ("N12V", "S12"), ("IRONCLAD", "SWARM"), ("S12", "N12M"), ("SWARM", "N12V")]


def _random_legal(rs, legal):
    u = rs.random_sample(legal.shape)
    u[~legal] = -1.0
    return u.argmax(axis=1).astype(np.uint8)


def _spec(n, seed, **kw):
    pairs = [np.stack([deck_indices(a), deck_indices(b)]) for a, b in PAIRS]
    decks = np.stack([pairs[i % len(pairs)] for i in range(n)])
    seed0 = (np.arange(n, dtype=np.uint32) * 104729 + seed).astype(np.uint32)
    return dict(seed0=seed0, decks=decks, **kw)


def test_symbols_declared_exported_and_bound():
    from monsoon_amd import _lib
    declared = header_functions()
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/monsoon.h"
        for ext in (0, 1, 2):
            assert hasattr(_lib.load(ext), name), (name, ext)
        assert name in _lib.SIGNATURES
    p, i32 = ctypes.c_void_p, ctypes.c_int32
    assert _lib.SIGNATURES["monsoon_env_entry_bytes"] == (ctypes.c_int, [p, ctypes.POINTER(i32)])
    assert _lib.SIGNATURES["monsoon_env_save_dev"] == (ctypes.c_int, [p, p, p, i32])
    assert _lib.SIGNATURES["monsoon_env_load_dev"] == (ctypes.c_int, [p, p, i32, p, p, i32, p])
    for ext, build in ((0, 0), (1, 0x10000), (2, 0x30000)):   # the version is bumped, the generation and the build bits stay
        v = _lib.load(ext).monsoon_version()
        assert v & 0xffff == 3 and v & 0x30000 == build and v >> 24 >= 1, hex(v)


def test_python_surface():
    import monsoon_amd
    from monsoon_amd.vec_env import EnvSnapshot, VecEnv
    assert monsoon_amd.EnvSnapshot is EnvSnapshot and "EnvSnapshot" in monsoon_amd.__all__
    assert isinstance(inspect.getattr_static(VecEnv, "entry_bytes"), property)
    assert list(inspect.signature(VecEnv.snapshot).parameters) == ["self", "slots", "out"]
    assert list(inspect.signature(VecEnv.restore).parameters) == ["self", "snap", "src", "dst", "loaded"]
    snap = EnvSnapshot(np.zeros((5, 8320), dtype=np.uint8), 3, 0, 8320)
    assert (len(snap), snap.capacity, snap.extended, snap.entry_bytes) == (3, 5, 0, 8320)


@pytest.mark.parametrize("opponent,agent_side", [(0, 0), (1, 1)])
def test_helper_without_forks_is_the_plain_model(opponent, agent_side):
    n, steps = 6, 60
    spec = _spec(n, 31 + opponent, opponent=opponent, agent_side=agent_side, max_steps=25)
    plain = VecEnvModel(**spec)
    helper = EnvSnapshotModel(spec)
    rs = np.random.RandomState(4)
    for k, w in plain.views.items():
        assert np.array_equal(helper.views()[k], w), k
    for t in range(steps):
        a = _random_legal(rs, plain.views["legal"])
        want, got = plain.step(a), helper.step(a)
        for k, w in want.items():
            assert got[k].dtype == w.dtype and np.array_equal(got[k], w), (t, k)
        assert np.array_equal(helper.hashes(), plain.hashes()), t
    assert plain.episode.min() >= 1
    # a lineage replayed from scratch is the slot, and a rewind on the model changes nothing but the per-call views
    assert replay(helper.lineage[3]).hashes()[0] == plain.hashes()[3]
    snap = helper.snapshot()
    assert helper.restore(snap).tolist() == [1] * n
    v = helper.views()
    assert np.array_equal(helper.hashes(), plain.hashes()) and np.array_equal(v["obs"], plain.views["obs"])
    assert not v["done"].any() and (v["winner"] == -2).all() and np.array_equal(v["episode"], plain.views["episode"])


def test_helper_fork_follows_the_source_then_the_destinations_schedule():
    """Slot 1's state loaded into slot 4: the same actions give the same states until the forked episode ends; the next
    episode starts from seed0[4] + k * stride with the carried count k and the carried decks."""
    n = 6
    spec = _spec(n, 77, opponent=0, max_steps=12)
    helper = EnvSnapshotModel(spec)
    rs = np.random.RandomState(9)
    for _ in range(5):
        helper.step(_random_legal(rs, helper.views()["legal"]))
    snap = helper.snapshot([1, 99])
    assert snap[1] is None
    assert helper.restore(snap, src=[0, 1, 0, 2], dst=[4, 2, 6, 3]).tolist() == [1, 0, 0, 0]
    assert helper.hashes()[4] == helper.hashes()[1]
    for t in range(7):   # max_steps 12: the episode ends at its 12th step
        legal = helper.views()["legal"]
        a = _random_legal(rs, legal)
        a[4] = a[1]
        v = helper.step(a)
        assert v["done"][4] == v["done"][1] and (v["done"][1] == (t == 6))
        if t < 6:
            assert helper.hashes()[4] == helper.hashes()[1]
    m1, m4 = helper.model[1], helper.model[4]
    assert m1.episode[0] == m4.episode[0] == 1
    assert m1.seed(0) == int(spec["seed0"][1]) + n and m4.seed(0) == int(spec["seed0"][4]) + n
    assert np.array_equal(m4.decks[0], spec["decks"][1]) and not np.array_equal(spec["decks"][4], spec["decks"][1])
    assert helper.hashes()[4] != helper.hashes()[1]


# build -> (body granules = record + rng_mt + rng_out, passes of the copy loop, granules of its last pass): the table of
# monsoon_amd/csrc/env_snap.hip's SNAP_PASS (64 x 10 granules per pass)
ENTRY_TABLE = {0: (47 + 156 + 312, 1, 515), 1: (150 + 156 + 312, 1, 618), 2: (521 + 156 + 312, 2, 349)}


@pytest.mark.parametrize("ext", [0, 1, 2])
def test_entry_layout_of_every_build(ext):
    """The entry model derives its sizes from the build's record size; they are the documented ones, and only the large
    entry takes a second pass of the copy loop, whose sixth load of 64 granules is live on 29 lanes."""
    from monsoon_amd import _lib
    lay = entry_layout(ext)
    body, passes, tail = ENTRY_TABLE[ext]
    assert (lay["body_granules"], lay["passes"], lay["tail_granules"]) == (body, passes, tail)
    assert lay["entry_bytes"] == 80 + 16 * body and lay["entry_bytes"] % 16 == 0
    assert lay["record_bytes"] // 16 == body - 156 - 312
    assert lay["mt_at"] == 80 + lay["record_bytes"] and lay["out_at"] == lay["mt_at"] + 2496 and lay["out_at"] + 4992 == lay["entry_bytes"]
    if ext == 0:
        assert lay["entry_bytes"] == 8320
    if ext == 2:
        assert lay["record_bytes"] == 8336 and tail - 5 * 64 == 29
    # build_entry puts the parts where the layout says
    blob_bytes = int(_lib.load(ext).monsoon_state_blob_bytes())
    blob = (np.arange(blob_bytes) % 251).astype(np.uint8)
    blob[4:8] = np.array([lay["record_bytes"]], dtype="<u4").view(np.uint8)
    decks = np.arange(24, dtype=np.uint8).reshape(2, 12) + 100
    e = build_entry(ext, 0x01030003, 7, decks, blob)
    assert len(e) == lay["entry_bytes"]
    assert e[:16].view("<u4").tolist() == [0x50414E53, 0x01030003, lay["record_bytes"] // 4, 7]
    assert np.array_equal(e[16:48], blob[8:40]) and np.array_equal(e[48:72], decks.reshape(24)) and not e[72:80].any()
    assert np.array_equal(e[80:lay["mt_at"]], blob[40:40 + lay["record_bytes"]])
    assert np.array_equal(e[lay["mt_at"]:], blob[40 + lay["record_bytes"]:])
