"""CPU tests of determinized forks (include/monsoon.h monsoon_env_load_determinized_dev, VecEnv.determinize): the ABI is
declared, exported by every built library and bound; the rule's text the kernel compiles (monsoon_amd/csrc/determinize.h,
a stand-alone program) gives the permutation of vec_env.determinize_order and of the test model; the model
(tests/env_determinize_model.py) keeps what the rule says it keeps; the rule deals uniformly; and VecEnv.determinize
refuses bad arguments before it needs a device."""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import env_determinize_model as M
from env_snapshot_model import SNAP_MAGIC, entry_layout
from monsoon_amd.fitness import hash32_array
from test_abi import header_functions

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "monsoon_env_load_determinized_dev"
SEEDS = [0, 1, 0x7FFFFFFF, 0xFFFFFFFF] + list(range(90210, 90410))


def test_symbol_declared_exported_and_bound():
    from monsoon_amd import _lib
    from monsoon_amd.engine import BatchEngine
    assert NAME in header_functions(), f"{NAME} is not declared in include/monsoon.h"
    for ext in (0, 1, 2):
        assert hasattr(_lib.load(ext), NAME), ext
    p, i32 = ctypes.c_void_p, ctypes.c_int32
    assert _lib.SIGNATURES[NAME] == (ctypes.c_int, [p, p, i32, p, p, i32, p, p, i32, p])
    assert list(inspect.signature(BatchEngine.env_load_determinized_dev).parameters) == [
        "self", "entries_ptr", "n_entries", "src_ptr", "dst_ptr", "m", "seeds_ptr", "observers_ptr", "what", "loaded_ptr"]
    text = open(os.path.join(REPO, "include", "monsoon.h")).read()
    assert "#define MONSOON_DET_STREAM 1" in text and "#define MONSOON_DET_HAND 2" in text
    for ext, build in ((0, 0), (1, 0x10000), (2, 0x30000)):   # entries stay interchangeable: the version did not move
        assert _lib.load(ext).monsoon_version() == 0x1000003 | build


def test_python_surface():
    from monsoon_amd import vec_env
    assert list(inspect.signature(vec_env.VecEnv.determinize).parameters) == ["self", "snap", "seeds", "src", "dst", "observer", "what", "loaded"]
    assert inspect.signature(vec_env.VecEnv.determinize).parameters["what"].default == "hand"
    assert list(inspect.signature(vec_env.determinize_order).parameters) == ["seed", "n_movable", "n_deck"]
    assert vec_env.DETERMINIZE == {"stream": 1, "hand": 3} and "determinize_order" in vec_env.__all__
    for bad in ((0, 6, 3), (0, -1, 3), (0, 2, 13)):
        with pytest.raises(ValueError):
            vec_env.determinize_order(*bad)


def test_host_build_of_the_device_text_equals_numpy(tmp_path):
    """tests/determinize_check.cpp over monsoon_amd/csrc/determinize.h, built plain and once more under the address and UB
    sanitizers, both stand-alone: every (k, d) with k in 0..5 and d in 0..12, for the edge seeds and 200 consecutive ones."""
    from monsoon_amd.vec_env import determinize_order
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the oracle too"
    (tmp_path / "seeds.bin").write_bytes(np.array(SEEDS, dtype="<u4").tobytes())
    want = []
    for s in SEEDS:
        for k in range(6):
            for d in range(13):
                o = determinize_order(s, k, d)
                assert o.dtype == np.int64 and sorted(o.tolist()) == list(range(k + d))
                assert o.tolist() == M.order(s, k, d), (s, k, d)   # the test model's own text of the rule
                want.extend(o.tolist())
    want = np.array(want, dtype=np.uint8)
    src = os.path.join(REPO, "tests", "determinize_check.cpp")
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe, out = str(tmp_path / f"determinize_check_{name}"), tmp_path / f"order_{name}.bin"
        subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(REPO, "monsoon_amd", "csrc"), src, "-o", exe], check=True)
        r = subprocess.run([exe, str(tmp_path / "seeds.bin"), str(out)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.split() == ["ok", str(len(SEEDS))], r.stdout[-2000:] + r.stderr[-2000:]
        got = np.frombuffer(out.read_bytes(), dtype=np.uint8)
        assert np.array_equal(got, want), (name, len(got), len(want))
    # no-ops: nothing movable, or one hidden card in all
    assert determinize_order(5, 0, 7).tolist() == list(range(7)) and determinize_order(5, 1, 0).tolist() == [0]


def _entry(rs, to_play, hands, decks, flags=None, result=-2):
    """A standard-record entry of random bytes with what the rule reads put in: header, GameMeta.result, H_TOPLAY, the two
    players' counts, and the hand flags `flags` ({(side, position): flag bits}; every other hand entry carries none of
    CF_ALIAS / CF_STR)."""
    lay = entry_layout(0)
    e = rs.randint(0, 256, lay["entry_bytes"]).astype(np.uint8)
    e[:16] = np.array([SNAP_MAGIC, 0x1000003, lay["record_bytes"] // 4, 3], dtype="<u4").view(np.uint8)
    e[M.META_RESULT] = np.array([result], dtype=np.int8).view(np.uint8)[0]
    e[M.META_RNG:M.META_RNG + 4] = np.array([0x10123], dtype="<u4").view(np.uint8)
    e[M.BODY_AT + M.H_TOPLAY] = to_play
    for side in (0, 1):
        pl = M.player_at(side)
        e[pl + M.P_HAND_N], e[pl + M.P_DECK_N] = hands[side], decks[side]
        for p in range(M.HAND_CAP):
            e[pl + M.P_HAND + 4 * p + 2] &= ~np.uint8(M.CF_ALIAS | M.CF_STR)
    for (side, p), f in (flags or {}).items():
        e[M.player_at(side) + M.P_HAND + 4 * p + 2] |= f
    return e


def _cards(e, places):
    return [bytes(e[a:a + 4]) for a in places]


@pytest.mark.parametrize("observer", [0, 1, 255])
def test_model_keeps_what_the_rule_keeps(observer):
    rs = np.random.RandomState(7 + observer)
    lay = entry_layout(0)
    moved = 0
    for case in range(60):
        hands, decks = rs.randint(0, 6, 2), rs.randint(0, 13, 2)
        flags = {}
        if case % 3 == 1:
            flags[(case % 2, 0)] = M.CF_ALIAS
        if case % 3 == 2:
            flags[(1 - case % 2, 2)] = M.CF_STR
        e = _entry(rs, case % 2, hands, decks, flags)
        side = M.hidden_side(e, observer)
        assert side == (1 - observer if observer != 255 else 1 - case % 2)
        seed = int(rs.randint(0, 2**32, dtype=np.uint64))
        got = M.determinize_entry(e, seed, observer, "hand")
        hand, deck = M.hidden_places(e, side)
        assert sorted(_cards(got, hand + deck)) == sorted(_cards(e, hand + deck))   # the hidden multiset
        moved += _cards(got, hand + deck) != _cards(e, hand + deck)
        # everything but the moved places, the stream cursor and the stream: the observer's block, ages, counts, pinned entries
        same = np.ones(lay["mt_at"], dtype=bool)
        for a in hand + deck:
            same[a:a + 4] = False
        same[M.META_RNG:M.META_RNG + 4] = False
        assert np.array_equal(got[:lay["mt_at"]][same], e[:lay["mt_at"]][same]), case
        pl, other = M.player_at(side), M.player_at(1 - side)
        assert np.array_equal(got[other:other + M.PL_SIZE], e[other:other + M.PL_SIZE])
        assert np.array_equal(got[pl + M.P_AGE:pl + M.PL_SIZE], e[pl + M.P_AGE:pl + M.PL_SIZE]) and np.array_equal(got[pl:pl + M.P_HAND], e[pl:pl + M.P_HAND])
        for (s, p), _ in flags.items():
            if s == side and p < hands[side]:
                assert pl + M.P_HAND + 4 * p not in hand
        # the stream is the seed's, with the cursor at its start, in both modes
        stream = M.determinize_entry(e, seed, observer, "stream")
        assert np.array_equal(stream[:M.META_RNG], e[:M.META_RNG])
        assert np.array_equal(stream[M.META_RNG + 4:lay["mt_at"]], e[M.META_RNG + 4:lay["mt_at"]])
        assert not stream[M.META_RNG:M.META_RNG + 4].any() and not got[M.META_RNG:M.META_RNG + 4].any()
        assert np.array_equal(stream[lay["mt_at"]:], got[lay["mt_at"]:]) and not np.array_equal(got[lay["mt_at"]:], e[lay["mt_at"]:])
        mt, out = M.seeded_stream(seed)
        assert np.array_equal(got[lay["mt_at"]:lay["out_at"]].view("<u4"), mt) and np.array_equal(got[lay["out_at"]:].view("<u4"), out)
    assert moved >= 30   # a sixth of the cases has an empty hand; most others move something
    # an episode that ended, or whose end is pending, is loaded verbatim
    for result in (-1, 0, 1):
        e = _entry(rs, 0, (4, 4), (8, 8), result=result)
        assert np.array_equal(M.determinize_entry(e, 5, observer, "hand"), e)


def test_seeded_stream_is_numpys_generator():
    """The first tempered block is the first 624 draws of a fresh RandomState, and drawing on continues where the raw state
    stands: the 1 249th draw of the same generator is the first output after one more twist."""
    for seed in (0, 1, 0xFFFFFFFF, 12345):
        mt, out = M.seeded_stream(seed)
        rs = np.random.RandomState(seed)
        first = rs.randint(0, 2**32, 624, dtype=np.uint32)
        assert np.array_equal(out[:624], first)
        init = np.random.RandomState(seed).get_state()[1]
        assert init[0] == seed and not np.array_equal(init, mt)
        cont = np.random.RandomState(0)
        cont.set_state(("MT19937", mt, 624, 0, 0.0))
        rs.randint(0, 2**32, 624, dtype=np.uint32)
        assert np.array_equal(cont.randint(0, 2**32, 8, dtype=np.uint32), rs.randint(0, 2**32, 8, dtype=np.uint32))


def test_rule_deals_uniformly():
    """Seeds 0 .. 11 999, k = 4, d = 8.  Each of the 12 cards is in the hand 4 000 +- 207 times (4 sigma, sigma =
    sqrt(12 000 * 1/3 * 2/3) = 51.6) and at hand position 0 1 000 +- 122 times (4 sigma, sigma = sqrt(12 000 * 1/12 * 11/12)
    = 30.3): conditions on these seeds, which the rule meets (largest deviations 92 and 58)."""
    n, k, d = 12000, 4, 8
    seeds = np.arange(n, dtype=np.uint64)
    a = np.tile(np.arange(k + d), (n, 1))
    rows = np.arange(n)
    for i in range(k):
        r = hash32_array(seeds, i, 0xD7).astype(np.uint64)
        j = (i + ((r * np.uint64(k + d - i)) >> np.uint64(32))).astype(np.int64)
        a[rows, i], a[rows, j] = a[rows, j].copy(), a[rows, i].copy()
    from monsoon_amd.vec_env import determinize_order
    for s in (0, 1, 5999, 11999):
        assert a[s].tolist() == determinize_order(s, k, d).tolist()
    in_hand = np.bincount(a[:, :k].ravel(), minlength=k + d)
    at_zero = np.bincount(a[:, 0], minlength=k + d)
    print("in hand:", in_hand.tolist(), "largest deviation", int(np.abs(in_hand - 4000).max()))
    print("at position 0:", at_zero.tolist(), "largest deviation", int(np.abs(at_zero - 1000).max()))
    assert (np.abs(in_hand - 4000) <= 207).all()
    assert (np.abs(at_zero - 1000) <= 122).all()


def test_argument_errors_need_no_device():
    """what and the record build are judged before anything else: on an object that never opened a device."""
    from monsoon_amd.vec_env import MonsoonError, VecEnv
    env = VecEnv.__new__(VecEnv)
    env.engine, env.views, env.extended, env.device = None, None, 1, 0
    with pytest.raises(ValueError, match="what"):
        env.determinize(None, None, what="deck")
    with pytest.raises(ValueError, match='what="stream"'):
        env.determinize(None, None, what="hand")
    env.extended = 2
    with pytest.raises(ValueError, match='what="stream"'):
        env.determinize(None, None)
    env.extended = 0
    for bad in (2, -1, 255, True, "0", 1.0, [0]):
        with pytest.raises(ValueError, match="observer"):
            env.determinize(None, None, observer=bad)
    with pytest.raises(MonsoonError, match="before reset"):
        env.determinize(None, None, what="stream")
    with pytest.raises(MonsoonError, match="before reset"):
        env.determinize(None, None, observer=1)
