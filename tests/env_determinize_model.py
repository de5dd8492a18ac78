"""Python model of a determinized load (include/monsoon.h monsoon_env_load_determinized_dev; test helper): the bytes of the
entry that a snapshot of the loaded slot gives, from the bytes of the source entry.

The layout is the standard record's (monsoon_amd/csrc/state.h; the constants of tests/test_cycle_draw_gpu.py) inside an
entry of tests/env_snapshot_model.py.  The rule is written out here on its own -- fitness.hash32 in scalar form and a list
that is swapped -- and not taken from monsoon_amd.vec_env.determinize_order, which the CPU tests compare with it.  The
stream comes from numpy: RandomState(seed).randint(0, 2**32, 1248, dtype=uint32) is the generator's raw output, the two
tempered blocks a seeded slot holds, and the state it leaves behind (two twists after init_genrand) is the raw state that
goes with them.
"""
import numpy as np

from env_snapshot_model import BODY_AT, HEAD_BYTES, entry_layout
from monsoon_amd.fitness import hash32

H_TOPLAY, OFF_PL, PL_SIZE = 0, 80, 96
P_HAND_N, P_DECK_N, P_HAND, P_DECK, P_AGE = 9, 10, 12, 32, 80
HAND_CAP, DECK_CAP, MT_N = 5, 12, 624
CF_SINGLE_USE, CF_FF, CF_STR, CF_ALIAS = 1, 2, 4, 8
META_RESULT, META_RNG = HEAD_BYTES + 8, HEAD_BYTES + 16   # GameMeta.result (int8), GameMeta.rng (u32) inside the entry
WHAT = ("stream", "hand")


def seeded_stream(seed):
    """(rng_mt, rng_out) of a slot whose stream is RandomState(seed) at its start: uint32 [624], [1248]."""
    rs = np.random.RandomState(int(seed) & 0xFFFFFFFF)
    out = rs.randint(0, 2**32, 2 * MT_N, dtype=np.uint32)
    state = rs.get_state()
    assert state[2] == MT_N   # both blocks used up: the raw state is the one the second block was made from
    return np.asarray(state[1], dtype=np.uint32), out


def order(seed, k, d):
    """The index in A = movable hand entries + deck entries of the entry that each place receives."""
    a = list(range(k + d))
    for i in range(k):
        r = hash32(int(seed) & 0xFFFFFFFF, i, 0xD7)
        j = i + ((r * (k + d - i)) >> 32)
        a[i], a[j] = a[j], a[i]
    return a


def player_at(side):
    """Offset of a player's block inside the entry."""
    return BODY_AT + OFF_PL + PL_SIZE * side


def hidden_side(entry, observer):
    return 1 - (int(observer) if observer != 255 else int(entry[BODY_AT + H_TOPLAY]) & 1)


def hidden_places(entry, side):
    """Entry offsets of the 4-byte entries the re-draw moves: the movable hand positions, then the deck."""
    pl = player_at(side)
    hn, dn = int(entry[pl + P_HAND_N]), int(entry[pl + P_DECK_N])
    movable = [p for p in range(hn) if not entry[pl + P_HAND + 4 * p + 2] & (CF_ALIAS | CF_STR)]
    return [pl + P_HAND + 4 * p for p in movable], [pl + P_DECK + 4 * i for i in range(dn)]


def determinize_entry(entry_bytes, seed, observer=255, what="hand", extended=0):
    """The entry of the slot that received `entry_bytes` (a uint8 array, one entry of record build `extended`) by a
    determinized load with this seed, observer byte (0, 1, 255) and mode."""
    assert what in WHAT and observer in (0, 1, 255)
    lay = entry_layout(extended)
    e = np.array(entry_bytes, dtype=np.uint8, copy=True)
    assert len(e) == lay["entry_bytes"]
    if e[META_RESULT:META_RESULT + 1].view(np.int8)[0] != -2:
        return e   # ended or end pending: verbatim
    if what == "hand":
        assert extended == 0, "the hand is re-dealt on the standard record only"
        hand, deck = hidden_places(e, hidden_side(e, observer))
        places = hand + deck
        if hand and len(places) > 1:
            cards = [e[a:a + 4].copy() for a in places]
            for a, src in zip(places, order(seed, len(hand), len(deck))):
                e[a:a + 4] = cards[src]
    mt, out = seeded_stream(seed)
    e[META_RNG:META_RNG + 4] = 0
    e[lay["mt_at"]:lay["out_at"]] = mt.astype("<u4").view(np.uint8)
    e[lay["out_at"]:] = out.astype("<u4").view(np.uint8)
    return e
