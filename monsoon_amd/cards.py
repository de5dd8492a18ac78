"""Card ids <-> table indices, and the fixed decks of the benchmark configurations.

The table (monsoon_amd/card_ids.json, monsoon_amd/csrc/card_table.inc) is generated from the
reference's card constructors by oracle/pyref/gen_card_table.py; index = position in the sorted
id list (so index order == card_id string order, which the observation's deck sort relies on,
games/stormbound.py:441).
"""
import json
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(_HERE, "card_ids.json")) as _f:
    CARD_META = json.load(_f)
CARD_IDS = [c["id"] for c in CARD_META]
CARD_INDEX = {cid: i for i, cid in enumerate(CARD_IDS)}

# Cards that need the extended per-game record (BatchEngine(extended=True), libmonsoon_hip_ext.so):
# ua20 grows the deck, b005 keeps deep copies of its neighbours.  The standard build refuses them.
UNSUPPORTED = frozenset({"ua20", "b005"})
NEEDS_EXTENDED = UNSUPPORTED
# int(card) raises for these (card.py:46): every observation containing one faults.
FAULT_CARDS = frozenset({"up01", "up02", "up03"})

# SURVEY.md Appendix G / games/stormbound.py:295-302
DECKS = {
    "N12V": "u001 u002 u003 u019 u020 u025 u027 u030 u031 u032 u069 b001".split(),
    "N12M": "u001 u007 u020 u021 u026 u053 u061 ua07 ue01 s001 s012 b002".split(),
    "S12": "u040 u206 u211 u212 u216 u217 ue21 ue22 ut21 ut22 s203 b203".split(),
    "IRONCLAD": "ua07 u007 u306 u061 b304 u305 u320 u302 u313 ua02 ut32 u316".split(),
    "SWARM": "ua07 u007 u001 u053 ue01 u211 u206 u071 u020 s013 b001 u061".split(),
}


def deck_indices(deck):
    """12 card ids (or a DECKS key) -> uint8[12] table indices."""
    if isinstance(deck, str):
        deck = DECKS[deck]
    arr = np.array([CARD_INDEX[c] if isinstance(c, str) else int(c) for c in deck], dtype=np.uint8)
    if arr.shape != (12,):
        raise ValueError("a deck has exactly 12 cards")
    return arr


def supported_pool(include_fault_cards=False, extended=False):
    return [c for c in CARD_IDS if (extended or c not in UNSUPPORTED) and (include_fault_cards or c not in FAULT_CARDS)]


# THE RULE, stated here once for the Python layer (msb_base.h deck_repeated_card states it for the
# native side): a deck pair needs the extended record if a deck holds ua20 / b005, or lists a unit or structure card
# more than once.  Unit / Structure equality is (card_id, player, position), so the reference's deck.remove(drawn card)
# takes the first EQUAL object: the drawn one stays in the deck while it also sits in the hand, and ages there.  Only
# the extended record (object ids, a weight per object) can express that; the standard build refuses such a deck.  A
# spell compares by identity, and a card both players hold is no repeat (equality includes the player).  up01 / up02 /
# up03 may repeat too: the shared object ages only in its owner's own play or cycle, and that owner never completes a
# step (the step's observation shows the card and raises, which ends the game: FAULT_CARDS).
_KIND_SPELL = 2
_REPEATABLE = np.array([c["kind"] == _KIND_SPELL or c["id"] in FAULT_CARDS for c in CARD_META], dtype=bool)   # by card index: may be listed twice


def _as_indices(decks):
    flat = [CARD_INDEX[c] if isinstance(c, str) else int(c) for c in np.asarray(decks, dtype=object).ravel()]
    if len(flat) % 12:
        raise ValueError("decks of exactly 12 cards")
    return np.array(flat, dtype=np.uint8).reshape(-1, 12)


def repeats_card(decks):
    """bool[n]: which 12-card decks (indices [n][12]) list a unit or structure card more than once."""
    decks = np.asarray(decks, dtype=np.uint8).reshape(-1, 12)
    s = np.sort(decks, axis=1)
    return ((s[:, 1:] == s[:, :-1]) & ~_REPEATABLE[s[:, 1:]]).any(axis=1)


def _deck_needs_extended(decks):
    """bool[n] for 12-card decks [n][12] (indices): the rule above."""
    return np.isin(decks, [CARD_INDEX[c] for c in NEEDS_EXTENDED]).any(axis=1) | repeats_card(decks)


def needs_extended(decks):
    """True if any deck (12 ids or indices each) needs the extended build: it holds ua20 / b005, or repeats a unit or
    structure card (the rule above)."""
    return bool(_deck_needs_extended(_as_indices(decks)).any())


def needs_extended_each(deck_pairs):
    """bool[n]: which deck pairs [n][2][12] (card indices) need the extended build (either deck does, by the rule above)."""
    decks = np.asarray(deck_pairs, dtype=np.uint8).reshape(-1, 12)
    return _deck_needs_extended(decks).reshape(-1, 2).any(axis=1)


# Configuration C5: every game draws its two decks from the 109 observable cards -- every card but
# up01/up02/up03, whose int(card) raises (card.py:46) and would end half of the games before their first step -- with a
# pre-stream of its own: RandomState(seed ^ C5_STREAM_XOR).choice(pool, 12, replace=False), P1's deck first.
RANDOM_DECK = "random109"
C5_STREAM_XOR = 0x9E3779B9


def observable_pool():
    return np.array([i for i, c in enumerate(CARD_IDS) if c not in FAULT_CARDS], dtype=np.uint8)


def draw_random_decks_numpy(seeds, pool=None):
    """The specification of monsoon_draw_decks, by numpy itself (150 us per game: tests and small schedules only)."""
    pool = observable_pool() if pool is None else np.asarray(pool, dtype=np.uint8)
    out = np.zeros((len(seeds), 2, 12), dtype=np.uint8)
    for k, s in enumerate(seeds):
        rs = np.random.RandomState(int(s))
        out[k, 0], out[k, 1] = rs.choice(pool, 12, replace=False), rs.choice(pool, 12, replace=False)
    return out
