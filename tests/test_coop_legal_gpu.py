"""The legal set that the wavefront-per-game kernels compute with the whole wave from tile and hand masks
(monsoon_amd/csrc/coop_legal.h, kernels.h legal_set) against the serial legal_mask_v() of monsoon_legal_mask (k_legal) and
against the CPU oracle, on every standard-record variant of the hot kernel.

The states are described once (tests/scenario_lib.py), built by monsoon_debug_build and by the oracle's scn_build from the
same description, saved with monsoon_state_save and loaded into the handle under test with monsoon_state_load, the way
tests/test_cycle_draw_gpu.py loads its blobs; the oracle's side is computed once for all variants.  They are the smallest
shapes at which the wave form can go wrong: hands of 0..5 cards (slot 4 lands in the second mask word, a spell there runs
into 148..155 and past the action space), mana 0 and mana equal to a cost, the front line at each of 0..4 for either side
to move, a full board, a board whose only empty tiles are in row 0 (front line 0: action 155; front line 1: no PLACE), an
untargeted spell, a targeted spell with no target and with its one target on each of the 20 tiles, the filters the card
table's spells use -- exclude-status (s021), strength limit with any kind on the friendly side (s105), enemy / friendly units
(s001 / s007) -- over boards that mix matching and non-matching entities, two and five targeted spells in one hand, the
replace flag set and cleared, and nothing playable.  No spell of the card table filters by unit type or non-hero or may
target a base: those descriptors reach get_targets from abilities only, and tests/coop_legal_check.cpp covers them with
synthetic descriptors against get_targets() on the host.

For each state one decision of k_play with scores (monsoon_decide): the scored actions (not NaN) are exactly the bits of
monsoon_legal_mask and of the oracle's mask, the look-ahead count the decision added to the game's row equals their number,
the scores equal the oracle's bit for bit, and the committed successor has the canonical hash of the oracle's after the
same action."""
import numpy as np
import pytest

import kernel_variants

pytestmark = pytest.mark.gpu

W0 = np.random.RandomState(2024).uniform(0, 1, 10)
BLOB_META_LOOKAHEAD = 8 + 20  # GameMeta.lookahead in a blob of monsoon_state_save (monsoon_hip.hip k_blob, kernels.h GameMeta)
UNIT, UNIT2, STRUCT = "u025", "u001", "b001"   # plain cards (no abilities) to hold and to stand on the board


def _meta():
    from monsoon_amd.cards import CARD_INDEX, CARD_META
    return CARD_INDEX, CARD_META


def _card(cid, cost=None):
    index, meta = _meta()
    m = meta[index[cid]]
    return dict(card=index[cid], cost=m["cost"] if cost is None else cost, single_use=False, ff=bool(m["ff"]),
                kind="spell" if m["kind"] == 2 else "other", strength=m["strength"], position=None, age=0)


def _entity(cid, owner, tile, strength=3, status=None):
    index, meta = _meta()
    m = meta[index[cid]]
    return dict(card=index[cid], owner=owner, strength=strength, movement=m["movement"], ff=bool(m["ff"]),
                status=status or [0] * 5, position=[tile % 4, tile // 4], damage_taken=0, single_use=False)


def _state(lo, hand, mana, front=None, tiles=None, replacable=True):
    """A PLAY-phase state with `lo` to move; hand: card ids or (id, cost); tiles: {tile: entity}."""
    players = []
    for o in range(2):
        mine = o == lo
        cards = [_card(*(c if isinstance(c, tuple) else (c,))) for c in (hand if mine else [UNIT, UNIT2])]
        deck = [_card(c) for c in (UNIT, UNIT2, STRUCT, "s012", UNIT, UNIT2)]
        for k, c in enumerate(cards + deck):
            c["oid"] = k
        for k, c in enumerate(deck):
            c["age"] = k
        players.append(dict(base=12, mana=mana if mine else 3, max_mana=9, front=(4 if o == 0 else 0) if (front is None or not mine) else front,
                            replacable=replacable if mine else True, leftmost_movable=True, faction=0, hand=cards, deck=deck))
    board = [None] * 20
    for t, e in (tiles or {}).items():
        board[t] = e
    return dict(local_order=lo, cp=lo, phase=1, resolving=False, history=[], players=players, tiles=board)


def _states():
    out = []
    some = {t: _entity(UNIT, t % 2, t) for t in (1, 6, 8, 15, 18)}   # every row keeps empty tiles
    full = {t: _entity(UNIT if t % 3 else STRUCT, (t // 2) % 2, t, 2 + t % 9) for t in range(20)}
    row0_open = {t: e for t, e in full.items() if t >= 4}
    for n in range(6):   # hand sizes; costs 0..4, all within reach
        out.append((f"hand{n}", _state(n % 2, [(UNIT, k) for k in range(n)], 4, 2 + n % 2, some)))
    out.append(("mana0", _state(0, [(UNIT, 0), (UNIT2, 1), ("s012", 0), ("s021", 0)], 0, 3, some)))
    out.append(("mana-equals-cost", _state(1, [(UNIT, 3), (UNIT2, 4), ("s012", 3), ("s021", 3), (STRUCT, 2)], 3, 1, some)))
    for lo in (0, 1):
        for fl in range(5):
            out.append((f"front{fl}-side{lo}", _state(lo, [UNIT, STRUCT, "s007", "s012"], 5, fl, some)))
    out.append(("full-board", _state(0, [UNIT, "s001", "s105", "s012"], 9, 2, full)))
    out.append(("row0-only-front0", _state(1, [UNIT, STRUCT, "s012"], 6, 0, row0_open)))
    out.append(("row0-only-front1", _state(0, [UNIT, STRUCT], 6, 1, row0_open)))
    out.append(("untargeted-alone", _state(0, ["s012"], 1, 4, {})))
    out.append(("untargeted-slot4", _state(1, [(UNIT, 9), (UNIT, 9), (UNIT, 9), (UNIT, 9), "s012"], 2, 0, some)))
    out.append(("targeted-no-target", _state(0, ["s021", (UNIT, 9)], 2, 4, {})))
    for t in range(20):   # the one target on each tile, the spell in slot t % 5 behind cards out of reach
        hand = [(UNIT, 9)] * (t % 5) + ["s021"]
        out.append((f"target-tile{t}", _state(t % 2, hand, 2, 2, {t: _entity(UNIT, (t // 2) % 2, t)})))
    confused = {t: _entity(UNIT, t % 2, t, 3, [0, 0, 1 if t % 3 == 0 else 0, 1 if t % 4 == 0 else 0, 0]) for t in (0, 3, 4, 9, 12, 13, 19)}
    confused[7] = _entity(STRUCT, 0, 7)
    out.append(("exclude-status", _state(0, ["s021", UNIT], 9, 2, confused)))
    limit = {t: _entity(UNIT if t % 2 else STRUCT, (t // 4) % 2, t, s) for t, s in ((0, 10), (2, 11), (5, 10), (7, 11), (9, 1), (12, 10), (14, 12), (19, 9))}
    for lo in (0, 1):
        out.append((f"limit-friendly-any-kind-side{lo}", _state(lo, [(UNIT, 9), "s105"], 9, 1, limit)))
    out.append(("enemy-and-friendly-units", _state(1, ["s001", "s007", UNIT], 9, 1, limit)))
    out.append(("two-targeted", _state(0, [(UNIT, 9), "s104", (UNIT, 9), "s007"], 4, 3, full)))
    out.append(("five-targeted", _state(1, ["s001", "s007", "s021", "s104", "s105"], 9, 0, full)))
    out.append(("five-targeted-few-targets", _state(0, ["s001", "s007", "s021", "s104", "s105"], 9, 4, some)))
    for flag in (True, False):
        out.append((f"replace-{'set' if flag else 'cleared'}", _state(0, [UNIT, STRUCT, "s012", (UNIT2, 9)], 4, 3, some, flag)))
    out.append(("nothing-playable", _state(1, [(UNIT, 5), ("s021", 2), ("s012", 1), (STRUCT, 3)], 0, 0, some, False)))
    out.append(("nothing-playable-may-replace", _state(0, [(UNIT, 5), ("s021", 2)], 1, 4, {}, True)))
    return out


def _bits(mask):
    return {a for a in range(156) if (int(mask[a >> 6]) >> (a & 63)) & 1}


@pytest.fixture(scope="module")
def reference():
    """Once for all variants: the blobs of the states, and the oracle's mask, scores, action and successor hash of each."""
    import oracle_lib
    import scenario_lib as S
    from monsoon_amd.engine import BatchEngine
    states = _states()
    assert len(states) <= 64
    build = BatchEngine(len(states))
    orc = oracle_lib.Oracle(len(states))
    ref = []
    for k, (name, st) in enumerate(states):
        enc = S.encode_state(st)
        assert build.debug_build(k, 4000 + k, 3 * k, enc) == 0, name
        assert orc.scn_build(k, 4000 + k, 3 * k, enc) == 0, name
    blobs = [build.save_state(k) for k in range(len(states))]
    build.close()
    for k, (name, st) in enumerate(states):
        mask = orc.legal_mask(k)
        a, scores, mask2 = orc.decide(k, W0)
        assert np.array_equal(mask, mask2)
        f, _, _ = orc.step(k, a)
        ref.append(dict(name=name, legal=_bits(mask), action=a, scores=scores, fault=f, hash=orc.canon_hash(k)))
    # the cases are what they are named after
    by = {r["name"]: r for r in ref}
    assert by["nothing-playable"]["legal"] == {155} and by["targeted-no-target"]["legal"] == {148, 149, 155}
    assert by["row0-only-front0"]["legal"] >= {155, 64 + 21 * 2} and not by["row0-only-front0"]["legal"] & set(range(64))
    assert not by["row0-only-front1"]["legal"] & set(range(64)) and 155 in by["row0-only-front1"]["legal"]
    assert by["untargeted-slot4"]["legal"] >= {148} and by["hand5"]["legal"] & set(range(64, 80))
    for t in range(20):   # 65 + 21 c + (4 - y) * 4 + x, which slot 4 carries into 149 .. 155 and past the end
        a = 65 + 21 * (t % 5) + (4 - t // 4) * 4 + t % 4
        assert (by[f"target-tile{t}"]["legal"] & set(range(65, 148))) == ({a} if a < 148 else set()), t
        assert a >= 156 or a in by[f"target-tile{t}"]["legal"], t
    assert by["five-targeted"]["legal"] & set(range(149, 155))
    assert not by["replace-cleared"]["legal"] & set(range(148, 152)) and by["replace-set"]["legal"] >= {148, 149, 150, 151}
    return blobs, ref


CASES = [(u, w) for u, w in kernel_variants.variants(False)]


@pytest.mark.parametrize("u,w", CASES, ids=[f"{u}x{w}" for u, w in CASES])
def test_decision_scores_exactly_the_serial_legal_set(monkeypatch, reference, u, w):
    from monsoon_amd.engine import BatchEngine
    blobs, ref = reference
    K = len(blobs)
    kernel_variants.select(monkeypatch, u, w)
    eng = BatchEngine(K)
    assert eng.variant() == (u, w)
    for k, bl in enumerate(blobs):
        eng.load_state(k, bl)
    serial = eng.legal_mask()   # k_legal: rules.h legal_mask_v, a lane per game
    action, _, scores = eng.decide(W0, want_scores=True)
    hashes = eng.state_hash()
    faults = eng.game_faults()
    for k, r in enumerate(ref):
        name = r["name"]
        assert _bits(serial[k]) == r["legal"], (name, sorted(_bits(serial[k]) ^ r["legal"]))
        scored = {a for a in range(156) if not np.isnan(scores[k, a])}
        assert scored == r["legal"], (name, sorted(scored ^ r["legal"]))
        added = int.from_bytes(eng.save_state(k)[BLOB_META_LOOKAHEAD:BLOB_META_LOOKAHEAD + 4], "little") - \
            int.from_bytes(blobs[k][BLOB_META_LOOKAHEAD:BLOB_META_LOOKAHEAD + 4], "little")
        assert added == len(r["legal"]), (name, added, len(r["legal"]))
        legal = sorted(r["legal"])
        assert np.array_equal(scores[k, legal].view(np.uint64), r["scores"][legal].view(np.uint64)), name
        assert int(action[k]) == r["action"], (name, int(action[k]), r["action"])
        assert (faults[k] == r["fault"] or (not r["fault"] and faults[k] >= 16)), (name, int(faults[k]), r["fault"])
        if not r["fault"]:
            assert int(hashes[k]) == r["hash"], name
    eng.close()
