"""Games and described states for tests/test_wide_ab_gpu.py: the short ability effects of rules.h on whole words (the status
methods on the entity image, gain_speed through set_path_known, random.choice asked of the hit mask; state.h MSB_WIDE_AB_*).

Games: the 64 N12M games x 40 decisions of tests/wide_lists_trace.py (its trace, computed once for every test file that plays
them) and 64 games x 40 decisions on TOUCHED_DECK, twelve different cards whose abilities the change touches.  reached() replays
the committed actions of both on the recursive oracle, reads its canonical record before and after every step and counts per
touched card how often its ability ran for certain:
    ON_PLAY units and spells   the committed action plays the card
    ON_DEATH units             a unit of the card that is not disabled is on the board before the step and gone after it
    AFTER_SURVIVING units      the one unit of the card and owner is weaker after the step, and alive
    BEFORE_MOVING units        the turn is passed on to a unit of the card that is neither frozen nor disabled
check_reached() asserts that each of the 12 touched cards ran at least once.

Described states (tests/scenario_lib.py, built by the oracle's scn_build and by monsoon_debug_build from one description), for
what those games do not reach; reference() steps each on the recursive oracle and asserts that it is what it is named after:
    sat-*          s007 on a friendly unit that is vitalized 255 times: healed, then FAULT_STATUS_SAT
    swap-*         s007 on a poisoned friendly unit: it is healed, one poison less and vitalized
    u061-alone-*   u061 played with no other friendly unit: no pick, no draw for it; the unit confuses itself, gains two steps and
                   walks them, the first to the side (gain_speed of a confused unit)
    base-pick-*    u018 played beside one unit with one enemy unit on the board, over eight stream positions: the strike of
                   the play lands on the enemy's base in some and on its unit in others (the base comes behind the tiles)
    row4-speed-*   u050 placed on its owner's back row with nothing ahead: it gains three steps and stands three rows on
    alone-speed-*  u053 placed with nothing around it: it gains two steps
disable() on a unit without an ability cannot be reached by a step (ua07, the one card that disables, has an ability): the
host program tests/wide_ab_check.cpp holds it.

The games say that a pick ran, not which element of which list it drew.  Every call site of the pick -- the ten these games and
states do not reach among them (u076 u111 u305 u306 u313 u320 ud31, u018 beyond base-pick-*, EACH_U017, the scripted bot's spell
target) -- is stepped from described states on every index of the draw, under both list orders where a step reaches them, by
tests/pick_sites.py (tests/test_pick_sites_cpu.py, tests/test_pick_sites_gpu.py)."""
import numpy as np

import oracle_lib
import wide_ent_states as E
import wide_ent_trace as ET
import wide_lists_trace as T
from monsoon_amd.cards import CARD_INDEX, CARD_META, deck_indices

W0, W1 = T.W0, T.W1
TOUCHED_DECK = "u007 u021 u061 u053 u051 u050 ua07 ud01 u055 s007 s012 ue03".split()
# what the change touches: the deck but ue03 (its pick is over empty_shape_tiles, whose order is not the tile order: it keeps
# the list), and N12M's ue01 (the pick of its EACH_UE01 rounds)
TOUCHED = [c for c in TOUCHED_DECK if c != "ue03"] + ["ue01"]
TR_ON_PLAY, TR_ON_DEATH, TR_AFTER_SURVIVING, TR_BEFORE_MOVING = 0, 1, 4, 5
ST_FROZEN, ST_POISONED, ST_CONFUSED, ST_DISABLED, ST_VITALIZED = 0, 1, 2, 3, 4
FAULT_STATUS_SAT = 21
NUM_CARDS = len(CARD_META)
assert all(c in CARD_INDEX for c in TOUCHED) and len(set(TOUCHED_DECK)) == 12

_cache = {}


def trace(deck):
    """The oracle's line of 64 games x 40 decisions on `deck` ("N12M": tests/wide_lists_trace.py's own), in that module's layout."""
    if deck == "N12M":
        return T.trace(False)
    if "touched" in _cache:
        return _cache["touched"]
    n, decisions = len(T.SEEDS), T.DECISIONS
    seeds = [1000 + s for s in T.SEEDS]
    decks = np.broadcast_to(deck_indices(TOUCHED_DECK), (n, 2, 12))
    orc = oracle_lib.Oracle(n)
    for i in range(n):
        assert orc.reset(i, seeds[i], decks[i, 0], decks[i, 1]) == 0
    t = dict(action=np.full((decisions, n), 255, dtype=np.uint8), scores=np.full((decisions, n, 156), np.nan), best=np.full((decisions, n), np.nan),
             hash=np.zeros((decisions, n), dtype=np.uint64), live=np.zeros((decisions, n), dtype=bool), clean=np.ones((decisions, n), dtype=bool))
    dead, faulted = [False] * n, [False] * n
    for r in range(decisions):
        for i in range(n):
            if not dead[i] and orc.have_winner(i):
                dead[i] = True
            if not dead[i]:
                a, sc, _ = orc.decide(i, W0 if orc.to_play(i) == 0 else W1)
                t["action"][r, i], t["scores"][r, i], t["best"][r, i], t["live"][r, i] = a, sc, sc[a], True
                if orc.step(i, a)[0]:   # an exception while applying the action ends the game as a draw
                    dead[i] = faulted[i] = True
            t["hash"][r, i] = orc.canon_hash(i)
            t["clean"][r, i] = not faulted[i]
    for v in t.values():
        v.setflags(write=False)
    t["decks"], t["seeds"] = decks, seeds
    _cache["touched"] = t
    return t


def _count(a, before, after, ran):
    mover, _, hands, b0 = before
    _, _, _, b1 = after
    if a < 148:
        card = hands[mover][a // 16 if a < 64 else (a - 64) // 21]
        if card < NUM_CARDS and (CARD_META[card]["kind"] == 2 or CARD_META[card]["trigger"] == TR_ON_PLAY):
            ran[card] += 1
    units = lambda b, c, o: [e for e in b.values() if e["card"] == c and e["owner"] == o]
    for c in range(NUM_CARDS):
        trig = CARD_META[c]["trigger"] if CARD_META[c]["kind"] == 0 else -1
        for o in (0, 1):
            u0, u1 = units(b0, c, o), units(b1, c, o)
            if trig == TR_ON_DEATH and len(u1) < len(u0) and all(e["status"][ST_DISABLED] == 0 for e in u0) and not (a < 64 and hands[mover][a // 16] == c):
                ran[c] += 1
            if trig == TR_AFTER_SURVIVING and len(u0) == 1 == len(u1) and 0 < u1[0]["strength"] < u0[0]["strength"] and u0[0]["status"][ST_DISABLED] == 0:
                ran[c] += 1
            if trig == TR_BEFORE_MOVING and a == 155 and o == 1 - mover and any(e["status"][ST_FROZEN] == 0 and e["status"][ST_DISABLED] == 0 for e in u0):
                ran[c] += 1


def reached():
    """{card id: how often its ability ran for certain in the committed steps of the two sets of games}"""
    if "reached" in _cache:
        return _cache["reached"]
    ran = [0] * NUM_CARDS
    for deck in ("N12M", "touched"):
        t = trace(deck)
        decisions, n = t["action"].shape
        orc = oracle_lib.Oracle(n)
        for i in range(n):
            assert orc.reset(i, t["seeds"][i], t["decks"][i, 0], t["decks"][i, 1]) == 0
            for d in range(decisions):
                if not t["live"][d, i]:
                    break
                a = int(t["action"][d, i])
                before = ET.parse(orc.canon(i))
                if orc.step(i, a)[0]:
                    break
                assert orc.canon_hash(i) == int(t["hash"][d, i])
                _count(a, before, ET.parse(orc.canon(i)), ran)
    _cache["reached"] = {c: ran[CARD_INDEX[c]] for c in TOUCHED}
    return _cache["reached"]


def check_reached():
    """Each of the 12 touched abilities runs at least once in the 128 games."""
    r = reached()
    assert len(r) == 12 and all(v > 0 for v in r.values()), r


# ---- described states -----------------------------------------------------------------------------------------------------
TILE = 3 * 4 + 1                 # (1, 3)
PLACE = (4 - 3) * 4 + 1          # hand[0] onto it
BASE_PICK_POSITIONS = 8


def _idx(card_id):
    return CARD_INDEX[card_id]


def _state(lo, card_id, tiles):
    st = E.state(lo, _idx(card_id), tiles)
    if CARD_META[_idx(card_id)]["kind"] == 2:
        st["players"][lo]["hand"][0]["kind"] = "spell"
    return st


def _spell_at(tile):
    """hand[0], a spell: the action that a target on `tile` makes legal.  It takes effect one tile further on in the order y = 4..0,
    x = 0..3 (rules.h step_impl, the reference's countdown), so the states put the unit that is meant on tile + 1."""
    return 64 + 1 + (4 - tile // 4) * 4 + tile % 4


def states():
    """[(name, state, [action, ...], (seed, stream position) or None = numbered)]"""
    b = E.plain_units()
    assert CARD_META[_idx("u018")]["trigger"] == TR_ON_PLAY
    out = []
    for lo in (0, 1):
        vit = [0, 0, 0, 0, 255]
        out.append((f"sat-{lo}", _state(lo, "s007", {TILE: E.entity(b[1], lo, TILE, 3), TILE + 1: E.entity(b[0], lo, TILE + 1, 4, vit)}), [_spell_at(TILE)], None))
        out.append((f"swap-{lo}", _state(lo, "s007", {TILE: E.entity(b[1], lo, TILE, 3), TILE + 1: E.entity(b[0], lo, TILE + 1, 4, [0, 2, 0, 0, 0])}), [_spell_at(TILE)], None))
        out.append((f"u061-alone-{lo}", E.state(lo, _idx("u061"), {}), [PLACE], None))
        out.append((f"row4-speed-{lo}", E.state(lo, _idx("u050"), {}), [(4 - 4) * 4 + 2], None))
        out.append((f"alone-speed-{lo}", E.state(lo, _idx("u053"), {}), [PLACE], None))
        for k in range(BASE_PICK_POSITIONS):
            tiles = {TILE + 1: E.entity(b[0], lo, TILE + 1, 4), 1: E.entity(b[1], 1 - lo, 1, 9)}
            out.append((f"base-pick-{k}-{lo}", E.state(lo, _idx("u018"), tiles), [PLACE], (8100 + lo, 5 + 3 * k)))
    return out


def reference(core="oracle"):
    """dict(names, enc, seeds, pos, rows): rows = [(state k, action, fault, hash after)]; every case asserted to be what it is
    named after (on the recursive oracle; core="product": the host build of the product core, for the CPU comparison)."""
    if core in _cache:
        return _cache[core]
    import scenario_lib as S
    sts = states()
    assert len(sts) <= 64
    orc = oracle_lib.Oracle(1, core=core) if core != "oracle" else oracle_lib.Oracle(1)
    names, encs, seeds, poss, rows = [], [], [], [], []
    base_hits, unit_hits = [0, 0], [0, 0]
    for k, (name, st, actions, stream) in enumerate(sts):
        enc = S.encode_state(st)
        seed, pos = stream if stream is not None else (8000 + k, 3 + 2 * k)
        lo = int(name[-1])
        for a in actions:
            assert orc.scn_build(0, seed, pos, enc) == 0, name
            assert a in orc.legal_actions(0), (name, a, orc.legal_actions(0))
            _, bases0, _, before = ET.parse(orc.canon(0))
            f = orc.step(0, a)[0]
            rows.append((k, a, f, orc.canon_hash(0)))
            _, bases1, _, after = ET.parse(orc.canon(0))
            if name.startswith("sat"):
                assert f == FAULT_STATUS_SAT, (name, f)
                continue
            assert f == 0, (name, f)
            if name.startswith("swap"):
                e = after[TILE + 1]
                assert e["strength"] == 4 + 7 and e["status"][ST_POISONED] == 1 and e["status"][ST_VITALIZED] == 1, (name, e)
            elif name.startswith("u061-alone"):
                mine = [(t, e) for t, e in after.items() if e["card"] == _idx("u061")]
                # the path of its two gained steps: one confused step to the side, one ahead
                assert len(mine) == 1 and len(after) == 1 and mine[0][0] // 4 == TILE // 4 - 1 and mine[0][0] % 4 != TILE % 4, (name, after)
                assert mine[0][1]["status"][ST_CONFUSED] == 0, (name, after)
            elif name.startswith("row4-speed"):
                assert list(after) == [1 * 4 + 2] and after[1 * 4 + 2]["card"] == _idx("u050"), (name, after)
            elif name.startswith("alone-speed"):
                assert list(after) == [TILE - 8] and after[TILE - 8]["card"] == _idx("u053"), (name, after)
            elif name.startswith("base-pick"):
                base_hits[lo] += bases1[1 - lo] < bases0[1 - lo]
                unit_hits[lo] += any(e["owner"] == 1 - lo and e["strength"] < 9 for e in after.values()) or \
                    not any(e["owner"] == 1 - lo for e in after.values())
            else:
                raise AssertionError(name)
        names.append(name), encs.append(enc), seeds.append(seed), poss.append(pos)
    if core == "oracle":
        assert min(base_hits) > 0 and min(unit_hits) > 0, (base_hits, unit_hits)
    _cache[core] = dict(names=names, enc=encs, seeds=seeds, pos=poss, rows=rows)
    return _cache[core]
