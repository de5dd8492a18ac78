"""Every call site of an ability's random pick (rules.h Pick / choice_tile, state.h MSB_WIDE_AB_PICK), from described states,
on every index the draw can give: the case table, a plain model of the list each card draws from, and the reference that
tests/test_pick_sites_cpu.py and tests/test_pick_sites_gpu.py share.

The sixteen sites (SITES) and how each ability is made to run (the modes):
    place         an ON_PLAY unit is placed on tile C = (1, 2) by the player to move                    u021 u061 u305 u306 u018 u017
    attack        u313 placed one row below a weaker enemy on C: it stands on C when AFTER_ATTACKING runs
    death_opp     the unit stands on C at strength 1 and the opponent, to move, places a unit under it: ON_DEATH in the
                  other player's turn, the point of view is not the local player                         u007 u111 ud01
    death_own     the unit at strength 1 below an enemy structure when the turn is passed to its owner (action 155 from a
                  state with mana 0, the board described flipped as tests/wide_ent_states.py does): it dies of its own move
    survive       u076 is struck by the opponent's placement and survives it; the striker is alive until its attack is over
                  and stands in the list: a draw that lands on it shows in the stream's cursor alone
    survive_opp   ue01 the same, struck for 1: one round of EACH_UE01 in the other player's turn
    survive_own   u076 / ue01 is the one other friendly entity when its owner places u306 in a far corner: u306's list of one
                  draws nothing and strikes it for 1 (ue01: one round of EACH_UE01 in its owner's turn)
    pass          u320 when the turn is passed to its owner, every other unit of that player frozen (BEFORE_MOVING)
    pass_attack   ud31 the same with an enemy unit ahead (BEFORE_ATTACKING)
    spell         s012 played from the hand; its order is the caster's ORDER, not a point of view: both through lo
    bot           expert_action on a state whose one card at the cost of the mana is a targeted spell (s021)
Each mode is built for both local orders lo.  A (site, order) pair that no step reaches is in UNREACHABLE with its reason, and
lengths a site cannot have in LENGTHS_OUT.

The plain model (model_list) is the reference's card text over board.py's get_targets: the matching tiles in ascending tile
order when the point of view is the local player, descending otherwise; the descriptor's bases behind the tiles; the caster's
tile removed where the card removes it; the card's type and status filters.  The draw is numpy's randint over the list's
length on the game's stream (model_draw, from the stream's own words: orc_rng_u32), so the model says for every (state, stream
position) which element is drawn and where the stream's cursor stands afterwards.  The recursive oracle and the device are both
held to it: reference() steps every state from consecutive stream positions (at most CAP) on the oracle, reads the canonical
record before and after, asserts that the one element that changed is model_list[r] and that the cursor is the model's, and
keeps the first position that gives each r = 0..n-1 (each state has one seed, fixed by _seed_for, which says how it is chosen).
check_coverage() asserts that nothing is missing, and that within a state the oracle's decision scores the triggering action
differently at two kept positions -- which is what lets the hot kernel's score row see the pick; SCORE_BLIND and SCORE_PARTLY
name the sites where it cannot, u061 among them."""
import ctypes

import numpy as np

import oracle_lib
import scenario_lib as S
import wide_ent_states as E
import wide_ent_trace as ET
import wide_lists_trace as T
from monsoon_amd.cards import CARD_INDEX, CARD_META

W0, W1 = T.W0, T.W1
CAP = 64                      # stream positions walked per state
POS0, SEED0 = 3, 8800
FAULT_PY_EXCEPTION = 1
UT_CONSTRUCT, UT_DRAGON = 0, 11
ST_CONFUSED = 2
UT_KNIGHT = 2
TOKEN_KNIGHT = len(CARD_META) + UT_KNIGHT   # canonical records name a token unit by its type, behind the cards

C = 2 * 4 + 1                 # the caster's tile when its ability runs, (1, 2)
UNDER, AHEAD = C + 4, C - 4
SURROUNDING = [t for t in range(20) if t != C and abs(t % 4 - C % 4) <= 1 and abs(t // 4 - C // 4) <= 1]
BORDERING = [t for t in SURROUNDING if abs(t % 4 - C % 4) + abs(t // 4 - C // 4) == 1]
# where the n targets go: different rows first, so that the look-ahead's features of two draws differ
ORDER_SUR = [4, 14, 10, 8, 6, 12, 5, 13]
ORDER_BOR = [8, 13, 10, 5]
ORDER_BOARD = [0, 19, 6, 15, 10, 3, 16, 12, 5, 14, 1, 18, 7]
ORDER_OUT = [19, 3, 16, 0]    # a matching unit outside a selector

_DPOV = "the point of view is board.current_player, and cp() is local() whenever a step runs an ability (the step toggles the local player before the turn's frame sets cp)"
_OWN = "the trigger runs only in its owner's turn, when its owner is the local player"

# pov: whose list it is ("me" the caster's owner, "cp" board.current_player); sel: the selector; kind / side / types / xtypes /
# xstatus: the card's descriptor; base: include_base; exclude: the caster's own tile is taken out; empty: what an empty list does
SITES = {
    "u007": dict(card="u007", pov="me", sel="sur", kind="unit", side="enemy", modes=["death_own", "death_opp"]),
    "u021": dict(card="u021", pov="cp", sel="board", kind="unit", side="friendly", exclude=True, modes=["place"]),
    "u061": dict(card="u061", pov="cp", sel="board", kind="unit", side="friendly", exclude=True, modes=["place"]),
    "u076": dict(card="u076", pov="cp", sel="sur", kind="unit", side="any", xtypes=1 << UT_DRAGON, modes=["survive_own", "survive"]),
    "u111": dict(card="u111", pov="me", sel="sur", kind="unit", side="friendly", modes=["death_own", "death_opp"], draws=10),
    "u305": dict(card="u305", pov="cp", sel="bor", kind="unit", side="friendly", types=1 << UT_CONSTRUCT, modes=["place"]),
    "u306": dict(card="u306", pov="cp", sel="board", kind="any", side="friendly", exclude=True, modes=["place"]),
    "u313": dict(card="u313", pov="cp", sel="sur", kind="unit", side="friendly", modes=["attack"]),
    "u320": dict(card="u320", pov="me", sel="sur", kind="unit", side="friendly", modes=["pass"]),
    "ud01": dict(card="ud01", pov="me", sel="board", kind="unit", side="friendly", types=1 << UT_DRAGON, modes=["death_own", "death_opp"]),
    "ud31": dict(card="ud31", pov="me", sel="sur", kind="unit", side="friendly", types=1 << UT_DRAGON, modes=["pass_attack"]),
    "s012": dict(card="s012", pov="order", sel="front", modes=["spell"]),
    "u018": dict(card="u018", pov="cp", sel="board", kind="any", side="enemy", base=True, modes=["place"]),
    "ue01": dict(card="ue01", pov="me", sel="board", kind="unit", side="enemy", modes=["survive_own", "survive_opp"]),
    "u017": dict(card="u017", pov="cp", sel="board", kind="unit", side="enemy", modes=["place"], empty="raise", spell="s001"),
    "bot": dict(card="s021", pov="cp", sel="board", kind="unit", side="any", xstatus=1 << ST_CONFUSED, modes=["bot"], empty="raise"),
}
# the orders a site's modes reach: True = ascending (pov == local()), False = descending
ORDERS = {"death_own": True, "death_opp": False, "survive_opp": False}
UNREACHABLE = {   # (site, ascending): why no step gets there
    ("u021", False): _DPOV, ("u061", False): _DPOV, ("u076", False): _DPOV, ("u305", False): _DPOV, ("u306", False): _DPOV,
    ("u313", False): _DPOV, ("u018", False): _DPOV, ("u017", False): _DPOV, ("bot", False): _DPOV,
    ("u320", False): "BEFORE_MOVING: " + _OWN, ("ud31", False): "BEFORE_ATTACKING: " + _OWN,
}
# lengths a site cannot have, with the reason
LENGTHS_OUT = {
    ("u007", "death_own", 8): "the enemy structure it dies on stands on one of the eight tiles and is no unit",
    ("u111", "death_own", 8): "the enemy it dies on stands on one of the eight tiles",
    ("u111", "death_opp", 8): "the unit that killed it stands on one of the eight tiles",
    ("u076", "survive", 0): "the unit that struck it is alive until its attack is over, stands beside it and is no dragon",
    ("ue01", "survive_opp", 0): "the unit that struck it is alive until its attack is over and is an enemy unit",
    ("u313", "attack", 8): "the tile it attacked from is one of the eight and empty",
    ("ud31", "pass_attack", 8): "the enemy unit ahead stands on one of the eight tiles",
    ("u018", "place", 0): "the enemy base is always in the list",
    ("bot", "bot", 0): "a targeted spell without a target is not in legal_mask, so expert_action never holds it as playable: the "
                       "empty list of rules.h expert_action is dead text for states a game reaches",
}
# Sites whose pick the score row of a decision cannot see: in no state do two kept positions give the triggering action
# another score.  check_coverage() asserts that too, so that a site does not stay here when it no longer belongs.
SCORE_BLIND = {
    "u061": "it only confuses the drawn unit: no feature of the one-step look-ahead reads a status, and the oracle's decision never "
            "commits the placement in these states, so the hash behind the commit does not carry it either; the step kernels "
            "(monsoon_step, the vector env) hold u061's pick on the device, the hot kernel does not",
    "bot": "its pick is no part of a step: no look-ahead calls expert_action",
}
# ... and sites where some states do not: at least one list length of every (mode, local order) does
SCORE_PARTLY = {
    "u111": "ten draws of +1 each: the kept positions are named after the first, and in some states the ten draws of "
            "two kept positions add up to the same strength on every target",
}
LENGTHS = {"sur": [0, 1, 2, 3, 4, 5, 8], "bor": [0, 1, 2, 3, 4], "board": [0, 1, 2, 3, 4, 5, 8, 9], "front": [0, 1, 2, 3, 4, 5, 8, 9]}

_cache = {}


def _idx(cid):
    return CARD_INDEX[cid]


def _ent(cid, owner, tile, strength, status=None):
    return E.entity(_idx(cid), owner, tile, strength, status)


def lengths(site, mode):
    s = SITES[site]
    out = []
    for n in LENGTHS[s["sel"]]:
        if (site, mode, n) in LENGTHS_OUT:
            if n == 8 and (site, mode, 7) not in LENGTHS_OUT:
                out.append(7)    # the most the site can have
            continue
        out.append(n)
    return out


# ---- the plain model --------------------------------------------------------------------------------------------------------
def _is_struct(e):
    return CARD_META[e["card"]]["kind"] == 1


def _matches(s, e, pov):
    if e["strength"] <= 0:
        return False
    if _is_struct(e):
        ok = s["kind"] == "any"
    else:
        ty = CARD_META[e["card"]]["types"]
        ok = (not s.get("types") or ty & s["types"]) and not (ty & s.get("xtypes", 0))
        ok = ok and not any(e["status"][k] for k in range(5) if s.get("xstatus", 0) >> k & 1)
    side = s["side"]
    return bool(ok) and (side == "any" or (side == "friendly") == (e["owner"] == pov))


def model_list(site, frame, pov, local):
    """The list the card draws from: tiles, then ("base", owner).  frame: {tile: entity} as the board stands when the ability runs,
    in the local player's view; the caster on C."""
    s = SITES[site]
    asc = pov == local
    if s["sel"] == "front":   # Player.get_within_front_line without the occupied tiles: the caster's ORDER sets rows and direction
        fl = 2
        tiles = [4 * y + x for y in range(fl, 5) for x in range(4)] if pov == 0 else [4 * y + x for y in range(fl, -1, -1) for x in range(3, -1, -1)]
        return [t for t in tiles if t not in frame]
    within = {"sur": SURROUNDING, "bor": BORDERING, "board": list(range(20))}[s["sel"]]
    out = [t for t in (range(20) if asc else range(19, -1, -1)) if t in within and t in frame and _matches(s, frame[t], pov)]
    if s.get("base"):   # the point of view's own base first
        out += [("base", o) for o, want in ((pov, "friendly"), (1 - pov, "enemy")) if s["side"] in (want, "any")]
    if s.get("exclude") and C in out:
        out.remove(C)
    return out


def model_draw(words, cursor, n):
    """numpy's randint(0, n) on the stream: (r, cursor behind it).  A list of one draws nothing."""
    if n <= 1:
        return 0, cursor
    mask = (1 << (n - 1).bit_length()) - 1
    while True:
        v = int(words[cursor]) & mask
        cursor += 1
        if v <= n - 1:
            return v, cursor


# ---- the states -------------------------------------------------------------------------------------------------------------
def _target_card(s):
    if s.get("types", 0) >> UT_DRAGON & 1:
        return "ud07"        # a plain dragon
    if s.get("types", 0) >> UT_CONSTRUCT & 1:
        return "u311"        # a plain construct
    return "u001"            # a plain knight


def build(site, mode, lo, n):
    """dict(frame, pov, local, state, action, pre, attacker): the board when the ability runs and the described state it comes from."""
    s = SITES[site]
    owner = lo if mode in ("place", "attack", "spell", "bot", "survive_own") else 1 - lo    # the caster's
    local = 1 - lo if mode in ("pass", "pass_attack", "death_own") else lo                 # when the ability runs
    pov = owner if s["pov"] in ("me", "order") else local
    frame, reserved = {}, set()
    caster_strength = 0 if mode.startswith("death") else CARD_META[_idx(s["card"])]["strength"]
    if mode not in ("spell", "bot"):
        frame[C] = _ent(s["card"], owner, C, caster_strength)
    if mode in ("death_own", "pass_attack"):   # what it walks into: a structure takes no part in a list of units
        frame[AHEAD] = _ent("b001" if mode == "death_own" else "u003", 1 - owner, AHEAD, 30)
    if mode in ("death_opp", "survive", "survive_opp", "attack"):
        reserved.add(UNDER)
    if mode == "survive_own":   # the striker is placed in a far corner and walks one tile on
        frame[C] = _ent(s["card"], owner, C, caster_strength - 1)
        reserved |= {19, 15}
    if site == "u061":   # its two gained steps: a confused one to a side, one ahead
        reserved |= {C - 1, C + 1, AHEAD, AHEAD - 1, AHEAD + 1}
    attacker = None
    if mode == "death_opp":   # the killer stands under it, struck for 1; 1 against 1 and both are dead
        attacker = _ent("u001", lo, UNDER, 0 if site == "u007" and n == 0 else 4)
    if mode in ("survive", "survive_opp"):   # the striker is alive until its attack is over
        attacker = _ent("u001", lo, UNDER, 1 if mode == "survive_opp" else 5)
    if site == "u018":        # one unit beside it: one type, one round of EACH_U018
        frame[C + 1] = _ent("u001", owner, C + 1, 4)

    side_of = {"friendly": pov, "enemy": 1 - pov, "any": pov}
    if s["sel"] == "front":
        within = model_list(site, {}, pov, local)
        empty = {within[(5 * j) % len(within)] for j in range(n)}   # n tiles stay empty, in different rows (5 is coprime to 12)
        for k, t in enumerate(t for t in within if t not in empty):
            frame[t] = _ent("u001", (lo + k) & 1, t, 3 + k)
    else:
        order = {"sur": ORDER_SUR, "bor": ORDER_BOR, "board": ORDER_BOARD}[s["sel"]]
        free = [t for t in order if t not in frame and t not in reserved]
        want = n - (1 if attacker is not None and _matches(s, attacker, pov) else 0)
        want -= len([x for x in ("friendly", "enemy") if s.get("base") and s["side"] in (x, "any")])   # the bases behind the tiles
        assert len(free) >= want, (site, mode, n)
        for k in range(want):
            t = free.pop(0)
            own = side_of[s["side"]] if s["side"] != "any" else (pov + k) & 1
            if mode == "survive_own":
                own = 1 - owner   # the striker's list of friendly entities is the caster alone
            frame[t] = _ent("b001" if s["kind"] == "any" and k % 3 == 1 else _target_card(s), own, t, 11 + 2 * k)
        # what the list must not hold: a unit of the wrong type or status, of the wrong side, a structure, a match outside the selector
        decoys = []
        if s.get("types") or s.get("xtypes"):
            decoys.append(("ud07" if s.get("xtypes") else "u001", side_of[s["side"]], None))
        if s.get("xstatus"):
            decoys.append(("u001", pov, [0, 0, 1, 0, 0]))
        if s["side"] != "any":
            decoys.append((_target_card(s), 1 - side_of[s["side"]], None))
        if s["kind"] == "unit":
            decoys.append(("b001", side_of[s["side"]], None))
        for k, (cid, own, status) in enumerate(decoys):
            if free and not (mode == "survive_own" and own == owner):   # (the striker's list is the caster alone)
                t = free.pop(0)
                frame[t] = _ent(cid, own, t, 40 + k, status)
        if s["sel"] != "board":
            t = next(t for t in ORDER_OUT if t not in frame and t not in reserved)
            frame[t] = _ent(_target_card(s), 1 - owner if mode == "survive_own" else side_of[s["side"]] if s["side"] != "any" else pov, t, 50)
    if attacker is not None:
        frame[UNDER] = attacker

    # ---- the described state that leads there
    b = E.plain_units()
    tiles = {t: dict(e) for t, e in frame.items()}
    first, mana, action, pre = b[4], 9, (4 - C // 4) * 4 + C % 4, 0
    if mode == "place":
        first = _idx(s["card"])
        del tiles[C]
    elif mode == "survive_own":
        first, action = _idx("u306"), (4 - 19 // 4) * 4 + 19 % 4
        tiles[C]["strength"] += 1
    elif mode == "attack":
        first, action = _idx(s["card"]), (4 - UNDER // 4) * 4 + UNDER % 4
        tiles[C] = _ent("u001", 1 - lo, C, 1)
    elif mode in ("death_opp", "survive", "survive_opp"):
        first, action = _idx("u001"), (4 - UNDER // 4) * 4 + UNDER % 4
        tiles.pop(UNDER, None)
        if mode == "death_opp":
            tiles[C]["strength"] = 1
    elif mode in ("pass", "pass_attack", "death_own"):
        mana, action, pre = 0, 155, 2   # the player that ends its turn draws one card: one random() of two words
        if mode == "death_own":
            tiles[C]["strength"] = 1
        for t, e in tiles.items():
            if e["owner"] == owner and t != C and not _is_struct(e):
                e["status"] = [1, 0, 0, 0, 0]
        tiles = {19 - t: dict(e, position=[(19 - t) % 4, (19 - t) // 4]) for t, e in tiles.items()}
    elif mode == "spell":
        first, action = _idx(s["card"]), 64
    elif mode == "bot":
        first, mana, action = _idx(s["card"]), 3, None
    st = E.state(lo, first, tiles, mana=mana)
    hand = st["players"][lo]["hand"]
    if mode in ("spell", "bot"):
        hand[0]["kind"] = "spell"
    if mode == "bot":
        hand[0]["cost"] = 3        # the one card at the cost of the mana; no card dearer than the mana, so no REPLACE
    if mode == "survive_opp":
        hand[0]["strength"] = 1    # struck for 1: one round
    if mode == "death_opp" and attacker["strength"] <= 0:
        hand[0]["strength"] = 1
    if site == "u017":             # a targeted and an untargeted spell: both are played, in shuffled order (one word)
        for k, cid in ((1, s["spell"]), (2, "s403")):
            hand[k].update(E.card(_idx(cid)), kind="spell", oid=hand[k]["oid"])
        pre = 1
    return dict(frame=frame, pov=pov, local=local, asc=(pov == 0) if s["sel"] == "front" else pov == local, state=st, enc=S.encode_state(st), action=action, pre=pre,
                attacker=attacker is not None, striker_dies=mode in ("survive", "survive_opp"))


def states():
    """[(name, site, mode, lo, n, built)]; name = site-mode-lo-n"""
    if "states" in _cache:
        return _cache["states"]
    out = []
    for site, s in SITES.items():
        for mode in s["modes"]:
            for lo in (0, 1):
                for n in lengths(site, mode):
                    out.append((f"{site}-{mode}-{lo}-n{n}", site, mode, lo, n, build(site, mode, lo, n)))
    _cache["states"] = out
    return out


# ---- the reference ----------------------------------------------------------------------------------------------------------
def stream_words(L, seed, n):
    out = np.zeros(n, dtype=np.uint32)
    L.orc_rng_u32(int(seed), n, out.ctypes.data_as(ctypes.c_void_p))
    return out


def _seed_for(L, k, pre, n):
    """State k's seed: the first of SEED0 + k, + 1000, ... whose stream the model says gives every r within CAP positions.  This
    is wider than one fixed seed per state with the cap alone deciding: a state whose first seed misses an r (a list of 8 or 9 has
    about one chance in 200 of that) takes the next one instead of failing, and fails only if twenty seeds miss; 2 of the 304
    states are on their second seed.  The choice is made from the stream's words by the model, before the oracle or the device
    has run; reference() then walks that one seed on the oracle and fails if an r is missing at the cap."""
    for seed in range(SEED0 + k, SEED0 + k + 20000, 1000):
        words = stream_words(L, seed, POS0 + CAP + 64)
        if len({model_draw(words, pos + pre, n)[0] for pos in range(POS0, POS0 + CAP)}) == max(n, 1):
            return seed, words
    raise AssertionError((k, n))


def _cursor(canon, words, start):
    """Where the game's stream stands: the canonical record ends in the stream's next word."""
    nxt = int(np.frombuffer(canon[-4:], dtype=np.uint32)[0])
    return next(p for p in range(start, len(words)) if int(words[p]) == nxt)


def _changed(site, bt, frame, before_bases, after_bases, after, lst):
    """The elements of the list that the step changed, each with by how much its strength moved; a unit among them also with
    the status the site's effect sets (STATUS), which must have gone up by one."""
    out = {}
    for el in lst:
        if isinstance(el, tuple):
            d = after_bases[el[1]] - before_bases[el[1]]
            if d:
                out[el] = d
            continue
        if SITES[site]["sel"] == "front":
            e = after.get(el)
            if e is not None and e["card"] == TOKEN_KNIGHT and e["strength"] == 5:
                out[el] = 5
            continue
        was = frame[el]
        e = after.get(el)
        if bt["attacker"] and el == UNDER and bt["striker_dies"]:
            continue
        if bt["attacker"] and el == UNDER:   # the killer has moved onto C; it was struck for 1 before the ability ran
            e = after.get(C)
            assert e is not None and e["owner"] == was["owner"], (site, after)
        if e is None or e["card"] != was["card"] or e["owner"] != was["owner"]:
            out[el] = -was["strength"]
        elif e["strength"] != was["strength"] or e["status"][1:] != was["status"][1:]:
            out[el] = e["strength"] - was["strength"]
            if site in STATUS:
                assert e["status"][STATUS[site]] == was["status"][STATUS[site]] + 1, (site, el, e)
    return out


EFFECT = {"u007": 5, "u021": 5, "u061": 0, "u076": -6, "u111": 1, "u305": 4, "u306": -1, "u313": 5, "u320": 4, "ud01": 7, "ud31": 2,
          "s012": 5, "u018": -2, "ue01": -1, "u017": -9}
STATUS = {"u007": 4, "u061": ST_CONFUSED}   # u007 vitalizes what it heals (ST_VITALIZED = 4), u061 confuses and heals nothing
POST = {"u061": 1}   # words the step draws behind the pick: the first of u061's two steps is a confused one, to the left or the right


def reference(core="oracle"):
    """dict(cases, ...): cases = [dict(name, site, mode, lo, n, r, asc, enc, seed, pos, action, fault, hash, decision)], one per kept
    (state, stream position); on the recursive oracle (core="oracle") every case is asserted to be what it is named after, and the
    kept positions are found.  core="product": the same cases -- the oracle's positions -- on the host build of the product core."""
    if core in _cache:
        return _cache[core]
    orc = oracle_lib.Oracle(1, core=core) if core != "oracle" else oracle_lib.Oracle(1)
    if core != "oracle":
        cases = [dict(c) for c in reference()["cases"]]
        for c in cases:
            c.update(_play(orc, c["enc"], c["seed"], c["pos"], c["action"], c["mode"] == "bot"))
        _cache[core] = dict(cases=cases)
        return _cache[core]
    cases = []
    for k, (name, site, mode, lo, n, bt) in enumerate(states()):
        s = SITES[site]
        seed, words = _seed_for(orc.L, k, bt["pre"], n)
        lst = model_list(site, bt["frame"], bt["pov"], bt["local"])
        assert len(lst) == n, (name, lst)
        assert bt["asc"] == ORDERS.get(mode, True) or site == "s012", name
        if site == "s012":
            assert bt["asc"] == (lo == 0)
        draws = s.get("draws", 1)
        found = {}
        for pos in range(POS0, POS0 + CAP):
            assert orc.scn_build(0, seed, pos, bt["enc"]) == 0, name
            c0 = orc.canon(0)
            _, bases0, _, before = ET.parse(c0)
            assert _cursor(c0, words, 0) == pos, name
            # the model: which elements, and where the stream stands afterwards
            cur, rs = pos + bt["pre"], []
            for _ in range(draws if n > 0 else 0):
                r, cur = model_draw(words, cur, n)
                rs.append(r)
            cur += POST.get(site, 0)
            if mode == "bot":
                a, f = orc.expert_action(0)
                t = lst[rs[0]]
                assert (a, f) == (65 + (4 - t // 4) * 4 + t % 4, 0), (name, pos, a, f, t)
                assert _cursor(orc.canon(0), words, 0) == cur, name
            else:
                a = bt["action"]
                assert a in orc.legal_actions(0), (name, a, orc.legal_actions(0))
                f = orc.step(0, a)[0]
                c1 = orc.canon(0)
                _, bases1, _, after = ET.parse(c1)
                if n == 0 and s.get("empty") == "raise":
                    assert f == FAULT_PY_EXCEPTION, (name, f)
                else:
                    assert f == 0, (name, f)
                    got = _changed(site, bt, bt["frame"], bases0, bases1, after, lst)
                    want = {}
                    for r in rs:
                        want[lst[r]] = want.get(lst[r], 0) + EFFECT[site]
                    if mode in ("survive", "survive_opp"):   # the striker dies of its own attack: a draw that lands on it shows in the cursor alone
                        want.pop(UNDER, None)
                    want = {el: max(d, -bt["frame"][el]["strength"]) if not isinstance(el, tuple) and s["sel"] != "front" else d for el, d in want.items()}
                    assert got == want, (name, pos, got, want, lst)
                    assert _cursor(c1, words, pos) == cur, (name, pos, _cursor(c1, words, pos), cur)
            r = rs[0] if rs else None
            if r not in found:
                found[r] = pos
            if len(found) == max(n, 1):
                break
        assert sorted(found, key=lambda x: -1 if x is None else x) == (list(range(n)) if n else [None]), (name, "stream positions walked without every r", found)
        for r, pos in sorted(found.items(), key=lambda x: x[1]):
            case = dict(name=f"{name}-r{r}", site=site, mode=mode, lo=lo, n=n, r=r, asc=bt["asc"], enc=bt["enc"], seed=seed, pos=pos,
                        action=bt["action"], element=lst[r] if r is not None else None)
            case.update(_play(orc, bt["enc"], seed, pos, bt["action"], mode == "bot"))
            cases.append(case)
    _cache[core] = dict(cases=cases)
    return _cache[core]


def _play(orc, enc, seed, pos, action, bot):
    """What both sides of every comparison are made of: the step's fault and hash, and the decision from the same state."""
    assert orc.scn_build(0, seed, pos, enc) == 0
    out = {}
    if bot:
        action, out["bot_fault"] = orc.expert_action(0)
        out["bot_action"] = action
    f = orc.step(0, action)[0]
    out.update(fault=f, hash=orc.canon_hash(0))
    if bot:   # ... and the same action from the state the bot has not touched (the vector env steps it so)
        assert orc.scn_build(0, seed, pos, enc) == 0
        f = orc.step(0, action)[0]
        out.update(plain_fault=f, plain_hash=orc.canon_hash(0))
    assert orc.scn_build(0, seed, pos, enc) == 0
    a, scores, _ = orc.decide(0, W0 if orc.to_play(0) == 0 else W1)
    f = orc.step(0, a)[0]
    out["decision"] = dict(action=a, scores=scores, fault=f, hash=orc.canon_hash(0))
    return out


def replay(extended):
    """[(fault, hash)] of every kept case's step on the recursive oracle of another record build (True the extended record, 2 the
    large one): what a handle of that build is held to.  The bot cases step the bot's action from the state the bot has not touched;
    extended=False: the standard record, from the reference itself."""
    key = ("replay", extended)
    if extended is False:
        return [(c["plain_fault"], c["plain_hash"]) if c["mode"] == "bot" else (c["fault"], c["hash"]) for c in reference()["cases"]]
    if key not in _cache:
        orc = oracle_lib.Oracle(1, extended=extended)
        out = []
        for c in reference()["cases"]:
            assert orc.scn_build(0, c["seed"], c["pos"], c["enc"]) == 0, c["name"]
            f = orc.step(0, c["bot_action"] if c["mode"] == "bot" else c["action"])[0]
            out.append((f, orc.canon_hash(0)))
        _cache[key] = out
    return _cache[key]


def check_coverage(ref=None):
    """All sixteen sites; every r of every listed n in every order the table declares reachable, for both local orders; every
    (site, order) pair either covered or declared unreachable; and in every state of a site with n >= 2, two kept
    positions whose triggering action the oracle's decision scores differently (the score row of the hot kernel then sees the
    pick), but for the sites of SCORE_BLIND and SCORE_PARTLY, which say why."""
    cases = (ref or reference())["cases"]
    assert len(SITES) == 16
    have = {(c["site"], c["mode"], c["lo"], c["n"], c["r"]) for c in cases}
    for site, s in SITES.items():
        orders = set()
        for mode in s["modes"]:
            for lo in (0, 1):
                for n in lengths(site, mode):
                    for r in (range(n) if n else [None]):
                        assert (site, mode, lo, n, r) in have, (site, mode, lo, n, r)
                orders |= {c["asc"] for c in cases if c["site"] == site and c["mode"] == mode and c["lo"] == lo}
        for asc in (True, False):
            assert (asc in orders) != ((site, asc) in UNREACHABLE), (site, asc, orders)
        # the oracle's score of the triggering action, compared between the kept positions of ONE state (two states score
        # differently whatever is drawn)
        seen = {}
        for c in cases:
            if c["site"] == site and c["n"] > 1 and c["mode"] != "bot":
                seen.setdefault((c["mode"], c["lo"], c["n"]), set()).add(np.float64(c["decision"]["scores"][c["action"]]).view(np.uint64).item())
        sees = {k for k, bits in seen.items() if len(bits) >= 2}
        if site in SCORE_BLIND:
            assert not sees, (site, "is declared blind, yet the score of its triggering action sees the pick in", sorted(sees))
        elif site in SCORE_PARTLY:
            assert {k[:2] for k in sees} == {k[:2] for k in seen}, (site, sorted(set(seen) - sees))
        else:
            assert sees == set(seen) and seen, (site, "the score of the triggering action does not see the pick in", sorted(set(seen) - sees))
    return len(cases)


def counts():
    """{site: (states, kept (state, position) pairs)}"""
    cases = reference()["cases"]
    return {site: (sum(1 for x in states() if x[1] == site), sum(1 for c in cases if c["site"] == site)) for site in SITES}
