"""The serial weighted draw of the product's rules core (monsoon_amd/csrc/rules.h draw(): the search decides
fl(acc / last) <= u without the division outside a band of a few ulps) against the recursive oracle, on the CPU: the host
build of the product core (oracle_lib core="product") and the oracle play the same table of weights and samples and a few
thousand games on per-game decks of the 109 observable cards, and every row must be equal.

The table: a mover with four cards in hand replaces one (actions 148 / 149) with decks of 0..12 cards whose ages are all 0,
all 1, mixed, dominated by one card at AGE_MAX - 1, or hold a card at AGE_MAX (a limit of the record: both sides report
it), with and without a single-use card under the replaced position, each at 48 consecutive stream positions (48 samples
u).  Samples planted exactly on a cdf boundary need a stream the host entry points cannot be given; those run on the GPU
(tests/test_cycle_draw_gpu.py), where the serial draw is also checked against numpy's definition computed in the test."""
import copy

import numpy as np

import oracle_lib
import scenario_lib as S
from monsoon_amd.cards import CARD_INDEX, supported_pool

AGE_MAX, DECK_CAP = 255, 12
W0 = np.random.RandomState(2024).uniform(0, 1, 10)


def _cards_and_template():
    """Card descriptions as the scenario fixtures hold them (fresh cards of the standard record), and a state to fill."""
    ext = {CARD_INDEX[c] for c in set(supported_pool(True, True)) - set(supported_pool(True, False))}
    cards, template = {}, None
    for case in S.load():
        for rec in case["records"]:
            st = rec["before"]
            if template is None and not st["resolving"] and not st.get("triggers"):
                template = st
            for p in st["players"]:
                for c in p["hand"] + p["deck"]:
                    if c["card"] not in ext and c.get("position") is None and not c["single_use"]:
                        cards.setdefault((c["card"], c["cost"], c.get("strength")), c)
    out = [cards[k] for k in sorted(cards, key=str)]
    assert len(out) >= 4 and template is not None
    return [out[i % len(out)] for i in range(4 + DECK_CAP)], template   # (equal cards may repeat: list.remove takes the first)


def _state(cards, template, n, ages, single):
    st = copy.deepcopy(template)
    st.update(local_order=0, cp=0, history=[], resolving=False)
    st["tiles"] = [None] * len(st["tiles"])
    for o, p in enumerate(st["players"]):
        p.update(mana=0, replacable=True, leftmost_movable=True)
        pick = [copy.deepcopy(c) for c in cards[:4 + n]]
        for i, c in enumerate(pick):
            c.update(oid=i, age=0, single_use=False)
        p["hand"], p["deck"] = pick[:4], pick[4:]
        if o == 0:
            for c, a in zip(p["deck"], ages):
                c["age"] = int(a)
            for h in single:
                p["hand"][h]["single_use"] = True
    return S.encode_state(st)


def test_weight_and_sample_table_equals_the_recursive_oracle():
    cards, template = _cards_and_template()
    rs = np.random.RandomState(5)
    orc, prod = oracle_lib.Oracle(1), oracle_lib.Oracle(1, core="product")
    rows = plain = 0
    for n in range(DECK_CAP + 1):
        patterns = {"zeros": [0] * n, "ones": [1] * n, "mixed": list(rs.randint(0, 60, n)),
                    "dominant": [int(a) for a in rs.randint(0, 8, n)], "fault": list(rs.randint(0, 60, n))}
        if n:
            patterns["dominant"][int(rs.randint(0, n))] = AGE_MAX - 1
            patterns["fault"][int(rs.randint(0, n))] = AGE_MAX
        for name, ages in patterns.items():
            for single in ((), (1,)):
                enc = _state(cards, template, n, ages, single)
                for pos in range(48):
                    for a in (148, 149):
                        got = []
                        for o in (orc, prod):
                            assert o.scn_build(0, 7000 + n, pos, enc) == 0, (n, name)
                            assert a in o.legal_actions(0), (n, name)
                            f, r, d = o.step(0, a)
                            got.append((f, r, d, o.canon(0)))
                        assert got[0] == got[1], (n, name, single, pos, a, got[0][0], got[1][0])
                        rows += 1
                        plain += got[0][0] == 0
    assert rows == (DECK_CAP + 1) * 5 * 2 * 48 * 2 and plain > rows // 2   # most rows are plain successful draws


def test_random109_games_equal_the_recursive_oracle():
    """Rollouts on per-game decks drawn from the 109 observable cards, extended record (the serial draw indexes weights by
    object id there): results, step counts and final hashes of the product core equal the oracle's."""
    pool = np.array([CARD_INDEX[c] for c in supported_pool(extended=True)], dtype=np.uint8)
    n = 3072
    orc, prod = oracle_lib.Oracle(n, extended=True), oracle_lib.Oracle(n, extended=True, core="product")
    for g in range(n):
        rs = np.random.RandomState(g ^ 0x9E3779B9)
        d0, d1 = rs.choice(pool, 12, replace=False), rs.choice(pool, 12, replace=False)
        for o in (orc, prod):
            assert o.reset(g, 9000 + g, d0, d1) == 0
    a = orc.rollout_batch(n, W0, 40, 16)
    b = prod.rollout_batch(n, W0, 40, 16)
    assert a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)
    assert [orc.game_fault(g) for g in range(n)] == [prod.game_fault(g) for g in range(n)]
