"""What the wave-cooperative features of the hot kernel (monsoon_amd/csrc/coop_features.h) newly make fragile, on every
hot-kernel instantiation of variants.def (run with -m gpu on an MI355X).

The kernel deals the 20 tiles to the sub-lanes of a candidate, carries the two ordered f64 sums from sub-lane to sub-lane
and divides the six independent quotients side by side, so the states here fill every sub-lane's tile run (a full board,
with and without strengths of -1), leave all of them empty, and give the hand 0, 1, 2, 3 (the one size that divides by
three) and 4 cards.  tests/test_heuristic_model_gpu.py already has a full board, an empty board and the three-card hand,
but decides them on the default variant of the standard and the extended build only; its per-variant test uses
random-policy states.  Here every (U, W) of every build decides every state: all scores, the action and the best score
are compared bit for bit with the independent float64 model, the serial monsoon_features kernel is compared with the same
model on the same states, and the legal sets must include ragged last passes (n_legal % U != 0)."""
import copy
import json

import numpy as np
import pytest

import heuristic_model as HM
import kernel_variants
import test_heuristic_model_gpu as T
from monsoon_amd.cards import CARD_INDEX

pytestmark = pytest.mark.gpu

VARIANTS, VARIANT_IDS = kernel_variants.matrix()


def _states():
    """Scenario states (tests/golden/scenarios.json.gz) with the board and the mover's hand rebuilt."""
    import scenario_lib as S
    ext_cards = [CARD_INDEX["ua20"], CARD_INDEX["b005"]]
    recs = [r for case in S.load() for r in case["records"]
            if not any(f'"card": {c},' in s or f'"card": {c}}}' in s for s in [json.dumps(r)] for c in ext_cards)
            and r["before"]["phase"] == 1 and not r["before"]["resolving"] and not r["before"]["triggers"]]
    bases = recs[::max(1, len(recs) // 6)][:6]
    unit = next(t for r in recs for t in r["before"]["tiles"] if t and t["kind"] == "unit" and not t.get("memory"))
    struct = next(t for r in recs for t in r["before"]["tiles"] if t and t["kind"] == "structure" and not t.get("memory"))

    def put(st, t, tmpl, owner, strength):
        e = copy.deepcopy(tmpl)
        e["owner"], e["position"], e["path"], e["strength"] = owner, [t % 4, t // 4], [], strength
        st["tiles"][t] = e

    def board(pattern):
        """pattern(t) -> None or (is_unit, owner, strength) for tile t."""
        def f(st):
            st["tiles"] = [None] * 20
            for t in range(20):
                p = pattern(t)
                if p:
                    put(st, t, unit if p[0] else struct, p[1], p[2])
        return f

    def hand(k):
        def f(st):
            for p in st["players"]:
                cards = p["hand"] + p["deck"]
                p["hand"], p["deck"] = cards[:k], cards[k:]
        return f

    muts = [
        # 20 entities: every sub-lane's run is full and both ordered sums have terms on every row
        ("full_units", board(lambda t: (True, (t + t // 4) % 2, 1 + (t * 7) % 5))),
        ("full_mixed", board(lambda t: (t % 3 != 0, t % 2, 2 + (t * 3) % 7))),
        ("full_mine", board(lambda t: (t % 5 != 0, 0, 3 + t % 4))),
        ("full_theirs", board(lambda t: (t % 5 != 0, 1, 3 + t % 4))),
        # strengths of -1 are skipped by every sum but still count as entities
        ("full_minus1", board(lambda t: (t % 4 != 1, t % 2, -1 if t % 3 == 0 else 4))),
        ("all_minus1", board(lambda t: (True, t % 2, -1))),
        ("one_minus1", board(lambda t: (True, t // 7 % 2, -1 if t == 7 else 2) if t in (3, 7, 12, 19) else None)),
        ("empty_board", board(lambda t: None)),
        # one entity at each end of the tile order: the first and the last sub-lane's run alone
        ("tile0", board(lambda t: (True, 1, 3) if t == 0 else None)),
        ("tile19", board(lambda t: (True, 0, 3) if t == 19 else None)),
        ("row_ends", board(lambda t: (True, t % 2, 5) if t % 4 in (0, 3) else None)),
    ] + [(f"hand{k}", hand(k)) for k in range(5)]
    out = []
    for r in bases:
        for name, f in muts:
            st = copy.deepcopy(r["before"])
            f(st)
            for p in st["players"]:
                for k, c in enumerate(p["hand"] + p["deck"]):
                    c["oid"] = k
            out.append((name, st))
        st = copy.deepcopy(r["before"])   # three cards over a full board: the longest sums and the division by three at once
        muts[1][1](st)
        hand(3)(st)
        for p in st["players"]:
            for k, c in enumerate(p["hand"] + p["deck"]):
                c["oid"] = k
        out.append(("full_hand3", st))
    return out


@pytest.mark.parametrize("ext,u,w", VARIANTS, ids=VARIANT_IDS)
def test_cooperative_features_on_edge_boards_and_hands(monkeypatch, ext, u, w):
    """Full boards (20 entities, with strengths of -1), empty and single-tile boards, hands of 0 to 4 cards, decided by
    variant (U, W) under the 19 weight vectors of the model tests (the one-hot ones expose each feature alone): every
    score, the action and the best score equal the independent model bit for bit; monsoon_features (the serial form)
    equals the model on the same states; some decision has a ragged last pass and, where U <= 8, several passes."""
    import scenario_lib as S
    from monsoon_amd._lib import MonsoonError
    from monsoon_amd.engine import BatchEngine
    kernel_variants.select(monkeypatch, u, w)
    states = _states()
    probe = BatchEngine(1, extended=ext)   # a state the record cannot hold never reaches the handle under test
    assert probe.variant() == (u, w)
    good = []
    for name, st in states:
        try:
            if probe.debug_build(0, st["seed"], st["stream_pos"], S.encode_state(st)) == 0:
                good.append((name, st))
        except MonsoonError:
            pass
    probe.close()
    names = {name for name, _ in good}
    assert len(names) == 17 and len(good) >= len(states) * 3 // 4, (len(good), len(states), sorted(names))
    eng = BatchEngine(len(good), extended=ext)
    for name, st in good:
        assert eng.debug_build(eng.n, st["seed"], st["stream_pos"], S.encode_state(st)) == 0, name
    obs, raises = eng.observe()
    feat = eng.features()
    ok = ~raises.astype(bool)
    assert np.isnan(feat[~ok]).all()
    assert np.array_equal(T._bits(HM.features(obs[ok])), T._bits(feat[ok]))
    n_legal = T._legal_bits(eng.legal_mask()).sum(axis=1)
    assert (n_legal % u != 0).any(), n_legal.tolist()
    if u <= 8:
        assert (n_legal > u).any(), n_legal.tolist()
    tally = dict(games=0, scores=0, limit=0, raising=0, zero_successors=0, over=0)
    T._check_decisions(eng, range(eng.n), T._weight_set(), ext, tally, HM.ScoreCache())
    eng.close()
    print(f"variant {T.NAMES[ext]} ({u}, {w}): {len(good)} of {len(states)} states built ({len(names)} kinds), "
          f"{tally['scores']} candidate scores of {tally['games']} decisions equal the model ({tally['over']} states with "
          f"a winner not decided, {tally['raising']} whose observation raises, {tally['limit']} skipped at a build limit); "
          f"legal actions per state {int(n_legal.min())}..{int(n_legal.max())}")
    assert tally["games"] >= len(good) // 2
