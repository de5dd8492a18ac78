"""The short ability effects on whole words (monsoon_amd/csrc/rules.h: random.choice asked of the hit mask, choice_tile /
targets_pick / shape_pick / empty_front_pick; the status methods on the entity image; gain_speed through set_path_known; state.h
MSB_WIDE_AB_*) inside whole games on the device: every standard variant of the hot kernel plays the 64 N12M games and the 64
games on the deck of the touched cards (tests/wide_ab_states.py) for 40 decisions, and every decision must stay on the
recursive oracle's line (run with -m gpu on an MI355X).

The CPU side first makes sure that each of the 12 touched abilities (u007 u021 u061 u053 u051 u050 ua07 ud01 u055 s007 s012
ue01) runs at least once in the committed steps of those games.  What the games do not reach is stepped from described
states: a status at 255, a poisoned unit that is vitalized, u061 with no other friendly unit (no draw), a pick whose draw lands
on a base, gain_speed from the back row, of a unit with nothing around it and of a confused unit.  Each is asserted on the
oracle to be what it is named after; then monsoon_step of the device must give the oracle's fault code and canonical hash for
every (state, action).

Which element a pick draws, at every list length and under both list orders, and the call sites these games do not reach
(u076 u111 u305 u306 u313 u320 ud31, EACH_U017, the scripted bot's spell target): tests/test_pick_sites_gpu.py over the case
table of tests/pick_sites.py."""
import numpy as np
import pytest

import kernel_variants
import wide_ab_states as W

STANDARD = [(False, u, w) for u, w in kernel_variants.variants(False)]
IDS = [f"{kernel_variants.BUILD_NAMES[e]}-{u}x{w}" for e, u, w in STANDARD]


def test_the_games_reach_every_touched_ability():
    """CPU: the fixture cannot silently lose a card (the GPU test asserts the same before it plays)."""
    W.check_reached()
    print(W.reached())


def test_the_described_states_are_what_they_are_named_after():
    """CPU: reference() asserts every case on the recursive oracle; the host build of the product core steps the same way."""
    ref, prod = W.reference(), W.reference("product")
    clean = lambda rows: [(k, a, f, 0 if f else h) for k, a, f, h in rows]   # (a step that faults leaves no state to compare)
    assert clean(ref["rows"]) == clean(prod["rows"]) and ref["pos"] == prod["pos"]
    assert sum(f == W.FAULT_STATUS_SAT for _, _, f, _ in ref["rows"]) == 2


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _engine(t):
    from monsoon_amd.engine import BatchEngine
    eng = BatchEngine(t["decks"].shape[0])
    eng.reset(np.array(t["seeds"], dtype=np.uint32), t["decks"][0])
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("deck", ["N12M", "touched"])
@pytest.mark.parametrize("ext,u,w", STANDARD, ids=IDS)
def test_every_decision_stays_on_the_oracle_line(monkeypatch, ext, u, w, deck):
    """Decision rounds with scores written: after every round the chosen action, the whole score row (NaN exactly at the
    actions that are not legal, bit patterns elsewhere), the best score and the state hash equal the oracle's.  Then the same
    games through play_rounds, 8 decisions per launch: the state hash after each launch equals the same line."""
    W.check_reached()
    kernel_variants.select(monkeypatch, u, w)
    t = W.trace(deck)
    decisions, n = t["action"].shape
    weights = np.broadcast_to(np.stack([W.W0, W.W1]), (n, 2, 10)).copy()
    eng = _engine(t)
    assert eng.variant() == (u, w)
    for r in range(decisions):
        action, best, scores = eng.decide(weights, want_scores=True)
        hashes = eng.state_hash()
        live, clean = t["live"][r], t["clean"][r]
        assert np.array_equal(action[live], t["action"][r][live]), (r, np.nonzero(action != t["action"][r])[0][:8])
        nan = np.isnan(t["scores"][r])
        assert np.array_equal(np.isnan(scores)[live], nan[live]), r
        assert np.array_equal(_bits(scores)[~nan], _bits(t["scores"][r])[~nan]), r
        assert np.array_equal(_bits(best)[live], _bits(t["best"][r])[live]) and np.isnan(best[~live]).all(), r
        assert np.array_equal(hashes[clean], t["hash"][r][clean]), (r, np.nonzero(hashes != t["hash"][r])[0][:8])
    eng.close()

    eng = _engine(t)
    eng.upload_weights(np.stack([W.W0, W.W1]))
    eng.assign_players(np.zeros(n, dtype=np.int32), np.ones(n, dtype=np.int32))
    for k in range(decisions // 8):
        eng.play_rounds(8)
        eng.sync()
        r = 8 * k + 7
        clean = t["clean"][r]
        assert np.array_equal(eng.state_hash()[clean], t["hash"][r][clean]), ("play_rounds", k)
    eng.close()


@pytest.mark.gpu
def test_described_states_step_as_the_oracle():
    """monsoon_step of every (state, action): the fault code is the oracle's, and where the step is clean the canonical hash."""
    from monsoon_amd.engine import BatchEngine
    ref = W.reference()
    K = len(ref["names"])
    eng = BatchEngine(K)
    for k in range(K):
        assert eng.debug_build(k, ref["seeds"][k], ref["pos"][k], ref["enc"][k]) == 0, ref["names"][k]
    assert [r[0] for r in ref["rows"]] == list(range(K))   # one action per state
    actions = np.array([r[1] for r in ref["rows"]], dtype=np.uint8)
    _, _, fault = eng.step(actions)
    hashes = eng.state_hash()
    for k, a, f, h in ref["rows"]:
        assert int(fault[k]) == f, (ref["names"][k], a, int(fault[k]), f)
        if not f:
            assert int(hashes[k]) == h, (ref["names"][k], a)
    eng.close()
