"""The hand, deck and path bookkeeping of a step on whole words (monsoon_amd/csrc/rules.h discard_wide, draw_take_wide, the hand
entry read once per play, set_path_impl) inside whole games on the device: every standard variant of the hot kernel plays
the 64 N12M games of tests/wide_lists_trace.py for 40 decisions, the default variants of the extended and large builds play
its 16 random-deck games for 20 (set_path is the part they share), and every decision must stay on the recursive oracle's
line (run with -m gpu on an MI355X).

The CPU side first makes sure that the N12M games give the new forms what games can give: a removal at each hand index an
action can name (0..3), a REPLACE that draws the deck's first entry, a path that turns to the side.  What 64 games do not
reach is stepped from described states (tests/wide_lists_states.py, built by monsoon_debug_build and by the oracle's
scn_build from one description): an age of 254 and of AGE_MAX in each of the three age words under a play and a REPLACE,
a five-card hand, an earlier equal card in the hand and in the deck, plain and positioned, two equal spells, a play into
a deck of eleven and of twelve, a REPLACE that draws the deck's first and its last entry.  Each is asserted on the oracle
to be what it is named after, then monsoon_step of the device must give the oracle's fault code and canonical hash for
every (state, action), and one decision of every standard variant of the hot kernel from every state the oracle's
scores, action and successor."""
import numpy as np
import pytest

import kernel_variants
import wide_lists_states as W
import wide_lists_trace as T

STANDARD = [(False, u, w) for u, w in kernel_variants.variants(False)]
OTHERS = [(ext,) + kernel_variants.variants(ext)[0] for ext in (True, 2)]
CASES = STANDARD + OTHERS
IDS = [f"{kernel_variants.BUILD_NAMES[e]}-{u}x{w}" for e, u, w in CASES]


def test_the_games_reach_the_whole_word_forms():
    """CPU: the fixture cannot silently lose a case (the GPU test asserts the same before it plays)."""
    T.check_reached()
    for ext in (True, 2):
        r = T.trace(ext)["reached"]
        assert r["sidestep"] > 0 and sum(r["remove"]) > 0, r


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _engine(ext, t):
    from monsoon_amd.engine import BatchEngine
    n = t["decks"].shape[0]
    eng = BatchEngine(n, extended=ext)
    eng.reset(np.array(t["seeds"], dtype=np.uint32), t["decks"] if ext else t["decks"][0])
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("ext,u,w", CASES, ids=IDS)
def test_every_decision_stays_on_the_oracle_line(monkeypatch, ext, u, w):
    """Decision rounds with scores written: after every round the chosen action, the whole score row (NaN exactly at the
    actions that are not legal, bit patterns elsewhere), the best score and the state hash equal the oracle's.  Then the same
    games through play_rounds, 8 decisions (4 on the other builds) per launch: the state hash after each launch equals the
    same line."""
    T.check_reached()
    kernel_variants.select(monkeypatch, u, w)
    t = T.trace(ext)
    decisions, n = t["action"].shape
    weights = np.broadcast_to(np.stack([T.W0, T.W1]), (n, 2, 10)).copy()
    eng = _engine(ext, t)
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
    assert eng.stats()["lookahead_steps"] == int(T.legal_counts(t).sum())
    eng.close()

    eng = _engine(ext, t)
    eng.upload_weights(np.stack([T.W0, T.W1]))
    eng.assign_players(np.zeros(n, dtype=np.int32), np.ones(n, dtype=np.int32))
    per = 4 if ext else 8
    for k in range(decisions // per):
        eng.play_rounds(per)
        eng.sync()
        r = per * k + per - 1
        clean = t["clean"][r]
        assert np.array_equal(eng.state_hash()[clean], t["hash"][r][clean]), ("play_rounds", k)
    assert eng.stats()["lookahead_steps"] == int(T.legal_counts(t).sum())
    eng.close()


# ---- described states: what the games do not reach (tests/wide_lists_states.py) ------------------------------------


def test_the_described_states_are_what_they_are_named_after():
    """CPU: reference() asserts every case on the recursive oracle; the host build of the product core steps the same way."""
    ref, prod = W.reference(), W.reference("product")
    assert ref["rows"] == prod["rows"] and ref["pos"] == prod["pos"]
    assert [(d["action"], d["fault"], d["hash"]) for d in ref["decisions"]] == [(d["action"], d["fault"], d["hash"]) for d in prod["decisions"]]


@pytest.fixture(scope="module")
def described():
    """The oracle's side once for all tests, and the blobs of the states as monsoon_debug_build makes them."""
    from monsoon_amd.engine import BatchEngine
    ref = W.reference()
    K = len(ref["names"])
    build = BatchEngine(K)
    for k in range(K):
        assert build.debug_build(k, ref["seeds"][k], ref["pos"][k], ref["enc"][k]) == 0, ref["names"][k]
    blobs = [build.save_state(k) for k in range(K)]
    build.close()
    return ref, blobs


@pytest.mark.gpu
def test_described_states_step_as_the_oracle(described):
    """monsoon_step of every (state, action): the fault code is the oracle's, and where the step is clean the canonical hash."""
    from monsoon_amd.engine import BatchEngine
    ref, blobs = described
    K = len(blobs)
    per_state = [[r for r in ref["rows"] if r[0] == k] for k in range(K)]
    compared = 0
    for rnd in range(max(len(p) for p in per_state)):
        eng = BatchEngine(K)
        for k, bl in enumerate(blobs):
            eng.load_state(k, bl)
        actions = np.array([p[rnd][1] if rnd < len(p) else 255 for p in per_state], dtype=np.uint8)
        _, _, fault = eng.step(actions)
        hashes = eng.state_hash()
        for k, p in enumerate(per_state):
            if rnd < len(p):
                _, a, f, h = p[rnd]
                assert int(fault[k]) == f, (ref["names"][k], a, int(fault[k]), f)
                if not f:
                    assert int(hashes[k]) == h, (ref["names"][k], a)
                compared += 1
        eng.close()
    assert compared == len(ref["rows"])


@pytest.mark.gpu
@pytest.mark.parametrize("ext,u,w", STANDARD, ids=IDS[:len(STANDARD)])
def test_described_states_decide_as_the_oracle(monkeypatch, described, ext, u, w):
    """One decision of the hot kernel from every described state: every legal action's look-ahead runs the whole-word forms
    on the candidate columns; the scores, the action and the committed successor are the oracle's."""
    from monsoon_amd.engine import BatchEngine
    ref, blobs = described
    kernel_variants.select(monkeypatch, u, w)
    eng = BatchEngine(len(blobs))
    assert eng.variant() == (u, w)
    for k, bl in enumerate(blobs):
        eng.load_state(k, bl)
    action, _, scores = eng.decide(W.W0, want_scores=True)
    hashes, faults = eng.state_hash(), eng.game_faults()
    for k, d in enumerate(ref["decisions"]):
        name = ref["names"][k]
        nan = np.isnan(d["scores"])
        assert np.array_equal(np.isnan(scores[k]), nan), name
        assert np.array_equal(_bits(scores[k])[~nan], _bits(d["scores"])[~nan]), name
        assert int(action[k]) == d["action"], (name, int(action[k]), d["action"])
        # monsoon_game_faults: the fault that stopped the game, else the first limit of the record a look-ahead hit
        assert faults[k] == d["fault"] or (not d["fault"] and faults[k] >= 16), (name, int(faults[k]), d["fault"])
        if not d["fault"]:
            assert int(hashes[k]) == d["hash"], name
    eng.close()
