"""The entity image of move, damage, destroy and Unit.play (monsoon_amd/csrc/rules.h h_move, call_entity_damage, call_destroy,
call_unit_play on ei_load / ei_*; state.h MSB_WIDE_ENT) inside whole games on the device: every standard variant of the hot
kernel plays the 64 N12M games of tests/wide_ent_trace.py for 40 decisions, the default variants of the extended and large
builds (which keep the per-field text) play its 16 random-deck games for 20, and every decision must stay on the recursive
oracle's line (run with -m gpu on an MI355X).

The CPU side first makes sure that the N12M games give the handlers what games can give: a quiet move of one tile; a fight
that kills the target, the mover and both; a base hit; a frozen unit thawing at a turn's start; a poisoned and a vitalized
mover.  What 64 games do not reach is stepped from described states (tests/wide_ent_states.py, built by monsoon_debug_build
and by the oracle's scn_build from one description): a quiet move of two tiles, movers with a BEFORE_ATTACKING and an
AFTER_ATTACKING ability, played and moved, disabled and not, confused movers in an edge and an inner column, and the recorded
boards on which one play runs into the depth guard (FAULT_DEPTH).  Each is asserted on the oracle to be what it is named after, then monsoon_step of the device must give the
oracle's fault code and canonical hash for every (state, action), and one decision of every standard variant of the hot
kernel from every state the oracle's scores, action and successor."""
import numpy as np
import pytest

import kernel_variants
import wide_ent_states as W
import wide_ent_trace as T

STANDARD = [(False, u, w) for u, w in kernel_variants.variants(False)]
OTHERS = [(ext,) + kernel_variants.variants(ext)[0] for ext in (True, 2)]
CASES = STANDARD + OTHERS
IDS = [f"{kernel_variants.BUILD_NAMES[e]}-{u}x{w}" for e, u, w in CASES]


def test_the_games_reach_the_handlers():
    """CPU: the fixture cannot silently lose a case (the GPU test asserts the same before it plays)."""
    T.check_reached()
    for ext in (True, 2):
        r = T.reached(ext)
        assert r["poisoned"] > 0 and r["base_hit"] > 0, r


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


# ---- described states: what the games do not reach (tests/wide_ent_states.py) ------------------------------------


def test_the_described_states_are_what_they_are_named_after():
    """CPU: reference() asserts every case on the recursive oracle; the host build of the product core steps the same way."""
    ref, prod = W.reference(), W.reference("product")
    clean = lambda rows: [(k, a, f, 0 if f else h) for k, a, f, h in rows]   # (a step that faults leaves no state to compare)
    assert clean(ref["rows"]) == clean(prod["rows"]) and ref["pos"] == prod["pos"]
    assert sum(f == W.FAULT_DEPTH for _, _, f, _ in ref["rows"]) >= 2
    decided = lambda ds: [(d["action"], d["fault"], 0 if d["fault"] else d["hash"]) for d in ds]
    assert decided(ref["decisions"]) == decided(prod["decisions"])


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
    """One decision of the hot kernel from every described state: every legal action's look-ahead runs the handlers on the
    candidate columns; the scores, the action and the committed successor are the oracle's."""
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
