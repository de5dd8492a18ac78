"""The work stack at depth, on the CPU: the positions of tests/golden/deep_steps.json.gz (tests/deep_steps.py) on every host
core -- the recursive oracle, the product's explicit work stack, the same with the device's 21-word resident stack (so that
wk_evict / h_evicted run: nested evictions, a block restored under a further eviction), and the large record -- against
what the Python reference did on them; the fixture's coverage; the word budget at the recursion guard; and the claim that
a guard of 200 instead of 40 levels changes no game."""
import numpy as np
import pytest

import deep_steps
import oracle_lib
from c5_games import c5_games

POS = deep_steps.positions()
CORES = [("oracle", None), ("product", None), ("product_evict", None), ("oracle", 2), ("product", 2)]   # (core, record: None = the position's tier)
GUARD_GAMES = [29409, 45162, 153288, 280013, 307878, 355025, 390846, 392460, 474669]   # C5 games below 524 288 that end with code 18
N_GUARD_CLAIM = 32768   # C5 games 0 .. N - 1 of the guard test (about 10 s on 8 threads; 29409 is among them)


def _play(core, record, p):
    orc = oracle_lib.Oracle(1, extended=p["tier"] if record is None else record, core=core)
    before = deep_steps.at_position(orc, 0, p)
    f, r, d = orc.step(0, p["action"])
    return orc, before, f, r, d


_played = {}


def played(key):
    """Every position on one core: [(fault, reward, done, canon, legal, obs hash, features, hash before)]."""
    if key not in _played:
        rows = []
        for p in POS:
            orc, before, f, r, d = _play(key[0], key[1], p)
            feat = orc.features(0)
            rows.append((f, r, d, orc.canon(0), orc.legal_mask(0), orc.obs_hash(0), None if feat is None else feat.tobytes(), before))
        _played[key] = rows
    return _played[key]


@pytest.mark.parametrize("core,record", CORES, ids=[f"{c}-{'tier' if r is None else 'large'}" for c, r in CORES])
def test_every_core_lands_on_the_reference(oracle_mod, core, record):
    """Canonical record, reward, done and legal mask after the deep step are the reference's; code 18 exactly where the
    reference raised RecursionError; the word budget's code 29 nowhere."""
    for p, (f, r, d, canon, legal, _, _, before) in zip(POS, played((core, record))):
        what = (core, record, p["cls"], p["source"], len(p["prefix"]), p["action"])
        assert before == p["hash_before"], what
        assert f != 29, what
        assert f == deep_steps.expected_fault(p), (what, f)
        if f == 0:
            assert canon == bytes.fromhex(p["canon"]), what
            assert (r, d) == (p["reward"], p["done"]), what
            assert np.array_equal(legal, deep_steps.legal_of(p)), what


@pytest.mark.parametrize("core,record", CORES[1:], ids=[f"{c}-{'tier' if r is None else 'large'}" for c, r in CORES[1:]])
def test_observation_and_features_equal_the_oracle_s(oracle_mod, core, record):
    """Observation hash and feature vector after every finite deep step: bit for bit the recursive oracle's."""
    for key in [(core, record)]:
        for p, a, b in zip(POS, played(CORES[0]), played(key)):
            if a[0] == 0:
                assert a[5] == b[5] and a[6] == b[6] and a[6] is not None, (key, p["source"], p["action"])


@pytest.fixture(scope="module")
def counted(oracle_mod):
    """Every position on the counting build: [(fault, depth, words, evictions pending, words at the guard, candidates of the
    decision that evict)]."""
    rows = []
    for p in POS:
        orc = oracle_lib.Oracle(1, extended=p["tier"], core="product_count")
        deep_steps.at_position(orc, 0, p)
        evicting = int(((orc.lookahead_counts(0)[:, 0] != 255) & (orc.lookahead_counts(0)[:, 3] >= 1)).sum())
        (f, _, _), (depth, words, seg, at_guard) = orc.step_counts(0, p["action"])
        rows.append((f, depth, words, seg, at_guard, evicting))
    return rows


def test_fixture_coverage(counted):
    """The classes of scripts/deep_step_search.py hold on the counting builds (the device's 21-word resident stack), and the
    figures recorded in the fixture are the ones measured here."""
    for p, (f, depth, words, seg, at_guard, _) in zip(POS, counted):
        c = p["count"]
        assert (f, depth, words, seg, at_guard) == (c["fault"], c["depth"], c["words"], c["seg"], c["at_guard"]), p["source"]
    cls = {k: [(p, c) for p, c in zip(POS, counted) if p["cls"] == k] for k in "ABCD"}
    a = [(p, c) for p, c in zip(POS, counted) if c[0] == 0 and c[3] >= 2 and p["raised"] is None]
    print("class A (seg >= 2, finite):", len(a), "standard", sum(p["tier"] == 0 for p, _ in a), "extended", sum(p["tier"] == 1 for p, _ in a),
          "seg >= 3 or >= 100 words:", sum(c[3] >= 3 or c[2] >= 100 for _, c in a), "against the bot:", sum(p["bot_side"] >= 0 for p, _ in a))
    assert len(a) >= 8 and any(p["tier"] == 0 for p, _ in a) and any(p["tier"] == 1 for p, _ in a)
    assert any(c[3] >= 3 or c[2] >= 100 for _, c in a)
    b = [(p, c) for p, c in cls["B"] if c[0] == 18 and p["raised"] == "RecursionError"]
    print("class B (guard, reference RecursionError):", len(b), "reference nesting", sorted({p["nesting"]["move"] + p["nesting"]["ability"] for p, _ in b}))
    assert len(b) >= 2 and len(b) == len(cls["B"])
    assert len(cls["C"]) == 1
    pc, cc = cls["C"][0]
    finite = [c for p, c in zip(POS, counted) if c[0] == 0]
    print("class C (deepest finite chain): depth", cc[1], "words", cc[2], "seg", cc[3])
    assert cc[0] == 0 and pc["raised"] is None and cc[1] == max(c[1] for c in finite) == pc["count"]["depth"]
    d = [(p, c) for p, c in cls["D"] if c[5] >= 3 and c[3] >= 1]
    print("class D (three or more candidates of one decision evict):", len(d), "candidates", [c[5] for _, c in d])
    assert len(d) >= 4 and len({(p["source"], len(p["prefix"])) for p, _ in d}) >= 4


def test_word_budget_does_not_bind_before_the_guard(counted):
    """Where the guard trips the stack holds at most SK_CAP - SK_MARGIN = 608 words by wk_reserve's count, so code 18 is the
    depth and never the budget (state.h records the largest figure: 307)."""
    at = [c[4] for p, c in zip(POS, counted) if p["cls"] == "B"]
    print("words where the guard tripped:", sorted(at))
    assert at and max(at) <= 608 and all(c[1] == 40 for p, c in zip(POS, counted) if p["cls"] == "B")
    assert max(at) == 307


def _rows(core, idx, threads=8):
    """(result, steps, fault, final hash) of C5 games `idx`, W0 on both sides, 200 turns, on the extended record of `core`."""
    m, pairs = c5_games(idx)
    orc = oracle_lib.Oracle(len(idx), extended=True, core=core)
    for j in range(len(idx)):
        assert orc.reset(j, int(m["seed"][j]), pairs[j, 0], pairs[j, 1]) == 0
    _, results, steps, hashes = orc.rollout_batch(len(idx), deep_steps.W0, 200, threads)
    faults = np.array([orc.game_fault(j) for j in range(len(idx))], dtype=np.uint8)
    return results, steps, faults, hashes


def test_a_guard_of_200_levels_changes_no_game(oracle_mod):
    """The recursive oracle with MAX_DEPTH = 200 (liboracle_depth200_ext.so) against the one with 40: C5 games 0 .. 32 767 and
    the nine guard games of the first 524 288, and every fixture position.  Result, steps and fault are identical in every
    game; so is the final hash, except where both report 18 (a step the guard ended leaves its record half-way).  The C5
    games all run on the extended record, which holds every deck of the family: the guard does not depend on the record,
    and the standard build (liboracle_depth200.so) is exercised by the standard-record fixture positions."""
    idx = list(range(N_GUARD_CLAIM)) + [k for k in GUARD_GAMES if k >= N_GUARD_CLAIM]
    r40, s40, f40, h40 = _rows("oracle", idx)
    r200, s200, f200, h200 = _rows("depth200", idx)
    print("games", len(idx), "code 18:", int((f40 == 18).sum()), "other codes >= 16:", int(((f40 >= 16) & (f40 != 18)).sum()))
    assert np.array_equal(r40, r200) and np.array_equal(s40, s200) and np.array_equal(f40, f200)
    both18 = (f40 == 18) & (f200 == 18)
    assert np.array_equal(h40[~both18], h200[~both18])
    assert int(both18.sum()) >= len(GUARD_GAMES) and all(f40[idx.index(k)] == 18 for k in GUARD_GAMES)
    for p in POS:
        a, b = _play("oracle", None, p), _play("depth200", None, p)
        assert a[2:] == b[2:] and a[1] == b[1], p["source"]
        if a[2] != 18:
            assert a[0].canon_hash(0) == b[0].canon_hash(0), p["source"]


def _deep_scenarios():
    import gzip
    import json
    import os
    with gzip.open(os.path.join(deep_steps.GOLD, "deep_scenarios.json.gz"), "rt") as f:
        return json.load(f)


@pytest.mark.parametrize("core,record", CORES + [("product_count", None)],
                         ids=[f"{c}-{'tier' if r is None else 'large'}" for c, r in CORES] + ["product_count-tier"])
def test_deep_positions_and_constructed_boards_as_scenario_records(oracle_mod, core, record):
    """tests/golden/deep_scenarios.json.gz (oracle/pyref/gen_deep_scenarios.py, the recorder of the reference's unit tests):
    every fixture position as a board -- the state before, the one engine call the deep action makes, the reference's
    canonical state after and its order of ability activations -- and five CONSTRUCTED boards, on which the reference
    completes chains of depth 30, 34, 36, 38 and 40: deeper than any game of the search, the last one exactly as deep as
    the recursion guard allows.  Every core lands on the reference's state and order; the guard's code where, and only
    where, the reference raised; on the counting build the call goes exactly as deep as recorded (for a position: as the
    game's step did), so the boards carry the nested evictions to the kernel that replays scenarios on the device."""
    import scenario_lib as S
    cases = _deep_scenarios()
    found = [c for c in cases if not c["constructed"]]
    built = [c for c in cases if c["constructed"]]
    assert len(found) == len(POS) and [c["count"] for c in found] == [p["count"] for p in POS]
    for case, p in zip(found, POS):
        assert (case["records"][0]["raised"], case["records"][0].get("after") if p["raised"] is None else None) == (p["raised"] is not None, p["canon"]), case["test"]
    depths = sorted(c["count"]["depth"] for c in built)
    print("constructed boards: depth", depths, "words", [c["count"]["words"] for c in built], "evictions pending", [c["count"]["seg"] for c in built])
    assert depths[0] >= 30 and depths[-1] == 40 and sum(30 <= d < 40 for d in depths) >= 3   # (40 = MAX_DEPTH: the guard's last finite level)
    assert all(c["count"]["fault"] == 0 and c["raised"] is None and not c["records"][0]["raised"] for c in built)
    for case in cases:
        assert len(case["records"]) == 1 and not case["skipped"]
        orc = oracle_lib.Oracle(1, extended=case["tier"] if record is None else record, core=core)
        rec = case["records"][0]
        st = rec["before"]
        assert orc.scn_build(0, st["seed"], st["stream_pos"], S.encode_state(st)) == 0, case["test"]
        if core == "product_count":
            c = orc.L.orc_frame_counts()
            c[12] = c[13] = c[14] = c[15] = 0
        f, log = orc.scn_op(0, S.encode_op(rec))
        assert f != 29, case["test"]
        if core == "product_count":
            k = case["count"]
            assert (f, int(c[13]), int(c[15]), int(c[14])) == (k["fault"], k["depth"], k["words"], k["seg"]), case["test"]
            assert int(c[15]) - int(c[14]) <= 608   # wk_reserve's count stays inside the word budget at every depth the guard allows
        if rec["raised"]:
            assert f == 18, (case["test"], f)
            continue
        assert f == 0 and orc.canon(0).hex() == rec["after"], (case["test"], f)
        assert log == S.expected_log(rec), case["test"]
