"""Decks that list a card more than once, CPU side.

The reference's Unit / Structure equality is (card_id, player, position), so Player.draw's deck.remove(choice) takes the
first EQUAL card: with a repeated card the drawn object can stay in the deck while it also sits in the hand, and ages
there.  tests/golden/trace_dup.npz, trace_heuristic_dup.npz and trace_vs_expert_dup.npz are the reference's own games on
such decks (oracle/pyref/gen_golden.py: dup, heuristic_dup, vs_expert_dup), with the coverage the generator counted on the
reference by object identity.  Here: the fixtures' conditions; the extended and the large record reproduce every step on
both host cores; the standard record refuses such a deck and plays the spells-only ones; the routing rule and the ladder.
"""
import numpy as np
import pytest

import oracle_lib
import rollout_log_model as R
import vs_expert_model as M
from monsoon_amd import EXPERT
from monsoon_amd.cards import CARD_INDEX, CARD_META, FAULT_CARDS, deck_indices, needs_extended, needs_extended_each, repeats_card
from monsoon_amd.fitness import MATCH_DTYPE, tiered_rollout

# (host core, record build): product_evict -- the device's 21-word resident work stack -- exists for two records
BUILDS = [("oracle", 1), ("oracle", 2), ("product", 1), ("product", 2), ("product_evict", 1)]
FAULT_UNSUPPORTED = 20


def _spells_only(g):
    return g["klass"] == list(g["class_names"]).index("spells_only")


def test_fixture_conditions(gold):
    """The conditions the generator met on the reference, from the counts it stored: every game whose decks repeat a unit
    or structure has a step behind which one object is listed in a hand and in its deck; the set has >= 10 steps with an
    object listed twice in one deck, >= 10 reweight calls over such a deck, >= 5 plays of a hand card whose weight is not
    1; at most a quarter of the games end by an exception; every class is there, four real explore-phase pairs among them."""
    g = gold("trace_dup.npz")
    n = len(g["seeds"])
    spells = _spells_only(g)
    assert 36 <= n <= 44 and (np.diff(g["offsets"]) > 0).all()
    assert (g["cov_shared"][~spells] >= 1).all() and not g["cov_shared"][spells].any() and not g["cov_twice"][spells].any()
    assert g["cov_twice"].sum() >= 10 and g["cov_reweight"].sum() >= 10 and g["cov_aged"].sum() >= 5
    assert 4 * int(g["fault"].sum()) <= n
    names = list(g["class_names"])
    assert names == ["unit_twice", "structure_twice", "three_repeats", "one_card_three_times", "next_to_b305", "next_to_ua20",
                     "next_to_b005", "explore_phase", "spells_only"]
    per_class = np.bincount(g["klass"], minlength=len(names))
    assert (per_class >= 4).all()
    kind = np.array([c["kind"] for c in CARD_META])
    for k in range(n):
        decks = np.stack([g["deck0"][k], g["deck1"][k]])
        name = names[g["klass"][k]]
        rep = repeats_card(decks)
        if name == "spells_only":   # a spell twice in both decks, nothing else repeated
            assert not rep.any() and all(len(set(d.tolist())) < 12 for d in decks)
            assert all(kind[c] == 2 for d in decks for c in set(d.tolist()) if (d == c).sum() > 1)
        elif name == "explore_phase":
            assert rep.any()
        else:
            assert rep.all(), (k, name)   # both players hold a repeat
        must = {"next_to_b305": "b305", "next_to_ua20": "ua20", "next_to_b005": "b005"}.get(name)
        assert must is None or (decks == CARD_INDEX[must]).any(axis=1).all()
        if name == "one_card_three_times":
            assert all(np.bincount(d).max() == 3 for d in decks)
        if name == "three_repeats":
            assert all((np.bincount(d) == 2).sum() == 3 for d in decks)
    h, v = gold("trace_heuristic_dup.npz"), gold("trace_vs_expert_dup.npz")
    assert len(h["seeds"]) == 8 and (h["cov_shared"] >= 1).all() and needs_extended_each(h["decks"]).all()
    assert len(v["seeds"]) == 4 and (v["cov_shared"] >= 1).all() and sorted(v["bot_side"].tolist()) == [0, 0, 1, 1]
    assert needs_extended_each(np.stack([v["deck0"], v["deck1"]], axis=1)).all()
    # the measured share of a generation's games that repeat a unit / structure card (and any card) in the explore phase
    share = {int(r[0]): (r[2] / r[1], r[3] / r[1]) for r in g["explore_share"]}
    assert sorted(share) == [3, 5, 7] and share[3][0] < share[5][0] < share[7][0] and all(a <= b for a, b in share.values())


def _replay_game(orc, g, k, feat_row):
    """One game of a trace_live_* style fixture, every step: legal mask, reward / done, state, observation, features.
    Returns (steps compared, feature rows used)."""
    lo, hi = int(g["offsets"][k]), int(g["offsets"][k + 1])
    assert orc.reset(0, int(g["seeds"][k]), g["deck0"][k], g["deck1"][k]) == 0, k
    assert orc.canon_hash(0) == int(g["init_hash"][k]), k
    rows = 0
    for t in range(lo, hi):
        assert np.array_equal(orc.legal_mask(0), g["legal"][t]), (k, t - lo)
        f, r, d = orc.step(0, int(g["action"][t]))
        if g["fault"][k] and t == hi - 1:   # the reference raised on this step: both sides stop here
            assert f != 0 or orc.observe(0) is None, (k, t - lo)
            break
        assert f == 0, (k, t - lo, f)
        assert orc.canon_hash(0) == int(g["hash"][t]), (k, t - lo)
        assert (r, d) == (int(g["reward"][t]), int(g["done"][t])), (k, t - lo)
        assert orc.obs_hash(0) == int(g["obs"][t]), (k, t - lo)
        assert np.array_equal(orc.features(0).view(np.uint64), g["feat"][feat_row + rows].view(np.uint64)), (k, t - lo)
        rows += 1
    return hi - lo, rows


def _feature_rows(g):
    """First feature row of every game: a faulted final step has none."""
    return np.concatenate([[0], np.cumsum(np.diff(g["offsets"]) - g["fault"])])


@pytest.mark.parametrize("core,build", BUILDS)
def test_extended_and_large_records_reproduce_every_step(gold, core, build):
    """trace_dup.npz on the records that can express a shared object: every step of every game, no game cut short."""
    g = gold("trace_dup.npz")
    orc = oracle_lib.Oracle(1, extended=build, core=core)
    first = _feature_rows(g)
    steps = sum(_replay_game(orc, g, k, int(first[k]))[0] for k in range(len(g["seeds"])))
    assert steps == len(g["action"]) and first[-1] == len(g["feat"])


@pytest.mark.parametrize("core", ["oracle", "product", "product_evict"])
def test_standard_record_refuses_a_repeated_unit_or_structure_and_plays_repeated_spells(gold, core):
    """orc_reset of either core's standard build answers FAULT_UNSUPPORTED (20) for a deck that lists a unit or structure
    card twice -- a fault, as monsoon_reset answers MONSOON_ERR_ARG: the game stays faulted -- and plays the games that
    repeat only spells (a spell compares by identity: list.remove takes the drawn object) as the reference does."""
    g = gold("trace_dup.npz")
    orc = oracle_lib.Oracle(1, core=core)
    spells = _spells_only(g)
    first = _feature_rows(g)
    played = 0
    for k in range(len(g["seeds"])):
        pair = np.stack([g["deck0"][k], g["deck1"][k]])
        if spells[k]:
            assert not needs_extended(pair)
            played += _replay_game(orc, g, k, int(first[k]))[0]
        elif not np.isin(pair, [CARD_INDEX["ua20"], CARD_INDEX["b005"]]).any():
            assert orc.reset(0, int(g["seeds"][k]), pair[0], pair[1]) == FAULT_UNSUPPORTED, k
            assert orc.step(0, int(g["action"][g["offsets"][k]]))[0] == FAULT_UNSUPPORTED, k   # and stays refused
            for side in (0, 1):   # either deck alone is enough
                clean = deck_indices("N12M")
                decks = [clean, clean]
                if repeats_card(pair[side])[0]:
                    decks[side] = pair[side]
                    assert orc.reset(0, 1, decks[0], decks[1]) == FAULT_UNSUPPORTED, (k, side)
    assert spells.sum() >= 4 and played == int(np.diff(g["offsets"])[spells].sum())
    assert orc.reset(0, 1, deck_indices("N12M"), deck_indices("N12M")) == 0   # the handle plays on


@pytest.mark.parametrize("core,build", BUILDS)
def test_heuristic_selfplay_on_repeated_decks(gold, monkeypatch, core, build):
    """trace_heuristic_dup.npz: every decision's action, best score (bit for bit), score-vector hash, legal count and
    committed state; then the packaged rollout and the model of the rollout log (tests/rollout_log_model.py) over the same
    games."""
    monkeypatch.setenv("MSB_ORACLE_CORE", core)
    g = gold("trace_heuristic_dup.npz")
    orc = oracle_lib.Oracle(1, extended=build, core=core)
    w, T = g["w0"], int(g["max_turns"])
    assert not g["fault"].any()
    for k, seed in enumerate(g["seeds"]):
        lo, hi = int(g["offsets"][k]), int(g["offsets"][k + 1])
        assert orc.reset(0, int(seed), g["decks"][k, 0], g["decks"][k, 1]) == 0
        for t in range(lo, hi):
            lf = orc.lookahead_faults(0)
            assert not ((lf >= 16) & (lf != 255)).any(), (k, t - lo)   # no look-ahead hits a limit of the build
            a, scores, _ = orc.decide(0, w)
            legal = ~np.isnan(scores)
            assert a == g["action"][t] and int(legal.sum()) == g["nlegal"][t], (k, t - lo)
            assert oracle_lib.fnv1a64(scores[legal].tobytes()) == int(g["shash"][t]), (k, t - lo)
            assert np.float64(scores[a]).view(np.uint64) == g["best"][t].view(np.uint64), (k, t - lo)
            assert orc.step(0, a)[0] == 0 and orc.canon_hash(0) == int(g["hash"][t]), (k, t - lo)
        orc.reset(0, int(seed), g["decks"][k, 0], g["decks"][k, 1])
        r = orc.rollout(0, w, w, T, trace=True)
        assert r["result"] == g["result"][k] and r["steps"] == hi - lo and r["fault"] == 0
        assert np.array_equal(r["actions"], g["action"][lo:hi]) and np.array_equal(r["hashes"], g["hash"][lo:hi])
    if core == "product_evict":
        return   # the models below load their oracle by the environment variable: the two full cores
    m = np.zeros(len(g["seeds"]), dtype=MATCH_DTYPE)
    m["seed"], m["deck"] = g["seeds"], np.arange(len(m))
    _, results, steps, log = R.ModelEngine(build).rollout_logged(w[None], m, g["decks"], T)
    assert np.array_equal(steps, np.diff(g["offsets"])) and np.array_equal(results, g["result"])
    for k in range(len(m)):
        lo, hi, n = int(g["offsets"][k]), int(g["offsets"][k + 1]), int(steps[k])
        assert np.array_equal(log.action[k, :n], g["action"][lo:hi]), k
        assert np.array_equal(log.score[k, :n].view(np.uint64), g["best"][lo:hi].view(np.uint64)), k
        assert np.array_equal(log.n_legal[k, :n], g["nlegal"][lo:hi]), k
        assert (log.action[k, n:] == 255).all() and np.isnan(log.score[k, n:]).all() and not log.n_legal[k, n:].any()


@pytest.mark.parametrize("core,build", BUILDS)
def test_agent_against_the_bot_on_repeated_decks(gold, monkeypatch, core, build):
    """trace_vs_expert_dup.npz, the bot on each side: the model of the contract (tests/vs_expert_model.py) reproduces every
    action, bot flag, committed-state hash, score-vector hash, result, fault and step count; the model of the rollout log
    its actions and bot rounds."""
    monkeypatch.setenv("MSB_ORACLE_CORE", core)
    g = gold("trace_vs_expert_dup.npz")
    orc = oracle_lib.Oracle(1, extended=build, core=core)
    w, T = g["w0"][None], int(g["max_turns"])
    for k in range(len(g["seeds"])):
        bot = int(g["bot_side"][k])
        rows = (0, EXPERT) if bot == 1 else (EXPERT, 0)
        r = M.play(orc, 0, int(g["seeds"][k]), g["deck0"][k], g["deck1"][k], rows, w, T, trace=True)
        lo, hi = int(g["offsets"][k]), int(g["offsets"][k + 1])
        slo, shi = int(g["soffsets"][k]), int(g["soffsets"][k + 1])
        assert r["actions"] == g["action"][lo:hi].tolist() and r["bots"] == g["bot"][lo:hi].tolist(), k
        assert r["hashes"] == [int(x) for x in g["hash"][lo:hi]], k
        assert r["shashes"] == [int(x) for x in g["shash"][slo:shi]] and r["decisions"] == shi - slo, k
        assert (r["result"], r["steps"], int(r["fault"] != 0)) == (int(g["result"][k]), int(g["steps"][k]), int(g["fault"][k])), k
        if not g["fault"][k]:
            assert r["final"] == int(g["final"][k]), k
    if core == "product_evict":
        return
    m = np.zeros(len(g["seeds"]), dtype=MATCH_DTYPE)
    m["seed"], m["deck"] = g["seeds"], np.arange(len(m))
    m["p1"] = np.where(g["bot_side"] == 1, 0, EXPERT)
    m["p2"] = np.where(g["bot_side"] == 1, EXPERT, 0)
    _, results, steps, log = R.ModelEngine(build).rollout_logged(w, m, np.stack([g["deck0"], g["deck1"]], axis=1), T)
    assert np.array_equal(steps, g["steps"]) and np.array_equal(results, g["result"])
    for k in range(len(m)):
        lo, hi, n = int(g["offsets"][k]), int(g["offsets"][k + 1]), int(steps[k])
        bot = g["bot"][lo:hi] == 1
        assert np.array_equal(log.action[k, :n], g["action"][lo:hi]), k
        assert np.array_equal(np.isnan(log.score[k, :n]), bot) and np.array_equal(log.n_legal[k, :n] == 0, bot), k


def test_routing_rule_on_hand_made_pairs():
    """needs_extended / needs_extended_each: a unit or structure card listed twice in ONE deck, in either seat; not a card
    the two players share (equality includes the player), not a spell twice; ua20 / b005 as before."""
    base, other = deck_indices("N12M"), deck_indices("N12V")
    unit, structure, spell = CARD_INDEX["u001"], CARD_INDEX["b002"], CARD_INDEX["s001"]
    assert CARD_META[unit]["kind"] == 0 and CARD_META[structure]["kind"] == 1 and CARD_META[spell]["kind"] == 2
    assert unit in base and unit in other and structure in base and spell in base   # u001 is shared between the two decks

    def twice(deck, card):
        out = deck.copy()
        out[np.nonzero(out != card)[0][0]] = card
        assert (out == card).sum() == 2
        return out
    ua20 = base.copy()
    ua20[0] = CARD_INDEX["ua20"]
    cases = [((base, other), False),                       # a card shared between the players is no repeat
             ((twice(base, unit), other), True),           # the repeat in P1 only
             ((base, twice(other, unit)), True),           # the repeat in P2 only
             ((twice(base, structure), base), True),
             ((twice(base, spell), twice(base, spell)), False),   # a spell twice
             ((ua20, base), True), ((base, ua20), True)]   # ua20 without a repeat
    pairs = np.array([np.stack(p) for p, _ in cases])
    want = [w for _, w in cases]
    assert needs_extended_each(pairs).tolist() == want
    assert [needs_extended(p) for p in pairs] == want
    assert needs_extended([list(np.array([c["id"] for c in CARD_META])[d]) for d in pairs[1]])   # ids as well as indices
    assert not needs_extended(base) and needs_extended(twice(base, unit))                        # one deck alone
    assert repeats_card(pairs[4].reshape(-1, 12)).tolist() == [False, False]
    # up01 / up02 / up03 may repeat: their owner never completes a step (tests/golden/trace_pool_up.npz holds such decks)
    up = base.copy()
    up[0] = up[1] = CARD_INDEX["up02"]
    assert not needs_extended(np.stack([up, up])) and oracle_lib.Oracle(1).reset(0, 1, up, up) == 0
    # the native check (check_decks) reads a card's id: the first letter is its kind, up0. the cards whose int_id is < 0
    assert all("ubs"[c["kind"]] == c["id"][0] for c in CARD_META)
    assert {c["id"] for c in CARD_META if c["id"].startswith("up0")} == {c["id"] for c in CARD_META if c["int_id"] < 0} == set(FAULT_CARDS)


def test_ladder_hands_tier_0_no_pair_with_a_repeat(gold):
    """tiered_rollout over a mixed schedule -- plain pairs, ua20 pairs, the fixture's repeated pairs, its spells-only
    pairs -- with a recording play: tier 0 is handed no pair that repeats a unit / structure card, every such game starts
    on tier 1, the spells-only pairs stay on tier 0."""
    g = gold("trace_dup.npz")
    fixture = np.stack([g["deck0"], g["deck1"]], axis=1)
    plain = np.stack([deck_indices("N12M"), deck_indices("N12V")])[None]
    pairs = np.concatenate([plain, fixture])
    m = np.zeros(3 * len(pairs), dtype=MATCH_DTYPE)
    m["seed"] = np.arange(len(m))
    m["deck"] = np.arange(len(m)) % len(pairs)
    seen = {0: [], 1: []}

    def play(tier, sub, sub_pairs):
        assert int(sub["deck"].max()) == len(sub_pairs) - 1
        seen[tier].append(np.asarray(sub_pairs))
        n = len(sub)
        counts = np.zeros((1, 3), dtype=np.int64)
        counts[0] = (0, n, n)
        return counts, np.full(n, -1, dtype=np.int8), np.ones(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    _, _, _, _, replays, sizes = tiered_rollout(play, 1, m, pairs)
    low, high = np.concatenate(seen[0]), np.concatenate(seen[1])
    assert not repeats_card(low.reshape(-1, 12)).any() and not needs_extended_each(low).any()
    assert needs_extended_each(high).all()
    spells = fixture[_spells_only(g)]
    assert all(any(np.array_equal(p, q) for q in low) for p in spells)
    need = needs_extended_each(pairs)
    assert replays == 0 and sizes == [3 * int((~need).sum()), 3 * int(need.sum())] and need.sum() == len(fixture) - len(spells)
