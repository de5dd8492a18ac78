"""GPU parity tests (run with -m gpu on an MI355X): every call goes through the C ABI
(libmonsoon_hip.so via ctypes).  The HIP path is compared with
  (1) the golden vectors generated from the Python reference (tests/golden/), directly, and
  (2) the CPU replay oracle on the same seeded inputs, up to BASELINE's full size (65 536 games).
Integer/byte work: the bar is bit-exact (canonical state records, legal masks, observations,
actions; float64 features and scores compared by bit pattern)."""
import numpy as np
import pytest

import kernel_variants
import oracle_lib
from monsoon_amd.cards import deck_indices

pytestmark = pytest.mark.gpu

W0 = np.random.RandomState(2024).uniform(0, 1, 10)


@pytest.fixture(scope="module")
def engines():
    from monsoon_amd.engine import BatchEngine
    cache = {}

    def get(n, lanes=0, extended=False):
        key = (n, lanes, extended)
        if key not in cache:
            cache[key] = BatchEngine(n, lanes_per_game=lanes, extended=extended)
        return cache[key]
    yield get
    for e in cache.values():
        e.close()


def test_initial_states_vs_reference(engines, gold):
    g = gold("initial_states.npz")
    ok = list(range(len(g["seeds"])))   # N12V, N12M, S12
    eng = engines(16)
    eng.reset(g["seeds"][ok].astype(np.uint32), np.stack([np.stack([g["decks"][k]] * 2) for k in ok]))
    for j, k in enumerate(ok):
        assert eng.export(j) == g["canon"][k][:g["length"][k]].tobytes(), k


def _fnv1a64_rows(rows):
    """oracle_lib.fnv1a64 of the bytes of every row of a 2-D uint8 array, vectorised over the rows."""
    h = np.full(len(rows), 0xCBF29CE484222325, dtype=np.uint64)
    prime = np.uint64(0x100000001B3)
    for j in range(rows.shape[1]):
        h = (h ^ rows[:, j]) * prime
    return h


@pytest.mark.parametrize("name", ["trace_random_N12V.npz", "trace_random_N12M.npz", "trace_random_IRONCLAD.npz",
                                  "trace_random_S12.npz", "trace_pool.npz", "trace_pool_ext.npz", "trace_pool_up.npz",
                                  "trace_live_pool.npz", "trace_live_pool_ext.npz", "trace_live_b005.npz",
                                  "trace_live_expert.npz"])
def test_random_policy_traces_vs_reference(engines, gold, name):
    """Replays the reference's seeded random-policy games through monsoon_step in lockstep
    (trace_pool_ext, trace_live_pool_ext and trace_live_b005: all 109 observable cards on the extended-record build;
    trace_live_expert: the reference's scripted bot on both sides, through monsoon_expert_action).  The device's
    observation is compared with the reference's own (its fnv1a64 hash in the fixture) and with the oracle's, and its
    features with the reference's rows where the fixture has them.  As in test_reference_live, a capacity limit of the
    extended record (fault 16 / 22 / 23) may end a game early, and a recorded expert action 255 ends it."""
    g = gold(name)
    n = len(g["seeds"])
    ext = name.endswith("_ext.npz") or "b005" in name
    expert = "expert" in name
    eng = engines(256, 0, ext)
    eng.reset(g["seeds"], np.stack([g["deck0"], g["deck1"]], axis=1))
    assert np.array_equal(eng.state_hash(), g["init_hash"])
    orc = oracle_lib.Oracle(n, extended=ext)
    for k in range(n):
        orc.reset(k, int(g["seeds"][k]), g["deck0"][k], g["deck1"][k])
    off = g["offsets"]
    lens = (off[1:] - off[:-1]).copy()
    # feature rows exist for the steps the reference completed: a game whose last step raised has one row less
    foff = np.concatenate([[0], np.cumsum(lens - g["fault"].astype(np.int64))]) if "feat" in g.files else None
    ended = np.zeros(n, dtype=bool)
    n_obs = n_feat = 0
    for t in range(int(lens.max())):
        live = np.nonzero((lens > t) & ~ended)[0]
        masks = eng.legal_mask()
        bot = eng.expert_action()[0] if expert else None   # advances every game's stream, as the reference's bot does
        acts = np.full(n, 255, dtype=np.uint8)
        for k in live:
            assert np.array_equal(masks[k], g["legal"][off[k] + t]), (k, t)
            acts[k] = g["action"][off[k] + t]
            if expert:
                ob, fe = orc.expert_action(k)
                if acts[k] == 255:   # the reference's bot raised: the game ends here
                    assert fe != 0, (k, t)
                    ended[k] = True
                    continue
                assert fe == 0 and ob == acts[k] == bot[k], (k, t)
        reward, done, fault = eng.step(acts)
        hashes = eng.state_hash()
        obs, raises = eng.observe()
        obs_hash = _fnv1a64_rows(obs.reshape(n, -1).view(np.uint8))
        feat = eng.features() if "feat" in g.files else None
        for k in live:
            if ended[k]:
                continue
            i = off[k] + t
            fo, _, _ = orc.step(k, int(acts[k]))
            if g["fault"][k] and t == lens[k] - 1:   # the reference raised on this step
                assert fault[k] != 0 or raises[k], (k, t)
                continue
            if ext and name.startswith("trace_live_") and fault[k] in (16, 22, 23):   # a capacity limit of the record, both sides
                assert fo == fault[k], (k, t)
                ended[k] = True
                continue
            assert fault[k] == 0 and fo == 0, (k, t, fault[k])
            assert hashes[k] == g["hash"][i], (k, t)
            assert (reward[k], done[k]) == (g["reward"][i], g["done"][i]), (k, t)
            assert not raises[k] and obs_hash[k] == g["obs"][i], (k, t)   # the reference's observation itself
            assert np.array_equal(obs[k], orc.observe(k)), (k, t)
            n_obs += 1
            if feat is not None:   # the reference's StateFeatures at EVERY step (the fixture holds no rows for faulted steps)
                assert np.array_equal(feat[k].view(np.uint64), g["feat"][foff[k] + t].view(np.uint64)), (k, t)
                n_feat += 1
    print(f"{name}: {n_obs} observations and {n_feat} feature rows equal the reference's")
    if "feat" in g.files:
        assert n_feat >= len(g["feat"]) - 20   # a few rows may be lost to a tolerated capacity limit


def test_expert_bot_vs_reference(engines, gold):
    """monsoon_expert_action + monsoon_step against the reference's scripted bot playing both sides."""
    g = gold("trace_expert.npz")
    n = len(g["seeds"])
    eng = engines(256)
    eng.reset(g["seeds"], np.stack([g["deck0"], g["deck1"]], axis=1))
    off = g["offsets"]
    lens = off[1:] - off[:-1]
    for t in range(int(lens.max())):
        live = np.nonzero(lens > t)[0]
        action, fault = eng.expert_action()   # advances every game's stream; finished traces are simply ignored
        acts = np.full(n, 255, dtype=np.uint8)
        for k in live:
            i = off[k] + t
            if g["action"][i] == 255:
                assert fault[k] != 0, (k, t)
                continue
            assert fault[k] == 0 and action[k] == g["action"][i], (k, t, action[k], g["action"][i])
            acts[k] = action[k]
        _, _, sf = eng.step(acts)
        hashes = eng.state_hash()
        for k in live:
            i = off[k] + t
            if acts[k] == 255 or (g["fault"][k] and t == lens[k] - 1):
                continue
            assert sf[k] == 0 and hashes[k] == g["hash"][i], (k, t)


HEURISTIC_FIXTURES = ["trace_heuristic_N12M.npz", "trace_heuristic_S12.npz", "trace_heuristic_IRONCLAD.npz",
                      "trace_heuristic_pool.npz", "trace_heuristic_pool_ext.npz", "trace_heuristic_c5_big.npz"]


def _fixture_build(fixture):
    # "_big": games of the C5 family whose nested b005 memories outgrow the extended record, on the large record
    return 2 if fixture.endswith("_big.npz") else fixture.endswith("_ext.npz")


@pytest.mark.parametrize("fixture", HEURISTIC_FIXTURES)
def test_heuristic_selfplay_vs_reference(engines, gold, fixture):
    """monsoon_decide against the reference's HeuristicAgent self-play (corrected loop): action,
    complete score vector, best score and committed state at every decision of the fixture's games (N12M mirror,
    the Swarm deck, the reference's default Ironclad-vs-Swarm pair, per-game random decks); a game that the reference
    ends with an exception (hash 0) faults here at the same decision."""
    _heuristic_selfplay(engines(32, extended=_fixture_build(fixture)), gold(fixture), fixture)


def _heuristic_selfplay(eng, g, fixture):
    n = len(g["seeds"])
    if "decks" in g.files:
        decks = g["decks"]                       # a pair of 12-card decks per game
    else:
        decks = np.stack([g["deck"], g["deck1"] if "deck1" in g.files else g["deck"]])
    eng.reset_stats()
    eng.reset(g["seeds"], decks)
    off = g["offsets"]
    for t in range(int(g["max_turns"])):
        action, best, scores = eng.decide(g["w0"], want_scores=True)
        hashes = eng.state_hash()
        faults = eng.game_faults()
        for k in range(n):
            i = off[k] + t
            if i >= off[k + 1]:
                continue
            assert action[k] == g["action"][i], (k, t)
            legal = ~np.isnan(scores[k])
            assert int(legal.sum()) == g["nlegal"][i]
            assert oracle_lib.fnv1a64(scores[k][legal].tobytes()) == int(g["shash"][i]), (k, t)
            assert best[k] == g["best"][i]
            if int(g["hash"][i]) == 0:
                assert faults[k] != 0, (k, t)
            else:
                assert faults[k] == 0 and hashes[k] == g["hash"][i], (k, t)
    # no look-ahead of these games hits a limit of the build -- except the recursion guard in game 29409 of the C5 family,
    # where the reference raises RecursionError at the same action (equal score vectors above) and then at the same commit
    assert eng.stats()["lookahead_capacity_faults"] == (1 if fixture.endswith("_big.npz") else 0)


def test_heuristic_two_weight_vectors_vs_reference(engines, gold):
    """Per-side weight vectors [n][2][10]: the kernel uses the mover's vector as the reference's
    agents[adapter.get_current_player()] does -- action, score vector, best score, committed state of every decision."""
    _heuristic_two_weight_vectors(engines(16), gold("trace_heuristic_N12M_2w.npz"))


def _heuristic_two_weight_vectors(eng, g):
    n = len(g["seeds"])
    eng.reset(g["seeds"], np.stack([g["deck"], g["deck1"]]))
    w = np.broadcast_to(np.stack([g["w0"], g["w1"]]), (n, 2, 10)).copy()
    off = g["offsets"]
    for t in range(int(g["max_turns"])):
        action, best, scores = eng.decide(w, want_scores=True)
        hashes = eng.state_hash()
        for k in range(n):
            i = off[k] + t
            if i >= off[k + 1]:
                continue
            assert action[k] == g["action"][i], (k, t)
            legal = ~np.isnan(scores[k])
            assert oracle_lib.fnv1a64(scores[k][legal].tobytes()) == int(g["shash"][i]), (k, t)
            assert best[k] == g["best"][i] and hashes[k] == g["hash"][i], (k, t)


VARIANTS, VARIANT_IDS = kernel_variants.matrix()


@pytest.mark.parametrize("ext,u,w", VARIANTS, ids=VARIANT_IDS)
def test_heuristic_fixtures_on_every_kernel_variant(gold, monkeypatch, ext, u, w):
    """The two tests above on every hot-kernel instantiation of variants.def (each a translation unit of its own, with its
    own register allocation and, for U = 4 / 16 on the extended and large records, its own PlayLds layout), selected with
    MONSOON_LANES / MONSOON_WPE: every reference heuristic fixture of the variant's build."""
    from monsoon_amd.engine import BatchEngine
    kernel_variants.select(monkeypatch, u, w)
    eng = BatchEngine(32, extended=ext)
    try:
        assert eng.variant() == (u, w)
        ran = []
        for fixture in HEURISTIC_FIXTURES:
            if _fixture_build(fixture) == ext:
                _heuristic_selfplay(eng, gold(fixture), fixture)
                ran.append(fixture)
        if ext is False:
            _heuristic_two_weight_vectors(eng, gold("trace_heuristic_N12M_2w.npz"))
            ran.append("trace_heuristic_N12M_2w.npz")
        assert len(ran) == {False: 5, True: 1, 2: 1}[ext]
        print(f"variant {kernel_variants.BUILD_NAMES[ext]} ({u}, {w}): {', '.join(ran)}")
    finally:
        eng.close()


@pytest.mark.parametrize("lanes", [4, 8, 16, 32, 64])
def test_rollout_vs_oracle_2048_games(engines, lanes):
    """Every hot-kernel variant of the build (candidate lanes per game; 4 and 8 lanes force several passes per decision,
    the best successor so far carried across them in registers) gives the oracle's games, played to the end inside one
    launch."""
    n = 2048
    deck = deck_indices("N12M")
    eng = engines(n, lanes)
    assert eng.variant()[0] == lanes   # the variant asked for is the one that runs: no silent substitute
    matches = np.zeros(n, dtype=[("p1", "<i4"), ("p2", "<i4"), ("seed", "<u4"), ("deck", "<u4")])
    matches["seed"] = np.arange(n) + 100000
    counts, results, steps = eng.rollout(W0[None], matches, np.stack([deck, deck])[None], 200, want_results=True)
    hashes = eng.state_hash()
    orc = oracle_lib.Oracle(n)
    for i in range(n):
        orc.reset(i, 100000 + i, deck, deck)
    total, ores, osteps, ohash = orc.rollout_batch(n, W0, 200, 16)
    assert np.array_equal(results, ores)
    assert np.array_equal(steps, osteps)
    assert np.array_equal(hashes, ohash)
    assert counts[0, 2] == n and counts[0, 0] == int((ores == 0).sum()) and counts[0, 1] == int((ores == -1).sum())
    st = eng.stats()
    assert st["capacity_faults"] == 0 and st["lookahead_capacity_faults"] == 0


def test_ragged_tail_and_persistent_rounds_give_the_same_games():
    """The default hot kernel plays whole rollouts of a ragged batch with a schedule of two weight vectors as the CPU
    replay does, and its 8-decisions-per-launch persistent form plays the same games as the 4-lane variant (same games,
    several passes per decision)."""
    from monsoon_amd.engine import BatchEngine
    n = 3001   # a ragged batch size
    deck = deck_indices("N12M")
    eng = BatchEngine(8192)
    try:
        assert eng.variant()[0] == 8
        w2 = np.stack([W0, np.random.RandomState(5).uniform(0, 1, 10)])
        matches = np.zeros(n, dtype=[("p1", "<i4"), ("p2", "<i4"), ("seed", "<u4"), ("deck", "<u4")])
        matches["seed"] = np.arange(n) + 300000
        matches["p2"] = np.arange(n) % 2
        counts, results, steps = eng.rollout(w2, matches, np.stack([deck, deck])[None], 200, want_results=True)
        hashes = eng.state_hash()
        orc = oracle_lib.Oracle(n)
        ores, osteps, ohash = np.zeros(n, np.int8), np.zeros(n, np.int32), np.zeros(n, np.uint64)
        for i in range(n):
            orc.reset(i, 300000 + i, deck, deck)
            r = orc.rollout(i, w2[0], w2[i % 2], 200)
            ores[i], osteps[i], ohash[i] = r["result"], r["steps"], orc.canon_hash(i)
        assert np.array_equal(results, ores) and np.array_equal(steps, osteps) and np.array_equal(hashes[:n], ohash)
        assert counts[0, 2] == n
        # decision rounds of 8 192 games (the persistent form: more games than resident wavefronts), 8 per launch, against
        # the 4-lane variant
        ref = BatchEngine(8192, lanes_per_game=4)
        try:
            assert ref.variant()[0] == 4
            for e in (eng, ref):
                e.reset(np.arange(8192, dtype=np.uint32) + 7, np.stack([deck, deck]))
                e.reset_stats()
                e.upload_weights(w2)
                e.assign_players(np.zeros(8192, dtype=np.int32), (np.arange(8192) % 2).astype(np.int32))
                for _ in range(3):
                    e.play_rounds(8)
                e.sync()
            assert np.array_equal(eng.state_hash(), ref.state_hash())
            assert eng.stats()["lookahead_steps"] == ref.stats()["lookahead_steps"]
        finally:
            ref.close()
    finally:
        eng.close()


def test_unknown_kernel_variant_is_refused():
    from monsoon_amd._lib import MonsoonError
    from monsoon_amd.engine import BatchEngine
    with pytest.raises(MonsoonError):
        BatchEngine(64, lanes_per_game=24)   # not a variant of the build (monsoon_amd/csrc/variants.def)
    with pytest.raises(MonsoonError):
        BatchEngine(64, lanes_per_game=2)


def test_small_batches_play_every_game(engines):
    """Batches smaller than the persistent grid's 8 ranges, and one-game tails of a batched rollout: every game is
    decided / played (a range without a wavefront once left games unplayed)."""
    from monsoon_amd.engine import BatchEngine
    deck = deck_indices("N12M")
    for n in range(1, 10):
        eng = BatchEngine(n)
        eng.reset(np.arange(n, dtype=np.uint32) + 500, np.stack([deck, deck]))
        orc = oracle_lib.Oracle(n)
        for i in range(n):
            orc.reset(i, 500 + i, deck, deck)
        for t in range(3):
            action, best = eng.decide(W0)
            hashes = eng.state_hash()
            for i in range(n):
                a, sc, _ = orc.decide(i, W0)
                assert a == action[i] and best[i] == sc[a], (n, t, i)
                orc.step(i, a)
                assert orc.canon_hash(i) == int(hashes[i]), (n, t, i)
        eng.close()
    # rollout of max_games + 1 matches: the second batch holds a single game
    cap = 24
    eng = BatchEngine(cap)
    m = np.zeros(cap + 1, dtype=[("p1", "<i4"), ("p2", "<i4"), ("seed", "<u4"), ("deck", "<u4")])
    m["seed"] = 900 + np.arange(cap + 1)
    counts, results, steps = eng.rollout(W0[None], m, np.stack([deck, deck])[None], 60, want_results=True)
    orc = oracle_lib.Oracle(1)
    for i in range(cap + 1):
        orc.reset(0, 900 + i, deck, deck)
        r = orc.rollout(0, W0, W0, 60)
        assert (r["result"], r["steps"]) == (results[i], steps[i]), i
    assert counts[0, 2] == cap + 1
    eng.close()


def test_numpy_stream_and_dot_known_answers_on_gpu(gold):
    """numpy's own outputs (tests/golden/rng_kat.npz: raw MT19937 words, random(), randint, shuffle; score_kat.npz: 2 000
    scores through np.dot) against the HIP code that restates them -- fixture vs device, bit for bit."""
    from monsoon_amd.engine import BatchEngine
    eng = BatchEngine(2)
    r = gold("rng_kat.npz")
    b = np.ascontiguousarray(r["randint_bounds"])
    for s in r["seeds"]:
        s = int(s)
        assert np.array_equal(eng.debug_kat(0, s, 1500), r[f"u32_{s}"]), s          # crosses two block refills
        assert np.array_equal(eng.debug_kat(1, s, 400).view(np.uint64), r[f"random_{s}"].view(np.uint64)), s
        assert np.array_equal(eng.debug_kat(2, s, len(b), b), r[f"randint_{s}"]), s
        assert np.array_equal(eng.debug_kat(3, s, 20), r[f"shuffle12_{s}"]), s
    k = gold("score_kat.npz")
    rows = np.concatenate([k["w"], k["before"], k["after"]], axis=1)
    got = eng.debug_kat(4, 0, len(rows), rows)
    assert np.array_equal(got.view(np.uint64), k["score"].view(np.uint64))
    eng.close()


@pytest.mark.parametrize("builds", ["standard+extended", "large"])
def test_reference_unit_tests_as_scenarios_on_gpu(builds):
    """The reference's own 113 unit tests (112 card tests + the engine-level trigger-order / respawn test, test.py:53-147),
    recorded call by call on the reference (tests/golden/scenarios.json.gz): the HIP engine is put into the state the
    reference had (monsoon_debug_build), makes the one call (monsoon_debug_op) and must land on the REFERENCE's canonical
    state and on the reference's order of ability activations -- fixture vs HIP, no oracle in between.  Once on the
    records a game normally runs on (standard; extended for ua20 / b005), once with every scenario on the large record."""
    import scenario_lib as S
    from monsoon_amd.cards import CARD_INDEX
    from monsoon_amd.engine import BatchEngine
    ext_cards = [CARD_INDEX["ua20"], CARD_INDEX["b005"]]
    if builds == "large":
        big = BatchEngine(2, extended=2)
        engs = {False: big, True: big}
    else:
        engs = {False: BatchEngine(2), True: BatchEngine(2, extended=True)}
    n_calls, n_tests = 0, 0
    for case in S.load():
        for k, rec in enumerate(case["records"]):
            eng = engs[S.needs_extended(rec, ext_cards)]
            st = rec["before"]
            assert eng.debug_build(0, st["seed"], st["stream_pos"], S.encode_state(st)) == 0, (case["test"], k)
            f, log = eng.debug_op(0, S.encode_op(rec))
            if rec["raised"]:
                assert f != 0, (case["test"], k, rec["op"])
                continue
            assert f == 0, (case["test"], k, rec["op"], f)
            assert eng.export(0).hex() == rec["after"], (case["test"], k, rec["op"])
            assert log == S.expected_log(rec), (case["test"], k, rec["op"])
            n_calls += 1
        n_tests += 1
    assert n_tests == 113 + 7 and n_calls > 550   # + the quirk scenarios of SURVEY §0 (G6)
    for e in set(engs.values()):
        e.close()


def test_play_rounds_equals_single_decision_rounds():
    """monsoon_play_rounds_dev(k): k decisions per game inside one launch (record resident in LDS, "before" features
    carried from decision to decision) leave exactly the states, cursors and counters of k single-decision launches."""
    from monsoon_amd.engine import BatchEngine
    n = 3000
    deck = deck_indices("N12M")
    a, bq = BatchEngine(n), BatchEngine(n)
    for e in (a, bq):
        e.reset(np.arange(n, dtype=np.uint32) + 31, np.stack([deck, deck]))
        e.upload_weights(W0.reshape(1, 10))
        e.assign_players(np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32))
    for k in (1, 7, 40, 3):
        a.play_rounds(k)
        for _ in range(k):
            bq.decide_round()
        a.sync()
        bq.sync()
        assert np.array_equal(a.state_hash(), bq.state_hash()), k
        assert a.stats() == bq.stats(), k
    assert a.export(17) == bq.export(17)
    a.close()
    bq.close()


def test_python_level_lookahead_on_clones_equals_the_fused_decision():
    """Seam G alone is enough to run the reference's agent layer: HeuristicAgent.score_action (evo/heuristic_agent.py:23-51)
    written in Python over Game.clone() + step() + features() -- deepcopy, apply, feature delta, np.dot -- gives, for every
    legal action of every decision of a game, exactly the score vector of the fused monsoon_decide, and its first maximum
    is the action monsoon_decide commits."""
    from monsoon_amd.engine import BatchEngine
    from monsoon_amd.game import Game, StepFault
    deck = "N12M"
    g = Game(21, deck0=deck, deck1=deck, faction0=0, faction1=0)
    fused = BatchEngine(1)
    fused.reset(np.array([21], dtype=np.uint32), np.stack([deck_indices(deck), deck_indices(deck)]))
    for t in range(30):
        legal = g.legal_actions()
        before = g.env.features()
        scores = []
        for a in legal:
            c = g.clone()
            try:
                c.step(a)
                d = c.env.features() - before                     # _compute_feature_delta
                agent, enemy = np.dot(W0, d), np.dot(W0, -d)       # WeightVector.dot_product
                eff = d[0]
                pen = abs(eff) * 0.2 if eff < -0.3 else 0.0        # _compute_resource_delta
                scores.append(enemy - agent - pen)
            except (StepFault, ValueError):
                scores.append(0.0)                                 # except Exception: return 0.0
            c.close()
        action, best, full = fused.decide(W0, want_scores=True)
        assert [a for a in range(156) if not np.isnan(full[0, a])] == legal, t
        assert np.array_equal(np.array(scores).view(np.uint64), full[0, legal].view(np.uint64)), t
        assert legal[int(np.argmax(scores))] == action[0], t
        g.step(int(action[0]))
        assert g.env.state_record() == fused.export(0), t
    g.close()
    fused.close()


def test_state_save_load_round_trip_and_clone(engines):
    """monsoon_state_save / monsoon_state_load: export -> import -> export is byte-identical for every state of a game,
    and a clone loaded into another handle continues exactly like the original (copy.deepcopy incl. the stream)."""
    from monsoon_amd.engine import BatchEngine
    deck = deck_indices("N12M")
    a = BatchEngine(4)
    bq = BatchEngine(4)
    a.reset(np.array([11, 12, 13, 14], dtype=np.uint32), np.stack([deck, deck]))
    bq.reset(np.array([1, 2, 3, 4], dtype=np.uint32), np.stack([deck, deck]))
    for t in range(40):
        blob = a.save_state(2)
        bq.load_state(1, blob)
        assert bq.save_state(1) == blob, t
        assert bq.export(1) == a.export(2), t
        act_a, best_a = a.decide(W0)
        act_b, best_b = bq.decide(W0)
        assert act_a[2] == act_b[1] and best_a[2] == best_b[1] or (np.isnan(best_a[2]) and np.isnan(best_b[1])), t
        assert a.export(2) == bq.export(1), t
    a.close()
    bq.close()


def test_rollout_schedule_two_weight_vectors(engines):
    """Different individuals on each side, mixed decks: per-individual counters equal the oracle's."""
    from oracle_rollout import oracle_rollout_fn
    rs = np.random.RandomState(3)
    weights = rs.uniform(0, 1, (6, 10))
    decks = np.stack([np.stack([deck_indices("N12M"), deck_indices("N12V")]), np.stack([deck_indices("IRONCLAD"), deck_indices("SWARM")])])
    m = np.zeros(96, dtype=[("p1", "<i4"), ("p2", "<i4"), ("seed", "<u4"), ("deck", "<u4")])
    m["p1"] = rs.randint(0, 6, 96)
    m["p2"] = rs.randint(0, 6, 96)
    m["seed"] = rs.randint(0, 2**31, 96)
    m["deck"] = rs.randint(0, 2, 96)
    eng = engines(64)   # capacity < matches: exercises the batching loop
    counts, results, steps = eng.rollout(weights, m, decks, 120, want_results=True)
    ocounts, ores, osteps = oracle_rollout_fn(weights, m, decks, 120, want_results=True)
    assert np.array_equal(results, ores) and np.array_equal(steps, osteps)
    assert np.array_equal(counts, ocounts)


def test_per_game_fault_codes_equal_cpu_replay(engines):
    """monsoon_game_faults: the code that stopped each game (reference-level exceptions included) equals the CPU
    replay's, on random 12-card decks where such stops are common."""
    from monsoon_amd.cards import CARD_INDEX, supported_pool
    pool = np.array([CARD_INDEX[c] for c in supported_pool()], dtype=np.uint8)
    n = 192
    pairs = np.zeros((n, 2, 12), dtype=np.uint8)
    for g in range(n):
        rs = np.random.RandomState(g ^ 0x9E3779B9)
        pairs[g, 0], pairs[g, 1] = rs.choice(pool, 12, replace=False), rs.choice(pool, 12, replace=False)
    m = np.zeros(n, dtype=[("p1", "<i4"), ("p2", "<i4"), ("seed", "<u4"), ("deck", "<u4")])
    m["seed"] = 7000 + np.arange(n)
    m["deck"] = np.arange(n)
    eng = engines(256)
    counts, results, steps = eng.rollout(W0.reshape(1, 10), m, pairs, 150, want_results=True)
    faults = eng.game_faults()
    orc = oracle_lib.Oracle(1)
    ofaults = np.zeros(n, dtype=np.uint8)
    for g in range(n):
        orc.reset(0, int(m["seed"][g]), pairs[g, 0], pairs[g, 1])
        r = orc.rollout(0, W0, W0, 150)
        ofaults[g] = r["fault"]
        assert (r["result"], r["steps"]) == (results[g], steps[g]), g
    assert np.array_equal(faults, ofaults)
    assert (faults != 0).sum() >= 5 and (faults >= 16).sum() == 0   # exceptions do occur here; none is a build limit


def test_fitness_with_deck_schedule_equals_cpu_replay():
    """Seam F with a DeckEvolutionConfig in its explore phase (a deck pair per game): fitness from the HIP rollout
    equals the fitness from the CPU replay of the same schedule."""
    from oracle_rollout import oracle_rollout_fn
    from monsoon_amd.cards import DECKS
    from monsoon_amd.config import EvolutionaryConfig
    from monsoon_amd.decks import DeckEvolutionConfig
    from monsoon_amd.fitness import FitnessEvaluator
    from monsoon_amd.weights import WeightVector
    np.random.seed(4)
    pop = [WeightVector(10) for _ in range(4)]
    cfg = EvolutionaryConfig(mu=4, lambda_=4, games_per_pairing=2, max_turns=60, max_concurrent_games=64)
    out = []
    for fn in (None, oracle_rollout_fn):
        dc = DeckEvolutionConfig(DECKS["IRONCLAD"], DECKS["SWARM"], exploit_generations=1, explore_generations=4, seed=5)
        ev = FitnessEvaluator(cfg, dc, rollout_fn=fn)
        out.append((ev.evaluate_population(pop, 0), ev.evaluate_population(pop, 3)))
    assert out[0] == out[1]


def test_full_size_65536_games_bit_exact_and_deterministic(engines):
    """BASELINE configs[1]: 65 536 concurrent N12M self-play games, 200 decision rounds; every
    final canonical record and per-game decision count equals the CPU replay; a second run of the
    same batch reproduces the same bytes."""
    n = 65536
    deck = deck_indices("N12M")
    eng = engines(n)
    seeds = np.arange(n, dtype=np.uint32)

    def run():
        eng.reset(seeds, np.stack([deck, deck]))
        eng.upload_weights(W0[None])
        eng.assign_players(np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32))
        m = np.zeros(n, dtype=[("p1", "<i4"), ("p2", "<i4"), ("seed", "<u4"), ("deck", "<u4")])
        m["seed"] = seeds
        _, results, steps = eng.rollout(W0[None], m, np.stack([deck, deck])[None], 200, want_results=True)
        return results, steps, eng.state_hash()
    r1, s1, h1 = run()
    r2, s2, h2 = run()
    assert np.array_equal(h1, h2) and np.array_equal(r1, r2) and np.array_equal(s1, s2)
    orc = oracle_lib.Oracle(n)
    for i in range(n):
        orc.reset(i, i, deck, deck)
    _, ores, osteps, ohash = orc.rollout_batch(n, W0, 200, 16)
    assert np.array_equal(r1, ores)
    assert np.array_equal(s1, osteps)
    assert np.array_equal(h1, ohash)
    assert eng.stats()["capacity_faults"] == 0


def test_random_deck_rollouts_extended_build_bit_exact(engines):
    """A slice of BASELINE configs[4] (C5): 2 048 games, every game its own pair of 12-card decks drawn from the 109
    observable cards (ua20 and b005 included -> extended build), heuristic self-play to 200 decisions; results,
    decision counts, fault codes and final canonical records equal the CPU replay."""
    from monsoon_amd.cards import CARD_IDS
    pool = np.array([i for i, c in enumerate(CARD_IDS) if c not in ("up01", "up02", "up03")], dtype=np.uint8)
    n = 2048
    pairs = np.zeros((n, 2, 12), dtype=np.uint8)
    for g in range(n):
        rs = np.random.RandomState(g ^ 0x9E3779B9)
        pairs[g, 0], pairs[g, 1] = rs.choice(pool, 12, replace=False), rs.choice(pool, 12, replace=False)
    m = np.zeros(n, dtype=[("p1", "<i4"), ("p2", "<i4"), ("seed", "<u4"), ("deck", "<u4")])
    m["seed"] = 90000 + np.arange(n)
    m["deck"] = np.arange(n)
    eng = engines(n, extended=True)
    _, results, steps = eng.rollout(W0[None], m, pairs, 200, want_results=True)
    hashes, faults = eng.state_hash(), eng.game_faults()
    orc = oracle_lib.Oracle(n, extended=True)
    for g in range(n):
        assert orc.reset(g, int(m["seed"][g]), pairs[g, 0], pairs[g, 1]) == 0
    _, ores, osteps, ohash = orc.rollout_batch(n, W0, 200, 16)
    assert np.array_equal(results, ores) and np.array_equal(steps, osteps)
    assert np.array_equal(hashes, ohash)
    # reference-level exceptions are frequent with these decks; restored nested b005 memories are reproduced (worlds,
    # state.h) -- what remains are the capacity limits of the record (64 entity slots, memory lists, worlds, deck
    # entries), reported per game (the rollout path replays them on the large record) and required to stay below 2 % here
    assert (faults == 1).sum() > n // 10 and (faults == 20).sum() == 0 and (faults >= 16).sum() <= n // 50


from c5_games import C5_OVERFLOWING, c5_games as _c5_games  # noqa: E402


def test_large_record_build_matches_its_replay(engines):
    """libmonsoon_hip_big.so (254 entity slots, 32 memory lists, 16 worlds): rollouts of C5 games -- the ones that overflow
    the extended record and 108 ordinary ones -- equal the CPU replay on the same record: results, decisions, fault codes,
    final canonical records.  On the games the extended record CAN hold, the three quantities also equal the extended
    build's: the record layout is not observable."""
    idx = C5_OVERFLOWING + list(range(108))
    m, pairs = _c5_games(idx)
    n = len(idx)
    big = engines(n, extended=2)
    assert big.lib.monsoon_version() & 0x20000
    _, results, steps = big.rollout(W0[None], m, pairs, 200, want_results=True)
    hashes, faults = big.state_hash(), big.rollout_faults(n)
    assert np.array_equal(faults, big.game_faults())
    from monsoon_amd._lib import MonsoonError
    with pytest.raises(MonsoonError):
        big.rollout_faults(n + 1)   # not the size of the last rollout: refused, nothing copied
    orc = oracle_lib.Oracle(n, extended=2)
    for g in range(n):
        assert orc.reset(g, int(m["seed"][g]), pairs[g, 0], pairs[g, 1]) == 0
    _, ores, osteps, ohash = orc.rollout_batch(n, W0, 200, 16)
    assert np.array_equal(results, ores) and np.array_equal(steps, osteps) and np.array_equal(hashes, ohash)
    assert np.array_equal(faults, [orc.game_fault(g) for g in range(n)])
    assert (faults[:len(C5_OVERFLOWING)] >= 16).sum() <= 4    # what not even 254 slots hold (2063, 6149, 10993 here)
    ext = engines(n, extended=True)
    _, r1, s1 = ext.rollout(W0[None], m, pairs, 200, want_results=True)
    f1, h1 = ext.rollout_faults(n), ext.state_hash()
    fits = f1 < 16
    assert (~fits).sum() >= len(C5_OVERFLOWING) - 1 and fits[len(C5_OVERFLOWING):].mean() > 0.9
    assert np.array_equal(r1[fits], results[fits]) and np.array_equal(s1[fits], steps[fits]) and np.array_equal(h1[fits], hashes[fits])
    assert np.array_equal(f1[fits], faults[fits])


def test_fitness_rollout_replays_overflowing_games_on_the_large_record():
    """FitnessEvaluator's rollout (Seam F): the games the extended record cannot hold are replayed on the large record and
    their rows replaced -- counts, results, decision counts and fault codes equal the CPU replay doing the same."""
    from oracle_rollout import oracle_rollout_fn_mt
    from monsoon_amd.config import EvolutionaryConfig
    from monsoon_amd.fitness import FitnessEvaluator
    idx = C5_OVERFLOWING + list(range(300, 492))
    m, pairs = _c5_games(idx)
    rs = np.random.RandomState(12)
    weights = rs.uniform(0, 1, (8, 10))
    weights[0] = W0
    m["p1"], m["p2"] = rs.randint(0, 8, len(idx)), rs.randint(0, 8, len(idx))
    m["p1"][:len(C5_OVERFLOWING)] = m["p2"][:len(C5_OVERFLOWING)] = 0    # W0 on both sides: the games known to overflow
    fe = FitnessEvaluator(EvolutionaryConfig(max_concurrent_games=128, max_turns=200))   # two batches on the extended build
    counts = fe._hip_rollout(weights, m, pairs, 200)
    results, steps, faults = fe.last_rollout
    ocounts, ores, osteps, ofaults = oracle_rollout_fn_mt(weights, m, pairs, 200, want_faults=True)
    assert np.array_equal(counts, ocounts) and counts[:, 2].sum() == len(idx)
    assert np.array_equal(results, ores) and np.array_equal(steps, osteps) and np.array_equal(faults, ofaults)
    st = fe.get_stats()
    from monsoon_amd.fitness import record_limited
    assert st["capacity_replays"] >= len(C5_OVERFLOWING) - 1 and st["capacity_faults"] == int(record_limited(ofaults).sum()) <= 4
    assert st["depth_faults"] == int((ofaults == 18).sum())   # the recursion guard = the reference's RecursionError: never replayed


def test_handles_of_several_builds_alive_at_once():
    """A standard, an extended and a large handle in one process (a deck schedule that mixes ua20 / b005 decks with plain
    ones, the replay tier): they share one hardware queue and one device-wide stack limit.  With a stream per handle
    every k_play launch cost 200-500 ms once two of them held scratch memory; a handle created later must
    not shrink the stack of the kernels of an earlier one either.  Decisions stay bit-exact and launches stay cheap."""
    import time
    from monsoon_amd.engine import BatchEngine
    deck = deck_indices("N12M")
    engs = [BatchEngine(32, extended=t) for t in (1, 0, 2, 0)]   # the standard build is created AFTER the extended one
    orcs = []
    for e in engs:
        e.reset(np.arange(32, dtype=np.uint32) + 7, np.stack([deck, deck]))
        o = oracle_lib.Oracle(32, extended=e.extended)
        for g in range(32):
            o.reset(g, g + 7, deck, deck)
        orcs.append(o)
    t0 = time.time()
    for _ in range(12):
        for e, o in zip(engs, orcs):
            action, _ = e.decide(W0)
            hashes = e.state_hash()
            for g in range(32):
                a, _, _ = o.decide(g, W0)
                assert a == action[g]
                o.step(g, a)
                assert o.canon_hash(g) == int(hashes[g])
    dt = time.time() - t0
    for e in engs:
        assert e.stats()["capacity_faults"] == 0
        e.close()
    assert dt < 10.0, f"48 decision rounds of 32 games took {dt:.1f} s: launches are paying for scratch hand-over again"


def test_own_stream_mode_gives_the_same_games():
    """MONSOON_OWN_STREAM=1 (a stream per handle instead of the device's default stream, include/monsoon.h) only changes
    where the launches are queued: a child process in that mode reaches the same states."""
    import subprocess
    import sys
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r);"
        "from monsoon_amd.engine import BatchEngine; from monsoon_amd.cards import deck_indices;"
        "d = deck_indices('N12M'); e = BatchEngine(64); e.reset(np.arange(64, dtype=np.uint32) + 3, np.stack([d, d]));"
        "w = np.random.RandomState(2024).uniform(0, 1, 10);"
        "[e.decide(w) for _ in range(6)];"
        "assert e.lib.monsoon_stream(e.h) %s;"
        "print(' '.join(str(int(h)) for h in e.state_hash()))"
    )
    import os
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for own in ("1", "0"):
        env = dict(os.environ, MONSOON_OWN_STREAM=own)
        r = subprocess.run([sys.executable, "-c", code % (repo, "is not None" if own == "1" else "is None")], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout.strip().splitlines()[-1])
    assert outs[0] == outs[1] and len(outs[0].split()) == 64


def test_config_c3_ga_loop_through_the_hip_path(tmp_path):
    """BASELINE configs[2] (C3): the GA driver loop of evo/evolution.py:60-111 -- mu = lambda = 128, 64 games per
    individual (ring schedule), N12M, seed 42 -- for two generations (8 192 + 16 384 games, 200 decisions each) through
    EvolutionEngine -> FitnessEvaluator -> monsoon_rollout.  The same run on the CPU replay gives the same fitness list,
    the same selected population and the same best individual."""
    from oracle_rollout import oracle_rollout_fn_mt
    from monsoon_amd.config import EvolutionaryConfig
    from monsoon_amd.evolution import EvolutionEngine
    runs = []
    for name, fn in (("hip", None), ("cpu", oracle_rollout_fn_mt)):
        cfg = EvolutionaryConfig(mu=128, lambda_=128, generations=2, schedule="ring", games_per_individual=64, deck="N12M", max_turns=200,
                                 seed=42, results_dir=str(tmp_path / name), save_logs=False, checkpoint_interval=1000,
                                 max_concurrent_games=16384)
        eng = EvolutionEngine(cfg, rollout_fn=fn)
        eng.initialize()
        res = eng.run()
        runs.append((list(eng.population.fitness_scores), np.stack([i.get_weights() for i in eng.population.individuals]), res))
        if fn is None:
            st = eng.fitness_evaluator.get_stats()
            assert st["total_games"] == 128 * 64 + 256 * 64 and st["env_steps"] > 50_000_000
    (f_hip, w_hip, r_hip), (f_cpu, w_cpu, r_cpu) = runs
    assert f_hip == f_cpu
    assert np.array_equal(w_hip.view(np.uint64), w_cpu.view(np.uint64))
    assert r_hip["best_fitness"] == r_cpu["best_fitness"] and r_hip["generations"] == 2


def test_config_c4_shape_on_one_gpu():
    """BASELINE configs[3] (C4) on one GPU: population 1 024 on the Swarm deck S12 (on-death / summon triggers), ring
    schedule, 8 games per individual = 8 192 games through FitnessEvaluator; per-individual fitness equals the CPU replay
    of the same schedule.  (The 8-GPU form shards this schedule by row individual: tests/test_distributed_cpu.py.)"""
    from oracle_rollout import oracle_rollout_fn_mt
    from monsoon_amd.config import EvolutionaryConfig
    from monsoon_amd.fitness import FitnessEvaluator
    from monsoon_amd.weights import WeightVector
    np.random.seed(5)
    pop = [WeightVector(10) for _ in range(1024)]
    cfg = EvolutionaryConfig(mu=1024, lambda_=1024, schedule="ring", games_per_individual=8, deck="S12", max_turns=200,
                             max_concurrent_games=8192)
    f_hip = FitnessEvaluator(cfg).evaluate_population(pop, generation=7)
    f_cpu = FitnessEvaluator(cfg, rollout_fn=oracle_rollout_fn_mt).evaluate_population(pop, generation=7)
    assert f_hip == f_cpu
    assert len(set(f_hip)) > 5   # games do get decided on this deck


def test_failed_rollouts_leave_device_memory_alone():
    """A schedule whose bad entry sits in what would be the SECOND batch is refused before anything is loaded, and
    repeated refusals (and successes) do not move the device's free memory: the rollout's result buffers live in the
    handle, nothing is allocated or leaked per call."""
    import torch
    from monsoon_amd import MonsoonError
    from monsoon_amd.engine import BatchEngine
    deck = deck_indices("N12M")
    pairs = np.stack([deck, deck])[None]
    dt = [("p1", "<i4"), ("p2", "<i4"), ("seed", "<u4"), ("deck", "<u4")]
    eng = BatchEngine(32)
    good = np.zeros(40, dtype=dt)
    eng.rollout(W0[None], good, pairs, 5)          # allocates the handle's buffers once
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    bad = np.zeros(40, dtype=dt)
    bad["p2"][36] = 9                              # second batch (capacity 32): only individual 0 exists
    for _ in range(5):
        with pytest.raises(MonsoonError, match="schedule entry 36"):
            eng.rollout(W0[None], bad, pairs, 5)
        counts = eng.rollout(W0[None], good, pairs, 5)
        assert counts[0, 2] == 40
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    eng.close()


def test_observation_tensor_view_on_device(engines):
    """the batched observation lands in a torch-ROCm tensor without a host round trip."""
    import torch
    eng = engines(256)
    deck = deck_indices("N12M")
    eng.reset(np.arange(200, dtype=np.uint32), np.stack([deck, deck]))
    orc = oracle_lib.Oracle(200)
    for k in range(200):
        orc.reset(k, k, deck, deck)
    for _ in range(5):
        action, _ = eng.decide(W0)
        for k in range(200):
            orc.step(k, int(action[k]))
    dev, draises = eng.observe_torch()
    assert dev.is_cuda and dev.shape == (200, 27, 5, 4) and dev.dtype == torch.int32
    got = dev.cpu().numpy()
    for k in range(200):   # against the CPU replay's observation of the same state, game by game
        assert np.array_equal(got[k], orc.observe(k)), k
    assert not draises.cpu().numpy().any()


def test_rollout_rejects_empty_and_out_of_range_schedules(engines):
    """Empty schedule, a match naming a missing deck or individual, a ragged deck array: refused with an error, no
    game is played (the reference would raise IndexError / produce nothing)."""
    from monsoon_amd import MonsoonError
    eng = engines(64)
    deck = deck_indices("N12M")
    pairs = np.stack([deck, deck])[None]
    dt = [("p1", "<i4"), ("p2", "<i4"), ("seed", "<u4"), ("deck", "<u4")]
    with pytest.raises(MonsoonError):
        eng.rollout(W0[None], np.zeros(0, dtype=dt), pairs, 10)
    m = np.zeros(4, dtype=dt)
    m["deck"][2] = 1                      # only deck 0 exists
    with pytest.raises(MonsoonError):
        eng.rollout(W0[None], m, pairs, 10)
    m = np.zeros(4, dtype=dt)
    m["p2"][1] = 3                        # only individual 0 exists
    with pytest.raises(MonsoonError):
        eng.rollout(W0[None], m, pairs, 10)
    with pytest.raises(ValueError):
        eng.rollout(W0[None], np.zeros(4, dtype=dt), np.zeros((1, 2, 11), dtype=np.uint8), 10)
    # and a well-formed call still works on the same handle afterwards
    counts = eng.rollout(W0[None], np.zeros(4, dtype=dt), pairs, 5)
    assert counts[0, 2] == 4


def test_game_view_and_error_behaviour(engines):
    from monsoon_amd import MonsoonError
    from monsoon_amd.engine import BatchEngine
    from monsoon_amd.game import Game
    g = Game(0)
    orc = oracle_lib.Oracle(1)
    orc.reset(0, 0, deck_indices("IRONCLAD"), deck_indices("SWARM"), 3, 2)
    assert g.legal_actions() == orc.legal_actions(0) == [0, 1, 2, 3, 16, 17, 18, 19, 32, 33, 34, 35, 148, 149, 150, 151]
    obs0 = g.reset()
    assert obs0.shape == (27, 5, 4) and obs0.dtype == np.int32 and np.array_equal(obs0, orc.observe(0))
    obs, reward, done = g.step(0)
    orc.step(0, 0)
    assert np.array_equal(obs, orc.observe(0)) and reward in (0, 10) and done is False
    assert g.to_play() == 0
    with pytest.raises(MonsoonError, match="illegal action"):
        g.step(64)   # no spell in hand slot 0
    g.close()
    e = BatchEngine(4)
    with pytest.raises(MonsoonError, match="monsoon_reset first"):
        e.legal_mask()
    ua20_deck = deck_indices("N12M").copy()
    ua20_deck[0] = __import__("monsoon_amd").CARD_INDEX["ua20"]   # needs the extended record
    bad = np.stack([ua20_deck, ua20_deck])
    with pytest.raises(MonsoonError, match="not supported"):
        e.reset(np.array([1], dtype=np.uint32), bad[None])
    e.close()


def test_draw_decks_on_device_equals_numpy(engines, gold):
    """monsoon_draw_decks (configuration C5's per-game decks) against numpy's own RandomState(seed).choice(pool, 12,
    replace=False): the committed known answers (1 024 seeds, oracle/pyref/gen_deck_draw.py) and 2 000 more seeds drawn by
    numpy right here; every deck holds 12 distinct observable cards."""
    from monsoon_amd.cards import draw_random_decks_numpy, observable_pool
    g = gold("deck_draw_kat.npz")
    eng = engines(64)
    assert np.array_equal(g["pool"], observable_pool())
    assert np.array_equal(eng.draw_decks(g["seeds"], g["pool"]), g["pairs"])
    seeds = (np.arange(2000, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(2**32)).astype(np.uint32)
    got = eng.draw_decks(seeds, observable_pool())
    assert np.array_equal(got, draw_random_decks_numpy(seeds))
    assert all(len(set(d.tolist())) == 12 for d in got.reshape(-1, 12))
    small = np.arange(12, dtype=np.uint8)   # a pool of exactly 12 cards: every draw is a permutation of it
    got12 = eng.draw_decks(seeds[:50], small)
    assert np.array_equal(np.sort(got12.reshape(-1, 12), axis=1), np.tile(small, (100, 1)))
    assert np.array_equal(got12, draw_random_decks_numpy(seeds[:50], small))   # ... and the one numpy draws
    from monsoon_amd import MonsoonError
    with pytest.raises(MonsoonError):
        eng.draw_decks(seeds[:4], np.arange(11, dtype=np.uint8))   # fewer than 12 cards: refused


def test_draw_decks_on_device_at_the_pool_sizes_that_move_the_mask(engines):
    """monsoon_draw_decks against RandomState(seed).choice(pool, 12, replace=False) taken twice, drawn by numpy right here
    (test_oracle_golden.draw_pool_cases: 64 seeds, 0, 1 and 2**32 - 1 among them, pool sizes on both sides of every power
    of two from 12 to 128, where the mask of the shuffle's random_interval(i) changes).  A pool of 129 is refused, as one
    of 11 is, and the handle draws the known answer afterwards."""
    from monsoon_amd import MonsoonError
    from test_oracle_golden import DRAW_POOL_SIZES, draw_pool_cases
    eng = engines(64)
    seen = []
    for pool, seeds, want in draw_pool_cases():
        got = eng.draw_decks(seeds, pool)
        bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
        assert len(bad) == 0, f"pool of {len(pool)}: {len(bad)} of {len(seeds)} seeds differ, first {int(seeds[bad[0]])}: {got[bad[0]].tolist()} != {want[bad[0]].tolist()}"
        seen.append(len(pool))
    assert tuple(seen) == DRAW_POOL_SIZES
    with pytest.raises(MonsoonError, match="status 1"):
        eng.draw_decks(seeds[:4], np.arange(129, dtype=np.uint8) % 112)
    assert np.array_equal(eng.draw_decks(seeds, pool), want)


def test_mixed_schedule_is_tiered_per_game_and_equals_cpu_replay():
    """A schedule mixing decks with and without ua20 / b005 (4 096 random109 games: 37 % need the extended record): the
    evaluator plays every game on the smallest record its decks need (fitness.tiered_rollout) and every row -- counts,
    results, decision counts, fault codes -- equals the CPU replay doing the same; the same schedule forced onto the
    extended record gives the same rows wherever no record limit was hit (the record layout is not observable)."""
    from oracle_rollout import oracle_draw_decks, oracle_rollout_fn_mt
    from monsoon_amd.cards import needs_extended_each, observable_pool
    from monsoon_amd.config import EvolutionaryConfig
    from monsoon_amd.fitness import MATCH_DTYPE, FitnessEvaluator
    n = 4096
    rs = np.random.RandomState(77)
    m = np.zeros(n, dtype=MATCH_DTYPE)
    m["seed"] = rs.randint(0, 2**31, n)
    m["p1"], m["p2"] = rs.randint(0, 6, n), rs.randint(0, 6, n)
    m["deck"] = np.arange(n)
    weights = rs.uniform(0, 1, (6, 10))
    fe = FitnessEvaluator(EvolutionaryConfig(max_concurrent_games=4096, max_turns=200))
    pairs = fe._engine(0).draw_decks(m["seed"] ^ np.uint32(0x9E3779B9), observable_pool())
    assert np.array_equal(pairs, oracle_draw_decks(m["seed"] ^ np.uint32(0x9E3779B9), observable_pool()))
    ext = needs_extended_each(pairs)
    assert 0.25 < ext.mean() < 0.5
    counts = fe._hip_rollout(weights, m, pairs, 200)
    results, steps, faults = fe.last_rollout
    assert fe.tier_games == [int((~ext).sum()), int(ext.sum())]
    oc, ores, osteps, of = oracle_rollout_fn_mt(weights, m, pairs, 200, want_faults=True)
    assert np.array_equal(counts, oc) and np.array_equal(results, ores) and np.array_equal(steps, osteps) and np.array_equal(faults, of)
    from monsoon_amd.engine import BatchEngine
    e1 = BatchEngine(n, extended=True)   # everything on the extended record
    _, r1, s1 = e1.rollout(weights, m, pairs, 200, want_results=True)
    ok = (e1.rollout_faults(n) < 16) & (faults < 16)
    assert ok.mean() > 0.97 and np.array_equal(r1[ok], results[ok]) and np.array_equal(s1[ok], steps[ok])
    e1.close()


def test_two_rollouts_with_a_small_tail_on_one_handle(engines):
    """A schedule of max_games + a tail smaller than the resident grid, twice on one handle: persistent, non-persistent,
    persistent, non-persistent launches of the hot kernel in turn.  The persistent form's game counters alternate
    between two sets, one of which a launch clears for the next: a non-persistent launch in between must not advance
    that alternation (round 2 did: the next persistent launch then played only the first game of every range and
    reported the rest as draws).  Every row equals the CPU replay."""
    from oracle_rollout import oracle_rollout_tier
    cap = 16384
    n = cap + 300
    deck = deck_indices("S12")
    pairs = np.stack([deck, deck])[None]
    eng = engines(cap)
    rs = np.random.RandomState(3)
    weights = rs.uniform(0, 1, (4, 10))
    for rep in range(2):
        m = np.zeros(n, dtype=[("p1", "<i4"), ("p2", "<i4"), ("seed", "<u4"), ("deck", "<u4")])
        m["seed"] = 7000 + rep * n + np.arange(n)
        m["p1"], m["p2"] = rs.randint(0, 4, n), rs.randint(0, 4, n)
        counts, results, steps = eng.rollout(weights, m, pairs, 200, want_results=True)
        oc, ores, osteps, of = oracle_rollout_tier(weights, m, pairs, 200, 0, threads=16)
        assert np.array_equal(results, ores) and np.array_equal(steps, osteps) and np.array_equal(counts, oc), rep
        assert (steps > 0).all()


def test_config_c3_full_size_ten_generations(tmp_path):
    """BASELINE configs[2] (C3) at its full size: mu = lambda = 128, 64 games per individual, N12M, ten generations (8 192 +
    9 x 16 384 = 155 648 games, ~0.7 G env-steps) through EvolutionEngine -> FitnessEvaluator -> monsoon_rollout; fitness
    lists, selected population and best individual equal the same GA run on the 16-thread CPU replay."""
    from oracle_rollout import oracle_rollout_fn_mt
    from monsoon_amd.config import EvolutionaryConfig
    from monsoon_amd.evolution import EvolutionEngine
    runs = []
    for name, fn in (("hip", None), ("cpu", oracle_rollout_fn_mt)):
        cfg = EvolutionaryConfig(mu=128, lambda_=128, generations=10, min_generations=50, schedule="ring", games_per_individual=64, deck="N12M",
                                 max_turns=200, seed=42, results_dir=str(tmp_path / name), save_logs=False, checkpoint_interval=1000,
                                 max_concurrent_games=16384)
        eng = EvolutionEngine(cfg, rollout_fn=fn)
        eng.initialize()
        res = eng.run()
        runs.append((list(eng.population.fitness_scores), np.stack([i.get_weights() for i in eng.population.individuals]), res))
        if fn is None:
            assert eng.fitness_evaluator.get_stats()["total_games"] == 128 * 64 + 9 * 256 * 64
    (f_hip, w_hip, r_hip), (f_cpu, w_cpu, r_cpu) = runs
    assert f_hip == f_cpu and np.array_equal(w_hip.view(np.uint64), w_cpu.view(np.uint64))
    assert r_hip["best_fitness"] == r_cpu["best_fitness"] and r_hip["generations"] == 10


def test_config_c4_full_size_on_one_gpu():
    """BASELINE configs[3] (C4) at its full size on one GPU: population 1 024 on the Swarm deck S12, ring schedule, 64 games per
    individual = 65 536 games; per-individual fitness, every result and every decision count equal the CPU replay."""
    from oracle_rollout import oracle_rollout_fn_mt
    from monsoon_amd.config import EvolutionaryConfig
    from monsoon_amd.fitness import FitnessEvaluator
    from monsoon_amd.weights import WeightVector
    np.random.seed(5)
    pop = [WeightVector(10) for _ in range(1024)]
    cfg = EvolutionaryConfig(mu=1024, lambda_=1024, schedule="ring", games_per_individual=64, deck="S12", max_turns=200, max_concurrent_games=65536)
    hip, cpu = FitnessEvaluator(cfg), FitnessEvaluator(cfg, rollout_fn=lambda *a, **k: oracle_rollout_fn_mt(*a, want_faults=True, **k)[0])
    f_hip = hip.evaluate_population(pop, generation=7)
    assert f_hip == cpu.evaluate_population(pop, generation=7) and hip.get_stats()["total_games"] == 65536
    assert hip.capacity_faults == 0 and len(set(f_hip)) > 30   # fitness values are multiples of 1/128


def test_config_c5_one_generation_full_size():
    """BASELINE configs[4] (C5), one whole generation on one GPU: population 4 096, 128 games per individual = 524 288 games,
    every game its own two decks drawn on the device from the 109 observable cards (monsoon_draw_decks), played on the
    record its decks need, overflowing games replayed on the next larger one -- through FitnessEvaluator.evaluate_population.
    Fitness of all 4 096 individuals, every result, decision count and fault code equal the CPU replay of the same schedule
    (decks by the CPU restatement of the draw, itself pinned to numpy's); what still ends on a record limit is reported."""
    import time
    from oracle_rollout import oracle_draw_decks, oracle_rollout_fn_mt
    from monsoon_amd.cards import RANDOM_DECK
    from monsoon_amd.config import EvolutionaryConfig
    from monsoon_amd.fitness import FitnessEvaluator
    from monsoon_amd.weights import WeightVector
    np.random.seed(11)
    pop = [WeightVector(10) for _ in range(4096)]
    cfg = EvolutionaryConfig(mu=4096, lambda_=4096, schedule="ring", games_per_individual=128, deck=RANDOM_DECK, max_turns=200,
                             max_concurrent_games=65536)
    hip = FitnessEvaluator(cfg)
    hip.use_hall_of_fame = False
    hip.evaluate_population(pop[:64], generation=0)   # creates the engines of both tiers
    hip.reset_stats()
    hip.tier_games, hip.capacity_replays, hip.capacity_faults = [0, 0], 0, 0
    t0 = time.time()
    f_hip = hip.evaluate_population(pop, generation=3)
    t_hip = time.time() - t0
    results, steps, faults = hip.last_rollout
    box = {}

    def cpu_rollout(weights, matches, deck_pairs, max_turns):
        box["rows"] = oracle_rollout_fn_mt(weights, matches, deck_pairs, max_turns, want_faults=True)
        return box["rows"][0]
    cpu = FitnessEvaluator(cfg, rollout_fn=cpu_rollout, deck_draw_fn=oracle_draw_decks)
    cpu.use_hall_of_fame = False
    t0 = time.time()
    f_cpu = cpu.evaluate_population(pop, generation=3)
    t_cpu = time.time() - t0
    _, ores, osteps, of = box["rows"]
    assert f_hip == f_cpu
    assert np.array_equal(results, ores) and np.array_equal(steps, osteps) and np.array_equal(faults, of)
    st = hip.get_stats()
    assert st["total_games"] == 524288 and sum(hip.tier_games) == 524288 and hip.tier_games[1] > 150000
    from monsoon_amd.fitness import record_limited
    left, deep = int(record_limited(faults).sum()), int((faults == 18).sum())
    print(f"C5 generation: {t_hip:.2f} s on the GPU end to end ({st['env_steps'] / 1e6:.0f} M env-steps), {t_cpu:.1f} s CPU replay; "
          f"tiers {hip.tier_games}, {hip.capacity_replays} replayed, {left} left on a record limit, {deep} ended by the recursion guard")
    assert left == hip.capacity_faults and deep == hip.depth_faults
    assert left <= 524288 // 2000   # 0.05 %: nested copies beyond 254 entity objects


def test_ga_operators_on_device(engines, gold):
    """Population.generate_offspring (evo/population.py:75-89, evo/weights.py:12-40) and the selection order
    on the device.  Against the host GA run by numpy itself (tests/golden/ga_kat.npz) and against the CPU restatement: the
    parents drawn, the polar-method rounds behind every child (the accept / reject pattern: 1 024 children x 21 normals)
    and the stream state handed back -- key, position, has_gauss -- are IDENTICAL; sigmas within 4 ulp, weights within
    1e-15 (exp / log / sqrt are the device library's).  Then a host GA generation and a device one from the same numpy
    state leave numpy's global stream in the same state."""
    from test_oracle_golden import orc_ga, ulps
    g = gold("ga_kat.npz")
    eng = engines(64)
    worst_s = worst_w = 0.0
    for tag in ("a", "b"):
        mu, lam, dim = (int(x) for x in g[f"{tag}_cfg"])
        tau, taup, mins = (float(x) for x in g[f"{tag}_params"])
        st0 = ("MT19937", g[f"{tag}_st0_key"], int(g[f"{tag}_st0_pos"][0]), int(g[f"{tag}_st0_pos"][1]), float(g[f"{tag}_st0_gauss"][0]))
        ow, osg, par, tries, st1 = eng.ga_offspring(st0, g[f"{tag}_pw"], g[f"{tag}_ps"], lam, tau, taup, mins)
        o_w, o_s, o_par, o_tries, o_key, o_pos, o_hg, o_g = orc_ga(g, tag)
        assert np.array_equal(par, o_par) and np.array_equal(tries, o_tries)
        assert np.array_equal(st1[1], g[f"{tag}_st1_key"]) and [st1[2], st1[3]] == g[f"{tag}_st1_pos"].tolist()
        assert ulps([st1[4]], g[f"{tag}_st1_gauss"]).max() <= 4
        worst_s = max(worst_s, float(ulps(osg, g[f"{tag}_ks"]).max()))
        worst_w = max(worst_w, float(np.abs(ow - g[f"{tag}_kw"]).max()))
    assert worst_s <= 4 and worst_w <= 1e-15, (worst_s, worst_w)
    print(f"device GA offspring vs numpy: sigmas within {worst_s:.0f} ulp, weights within {worst_w:.2e}")
    # the wrapper: numpy's global stream ends in the same state whichever side mutates
    from monsoon_amd.config import EvolutionaryConfig
    from monsoon_amd.population import Population
    states = []
    for use_device in (False, True):
        pop = Population(EvolutionaryConfig(mu=64, lambda_=256, seed=123))
        pop.initialize_population(10)
        kids = pop.generate_offspring(engine=eng if use_device else None)
        st = np.random.get_state()
        states.append((st[1].copy(), st[2], st[3], np.stack([k.weights for k in kids]), np.stack([k.sigmas for k in kids])))
    (k0, p0, h0, w0, s0), (k1, p1, h1, w1, s1) = states
    assert np.array_equal(k0, k1) and (p0, h0) == (p1, h1)
    assert np.abs(w0 - w1).max() <= 1e-15 and ulps(s0, s1).max() <= 4
    # selection order = Python's stable sort, reverse=True (evo/population.py:98-103), ties included
    rs = np.random.RandomState(4)
    fit = np.round(rs.uniform(0, 1, 3000), 2)   # many ties
    order = eng.ga_select(fit)
    want = [i for _, i in sorted(zip(fit.tolist(), range(len(fit))), key=lambda p: p[0], reverse=True)]
    assert order.tolist() == want
