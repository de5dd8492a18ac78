"""The device's features and hot-kernel scores against the independent model of tests/heuristic_model.py (run with
-m gpu on an MI355X): monsoon_features at full batch size on every record build, monsoon_decide's score vectors over a
spread of weight vectors and on hand-made edge states, and every hot-kernel instantiation of variants.def."""
import copy
import json

import numpy as np
import pytest

import heuristic_model as HM
import kernel_variants
import oracle_lib
from monsoon_amd.cards import CARD_INDEX, UNSUPPORTED, deck_indices, observable_pool

pytestmark = pytest.mark.gpu

NAMES = kernel_variants.BUILD_NAMES
W0 = np.random.RandomState(2024).uniform(0, 1, 10)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _pool(ext):
    pool = observable_pool()
    if not ext:
        pool = np.array([c for c in pool if c not in {CARD_INDEX[x] for x in UNSUPPORTED}], dtype=np.uint8)
    return pool


def _legal_bits(masks):
    return np.unpackbits(np.ascontiguousarray(masks).view(np.uint8).reshape(len(masks), 24), axis=1, bitorder="little")[:, :156].astype(bool)


def _random_actions(eng, rs):
    """A uniformly random legal action for every game that has one and has not faulted, else 255 (skip)."""
    legal = _legal_bits(eng.legal_mask())
    keys = rs.random_sample(legal.shape)
    keys[~legal] = -1.0
    acts = keys.argmax(axis=1).astype(np.uint8)
    acts[~legal.any(axis=1) | (eng.game_faults() != 0)] = 255
    return acts


def _weight_set():
    """The weight vectors the score tests use, with names."""
    rs = np.random.RandomState(77)
    ws = [("uniform", rs.uniform(0, 1, 10)), ("uniform", rs.uniform(0, 1, 10))]
    for _ in range(2):   # GA-shaped: Gaussian steps clipped to [0, 1] (Population's mutation), exact 0.0 and 1.0 entries
        v = np.clip(rs.uniform(0, 1, 10) + rs.normal(0, 0.6, 10), 0.0, 1.0)
        v[rs.randint(10)], v[rs.randint(10)] = 0.0, 1.0
        ws.append(("ga", v))
    ws.append(("zero", np.zeros(10)))
    for i in range(10):
        ws.append((f"onehot{i}", np.eye(10)[i]))
    ws.append(("signed", rs.uniform(-1, 1, 10)))
    ws.append(("signed", rs.normal(0, 3, 10)))
    ws.append(("tiny", rs.uniform(0, 1, 10) * 1e-300))
    ws.append(("subnormal", rs.uniform(-1, 1, 10) * 1e-308))   # the products are subnormal
    return ws


def _check_decisions(src, idxs, weights, ext, tally, cache):
    """monsoon_decide's complete score vector, best score and action for games idxs of handle src under every weight
    vector, against the model: one clone per legal action (save_state / load_state into a second handle) is stepped and
    observed, and the model scores it.  A successor that faults or whose observation raises scores 0.0; every action
    scores 0.0 when the current observation raises; NaN marks exactly the illegal actions.  A game that already has a
    winner is not decided (action 255, no scores), as the reference's game loop never asks its agent."""
    from monsoon_amd.engine import BatchEngine
    idxs = [int(i) for i in idxs]
    legal = _legal_bits(src.legal_mask()[idxs])
    obs, raises = src.observe()
    obs, raises = obs[idxs], raises[idxs]
    live = src.game_faults()[idxs] == 0
    over = src.status()[idxs, 1] != 0
    keep = [j for j in range(len(idxs)) if legal[j].any() and live[j] and not over[j]]
    ended = [j for j in range(len(idxs)) if live[j] and over[j]]
    blobs = {j: src.save_state(idxs[j]) for j in keep + ended}
    cand = [(j, int(a)) for j in keep for a in np.nonzero(legal[j])[0]]
    cl = BatchEngine(len(cand), extended=ext)
    for j, _ in cand:
        cl.load_state(cl.n, blobs[j])
    _, _, cfault = cl.step(np.array([a for _, a in cand], dtype=np.uint8))
    cobs, craises = cl.observe()
    cl.close()
    after = HM.features(cobs)
    before = HM.features(obs)
    limit = {j for (j, _), f in zip(cand, cfault) if f >= 16}   # a limit of this build: no reference behaviour to model
    succ = {}
    for (j, a), f, r, x in zip(cand, cfault, craises, after):
        succ[(j, a)] = None if (f != 0 or r) else x
    games = [j for j in keep if j not in limit]
    slots = [(j, v) for j in games for v in range(len(weights))] + [(j, 0) for j in ended]
    dh = BatchEngine(max(1, len(slots)), extended=ext)
    wt = np.zeros((len(slots), 2, 10))
    for s, (j, v) in enumerate(slots):
        wt[s] = weights[v][1]
        dh.load_state(dh.n, blobs[j])
    action, best, scores = dh.decide(wt, want_scores=True) if slots else (None, None, None)
    dh.close()
    for s, (j, v) in enumerate(slots):
        if over[j]:
            assert action[s] == 255 and np.isnan(scores[s]).all(), j
            continue
        w = weights[v][1]
        acts = np.nonzero(legal[j])[0]
        assert np.array_equal(np.isnan(scores[s]), ~legal[j]), (j, v)
        if raises[j]:
            want = [0.0] * len(acts)
        else:
            want = [0.0 if succ[(j, int(a))] is None else cache(w, before[j], succ[(j, int(a))]) for a in acts]
        got = scores[s][acts]
        assert np.array_equal(_bits(got), _bits(want)), (weights[v][0], j, [(int(a), x, y) for a, x, y in zip(acts, got, want) if _bits(x) != _bits(y)][:4])
        b = HM.first_max(want)
        assert action[s] == acts[b] and _bits(best[s]) == _bits(want[b]), (weights[v][0], j, action[s], acts[b])
    tally["games"] += len(games)
    tally["scores"] += sum(int(legal[j].sum()) for j, _ in slots if not over[j])
    tally["over"] += len(ended)
    tally["limit"] += len(limit)
    tally["raising"] += int(sum(raises[j] for j in games))
    tally["zero_successors"] += sum(1 for (j, a), x in succ.items() if x is None and j in games)


# ---- monsoon_features at scale ---------------------------------------------------------------------------------

@pytest.mark.parametrize("ext,n", [(False, 65536), (True, 65536), (2, 4096)], ids=["standard", "extended", "large"])
def test_features_at_scale_equal_the_model(ext, n):
    """n games on pool decks of the build, a random legal policy for 48 steps; monsoon_observe and monsoon_features at
    every step: the model on the device's observation equals the device's features bit for bit, and the row is all NaN
    exactly where the observation raises."""
    from monsoon_amd.engine import BatchEngine
    eng = BatchEngine(n, extended=ext)
    rs = np.random.RandomState(4242 + int(ext))
    seeds = (np.arange(n) + 310000).astype(np.uint32)
    eng.reset(seeds, eng.draw_decks(seeds ^ np.uint32(0x5BD1E995), _pool(ext)))
    rows = nan_rows = 0
    for t in range(49):
        if t:
            eng.step(_random_actions(eng, rs))
        obs, raises = eng.observe()
        feat = eng.features()
        ok = eng.game_faults() == 0   # a game stopped by a fault is left mid-step
        r = raises.astype(bool) & ok
        assert np.isnan(feat[r]).all()
        m = ok & ~r
        got = HM.features(obs[m])
        assert not np.isnan(feat[m]).any()
        bad = np.nonzero((_bits(got) != _bits(feat[m])).any(axis=1))[0]
        assert len(bad) == 0, (t, len(bad), obs[m][bad[0]].tolist(), feat[m][bad[0]], got[bad[0]])
        rows += int(m.sum())
        nan_rows += int(r.sum())
    eng.close()
    print(f"{NAMES[ext]}: {rows} device feature rows equal the model, {nan_rows} NaN rows where the observation raises")
    assert rows > 40 * n * 0.5


# ---- hot-kernel scores -----------------------------------------------------------------------------------------

def _decision_states(ext, n, seed, steps=(0, 5, 14)):
    """A handle with n random-policy games on pool decks, yielded at the given step counts."""
    from monsoon_amd.engine import BatchEngine
    eng = BatchEngine(n, extended=ext)
    rs = np.random.RandomState(seed)
    seeds = (np.arange(n) + seed).astype(np.uint32)
    eng.reset(seeds, eng.draw_decks(seeds, _pool(ext)))
    t = 0
    for s in steps:
        while t < s:
            eng.step(_random_actions(eng, rs))
            t += 1
        yield eng
    eng.close()


@pytest.mark.parametrize("ext,n", [(False, 256), (True, 256), (2, 96)], ids=["standard", "extended", "large"])
def test_decide_scores_equal_the_model(ext, n):
    """monsoon_decide(want_scores) at three decision points of n games, under uniform, GA-shaped (exact 0.0 / 1.0
    entries), all-zero (every decision a tie), one-hot, signed, tiny and subnormal weight vectors: every legal score, the
    NaNs, the action and the best score equal the model's."""
    weights = _weight_set()
    tally = dict(games=0, scores=0, limit=0, raising=0, zero_successors=0, over=0)
    cache = HM.ScoreCache()
    for eng in _decision_states(ext, n, 5100 + int(ext)):
        _check_decisions(eng, range(eng.n), weights, ext, tally, cache)
    print(f"{NAMES[ext]}: {tally['scores']} candidate scores of {tally['games']} decisions x {len(weights)} weight vectors "
          f"equal the model ({tally['raising']} decisions whose observation raises, {tally['zero_successors']} successors "
          f"that fault or raise, {tally['limit']} decisions skipped at a build limit)")
    assert tally["games"] >= n * 2 and tally["limit"] <= n // 20


# ---- edge states -----------------------------------------------------------------------------------------------

def _edge_states():
    """Scenario states (tests/golden/scenarios.json.gz) mutated towards the edges of the feature formulas."""
    import scenario_lib as S
    ext_cards = [CARD_INDEX["ua20"], CARD_INDEX["b005"]]
    # the extended cards stay out; a card object listed twice (needs_extended's other reason) gets objects of its own below
    recs = [r for case in S.load() for r in case["records"]
            if not any(f'"card": {c},' in s or f'"card": {c}}}' in s for s in [json.dumps(r)] for c in ext_cards)
            and r["before"]["phase"] == 1 and not r["before"]["resolving"] and not r["before"]["triggers"]]
    bases = recs[::max(1, len(recs) // 12)][:12]
    unit = next(t for r in recs for t in r["before"]["tiles"] if t and t["kind"] == "unit" and not t.get("memory"))
    struct = next(t for r in recs for t in r["before"]["tiles"] if t and t["kind"] == "structure" and not t.get("memory"))

    def put(st, t, tmpl, owner, strength=None):
        e = copy.deepcopy(tmpl)
        e["owner"], e["position"], e["path"] = owner, [t % 4, t // 4], []
        if strength is not None:
            e["strength"] = strength
        st["tiles"][t] = e

    def move_deck_to_hand(p, k, pick=lambda c: True):
        for c in [c for c in p["deck"] if pick(c)][:k]:
            p["deck"].remove(c)
            p["hand"].append(c)

    muts = []
    for who in (0, 1):
        for v in (-1, 0):
            muts.append((f"base{who}={v}", lambda st, who=who, v=v: st["players"][who].__setitem__("base", v)))
    for v in (0, 7, 8, 10, 13):
        muts.append((f"mana={v}", lambda st, v=v: [p.update(mana=v, max_mana=max(v, p["max_mana"])) for p in st["players"]]))

    def hand3(st):
        for p in st["players"]:
            move_deck_to_hand(p, max(0, 3 - len(p["hand"])))
            p["deck"] = p["hand"][3:] + p["deck"]
            p["hand"] = p["hand"][:3]
    muts.append(("hand3", hand3))
    muts.append(("zero_cost", lambda st: [c.update(cost=0) for p in st["players"] for c in p["hand"]]))

    def spells_only(st):
        for p in st["players"]:
            p["deck"] = [c for c in p["hand"] if c["kind"] != "spell"] + p["deck"]
            p["hand"] = [c for c in p["hand"] if c["kind"] == "spell"]
            move_deck_to_hand(p, 4 - len(p["hand"]), lambda c: c["kind"] == "spell")
    muts.append(("spells_only", spells_only))
    muts.append(("hand5", lambda st: [move_deck_to_hand(p, 5 - len(p["hand"])) for p in st["players"]]))   # HAND_CAP
    muts.append(("empty_board", lambda st: st.__setitem__("tiles", [None] * 20)))

    def full_board(st):
        for t in range(20):
            if st["tiles"][t] is None:
                put(st, t, unit if t % 3 else struct, t % 2)
    muts.append(("full_board", full_board))

    def structures_only(st):
        st["tiles"] = [x if x and x["kind"] == "structure" else None for x in st["tiles"]]
        for t in (1, 6, 13):
            put(st, t, struct, t % 2)
    muts.append(("structures_only", structures_only))

    def enemy_row4(st):
        for t in (16, 17, 18, 19):
            put(st, t, unit, 1 - st["cp"], 3)
    muts.append(("enemy_row4", enemy_row4))

    def thirds(st):   # board strength 2 : 1 (ratio 1/3), 5 : 2 (3/7); hand values 7/3, 5/6
        st["tiles"] = [None] * 20
        me = st["cp"]
        put(st, 5, unit, me, 2)
        put(st, 10, unit, 1 - me, 1)
        put(st, 14, struct, me, 3)
        put(st, 2, unit, 1 - me, 1)
        for p in st["players"]:
            for c, (s, k) in zip([c for c in p["hand"] if c["kind"] != "spell"], [(7, 3), (5, 6), (1, 7)]):
                c.update(strength=s, cost=k)
    muts.append(("thirds", thirds))
    out = []
    for r in bases:
        for name, f in muts:
            st = copy.deepcopy(r["before"])
            f(st)
            for p in st["players"]:
                for k, c in enumerate(p["hand"] + p["deck"]):
                    c["oid"] = k
            out.append((name, st))
    return out


@pytest.mark.parametrize("ext", [False, True], ids=["standard", "extended"])
def test_edge_states_equal_the_model(ext):
    """Scenario states pushed to the edges of the formulas (bases at -1 and 0; mana 0, 7, 8, 10, 13; three cards, zero-cost
    cards, spells only and five cards in hand; empty, full, structures-only boards, enemy units on row 4; strength ratios
    that do not terminate in binary): monsoon_features and monsoon_decide's scores equal the model."""
    import scenario_lib as S
    from monsoon_amd._lib import MonsoonError
    from monsoon_amd.engine import BatchEngine
    states = _edge_states()
    probe = BatchEngine(1, extended=ext)   # a state the record cannot hold never reaches the handle under test
    good = []
    for name, st in states:
        try:
            if probe.debug_build(0, st["seed"], st["stream_pos"], S.encode_state(st)) == 0:
                good.append((name, st))
        except MonsoonError:
            pass
    probe.close()
    names = {name for name, _ in good}
    eng = BatchEngine(len(good), extended=ext)
    for name, st in good:
        assert eng.debug_build(eng.n, st["seed"], st["stream_pos"], S.encode_state(st)) == 0, name
    assert len(good) >= len(states) // 2 and len(names) == 18, (len(good), len(states), sorted(names))
    obs, raises = eng.observe()
    feat = eng.features()
    ok = ~raises.astype(bool)
    assert np.isnan(feat[~ok]).all()
    assert np.array_equal(_bits(HM.features(obs[ok])), _bits(feat[ok]))
    weights = [x for x in _weight_set() if x[0] in ("uniform", "ga", "zero", "signed", "subnormal")]
    tally = dict(games=0, scores=0, limit=0, raising=0, zero_successors=0, over=0)
    _check_decisions(eng, range(eng.n), weights, ext, tally, HM.ScoreCache())
    eng.close()
    print(f"{NAMES[ext]}: {len(good)} of {len(states)} edge states built ({len(names)} kinds), {int(ok.sum())} feature "
          f"rows and {tally['scores']} candidate scores equal the model ({tally['over']} states with a winner not decided, "
          f"{tally['raising']} whose observation raises, {tally['limit']} skipped at a build limit)")
    assert tally["games"] >= len(good) // 2


# ---- every hot-kernel instantiation ----------------------------------------------------------------------------

VARIANTS, VARIANT_IDS = kernel_variants.matrix()
_ORACLE_ROLLOUTS = {}


def _rollout_games(ext):
    n = 2048
    m = np.zeros(n, dtype=[("p1", "<i4"), ("p2", "<i4"), ("seed", "<u4"), ("deck", "<u4")])
    if ext is False:   # N12M mirror
        deck = deck_indices("N12M")
        m["seed"] = np.arange(n) + 100000
        pairs = np.stack([deck, deck])[None]
    else:              # every game its own pool decks
        rs = np.random.RandomState(61 + int(ext))
        pool = _pool(ext)
        pairs = np.stack([np.stack([rs.choice(pool, 12, replace=False), rs.choice(pool, 12, replace=False)]) for _ in range(n)])
        m["seed"] = np.arange(n) + 120000
        m["deck"] = np.arange(n)
    return m, pairs


def _oracle_rollouts(ext):
    if ext not in _ORACLE_ROLLOUTS:
        m, pairs = _rollout_games(ext)
        n = len(m)
        orc = oracle_lib.Oracle(n, extended=ext)
        for g in range(n):
            p = pairs[m["deck"][g]]
            assert orc.reset(g, int(m["seed"][g]), p[0], p[1]) == 0
        total, res, steps, hashes = orc.rollout_batch(n, W0, 200, 16)
        faults = np.array([orc.game_fault(g) for g in range(n)])
        # a game stopped at a limit of the record (fault >= 16) is left mid-step, where the oracle's recursive rules core
        # and the library's explicit work stack stop at different points: its final state is the one the host build of
        # the library's own core reaches
        limit = faults >= 16
        if limit.any():
            prod = oracle_lib.Oracle(n, extended=ext, core="product")
            for g in range(n):
                p = pairs[m["deck"][g]]
                assert prod.reset(g, int(m["seed"][g]), p[0], p[1]) == 0
            ptotal, pres, psteps, phashes = prod.rollout_batch(n, W0, 200, 16)
            assert ptotal == total and np.array_equal(pres, res) and np.array_equal(psteps, steps)
            assert np.array_equal(phashes[~limit], hashes[~limit])
            hashes = np.where(limit, phashes, hashes)
        _ORACLE_ROLLOUTS[ext] = (total, res, steps, hashes, faults)
    return _ORACLE_ROLLOUTS[ext]


def _handle(monkeypatch, ext, n, uw):
    """A handle of variant uw = (U, W), or of the build's default with uw = None."""
    from monsoon_amd.engine import BatchEngine
    if uw is None:
        monkeypatch.delenv("MONSOON_LANES", raising=False)
        monkeypatch.delenv("MONSOON_WPE", raising=False)
    else:
        kernel_variants.select(monkeypatch, *uw)
    return BatchEngine(n, extended=ext)


@pytest.mark.parametrize("ext,u,w", VARIANTS, ids=VARIANT_IDS)
def test_every_kernel_variant_equals_the_oracle_and_its_default(monkeypatch, ext, u, w):
    """Each (U, W) of variants.def, selected with MONSOON_LANES / MONSOON_WPE: (b) 2 048 games played to the end equal
    the oracle on the same record -- results, decisions, final states, fault codes, look-ahead transitions (the final
    state of a game stopped at a record limit: that of the host build of the library's rules core); (c) decide's
    score vectors under the zero and signed weights equal, bit for bit, those of the build's default variant."""
    eng = _handle(monkeypatch, ext, 2048, (u, w))
    try:
        assert eng.variant() == (u, w)
        # (b)
        m, pairs = _rollout_games(ext)
        eng.reset_stats()
        _, results, steps = eng.rollout(W0[None], m, pairs, 200, want_results=True)
        total, ores, osteps, ohash, ofault = _oracle_rollouts(ext)
        assert np.array_equal(results, ores) and np.array_equal(steps, osteps)
        assert np.array_equal(eng.state_hash(), ohash)
        assert np.array_equal(eng.rollout_faults(len(m)), ofault)
        assert eng.stats()["lookahead_steps"] == total
    finally:
        eng.close()
    # (c)
    ws = [x[1] for x in _weight_set() if x[0] in ("zero", "signed")]
    n_cmp = 0
    for src in _decision_states(ext, 128, 8800 + int(ext), steps=(0, 9)):
        live = [i for i in range(src.n) if src.game_faults()[i] == 0 and src.legal_mask()[i].any()]
        blobs = [src.save_state(i) for i in live]
        wt = np.array([ws[k % len(ws)] for k in range(len(live))])[:, None, :].repeat(2, axis=1)
        out = []
        for uw in (None, (u, w)):   # a fresh handle of the default variant, then of the variant under test
            h = _handle(monkeypatch, ext, len(live), uw)
            assert h.variant() == (uw or kernel_variants.variants(ext)[0])
            for b in blobs:
                h.load_state(h.n, b)
            out.append(h.decide(wt, want_scores=True))
            h.close()
        (a0, b0, s0), (a1, b1, s1) = out
        assert np.array_equal(a0, a1) and np.array_equal(_bits(b0), _bits(b1))
        assert np.array_equal(np.isnan(s0), np.isnan(s1))
        assert np.array_equal(_bits(np.nan_to_num(s0)), _bits(np.nan_to_num(s1)))
        n_cmp += int((~np.isnan(s0)).sum())
    print(f"variant {NAMES[ext]} ({u}, {w}): 2048 rollouts equal the oracle, {n_cmp} scores equal the default's")
