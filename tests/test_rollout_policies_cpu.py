"""The per-individual rollout off the device: engine.Policies, the model (tests/policy_model.py) against the models of the
calls it generalises, game_log.behaviour_prob as a probability over the whole legal list, and the model through
game_log.logged_rollout."""
import os

import numpy as np
import pytest

import explore_model as X
import policy_model as P
import sample_model as S
from monsoon_amd import EXPERT, _lib, game_log
from monsoon_amd.cards import CARD_INDEX, deck_indices, needs_extended_each
from monsoon_amd.engine import _LOG_ENTRIES, LOG_ARRAYS, BatchEngine, Explore, Policies, RolloutLog, _log_arrays
from monsoon_amd.fitness import MATCH_DTYPE, hash32, hash32_array

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << 24
W4 = np.stack([np.random.RandomState(s).uniform(0, 1, 10) for s in (2024, 7, 11, 13)])   # four weight vectors
# the rows of a mixed table: greedy, uniform at 0.5, T = 1 at eps = 1, T = 0.25 at eps = 0.3
MIXED_EPS, MIXED_T = (0.0, 0.5, 1.0, 0.3), (1.0, np.inf, 1.0, 0.25)
T = 60


def _matches():
    """6 N12M matches over the four rows: different rows against each other, a self-match, the bot on either side."""
    m = np.zeros(6, dtype=MATCH_DTYPE)
    m["seed"] = hash32_array(61, np.arange(6), 0xE)
    m["p1"] = (0, 1, 2, 3, EXPERT, 3)
    m["p2"] = (1, 2, 3, 3, 2, EXPERT)
    return m, np.stack([deck_indices("N12M")] * 2)[None]


def _run(model, rule):
    m, pairs = _matches()
    counts, results, steps, log = model.rollout_logged(W4, m, pairs, T, explore=rule)
    return dict(counts=counts, results=results, steps=steps, log=log, finals=model.finals, games=model.games)


@pytest.fixture(scope="module")
def mixed():
    return _run(P.ModelEngine(), Policies(MIXED_EPS, MIXED_T, 5))


def test_policies_validation():
    p = Policies(MIXED_EPS, MIXED_T, 5, sides="second", until_step=3)
    assert p.samples is True and p.per_individual is True and len(p) == 4
    assert p.thresholds.dtype == np.uint32 and p.thresholds.tolist() == [0, 1 << 31, 0xFFFFFFFF, min(int(0.3 * 2**32), 0xFFFFFFFF)]
    assert p.thresholds.tolist() == [Explore(e, 5).threshold for e in MIXED_EPS]
    assert p.inv_temperatures.dtype == np.float64 and p.inv_temperatures.tolist() == [1.0, 0.0, 1.0, 4.0]
    assert p.may_explore(1, 2) and not p.may_explore(0, 2) and not p.may_explore(1, 3)
    assert np.array_equal(p.may_explore(np.array([0, 1, 1]), np.array([0, 0, 5])), [False, True, False])
    c = p.c_struct()
    assert (c.seed, c.sides, c.until_step) == (5, 2, 3) and c.threshold == p.thresholds.ctypes.data and c.inv_temperature == p.inv_temperatures.ctypes.data
    for eps in ([-0.1, 0.5], [0.5, 1.5], [np.nan, 0.5]):
        with pytest.raises(ValueError):
            Policies(eps, [1.0, 1.0], 1)
    for temp in ([0.0, 1.0], [-1.0, 1.0], [np.nan, 1.0], [5e-324, 1.0], [-np.inf, 1.0]):
        with pytest.raises(ValueError):
            Policies([0.5, 0.5], temp, 1)
    with pytest.raises(ValueError):
        Policies([0.5, 0.5], [1.0], 1)            # two lengths
    with pytest.raises(ValueError):
        Policies(0.5, 1.0, 1)                      # scalars are Explore's
    with pytest.raises(ValueError):
        Policies([0.5], [1.0], 1, sides="all")
    # the length mismatch is refused before the library is touched (the handle is never read)
    eng = BatchEngine.__new__(BatchEngine)
    m, pairs = _matches()
    with pytest.raises(ValueError, match=r"3 rows.*4\b"):
        eng.rollout_logged(W4, m, pairs, T, explore=Policies([0.5] * 3, [1.0] * 3, 1))


def test_entry_point_binding_and_header():
    assert _LOG_ENTRIES[-1] == "monsoon_rollout_policies" and not [a for a in LOG_ARRAYS if a[4] == "monsoon_rollout_policies"]
    assert _log_arrays("monsoon_rollout_policies") == _log_arrays("monsoon_rollout_sample")
    assert len(_lib.SIGNATURES["monsoon_rollout_policies"][1]) == len(_lib.SIGNATURES["monsoon_rollout_sample"][1])
    assert [f[0] for f in _lib.Policies._fields_] == ["seed", "sides", "until_step", "threshold", "inv_temperature"]
    assert (_lib.Policies.threshold.offset, _lib.Policies.inv_temperature.offset) == (16, 24)
    header = open(os.path.join(REPO, "include", "monsoon.h")).read()
    assert "int monsoon_rollout_policies(" in header and "} monsoon_policies;" in header
    assert "NaN or infinite best" in header and "WEIGHTS ON EVERY COVERED DECISION" in header


def test_equal_rows_play_the_sampling_models_games():
    """Every row at eps = 0.5, T = 1: sample_model's games array by array, except that the weights are also there on covered
    decisions that did not sample -- total as sample_weights gives it, 2**24 taken."""
    ref = _run(S.ModelEngine(), Explore(0.5, 5, temperature=1.0))
    got = _run(P.ModelEngine(), Policies([0.5] * 4, [1.0] * 4, 5))
    for key in ("counts", "results", "steps", "finals"):
        assert np.array_equal(got[key], ref[key]), key
    assert X.same_log(got["log"], ref["log"])
    a, b = got["log"], ref["log"]
    sampled, decision = a.explored != 0, a.n_legal > 0
    assert sampled.any() and (decision & ~sampled).any()
    assert np.array_equal(a.weight_total[sampled], b.weight_total[sampled]) and np.array_equal(a.taken_weight[sampled], b.taken_weight[sampled])
    assert not b.weight_total[~sampled].any()
    assert (a.weight_total[decision & ~sampled] >= ONE).all() and (a.taken_weight[decision & ~sampled] == ONE).all()
    assert not a.weight_total[~decision].any() and not a.taken_weight[~decision].any()
    for g in got["games"]:   # the unsampled totals are the weights' sums
        for k in range(g["steps"]):
            if g["covered"][k] and not g["explored"][k]:
                s = g["legal_scores"][k]
                assert g["weight_total"][k] == int(game_log.sample_weights(s, g["score"][k], 1.0).astype(np.uint64).sum())


def test_infinite_temperature_plays_the_exploring_models_games():
    """Every row at T = inf: explore_model's games (every score of these games is finite)."""
    ref = _run(X.ModelEngine(), Explore(0.5, 5))
    got = _run(P.ModelEngine(), Policies([0.5] * 4, [np.inf] * 4, 5))
    for key in ("counts", "results", "steps", "finals"):
        assert np.array_equal(got[key], ref[key]), key
    assert X.same_log(got["log"], ref["log"])
    a = got["log"]
    sampled = a.explored != 0
    assert sampled.any() and (a.action != a.greedy).any() and np.isfinite(a.score[a.n_legal > 0]).all()
    assert np.array_equal(a.weight_total[a.n_legal > 0], a.n_legal[a.n_legal > 0].astype(np.uint32) * ONE)
    assert (a.taken_weight[a.n_legal > 0] == ONE).all()
    ranks = [(g["rank"][k], r["rank"][k]) for g, r in zip(got["games"], ref["games"]) for k in range(g["steps"]) if g["explored"][k]]
    assert ranks and all(x == y for x, y in ranks)


def test_zero_eps_plays_the_logged_models_games():
    ref = _run(X.ModelEngine(), None)
    got = _run(P.ModelEngine(), Policies([0.0] * 4, MIXED_T, 5))
    for key in ("counts", "results", "steps", "finals"):
        assert np.array_equal(got[key], ref[key]), key
    a, b = got["log"], ref["log"]
    assert np.array_equal(a.action, b.action) and np.array_equal(a.n_legal, b.n_legal) and X._same_f64(a.score, b.score)
    decision = a.n_legal > 0
    assert np.array_equal(a.greedy[decision], a.action[decision]) and not a.explored.any()
    assert not a.weight_total.any() and not a.taken_weight.any()


def test_behaviour_prob_is_a_probability(mixed):
    """For every covered decision of the mixed run mu is rebuilt over the whole legal list from the model's scores: it sums to
    1 within 1e-12, and behaviour_prob's entry is the committed action's term.  Elsewhere: 1.0 on decisions, NaN on bot steps
    and padding."""
    pol = Policies(MIXED_EPS, MIXED_T, 5)
    m, _ = _matches()
    log, games = mixed["log"], mixed["games"]
    mu = game_log.behaviour_prob(pol, m, log, P.sides_of(games, log.action.shape))
    assert mu.dtype == np.float64 and mu.shape == log.action.shape
    covered = by_row = 0
    seen_rows = set()
    for i, g in enumerate(games):
        assert np.isnan(mu[i, g["steps"]:]).all()
        for k in range(g["steps"]):
            if g["bot"][k]:
                assert np.isnan(mu[i, k])
                continue
            assert g["row"][k] == (m["p1"][i] if g["side"][k] == 0 else m["p2"][i])
            if not g["covered"][k] or not g["weight_total"][k]:
                assert mu[i, k] == 1.0 and g["action"][k] == g["greedy"][k]
                continue
            r = g["row"][k]
            eps = int(pol.thresholds[r]) / 2.0**32
            w = game_log.sample_weights(g["legal_scores"][k], g["score"][k], pol.inv_temperatures[r]).astype(np.float64)
            full = eps * w / w.sum()
            full[g["greedy_rank"][k]] += 1.0 - eps
            assert abs(full.sum() - 1.0) <= 1e-12
            legal_rank = g["rank"][k] if g["rank"][k] >= 0 else g["greedy_rank"][k]
            assert abs(mu[i, k] - full[legal_rank]) <= 1e-15 and 0.0 < mu[i, k] <= 1.0
            covered += 1
            seen_rows.add(r)
            by_row += g["explored"][k]
    assert covered > 50 and by_row > 10 and seen_rows == {1, 2, 3}
    assert (mu[np.isfinite(mu)] <= 1.0).all() and (mu[np.isfinite(mu)] < 1.0).any()
    with pytest.raises(ValueError):
        game_log.behaviour_prob(Explore(0.5, 5, temperature=1.0), m, log, P.sides_of(games, log.action.shape))


def test_mixed_table_each_row_plays_its_own_rule(mixed):
    """The greedy row never leaves its arg-max and logs no weights; row 2 (eps = 1) samples on every decision; the uniform
    row's totals are n_legal * 2**24; the draws are hash32's."""
    m, _ = _matches()
    n_by_row = dict.fromkeys(range(4), 0)
    for i, g in enumerate(mixed["games"]):
        for k in range(g["steps"]):
            r = g["row"][k]
            if r < 0:
                continue
            n_by_row[r] += 1
            draw = hash32(5, int(m["seed"][i]), k, 0)
            if r == 0:
                assert not g["covered"][k] and g["weight_total"][k] == 0 and g["explored"][k] == 0 and g["action"][k] == g["greedy"][k]
            else:
                assert g["covered"][k] and g["explored"][k] == (draw < int(Policies(MIXED_EPS, MIXED_T, 5).thresholds[r]))
            if r == 1:
                assert g["weight_total"][k] == g["n_legal"][k] * ONE and g["taken_weight"][k] == ONE
            if r == 2:
                assert g["explored"][k] == 1
    assert all(v > 0 for v in n_by_row.values()), n_by_row


def test_model_through_the_tier_ladder():
    """One b005 / ua20 pair and one standard pair through game_log.logged_rollout on ModelEngines of tiers 0 and 1 with the mixed
    table: the sub-schedules keep their row indices, so every game is the game its own single-match run plays."""
    std = deck_indices("N12M")
    a, b = std.copy(), std.copy()
    a[0], b[1] = CARD_INDEX["ua20"], CARD_INDEX["b005"]
    pairs = np.stack([np.stack([std, std]), np.stack([a, b])])
    assert np.array_equal(needs_extended_each(pairs), [False, True])
    m = np.zeros(4, dtype=MATCH_DTYPE)
    m["seed"], m["p1"], m["p2"], m["deck"] = hash32_array(62, np.arange(4), 0xE), (1, 3, 2, 0), (3, 2, 1, 3), (0, 1, 0, 1)
    pol = Policies(MIXED_EPS, MIXED_T, 8)
    engines = {}
    counts, results, steps, faults, log = game_log.logged_rollout(lambda t: engines.setdefault(t, P.ModelEngine(t)), W4, m, pairs, T, pol)
    assert set(engines) >= {0, 1} and counts[:, 2].sum() == 4 and (steps > 0).all()
    assert log.weight_total is not None and log.weight_total.any() and (log.explored != 0).any()
    for i in range(4):
        if faults[i] >= 16:   # (played again on a larger record)
            continue
        one = m[i:i + 1].copy()
        one["deck"] = 0
        _, _, s1, lg1 = P.ModelEngine(int(m["deck"][i])).rollout_logged(W4, one, pairs[m["deck"][i]][None], T, explore=pol)
        assert s1[0] == steps[i]
        for c in ("action", "greedy", "explored", "weight_total", "taken_weight"):
            assert np.array_equal(getattr(lg1, c)[0], getattr(log, c)[i]), (i, c)
