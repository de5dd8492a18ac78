"""monsoon_rollout_policies on the device (k_play_policy): a mixed table entry by entry against the model over the CPU oracle
(tests/policy_model.py) on the three record builds, with the places the kernel can go wrong counted from the model's own
log; against monsoon_rollout_sample, monsoon_rollout_explore and monsoon_rollout_logged where the table says what those
calls say; batches, sides and the step limit, the dataset columns and the behaviour probability, and what is refused."""
import ctypes

import numpy as np
import pytest

import policy_model as P
import sample_model as S
from monsoon_amd import EXPERT, _lib, game_log
from monsoon_amd.cards import C5_STREAM_XOR, CARD_INDEX, deck_indices, draw_random_decks_numpy, needs_extended_each
from monsoon_amd.engine import BatchEngine, Explore, Policies, RolloutLog, _ptr
from monsoon_amd.fitness import MATCH_DTYPE, hash32_array

pytestmark = pytest.mark.gpu

ONE = 1 << 24
W4 = np.stack([np.random.RandomState(s).uniform(0, 1, 10) for s in (2024, 7, 11, 13)])   # four weight rows
U = 8   # candidate lanes per pass of every build's default variant (variants.def)
# the mixed table: row 0 greedy, row 1 uniform at 0.5, row 2 T = 1 at eps = 1, row 3 T = 0.25 at eps = 0.3
MIXED_EPS, MIXED_T = (0.0, 0.5, 1.0, 0.3), (1.0, np.inf, 1.0, 0.25)
SEED0, RULE_SEED = 21, 9   # of the standard set: chosen on the CPU model so that it alone meets every count of the reach test


def _schedule(n, seed0=0):
    """n matches over the four rows of W4: a third each of bot-FIRST, bot-SECOND and plain; a plain match pairs two different
    rows (every ordered pair comes up), except match 5, which plays row 1 against itself; row 3 plays from match 3 on."""
    m = np.zeros(n, dtype=MATCH_DTYPE)
    k = np.arange(n)
    row, third = k % 4, k % 3
    other = (row + 1 + (k // 12) % 3) % 4
    other[5:6] = row[5:6]
    m["seed"] = hash32_array(seed0, k, 0xE)
    m["p1"] = np.where(third == 0, EXPERT, row)
    m["p2"] = np.where(third == 1, EXPERT, np.where(third == 0, row, other))
    return m


def _n12m():
    d = deck_indices("N12M")
    return np.stack([d, d])[None]


def _standard_set(seed0=SEED0):
    """48 mixed matches: the even ones on N12M, the odd ones on random 109-card pairs the standard record holds."""
    n = 48
    m = _schedule(n, seed0=seed0)
    drawn = draw_random_decks_numpy(hash32_array(77, np.arange(4 * n)) ^ np.uint32(C5_STREAM_XOR))
    drawn = drawn[~needs_extended_each(drawn)][:n // 2]
    assert len(drawn) == n // 2
    pairs = np.concatenate([_n12m(), drawn])
    m["deck"] = np.where(np.arange(n) % 2 == 0, 0, 1 + np.arange(n) // 2)
    return m, pairs


def _mixed(seed, **how):
    return Policies(MIXED_EPS, MIXED_T, seed, **how)


def _engine(max_games=64, build=0):
    """A handle; torch loads its runtime before the library does (VecEnv.__init__ says why), for the sake of dataset."""
    import torch
    assert torch.cuda.is_available()
    return BatchEngine(max_games, extended=build)


def _device(build, cap, m, pairs, T, rule):
    eng = _engine(cap, build)
    assert eng.variant()[0] == U
    counts, results, steps, log = eng.rollout_logged(W4, m, pairs, T, explore=rule)
    out = dict(counts=counts, results=results, steps=steps, log=log, faults=eng.rollout_faults(len(m)), hashes=eng.state_hash(), n=eng.n,
               stats=eng.stats())
    eng.close()
    return out


def _model(build, m, pairs, T, pol):
    model = P.ModelEngine(build)
    counts, results, steps, log = model.rollout_logged(W4, m, pairs, T, explore=pol)
    return dict(counts=counts, results=results, steps=steps, log=log, faults=model.rollout_faults(len(m)), finals=model.finals,
                games=model.games)


def _assert_equals_model(dev, ref, last_batch_from=0, min_clean=0.7):
    assert np.array_equal(dev["steps"], ref["steps"]) and np.array_equal(dev["results"], ref["results"])
    assert np.array_equal(dev["counts"], ref["counts"]) and np.array_equal(dev["faults"], ref["faults"])
    for c in ("action", "n_legal", "greedy", "explored", "weight_total", "taken_weight"):
        assert np.array_equal(getattr(dev["log"], c), getattr(ref["log"], c)), c
    assert S.same_log(dev["log"], ref["log"])   # (score and taken_score bit for bit among them)
    ok = ref["faults"][last_batch_from:] == 0   # (behind a faulting step the kernel and the oracle stop at different points)
    assert ok.sum() >= min_clean * len(ok) and np.array_equal(dev["hashes"][ok], ref["finals"][last_batch_from:][ok])
    assert dev["stats"]["decisions"] == sum(g["decisions"] for g in ref["games"])
    assert dev["stats"]["lookahead_steps"] == sum(g["lookahead"] for g in ref["games"])


def reach(games, n_faultless):
    """The places the kernel can go wrong, counted from the model's games alone."""
    seen = dict.fromkeys(("both_sides_different_rows", "row1_sampled", "row2_sampled", "row3_sampled", "unsampled_total_above_one",
                          "greedy_row_next_to_sampled", "later_pass", "third_pass", "last_of_partial", "tie", "zero_weight", "one_legal",
                          "uniform_pick"), 0)
    for g in games:
        n = g["steps"]
        picked = [g["rank"][k] >= 0 for k in range(n)]
        first = {g["row"][k] for k in range(n) if picked[k] and g["side"][k] == 0}
        second = {g["row"][k] for k in range(n) if picked[k] and g["side"][k] == 1}
        seen["both_sides_different_rows"] += any(a != b for a in first for b in second)
        for k in range(n):
            if g["bot"][k]:
                continue
            r, nl = g["rank"][k], g["n_legal"][k]
            if g["row"][k] == 0:
                seen["greedy_row_next_to_sampled"] += (k > 0 and picked[k - 1]) or (k + 1 < n and picked[k + 1])
            if g["covered"][k] and not g["explored"][k]:
                seen["unsampled_total_above_one"] += g["weight_total"][k] > ONE
            if g["covered"][k] and g["weight_total"][k]:   # (weighed: the scan ran over these weights, drawn or not)
                seen["zero_weight"] += g["zero_weight"][k]
                seen["tie"] += g["tie"][k]
            if r < 0:
                continue
            seen[f"row{g['row'][k]}_sampled"] += 1
            seen["uniform_pick"] += g["row"][k] == 1
            seen["later_pass"] += r >= U
            seen["third_pass"] += r >= 2 * U
            seen["last_of_partial"] += r == nl - 1 and nl % U != 0 and nl > 1
            seen["one_legal"] += nl == 1
    seen["faultless_games"] = int(n_faultless)
    return seen


@pytest.fixture(scope="module")
def standard():
    """The standard set under the mixed table, by the model and by a 64-game handle: computed once, read by several tests."""
    m, pairs = _standard_set()
    pol, T = _mixed(RULE_SEED), 200
    return m, pairs, pol, T, _model(0, m, pairs, T, pol), _device(0, 64, m, pairs, T, pol)


def test_the_standard_set_reaches_every_place_the_kernel_can_go_wrong(standard):
    ref = standard[4]
    seen = reach(ref["games"], (ref["faults"] == 0).sum())
    print(seen)
    assert all(v > 0 for v in seen.values()), seen
    assert seen["faultless_games"] >= 0.7 * 48
    m = standard[0]
    plain = (m["p1"] >= 0) & (m["p2"] >= 0)
    assert (m["p1"][plain] == m["p2"][plain]).sum() == 1 and (m["p1"] == 3).any() and (m["p2"] == 3).any()
    assert (m["p1"] < 0).any() and (m["p2"] < 0).any()


def test_device_log_equals_model_log_standard(standard):
    m, pairs, pol, T, ref, dev = standard
    _assert_equals_model(dev, ref)
    log = dev["log"]
    sampled, decision = log.explored != 0, log.n_legal > 0
    assert sampled.any() and (log.greedy != log.action).any() and np.isnan(log.taken_score[log.action != 255]).any()
    assert (decision & ~sampled & (log.weight_total > ONE) & (log.taken_weight == ONE)).any()   # an unsampled covered decision
    assert (decision & (log.weight_total == 0)).any()                                            # the greedy row's
    assert (log.taken_weight <= log.weight_total).all() and not log.weight_total[~decision].any()
    assert (log.taken_score[decision] <= log.score[decision]).all()


def test_device_log_equals_model_log_extended():
    """8 matches with ua20 / b005 on a side, on the extended build."""
    n, T = 8, 120
    m = _schedule(n, seed0=31)
    std = deck_indices("N12M")
    a, b = std.copy(), std.copy()
    a[0], b[1] = CARD_INDEX["ua20"], CARD_INDEX["b005"]
    pairs = np.stack([np.stack([a, b]), np.stack([b, a])])
    assert needs_extended_each(pairs).all()
    m["deck"] = np.arange(n) % 2
    pol = _mixed(10)
    ref = _model(1, m, pairs, T, pol)
    assert any((np.array(g["rank"]) >= U).any() for g in ref["games"])
    _assert_equals_model(_device(1, 64, m, pairs, T, pol), ref)


def test_device_log_equals_model_log_large():
    """4 matches on the large build."""
    n, T = 4, 120
    m, pairs = _schedule(n, seed0=32), _n12m()
    pol = _mixed(11)
    ref = _model(2, m, pairs, T, pol)
    assert any((np.array(g["rank"]) >= U).any() for g in ref["games"])
    _assert_equals_model(_device(2, 64, m, pairs, T, pol), ref)


def _same_games(a, b):
    for key in ("counts", "results", "steps", "faults", "hashes"):
        assert np.array_equal(a[key], b[key]), key
    assert a["stats"] == b["stats"]


def test_equal_rows_equal_the_sampling_call():
    """64 N12M matches, every row at eps = 0.5, T = 1: monsoon_rollout_sample's games, hashes and statistics; the weights are
    that call's where it sampled, and total >= 2**24 with 2**24 taken on the decisions it left without."""
    n, T = 64, 200
    m, pairs = _schedule(n, seed0=35), _n12m()
    ref = _device(0, 64, m, pairs, T, Explore(0.5, 14, temperature=1.0))
    got = _device(0, 64, m, pairs, T, Policies([0.5] * 4, [1.0] * 4, 14))
    _same_games(got, ref)
    a, b = got["log"], ref["log"]
    assert P.X.same_log(a, b)
    sampled, decision = a.explored != 0, a.n_legal > 0
    assert sampled.any() and (decision & ~sampled).any()
    assert np.array_equal(a.weight_total[sampled], b.weight_total[sampled]) and np.array_equal(a.taken_weight[sampled], b.taken_weight[sampled])
    assert (a.weight_total[decision & ~sampled] >= ONE).all() and (a.taken_weight[decision & ~sampled] == ONE).all()
    assert not a.weight_total[~decision].any() and not a.taken_weight[~decision].any()


def test_zero_inverse_temperature_equals_the_exploring_call():
    """64 N12M matches, every row at T = inf: monsoon_rollout_explore's action, greedy, explored, taken_score, results and
    hashes (every decision's score is finite, so no decision falls back to its arg-max)."""
    n, T = 64, 200
    m, pairs = _schedule(n, seed0=36), _n12m()
    ref = _device(0, 64, m, pairs, T, Explore(0.5, 15))
    got = _device(0, 64, m, pairs, T, Policies([0.5] * 4, [np.inf] * 4, 15))
    a, b = got["log"], ref["log"]
    decision = b.n_legal > 0
    assert np.isfinite(b.score[decision]).all() and np.isfinite(b.taken_score[decision]).all()
    _same_games(got, ref)
    assert P.X.same_log(a, b) and (a.explored != 0).any() and (a.action != a.greedy).any()
    assert np.array_equal(a.weight_total[decision], a.n_legal[decision].astype(np.uint32) * ONE) and (a.taken_weight[decision] == ONE).all()


def test_zero_thresholds_equal_the_logged_call():
    """64 N12M matches, every threshold 0: monsoon_rollout_logged bit for bit, the padding included; greedy = action, explored
    = 0, taken_score = score on decisions, both weights 0."""
    n, T = 64, 200
    m, pairs = _schedule(n, seed0=37), _n12m()
    ref = _device(0, 64, m, pairs, T, None)
    got = _device(0, 64, m, pairs, T, Policies([0.0] * 4, MIXED_T, 16))
    _same_games(got, ref)
    zl, log = got["log"], ref["log"]
    decision = log.n_legal > 0
    assert (log.steps > 0).all() and decision.any() and np.isnan(log.score[log.action != 255]).any()
    assert np.array_equal(zl.action, log.action) and np.array_equal(zl.n_legal, log.n_legal)
    assert np.array_equal(zl.score.view(np.uint64), log.score.view(np.uint64))   # the padding's bits too
    assert np.array_equal(zl.greedy[decision], log.action[decision]) and (zl.greedy[~decision] == 255).all()
    assert not zl.explored.any()
    assert np.array_equal(zl.taken_score[decision].view(np.uint64), log.score[decision].view(np.uint64))
    assert np.isnan(zl.taken_score[~decision]).all()
    assert zl.weight_total.dtype == np.uint32 and not zl.weight_total.any() and not zl.taken_weight.any()


def test_batch_invariance(standard):
    """The 48-match set on a 16-game handle (three batches) gives the 64-game handle's logs and results."""
    m, pairs, pol, T, ref, dev = standard
    small = _device(0, 16, m, pairs, T, pol)
    assert small["n"] == 16 and dev["n"] == 48
    for key in ("counts", "results", "steps", "faults"):
        assert np.array_equal(small[key], dev[key]), key
    assert S.same_log(small["log"], dev["log"])
    assert np.array_equal(small["hashes"], dev["hashes"][32:])   # the last batch


def test_sides_and_step_limit():
    """sides="first", until_step=4 on the mixed table: weights and explored are non-zero only on FIRST's heuristic decisions with
    k < 4 whose row has a threshold > 0 -- the weights on every one of those -- and the whole log is the model's."""
    n, T = 16, 200
    m, pairs = _schedule(n, seed0=33), _n12m()
    pol = _mixed(12, sides="first", until_step=4)
    ref = _model(0, m, pairs, T, pol)
    dev = _device(0, 64, m, pairs, T, pol)
    _assert_equals_model(dev, ref)
    log, found = dev["log"], 0
    for i, g in enumerate(ref["games"]):
        side, bot, row = np.array(g["side"]), np.array(g["bot"]), np.array(g["row"])
        may = (np.arange(g["steps"]) < 4) & (side == 0) & (bot == 0) & (pol.thresholds[np.maximum(row, 0)] > 0)
        assert np.array_equal(np.nonzero(log.weight_total[i])[0], np.nonzero(may)[0])   # (every score of these decisions is finite)
        assert np.array_equal(np.nonzero(log.taken_weight[i])[0], np.nonzero(may)[0])
        assert not log.explored[i][:g["steps"]][~may].any()
        found += int(log.explored[i].sum())
    assert found > 0 and (log.weight_total != 0).sum() > found


def test_dataset_and_behaviour_prob(standard):
    """game_log.dataset over the log, bot games included, under a keep mask that drops entries: every game replays to its end,
    and weight_total / taken_weight are the log's arrays at the kept entries in row order.  behaviour_prob over step_sides: in
    (0, 1] on decisions, below 1 somewhere, NaN on the bot's steps and behind."""
    m, pairs, pol, T, ref, dev = standard
    log = dev["log"]
    keep = np.ones(log.action.shape, dtype=np.uint8)
    keep[:, 1::3] = 0
    keep[5] = 0
    eng = _engine()
    d = game_log.dataset(eng, m, pairs, log, keep=keep, columns=("action", "game", "step", "greedy", "explored", "weight_total", "taken_weight"))
    hashes = eng.state_hash()
    sides = game_log.step_sides(eng, m, pairs, log)
    eng.close()
    assert not d["status"].any() and np.array_equal(d["replayed"], log.steps)
    assert np.array_equal(hashes, dev["hashes"])
    game, step = d["game"].cpu().numpy(), d["step"].cpu().numpy()
    assert len(game) == int(game_log.kept_counts(log.steps, keep).sum()) and not (game == 5).any() and not (step % 3 == 1).any()
    for c in ("action", "greedy", "explored", "weight_total", "taken_weight"):
        assert np.array_equal(d[c].cpu().numpy(), getattr(log, c)[game, step]), c
    assert d["weight_total"].any() and (d["greedy"] != d["action"]).any()
    to_play, bot = sides
    assert np.array_equal(to_play, P.sides_of(ref["games"], log.action.shape)[0]) and np.array_equal(bot, P.sides_of(ref["games"], log.action.shape)[1])
    mu = game_log.behaviour_prob(pol, m, log, sides)
    decision = log.n_legal > 0
    assert bot.any() and np.isnan(mu[bot]).all() and np.isnan(mu[log.action == 255]).all()
    assert (mu[decision] > 0).all() and (mu[decision] <= 1).all() and (mu[decision] < 1).any()
    assert np.array_equal(np.isnan(mu), ~decision)
    assert np.array_equal(mu, game_log.behaviour_prob(pol, m, ref["log"], sides), equal_nan=True)


def test_bad_arguments_leave_the_games_untouched():
    """NULL tables, an inverse temperature of -1, NaN or inf (also in a row whose threshold is 0), a sides bit above bit 1 and
    what the logged call refuses are MONSOON_ERR_ARG: nothing is written, the loaded games keep their states, and the handle
    plays on."""
    n, T = 16, 50
    m, pairs = _schedule(n, seed0=34), _n12m()
    eng = _engine()
    good = _mixed(3)
    eng.rollout_logged(W4, m, pairs, T, explore=good)
    before = eng.state_hash()
    counts = np.zeros((4, 3), dtype=np.int32)
    log = RolloutLog.empty(n, T, sample=True)
    c_log = _lib.RolloutLog(_ptr(log.action), _ptr(log.score), _ptr(log.n_legal))
    c_xlog = _lib.ExploreLog(_ptr(log.greedy), _ptr(log.explored), _ptr(log.taken_score))
    c_slog = _lib.SampleLog(_ptr(log.weight_total), _ptr(log.taken_weight))
    args = (_ptr(np.ascontiguousarray(W4)), 4, _ptr(m), n, _ptr(np.ascontiguousarray(pairs)), 1, T, _ptr(counts), None, None)
    thr, inv = good.thresholds, good.inv_temperatures
    assert thr[0] == 0
    tables = [(None, _ptr(inv)), (_ptr(thr), None)]
    keep_alive = []
    for bad in (-1.0, float("nan"), float("inf")):
        for r in (0, 2):   # (row 0's threshold is 0: its temperature is checked all the same)
            t = inv.copy()
            t[r] = bad
            keep_alive.append(t)
            tables.append((_ptr(thr), _ptr(t)))
    rules = [_lib.Policies(3, 3, 0, a, b) for a, b in tables] + [_lib.Policies(3, sides, 0, _ptr(thr), _ptr(inv)) for sides in (4, 7, 1 << 31)]
    for c_pol in rules + [None]:
        rc = eng.lib.monsoon_rollout_policies(eng.h, *args, ctypes.byref(c_log), ctypes.byref(c_pol) if c_pol is not None else None,
                                              ctypes.byref(c_xlog), ctypes.byref(c_slog))
        assert rc == _lib.ERR_ARG and not counts.any() and (log.action == 255).all() and not log.weight_total.any()
    c_pol = good.c_struct()
    for bad_log in (None, ctypes.byref(_lib.RolloutLog(None, None, None))):   # what monsoon_rollout_logged refuses
        rc = eng.lib.monsoon_rollout_policies(eng.h, *args, bad_log, ctypes.byref(c_pol), ctypes.byref(c_xlog), ctypes.byref(c_slog))
        assert rc == _lib.ERR_ARG
    bad_args = args[:1] + (0,) + args[2:]   # n_individuals = 0
    assert eng.lib.monsoon_rollout_policies(eng.h, *bad_args, ctypes.byref(c_log), ctypes.byref(c_pol), None, None) == _lib.ERR_ARG
    assert (log.action == 255).all() and np.array_equal(eng.state_hash(), before)
    # and the handle plays on: NULL xlog and slog
    assert eng.lib.monsoon_rollout_policies(eng.h, *args, ctypes.byref(c_log), ctypes.byref(c_pol), None, None) == _lib.OK
    again = eng.rollout_logged(W4, m, pairs, T, explore=good)
    assert np.array_equal(again[3].action, log.action) and counts[:, 2].sum() == n
    with pytest.raises(ValueError, match="3 rows"):
        eng.rollout_logged(W4, m, pairs, T, explore=Policies([0.5] * 3, [1.0] * 3, 1))
    eng.close()
