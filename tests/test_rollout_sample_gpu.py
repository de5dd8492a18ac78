"""monsoon_rollout_sample on the device (k_play_sample): against monsoon_rollout_logged where nothing samples, entry by entry
against the model over the CPU oracle (tests/sample_model.py) where decisions do -- on the three record builds, with the
places the kernel can go wrong counted from the model's own log -- and the sampler alone on synthetic rows
(monsoon_debug_sample_kat) against game_log.sample_weights / sample_rank."""
import ctypes

import numpy as np
import pytest

import sample_model as S
from monsoon_amd import EXPERT, _lib, game_log
from monsoon_amd.cards import C5_STREAM_XOR, CARD_INDEX, deck_indices, draw_random_decks_numpy, needs_extended_each
from monsoon_amd.engine import BatchEngine, Explore, RolloutLog, _ptr
from monsoon_amd.fitness import MATCH_DTYPE, hash32_array

pytestmark = pytest.mark.gpu

ONE = 1 << 24
W0 = np.random.RandomState(2024).uniform(0, 1, 10)
W2 = np.stack([W0, np.random.RandomState(7).uniform(0, 1, 10)])   # two weight vectors
U = 8   # candidate lanes per pass of every build's default variant (variants.def)


def _schedule(n, seed0=0, bot=True):
    """n matches over the two rows of W2: a third each of bot-FIRST, bot-SECOND and plain; bot=False: the same seeds and rows
    without the bot."""
    m = np.zeros(n, dtype=MATCH_DTYPE)
    k = np.arange(n)
    row, third = k % 2, k % 3 if bot else np.full(n, 2)
    m["seed"] = hash32_array(seed0, k, 0xE)
    m["p1"] = np.where(third == 0, EXPERT, row)
    m["p2"] = np.where(third == 1, EXPERT, np.where(third == 0, row, 1 - row))
    return m


def _n12m():
    d = deck_indices("N12M")
    return np.stack([d, d])[None]


def _standard_set():
    """48 mixed matches: the even ones on N12M, the odd ones on random 109-card pairs the standard record holds."""
    n = 48
    m = _schedule(n, seed0=21)
    drawn = draw_random_decks_numpy(hash32_array(77, np.arange(4 * n)) ^ np.uint32(C5_STREAM_XOR))
    drawn = drawn[~needs_extended_each(drawn)][:n // 2]
    assert len(drawn) == n // 2
    pairs = np.concatenate([_n12m(), drawn])
    m["deck"] = np.where(np.arange(n) % 2 == 0, 0, 1 + np.arange(n) // 2)
    return m, pairs


def _engine(max_games=64, build=0):
    """A handle; torch loads its runtime before the library does (VecEnv.__init__ says why), for the sake of dataset."""
    import torch
    assert torch.cuda.is_available()
    return BatchEngine(max_games, extended=build)


def _device(build, cap, m, pairs, T, ex):
    eng = _engine(cap, build)
    assert eng.variant()[0] == U
    counts, results, steps, log = eng.rollout_logged(W2, m, pairs, T, explore=ex)
    out = dict(counts=counts, results=results, steps=steps, log=log, faults=eng.rollout_faults(len(m)), hashes=eng.state_hash(), n=eng.n,
               stats=eng.stats())
    eng.close()
    return out


def _model(build, m, pairs, T, ex):
    model = S.ModelEngine(build)
    counts, results, steps, log = model.rollout_logged(W2, m, pairs, T, explore=ex)
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


def _sampled(games):
    """(game, k) of every decision of the model's log that sampled an action (its weights did not sum to 0)."""
    return [(g, k) for g in games for k in range(g["steps"]) if g["rank"][k] >= 0]


@pytest.fixture(scope="module")
def standard():
    """The standard set under Explore(0.5, 9, temperature=1.0), by the model and by a 64-game handle: computed once, read by
    several tests."""
    m, pairs = _standard_set()
    ex, T = Explore(0.5, 9, temperature=1.0), 200
    return m, pairs, ex, T, _model(0, m, pairs, T, ex), _device(0, 64, m, pairs, T, ex)


def test_nothing_changes_without_sampling():
    """64 mixed matches: Explore(0, s, temperature=1) equals monsoon_rollout_logged bit for bit -- log (padding included),
    counts, results, steps, faults, hashes, statistics -- and greedy = action, explored = 0, taken_score = score on decisions,
    both weights 0."""
    n, T = 64, 200
    m, pairs = _schedule(n), _n12m()
    eng = _engine()
    counts = np.zeros((2, 3), dtype=np.int32)
    results, steps, log = np.zeros(n, dtype=np.int8), np.zeros(n, dtype=np.int32), RolloutLog.empty(n, T)
    c_log = _lib.RolloutLog(_ptr(log.action), _ptr(log.score), _ptr(log.n_legal))
    args = (_ptr(np.ascontiguousarray(W2)), 2, _ptr(m), n, _ptr(np.ascontiguousarray(pairs)), 1, T)
    assert eng.lib.monsoon_rollout_logged(eng.h, *args, _ptr(counts), _ptr(results), _ptr(steps), ctypes.byref(c_log)) == _lib.OK
    eng.n = n
    parent = dict(counts=counts, results=results, steps=steps, faults=eng.rollout_faults(n), hashes=eng.state_hash(), stats=eng.stats())
    eng.close()
    assert (steps > 0).all() and (log.n_legal > 0).any() and np.isnan(log.score[log.action != 255]).any()
    zero = _device(0, 64, m, pairs, T, Explore(0.0, 1234, temperature=1.0))
    for key in ("counts", "results", "steps", "faults", "hashes"):
        assert np.array_equal(zero[key], parent[key]), key
    assert zero["stats"] == parent["stats"]
    zl, decision = zero["log"], log.n_legal > 0
    assert np.array_equal(zl.action, log.action) and np.array_equal(zl.n_legal, log.n_legal)
    assert np.array_equal(zl.score.view(np.uint64), log.score.view(np.uint64))   # the padding's bits too
    assert np.array_equal(zl.greedy[decision], log.action[decision]) and (zl.greedy[~decision] == 255).all()
    assert not zl.explored.any()
    assert np.array_equal(zl.taken_score[decision].view(np.uint64), log.score[decision].view(np.uint64))
    assert np.isnan(zl.taken_score[~decision]).all()
    assert zl.weight_total.dtype == np.uint32 and not zl.weight_total.any() and not zl.taken_weight.any()


def test_the_standard_set_reaches_every_place_the_kernel_can_go_wrong(standard):
    """From the model's log alone: the chosen rank in the first pass, in a later pass, in a third or later pass, at the end of a
    partial last pass, equal to the greedy action, the greedy action in a later and in an earlier pass than the chosen one, a
    zero weight, a single legal action, a tie for the best, and a non-greedy action taken whose score is exactly 0.0."""
    seen = dict.fromkeys(("first_pass", "later_pass", "third_pass", "last_of_partial", "is_greedy", "greedy_later", "greedy_earlier",
                          "zero_weight", "one_legal", "tie", "zero_score_taken"), 0)
    picks = _sampled(standard[4]["games"])
    for g, k in picks:
        r, gr, nl = g["rank"][k], g["greedy_rank"][k], g["n_legal"][k]
        seen["first_pass"] += r < U
        seen["later_pass"] += r >= U
        seen["third_pass"] += r >= 2 * U
        seen["last_of_partial"] += r == nl - 1 and nl % U != 0
        seen["is_greedy"] += g["action"][k] == g["greedy"][k]
        seen["greedy_later"] += gr // U > r // U
        seen["greedy_earlier"] += gr // U < r // U
        seen["zero_weight"] += g["zero_weight"][k]
        seen["one_legal"] += nl == 1
        seen["tie"] += g["tie"][k]
        seen["zero_score_taken"] += g["action"][k] != g["greedy"][k] and g["taken_score"][k] == 0.0
    print(len(picks), "sampled decisions:", seen, "games without a fault:", int((standard[4]["faults"] == 0).sum()))
    assert all(v > 0 for v in seen.values()), seen


def test_device_log_equals_model_log_standard(standard):
    m, pairs, ex, T, ref, dev = standard
    _assert_equals_model(dev, ref)
    log = dev["log"]
    sampled = log.explored != 0
    assert sampled.any() and (log.greedy != log.action).any() and np.isnan(log.taken_score[log.action != 255]).any()
    assert (log.weight_total[sampled] >= ONE).all() and (log.taken_weight <= log.weight_total).all()
    assert not log.weight_total[~sampled].any() and not log.taken_weight[~sampled].any()
    assert (log.taken_score[sampled] <= log.score[sampled]).all()   # (the arg-max is the arg-max)


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
    ex = Explore(0.5, 10, temperature=1.0)
    ref = _model(1, m, pairs, T, ex)
    assert any((np.array(g["rank"]) >= U).any() for g in ref["games"])
    _assert_equals_model(_device(1, 64, m, pairs, T, ex), ref)


def test_device_log_equals_model_log_large():
    """4 matches on the large build."""
    n, T = 4, 120
    m, pairs = _schedule(n, seed0=32), _n12m()
    ex = Explore(0.5, 11, temperature=1.0)
    ref = _model(2, m, pairs, T, ex)
    assert any((np.array(g["rank"]) >= U).any() for g in ref["games"])
    _assert_equals_model(_device(2, 64, m, pairs, T, ex), ref)


def test_cold_temperature_commits_a_best_action():
    """temperature=1e-6, eps = 1 on the first 16 matches of the standard set: every sampled decision commits an action whose
    score equals the best one -- the arg-max or one tied with it -- and weight_total is a multiple of 2**24."""
    (m, pairs), T = _standard_set(), 200
    m = m[:16]
    ex = Explore(1.0, 9, temperature=1e-6)
    ref, dev = _model(0, m, pairs, T, ex), _device(0, 64, m, pairs, T, ex)
    _assert_equals_model(dev, ref, min_clean=0.0)   # (how many of these games end on a fault is not this test's matter)
    log = dev["log"]
    sampled = log.explored != 0
    assert sampled.sum() > 100 and np.array_equal(sampled, log.n_legal > 0)
    assert (log.taken_score[sampled] == log.score[sampled]).all()
    assert (log.weight_total[sampled] % ONE == 0).all() and (log.weight_total[sampled] >= ONE).all() and (log.taken_weight[sampled] == ONE).all()


def test_hot_temperature_is_nearly_uniform():
    """temperature=1e6, eps = 1 on the first 16 matches of the standard set: every weight the model computes is >= 2**24 - 2**12
    (exp(-g / 1e6) for a score gap g up to 244; the largest gap of these games is below that), and the log equals the model's."""
    (m, pairs), T = _standard_set(), 200
    m = m[:16]
    ex = Explore(1.0, 9, temperature=1e6)
    ref, dev = _model(0, m, pairs, T, ex), _device(0, 64, m, pairs, T, ex)
    picks = _sampled(ref["games"])
    assert len(picks) > 100 and all(g["min_weight"][k] >= ONE - (1 << 12) for g, k in picks)
    _assert_equals_model(dev, ref, min_clean=0.0)   # (likewise)
    assert (dev["log"].action != dev["log"].greedy).any()


KAT_N_LEGAL = (1, 7, 8, 9, 63, 64, 65, 128, 129, 156)


def _kat_rows():
    """(scores[m][156], n_legal[m], best[m], inv_temperature[m], draw1[m]) of the synthetic decisions: for every n_legal a row
    of equal scores, a row whose best is NaN, a row with +inf in it, the draws 0, 1, 2**31, 2**32 - 1 and 16 random draws over
    seeded scores scaled so that zero weights occur."""
    rs = np.random.RandomState(99)
    rows = []
    for n in KAT_N_LEGAL:
        def fresh():
            s = np.zeros(156)
            s[:n] = rs.uniform(-60.0, 0.0, n) * rs.choice([0.1, 1.0])
            return s
        equal = np.zeros(156)
        equal[:n] = 3.25
        rows.append((equal, n, 3.25, 1.0, int(rs.randint(0, 2 ** 32, dtype=np.uint64))))
        s = fresh()
        rows.append((s, n, np.nan, 1.0, 12345))
        s = fresh()
        s[rs.randint(n)] = np.inf
        rows.append((s, n, np.inf, 1.0, 12345))
        for d in (0, 1, 1 << 31, 0xFFFFFFFF):
            s = fresh()
            rows.append((s, n, s[:n].max(), 1.0, d))
        for _ in range(16):
            s = fresh()
            rows.append((s, n, s[:n].max(), float(rs.choice([0.5, 1.0, 4.0])), int(rs.randint(0, 2 ** 32, dtype=np.uint64))))
    cols = list(zip(*rows))
    return (np.stack(cols[0]), np.array(cols[1], dtype=np.int32), np.array(cols[2]), np.array(cols[3]), np.array(cols[4], dtype=np.uint32))


def test_sampler_on_synthetic_rows():
    """monsoon_debug_sample_kat: j*, total and w_j* of every row equal sample_weights / sample_rank exactly.  The rows with more
    than 64 legal actions are where a lane holds more than one rank."""
    scores, n_legal, best, inv_t, draw1 = _kat_rows()
    assert len(scores) == len(KAT_N_LEGAL) * 23
    eng = _engine()
    rank, total, weight = eng.debug_sample_kat(scores, n_legal, best, inv_t, draw1)
    bad = np.zeros(1, dtype=np.int32)
    for n in (0, 157, -1):   # refused, nothing launched
        rc = eng.lib.monsoon_debug_sample_kat(eng.h, 1, _ptr(scores[:1].copy()), _ptr(np.array([n], dtype=np.int32)), _ptr(best[:1].copy()),
                                              _ptr(inv_t[:1].copy()), _ptr(draw1[:1].copy()), _ptr(bad), _ptr(np.zeros(1, dtype=np.uint32)),
                                              _ptr(np.zeros(1, dtype=np.uint32)))
        assert rc == _lib.ERR_ARG
    eng.close()
    zero_weights = later_lanes = empty = 0
    for i in range(len(scores)):
        n = int(n_legal[i])
        w = game_log.sample_weights(scores[i, :n], best[i], inv_t[i])
        want_total = int(w.astype(np.uint64).sum())
        j = game_log.sample_rank(w, int(draw1[i]))
        assert (int(rank[i]), int(total[i]), int(weight[i])) == (j, want_total, int(w[j]) if j >= 0 else 0), (i, n)
        zero_weights += bool((w == 0).any()) and want_total > 0
        later_lanes += j >= 64
        empty += want_total == 0
    assert zero_weights > 20 and later_lanes > 20 and empty == 2 * len(KAT_N_LEGAL)
    equal = np.arange(len(scores)) % 23 == 0   # the rows of equal scores: every action weighs 2**24
    assert np.array_equal(total[equal], (n_legal[equal] * ONE).astype(np.uint32)) and (weight[equal] == ONE).all()


def test_batch_invariance(standard):
    """The 48-match sampling schedule on a 16-game handle (three batches) gives the 64-game handle's logs and results."""
    m, pairs, ex, T, ref, dev = standard
    small = _device(0, 16, m, pairs, T, ex)
    assert small["n"] == 16 and dev["n"] == 48
    for key in ("counts", "results", "steps", "faults"):
        assert np.array_equal(small[key], dev[key]), key
    assert S.same_log(small["log"], dev["log"])
    assert np.array_equal(small["hashes"], dev["hashes"][32:])   # the last batch


def test_sides_and_step_limit():
    """Explore(1.0, s, sides="first", until_step=4, temperature=1.0): the sampled entries are exactly FIRST's decisions with
    k < 4, and the whole log is the model's."""
    n, T = 16, 200
    m, pairs = _schedule(n, seed0=33), _n12m()
    ex = Explore(1.0, 12, sides="first", until_step=4, temperature=1.0)
    ref = _model(0, m, pairs, T, ex)
    dev = _device(0, 64, m, pairs, T, ex)
    _assert_equals_model(dev, ref)
    log, found = dev["log"], 0
    for i, g in enumerate(ref["games"]):
        side, bot = np.array(g["side"]), np.array(g["bot"])
        where = np.nonzero(log.explored[i])[0]
        may = (np.arange(g["steps"]) < 4) & (side == 0) & (bot == 0)
        assert np.array_equal(np.nonzero(may)[0], where)   # (no draw0 of these games is 0xFFFFFFFF)
        assert np.array_equal(np.nonzero(log.weight_total[i])[0], where)
        found += len(where)
    assert found > 0 and (log.explored.sum(axis=1) <= 4).all()


def test_dataset_carries_the_new_columns(standard):
    """game_log.dataset over the sampled log, bot games included, under a keep mask that drops entries: every game replays to
    its end (a sampled action is legal), the final hashes are the rollout's, and weight_total / taken_weight are the log's
    arrays gathered at the kept entries in row order."""
    m, pairs, ex, T, ref, dev = standard
    log = dev["log"]
    keep = np.ones(log.action.shape, dtype=np.uint8)
    keep[:, 1::3] = 0
    keep[5] = 0
    eng = _engine()
    d = game_log.dataset(eng, m, pairs, log, keep=keep, columns=("action", "game", "step", "greedy", "explored", "weight_total", "taken_weight"))
    hashes = eng.state_hash()
    eng.close()
    assert not d["status"].any() and np.array_equal(d["replayed"], log.steps)
    assert np.array_equal(hashes, dev["hashes"])
    game, step = d["game"].cpu().numpy(), d["step"].cpu().numpy()
    assert len(game) == int(game_log.kept_counts(log.steps, keep).sum()) and not (game == 5).any() and not (step % 3 == 1).any()
    assert np.array_equal(d["action"].cpu().numpy(), log.action[game, step])
    assert np.array_equal(d["greedy"].cpu().numpy(), log.greedy[game, step])
    assert np.array_equal(d["explored"].cpu().numpy(), log.explored[game, step])
    assert np.array_equal(d["weight_total"].cpu().numpy(), log.weight_total[game, step])
    assert np.array_equal(d["taken_weight"].cpu().numpy(), log.taken_weight[game, step])
    assert d["weight_total"].any() and (d["greedy"] != d["action"]).any()
    plain = RolloutLog(log.action, log.score, log.n_legal, log.steps, log.greedy, log.explored, log.taken_score)
    with pytest.raises(ValueError, match="Explore rule"):
        game_log.dataset(None, m, pairs, plain, columns=("weight_total",))


def test_bad_arguments_leave_the_games_untouched():
    """inv_temperature 0, -1, NaN, +inf and a sides bit above bit 1 are MONSOON_ERR_ARG: nothing is written, the loaded games
    keep their states, and the handle plays on."""
    n, T = 16, 50
    m, pairs = _schedule(n, seed0=34), _n12m()
    eng = _engine()
    good = Explore(0.5, 3, temperature=1.0)
    eng.rollout_logged(W2, m, pairs, T, explore=good)
    before = eng.state_hash()
    counts = np.zeros((2, 3), dtype=np.int32)
    log = RolloutLog.empty(n, T, sample=True)
    c_log = _lib.RolloutLog(_ptr(log.action), _ptr(log.score), _ptr(log.n_legal))
    c_xlog = _lib.ExploreLog(_ptr(log.greedy), _ptr(log.explored), _ptr(log.taken_score))
    c_slog = _lib.SampleLog(_ptr(log.weight_total), _ptr(log.taken_weight))
    args = (_ptr(np.ascontiguousarray(W2)), 2, _ptr(m), n, _ptr(np.ascontiguousarray(pairs)), 1, T, _ptr(counts), None, None)
    rules = [_lib.Sample(_lib.Explore(3, 1 << 31, 3, 0), bad) for bad in (0.0, -1.0, float("nan"), float("inf"))]
    rules += [_lib.Sample(_lib.Explore(3, 1 << 31, sides, 0), 1.0) for sides in (4, 7, 1 << 31)]
    rules += [_lib.Sample(_lib.Explore(3, 0, 3, 0), float("nan"))]   # (also where the rule would never sample)
    for c_sm in rules:
        rc = eng.lib.monsoon_rollout_sample(eng.h, *args, ctypes.byref(c_log), ctypes.byref(c_sm), ctypes.byref(c_xlog), ctypes.byref(c_slog))
        assert rc == _lib.ERR_ARG and not counts.any() and (log.action == 255).all() and not log.weight_total.any()
    for bad_log in (None, ctypes.byref(_lib.RolloutLog(None, None, None))):   # what monsoon_rollout_logged refuses
        c_sm = good.c_sample()
        rc = eng.lib.monsoon_rollout_sample(eng.h, *args, bad_log, ctypes.byref(c_sm), ctypes.byref(c_xlog), ctypes.byref(c_slog))
        assert rc == _lib.ERR_ARG
    assert np.array_equal(eng.state_hash(), before)
    c_sm = good.c_sample()   # and the handle plays on: NULL xlog and slog
    assert eng.lib.monsoon_rollout_sample(eng.h, *args, ctypes.byref(c_log), ctypes.byref(c_sm), None, None) == _lib.OK
    again = eng.rollout_logged(W2, m, pairs, T, explore=good)
    assert np.array_equal(again[3].action, log.action) and counts[:, 2].sum() == n
    eng.close()
