"""The sampling rollout off the device: game_log.sample_weights against exp and against the host build of the text the
kernels compile (monsoon_amd/csrc/sample_weight.h, a stand-alone program, once more under the sanitizers),
game_log.sample_rank on hand-made weights, engine.Explore(temperature=), and the model (tests/sample_model.py) through
game_log.logged_rollout."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib
import sample_model as S
from monsoon_amd import _lib, game_log
from monsoon_amd.cards import CARD_INDEX, deck_indices, needs_extended_each
from monsoon_amd.engine import Explore, RolloutLog, explore_entry_bytes, sample_entry_bytes
from monsoon_amd.fitness import MATCH_DTYPE, hash32_array

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << 24
W0 = np.random.RandomState(2024).uniform(0, 1, 10)
W2 = np.stack([W0, np.random.RandomState(7).uniform(0, 1, 10)])


def _grid():
    """x of the weight function: a fine grid of [-33, 0], the points round every half-integer multiple of ln 2 (where the
    range reduction switches n), the edges and what weighs nothing."""
    rs = np.random.RandomState(5)
    fine = np.linspace(-33.0, 0.0, 100001)
    ln2 = math.log(2.0)
    knots = np.array([(k + 0.5) * ln2 for k in range(-48, 1)])
    near = np.concatenate([np.nextafter(knots, -np.inf), knots, np.nextafter(knots, np.inf)])
    edges = np.array([0.0, -0.0, -32.0, np.nextafter(-32.0, -np.inf), np.nextafter(-32.0, 0.0), -5e-324, -1e-300, -1e-17, -33.0, -1e3,
                      -np.inf, np.nan])
    return np.concatenate([fine, near, edges, -rs.uniform(0, 33, 50000), -np.exp(rs.uniform(-40, 3.5, 50000))])


def test_sample_weights_fixed_points_and_monotony():
    w = game_log.sample_weights
    assert w(0.0, 0.0, 1.0) == ONE and w(3.5, 3.5, 0.25) == ONE and w(-0.0, 0.0, 1.0) == ONE
    assert w(0.0, 0.0, 1.0).dtype == np.uint32
    for x in (np.nan, -np.inf, np.nextafter(-32.0, -np.inf), -33.0, -1e300):
        assert w(x, 0.0, 1.0) == 0
    assert w(1.0, np.nan, 1.0) == 0 and w(np.inf, np.inf, 1.0) == 0 and w(1.0, np.inf, 1.0) == 0   # a NaN or infinite best
    x = np.sort(_grid()[:100001])
    ws = w(x, 0.0, 1.0).astype(np.int64)
    assert (np.diff(ws) >= 0).all() and ws[0] == 0 and ws[-1] == ONE and (ws <= ONE).all()
    # any shape, broadcasting: scores [3][4] against a best per row and one temperature
    scores = -np.arange(12.0).reshape(3, 4)
    got = w(scores, scores.max(axis=1, keepdims=True), 0.5)
    assert got.shape == (3, 4) and (got[:, 0] == ONE).all()
    assert np.array_equal(got, np.array([[w(s, row.max(), 0.5) for s in row] for row in scores]).reshape(3, 4))


def test_sample_weights_equal_floor_exp():
    """floor(exp(x) * 2**24) within +-1 on 10**5 points of [-33, 0] (0 differences measured)."""
    x = np.linspace(-33.0, 0.0, 100001)
    got = game_log.sample_weights(x, 0.0, 1.0).astype(np.int64)
    want = np.where(x >= -32.0, np.floor(np.exp(x) * ONE), 0.0).astype(np.int64)
    diff = np.abs(got - want)
    print("differences from floor(exp(x) * 2**24):", int((diff != 0).sum()), "max", int(diff.max()))
    assert diff.max() <= 1


def test_host_build_of_the_device_text_equals_numpy_bit_for_bit(tmp_path):
    """tests/sample_weight_check.cpp over monsoon_amd/csrc/sample_weight.h: built as the library is (-O2 -ffp-contract=off)
    and once more under the address and UB sanitizers, both stand-alone; the weights of the whole grid equal numpy's."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the oracle too"
    x = _grid()
    (tmp_path / "x.bin").write_bytes(x.astype("<f8").tobytes())
    want = game_log.sample_weights(x, 0.0, 1.0)
    assert (want == 0).any() and (want == ONE).any() and len(np.unique(want)) > 50000
    src = os.path.join(REPO, "tests", "sample_weight_check.cpp")
    for name, flags in (("plain", ["-O2", "-ffp-contract=off"]),
                        ("san", ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe, out = str(tmp_path / f"sample_weight_check_{name}"), tmp_path / f"w_{name}.bin"
        subprocess.run([cxx, "-std=c++17", *flags, "-I", os.path.join(REPO, "monsoon_amd", "csrc"), src, "-o", exe], check=True)
        r = subprocess.run([exe, str(tmp_path / "x.bin"), str(out)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.split() == ["ok", str(len(x))], r.stdout[-2000:] + r.stderr[-2000:]
        got = np.frombuffer(out.read_bytes(), dtype="<u4")
        assert np.array_equal(got, want), (name, int((got != want).sum()))


def test_sample_rank_on_hand_made_weights():
    rank = game_log.sample_rank
    w = np.array([0, 5, 0, 0, 7, 3, 0], dtype=np.uint32)   # total 15; prefixes 0 5 5 5 12 15 15
    total = 15

    def draw_for(r):   # the smallest draw1 with (draw1 * total) >> 32 == r
        return -((-r << 32) // total)
    assert (draw_for(4) * total) >> 32 == 4 and ((draw_for(4) - 1) * total) >> 32 == 3
    assert rank(w, 0) == 1                                   # r = 0: the first positive weight
    assert rank(w, 0xFFFFFFFF) == 5                          # r = total - 1: the last positive weight
    assert (0xFFFFFFFF * total) >> 32 == total - 1
    assert rank(w, draw_for(4)) == 1 and rank(w, draw_for(5)) == 4      # r == a prefix goes to the next action
    assert rank(w, draw_for(11)) == 4 and rank(w, draw_for(12)) == 5
    assert {rank(w, draw_for(r)) for r in range(total)} == {1, 4, 5}    # a zero-weight action is never picked
    counts = np.bincount([rank(w, draw_for(r)) for r in range(total)], minlength=7)
    assert np.array_equal(counts, w)                         # each action owns as many r as it weighs
    assert rank(np.zeros(4, dtype=np.uint32), 123) == -1 and rank(np.array([ONE], dtype=np.uint32), 0xFFFFFFFF) == 0
    full = np.full(156, ONE, dtype=np.uint32)                # the largest total: 156 * 2**24 < 2**32, no wrap in the prefix
    assert rank(full, 0) == 0 and rank(full, 0xFFFFFFFF) == 155 and rank(full, 1 << 31) == 78


def test_explore_temperature_validation():
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"), 5e-324):
        with pytest.raises(ValueError):
            Explore(0.5, 1, temperature=bad)
    for T in (1.0, 0.3, 1e-6, 1e6, 7):
        ex = Explore(0.5, 1, temperature=T)
        assert ex.samples and ex.temperature == float(T) and ex.inv_temperature == 1.0 / T
        c = ex.c_sample()
        assert c.inv_temperature == 1.0 / T
        assert (c.rule.seed, c.rule.threshold, c.rule.sides, c.rule.until_step) == (1, 1 << 31, 3, 0)
    plain, none = Explore(0.25, 9, sides="second", until_step=4), Explore(0.25, 9, sides="second", until_step=4, temperature=None)
    assert not plain.samples and not none.samples and none.inv_temperature is None and none.temperature is None
    assert bytes(plain.c_struct()) == bytes(none.c_struct()) == bytes(Explore(0.25, 9, "second", 4, temperature=2.0).c_struct())
    assert vars(plain) == vars(none)


def test_log_arrays_entry_bytes_and_abi():
    log = RolloutLog.empty(3, 7, sample=True)
    assert log.weight_total.dtype == log.taken_weight.dtype == np.uint32 and log.weight_total.shape == (3, 7)
    assert log.greedy is not None and not log.weight_total.any()
    assert RolloutLog.empty(3, 7, explore=True).weight_total is None and RolloutLog.empty(3, 7).taken_weight is None
    with pytest.raises(ValueError):
        RolloutLog.empty(3, 7, explore=True).taken_prob()
    other = RolloutLog.empty(1, 7, sample=True)
    other.weight_total[0, :2], other.taken_weight[0, :2] = (3 * ONE, ONE + 5), (ONE, 5)
    log.put([1], other)
    p = log.taken_prob()
    assert p.dtype == np.float64 and p[1, 0] == 1 / 3 and p[1, 1] == 5 / (ONE + 5) and np.isnan(p[0]).all() and np.isnan(p[1, 2:]).all()
    assert sample_entry_bytes() == 29 and sample_entry_bytes(False, False, False, False, False, False, False) == 1
    assert sample_entry_bytes(weight_total=False, taken_weight=False) == explore_entry_bytes() == 21
    header = open(os.path.join(REPO, "include", "monsoon.h")).read()
    assert "int monsoon_rollout_sample(" in header and "int monsoon_debug_sample_kat(" in header
    assert "typedef struct { monsoon_explore rule; double inv_temperature; } monsoon_sample;" in header
    assert "typedef struct { uint32_t* weight_total; uint32_t* taken_weight; } monsoon_sample_log;" in header
    assert "share the probability equally" in header and "ONE STEP MORE" in header
    assert len(_lib.SIGNATURES["monsoon_rollout_sample"][1]) == len(_lib.SIGNATURES["monsoon_rollout_explore"][1]) + 1
    assert [f[0] for f in _lib.Sample._fields_] == ["rule", "inv_temperature"] and _lib.Sample.inv_temperature.offset == 16
    assert [f[0] for f in _lib.SampleLog._fields_] == ["weight_total", "taken_weight"]
    assert game_log.LOG_COLUMNS["weight_total"][1] == game_log.LOG_COLUMNS["taken_weight"][1] == ()


def test_empty_log_arrays_dtypes_shapes_and_padding():
    """RolloutLog.empty for the four combinations of explore and sample, against literal values: which arrays there are,
    their dtypes and shapes, and the value every entry holds (what the device pads with behind a game's last step)."""
    base = {"action": ("|u1", 255), "score": ("<f8", None), "n_legal": ("<i2", 0)}
    explore = {"greedy": ("|u1", 255), "explored": ("|u1", 0), "taken_score": ("<f8", None)}
    sample = {"weight_total": ("<u4", 0), "taken_weight": ("<u4", 0)}
    names = ("action", "score", "n_legal", "greedy", "explored", "taken_score", "weight_total", "taken_weight")
    for ex, sm, want in ((False, False, base), (True, False, {**base, **explore}), (False, True, {**base, **explore, **sample}),
                         (True, True, {**base, **explore, **sample})):
        log = RolloutLog.empty(5, 3, explore=ex, sample=sm)
        assert sorted(vars(log)) == sorted(names + ("steps",))
        assert log.steps.dtype == np.int32 and log.steps.shape == (5,) and not log.steps.any()
        for name in names:
            a = getattr(log, name)
            if name not in want:
                assert a is None, (ex, sm, name)
                continue
            dtype, pad = want[name]
            assert a.dtype.str == dtype and a.shape == (5, 3) and a.flags.c_contiguous and a.flags.writeable, (ex, sm, name)
            assert np.isnan(a).all() if pad is None else (a == pad).all(), (ex, sm, name)
        arrays = [getattr(log, name) for name in names if name in want] + [log.steps]
        assert all(not np.shares_memory(a, b) for i, a in enumerate(arrays) for b in arrays[:i])
    bare = RolloutLog.empty(2, 4, scores=False, n_legal=False, sample=True)
    assert bare.score is None and bare.n_legal is None and bare.action.shape == (2, 4) and bare.taken_weight.dtype == np.uint32


class _OracleEngine:
    """BatchEngine's reset / legal_mask / step / status / observe / state_hash over one record of the oracle, for game_log.replay."""

    def __init__(self, tier):
        self.tier = tier

    def reset(self, seeds, decks):
        self.n = len(seeds)
        self.orc = oracle_lib.Oracle(self.n, extended=self.tier)
        for i in range(self.n):
            assert self.orc.reset(i, int(seeds[i]), decks[i][0], decks[i][1]) == 0

    def legal_mask(self):
        return np.stack([self.orc.legal_mask(i) for i in range(self.n)])

    def step(self, actions):
        for i, a in enumerate(actions):
            if a != 255:
                self.orc.step(i, int(a))

    def status(self):
        return np.array([[self.orc.to_play(i), int(self.orc.have_winner(i)), 0, 0] for i in range(self.n)], dtype=np.int32)

    def observe(self):
        obs = [self.orc.observe(i) for i in range(self.n)]
        return np.stack([np.zeros((27, 5, 4), dtype=np.int32) if o is None else o for o in obs]), np.array([o is None for o in obs])

    def state_hash(self):
        return np.array([self.orc.canon_hash(i) for i in range(self.n)], dtype=np.uint64)


def test_model_through_logged_rollout():
    """8 standard and 4 extended bot-free matches under Explore(0.5, 9, temperature=1.0) through the tier ladder: the weights
    are consistent, an action that weighs 2**24 without a tie is the arg-max, and every committed action is legal -- the
    games replay through game_log.replay to the states the model ended in."""
    n, T = 12, 80
    m = np.zeros(n, dtype=MATCH_DTYPE)
    k = np.arange(n)
    m["seed"], m["p1"], m["p2"] = hash32_array(51, k, 0xE), k % 2, 1 - k % 2
    std = deck_indices("N12M")
    a, b = std.copy(), std.copy()
    a[0], b[1] = CARD_INDEX["ua20"], CARD_INDEX["b005"]
    pairs = np.stack([np.stack([std, std]), np.stack([a, b]), np.stack([b, a])])
    m["deck"] = np.where(k < 8, 0, 1 + k % 2)
    assert np.array_equal(needs_extended_each(pairs), [False, True, True])
    ex = Explore(0.5, 9, temperature=1.0)
    engines = {}

    def engine_for_tier(t):
        return engines.setdefault(t, S.ModelEngine(t))
    counts, results, steps, faults, log = game_log.logged_rollout(engine_for_tier, W2, m, pairs, T, ex)
    assert set(engines) >= {0, 1} and counts[:, 2].sum() == n and (steps > 0).all()
    assert log.weight_total is not None and log.weight_total.dtype == np.uint32
    sampled = log.explored != 0
    decision = log.n_legal > 0
    assert sampled.sum() > 50 and (sampled & ~decision).sum() == 0
    assert (log.taken_weight <= log.weight_total).all()
    assert (log.weight_total[sampled] >= ONE).all() and (log.taken_weight[sampled] > 0).all()
    assert not log.weight_total[~sampled].any() and not log.taken_weight[~sampled].any()
    assert np.array_equal(log.greedy[decision & ~sampled], log.action[decision & ~sampled])
    p = log.taken_prob()
    assert np.isnan(p[~sampled]).all() and (p[sampled] > 0).all() and (p[sampled] <= 1).all()
    # an action that weighs 2**24 where no other does is the arg-max; with a tie it need not be
    tie = np.zeros(log.action.shape, dtype=bool)
    games = {}
    # (the ladder's sub-schedules lose the match order: find every game's record by its seed through one more model run)
    for i in range(n):
        one = m[i:i + 1].copy()
        one["deck"] = 0
        tier = int(needs_extended_each(pairs[m["deck"][i]][None])[0])
        eng = S.ModelEngine(tier)
        _, r1, s1, lg1 = eng.rollout_logged(W2, one, pairs[m["deck"][i]][None], T, explore=ex)
        if faults[i] < 16:   # (not replayed on a larger record)
            assert s1[0] == steps[i] and np.array_equal(lg1.action[0], log.action[i]) and np.array_equal(lg1.weight_total[0], log.weight_total[i])
            tie[i, :s1[0]] = eng.games[0]["tie"]
            games[i] = eng.games[0]
    full = sampled & (log.taken_weight == ONE) & ~tie
    assert full.any() and np.array_equal(log.action[full], log.greedy[full])
    assert (sampled & (log.action != log.greedy)).any()
    assert (log.taken_score[sampled] <= log.score[sampled]).all()
    # every committed action is legal: the games replay to their ends, tier by tier
    for tier, rows in ((0, k < 8), (1, k >= 8)):
        sub = m[rows].copy()
        sub_log = RolloutLog(log.action[rows], log.score[rows], log.n_legal[rows], log.steps[rows])
        gen = game_log.replay(_OracleEngine(tier), sub, pairs, sub_log)
        n_items = 0
        while True:
            try:
                next(gen)
                n_items += 1
            except StopIteration as stop:
                finals = stop.value
                break
        assert n_items == sub_log.steps.max()
        idx = np.nonzero(rows)[0]
        clean = np.array([faults[i] == 0 for i in idx])
        assert clean.any()
        want = np.array([games[i]["final"] for i in idx if faults[i] == 0], dtype=np.uint64)
        assert np.array_equal(finals[clean], want)
