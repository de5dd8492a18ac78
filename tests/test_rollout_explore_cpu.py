"""The exploring rollout off the device: its model (tests/explore_model.py) against the model of the logged rollout,
engine.Explore, game_log.explore_draws, the tier ladder under exploration, the layout and batch cap of the larger device
log (a stand-alone host program under the sanitizers), and the ABI surface."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import explore_model as X
import rollout_log_model as R
from monsoon_amd import EXPERT, _lib, game_log
from monsoon_amd.cards import CARD_INDEX, deck_indices, needs_extended_each
from monsoon_amd.engine import LOG_BUDGET, Explore, RolloutLog, explore_entry_bytes
from monsoon_amd.fitness import MATCH_DTYPE, hash32, hash32_array

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W0 = np.random.RandomState(2024).uniform(0, 1, 10)
W2 = np.stack([W0, np.random.RandomState(7).uniform(0, 1, 10)])


def _mixed(n, seed0):
    """A third each of bot-FIRST, bot-SECOND and plain matches over the two rows of W2."""
    m = np.zeros(n, dtype=MATCH_DTYPE)
    k = np.arange(n)
    row, third = k % 2, k % 3
    m["seed"] = hash32_array(seed0, k, 0xE)
    m["p1"] = np.where(third == 0, EXPERT, row)
    m["p2"] = np.where(third == 1, EXPERT, np.where(third == 0, row, 1 - row))
    return m


def _n12m():
    d = deck_indices("N12M")
    return np.stack([d, d])[None]


def test_model_without_exploration_is_the_logged_rollouts_model():
    """8 N12M games, the bot in two thirds of them: with eps = 0 (and with no rule at all) the exploring model's log,
    results, counts and faults are rollout_log_model's; greedy = action, explored = 0, taken_score = score on decisions."""
    m, pairs, T = _mixed(8, 11), _n12m(), 200
    ref_eng = R.ModelEngine(0)
    ref = ref_eng.rollout_logged(W2, m, pairs, T)
    for rule in (None, Explore(0.0, 5)):
        eng = X.ModelEngine(0)
        got = eng.rollout_logged(W2, m, pairs, T, explore=rule)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
        assert np.array_equal(eng.rollout_faults(8), ref_eng.rollout_faults(8)) and np.array_equal(eng.finals, ref_eng.finals)
        log = got[3]
        assert R.same_log(log, ref[3])
        if rule is None:
            assert log.greedy is None and log.explored is None and log.taken_score is None
            continue
        decision = log.n_legal > 0
        assert decision.any() and (~decision & (log.action != 255)).any()   # decisions and bot steps
        assert np.array_equal(log.greedy[decision], log.action[decision]) and (log.greedy[~decision] == 255).all()
        assert not log.explored.any()
        assert np.array_equal(log.taken_score[decision].view(np.uint64), log.score[decision].view(np.uint64))
        assert np.isnan(log.taken_score[~decision]).all()


def test_explore_validation_and_threshold_edges():
    assert Explore(0, 1).threshold == 0
    assert Explore(1, 1).threshold == 0xFFFFFFFF
    assert Explore(2.0 ** -32, 1).threshold == 1
    assert Explore(0.5, 1).threshold == 1 << 31 and Explore(0.1, 1).threshold == int(0.1 * 2 ** 32)
    for bad in (-1e-9, 1.0000001, 2, float("nan")):
        with pytest.raises(ValueError):
            Explore(bad, 1)
    with pytest.raises(ValueError):
        Explore(0.1, 1, sides="third")
    assert [Explore(0.1, 1, sides=s).side_bits for s in ("first", "second", "both")] == [1, 2, 3]
    ex = Explore(0.1, 2 ** 32 + 7, sides="second", until_step=4)
    c = ex.c_struct()
    assert (c.seed, c.threshold, c.sides, c.until_step) == (7, ex.threshold, 2, 4)
    assert [bool(ex.may_explore(s, k)) for s, k in ((0, 0), (1, 0), (1, 3), (1, 4))] == [False, True, True, False]
    assert bool(Explore(0.1, 1).may_explore(0, 10 ** 6)) and bool(Explore(0.1, 1, until_step=-3).may_explore(1, 50))


def test_explore_draws_equal_scalar_hash32():
    rs = np.random.RandomState(3)
    seeds = rs.randint(0, 2 ** 32, size=200, dtype=np.uint64).astype(np.uint32)
    seeds[:3] = (0, 1, 0xFFFFFFFF)
    k = rs.randint(0, 300, size=200)
    n_legal = rs.randint(1, 157, size=200)
    for ex in (Explore(0.25, 0xDEADBEEF), Explore(1.0, 0), Explore(0.0, 9), Explore(2.0 ** -32, 4)):
        explores, rank = game_log.explore_draws(ex, seeds, k, n_legal)
        assert explores.dtype == bool and explores.shape == rank.shape == (200,)
        for i in range(200):
            d0, d1 = hash32(ex.seed, int(seeds[i]), int(k[i]), 0), hash32(ex.seed, int(seeds[i]), int(k[i]), 1)
            assert bool(explores[i]) == (d0 < ex.threshold) and int(rank[i]) == (d1 * int(n_legal[i])) >> 32
            assert (bool(explores[i]), int(rank[i])) == X.draw(ex, int(seeds[i]), int(k[i]), int(n_legal[i]))
        assert (rank >= 0).all() and (rank < n_legal).all()
    assert 30 < game_log.explore_draws(Explore(0.25, 1), seeds, k, n_legal)[0].sum() < 70   # about a quarter of 200
    # broadcasting: one match, all its steps
    e, r = game_log.explore_draws(Explore(0.5, 2), 77, np.arange(10), 5)
    assert e.shape == (10,) and [int(x) for x in r] == [(hash32(2, 77, j, 1) * 5) >> 32 for j in range(10)]


class _LimitedOnce(X.ModelEngine):
    """A tier-0 model that reports the games with the seeds `victims` as ended on a limit of its record (code 16, a draw),
    as the standard record does for games it cannot hold: the ladder plays them again on the next record."""

    def __init__(self, victims):
        super().__init__(0)
        self.victims = set(int(v) for v in victims)

    def rollout_logged(self, weights, matches, deck_pairs, max_turns, scores=True, n_legal=True, explore=None):
        counts, results, steps, log = super().rollout_logged(weights, matches, deck_pairs, max_turns, scores, n_legal, explore)
        self.first_logs = {int(m["seed"]): (log.action[i].copy(), log.explored[i].copy(), list(self.games[i]["rank"]))
                           for i, m in enumerate(matches)}
        for i, m in enumerate(matches):
            if int(m["seed"]) in self.victims:
                row, win = (int(m["p1"]), 0) if m["p1"] >= 0 else (int(m["p2"]), 1)
                counts[row] -= (results[i] == win, results[i] == -1, 0)
                counts[row, 1] += 1
                results[i], self.faults[i] = -1, 16
        return counts, results, steps, log


def test_ladder_replays_explore_as_the_draws_prescribe():
    """12 games, two of them on a deck pair holding ua20 (they start on the extended record), three of the others reported
    record-limited by the standard tier: every game of the final log -- the replayed ones on the larger record among them
    -- has exactly the explored flags and ranks that explore_draws prescribes from its seed, step and legal count, and a
    replayed game explored on the larger record as it did on the smaller one."""
    n, T = 12, 60
    ex = Explore(0.3, 41)
    m = _mixed(n, 17)
    std = deck_indices("N12M")
    ext = std.copy()
    ext[0] = CARD_INDEX["ua20"]
    pairs = np.stack([np.stack([std, std]), np.stack([std, ext])])
    assert needs_extended_each(pairs).tolist() == [False, True]
    m["deck"] = (np.arange(n) % 6 == 5).astype(np.uint32)
    victims = m["seed"][[1, 2, 6]]
    engines = {0: _LimitedOnce(victims)}
    counts, results, steps, faults, log = game_log.logged_rollout(lambda t: engines.setdefault(t, X.ModelEngine(t)), W2, m, pairs, T, explore=ex)
    assert [c[0] for c in engines[0].calls] == [10] and [c[0] for c in engines[1].calls] == [2, 3] and 2 not in engines
    assert sorted(engines[1].calls[1][1].tolist()) == sorted(victims.tolist()) and not faults.any()
    assert log.greedy is not None and log.explored.any() and counts[:, 2].sum() == n
    replayed = {int(s): g for s, g in zip(engines[1].calls[1][1], engines[1].games)}
    for i in range(n):
        seed, ln = int(m["seed"][i]), int(steps[i])
        decision = log.n_legal[i, :ln] > 0
        k = np.arange(ln)
        explores, rank = game_log.explore_draws(ex, seed, k, np.maximum(log.n_legal[i, :ln], 1))
        assert np.array_equal(log.explored[i, :ln] != 0, explores & decision), i
        assert not log.explored[i, ln:].any() and (log.greedy[i, ln:] == 255).all()
        same = decision & ~explores
        assert np.array_equal(log.greedy[i, :ln][same], log.action[i, :ln][same])
        if seed in replayed:   # the rows are the larger record's, and its ranks are the prescribed ones
            g = replayed[seed]
            assert g["steps"] == ln and np.array_equal(g["action"], log.action[i, :ln])
            want = np.where(explores & decision, rank, -1)
            assert np.array_equal(np.array(g["rank"]), want), i
            a0, e0, r0 = engines[0].first_logs[seed]   # N12M plays the same game on both records
            assert np.array_equal(a0, log.action[i]) and np.array_equal(e0, log.explored[i]) and r0 == g["rank"]
    assert any((np.array(g["rank"]) >= 0).any() for g in replayed.values())


def test_device_log_layout_and_batch_cap_under_sanitizers(tmp_path):
    """tests/explore_layout_check.cpp over host_layout.h's log_layout / log_entry_bytes / log_batch_cap -- all 128 choices of
    the seven optional columns, each against the layouts the one table replaced -- and the same cap formula in the Python layer."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the oracle too"
    exe = str(tmp_path / "explore_layout_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "monsoon_amd", "csrc"), os.path.join(REPO, "tests", "explore_layout_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) == 6 * 3 * 128 and int(words[3]) == 4 * 3 * 4, r.stdout
    assert explore_entry_bytes() == 21 and explore_entry_bytes(False, False) == 11 and explore_entry_bytes(True, True, False, False, False) == 11
    assert LOG_BUDGET // (explore_entry_bytes() * 30000) == 426 and LOG_BUDGET // (explore_entry_bytes() * 200) == 63913
    header = open(os.path.join(REPO, "include", "monsoon.h")).read()
    assert "1 + 8 [score] + 2 [n_legal] + 1 [greedy] + 1 [explored] + 8 [taken_score]" in header
    assert "256 MiB / (B * max_turns)" in header


def test_abi_surface():
    """monsoon_rollout_explore, monsoon_explore and monsoon_explore_log are declared in the header and bound with the same
    shape; the log grows by the three arrays and keeps them through put."""
    header = open(os.path.join(REPO, "include", "monsoon.h")).read()
    decl = re.search(r"int monsoon_rollout_explore\(([^;]*)\);", header)
    assert decl and len(decl.group(1).split(",")) == 14
    res, args = _lib.SIGNATURES["monsoon_rollout_explore"]
    assert len(args) == 14 and res is _lib.ctypes.c_int
    assert args[:12] == _lib.SIGNATURES["monsoon_rollout_logged"][1]
    st = re.search(r"typedef struct \{([^}]*)\} monsoon_explore;", header)
    assert [f.split()[-1].rstrip(";") for f in re.findall(r"\w+\s+\w+;", st.group(1))] == [n for n, _ in _lib.Explore._fields_]
    assert _lib.ctypes.sizeof(_lib.Explore) == 16
    st = re.search(r"typedef struct \{([^}]*)\} monsoon_explore_log;", header)
    assert re.findall(r"\*\s*(\w+);", st.group(1)) == [n for n, _ in _lib.ExploreLog._fields_]
    a, b = RolloutLog.empty(3, 4, explore=True), RolloutLog.empty(2, 4, explore=True)
    b.greedy[:], b.explored[:], b.taken_score[:], b.action[:], b.steps[:] = 7, 1, 0.5, 9, 4
    a.put(np.array([0, 2]), b)
    assert a.greedy[:, 0].tolist() == [7, 255, 7] and a.explored[:, 0].tolist() == [1, 0, 1] and a.taken_score[2, 3] == 0.5
    assert np.isnan(a.taken_score[1]).all() and a.action[:, 0].tolist() == [9, 255, 9]
    plain = RolloutLog.empty(2, 4)
    assert plain.greedy is None and plain.explored is None and plain.taken_score is None
    with pytest.raises(ValueError, match="Explore rule"):
        game_log._log_columns(plain, ("action", "greedy"))
    assert game_log._log_columns(a, ("obs", "greedy", "explored")) == ["greedy", "explored"]
    assert "greedy" in game_log._want(("greedy",)) and "action" in game_log._want(("greedy",))
