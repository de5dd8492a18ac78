"""The Python layer's one tier ladder (fitness._ladder) through its two entries, fitness.tiered_rollout and
game_log.logged_rollout, on a synthetic fault table; and the rule of replace_capacity_faulted next to the ladder's."""
import numpy as np

from monsoon_amd import game_log
from monsoon_amd.cards import CARD_INDEX, deck_indices, needs_extended_each
from monsoon_amd.engine import RolloutLog
from monsoon_amd.fitness import MATCH_DTYPE, replace_capacity_faulted, tiered_rollout

# fault code of game `seed` on record `tier`: 0 plays through, 16 / 23 / 29 are limits of a record, 18 is the recursion guard
FAULT = {0: (0, 0, 0), 1: (16, 0, 0), 2: (18, 18, 18), 3: (23, 23, 0), 4: (None, 29, 29), 5: (None, 0, 0)}
T = 4   # max_turns of the fake log


def _schedule():
    """Six games over two rows; games 0-3 on a standard deck pair, 4 and 5 on a pair holding ua20 (the extended record)."""
    std = deck_indices("N12M")
    ext = std.copy()
    ext[0] = CARD_INDEX["ua20"]
    pairs = np.stack([np.stack([std, std]), np.stack([std, ext])])
    assert needs_extended_each(pairs).tolist() == [False, True]
    m = np.zeros(6, dtype=MATCH_DTYPE)
    m["seed"] = np.arange(6)
    m["p1"], m["p2"] = m["seed"] % 2, 1 - m["seed"] % 2
    m["deck"] = [0, 0, 0, 0, 1, 1]
    return m, pairs


def _played(tier, sub, n_rows=2):
    """(counts, results, steps, faults) of a call: a faulted game is a draw, any other a win of FIRST; steps name the tier."""
    f = np.array([FAULT[int(s)][tier] for s in sub["seed"]], dtype=np.uint8)
    r = np.where(f != 0, -1, 0).astype(np.int8)
    c = np.zeros((n_rows, 3), dtype=np.int32)
    np.add.at(c[:, 0], sub["p1"], r == 0)
    np.add.at(c[:, 1], sub["p1"], r == -1)
    np.add.at(c[:, 2], sub["p1"], 1)
    return c, r, (10 * tier + sub["seed"]).astype(np.int32), f


def _call(tier, sub, sub_pairs, pairs):
    names = ["std" if np.array_equal(p, pairs[0]) else "ext" if np.array_equal(p, pairs[1]) else "?" for p in sub_pairs]
    return tier, sub["seed"].tolist(), sub["deck"].tolist(), names


class _FakeEngine:
    """rollout_logged / rollout_faults of a BatchEngine over the fault table; every log row holds the tier that wrote it."""

    def __init__(self, tier, calls, pairs):
        self.tier, self.calls, self.pairs, self.faults = tier, calls, pairs, None

    def rollout_logged(self, weights, sub, sub_pairs, max_turns):
        self.calls.append(_call(self.tier, sub, sub_pairs, self.pairs))
        c, r, s, self.faults = _played(self.tier, sub, len(weights))
        log = RolloutLog.empty(len(sub), max_turns)
        log.action[:], log.score[:], log.n_legal[:], log.steps[:] = self.tier, self.tier, self.tier, s
        return c, r, s, log

    def rollout_faults(self, n):
        assert n == len(self.faults)
        return self.faults


def test_tiered_and_logged_rollout_climb_the_same_ladder():
    """One fault table through both entries of the ladder: the same calls (tier, seeds, remapped deck column, deck pairs
    handed), counts, results, steps and faults, and the log rows of a replayed game are those of the last tier that played
    it.  The expected calls follow from the rule by hand: games 0-3 start on the standard record, 4 and 5 on the extended
    one; rung 1 takes the record-limited games below it (1: code 16, 3: code 23; not 2, whose 18 is the recursion guard),
    rung 2 those still limited below it (3: 23 again on the extended record; 4: 29 there), and 4 keeps its 29."""
    m, pairs = _schedule()
    expected = [(0, [0, 1, 2, 3], [0, 0, 0, 0], ["std"]),
                (1, [4, 5], [0, 0], ["ext"]),
                (1, [1, 3], [0, 0], ["std"]),
                (2, [3, 4], [0, 1], ["std", "ext"])]
    calls = []

    def play(tier, sub, sub_pairs):
        calls.append(_call(tier, sub, sub_pairs, pairs))
        return _played(tier, sub)
    counts, results, steps, faults, replays, sizes = tiered_rollout(play, 2, m, pairs)
    assert calls == expected and replays == 4 and sizes == [4, 2]
    assert counts.dtype == np.int64 and counts.tolist() == [[1, 2, 3], [3, 0, 3]]
    assert results.tolist() == [0, 0, -1, 0, -1, 0] and steps.tolist() == [0, 11, 2, 23, 24, 15] and faults.tolist() == [0, 0, 18, 0, 29, 0]

    logged_calls, engines = [], {}
    c2, r2, s2, f2, log = game_log.logged_rollout(lambda t: engines.setdefault(t, _FakeEngine(t, logged_calls, pairs)),
                                                  np.zeros((2, 10)), m, pairs, T)
    assert logged_calls == expected
    assert c2.dtype == np.int64 and np.array_equal(c2, counts)
    assert np.array_equal(r2, results) and np.array_equal(s2, steps) and np.array_equal(f2, faults)
    last_tier = [0, 1, 0, 2, 2, 1]
    assert log.action.shape == (6, T) and (log.action == np.array(last_tier, dtype=np.uint8)[:, None]).all()
    assert (log.score == np.array(last_tier, dtype=np.float64)[:, None]).all() and (log.n_legal == np.array(last_tier)[:, None]).all()
    assert np.array_equal(log.steps, steps)


def test_replace_capacity_faulted_replays_the_recursion_guard_and_the_ladder_does_not():
    """The two rules differ on code 18 on purpose: replace_capacity_faulted takes every code >= 16, the ladder
    (record_limited) leaves the recursion guard alone."""
    m, pairs = _schedule()
    one = m[2:3]   # the game whose every record ends on 18
    calls = []

    def play(tier, sub, sub_pairs):
        calls.append(tier)
        return _played(tier, sub)
    counts, results, steps, faults, replays, _ = tiered_rollout(play, 2, one, pairs)
    assert (calls, replays, faults.tolist()) == ([0], 0, [18])
    again = []
    counts, results, steps, faults = (np.array(x) for x in _played(0, one))
    n = replace_capacity_faulted(counts, results, steps, faults, one, lambda sub: again.append(sub["seed"].tolist()) or _played(1, sub))
    assert (n, again, steps.tolist(), counts.tolist()) == (1, [[2]], [12], [[0, 1, 1], [0, 0, 0]])
