"""Split calls of monsoon_play_rounds_dev / monsoon_decide_round_dev (monsoon_hip.hip launch_play): a call whose halves
are both still persistent launches plays games [0, n/2) on the handle's stream and [n/2, n) on a second one, so that
the next call's first half fills the drain of this call's second.  Games are independent, so nothing a caller can read
may depend on the cut: every case plays the same call sequence on an engine with the split on (MONSOON_SPLIT=2) and on
one with it off (MONSOON_SPLIT=0), from the same seeds and decks, and compares everything.  MONSOON_GRID forces a small
persistent grid (both are read per call), so small batches are cut.  A call is cut when n / 2 > grid: with a grid of 8,
n = 18 is the smallest batch that is (halves of 9 and 9); 17 (8 and 9) is not, its first half would be a launch of one
wavefront per game."""
import os
import time

import numpy as np
import pytest

import oracle_lib
from monsoon_amd.cards import deck_indices

pytestmark = pytest.mark.gpu

W2 = np.stack([np.random.RandomState(2024).uniform(0, 1, 10), np.random.RandomState(5).uniform(0, 1, 10)])


class Pair:
    """Two engines with the same games, the split on for one and off for the other; do() makes the same call on both."""

    def __init__(self, monkeypatch, n, grid, seed0):
        from monsoon_amd.engine import BatchEngine
        self.mp, self.n = monkeypatch, n
        monkeypatch.setenv("MONSOON_GRID", str(grid))
        self.deck = deck_indices("N12M")
        self.engines = [(BatchEngine(n), "2"), (BatchEngine(n), "0")]
        self.do(lambda e: e.reset(np.arange(n, dtype=np.uint32) + seed0, np.stack([self.deck, self.deck])))
        self.do(lambda e: e.upload_weights(W2))
        self.do(lambda e: e.assign_players(np.zeros(n, dtype=np.int32), (np.arange(n) % 2).astype(np.int32)))

    def do(self, f):
        out = []
        for e, split in self.engines:
            self.mp.setenv("MONSOON_SPLIT", split)
            out.append(f(e))
        return out

    def same(self, what=""):
        """Everything a caller can read is equal on the two engines; returns the split engine's hashes."""
        h = self.do(lambda e: e.state_hash())
        assert np.array_equal(h[0], h[1]), what
        for name in ("status", "features", "game_faults"):
            a, b = self.do(lambda e: getattr(e, name)())
            assert np.array_equal(a, b, equal_nan=(name == "features")), (what, name)
        a, b = self.do(lambda e: e.stats())
        assert a == b, what
        return h[0]

    def close(self):
        for e, _ in self.engines:
            e.close()


@pytest.mark.parametrize("n", [1, 15, 17, 18, 19])
def test_split_fallback(monkeypatch, n):
    """Grid 8: 1, 15 and 17 games fall back to the single launch, 18 and 19 are the smallest batches that are cut."""
    p = Pair(monkeypatch, n, 8, 4000)
    try:
        for k in range(3):
            p.do(lambda e: e.play_rounds(3))
            p.do(lambda e: e.decide_round())
        h = p.same(n)
        st = p.engines[0][0].stats()
        assert st["decisions"] > 0 and len(h) == n
    finally:
        p.close()


def test_sub_batch_boundary(monkeypatch):
    """257 games, grid 16: halves of 128 and 129.  Reads between the calls join the two streams; calls of one decision and
    of several alternate (under the forced MONSOON_GRID they share one grid: the join for a changed grid or cut is pinned
    in test_split_transitions_gpu.py) and a reset replaces games under both halves."""
    n = 257
    p = Pair(monkeypatch, n, 16, 7000)
    sub = np.array([0, 1, 126, 127, 128, 129, 130, 255, 256])
    try:
        h_init = p.same("initial")
        fresh = p.do(lambda e: [e.save_state(int(i)) for i in sub])
        p.do(lambda e: e.play_rounds(3))
        h0 = p.same("after play_rounds(3)")
        p.do(lambda e: e.play_rounds(1))
        p.do(lambda e: e.decide_round())
        p.do(lambda e: e.play_rounds(8))
        h1 = p.same("after the mixed calls")
        assert (h0 != h1)[sub].all()   # the games either side of the cut and at the ends of both halves moved on
        # the games around the cut and at the ends of both halves start again (their saved initial states come back)
        for (e, _), bl in zip(p.engines, fresh):
            for i, b in zip(sub, bl):
                e.load_state(int(i), b)
        h1b = p.same("after the reset of a subset")
        assert np.array_equal(h1b[sub], h_init[sub]) and np.array_equal(np.delete(h1b, sub), np.delete(h1, sub))
        p.do(lambda e: e.play_rounds(2))
        h2 = p.same("after play_rounds(2)")
        assert (h2 != h1b)[sub].all()
    finally:
        p.close()


@pytest.fixture(scope="module")
def long_run():
    """30 calls of play_rounds(8) on 512 games (grid 16: halves of 256) without a synchronisation in between, split on and
    off: the hashes, kernel_time() and the wall time around the calls, and the CPU oracle's replay of the same games."""
    from monsoon_amd.engine import BatchEngine
    n, calls = 512, 30
    deck = deck_indices("N12M")
    old = {k: os.environ.get(k) for k in ("MONSOON_GRID", "MONSOON_SPLIT")}
    os.environ["MONSOON_GRID"] = "16"
    out = {}
    try:
        for split in ("2", "0"):
            os.environ["MONSOON_SPLIT"] = split
            e = BatchEngine(n)
            try:
                e.reset(np.arange(n, dtype=np.uint32) + 90000, np.stack([deck, deck]))
                e.upload_weights(W2[:1])
                e.assign_players(np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32))
                e.reset_stats()
                e.sync()
                t0 = time.perf_counter()
                for _ in range(calls):
                    e.play_rounds(8)
                e.sync()
                wall_ms = 1000.0 * (time.perf_counter() - t0)
                out[split] = dict(kernel_time=e.kernel_time(), wall_ms=wall_ms, hashes=e.state_hash(), status=e.status(),
                                  faults=e.game_faults(), stats=e.stats())
            finally:
                e.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    orc = oracle_lib.Oracle(n)
    for i in range(n):
        orc.reset(i, 90000 + i, deck, deck)
    # a game plays until it has a winner or a fault stops it, 8 x 30 decisions at the most
    total, ores, osteps, ohash = orc.rollout_batch(n, W2[0], 8 * calls, 16)
    out["oracle"] = dict(hashes=ohash, results=ores, steps=osteps, lookahead=total)
    return out


@pytest.mark.parametrize("split", ["2", "0"])
def test_thirty_calls_equal_the_oracle(long_run, split):
    """Fifteen parity flips of both counter pairs, nothing read in between: the final states are the CPU oracle's after
    the same 240 decisions per game."""
    r, o = long_run[split], long_run["oracle"]
    assert np.array_equal(r["hashes"], o["hashes"])
    assert r["stats"] == long_run["0"]["stats"] and r["stats"]["decisions"] > 0
    assert r["stats"]["capacity_faults"] == 0 and r["stats"]["lookahead_capacity_faults"] == 0
    assert np.array_equal(long_run["2"]["status"], long_run["0"]["status"])
    assert np.array_equal(long_run["2"]["faults"], long_run["0"]["faults"])


@pytest.mark.parametrize("split", ["2", "0"])
def test_timing_identity(long_run, split):
    """kernel_time() counts API calls, and consecutive split calls never count the same wall time twice: the total cannot
    exceed the wall time around the calls and the final synchronisation (an identity of the rule in drain_timing)."""
    ms, launches = long_run[split]["kernel_time"]
    print(f"split {split}: kernel {ms:.3f} ms in {launches} launches, wall {long_run[split]['wall_ms']:.3f} ms")
    assert launches == 30
    assert 0 < ms <= long_run[split]["wall_ms"]


def test_two_handles_alternating(monkeypatch):
    """Two handles alive at once, both splitting, called in turn: each plays what it plays alone."""
    from monsoon_amd.engine import BatchEngine
    n = 257
    monkeypatch.setenv("MONSOON_GRID", "16")
    monkeypatch.setenv("MONSOON_SPLIT", "2")
    deck = deck_indices("N12M")

    def start(seed0):
        e = BatchEngine(n)
        e.reset(np.arange(n, dtype=np.uint32) + seed0, np.stack([deck, deck]))
        e.upload_weights(W2)
        e.assign_players(np.zeros(n, dtype=np.int32), (np.arange(n) % 2).astype(np.int32))
        return e

    def read(e):
        return e.state_hash(), e.status(), e.features(), e.game_faults(), e.stats()

    alone = []
    for seed0 in (11000, 12000):
        e = start(seed0)
        try:
            for _ in range(6):
                e.play_rounds(4)
            e.decide_round()
            alone.append(read(e))
        finally:
            e.close()
    a, b = start(11000), start(12000)
    try:
        for _ in range(6):
            a.play_rounds(4)
            b.play_rounds(4)
        a.decide_round()
        b.decide_round()
        for e, ref in ((a, alone[0]), (b, alone[1])):
            got = read(e)
            for x, y in zip(got[:4], ref[:4]):
                assert np.array_equal(x, y, equal_nan=True)
            assert got[4] == ref[4]
    finally:
        a.close()
        b.close()
