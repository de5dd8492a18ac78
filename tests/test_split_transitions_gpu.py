"""Split calls of monsoon_play_rounds_dev / monsoon_decide_round_dev (monsoon_hip.hip launch_play) where the cut, the
grid, the caller or the capture state changes between two calls: the joins of bind_device that tests/test_split_launch_gpu.py
never reaches because it reads between its calls (a read joins the streams) and keeps one MONSOON_GRID / MONSOON_SPLIT
for the life of an engine.

The reference is the CPU oracle (oracle_lib.Oracle, the recursive core), replayed segment by segment where weights,
players or games change; an engine with MONSOON_SPLIT=0 is a second witness.  The GPU side plays every sequence without a
read or a sync() between the calls under test and reads once at the end.  Every comparison is exact."""
import ctypes
import struct
import time

import numpy as np
import pytest

try:   # before the first handle exists: torch brings a HIP runtime of its own, and the one loaded first is the process's
    import torch
except ImportError:
    torch = None

import kernel_variants
import oracle_lib
from c5_games import C5_OVERFLOWING, c5_games
from monsoon_amd.cards import deck_indices, needs_extended_each
from test_split_launch_gpu import W2

pytestmark = pytest.mark.gpu

RUNNING = -2   # GameMeta.result of a game that still plays (kernels.h)
W_B = np.stack([np.random.RandomState(77).uniform(0, 1, 10), np.random.RandomState(78).uniform(0, 1, 10),
                np.random.RandomState(79).uniform(0, 1, 10)])


def n12m(n):
    d = deck_indices("N12M")
    return np.broadcast_to(np.stack([d, d]), (n, 2, 12)).copy()


class Replay:
    """The oracle's side of a call sequence.  play(k) is one call of k decisions on every loaded game: a game that has a
    winner or was stopped by a fault plays no more, as in k_play.  The kernel writes a winner's result when it next looks
    at the game (the round after the winning commit, in the same call or the next one), so a game that won with the very
    last decision offered to it still reads as running."""

    def __init__(self, seeds, decks, extended=False):
        self.n = len(seeds)
        self.orc = oracle_lib.Oracle(self.n, extended=extended)
        self.steps = np.zeros(self.n, dtype=np.int64)
        self.offered = np.zeros(self.n, dtype=np.int64)
        self.result = np.full(self.n, RUNNING, dtype=np.int64)
        self.stopped = np.zeros(self.n, dtype=bool)
        self.gone = 0   # decisions of games that were replaced since (monsoon_reset folds them into the statistics)
        for i in range(self.n):
            self.reset(i, seeds[i], decks[i])

    def reset(self, i, seed, pair):
        assert self.orc.reset(i, int(seed), pair[0], pair[1]) == 0
        self.steps[i] = self.offered[i] = 0
        self.result[i], self.stopped[i] = RUNNING, False

    def play(self, k, w, p1, p2):
        for i in range(self.n):
            if self.result[i] != RUNNING:
                continue
            if not self.stopped[i]:
                r = self.orc.rollout(i, w[p1[i]], w[p2[i]], k)
                self.steps[i] += r["steps"]
                if r["fault"]:
                    self.result[i], self.stopped[i] = -1, True
                    continue
                self.stopped[i] = self.orc.have_winner(i)
                if self.stopped[i] and r["steps"] < k:
                    self.result[i] = r["result"]
            else:   # the winner of the call before: this call's first look at the game writes the result
                self.result[i] = self.orc.rollout(i, w[p1[i]], w[p2[i]], 0)["result"]

    def expect(self):
        o, n = self.orc, self.n
        return dict(hashes=np.array([o.canon_hash(i) for i in range(n)], dtype=np.uint64),
                    to_play=np.array([o.to_play(i) for i in range(n)]), winner=np.array([int(o.have_winner(i)) for i in range(n)]),
                    faults=np.array([o.game_fault(i) for i in range(n)], dtype=np.uint8), steps=self.steps.copy(),
                    result=self.result.copy(), decisions=int(self.steps.sum()) + self.gone)


def start(n, seeds, decks, w, p2, extended=False):
    from monsoon_amd.engine import BatchEngine
    e = BatchEngine(n, extended=extended)
    e.reset(np.asarray(seeds, dtype=np.uint32), decks)
    e.upload_weights(w)
    e.assign_players(np.zeros(n, dtype=np.int32), np.asarray(p2, dtype=np.int32))
    e.reset_stats()
    return e


def read(e):
    """Everything a caller can read, once.  result and steps are the bookkeeping row inside the blob of monsoon_state_save
    (the blob's header is 8 bytes; GameMeta in kernels.h: result int8 at 8, steps uint16 at 12)."""
    out = dict(hashes=e.state_hash(), status=e.status(), faults=e.game_faults(), features=e.features(), stats=e.stats())
    blobs = [e.save_state(i) for i in range(e.n)]
    out["result"] = np.array([struct.unpack_from("<b", b, 16)[0] for b in blobs], dtype=np.int64)
    out["steps"] = np.array([struct.unpack_from("<H", b, 20)[0] for b in blobs], dtype=np.int64)
    return out


def assert_equals_oracle(got, want, what=""):
    assert np.array_equal(got["hashes"], want["hashes"]), (what, np.nonzero(got["hashes"] != want["hashes"])[0])
    assert np.array_equal(got["status"][:, 0], want["to_play"]) and np.array_equal(got["status"][:, 1], want["winner"]), what
    assert np.array_equal(got["faults"], want["faults"]), what
    assert np.array_equal(got["steps"], want["steps"]), what
    assert np.array_equal(got["result"], want["result"]), what
    assert got["stats"]["decisions"] == want["decisions"], what
    assert got["stats"]["capacity_faults"] == 0 and got["stats"]["lookahead_capacity_faults"] == 0, what


def assert_equals_witness(got, wit, what=""):
    for k in ("hashes", "status", "faults", "features", "result", "steps"):
        assert np.array_equal(got[k], wit[k], equal_nan=(k == "features")), (what, k)
    assert got["stats"] == wit["stats"], what


class Env:
    """MONSOON_GRID / MONSOON_SPLIT for the next call (launch_play reads both per call); split=False: the witness, whose
    calls are never cut whatever a sequence asks for."""

    def __init__(self, monkeypatch, split=True):
        self.mp, self.split = monkeypatch, split

    def __call__(self, grid, split="2"):
        self.mp.setenv("MONSOON_GRID", str(grid))
        self.mp.setenv("MONSOON_SPLIT", split if self.split else "0")


# ---- A: the cut changes in flight -----------------------------------------------------------------------------------
# (decisions, grid, MONSOON_SPLIT); 0 decisions = decide_round()
CUT_SEQUENCE = [(8, 16, "2"),    # cut
                (4, 32, "2"),    # cut, another grid: behind everything in flight; grow_ovf doubles under step 1
                (4, 32, "0"),    # one persistent launch: plays the second half's games on the handle's stream
                (0, 64, "2"),    # decide_round, cut (n / 2 = 65 > 64)
                (4, 128, "2"),   # one persistent launch (65 <= 128)
                (2, 256, "2"),   # a wavefront per game: leaves every parity alone
                (8, 16, "2"),    # cut again
                (8, 16, "2")]
CUT_DECISIONS = sum(max(k, 1) for k, _, _ in CUT_SEQUENCE)


@pytest.mark.parametrize("n", [130, 131])
def test_cut_changes_in_flight(monkeypatch, n):
    """One handle, eight calls, each cut differently from the one before (see CUT_SEQUENCE): the joins of launch_play for
    `parts != split_live` and `grid != split_grid`.  Without them an unsplit launch would play games [n/2, n) while the old
    second half still holds them, and a larger grid's first-half overflow blocks would lie over the old second half's.
    131 games: halves of 65 and 66."""
    assert CUT_DECISIONS == 39
    seeds, decks, p1, p2 = np.arange(n) + 21000, n12m(n), np.zeros(n, dtype=int), np.arange(n) % 2
    rep = Replay(seeds, decks)
    for k, _, _ in CUT_SEQUENCE:
        rep.play(max(k, 1), W2, p1, p2)
    want = rep.expect()
    # the oracle's side of the bargain: every game plays all 39 decisions, none finishes, none faults
    assert (want["steps"] == 39).all() and (want["result"] == RUNNING).all() and not want["winner"].any() and not want["faults"].any()
    got = {}
    for split in (True, False):
        env = Env(monkeypatch, split)
        env(16)
        e = start(n, seeds, decks, W2, p2)
        try:
            e.sync()
            t0 = time.perf_counter()
            for k, grid, s in CUT_SEQUENCE:
                env(grid, s)
                if k:
                    e.play_rounds(k)
                else:
                    e.decide_round()
            e.sync()
            wall_ms = 1000.0 * (time.perf_counter() - t0)
            ms, launches = e.kernel_time()
            got[split] = read(e)
        finally:
            e.close()
        print(f"n {n} split {split}: kernel {ms:.3f} ms in {launches} calls, wall {wall_ms:.3f} ms")
        assert launches == len(CUT_SEQUENCE)
        assert 0 < ms <= wall_ms   # the identity of drain_timing, over calls of mixed kinds
        assert_equals_oracle(got[split], want, split)
    assert np.array_equal(got[True]["features"], np.array([rep.orc.features(i) for i in range(n)]))
    assert_equals_witness(got[True], got[False])


# ---- B: a writer directly behind a split call -------------------------------------------------------------------------
@pytest.mark.parametrize("writer", ["load_state", "upload_weights", "upload_weights_grown", "assign_players", "reset"])
def test_writer_follows_split_call(monkeypatch, writer):
    """66 games, grid 16 (halves of 33): a split play_rounds(8), at once a writer, at once another split play_rounds(8), one
    read.  Each writer reaches the stream by its own path (monsoon_state_load, monsoon_upload_weights with and without a
    new table, monsoon_assign_players, monsoon_reset through fold_stats) and each relies on bind_device's join: were it
    missing, the writer would run under the second half of the first call."""
    n = 66
    seeds, decks, p1, p2 = np.arange(n) + 33000, n12m(n), np.zeros(n, dtype=int), np.arange(n) % 2
    new_seeds = np.arange(n) + 35000
    sub = [0, 32, 33, 65]
    rep = Replay(seeds, decks)
    rep.play(8, W2, p1, p2)
    assert (rep.steps == 8).all() and not rep.stopped.any()
    if writer == "load_state":
        for i in sub:
            rep.reset(i, seeds[i], decks[i])
        rep.play(8, W2, p1, p2)
    elif writer.startswith("upload_weights"):
        rep.play(8, W_B, p1, p2)
    elif writer == "assign_players":
        rep.play(8, W2, p1, 1 - p2)
    else:
        rep.gone = int(rep.steps.sum())
        for i in range(n):
            rep.reset(i, new_seeds[i], decks[i])
        rep.play(8, W2, p1, p2)
    want = rep.expect()
    assert (want["result"] == RUNNING).all() and not want["faults"].any()
    assert want["decisions"] == (16 * n - 8 * len(sub) if writer == "load_state" else 16 * n)
    got = {}
    for split in (True, False):
        Env(monkeypatch, split)(16)
        e = start(n, seeds, decks, W2, p2)
        try:
            fresh = [e.save_state(i) for i in sub] if writer == "load_state" else None
            e.play_rounds(8)
            if writer == "load_state":
                for i, b in zip(sub, fresh):
                    e.load_state(i, b)
            elif writer == "upload_weights":
                e.upload_weights(W_B[:2])   # as many rows as before: the table stays where it is
            elif writer == "upload_weights_grown":
                e.upload_weights(W_B)       # a third row: the table is freed and allocated anew
            elif writer == "assign_players":
                e.assign_players(p1.astype(np.int32), (1 - p2).astype(np.int32))
            else:
                e.reset(new_seeds.astype(np.uint32), decks)
                e.assign_players(p1.astype(np.int32), p2.astype(np.int32))
            e.play_rounds(8)
            got[split] = read(e)
        finally:
            e.close()
        assert_equals_oracle(got[split], want, (writer, split))
    assert_equals_witness(got[True], got[False], writer)


# ---- C: games that finish, in both halves -----------------------------------------------------------------------------
# C5 games (tests/c5_games.py) on decks the standard record holds that have a winner within 40 decisions of W2[0]
# self-play, found with the oracle: slot -> index k.  (Such games are rare: of the first 4 000 indices only 701 is one;
# these are the first twelve.)  The oracle's decisions per game, in slot order: 30 40 28 36 30 27 | 39 29 40 39 37 26.
FINISHING = {0: 701, 5: 6867, 11: 8131, 17: 11600, 23: 14606, 32: 16259,
             33: 17561, 40: 17842, 47: 20302, 54: 23108, 61: 24081, 65: 24585}


def test_finished_games_in_both_halves(monkeypatch):
    """66 games, grid 16: six games in each half end with a winner at different calls, so the halves are unequally long and
    pops land on games with nothing left to do; slots 0, 32, 33 and 65 are such games.  The others are N12M games, which
    do not finish.  Six calls of 8 decisions, then two more, which must leave the finished games alone."""
    n = 66
    slots = sorted(FINISHING)
    m, pairs = c5_games([FINISHING[s] for s in slots])
    assert not needs_extended_each(pairs).any()
    seeds, decks = np.arange(n) + 30000, n12m(n)
    seeds[slots], decks[slots] = m["seed"], pairs
    z = np.zeros(n, dtype=int)
    rep = Replay(seeds, decks)
    for _ in range(6):
        rep.play(8, W2, z, z)
    want = rep.expect()
    done = want["result"] != RUNNING
    for half in (slice(0, n // 2), slice(n // 2, n)):   # the oracle's side, before the GPU is touched
        assert done[half].sum() == 6 and want["winner"][half].sum() == 6
        assert (want["steps"][half][done[half]] < 48).all() and len(set(want["steps"][half][done[half]])) >= 3
        assert (want["steps"][half][~done[half]] == 48).all()
    assert np.array_equal(np.nonzero(done)[0], slots) and not want["faults"].any()
    assert set(want["result"][done]) == {0, 1}
    for _ in range(2):
        rep.play(8, W2, z, z)
    want2 = rep.expect()
    assert np.array_equal(want2["steps"][done], want["steps"][done]) and (want2["steps"][~done] == 64).all()
    got = {}
    for split in (True, False):
        Env(monkeypatch, split)(16)
        e = start(n, seeds, decks, W2[:1], z)
        try:
            for _ in range(6):
                e.play_rounds(8)
            a = read(e)
            for _ in range(2):
                e.play_rounds(8)
            b = read(e)
            got[split] = (a, b)
        finally:
            e.close()
        assert_equals_oracle(a, want, (split, "six calls"))
        assert_equals_oracle(b, want2, (split, "eight calls"))
        assert np.array_equal(b["hashes"][done], a["hashes"][done]) and np.array_equal(b["steps"][done], a["steps"][done])
        assert b["stats"]["decisions"] - a["stats"]["decisions"] == 16 * int((~done).sum())
        assert b["stats"]["games_finished"] == 12
    for x, y in zip(got[True], got[False]):
        assert_equals_witness(x, y)


# ---- D: every variant of every record build ----------------------------------------------------------------------------
VARIANTS, VARIANT_IDS = kernel_variants.matrix()
_variant_games = {}


def variant_games(ext):
    """40 games of a build and the oracle's replay of four calls of 6 decisions, computed once per build: N12M on the
    standard record, the C5 deck pairs of test_gpu_parity.py on the extended one (indices 0 .. 39) and on the large one
    (the pairs that outgrow the extended record, then indices 0 .. 19)."""
    if ext not in _variant_games:
        n = 40
        if ext is False:
            seeds, decks = np.arange(n) + 41000, n12m(n)
        else:
            m, decks = c5_games(list(range(n)) if ext is True else C5_OVERFLOWING + list(range(n - len(C5_OVERFLOWING))))
            seeds = m["seed"].astype(np.int64)
        p1, p2 = np.zeros(n, dtype=int), np.arange(n) % 2
        rep = Replay(seeds, decks, extended=ext)
        for _ in range(4):
            rep.play(6, W2, p1, p2)
        want = rep.expect()
        assert (want["faults"] < 16).all()   # no limit of the build's record on these decks: the GPU must report none either
        assert want["steps"].max() == 24
        _variant_games[ext] = (seeds, decks, p2, want)
    return _variant_games[ext]


@pytest.mark.parametrize("ext,u,w", VARIANTS, ids=VARIANT_IDS)
def test_split_on_every_variant(monkeypatch, ext, u, w):
    """40 games, grid 16 (halves of 20), four split calls of 6 decisions without a read: the overflow offset of the second
    half and grow_ovf's size depend on U, and the extended and large builds have their own PlayLds."""
    seeds, decks, p2, want = variant_games(ext)
    kernel_variants.select(monkeypatch, u, w)
    Env(monkeypatch)(16)
    e = start(len(seeds), seeds, decks, W2, p2, extended=ext)
    try:
        assert e.variant() == (u, w)
        for _ in range(4):
            e.play_rounds(6)
        got = read(e)
    finally:
        e.close()
    assert_equals_oracle(got, want, (ext, u, w))


# ---- E: a captured call, replayed ---------------------------------------------------------------------------------------
def _kernel_nodes(graph):
    """(nodes, kernel nodes) of a captured graph."""
    hip = ctypes.CDLL("libamdhip64.so.7")   # the runtime torch and this library share (one soname per process)
    raw = ctypes.c_void_p(graph.raw_cuda_graph())
    nn = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(raw, None, ctypes.byref(nn)) == 0
    nodes = (ctypes.c_void_p * max(nn.value, 1))()
    assert hip.hipGraphGetNodes(raw, nodes, ctypes.byref(nn)) == 0
    kernels = 0
    for i in range(nn.value):
        kind = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(nodes[i]), ctypes.byref(kind)) == 0
        kernels += kind.value == 0   # hipGraphNodeTypeKernel
    return nn.value, kernels


def test_captured_play_rounds_replays(monkeypatch):
    """A play_rounds(4) captured into a graph and replayed three times in a row, between eager split calls.  A captured
    persistent launch cannot be replayed twice (its parity is fixed in the graph, so the second replay starts from the
    first one's pop counts and plays one game per wavefront); launch_play records the form without counters instead, one
    launch on the handle's stream, untimed.  The capture itself plays nothing: 4 + 3 x 4 + 4 = 20 decisions per game."""
    if torch is None or not torch.cuda.is_available():
        pytest.skip("needs torch and a GPU")
    from test_vec_env_gpu import _graph_is_a_chain
    n = 66
    seeds, decks, p1, p2 = np.arange(n) + 52000, n12m(n), np.zeros(n, dtype=int), np.arange(n) % 2
    rep = Replay(seeds, decks)
    for _ in range(5):
        rep.play(4, W2, p1, p2)
    want = rep.expect()
    assert (want["steps"] == 20).all() and (want["result"] == RUNNING).all() and not want["faults"].any()
    Env(monkeypatch)(16)
    e = start(n, seeds, decks, W2, p2)
    try:
        e.play_rounds(4)   # eager and split: the warm-up
        # fetched after the last eager call: the getter joins the streams
        s = torch.cuda.ExternalStream(e.stream_ptr(), device=torch.device("cuda", e.device))
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(g, stream=s):
            e.play_rounds(4)
        nodes, edges = _graph_is_a_chain(torch, g)
        assert (nodes, edges) == (1, 0) and _kernel_nodes(g) == (1, 1)
        g.instantiate()
        with torch.cuda.stream(s):   # a replay goes to torch's current stream: the handle's
            for _ in range(3):
                g.replay()
        e.play_rounds(4)   # eager and split again, behind the replays on the handle's stream
        e.sync()
        ms, launches = e.kernel_time()
        got = read(e)
    finally:
        e.close()
    assert launches == 2 and ms > 0   # the two eager calls; nothing of the handle's timing went into the graph
    assert_equals_oracle(got, want)


# ---- F: smaller ones ----------------------------------------------------------------------------------------------------
def test_monsoon_split_values(monkeypatch):
    """MONSOON_SPLIT is clamped to [1, SPLIT_MAX]: "1" and "-5" are one launch, "3" is two halves.  Whatever it says, the
    games are the oracle's."""
    n = 40
    seeds, decks, p1, p2 = np.arange(n) + 61000, n12m(n), np.zeros(n, dtype=int), np.arange(n) % 2
    rep = Replay(seeds, decks)
    for k in (4, 4, 1, 4):
        rep.play(k, W2, p1, p2)
    want = rep.expect()
    assert (want["steps"] == 13).all() and not want["faults"].any()
    got = {}
    for value in ("1", "3", "-5", "0", "2"):
        monkeypatch.setenv("MONSOON_GRID", "16")
        monkeypatch.setenv("MONSOON_SPLIT", value)
        e = start(n, seeds, decks, W2, p2)
        try:
            e.play_rounds(4)
            e.play_rounds(4)
            e.decide_round()
            e.play_rounds(4)
            got[value] = read(e)
        finally:
            e.close()
        assert_equals_oracle(got[value], want, value)
    for value in ("1", "3", "-5", "0"):
        assert_equals_witness(got[value], got["2"], value)


def test_kernel_time_across_kinds_of_calls(monkeypatch):
    """drain_timing takes pair i - 1 whatever call it timed: a split call, a rollout of two batches on the same handle (it is
    timed and drains itself, once per batch), new games, a split call.  launches counts the timed calls, the time stays
    inside the wall time, and both the rollout and the games around it are the oracle's."""
    n, n_matches = 66, 100
    seeds, decks, z = np.arange(n) + 71000, n12m(n), np.zeros(n, dtype=int)
    new_seeds = np.arange(n) + 72000
    matches = np.zeros(n_matches, dtype=[("p1", "<i4"), ("p2", "<i4"), ("seed", "<u4"), ("deck", "<u4")])
    matches["seed"] = np.arange(n_matches) + 73000
    roll = Replay(matches["seed"], n12m(n_matches))
    roll.play(30, W2, np.zeros(n_matches, dtype=int), np.zeros(n_matches, dtype=int))
    first = Replay(seeds, decks)
    first.play(8, W2, z, z)
    rep = Replay(new_seeds, decks)
    rep.play(8, W2, z, z)
    rep.gone = int(first.steps.sum() + roll.steps.sum())
    want = rep.expect()
    assert (want["steps"] == 8).all() and (roll.steps == 30).all() and not roll.stopped.any()
    Env(monkeypatch)(16)
    e = start(n, seeds, decks, W2[:1], z)
    try:
        e.sync()
        t0 = time.perf_counter()
        e.play_rounds(8)
        _, results, steps = e.rollout(W2[:1], matches, decks[:1], 30, want_results=True)
        e.reset(new_seeds.astype(np.uint32), decks)
        e.assign_players(z.astype(np.int32), z.astype(np.int32))
        e.play_rounds(8)
        e.sync()
        wall_ms = 1000.0 * (time.perf_counter() - t0)
        ms, launches = e.kernel_time()
        got = read(e)
    finally:
        e.close()
    print(f"kernel {ms:.3f} ms in {launches} calls, wall {wall_ms:.3f} ms")
    assert launches == 2 + 2   # the split calls and one launch per rollout batch (66 + 34 matches)
    assert 0 < ms <= wall_ms
    assert np.array_equal(steps, roll.steps) and (results == -1).all()   # 30 decisions each, no winner: draws
    assert_equals_oracle(got, want)


def test_destroy_under_a_split_call(monkeypatch):
    """close() with both halves of a split call in flight: monsoon_destroy waits for both streams before it frees what they
    work on.  A fresh engine then plays the same games as the oracle does."""
    n = 66
    seeds, decks, p1, p2 = np.arange(n) + 81000, n12m(n), np.zeros(n, dtype=int), np.arange(n) % 2
    rep = Replay(seeds, decks)
    rep.play(8, W2, p1, p2)
    want = rep.expect()
    Env(monkeypatch)(16)
    e = start(n, seeds, decks, W2, p2)
    e.play_rounds(8)
    e.close()
    e = start(n, seeds, decks, W2, p2)
    try:
        e.play_rounds(8)
        got = read(e)
    finally:
        e.close()
    assert_equals_oracle(got, want)
