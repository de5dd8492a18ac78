"""The work stack at depth, on the GPU: the positions of tests/golden/deep_steps.json.gz (tests/deep_steps.py: nested
evictions, the recursion guard, the deepest finite chain, decisions with many evicting candidates) through the stepping
kernels, each of which computes the base of its workgroup's eviction block in HBM itself.

The batch: 131 slots (two workgroups of the standard build's 64-lane API kernels and three slots of a third, nine of the
extended build's, seventeen of the large one's) -- the deep positions the build's record holds, again and again in
alternating order, every other slot a shallow filler game (the C5 family, heuristic self-play, a few decisions in): the
lanes of a workgroup sit at different depths, deep lanes lie on both sides of every workgroup boundary, and a write into
a neighbour's column of the block shows in the filler's hash.  Expected values: the fixture (the Python reference) for the
deep step, the recursive CPU oracle for everything else.  Positions of games against the scripted bot are left to the
rollout test (the API's expert_action draws for every loaded game at once, so they cannot be stepped in a mixed batch);
there they sit in batches with fillers like the others.
No test expects a GPU fault: every code is a per-game fault byte of a kernel that ends normally."""
import os
import re

import numpy as np
import pytest

try:
    # torch brings a HIP runtime of its own; the process must load it before libmonsoon_hip*.so pulls in the system's, or
    # torch finds no device afterwards.  In a run of the whole suite the collection of tests/test_distributed_cpu.py has
    # imported torch long before; this keeps the vector-env tests below running when the file is run on its own.
    import torch  # noqa: F401
except ImportError:
    pass

import deep_steps
import kernel_variants
import oracle_lib
import vs_expert_model
from c5_games import c5_games
from oracle_rollout import oracle_rollout_tier

pytestmark = pytest.mark.gpu

W0 = deep_steps.W0
N = 131
POS = deep_steps.positions()
BUILDS = [False, True, 2]
BUILD_IDS = [kernel_variants.BUILD_NAMES[b] for b in BUILDS]


def _fits(p, ext):
    return p["tier"] <= int(ext)


def _canon_hash(p):
    return oracle_lib.fnv1a64(bytes.fromhex(p["canon"]))


class Batch:
    """The slots of one build: per slot the game (seed, decks), its action prefix and the action of the compared step; the
    oracle at the positions (self.at) and what it gives for the step (self.want)."""

    def __init__(self, ext):
        from monsoon_amd.cards import CARD_IDS
        self.ext = ext
        deep = [p for p in POS if _fits(p, ext) and p["bot_side"] < 0]
        assert len(deep) >= 8
        big = {CARD_IDS.index("ua20"), CARD_IDS.index("b005")}
        self.slots = []
        k = turn = 0
        while len(self.slots) < N:
            j = len(self.slots) // 2
            if len(self.slots) % 2 == 0:
                order = deep if (j // len(deep)) % 2 == 0 else deep[::-1]
                p = order[j % len(deep)]
                self.slots.append(dict(p=p, seed=p["seed"], decks=np.array(p["decks"], dtype=np.uint8), prefix=list(p["prefix"]), action=p["action"]))
                turn = len(p["prefix"])
                continue
            while True:   # the next C5 game this build's record holds
                m, pairs = c5_games([k])
                k += 1
                if int(ext) >= 1 or not (big & set(pairs[0].reshape(-1).tolist())):
                    break
            want = min(turn, 24) + j % 5
            orc = oracle_lib.Oracle(1, extended=ext)
            assert orc.reset(0, int(m["seed"][0]), pairs[0, 0], pairs[0, 1]) == 0
            acts = [int(a) for a in orc.rollout(0, W0, W0, want + 1, trace=True)["actions"]]
            self.slots.append(dict(p=None, seed=int(m["seed"][0]), decks=pairs[0], prefix=acts[:-1], action=acts[-1]))
        self.seeds = np.array([s["seed"] for s in self.slots], dtype=np.uint32)
        self.decks = np.stack([s["decks"] for s in self.slots])
        self.at = self._oracle()
        self.hash_at = np.array([self.at.canon_hash(i) for i in range(N)], dtype=np.uint64)
        self.legal_at = np.stack([self.at.legal_mask(i) for i in range(N)])
        for i, s in enumerate(self.slots):
            if s["p"] is not None:
                assert int(self.hash_at[i]) == s["p"]["hash_before"]
        # the compared step: fixture values for the deep slots, the oracle's for the fillers
        stepped = self._oracle()
        self.want = []
        for i, s in enumerate(self.slots):
            f, r, d = stepped.step(i, s["action"])
            p = s["p"]
            if p is not None:
                assert f == deep_steps.expected_fault(p)
                row = dict(fault=f, reward=p["reward"], done=p["done"], hash=_canon_hash(p), legal=deep_steps.legal_of(p)) if f == 0 else dict(fault=f)
            else:
                row = dict(fault=f, reward=r, done=d, hash=stepped.canon_hash(i), legal=stepped.legal_mask(i)) if f == 0 else dict(fault=f)
            self.want.append(row)
        self._blobs = self._decided = None
        self._played = {}

    def _oracle(self):
        orc = oracle_lib.Oracle(N, extended=self.ext)
        for i, s in enumerate(self.slots):
            assert orc.reset(i, s["seed"], s["decks"][0], s["decks"][1]) == 0
            for a in s["prefix"]:
                assert orc.step(i, a)[0] == 0
        return orc

    def engine_at_positions(self, eng):
        """monsoon_reset, then the prefixes in lockstep through monsoon_step (255 parks a slot whose prefix is done)."""
        eng.reset(self.seeds, self.decks)
        for t in range(max(len(s["prefix"]) for s in self.slots)):
            a = np.array([s["prefix"][t] if t < len(s["prefix"]) else 255 for s in self.slots], dtype=np.uint8)
            _, _, f = eng.step(a)
            assert not f.any(), t
        assert np.array_equal(eng.state_hash(), self.hash_at)
        assert np.array_equal(eng.legal_mask(), self.legal_at)

    def blobs(self):
        """monsoon_state_save of every slot at its position (of a handle of the build's default variant)."""
        if self._blobs is None:
            from monsoon_amd.engine import BatchEngine
            eng = BatchEngine(N, extended=self.ext)
            try:
                self.engine_at_positions(eng)
                self._blobs = [eng.save_state(i) for i in range(N)]
            finally:
                eng.close()
        return self._blobs

    def decided(self):
        """Oracle.decide (action, score vector) and lookahead_faults at every position."""
        if self._decided is None:
            orc = self._oracle()
            self._decided = [orc.decide(i, W0)[:2] + (orc.lookahead_faults(i),) for i in range(N)]
        return self._decided

    def played(self, rounds):
        """Per slot after `rounds` more heuristic decisions on the oracle: (canonical hash, monsoon_game_faults' code -- the
        fault that stopped the game, else the first capacity code a look-ahead met --, the committed step's fault)."""
        if rounds not in self._played:
            orc = self._oracle()
            out = []
            for i in range(N):
                r = orc.rollout(i, W0, W0, rounds)
                out.append((orc.canon_hash(i), orc.game_fault(i), r["fault"]))
            self._played[rounds] = out
        return self._played[rounds]


_batches = {}


def batch(ext):
    if ext not in _batches:
        _batches[ext] = Batch(ext)
    return _batches[ext]


def _load(eng, b):
    eng.upload_weights(W0[None])
    for i, blob in enumerate(b.blobs()):
        eng.load_state(i, blob)
    eng.assign_players(np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32))
    assert np.array_equal(eng.state_hash(), b.hash_at)


@pytest.mark.parametrize("ext", BUILDS, ids=BUILD_IDS)
def test_api_step_kernel(ext):
    """monsoon_step (the API kernels: block base blockIdx.x * API_LANES * OVF_WORDS) with the deep actions of every slot in
    one call: fault, reward, done, monsoon_state_hash and monsoon_legal_mask."""
    from monsoon_amd.engine import BatchEngine
    b = batch(ext)
    eng = BatchEngine(N, extended=ext)
    try:
        b.engine_at_positions(eng)
        reward, done, fault = eng.step(np.array([s["action"] for s in b.slots], dtype=np.uint8))
        hashes, legal = eng.state_hash(), eng.legal_mask()
        deep = guard = 0
        for i, (s, w) in enumerate(zip(b.slots, b.want)):
            what = (i, s["p"] and (s["p"]["cls"], s["p"]["source"]), s["action"])
            assert int(fault[i]) == w["fault"] and int(fault[i]) != 29, (what, fault[i])
            if w["fault"] == 0:
                assert (int(reward[i]), int(done[i])) == (w["reward"], w["done"]), what
                assert int(hashes[i]) == w["hash"], what
                assert np.array_equal(legal[i], w["legal"]), what
            deep += s["p"] is not None and w["fault"] == 0
            guard += w["fault"] == 18
        assert deep >= 16 and guard >= 4
    finally:
        eng.close()


VARIANTS, VARIANT_IDS = kernel_variants.matrix()


@pytest.mark.parametrize("ext,u,w", VARIANTS, ids=VARIANT_IDS)
def test_k_play_decides_and_plays_across_the_deep_step(monkeypatch, ext, u, w):
    """Every hot-kernel variant, on the positions before the deep action.  monsoon_decide (it commits its choice): the action,
    the whole score vector bit for bit, monsoon_game_faults and the committed state against Oracle.decide / lookahead_faults
    and the oracle one decision on (the deep action is one of the candidates: its successor's features are in the vector,
    or 0.0 where the guard ended it).  monsoon_play_rounds_dev(2) across the
    step: a persistent grid of 8 with the call cut in two (the second half's blocks lie behind the first's: base
    (half * grid + block) * U * OVF_WORDS) and uncut, and a wavefront per game: the same hashes, the oracle's."""
    from monsoon_amd.engine import BatchEngine
    b = batch(ext)
    b.blobs()   # (saved on a handle of the default variant, before the variant is selected)
    kernel_variants.select(monkeypatch, u, w)
    eng = BatchEngine(N, extended=ext)
    try:
        assert eng.variant() == (u, w)
        _load(eng, b)
        action, best, scores = eng.decide(W0, want_scores=True)   # (decides and commits)
        faults, hashes = eng.game_faults(), eng.state_hash()
        saw_guard = 0
        for i, (s, (oa, oscores, olf), (h1, gf1, f1)) in enumerate(zip(b.slots, b.decided(), b.played(1))):
            legal = ~np.isnan(oscores)
            assert int(action[i]) == oa, i
            assert np.array_equal(np.isnan(scores[i]), ~legal), i
            assert np.array_equal(scores[i][legal].view(np.uint64), oscores[legal].view(np.uint64)), i
            assert best[i] == oscores[oa], i
            assert int(faults[i]) == gf1 and gf1 != 29, (i, faults[i], gf1)
            if f1 == 0:
                assert int(hashes[i]) == h1, i
            if s["p"] is not None and s["p"]["cls"] == "B":
                assert olf[s["action"]] == 18 and scores[i][s["action"]] == 0.0 and gf1 == 18
                saw_guard += 1
        assert saw_guard >= 4
    finally:
        eng.close()
    want = b.played(2)
    pop_parts, split_max = _launch_rule()
    assert pop_parts <= 8 < N and split_max >= 2 and N // 2 > 8   # MONSOON_GRID=8: persistent, and cut in two
    got = {}
    for grid, split in (("8", "2"), ("8", "0"), (None, None)):
        if grid is None:
            monkeypatch.delenv("MONSOON_GRID", raising=False)
            monkeypatch.delenv("MONSOON_SPLIT", raising=False)
        else:
            monkeypatch.setenv("MONSOON_GRID", grid)
            monkeypatch.setenv("MONSOON_SPLIT", split)
        eng = BatchEngine(N, extended=ext)
        try:
            _load(eng, b)
            eng.play_rounds(2)
            got[(grid, split)] = (eng.state_hash(), eng.game_faults(), eng.status())
        finally:
            eng.close()
    ref = got[("8", "2")]
    for key, g in got.items():
        for x, y in zip(g, ref):
            assert np.array_equal(x, y), key
    committed_deep = 0
    for i, (h, gf, f) in enumerate(want):
        assert int(ref[1][i]) == gf, (i, ref[1][i], gf)
        if f == 0:
            assert int(ref[0][i]) == h, i
        committed_deep += b.slots[i]["p"] is not None and b.slots[i]["p"]["committed"]
    assert committed_deep >= 4   # (heuristic games: the deep action is the one the decision commits)


def _launch_rule():
    """(POP_PARTS, SPLIT_MAX).  launch_play falls back silently (one launch, or a wavefront per game), and the ABI does not
    show which form ran: the inputs of its rule are asserted by the callers instead, read from the source.  A call of n
    games under MONSOON_GRID=g is persistent when POP_PARTS <= g < n and cut in two when SPLIT_MAX >= 2 and n / 2 > g; the
    rule itself, and k_play's block base for the second half, must still read as they did."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "monsoon_amd", "csrc")
    with open(os.path.join(csrc, "kernels.h")) as f:
        m = re.search(r"constexpr int POP_PARTS = (\d+), POP_STRIDE = \d+, SPLIT_MAX = (\d+);", f.read())
    pop_parts, split_max = int(m.group(1)), int(m.group(2))
    with open(os.path.join(csrc, "monsoon_hip.hip")) as f:
        host = f.read()
    assert "grid < n && grid >= POP_PARTS) ? 1 : 0;" in host and "if (n / parts <= grid) parts = 1;" in host
    assert "lds_init_wtab(b.wk_ovf + ((size_t)half * gridDim.x + blockIdx.x) * (U * OVF_WORDS));" in open(os.path.join(csrc, "kernels.h")).read()
    return pop_parts, split_max


def _source_games():
    """The games the class A and class B positions came from that a rollout can replay -- heuristic self-play (policy h) and
    heuristic against the bot (policy b; the search found positions there: none would have to be said here) -- each with
    the turn just past its last deep step.  Random-policy games cannot be replayed by a rollout."""
    games = {}
    for p in POS:
        if p["cls"] in "AB" and p["policy"] in "hb":
            g = games.setdefault(p["source"], dict(p=p, turns=0))
            g["turns"] = max(g["turns"], len(p["prefix"]) + 1)
    return games


ROLLOUT_N = 17   # matches per call: the source game in the nine even rows, eight distinct fillers between them


@pytest.mark.parametrize("ext", BUILDS, ids=BUILD_IDS)
def test_whole_games_through_the_rollout_kernels(monkeypatch, ext):
    """monsoon_rollout (k_play) and monsoon_rollout_vs_expert (k_play_vs: block base blockIdx.x * U * OVF_WORDS) on the games
    the class A and B positions came from.  max_turns belongs to the call, so every source game gets calls of its own, cut
    just past its deep step: 17 matches, the deep game in every even row and shallow C5 filler games (against the bot
    too, for a bot game) in the odd ones, once as a wavefront per game (17 workgroups) and once on a persistent grid of 8
    that hands the games out: the deep game runs in workgroups other than 0 next to shallow ones.  Counts, results, steps
    and faults equal oracle_rollout / vs_expert_model; every copy of the deep game gives the same row."""
    from monsoon_amd.cards import CARD_IDS
    from monsoon_amd.engine import BatchEngine
    games = {k: g for k, g in _source_games().items() if _fits(g["p"], ext)}
    big = {CARD_IDS.index("ua20"), CARD_IDS.index("b005")}
    fill = []
    k = 0
    while len(fill) < ROLLOUT_N // 2:
        fm, fp = c5_games([k])
        k += 1
        if int(ext) >= 1 or not (big & set(fp[0].reshape(-1).tolist())):
            fill.append((int(fm["seed"][0]), fp[0]))
    eng = BatchEngine(ROLLOUT_N, extended=ext)
    ran = dict(h=0, b=0)
    try:
        for src, g in sorted(games.items()):
            p = g["p"]
            pairs = np.stack([np.array(p["decks"], dtype=np.uint8)] + [d for _, d in fill])
            m = np.zeros(ROLLOUT_N, dtype=[("p1", "<i4"), ("p2", "<i4"), ("seed", "<u4"), ("deck", "<u4")])
            for j in range(ROLLOUT_N):
                m["seed"][j], m["deck"][j] = (p["seed"], 0) if j % 2 == 0 else (fill[j // 2][0], 1 + j // 2)
            if p["policy"] == "h":
                want = oracle_rollout_tier(W0[None], m, pairs, g["turns"], ext)
            else:
                m["p2"] = vs_expert_model.EXPERT
                want = vs_expert_model.rollout_tier(W0[None], m, pairs, g["turns"], ext)[:4]
            for grid in (None, "8"):
                if grid is None:
                    monkeypatch.delenv("MONSOON_GRID", raising=False)
                else:
                    monkeypatch.setenv("MONSOON_GRID", grid)
                    assert _launch_rule()[0] <= 8 < ROLLOUT_N   # persistent (rollouts are never cut)
                if p["policy"] == "h":
                    got = eng.rollout(W0[None], m, pairs, g["turns"], want_results=True)
                else:
                    got = eng.rollout_vs_expert(W0[None], m, pairs, g["turns"], want_results=True)
                faults = eng.rollout_faults(ROLLOUT_N)
                for x, y in zip(tuple(got) + (faults,), want):
                    assert np.array_equal(x, y), (src, grid, x, y)
                assert not (faults == 29).any()
                assert len(set(zip(got[1][::2].tolist(), got[2][::2].tolist(), faults[::2].tolist()))) == 1, (src, grid)
                if any(q["cls"] == "B" and q["source"] == src and q["committed"] for q in POS):
                    assert int(faults[0]) == 18, src
            ran[p["policy"]] += 1
    finally:
        eng.close()
    print("games:", ran)
    assert ran["h"] >= 4 and ran["b"] >= 2


def _torch():
    """torch, which must see the GPU: these tests carry the gpu marker, and a torch that finds no device on a GPU box is the
    load-order fault described at the head of this file, not a reason to skip."""
    import torch
    assert torch.cuda.is_available(), "torch finds no GPU: was libmonsoon_hip*.so loaded before torch?"
    return torch


@pytest.mark.parametrize("how", ["played", "restored"])
@pytest.mark.parametrize("ext,lanes", [(False, 0), (True, 0), (2, 0), (False, 4), (False, 64)],
                         ids=["standard", "extended", "large", "standard-lanes4", "standard-lanes64"])
def test_vec_env_steps_and_afterstates(ext, lanes, how):
    """The vector env without an opponent on the same batch.  The fillers are live slots: they play their prefixes in
    lockstep through VecEnv.step (255 parks a slot).  The deep slots either play theirs alongside ("played") or sit parked
    and then receive their positions by restore() ("restored"): the monsoon_state_save blobs of the API test's handle,
    turned into entries by env_snapshot_model.build_entry, loaded into the even slots between the live odd ones.  Then
    afterstates() at the positions -- every successor of every deep slot and of a few fillers, the deep one included,
    against env_afterstates_model -- and the deep actions in one step against vec_env_model (a step the guard ends closes
    the episode with fault 18 and the slot starts its next one).  On the standard build also on handles opened with 4 and
    64 lanes per game."""
    torch = _torch()
    from env_afterstates_model import AfterstatesModel, History, compare_slot
    from env_snapshot_model import build_entry
    from monsoon_amd import _lib
    from monsoon_amd.vec_env import EnvSnapshot, VecEnv
    from test_vec_env_gpu import assert_views_equal, host_views
    from vec_env_model import VecEnvModel
    b = batch(ext)
    blobs = b.blobs() if how == "restored" else None
    env = VecEnv(N, extended=ext, lanes_per_game=lanes)   # (k_env_after scales its block base by the lanes per workgroup)
    assert lanes == 0 or env.engine.variant()[0] == lanes
    try:
        views = env.reset(b.seeds, b.decks, opponent="none")
        hist = History()
        model = VecEnvModel(b.seeds, b.decks, opponent=0, extended=ext, on_commit=hist)
        assert_views_equal(host_views(views), model.views, "reset")
        deep = np.array([s["p"] is not None for s in b.slots])
        longest = max(len(s["prefix"]) for s in b.slots)
        for t in range(longest):
            a = np.array([s["prefix"][t] if t < len(s["prefix"]) else 255 for s in b.slots], dtype=np.uint8)
            want = model.step(a)
            if how == "restored":
                if not (a[~deep] != 255).any():
                    continue
                a = np.where(deep, 255, a).astype(np.uint8)
            got = env.step(torch.from_numpy(a).cuda())
            if how == "played" and (t % 16 == 15 or t == longest - 1):
                assert_views_equal(host_views(got), want, f"prefix step {t}")
        if how == "restored":
            assert np.array_equal(env.state_hash()[~deep], b.hash_at[~deep]) and (env.state_hash()[deep] != b.hash_at[deep]).all()
            version = int(_lib.load(int(ext)).monsoon_version())
            idx = np.nonzero(deep)[0]
            entries = np.stack([build_entry(int(ext), version, 0, b.decks[i], blobs[i]) for i in idx])
            assert entries.shape[1] == env.entry_bytes
            snap = EnvSnapshot(torch.from_numpy(entries).cuda(), len(idx), int(ext), env.entry_bytes)
            loaded = torch.zeros(len(idx), dtype=torch.uint8, device="cuda")
            got = host_views(env.restore(snap, dst=torch.from_numpy(idx.astype(np.int32)).cuda(), loaded=loaded))
            assert loaded.cpu().numpy().all()
            for k in ("obs", "legal", "obs_raises", "to_play", "episode"):
                assert np.array_equal(got[k], model.views[k]), k
        assert np.array_equal(env.state_hash(), b.hash_at) and np.array_equal(model.hashes(), b.hash_at)
        am = AfterstatesModel(model, hist, extended=ext)
        got = host_views(env.afterstates(156))
        assert np.array_equal(env.state_hash(), b.hash_at)
        seen, entries, guard = set(), 0, 0
        for i, s in enumerate(b.slots):
            key = id(s["p"]) if s["p"] is not None else None
            if key in seen or (key is None and i % 16 != 1):
                continue
            seen.add(key)
            want = am.slot(i, 156)
            entries += compare_slot(want, got, i, 156, ("afterstates", i))
            if s["p"] is not None:
                e = [x for x in want["entries"] if x["action"] == s["action"]]
                assert len(e) == 1 and e[0]["status"] == deep_steps.expected_fault(s["p"])
                guard += e[0]["status"] == 18
        assert entries > 100 and guard >= 4
        a = np.array([s["action"] for s in b.slots], dtype=np.uint8)
        got = host_views(env.step(torch.from_numpy(a).cuda()))
        want = model.step(a)
        assert_views_equal(got, want, "the deep step")
        assert np.array_equal(env.state_hash(), model.hashes())
        for i, (s, w) in enumerate(zip(b.slots, b.want)):
            assert int(got["fault"][i]) == w["fault"] and bool(got["done"][i]) == (w["fault"] != 0 or bool(w["done"])), i
            if w["fault"] == 0 and not w["done"]:
                assert int(env.state_hash()[i]) == w["hash"], i
    finally:
        env.close()


class _Counted:
    """What monsoon_debug_counters words 7 and 16 count, on the model: the opponent's committed steps and its look-ahead
    transitions (one per legal action of every decision)."""

    def __init__(self):
        self.commits = self.agent = self.lookahead = 0
        self.decided = {}

    def on_commit(self, j, episode, action, canon_hash):
        self.commits += 1

    def on_decide(self, j, action, mask):
        self.lookahead += sum(bin(int(x)).count("1") for x in mask)
        self.decided[j] = self.decided.get(j, 0) + 1


def _heuristic_slots(ext, agent_side):
    """The batch's slots of heuristic self-play games (the fixture's policy h, and every filler) whose compared decision is
    the OTHER side's: per slot the agent's own actions of the prefix, in order.  With W0 as the opponent the env plays the
    game the prefix records, and the opponent's turn after the agent's last action contains the deep decision."""
    b = batch(ext)
    orc = oracle_lib.Oracle(1, extended=ext)
    out = []
    for i, s in enumerate(b.slots):
        if s["p"] is not None and (s["p"]["policy"] != "h" or any(id(s["p"]) == id(x["p"]) for x, _, _ in out)):
            continue
        assert orc.reset(0, s["seed"], s["decks"][0], s["decks"][1]) == 0
        mine, opp_decisions = [], 0
        for a in s["prefix"]:
            if orc.to_play(0) == agent_side:
                mine.append(a)
            else:
                opp_decisions += 1
            orc.step(0, a)
        if orc.to_play(0) != agent_side:
            out.append((s, mine, opp_decisions + 1))
    return out


@pytest.mark.parametrize("ext,lanes,agent_side", [(False, 0, 0), (True, 0, 0), (True, 0, 1), (2, 0, 0), (2, 0, 1), (False, 4, 0), (False, 64, 0)],
                         ids=["standard-0", "extended-0", "extended-1", "large-0", "large-1", "standard-lanes4", "standard-lanes64"])
def test_vec_env_heuristic_opponent_decides_on_the_deep_position(ext, lanes, agent_side):
    """k_env_opp: the heuristic opponent (W0) meets the deep position in ITS decision, one agent ply after the env's last
    step: the agent replays its own side of the recorded self-play game, the opponent reproduces the other.  Views and state
    hashes against vec_env_heuristic_model, and the opponent's committed steps and look-ahead transitions
    (monsoon_debug_counters words 7 and 16).  Once more on handles opened with 4 and 64 lanes per game."""
    import ctypes
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    from test_vec_env_gpu import assert_views_equal, host_views
    from vec_env_heuristic_model import HeuristicVecEnvModel
    slots = _heuristic_slots(ext, agent_side)
    deep = [j for j, (s, _, _) in enumerate(slots) if s["p"] is not None]
    assert len(deep) >= 2 and len(slots) > len(deep), (len(deep), len(slots))
    n = len(slots)
    seed0 = np.array([s["seed"] for s, _, _ in slots], dtype=np.uint32)
    decks = np.stack([s["decks"] for s, _, _ in slots])
    cnt = _Counted()
    model = HeuristicVecEnvModel(seed0, W0[None], None, decks=decks, agent_side=agent_side, extended=ext, on_commit=cnt.on_commit, on_decide=cnt.on_decide)
    env = VecEnv(n, extended=ext, lanes_per_game=lanes)
    try:
        views = env.reset(seed0, decks, opponent="heuristic", agent_side=agent_side, opponent_weights=W0[None])
        assert_views_equal(host_views(views), model.views, "reset")
        for t in range(max(len(mine) for _, mine, _ in slots)):
            a = np.array([mine[t] if t < len(mine) else 255 for _, mine, _ in slots], dtype=np.uint8)
            cnt.agent += int(((a != 255) & (model.result == -2)).sum())
            got = host_views(env.step(torch.from_numpy(a).cuda()))
            assert_views_equal(got, model.step(a), f"step {t}")
            assert np.array_equal(env.state_hash(), model.hashes()), t
        for j, (s, _, decisions) in enumerate(slots):   # the opponent did decide on the compared position
            assert cnt.decided.get(j, 0) >= decisions or model.episode[j] > 0, (j, cnt.decided.get(j, 0), decisions)
        out = (ctypes.c_ulonglong * 192)()
        assert env.engine.lib.monsoon_debug_counters(env.engine.h, out) == 0
        assert (int(out[6]), int(out[7]), int(out[16])) == (cnt.agent, cnt.commits - cnt.agent, cnt.lookahead)
    finally:
        env.close()


@pytest.mark.parametrize("ext,agent_side", [(False, 0), (True, 0), (True, 1), (2, 1)], ids=["standard-0", "extended-0", "extended-1", "large-1"])
def test_vec_env_heuristic_opponent_after_restore(ext, agent_side):
    """The same meeting, by restore(): the deep slots sit parked while the fillers play, then receive the state ONE AGENT PLY
    before the opponent's deep decision -- monsoon_state_save blobs of a plain handle stepped through the prefix up to the
    agent's last action, turned into entries by env_snapshot_model.build_entry -- between the live filler slots.  One more
    step: the agent's last action, and the opponent's turn behind it holds the deep decision.  Views of the restored state
    and of the step, and every hash, against vec_env_heuristic_model (which plays the prefix)."""
    torch = _torch()
    from env_snapshot_model import build_entry
    from monsoon_amd import _lib
    from monsoon_amd.engine import BatchEngine
    from monsoon_amd.vec_env import EnvSnapshot, VecEnv
    from test_vec_env_gpu import assert_views_equal, host_views
    from vec_env_heuristic_model import HeuristicVecEnvModel
    slots = _heuristic_slots(ext, agent_side)
    n = len(slots)
    restored = [j for j, (s, mine, _) in enumerate(slots) if s["p"] is not None and mine]
    assert len(restored) >= 2 and n > 2 * len(restored)
    # the states one agent ply earlier: the prefix up to the agent's last action, on a plain handle
    orc = oracle_lib.Oracle(1, extended=ext)
    cuts = []
    for j in restored:
        s = slots[j][0]
        assert orc.reset(0, s["seed"], s["decks"][0], s["decks"][1]) == 0
        cut = None
        for k, a in enumerate(s["prefix"]):
            if orc.to_play(0) == agent_side:
                cut = k
            orc.step(0, a)
        cuts.append(cut)
    eng = BatchEngine(len(restored), extended=ext)
    try:
        eng.reset(np.array([slots[j][0]["seed"] for j in restored], dtype=np.uint32), np.stack([slots[j][0]["decks"] for j in restored]))
        for t in range(max(cuts)):
            a = np.array([slots[j][0]["prefix"][t] if t < c else 255 for j, c in zip(restored, cuts)], dtype=np.uint8)
            assert not eng.step(a)[2].any()
        blobs = [eng.save_state(i) for i in range(len(restored))]
    finally:
        eng.close()
    seed0 = np.array([s["seed"] for s, _, _ in slots], dtype=np.uint32)
    decks = np.stack([s["decks"] for s, _, _ in slots])
    cnt = _Counted()
    model = HeuristicVecEnvModel(seed0, W0[None], None, decks=decks, agent_side=agent_side, extended=ext, on_commit=cnt.on_commit, on_decide=cnt.on_decide)
    env = VecEnv(n, extended=ext)
    try:
        env.reset(seed0, decks, opponent="heuristic", agent_side=agent_side, opponent_weights=W0[None])
        steps = max(len(mine) for _, mine, _ in slots)
        is_restored = np.zeros(n, dtype=bool)
        is_restored[restored] = True

        def actions(t):   # the restored slots play their last action in the last step, the others from the first step on
            out = []
            for j, (_, mine, _) in enumerate(slots):
                k = t - (steps - len(mine)) if is_restored[j] else t
                out.append(mine[k] if 0 <= k < len(mine) else 255)
            return np.array(out, dtype=np.uint8)
        for t in range(steps - 1):
            a = actions(t)
            model.step(a)
            a = np.where(is_restored, 255, a).astype(np.uint8)
            if (a != 255).any():
                env.step(torch.from_numpy(a).cuda())
        version = int(_lib.load(int(ext)).monsoon_version())
        entries = np.stack([build_entry(int(ext), version, 0, decks[j], blob) for j, blob in zip(restored, blobs)])
        snap = EnvSnapshot(torch.from_numpy(entries).cuda(), len(restored), int(ext), env.entry_bytes)
        loaded = torch.zeros(len(restored), dtype=torch.uint8, device="cuda")
        got = host_views(env.restore(snap, dst=torch.from_numpy(np.array(restored, dtype=np.int32)).cuda(), loaded=loaded))
        assert loaded.cpu().numpy().all()
        for k in ("obs", "legal", "obs_raises", "to_play", "episode"):
            assert np.array_equal(got[k], model.views[k]), k
        assert np.array_equal(env.state_hash(), model.hashes())
        a = actions(steps - 1)
        assert (a[is_restored] != 255).all()
        before = dict(cnt.decided)
        got = host_views(env.step(torch.from_numpy(a).cuda()))
        assert_views_equal(got, model.step(a), "the step after the restore")
        assert np.array_equal(env.state_hash(), model.hashes())
        for j in restored:   # the opponent decided behind that action: the deep position was one of its decisions
            assert cnt.decided.get(j, 0) > before.get(j, 0) and cnt.decided[j] >= slots[j][2], j
    finally:
        env.close()


def _deep_scenarios():
    import gzip
    import json
    with gzip.open(os.path.join(deep_steps.GOLD, "deep_scenarios.json.gz"), "rt") as f:
        return json.load(f)


@pytest.mark.parametrize("builds", ["tier", "large"])
def test_k_debug_replays_the_deep_boards(builds):
    """k_debug (monsoon_debug_build + monsoon_debug_op), which takes the bare pointer of the eviction blocks: the deep
    positions as constructed boards (tests/golden/deep_scenarios.json.gz, recorded on the reference by
    oracle/pyref/gen_deep_scenarios.py with the recorder of its unit tests) -- the state before, ONE engine call
    (Player.play or Board.to_next_turn), the reference's canonical state after and its order of ability activations;
    fixture against HIP as in test_reference_unit_tests_as_scenarios_on_gpu.  With them the five constructed boards on which
    the reference completes chains of depth 30 to 40 (the guard's last finite level: 338 words, 39 evictions pending).
    Code 18 exactly where the reference raised RecursionError, 29 nowhere.  In slot 1 of a handle whose slot 0 holds a
    shallow game that must not change."""
    import scenario_lib as S
    from monsoon_amd.cards import deck_indices
    from monsoon_amd.engine import BatchEngine
    engs = {t: BatchEngine(2, extended=(2 if builds == "large" else bool(t))) for t in (0, 1)}
    try:
        deck = deck_indices("N12M")
        for e in engs.values():
            e.reset(np.array([5], dtype=np.uint32), np.stack([deck, deck]))
        h0 = {t: int(e.state_hash()[0]) for t, e in engs.items()}
        finite = guard = deepest = 0
        for case in _deep_scenarios():
            eng = engs[case["tier"]]
            for k, rec in enumerate(case["records"]):
                st = rec["before"]
                assert eng.debug_build(1, st["seed"], st["stream_pos"], S.encode_state(st)) == 0, (case["test"], k)
                f, log = eng.debug_op(1, S.encode_op(rec))
                assert f != 29, case["test"]
                if rec["raised"]:
                    assert f == case["count"]["fault"] == 18, (case["test"], f)
                    guard += 1
                    continue
                assert f == 0, (case["test"], k, rec["op"], f)
                assert eng.export(1).hex() == rec["after"], (case["test"], k, rec["op"])
                assert log == S.expected_log(rec), (case["test"], k, rec["op"])
                finite += case["count"]["seg"] >= 2
                deepest = max(deepest, case["count"]["depth"])
            assert int(eng.state_hash()[0]) == h0[case["tier"]], case["test"]
        assert finite >= 8 and guard >= 2 and deepest == 40
    finally:
        for e in engs.values():
            e.close()
