"""CPU tests of the vector env (include/monsoon.h monsoon_env_*, monsoon_amd/vec_env.py): the ABI is exported and bound,
VecEnv refuses to run without a device, and the Python model the GPU tests compare against (tests/vec_env_model.py) is
pinned to the reference's own bot-vs-bot traces and to fresh oracle resets."""
import numpy as np
import pytest

from monsoon_amd.cards import C5_STREAM_XOR, CARD_IDS, FAULT_CARDS, UNSUPPORTED, deck_indices
from vec_env_model import BOT_BOUND, FAULT_BOT_BOUND, VecEnvModel

ENV_SYMBOLS = ("monsoon_env_reset", "monsoon_env_step_dev")


def test_env_symbols_exported_and_bound():
    from monsoon_amd import _lib
    for ext in (0, 1, 2):
        lib = _lib.load(ext)
        for name in ENV_SYMBOLS:
            assert hasattr(lib, name), (ext, name)
    for name in ENV_SYMBOLS:
        assert name in _lib.SIGNATURES
    # the ctypes structs have the C layout: 5 int32 + 128 bytes, 12 pointers
    assert _lib.ctypes.sizeof(_lib.EnvConfig) == 20 + 128
    assert _lib.ctypes.sizeof(_lib.EnvViews) == 12 * 8


def test_fault_code_of_the_bot_bound_is_declared():
    import os
    from conftest import REPO
    src = open(os.path.join(REPO, "monsoon_amd", "csrc", "msb_base.h")).read()
    assert f"FAULT_BOT_BOUND = {FAULT_BOT_BOUND}," in src and BOT_BOUND == 64


def test_vec_env_has_no_cpu_fallback():
    import torch
    from monsoon_amd import MonsoonError
    from monsoon_amd.vec_env import VecEnv
    with pytest.raises(MonsoonError, match="no usable HIP device"):
        VecEnv(4, device=99)
    if not torch.cuda.is_available():
        for ext in (0, 1):
            with pytest.raises(MonsoonError, match="no usable HIP device"):
                VecEnv(4, extended=ext)


def _expert_pool():
    """The pool the reference's expert traces drew their second half from: every card of the standard record but the three
    whose int(card) raises, in card-id order."""
    return np.array([i for i, c in enumerate(CARD_IDS) if c not in UNSUPPORTED and c not in FAULT_CARDS], dtype=np.uint8)


def bot_bound_cut(actions, agent_side):
    """Where the env's bot guard ends a trace game: the bot's 64th action of one turn that is not a PASS (None: never)."""
    side, run = 0, 0
    for t, a in enumerate(actions):
        if side != agent_side:
            run += 1
            if run == BOT_BOUND and a != 155:
                return t + 1
        if a == 155:
            side, run = side ^ 1, 0
    return None


@pytest.mark.parametrize("agent_side", [0, 1])
def test_model_reproduces_expert_traces(oracle_mod, gold, agent_side):
    """Bot-vs-bot through the model (the agent plays Stormbound.expert_action too): one slot per half of
    trace_expert.npz, stride 1 and max_steps 300 as the traces were recorded, so the slot's consecutive episodes ARE the
    traces' consecutive games -- every committed step's hash, and the way each game ended."""
    g = gold("trace_expert.npz")
    off = g["offsets"]
    n_games = len(g["seeds"])
    half = n_games // 2
    assert np.all(np.diff(g["seeds"].astype(np.int64)) == 1)
    total_cuts = 0
    for lo_game, pool in ((0, None), (half, _expert_pool())):
        cuts = 0
        log = []
        kw = dict(decks=np.stack([g["deck0"][lo_game], g["deck1"][lo_game]])[None]) if pool is None else dict(pool=pool)
        if pool is None:
            assert all(np.array_equal(g["deck0"][k], g["deck0"][0]) and np.array_equal(g["deck1"][k], g["deck1"][0]) for k in range(half))
        model = VecEnvModel([int(g["seeds"][lo_game])], opponent=1, agent_side=agent_side, seed_stride=1, max_steps=300,
                            on_commit=lambda j, ep, a, h: log.append((ep, a, h)), **kw)
        for k in range(lo_game, lo_game + half):
            ep = k - lo_game
            if pool is not None:
                assert np.array_equal(model.decks[0], np.stack([g["deck0"][k], g["deck1"][k]])), k
            while True:
                a, f = model.orc.expert_action(0)
                assert f == 0, k
                v = model.step([a])
                if v["done"][0]:
                    break
            lo, hi = int(off[k]), int(off[k + 1])
            mine = [(a, h) for e, a, h in log if e == ep]
            cut = bot_bound_cut(g["action"][lo:hi], agent_side)
            if cut is not None:   # the reference's bot never ends this turn: the env's guard ends the episode
                assert [a for a, _ in mine] == [int(x) for x in g["action"][lo:lo + cut]], k
                assert [h for _, h in mine] == [int(x) for x in g["hash"][lo:lo + cut]], k
                assert v["fault"][0] == FAULT_BOT_BOUND and v["winner"][0] == -1, k
                cuts += 1
                continue
            assert [a for a, _ in mine] == [int(x) for x in g["action"][lo:hi]], k
            last = hi - 1 if g["fault"][k] else hi
            assert [h for _, h in mine[:last - lo]] == [int(x) for x in g["hash"][lo:last]], k
            if g["fault"][k]:
                assert v["fault"][0] != 0 and v["winner"][0] == -1, k
            elif hi - lo < 300:   # have_winner() ended the game (after a PASS the reference's done still reads 0)
                assert v["winner"][0] in (-1, 0, 1) and not v["truncated"][0], k
            else:
                assert v["truncated"][0] and v["winner"][0] == -1 or v["winner"][0] in (0, 1), k
            assert v["episode"][0] == ep + 1
        assert model.bot_bound_hits == cuts
        total_cuts += cuts
    # game 28 of the traces: the bot playing SECOND picks USE actions whose index does nothing and costs nothing (84, 126)
    # for 297 actions in one turn -- the reference's bot would never hand the turn back
    assert total_cuts == (1 if agent_side == 0 else 0)


def test_model_episode_k_is_a_fresh_reset(oracle_mod):
    """Auto-reset: every episode of a slot starts as a fresh oracle reset with seed0 + k * stride (stride 0 = n), the reset
    decks, and factions only for episode 0; with a pool, the decks drawn from the episode seed ^ 0x9E3779B9."""
    n = 3
    seed0 = np.array([7, 1000, 0xFFFFFFFE], dtype=np.uint32)
    deck = np.stack([deck_indices("N12M"), deck_indices("S12")])
    factions = np.array([[1, 2], [0, 3], [2, 2]], dtype=np.uint8)
    fresh = oracle_mod.Oracle(1)
    for pool in (None, _expert_pool()):
        kw = dict(decks=deck, factions=factions) if pool is None else dict(pool=pool)
        model = VecEnvModel(seed0, max_steps=40, **kw)
        rs = np.random.RandomState(5)
        seen = 0
        for _ in range(130):
            for j in range(n):   # the state each slot starts its current episode in, once per episode
                if model.steps[j] == 0:
                    k = int(model.episode[j])
                    s = (int(seed0[j]) + k * n) & 0xFFFFFFFF
                    if pool is None:
                        d, f = deck, (factions[j] if k == 0 else (0, 0))
                    else:
                        from monsoon_amd.cards import draw_random_decks_numpy
                        d, f = draw_random_decks_numpy([s ^ C5_STREAM_XOR], pool)[0], (0, 0)
                    fresh.reset(0, s, d[0], d[1], int(f[0]), int(f[1]))
                    assert fresh.canon_hash(0) == model.orc.canon_hash(j), (j, k)
                    seen += 1
            acts = []
            for j in range(n):
                la = model.orc.legal_actions(j)
                acts.append(la[rs.randint(len(la))])
            model.step(acts)
        assert seen >= 3 * n and model.episode.min() >= 2


def test_model_illegal_and_skip_leave_the_slot(oracle_mod):
    model = VecEnvModel([11, 12], decks=np.stack([deck_indices("N12M")] * 2))
    h0 = model.hashes()
    legal = model.orc.legal_actions(0)
    bad = next(a for a in range(155) if a not in legal)
    v = model.step([bad, 255])
    assert list(v["illegal"]) == [1, 0] and not v["done"].any()
    assert np.array_equal(model.hashes(), h0)
    v = model.step([155, 155])
    assert not v["illegal"].any() and not np.array_equal(model.hashes(), h0)
