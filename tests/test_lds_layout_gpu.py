"""The candidate records' LDS map of the wavefront-per-game kernels (monsoon_amd/csrc/lds_layout.h; kernels.h PlayLds: one
contiguous column per candidate on the standard record, the 16-byte interleave on the extended and the large one) on the
device.  tests/test_lds_layout_cpu.py pins the map itself; here every kernel that moves a record between registers and the
columns, steps it through the per-lane accessors and reads it through the column-0 and sub-lane accessors must still compute
what the serial kernels and the oracle compute (run with -m gpu on an MI355X).

Every variant of variants.def in the three builds plays the 64 games of tests/lds_layout_line.py for 40 decisions through
play_rounds, one decision per launch and eight per launch: state hash, to_play / have_winner, the ten features and the fault
code equal the oracle's line game for game.  The games hold a decision with one legal action (the first column alone), with
exactly U (the last column) and with more than 2 U (several passes; 69 at U = 64, where more than 128 cannot occur:
lds_layout_line.wanted), and
sixteen of them start within 16 words of the end of a stream block, so that the commit regenerates the block in the area the
columns lie in and restores column 0 behind it.

The other consumers of PlayLds at 16 games or slots each, by the comparisons their own tests make: the vector env's heuristic
opponent against its model (monsoon_step / monsoon_legal_mask lines of tests/vec_env_heuristic_model.py), the afterstates
against theirs, a logged rollout against the model of the log and its replay into rows against the replay model."""
import struct

import numpy as np
import pytest

import kernel_variants
import lds_layout_line as LL

pytestmark = pytest.mark.gpu

VARIANTS, VARIANT_IDS = kernel_variants.matrix()
BLOB_META_RNG = 8 + 16   # GameMeta.rng in a blob of monsoon_state_save: cursor | current block << 16 (kernels.h GameMeta)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _engine(ext):
    import torch  # noqa: F401  (its runtime before the library's: the env tests below need it, VecEnv.__init__ says why)
    from monsoon_amd.cards import deck_indices
    from monsoon_amd.engine import BatchEngine
    deck = deck_indices("N12M")
    eng = BatchEngine(LL.N, extended=ext)
    seeds = np.array(LL.SEEDS + [0] * (LL.N - LL.N_RESET), dtype=np.uint32)
    eng.reset(seeds, np.stack([deck, deck]))
    for k in range(LL.N - LL.N_RESET):
        seed, pos, enc = LL.scenario(k)
        assert eng.debug_build(LL.N_RESET + k, seed, pos, enc) == 0, k
    eng.upload_weights(np.stack([LL.W0, LL.W1]))
    eng.assign_players(np.zeros(LL.N, dtype=np.int32), np.ones(LL.N, dtype=np.int32))
    return eng


def _compare(eng, t, r, ctx):
    clean = t["clean"][r]
    hashes, status, feats, faults = eng.state_hash(), eng.status(), eng.features(), eng.game_faults()
    print(ctx, "round", r, "hash mismatches", int((hashes[clean] != t["hash"][r][clean]).sum()), "fault mismatches", int((faults != t["fault"][r]).sum()))
    assert np.array_equal(faults, t["fault"][r]), (ctx, r, np.nonzero(faults != t["fault"][r])[0][:8])
    assert np.array_equal(hashes[clean], t["hash"][r][clean]), (ctx, r, np.nonzero(hashes != t["hash"][r])[0][:8])
    assert np.array_equal(status[clean, :2], t["status"][r][clean]), (ctx, r)
    have = clean & ~np.isnan(t["features"][r]).any(axis=1)
    assert have.sum() >= LL.N // 2
    assert np.array_equal(_bits(feats[have]), _bits(t["features"][r][have])), (ctx, r)


@pytest.mark.parametrize("ext,u,w", VARIANTS, ids=VARIANT_IDS)
def test_every_variant_stays_on_the_oracle_line(monkeypatch, ext, u, w):
    t = LL.line(ext)
    LL.check_cases(t, [u])
    kernel_variants.select(monkeypatch, u, w)
    for rounds in (1, 8):
        eng = _engine(ext)
        assert eng.variant() == (u, w)
        start = [struct.unpack_from("<I", eng.save_state(i), BLOB_META_RNG)[0] for i in range(LL.N_RESET, LL.N)]
        for k in range(LL.DECISIONS // rounds):
            eng.play_rounds(rounds)
            eng.sync()
            _compare(eng, t, rounds * k + rounds - 1, f"play_rounds({rounds})")
        end = [struct.unpack_from("<I", eng.save_state(i), BLOB_META_RNG)[0] for i in range(LL.N_RESET, LL.N)]
        crossed = sum(((e ^ s) >> 16) & 1 for s, e in zip(start, end))   # the current block changed: the wave refilled the used-up one in the column area
        print("games that crossed a stream block:", crossed)
        assert crossed >= 1, end
        st = eng.stats()
        assert st["capacity_faults"] == 0 and st["lookahead_capacity_faults"] == 0
        eng.close()


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.mark.parametrize("agent_side", [0, 1])
def test_heuristic_opponent_of_the_vector_env(agent_side):
    """k_env_opp: 16 slots in lockstep with the model, every view and the state hash after every step."""
    torch = _torch()
    from monsoon_amd.vec_env import VecEnv
    from test_vec_env_gpu import assert_views_equal, host_views, mixed_decks
    from test_vec_env_heuristic_gpu import league, lockstep
    from vec_env_heuristic_model import HeuristicVecEnvModel
    n, steps = 16, 60
    seed0 = (np.arange(n, dtype=np.uint32) * 7919 + 11 + 100 * agent_side).astype(np.uint32)
    decks, w = mixed_decks(n), league(8)
    rows = (np.arange(n) * 5) % len(w)
    env = VecEnv(n)
    views = env.reset(seed0, decks, opponent="heuristic", agent_side=agent_side, max_steps=0, opponent_weights=w, opponent_rows=rows)
    model = HeuristicVecEnvModel(seed0, w, rows, decks=decks, agent_side=agent_side, max_steps=0)
    assert_views_equal(host_views(views), model.views, "reset")
    lockstep(torch, env, model, n, steps, np.random.RandomState(5 + agent_side), "16 slots")
    env.close()


@pytest.mark.parametrize("ext", [0, 2], ids=["standard", "large"])
def test_afterstates_of_the_vector_env(ext):
    """k_env_after: 16 slots (8 on the large record), the afterstates of every slot before every step against the model's."""
    torch = _torch()
    from env_afterstates_model import AfterstatesModel, History, compare_slot
    from monsoon_amd.vec_env import VecEnv
    from test_env_afterstates_gpu import _ext_decks, n12m
    from test_vec_env_gpu import host_views, random_legal
    from vec_env_model import VecEnvModel
    n, steps = (16, 24) if not ext else (8, 12)
    seed0 = (np.arange(n, dtype=np.uint32) * 2654435 + 1234 + ext).astype(np.uint32)
    decks = n12m(n) if not ext else _ext_decks(n)
    hist = History()
    model = VecEnvModel(seed0, decks, opponent=0, agent_side=0, max_steps=50, extended=ext, on_commit=hist)
    am = AfterstatesModel(model, hist, extended=ext)
    env = VecEnv(n, extended=ext)
    env.reset(seed0, decks, opponent="none", agent_side=0, max_steps=50)
    rs = np.random.RandomState(3)
    entries = passes = 0
    for t in range(steps):
        got = host_views(env.afterstates(156))
        for j in range(n):
            want = am.slot(j, 156)
            compare_slot(want, got, j, 156, (ext, t, j))
            entries += len(want["entries"])
            passes += want["n_legal"] > 8
        a = random_legal(rs, model.views["legal"])
        model.step(a)
        env.step(torch.from_numpy(a).cuda())
        assert np.array_equal(env.state_hash(), model.hashes())
    env.close()
    assert entries > 0 and passes > 0


def test_logged_rollout_and_its_replay():
    """k_play_log and k_replay_log: 16 matches of the mixed schedule (the bot on either side, none), S12 and N12M alternating,
    every entry of the log against the model of the log, every row of the replay against the replay model."""
    _torch()
    import replay_model as RM
    import rollout_log_model as R
    from monsoon_amd import game_log
    from monsoon_amd.cards import deck_indices
    from monsoon_amd.engine import BatchEngine
    from test_rollout_log_gpu import W2, _schedule
    n, T = 16, 200
    m = _schedule(n, seed0=3)
    m["deck"] = (np.arange(n) // 3) % 2
    pairs = np.stack([np.stack([deck_indices(d)] * 2) for d in ("S12", "N12M")])
    eng = BatchEngine(64)
    counts, results, steps, log = eng.rollout_logged(W2, m, pairs, T)
    faults = eng.rollout_faults(n)
    d = game_log.dataset(eng, m, pairs, log, results=results)
    eng.close()
    model = R.ModelEngine(0)
    ref = model.rollout_logged(W2, m, pairs, T)
    assert np.array_equal(counts, ref[0]) and np.array_equal(results, ref[1]) and np.array_equal(faults, model.rollout_faults(n))
    assert R.same_log(log, ref[3])
    rows = RM.replay(m, pairs, log.action, steps)
    assert RM.same_rows(d, rows) is None and rows["reached"].all() and not d["status"].any()
