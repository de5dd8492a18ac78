"""One handle's whole life, three times in one process: every buffer the library allocates lazily is touched once --
observe, features, decide with scores; a logged rollout; a rollout whose table and schedule grow between two calls (the
grow-and-replace path); an env with the heuristic opponent and a deck schedule, one step, afterstates, save + load; the
per-call temporaries of monsoon_draw_decks, monsoon_draw_schedule and both GA calls -- then the handle is closed.  The
three passes must return bit-identical arrays: whoever owns the device memory, a fresh handle computes the same.  Success
paths only."""
import numpy as np
import pytest

from monsoon_amd.cards import DECKS, deck_indices
from test_vec_env_gpu import _first_legal, host_views
from vec_env_schedule_model import FACTIONS, standard_schedule

pytestmark = pytest.mark.gpu

N = 64        # the handle's games
SLOTS = 16    # the env's
MAX_TURNS = 40


def _matches(n, n_individuals, n_decks, salt):
    i = np.arange(n)
    return np.stack([i % n_individuals, (i * 3 + 1) % n_individuals, 1000 * salt + i, i % n_decks], axis=1)


def _one_life(torch):
    from monsoon_amd.vec_env import VecEnv
    out = {}
    rs = np.random.RandomState(2024)
    env = VecEnv(N, extended=1)   # the explore schedule below can repeat a card: only the extended record takes it
    eng = env.engine
    deck = deck_indices("N12M")
    pairs = np.stack([np.stack([deck, deck]), np.stack([deck_indices(DECKS["IRONCLAD"]), deck_indices(DECKS["SWARM"])])])

    # the lane-per-game calls and a decision round
    eng.reset(np.arange(N, dtype=np.uint32), pairs[0])
    out["obs"], out["raises"] = eng.observe()
    out["features"] = eng.features()
    out["action"], out["best"], out["scores"] = eng.decide(rs.uniform(0, 1, 10), want_scores=True)
    out["hash_after_decide"] = eng.state_hash()

    # rollouts: logged; then one whose weight table and schedule outgrow the buffers of the calls before it
    weights = rs.uniform(0, 1, (6, 10))
    counts, results, steps, log = eng.rollout_logged(weights[:4], _matches(16, 4, 2, 1), pairs, MAX_TURNS)
    out.update(log_counts=counts, log_results=results, log_steps=steps, log_action=log.action, log_score=log.score, log_n_legal=log.n_legal)
    out["log_faults"] = eng.rollout_faults(16)
    out["small_counts"], out["small_results"], out["small_steps"] = eng.rollout(weights[:2], _matches(8, 2, 2, 2), pairs, MAX_TURNS, want_results=True)
    out["grown_counts"], out["grown_results"], out["grown_steps"] = eng.rollout(weights, _matches(24, 6, 2, 3), pairs, MAX_TURNS, want_results=True)
    out["grown_faults"] = eng.rollout_faults(24)

    # the env: heuristic opponent, schedule mode, a step, afterstates, save + load
    params = standard_schedule(1, n_preserve=4, generation=33)
    seed0 = (np.arange(SLOTS, dtype=np.uint64) * 2654435761 + 5).astype(np.uint32)
    views = env.reset(seed0, factions=np.tile(np.array(FACTIONS, dtype=np.uint8), (SLOTS, 1)), opponent="heuristic", max_steps=12,
                      opponent_weights=weights, opponent_rows=np.arange(SLOTS) % 6, deck_schedule=params)
    for k, v in host_views(views).items():
        out["reset_" + k] = v
    out["env_decks"] = env.decks().cpu().numpy()
    snap = env.snapshot()
    hash_saved = env.state_hash()
    for k, v in host_views(env.step(_first_legal(torch, views["legal"]))).items():
        out["step_" + k] = v
    out["hash_after_step"] = env.state_hash()
    after = {k: t.cpu().numpy() for k, t in env.afterstates(max_after=8, obs=False).items()}
    valid = (np.arange(8)[None, :] < np.minimum(after["n_legal"], 8)[:, None])
    for k in ("n_legal", "action", "before_features"):
        out["after_" + k] = after[k]
    for k in ("status", "reward", "winner"):
        out["after_" + k] = np.where(valid, after[k], 0)
    out["after_features"] = np.where((valid & (after["status"] == 0))[:, :, None], after["features"], 0.0)
    env.restore(snap)
    out["hash_restored"] = env.state_hash()
    assert np.array_equal(out["hash_restored"], hash_saved)
    out["counters"] = np.asarray(eng.debug_counters())[:24]

    # calls that allocate and free their own temporaries
    pool = params["pool"][0, :params["pool_n"][0]]
    out["draw_decks"] = eng.draw_decks(np.arange(70, dtype=np.uint32) * 7919, pool)
    out["draw_schedule"] = eng.draw_schedule(params, np.arange(70, dtype=np.uint32) * 104729)
    ow, osg, par, tries, state = eng.ga_offspring(np.random.RandomState(11).get_state(), rs.uniform(0, 1, (5, 10)), rs.uniform(0.05, 0.2, (5, 10)),
                                                  7, 0.3, 0.2, 1e-3)
    out.update(ga_w=ow, ga_s=osg, ga_parent=par, ga_tries=tries, ga_key=state[1], ga_pos=np.array(state[2:4]), ga_gauss=np.array(state[4]))
    out["ga_order"] = eng.ga_select(np.array([0.5, 0.25, 0.5, 1.0, 0.0, 0.25, 0.75]))
    env.close()
    return out


def test_three_lives_in_one_process_compute_the_same():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    lives = [_one_life(torch) for _ in range(3)]
    first = lives[0]
    assert first["log_action"].shape == (16, MAX_TURNS) and (first["log_steps"] > 0).all()
    assert sorted(first["ga_order"].tolist()) == list(range(7)) and first["ga_order"][0] == 3
    assert first["grown_counts"].shape == (6, 3) and first["grown_steps"].shape == (24,) and (first["grown_steps"] > 0).all()
    for k, life in enumerate(lives[1:], 1):
        assert life.keys() == first.keys()
        for name, a in first.items():
            b = life[name]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (k, name)   # bit for bit, NaN padding included
