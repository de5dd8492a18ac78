"""Every call site of an ability's random pick on the device (tests/pick_sites.py: sixteen sites, every list length, every
index of the draw, both local orders, both list orders where a step reaches them; run with -m gpu on an MI355X).  Every kept
(state, stream position) of the reference is built with monsoon_debug_build from the description the oracle was built from,
and one step of it is held to the recursive oracle exactly: fault codes, canonical hashes, action indices, bit patterns of
scores.
    the API step kernel       monsoon_step on the standard record (the pick on the hit mask) and on the extended and large
                              records (the list text)
    the hot kernel            every standard variant: monsoon_decide with scores written -- the look-ahead steps the
                              triggering action with the pick compiled over the LDS column memories -- and the committed
                              action and hash.  pick_sites.check_coverage asserts that within a state the oracle's score of
                              that action differs between kept positions, so the row sees the pick; not for u061, whose
                              effect no feature reads (pick_sites.SCORE_BLIND), and not in three states of u111
                              (SCORE_PARTLY): there this test holds the look-ahead but not the drawn element
    the bot                   monsoon_expert_action, then a step of the action it returned
    the vector env            the states saved from the API handle, restored into a VecEnv without an opponent, one step
Every test first runs the CPU side's coverage assertion: a fixture that lost a case fails before it plays."""
import numpy as np
import pytest

try:
    # torch brings a HIP runtime of its own, which the process must load before libmonsoon_hip*.so pulls in the system's
    # (tests/test_deep_steps_gpu.py): the vector-env test below needs torch to see the device when this file runs alone
    import torch  # noqa: F401
except ImportError:
    pass

import kernel_variants
import pick_sites as P

STANDARD = kernel_variants.variants(False)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _built(extended=False):
    """(engine, cases): every kept case in a slot of its own."""
    from monsoon_amd.engine import BatchEngine
    assert P.check_coverage() == len(P.reference()["cases"])
    cases = P.reference()["cases"]
    eng = BatchEngine(len(cases), extended=extended)
    for k, c in enumerate(cases):
        assert eng.debug_build(k, c["seed"], c["pos"], c["enc"]) == 0, c["name"]
    return eng, cases


def _step_actions(cases):
    return np.array([c["bot_action"] if c["mode"] == "bot" else c["action"] for c in cases], dtype=np.uint8)


def _assert_steps(cases, want, fault, hashes, ctx):
    for k, (c, (f, h)) in enumerate(zip(cases, want)):
        assert int(fault[k]) == f, (ctx, c["name"], int(fault[k]), f)
        if not f:   # (a step that faults leaves no state to compare)
            assert int(hashes[k]) == h, (ctx, c["name"])


@pytest.mark.gpu
@pytest.mark.parametrize("ext", [False, True, 2], ids=["standard", "extended", "large"])
def test_api_step_kernel(ext):
    eng, cases = _built(ext)
    _, _, fault = eng.step(_step_actions(cases))
    _assert_steps(cases, P.replay(ext), fault, eng.state_hash(), kernel_variants.BUILD_NAMES[ext])
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("u,w", STANDARD, ids=[f"{u}x{w}" for u, w in STANDARD])
def test_hot_kernel_scores_and_commit(monkeypatch, u, w):
    """The whole score row of every case's decision equals the oracle's bit for bit, NaN exactly at the actions that are not
    legal; so do the committed action and the hash behind it."""
    kernel_variants.select(monkeypatch, u, w)
    eng, cases = _built()
    assert eng.variant() == (u, w)
    weights = np.broadcast_to(np.stack([P.W0, P.W1]), (len(cases), 2, 10)).copy()
    action, best, scores = eng.decide(weights, want_scores=True)
    hashes = eng.state_hash()
    for k, c in enumerate(cases):
        d = c["decision"]
        nan = np.isnan(d["scores"])
        assert np.array_equal(np.isnan(scores[k]), nan), c["name"]
        assert np.array_equal(_bits(scores[k])[~nan], _bits(d["scores"])[~nan]), (c["name"], np.nonzero(_bits(scores[k]) != _bits(d["scores"]))[0][:8])
        assert int(action[k]) == d["action"] and _bits(best[k]) == _bits(d["scores"][d["action"]]), (c["name"], int(action[k]), d["action"])
        if not d["fault"]:
            assert int(hashes[k]) == d["hash"], c["name"]
    eng.close()


@pytest.mark.gpu
def test_the_bot():
    eng, cases = _built()
    action, fault = eng.expert_action()
    bots = [k for k, c in enumerate(cases) if c["mode"] == "bot"]
    assert len(bots) >= 60
    for k in bots:
        assert (int(action[k]), int(fault[k])) == (cases[k]["bot_action"], cases[k]["bot_fault"]), cases[k]["name"]
    step = np.full(len(cases), 255, dtype=np.uint8)
    step[bots] = action[bots]
    _, _, fault = eng.step(step)
    hashes = eng.state_hash()
    for k in bots:
        assert int(fault[k]) == cases[k]["fault"], cases[k]["name"]
        if not cases[k]["fault"]:
            assert int(hashes[k]) == cases[k]["hash"], cases[k]["name"]
    eng.close()


@pytest.mark.gpu
def test_vec_env_step_kernel():
    """The cases' states restored into a VecEnv without an opponent (as tests/test_deep_steps_gpu.py restores its positions)
    and stepped with the case's action: the slot's hash is the oracle's; a step that raises closes the episode with the
    oracle's fault code."""
    import torch
    assert torch.cuda.is_available(), "torch finds no GPU: was libmonsoon_hip*.so loaded before torch?"
    from env_snapshot_model import build_entry
    from monsoon_amd import _lib
    from monsoon_amd.cards import deck_indices
    from monsoon_amd.vec_env import EnvSnapshot, VecEnv
    eng, cases = _built()
    # (the bot's draw is no part of a step: its cases step the action the bot chose from the built state, the stream unmoved)
    blobs = [eng.save_state(k) for k in range(len(cases))]
    eng.close()
    n = len(cases)
    decks = np.broadcast_to(deck_indices("N12M"), (n, 2, 12)).copy()
    env = VecEnv(n)
    try:
        env.reset(np.arange(n, dtype=np.uint32), decks, opponent="none")
        version = int(_lib.load(0).monsoon_version())
        entries = np.stack([build_entry(0, version, 0, decks[k], blobs[k]) for k in range(n)])
        assert entries.shape[1] == env.entry_bytes
        loaded = torch.zeros(n, dtype=torch.uint8, device="cuda")
        env.restore(EnvSnapshot(torch.from_numpy(entries).cuda(), n, 0, env.entry_bytes), loaded=loaded)
        assert loaded.cpu().numpy().all()
        views = env.step(torch.from_numpy(_step_actions(cases)).cuda())
        fault, illegal = views["fault"].cpu().numpy(), views["illegal"].cpu().numpy()
        hashes = env.state_hash()
        assert not illegal.any()
        for k, (c, (f, h)) in enumerate(zip(cases, P.replay(False))):
            assert int(fault[k]) == f, (c["name"], int(fault[k]), f)
            if not f:
                assert int(hashes[k]) == h, c["name"]
    finally:
        env.close()
