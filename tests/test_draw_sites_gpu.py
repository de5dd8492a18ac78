"""The random draws of the rules that are no Pick, on the device (tests/draw_sites.py: choice over a list the card builds,
shuffle and slice, sort by (key, random()), a drawn value; run with -m gpu on an MI355X).  Every kept (state, stream position)
of the reference is built with monsoon_debug_build from the description the oracle was built from, each in a slot of its own,
and one step of it is held to the recursive oracle exactly: fault codes, canonical hashes, action indices, bit patterns of
scores.  No comparison has a tolerance.
    the API step kernel       monsoon_step on the standard, the extended and the large record
    the hot kernel            every standard variant, and every extended variant for ua20: monsoon_decide with scores
                              written, and the committed action and hash.
                              draw_sites.check_coverage asserts state by state that the oracle's score of the triggering action
                              differs between kept positions, so the row sees the draw; not for the sites of SCORE_BLIND and
                              some states of SCORE_PARTLY.  For the blind sites of ALT_WEIGHTS the same positions are decided
                              once more under a weight pair that commits the triggering action: there the committed hash
                              carries the draw.  For those of NO_COMMIT the hot kernel holds the look-ahead but not the draw;
                              the step kernels do
    the vector env            the states saved from the API handle, restored into a VecEnv without an opponent, one step
Every test first runs the CPU side's coverage assertion: a table that lost a case fails before it plays."""
import numpy as np
import pytest

try:
    # torch brings a HIP runtime of its own, which the process must load before libmonsoon_hip*.so pulls in the system's
    # (tests/test_deep_steps_gpu.py): the vector-env test below needs torch to see the device when this file runs alone
    import torch  # noqa: F401
except ImportError:
    pass

import draw_sites as D
import kernel_variants

STANDARD = kernel_variants.variants(False)
EXTENDED = kernel_variants.variants(True)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _built(extended=False, alt=True, only_ext=False):
    """(engine, cases): every kept case in a slot of its own; alt=False: without the cases that differ in weights alone;
    only_ext: the cases of the sites that need the extended record (ua20)."""
    from monsoon_amd.engine import BatchEngine
    assert D.check_coverage() == len(D.reference()["cases"])
    cases = [c for c in D.reference()["cases"] if (alt or not c["alt"]) and (c["ext"] or not only_ext)]
    eng = BatchEngine(len(cases), extended=extended)
    for k, c in enumerate(cases):
        assert eng.debug_build(k, c["seed"], c["pos"], c["enc"]) == 0, c["name"]
    return eng, cases


def _step_actions(cases):
    return np.array([c["action"] for c in cases], dtype=np.uint8)


def _want(cases, extended):
    """(fault, hash) of each of `cases` on the recursive oracle of that record build."""
    by_name = {c["name"]: w for c, w in zip(D.reference()["cases"], D.replay(extended))}
    return [by_name[c["name"]] for c in cases]


@pytest.mark.gpu
@pytest.mark.parametrize("ext", [False, True, 2], ids=["standard", "extended", "large"])
def test_api_step_kernel(ext):
    eng, cases = _built(ext, alt=False)
    _, _, fault = eng.step(_step_actions(cases))
    hashes = eng.state_hash()
    for k, (c, (f, h)) in enumerate(zip(cases, _want(cases, ext))):
        assert int(fault[k]) == f, (kernel_variants.BUILD_NAMES[ext], c["name"], int(fault[k]), f)
        if not f:   # (a step that faults leaves no state to compare)
            assert int(hashes[k]) == h, (kernel_variants.BUILD_NAMES[ext], c["name"])
    eng.close()


def _assert_decisions(eng, cases, decisions):
    weights = np.stack([c["weights"] for c in cases]).astype(np.float64)
    action, best, scores = eng.decide(weights, want_scores=True)
    hashes = eng.state_hash()
    for k, (c, d) in enumerate(zip(cases, decisions)):
        nan = np.isnan(d["scores"])
        assert np.array_equal(np.isnan(scores[k]), nan), c["name"]
        assert np.array_equal(_bits(scores[k])[~nan], _bits(d["scores"])[~nan]), (c["name"], np.nonzero(_bits(scores[k]) != _bits(d["scores"]))[0][:8])
        assert int(action[k]) == d["action"] and _bits(best[k]) == _bits(d["scores"][d["action"]]), (c["name"], int(action[k]), d["action"])
        if not d["fault"]:
            assert int(hashes[k]) == d["hash"], c["name"]


@pytest.mark.gpu
@pytest.mark.parametrize("u,w", STANDARD, ids=[f"{u}x{w}" for u, w in STANDARD])
def test_hot_kernel_scores_and_commit(monkeypatch, u, w):
    """The whole score row of every case's decision equals the oracle's bit for bit, NaN exactly at the actions that are not
    legal; so do the committed action and the hash behind it, each case under its own weight pair.  ua20's cases are held to
    what the oracle of the standard record decides."""
    kernel_variants.select(monkeypatch, u, w)
    eng, cases = _built()
    assert eng.variant() == (u, w)
    _assert_decisions(eng, cases, [c["std"]["decision"] if c["ext"] else c["decision"] for c in cases])
    assert {c["site"] for c in cases if c["alt"] and c["decision"]["action"] == c["action"]} == set(D.ALT_WEIGHTS)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("u,w", EXTENDED, ids=[f"ext-{u}x{w}" for u, w in EXTENDED])
def test_hot_kernel_on_the_extended_record(monkeypatch, u, w):
    """ua20's cases on every extended variant: the score row, the committed action and the hash of the extended oracle."""
    kernel_variants.select(monkeypatch, u, w)
    eng, cases = _built(True, only_ext=True)
    assert eng.variant() == (u, w) and len(cases) >= 10
    _assert_decisions(eng, cases, [c["decision"] for c in cases])
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
    eng, cases = _built(alt=False)
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
        for k, (c, (f, h)) in enumerate(zip(cases, _want(cases, False))):
            assert int(fault[k]) == f, (c["name"], int(fault[k]), f)
            if not f:
                assert int(hashes[k]) == h, c["name"]
    finally:
        env.close()
