"""Differential check against the Python reference: bounded slices of oracle/pyref/difffuzz.py, replayed from what the
reference produced on those games (tests/golden/trace_live_*.npz and checkpoint_reference.pkl, written by the
live_* and checkpoint entries of oracle/pyref/gen_golden.py), so that no reference tree is needed to run them."""
import os
import pickle
import sys

import numpy as np
import pytest

import oracle_lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")

# --seed0 of the difffuzz.py run -> the fixture that recorded the reference's side of it
FIXTURES = {88000: "trace_live_pool.npz", 89000: "trace_live_pool_ext.npz", 90000: "trace_live_b005.npz", 91000: "trace_live_expert.npz"}


def _replay(g, ext, expert):
    """difffuzz.play over the recorded games: legal list, reward / done, canonical state, observation and features after
    every step, on the oracle.  Returns (games, mismatches); a capacity limit of the extended record (fault codes
    16 / 22 / 23) may end a game early, as difffuzz.py allows."""
    orc = oracle_lib.Oracle(1, extended=ext, core="oracle")
    bad = []
    faulted_before = 0   # a faulted final step has no feature row
    for k in range(len(g["seeds"])):
        lo, hi = int(g["offsets"][k]), int(g["offsets"][k + 1])
        seed = int(g["seeds"][k])
        if orc.reset(0, seed, g["deck0"][k], g["deck1"][k]) != 0 or orc.canon_hash(0) != int(g["init_hash"][k]):
            bad.append(f"seed {seed}: initial state differs")
            continue
        for t in range(lo, hi):
            if not np.array_equal(orc.legal_mask(0), g["legal"][t]):
                bad.append(f"seed {seed} step {t - lo}: legal differs")
                break
            a = int(g["action"][t])
            if expert:
                b, fe = orc.expert_action(0)
                if a == 255:   # the reference's bot raised
                    if fe == 0:
                        bad.append(f"seed {seed} step {t - lo}: reference expert raised, ours did not")
                    break
                if fe != 0 or a != b:
                    bad.append(f"seed {seed} step {t - lo}: expert action ref={a} ours={b} fault={fe}")
                    break
            f, r, d = orc.step(0, a)
            if g["fault"][k] and t == hi - 1:   # the reference raised on this step
                if f == 0 and orc.observe(0) is not None:
                    bad.append(f"seed {seed} step {t - lo} action {a}: reference raised, ours did not")
                break
            if f != 0:
                if not (ext and f in (16, 22, 23)):
                    bad.append(f"seed {seed} step {t - lo} action {a}: ours faulted ({f}), reference did not")
                break
            if orc.canon_hash(0) != int(g["hash"][t]):
                bad.append(f"seed {seed} step {t - lo} action {a}: state differs")
                break
            if (r, d) != (int(g["reward"][t]), int(g["done"][t])):
                bad.append(f"seed {seed} step {t - lo} action {a}: reward/done ref={(int(g['reward'][t]), int(g['done'][t]))} ours={(r, d)}")
                break
            if orc.obs_hash(0) != int(g["obs"][t]):
                bad.append(f"seed {seed} step {t - lo} action {a}: observation differs")
                break
            feat = orc.features(0)
            if feat is None or not np.array_equal(feat.view(np.uint64), g["feat"][t - faulted_before].view(np.uint64)):
                bad.append(f"seed {seed} step {t - lo}: features differ ref={g['feat'][t - faulted_before]} ours={feat}")
                break
        faulted_before += int(g["fault"][k])
    return len(g["seeds"]), bad


@pytest.mark.parametrize("args,ext", [
    (["--pool", "all", "--games", "30", "--steps", "300", "--seed0", "88000"], False),                   # 107 standard-record cards
    (["--pool", "all", "--games", "30", "--steps", "300", "--seed0", "89000"], True),                    # all 109 observable cards
    (["--pool", "all", "--must", "b005", "--games", "40", "--steps", "300", "--seed0", "90000"], True),  # nested b005 memories
    (["--deck", "IRONCLAD", "--deck2", "SWARM", "--games", "12", "--steps", "300", "--seed0", "91000", "--expert"], False),
])
def test_random_policy_games_equal_the_reference_step_by_step(oracle_mod, args, ext):
    """Seeded games of the reference (a random legal policy, or its scripted bot on both sides), every action mirrored on
    the C++ restatement: legal lists, reward / done, canonical state, observation and features after every step.  A
    capacity limit of the extended record (fault codes 16 / 22 / 23) may end a game early; any other difference fails."""
    g = np.load(os.path.join(GOLD, FIXTURES[int(args[args.index("--seed0") + 1])]))
    games, bad = _replay(g, ext, "--expert" in args)
    assert not bad, bad
    assert games == int(args[args.index("--games") + 1])


class _Stand:
    """What a checkpoint's evo.* object unpickles to here: the reference's classes are not importable."""


def _load(path):
    """Unpickle a checkpoint with stand-ins for the reference's classes; returns (data, the evo.* classes it names)."""
    named = set()

    class Loader(pickle.Unpickler):
        def find_class(self, module, name):
            if module.split(".")[0] == "evo":
                named.add((module, name))
                return type(name, (_Stand,), {"__module__": module})
            if module.split(".")[0] in ("numpy", "copyreg", "builtins", "_codecs"):
                return super().find_class(module, name)
            raise pickle.UnpicklingError(f"unexpected global {module}.{name}")
    with open(path, "rb") as f:
        return Loader(f).load(), named


def test_reference_loads_the_exported_checkpoint(tmp_path):
    """SURVEY §8f rank 4, checkpoint compatibility: Population.save_reference_checkpoint writes a pickle in the reference's own
    class names.  The reference loads a checkpoint with pickle.load and reads its fields (evo/population.py:296-310), and
    WeightVector.mutate / copy read weights, sigmas and size: so the export must name exactly the classes the reference's
    own checkpoint of the same population names (tests/golden/checkpoint_reference.pkl), and hold the same generation,
    fitness scores, weights and sigmas, every attribute the reference's objects have, and the configuration's fields."""
    sys.path.insert(0, REPO)
    from monsoon_amd.config import EvolutionaryConfig
    from monsoon_amd.population import Population
    pop = Population(EvolutionaryConfig(mu=12, lambda_=12, seed=9))
    pop.initialize_population(10)
    pop.fitness_scores = [i / 12 for i in range(12)]
    pop.generation = 7
    path = str(tmp_path / "population.pkl")
    pop.save_reference_checkpoint(path)
    assert "evo.weights" not in sys.modules and "evo.config" not in sys.modules   # the stand-ins are gone again
    ref_path = os.path.join(GOLD, "checkpoint_reference.pkl")
    ours, named = _load(path)
    ref, ref_named = _load(ref_path)
    assert named == ref_named == {("evo.weights", "WeightVector"), ("evo.config", "EvolutionaryConfig")}
    assert set(ours) == set(ref) == {"generation", "individuals", "fitness_scores", "config"}
    assert ours["generation"] == ref["generation"] == 7
    assert ours["fitness_scores"] == ref["fitness_scores"] and ours["fitness_scores"][11] == 11 / 12
    assert len(ours["individuals"]) == len(ref["individuals"]) == 12
    for v, rv, mine in zip(ours["individuals"], ref["individuals"], pop.individuals):
        assert type(v).__module__ == "evo.weights" and type(v).__name__ == "WeightVector"
        assert set(vars(v)) == set(vars(rv)) == {"weights", "sigmas", "size"}
        for k in ("weights", "sigmas"):
            a, b = getattr(v, k), getattr(rv, k)
            assert isinstance(a, np.ndarray) and a.dtype == b.dtype == np.float64 and a.shape == b.shape == (10,)
            assert np.array_equal(a, b)
        assert np.array_equal(v.weights, mine.weights) and np.array_equal(v.sigmas, mine.sigmas)
        assert type(v.size) is int and v.size == rv.size == 10
    cfg, rcfg = ours["config"], ref["config"]
    assert type(cfg).__module__ == "evo.config" and type(cfg).__name__ == "EvolutionaryConfig"
    for k, val in vars(rcfg).items():
        assert k in vars(cfg) and getattr(cfg, k) == val, k
    assert cfg.mu == 12 and cfg.tau == 0.1
