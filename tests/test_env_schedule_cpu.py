"""Schedule mode of the vector env (monsoon_env_set_schedule, VecEnv.reset(deck_schedule=...)), CPU side.

1. monsoon_amd/csrc/deck_schedule.h -- the text k_env_reseed_schedule compiles -- walked on the host by the stand-alone
   program of tests/deck_schedule_check.cpp under the address and UB sanitizers: phase 0 (both archetypes, no output of
   the stream read, n_preserve and pools ignored) and phases 1 / 2 keyed with the env's tag 3, against Python's own
   random.Random (deck_schedule_cases.params_decks) and the archetypes.
2. DeckEvolutionConfig.env_schedule against schedule_params and game_decks over exploit, explore and balance generations.
3. The host-side contract that needs no device: the ABI's new entry points, the model helper, EvolutionaryGame's decks."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import deck_schedule_cases as C
from monsoon_amd.cards import CARD_INDEX, DECKS, deck_indices
from monsoon_amd.decks import IRONCLAD, SHADOWFEN, SWARM, TAG_ENV, TAG_EXPERT, TAG_POPULATION, DeckEvolutionConfig, available_cards
from vec_env_schedule_model import FACTIONS, schedule_decks, standard_schedule

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = 300   # per case

# (name, schedule): the cases of tests/test_env_schedule_gpu.py's parity test, and phase 0 with fields it must ignore
WALKS = (("static", standard_schedule(0, n_preserve=5, generation=2)),
         ("explore-keep9", standard_schedule(1, n_preserve=9, generation=31)),    # 3 of 56+: the set path
         ("explore-keep3", standard_schedule(1, n_preserve=3, generation=50)),    # 9 of 56+: the pool path
         ("explore-keep12", standard_schedule(1, n_preserve=12, generation=30)),
         ("balance-0.7", standard_schedule(2, ratio=0.7, generation=61)))


def test_walk_of_the_env_phases_equals_stdlib_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the oracle too"
    exe = str(tmp_path / "deck_schedule_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "monsoon_amd", "csrc"), os.path.join(REPO, "tests", "deck_schedule_check.cpp"), "-o", exe],
                   check=True)
    lines = [str(len(WALKS))]
    seeds = C.game_seeds(GAMES, 77)
    for _, p in WALKS:
        assert p["tag"] == TAG_ENV == 3
        n0, n1 = int(p["pool_n"][0]), int(p["pool_n"][1])
        lines.append(" ".join(str(v) for v in (p["seed"], p["generation"], p["tag"], p["phase"], p["n_preserve"],
                                               float(p["balance_archetype_ratio"]).hex(), n0, n1, len(seeds))))
        lines.append(" ".join(str(int(v)) for v in np.concatenate([p["archetype"].ravel(), p["pool"][0, :n0], p["pool"][1, :n1]])))
        lines.append(" ".join(str(int(s)) for s in seeds))
    inp = tmp_path / "cases.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.split("\n")
    pos = 0
    for i, (name, p) in enumerate(WALKS):
        head = out[pos].split()
        assert head[:2] == ["case", str(i)], out[pos]
        assert int(head[3]) == 0, f"{name}: {head[3]} games ran past the 624-output window"
        used = int(head[5])
        got = np.frombuffer(bytes.fromhex("".join(out[pos + 1:pos + 1 + GAMES])), dtype=np.uint8).reshape(GAMES, 2, 12)
        pos += 1 + GAMES
        want = np.stack([schedule_decks(p, int(s)) for s in seeds])
        bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
        assert len(bad) == 0, f"{name}: {len(bad)} of {GAMES} games differ, first at seed {int(seeds[bad[0]])}: {got[bad[0]].tolist()} != {want[bad[0]].tolist()}"
        if p["phase"] == 0 or p["n_preserve"] == 12:
            assert used == 0 and (got == p["archetype"][None]).all(), name   # no output read, whatever n_preserve and the pools say
        else:
            assert 4 <= used < 624, (name, used)
            assert len({g.tobytes() for g in got}) > GAMES // 4, name        # (balance at 0.7 keeps both archetypes in half of the games)
    # the tag keys the stream: the env's episode never plays the population's or the bot's game of the same seed
    p = WALKS[2][1]
    for tag in (TAG_POPULATION, TAG_EXPERT):
        other = dict(p, tag=tag)
        assert all((schedule_decks(p, int(s)) != schedule_decks(other, int(s))).any() for s in seeds[:50])


def _config(**kw):
    kw = dict(dict(exploit_generations=2, explore_generations=6, seed=5 + (9 << 32), per_game=True), **kw)
    return DeckEvolutionConfig(DECKS["IRONCLAD"], DECKS["SWARM"], **kw)


def _indices(pair):
    return np.stack([deck_indices(pair[0]), deck_indices(pair[1])])


def test_env_schedule_against_schedule_params_and_game_decks():
    dc = _config()
    seeds = [int(s) for s in C.game_seeds(25, 3)]
    for g in range(12):   # 0-1 exploit, 2-7 explore, 8.. balance
        p = dc.env_schedule(g)
        assert (p["seed"], p["generation"], p["tag"]) == (5, g, TAG_ENV)
        ref = dc.schedule_params(g, TAG_ENV)
        if g < 2:
            assert ref is None and p["phase"] == 0
            assert np.array_equal(p["archetype"], _indices((DECKS["IRONCLAD"], DECKS["SWARM"])))
            assert p["pool"].shape == (2, 128) and p["pool"].dtype == np.uint8 and p["archetype"].dtype == np.uint8
        else:
            assert p["phase"] == (1 if g < 8 else 2) and sorted(p) == sorted(ref)
            assert all(np.array_equal(p[k], ref[k]) for k in p)
        for s in seeds:   # the walk over the fields, by the stdlib, is the specification's pair
            assert np.array_equal(schedule_decks(p, s), _indices(dc.game_decks(g, s, TAG_ENV))), (g, s)
    assert dc.schedule_params(0) is None and dc.schedule_params(3)["tag"] == TAG_POPULATION   # schedule_params itself stays as it is
    with pytest.raises(ValueError, match="per_game"):
        DeckEvolutionConfig(DECKS["IRONCLAD"], DECKS["SWARM"], seed=5).env_schedule(0)
    short = DeckEvolutionConfig(DECKS["IRONCLAD"][:11], DECKS["SWARM"], exploit_generations=1, seed=1, per_game=True)
    for g in (0, 2):   # where schedule_params returns None for another reason than the exploit phase
        with pytest.raises(ValueError, match="12 cards"):
            short.env_schedule(g)


def test_faction_pools_need_the_extended_build():
    """Why a config-derived schedule needs VecEnv(extended=1) once it draws, and the hand-made one of the tests does not."""
    for f in (IRONCLAD, SWARM, SHADOWFEN):
        assert "ua20" in available_cards(f)
    assert "b005" in available_cards(SHADOWFEN) and "b005" not in available_cards(IRONCLAD)
    p = standard_schedule(1, 3)
    bad = {CARD_INDEX["ua20"], CARD_INDEX["b005"]}
    assert tuple(p["pool_n"]) == tuple(len(available_cards(f)) - 1 for f in FACTIONS) and min(p["pool_n"]) >= 56
    assert not bad & set(p["pool"][0, :p["pool_n"][0]].tolist()) and not bad & set(p["pool"][1, :p["pool_n"][1]].tolist())
    assert not bad & set(p["archetype"].ravel().tolist())


def test_abi_and_python_surface():
    from monsoon_amd import _lib
    from monsoon_amd.engine import BatchEngine
    from monsoon_amd.game import EvolutionaryGame, Game
    from monsoon_amd.vec_env import VecEnv
    assert {"monsoon_env_set_schedule", "monsoon_env_decks_dev"} <= set(_lib.SIGNATURES)
    header = open(os.path.join(REPO, "include", "monsoon.h")).read()
    assert "int monsoon_env_set_schedule(monsoon_t* h, const monsoon_deck_schedule* schedule);" in header
    assert "int monsoon_env_decks_dev(monsoon_t* h, void* out_dev);" in header and "word 17" in header
    for name in ("env_set_schedule", "env_decks_dev"):
        assert callable(getattr(BatchEngine, name))
    for name in ("set_deck_schedule", "decks"):
        assert callable(getattr(VecEnv, name))
    assert issubclass(EvolutionaryGame, Game)
    sc = BatchEngine._deck_schedule(standard_schedule(2, ratio=0.25, generation=9))
    assert (sc.seed, sc.generation, sc.tag, sc.phase, sc.balance_archetype_ratio) == (20240519, 9, 3, 2, 0.25)
    assert bytes(sc.archetype) == standard_schedule(2)["archetype"].tobytes()
