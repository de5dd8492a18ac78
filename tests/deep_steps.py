"""The deep-step fixture (tests/golden/deep_steps.json.gz) shared by the CPU and GPU tests: positions found by
scripts/deep_step_search.py -- steps that drive the rules core's work stack through nested evictions or into the recursion
guard -- with what the Python reference did on them (oracle/pyref/gen_deep_steps.py).  Test infrastructure only."""
import gzip
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W0 = np.random.RandomState(2024).uniform(0, 1, 10)

_fixture = None


def fixture():
    """{"search": the search's size, "positions": [...]}; a position: cls (A nested evictions / B the guard / C the deepest
    finite chain / D several evicting candidates), tier, seed, decks, factions, bot_side (-1, or the side the scripted bot
    plays: it draws from the game's stream before each of its steps), prefix, action, count {fault, depth, words, seg,
    at_guard} of the counting host build, and the reference's side: hash_before, raised (class name or None), nesting,
    canon (hex), reward, done, legal."""
    global _fixture
    if _fixture is None:
        with gzip.open(os.path.join(GOLD, "deep_steps.json.gz"), "rt") as f:
            _fixture = json.load(f)
    return _fixture


def positions():
    return fixture()["positions"]


def at_position(orc, i, p):
    """Reset game i and play the prefix; the deep action is still to be stepped.  Returns the canonical hash there."""
    assert orc.reset(i, p["seed"], p["decks"][0], p["decks"][1], *p["factions"]) == 0
    for a in p["prefix"]:
        bot_draws(orc, i, p, a)
        f = orc.step(i, a)[0]
        assert f == 0, (p["source"], a, f)
    h = orc.canon_hash(i)
    bot_draws(orc, i, p, p["action"])
    return h


def bot_draws(orc, i, p, a):
    if orc.to_play(i) == p["bot_side"]:
        b, f = orc.expert_action(i)
        assert (b, f) == (a, 0), (p["source"], a, b, f)


def expected_fault(p):
    """The engine's code for what the reference did: 18 for RecursionError, 1 for any other exception, 0."""
    return 0 if p["raised"] is None else 18 if p["raised"] == "RecursionError" else 1


def legal_of(p):
    return np.array(p["legal"], dtype=np.uint64)
