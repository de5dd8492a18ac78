#!/usr/bin/env python3
"""tests/golden/trace_vs_expert.npz: the evolved agent against the scripted bot, recorded from the Python reference.

TEST INFRASTRUCTURE (build container only: needs the reference tree, through oracle/pyref/harness.py).  The fixture is
data only.  The loop is the rollout contract of include/monsoon.h (monsoon_rollout_vs_expert) with the reference's own
players, as play_vs_expert.py pairs them: HeuristicAgent.score_action + np.argmax on one side, Stormbound.expert_action
on the other, Stormbound.step for both.

Per game: seed, the two decks, which side is the bot, result (-1 / 0 / 1 by the project's rule), fault (1 = an
exception ended it: 255 as its last action if the bot raised, else the action whose step raised), steps.
Per step: the action, whether the bot made it, the canonical-record hash behind it (0 behind a step that raised).
Per heuristic decision: the hash of the score vector over the sorted legal list.

Run with PYTHONHASHSEED=0 (s203's set order).  Games: N12M both sides, 8 seeds x bot on each side; IRONCLAD (agent) against SWARM (bot), 8 seeds x each side; 8 games
on random decks from the 107-card pool of the standard record, bot side alternating.  max_turns 200, weights W0.
"""
import argparse
import contextlib
import io
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle", "pyref"))
import harness as H  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
W0 = np.random.RandomState(2024).uniform(0, 1, 10)   # the weight vector of the heuristic fixtures
MAX_TURNS = 200
POOL_OUT = ("ua20", "b005", "up01", "up02", "up03")   # the standard record's pool (107 cards)


def idx(deck):
    return [H.CARD_INDEX[c] for c in deck]


def play(args):
    seed, d0, d1, bot_side = args
    from evo.game_adapter import StormboundAdapter
    from evo.heuristic_agent import HeuristicAgent
    from evo.weights import WeightVector
    from games.stormbound import Game

    game = Game.__new__(Game)
    game.env = env = H.make_game(seed, d0, d1)
    wv = WeightVector(10)
    wv.weights = W0.copy()
    agent = HeuristicAgent(wv, 1 - bot_side)
    rec = dict(action=[], bot=[], hash=[], shash=[])
    steps = fault = shared = twice = 0   # shared / twice: steps behind which one card OBJECT is listed in a hand and its deck / twice in a deck
    with contextlib.redirect_stdout(io.StringIO()):
        while not env.have_winner() and steps < MAX_TURNS:
            adapter = StormboundAdapter(game)   # as play_vs_expert.py does every turn: the adapter caches its observation
            bot = adapter.get_current_player() == bot_side
            if bot:
                try:
                    a = int(env.expert_action())
                except Exception:  # noqa: BLE001  random.choice([]) inside the bot: a draw, nothing is stepped
                    rec["action"].append(255)
                    rec["bot"].append(1)
                    rec["hash"].append(0)
                    fault = 1
                    break
            else:
                legal = adapter.get_legal_actions()
                scores = np.array([agent.score_action(adapter, x) for x in legal], dtype=np.float64)
                a = int(legal[int(np.argmax(scores))])
                rec["shash"].append(H.fnv1a64(scores.tobytes()))
            rec["action"].append(a)
            rec["bot"].append(int(bot))
            steps += 1
            try:
                env.step(a)   # returns get_observation(): an observation that raises ends the game here too
            except Exception:  # noqa: BLE001  evo/fitness.py:208-210: a draw
                rec["hash"].append(0)
                fault = 1
                break
            rec["hash"].append(H.fnv1a64(H.canon(env)))
            players = (env.board.local, env.board.remote)
            shared += any(c is d for p in players for c in p.hand for d in p.deck)
            twice += any(len({id(c) for c in p.deck}) < len(p.deck) for p in players)
    b = {int(env.board.local.order): env.board.local.strength, int(env.board.remote.order): env.board.remote.strength}
    result = -1 if fault else (0 if (b[1] < 0 <= b[0]) else 1 if (b[0] < 0 <= b[1]) else -1)
    return dict(seed=seed, bot_side=bot_side, result=result, fault=fault, steps=steps, winner=int(env.have_winner()),
                final=H.fnv1a64(H.canon(env)), shared=shared, twice=twice, **rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    tasks = []
    for bot_side in (1, 0):
        for seed in range(8):
            tasks.append((seed, H.DECKS["N12M"], H.DECKS["N12M"], bot_side))
    for bot_side in (1, 0):   # the agent plays IRONCLAD, the bot SWARM
        for seed in range(8):
            d = (H.DECKS["IRONCLAD"], H.DECKS["SWARM"]) if bot_side == 1 else (H.DECKS["SWARM"], H.DECKS["IRONCLAD"])
            tasks.append((seed,) + d + (bot_side,))
    pool = [c for c in H.CARD_IDS if c not in POOL_OUT]
    for k in range(8):
        seed = 900 + k
        rs = np.random.RandomState(seed ^ 0x9E3779B9)
        d0 = [str(c) for c in rs.choice(pool, 12, replace=False)]
        d1 = [str(c) for c in rs.choice(pool, 12, replace=False)]
        tasks.append((seed, d0, d1, k % 2))
    with ProcessPoolExecutor(args.jobs) as ex:
        games = list(ex.map(play, tasks))
    offsets, soffsets = [0], [0]
    for g in games:
        offsets.append(offsets[-1] + len(g["action"]))
        soffsets.append(soffsets[-1] + len(g["shash"]))
    cat = lambda k, dt: np.array([x for g in games for x in g[k]], dtype=dt)   # noqa: E731
    col = lambda k, dt: np.array([g[k] for g in games], dtype=dt)   # noqa: E731
    path = os.path.join(GOLD, "trace_vs_expert.npz")
    np.savez_compressed(
        path, seeds=col("seed", np.uint32), bot_side=col("bot_side", np.int8), result=col("result", np.int8),
        fault=col("fault", np.uint8), steps=col("steps", np.int32), winner=col("winner", np.uint8), final=col("final", np.uint64),
        deck0=np.array([idx(t[1]) for t in tasks], dtype=np.uint8), deck1=np.array([idx(t[2]) for t in tasks], dtype=np.uint8),
        offsets=np.array(offsets, dtype=np.int64), soffsets=np.array(soffsets, dtype=np.int64),
        action=cat("action", np.uint8), bot=cat("bot", np.uint8), hash=cat("hash", np.uint64), shash=cat("shash", np.uint64),
        w0=W0, max_turns=np.int32(MAX_TURNS))
    bot_steps = int(cat("bot", np.uint8).sum())
    print("trace_vs_expert.npz games", len(games), "entries", offsets[-1], "of them the bot's", bot_steps, "bytes", os.path.getsize(path))
    for g in games:
        print(" seed", g["seed"], "bot", g["bot_side"], "result", g["result"], "fault", g["fault"], "steps", g["steps"], "winner", g["winner"])


if __name__ == "__main__":
    main()
