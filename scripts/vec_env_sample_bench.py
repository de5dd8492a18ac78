#!/usr/bin/env python3
"""What the sampling opponent kernel costs in the vector env (VecEnv opponent_explore with a temperature, k_env_opp_sample).

vec_env_explore_bench.py's workload and method -- --slots slots (default 65 536), N12M decks, the agent FIRST with a random
policy sampled on the device from the legal mask, the heuristic opponent with 8 weight vectors (slot i playing row i % 8),
--warmup steps, then --windows timed windows, each ended by a synchronise, the median window reported with min - max --
with five arms in one process on the same seeds and the same policy stream:

  plain           the env without a rule: k_env_opp
  explore-silent  the uniform rule with all thresholds 0: the same games through k_env_opp_explore
  explore         the uniform rule at --eps in every slot: other games
  sample-silent   the sampling rule with all thresholds 0: the same games through k_env_opp_sample -- every candidate's
                  score stored to the score table, the post-pass block entered and left at its draw
  sample          the sampling rule at --eps, temperature --temperature in every slot: other games, and a re-step for every
                  sampling decision that did not draw its arg-max

A window is a fixed number of steps (--steps), not a fixed time, so that window k of the three arms that play the same
games is the same steps of the same games: their ratio per window is the kernel's cost, free of what the games' phase does
to a step's cost.  The arms run one after the other, each in a fresh VecEnv; --rounds repeats the whole sequence.  One JSON
line per arm and round, and one per ratio (sample-silent / explore-silent, sample-silent / plain, sample / explore; the last
compares other games, so it holds on average only); --out appends them to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from monsoon_amd.cards import deck_indices  # noqa: E402
from monsoon_amd.vec_env import OpponentExplore, VecEnv  # noqa: E402


def arms(args):
    """name -> the OpponentExplore of the arm (None = no rule)."""
    return (("plain", None), ("explore-silent", OpponentExplore(0.0, 2024)), ("explore", OpponentExplore(args.eps, 2024)),
            ("sample-silent", OpponentExplore(0.0, 2024, temperature=args.temperature)),
            ("sample", OpponentExplore(args.eps, 2024, temperature=args.temperature)))


def sample(torch, legal, gen):
    u = torch.rand(legal.shape, device=legal.device, generator=gen)
    u.masked_fill_(~legal, -1.0)
    return u.argmax(dim=1).to(torch.uint8)


def run_arm(torch, args, rule):
    n = args.slots
    seed0 = np.arange(n, dtype=np.uint32) + 1000
    deck = np.stack([deck_indices("N12M"), deck_indices("N12M")])
    env = VecEnv(n)
    kw = dict(opponent="heuristic", agent_side=0, max_steps=args.max_steps,
              opponent_weights=np.random.RandomState(42).uniform(0, 1, (8, 10)), opponent_rows=np.arange(n) % 8)
    if rule is not None:
        kw["opponent_explore"] = rule
    views = env.reset(seed0, np.broadcast_to(deck, (n, 2, 12)).copy(), **kw)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)

    def counts():
        c = env.engine.debug_counters()
        return int(c[6]), int(c[7]), (int(env.opponent_explored().sum().item()) if rule is not None else 0)

    for _ in range(args.warmup):
        views = env.step(sample(torch, views["legal"], gen))
    torch.cuda.synchronize()
    res = []
    for _ in range(args.windows):
        a0, d0, x0 = counts()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            views = env.step(sample(torch, views["legal"], gen))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        a1, d1, x1 = counts()
        res.append(dict(agent=(a1 - a0) / dt, decisions=(d1 - d0) / dt, explored=x1 - x0, decided=d1 - d0, seconds=dt))
    final = env.state_hash()
    env.close()
    return res, final


def summary(res, key):
    v = sorted(r[key] for r in res)
    return dict(median=round(v[len(v) // 2]), min=round(v[0]), max=round(v[-1]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--slots", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40, help="steps per window")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--max-steps", type=int, default=0)
    ap.add_argument("--eps", type=float, default=0.25)
    ap.add_argument("--temperature", type=float, default=0.5)
    ap.add_argument("--out", default="", help="append the JSON lines to this file")
    args = ap.parse_args()
    import torch
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    for rnd in range(args.rounds):
        got = {}
        for name, rule in arms(args):
            res, final = run_arm(torch, args, rule)
            got[name] = (res, final)
            emit(dict(arm=name, round=rnd, slots=args.slots, windows=args.windows, steps_per_window=args.steps,
                      agent_steps_per_s=summary(res, "agent"), opponent_decisions_per_s=summary(res, "decisions"),
                      explored_decisions=sum(r["explored"] for r in res), opponent_decisions=sum(r["decided"] for r in res),
                      window_s=[round(r["seconds"], 4) for r in res]))
        for num, den in (("sample-silent", "explore-silent"), ("sample-silent", "plain"), ("explore-silent", "plain"), ("sample", "explore")):
            same = bool(np.array_equal(got[num][1], got[den][1]))   # the two arms played the same games to the same states
            ratio = [a["seconds"] / b["seconds"] for a, b in zip(got[num][0], got[den][0])]
            emit(dict(arm=f"{num}/{den}", round=rnd, same_final_states=same, window_time_ratio=[round(r, 4) for r in ratio],
                      median=round(sorted(ratio)[len(ratio) // 2], 4), min=round(min(ratio), 4), max=round(max(ratio), 4)))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
