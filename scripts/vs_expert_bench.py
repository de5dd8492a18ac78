#!/usr/bin/env python3
"""Throughput of rollouts against the scripted bot (monsoon_rollout_vs_expert) next to self-play (monsoon_rollout).

65 536 games, N12M both sides, weights W0, max_turns 200: the bot SECOND, the bot FIRST and the same number of self-play
games, alternating in one process on one handle, five repetitions each after one warm-up round.  Per configuration and
repetition: wall ms, kernel ms (monsoon_kernel_time), committed steps, heuristic decisions, look-ahead steps; the summary
line holds the medians and the kernel time per committed step.  JSON lines on stdout and in --out.

    python scripts/vs_expert_bench.py --out profiles/vs_expert_bench.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monsoon_amd import EXPERT  # noqa: E402
from monsoon_amd.cards import deck_indices  # noqa: E402
from monsoon_amd.engine import BatchEngine  # noqa: E402
from monsoon_amd.fitness import MATCH_DTYPE  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--max-turns", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--deck", default="N12M")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.games
    w = np.random.RandomState(2024).uniform(0, 1, 10)[None]
    d = deck_indices(args.deck)
    pairs = np.stack([d, d])[None]
    sched = {}
    for name, p1, p2 in (("bot_second", 0, EXPERT), ("bot_first", EXPERT, 0), ("self_play", 0, 0)):
        m = np.zeros(n, dtype=MATCH_DTYPE)
        m["p1"], m["p2"], m["seed"] = p1, p2, np.arange(n)
        sched[name] = m
    eng = BatchEngine(n)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def run(name):
        m = sched[name]
        play = eng.rollout if name == "self_play" else eng.rollout_vs_expert
        st0, (k0, _) = eng.stats(), eng.kernel_time()
        t0 = time.perf_counter()
        _, results, steps = play(w, m, pairs, args.max_turns, want_results=True)
        wall = (time.perf_counter() - t0) * 1e3
        st1, (k1, _) = eng.stats(), eng.kernel_time()
        return dict(config=name, games=n, wall_ms=wall, kernel_ms=k1 - k0, steps=int(steps.sum()),
                    decisions=st1["decisions"] - st0["decisions"], lookahead_steps=st1["lookahead_steps"] - st0["lookahead_steps"],
                    capped=int((steps == args.max_turns).sum()), draws=int((results == -1).sum()))

    for name in sched:   # warm-up: code objects, launch-time buffers
        run(name)
    reps = {name: [] for name in sched}
    for rep in range(args.reps):
        for name in sched:   # alternating
            r = run(name)
            r["rep"] = rep
            reps[name].append(r)
            emit(r)
    for name, rs in reps.items():
        med = lambda k: float(np.median([r[k] for r in rs]))   # noqa: E731
        ns = [r["kernel_ms"] * 1e6 / r["steps"] for r in rs]
        emit(dict(config=name, summary=True, games=n, deck=args.deck, max_turns=args.max_turns, reps=args.reps, wall_ms=med("wall_ms"),
                  kernel_ms=med("kernel_ms"), steps=rs[0]["steps"], decisions=rs[0]["decisions"], lookahead_steps=rs[0]["lookahead_steps"],
                  capped=rs[0]["capped"], kernel_ns_per_step=float(np.median(ns)), kernel_ns_per_step_min=min(ns), kernel_ns_per_step_max=max(ns)))
    eng.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
