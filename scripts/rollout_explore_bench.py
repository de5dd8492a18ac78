#!/usr/bin/env python3
"""What exploring costs a logged rollout: monsoon_rollout_explore (k_play_explore) next to monsoon_rollout_logged
(k_play_log) on the same handle, the same schedule, in one process.

Workload: --games matches of N12M against N12M, max_turns 200, 64 weight vectors (default 61 440 games: the 21-byte log of
the exploring call lets 63 913 games of 200 turns into a batch, so every arm plays the schedule as ONE batch), as two schedules:
  * plain: no bot;
  * mixed: a third each of bot-FIRST, bot-SECOND and plain matches.
Arms, called in turn (alternating, so that a drift of the box hits them alike):
  * logged:     rollout_logged(...), all three arrays -- the yardstick, the call as it was before exploration existed;
  * explore_0:  rollout_logged(..., explore=Explore(0.0, s)) -- k_play_explore playing the very same games (the assertion
                below checks the steps), all six arrays: the cost of the kernel's form and of the larger log alone;
  * explore_10: rollout_logged(..., explore=Explore(0.1, s)) -- other games, usually longer ones, so the figure to compare
                is the time per committed step next to the time per call.
Method: --reps rounds after --warmup; per call the kernel time is the difference of BatchEngine.kernel_time() (HIP events
round the launch) and the wall time is the whole Python call, which ends in the library's synchronise: reset, launch,
collection, the fill of the device log, its copy to the host and the allocation of the host arrays.  One JSON line per
schedule and arm with the median, min and max of both, and both per committed step, appended to --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from monsoon_amd import EXPERT  # noqa: E402
from monsoon_amd.cards import deck_indices  # noqa: E402
from monsoon_amd.engine import BatchEngine, Explore, explore_entry_bytes  # noqa: E402
from monsoon_amd.fitness import MATCH_DTYPE, hash32_array  # noqa: E402


def summary(v):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], 3), min=round(v[0], 3), max=round(v[-1], 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--games", type=int, default=61440)
    ap.add_argument("--max-turns", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rollout_explore_bench.jsonl"))
    args = ap.parse_args()
    n, T = args.games, args.max_turns
    d = deck_indices("N12M")
    pairs = np.stack([d, d])[None]
    w = np.random.RandomState(42).uniform(0, 1, (64, 10))
    k = np.arange(n)
    plain = np.zeros(n, dtype=MATCH_DTYPE)
    plain["p1"], plain["p2"], plain["seed"] = k % 64, (k + 1) % 64, hash32_array(0, k, 0xE)
    mixed = plain.copy()
    mixed["p1"][k % 3 == 0] = EXPERT
    mixed["p2"][k % 3 == 1] = EXPERT
    eng = BatchEngine(n)
    arms = {
        "logged": (None, 11),
        "explore_0": (Explore(0.0, 7), explore_entry_bytes()),
        "explore_10": (Explore(0.1, 7), explore_entry_bytes()),
    }
    rows = []
    for name, m in (("plain", plain), ("mixed", mixed)):
        kernel, wall, steps, explored = {a: [] for a in arms}, {a: [] for a in arms}, {}, {}
        for i in range(args.warmup + args.reps):
            for a, (rule, _) in arms.items():
                k0 = eng.kernel_time()[0]
                t0 = time.perf_counter()
                log = eng.rollout_logged(w, m, pairs, T, explore=rule)[3]
                t1 = time.perf_counter()
                if i >= args.warmup:
                    kernel[a].append(eng.kernel_time()[0] - k0)
                    wall[a].append((t1 - t0) * 1e3)
                steps[a] = int(log.steps.sum())
                explored[a] = 0 if log.explored is None else int(log.explored.sum())
        assert steps["logged"] == steps["explore_0"] and explored["explore_0"] == 0, steps   # the same games
        for a, (_, entry_bytes) in arms.items():
            ks, ws = summary(kernel[a]), summary(wall[a])
            row = dict(schedule=name, arm=a, games=n, max_turns=T, committed_steps=steps[a], explored_decisions=explored[a], kernel_ms=ks,
                       wall_ms=ws, kernel_ns_per_step=round(ks["median"] * 1e6 / steps[a], 2), wall_ns_per_step=round(ws["median"] * 1e6 / steps[a], 2),
                       log_bytes_copied=n * T * entry_bytes, reps=args.reps)
            rows.append(row)
            print(json.dumps(row), flush=True)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
