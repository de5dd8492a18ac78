#!/usr/bin/env python3
"""What logging costs a rollout: monsoon_rollout_logged (k_play_log) next to the unlogged rollouts on the same handle.

Workload: --games matches (default 65 536) of N12M against N12M, max_turns 200, 64 weight vectors, as two schedules:
  * plain: no bot.  Arms: rollout (k_play), rollout_vs_expert (k_play too: a batch without a bot is k_play's),
    rollout_logged with the action array only, rollout_logged with all three arrays (k_play_log).
  * mixed: a third each of bot-FIRST, bot-SECOND and plain matches.  Arms: rollout_vs_expert (k_play_vs) and the two
    rollout_logged forms.
Method: one handle, the arms of a schedule called in turn, --reps rounds after --warmup; per call the kernel time is the
difference of BatchEngine.kernel_time() (HIP events round the launch) and the wall time is the whole Python call: reset,
launch, collection and, for the logged arms, the fill of the device log, its copy to the host and the allocation of the
host arrays.  One JSON line per schedule and arm with the median, min and max of both, appended to --out.
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
from monsoon_amd.engine import BatchEngine  # noqa: E402
from monsoon_amd.fitness import MATCH_DTYPE, hash32_array  # noqa: E402


def summary(v):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], 3), min=round(v[0], 3), max=round(v[-1], 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--max-turns", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rollout_log_bench.jsonl"))
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
        "rollout": lambda m: eng.rollout(w, m, pairs, T, want_results=True)[2],
        "rollout_vs_expert": lambda m: eng.rollout_vs_expert(w, m, pairs, T, want_results=True)[2],
        "rollout_logged_action": lambda m: eng.rollout_logged(w, m, pairs, T, scores=False, n_legal=False)[2],
        "rollout_logged_all": lambda m: eng.rollout_logged(w, m, pairs, T)[2],
    }
    rows = []
    for name, m in (("plain", plain), ("mixed", mixed)):
        names = [a for a in arms if name == "plain" or a != "rollout"]
        kernel, wall, steps = {a: [] for a in names}, {a: [] for a in names}, {}
        for i in range(args.warmup + args.reps):
            for a in names:
                k0 = eng.kernel_time()[0]
                t0 = time.perf_counter()
                s = arms[a](m)
                t1 = time.perf_counter()
                if i >= args.warmup:
                    kernel[a].append(eng.kernel_time()[0] - k0)
                    wall[a].append((t1 - t0) * 1e3)
                steps[a] = int(s.sum())
        assert len(set(steps.values())) == 1, steps   # every arm played the same games
        for a in names:
            entries = steps[a]
            log_bytes = 0 if "logged" not in a else n * T * (11 if a.endswith("all") else 1)
            row = dict(schedule=name, arm=a, games=n, max_turns=T, committed_steps=entries, kernel_ms=summary(kernel[a]),
                       wall_ms=summary(wall[a]), log_bytes_copied=log_bytes, reps=args.reps)
            rows.append(row)
            print(json.dumps(row), flush=True)
    eng.close()
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
