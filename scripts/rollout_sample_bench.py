#!/usr/bin/env python3
"""What sampling costs a logged rollout: monsoon_rollout_sample (k_play_sample) next to monsoon_rollout_explore
(k_play_explore) at the same eps and to monsoon_rollout_logged (k_play_log), on the same handle, the same schedule, in one
process.

Workload: rollout_explore_bench.py's -- --games matches of N12M against N12M, max_turns 200, 64 weight vectors, as a plain
schedule (no bot) and a mixed one (a third each of bot-FIRST, bot-SECOND and plain matches).  Default 45 056 games: the
29-byte log of the sampling call lets 46 283 games of 200 turns into a batch, so every arm plays the schedule as ONE batch.
Arms, called in turn (alternating, so that a drift of the box hits them alike):
  * logged:       rollout_logged(...), all three arrays -- the yardstick;
  * sample_0:     explore=Explore(0.0, s, temperature=1.0) -- k_play_sample playing the very same games as `logged` (the
                  assertion below checks the steps), all eight arrays: the cost of the kernel's form and of the larger log alone;
  * explore_25 / explore_100:  explore=Explore(eps, s), the uniform rule at eps = 0.25 / 1.0, all six arrays;
  * sample_25 / sample_100:    explore=Explore(eps, s, temperature=1.0), the sampling rule at the same eps, all eight arrays.
The arms play different games (an explored game is not a sampled one), so the figures to compare are games/s next to
decisions/s and the time per look-ahead step; a sampling decision that does not draw its arg-max executes one step more than
lookahead counts (restepped = sampled decisions whose action is not the greedy one).
Method: --reps rounds after --warmup; per call the kernel time is the difference of BatchEngine.kernel_time() (HIP events
round the launch) and the wall time is the whole Python call, which ends in the library's synchronise.  One JSON line per
schedule and arm with the median, min and max of both, appended to --out.
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
from monsoon_amd.engine import BatchEngine, Explore, explore_entry_bytes, sample_entry_bytes  # noqa: E402
from monsoon_amd.fitness import MATCH_DTYPE, hash32_array  # noqa: E402


def summary(v):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], 3), min=round(v[0], 3), max=round(v[-1], 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--games", type=int, default=45056)
    ap.add_argument("--max-turns", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rollout_sample_bench.jsonl"))
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
        "sample_0": (Explore(0.0, 7, temperature=args.temperature), sample_entry_bytes()),
        "explore_25": (Explore(0.25, 7), explore_entry_bytes()),
        "sample_25": (Explore(0.25, 7, temperature=args.temperature), sample_entry_bytes()),
        "explore_100": (Explore(1.0, 7), explore_entry_bytes()),
        "sample_100": (Explore(1.0, 7, temperature=args.temperature), sample_entry_bytes()),
    }
    rows = []
    for name, m in (("plain", plain), ("mixed", mixed)):
        kernel, wall, facts = {a: [] for a in arms}, {a: [] for a in arms}, {}
        for i in range(args.warmup + args.reps):
            for a, (rule, _) in arms.items():
                k0 = eng.kernel_time()[0]
                t0 = time.perf_counter()
                log = eng.rollout_logged(w, m, pairs, T, explore=rule)[3]
                t1 = time.perf_counter()
                if i >= args.warmup:
                    kernel[a].append(eng.kernel_time()[0] - k0)
                    wall[a].append((t1 - t0) * 1e3)
                if a not in facts:
                    left = 0 if log.explored is None else int(((log.explored != 0) & (log.action != log.greedy)).sum())
                    facts[a] = dict(committed_steps=int(log.steps.sum()), decisions=int((log.n_legal > 0).sum()),
                                    lookahead_steps=int(log.n_legal.astype(np.int64).sum()),
                                    left_argmax_by_draw=0 if log.explored is None else int(log.explored.sum()),
                                    restepped=left if rule is not None and rule.samples else 0)
        assert facts["logged"]["committed_steps"] == facts["sample_0"]["committed_steps"] and facts["sample_0"]["left_argmax_by_draw"] == 0   # the same games
        for a, (_, entry_bytes) in arms.items():
            ks, ws, f = summary(kernel[a]), summary(wall[a]), facts[a]
            row = dict(schedule=name, arm=a, games=n, max_turns=T, **f, kernel_ms=ks, wall_ms=ws,
                       games_per_s_kernel=round(n / ks["median"] * 1e3), decisions_per_s_kernel=round(f["decisions"] / ks["median"] * 1e3),
                       games_per_s_wall=round(n / ws["median"] * 1e3), decisions_per_s_wall=round(f["decisions"] / ws["median"] * 1e3),
                       kernel_ns_per_lookahead_step=round(ks["median"] * 1e6 / max(f["lookahead_steps"], 1), 2),
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
