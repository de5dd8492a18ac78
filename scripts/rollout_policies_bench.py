#!/usr/bin/env python3
"""What a rule per individual costs a sampling rollout: monsoon_rollout_policies (k_play_policy) next to
monsoon_rollout_sample (k_play_sample) on the same handle, the same schedules, in one process.

Workload: rollout_sample_bench.py's -- --games matches of N12M against N12M, max_turns 200, 64 weight vectors, as a plain
schedule (no bot) and a mixed one (a third each of bot-FIRST, bot-SECOND and plain matches); 45 056 games are ONE batch of
the 29-byte log.  Arms, called in turn (alternating, so that a drift of the box hits them alike), all eight arrays each:
  * sample_25:       explore=Explore(0.25, s, temperature=1.0) -- the yardstick, an existing kernel;
  * policies_same:   explore=Policies with eps 0.25 / T 1.0 in every row -- the very same games (the assertion below checks the
                     steps): two table loads per decision, and sample_pick also on the covered decisions that did not sample;
  * policies_mixed:  rows cycling through greedy, uniform at 0.5, T = 1 at eps = 1, T = 0.25 at eps = 0.3 -- other games;
  * sample_100 / policies_100:  the first two arms at eps = 1, where every covered decision samples in both calls (the same
                     games again): what is left between them is the table loads alone.
Method: --reps rounds after --warmup; per call the kernel time is the difference of BatchEngine.kernel_time() (HIP events
round the launch) and the wall time is the whole Python call, which ends in the library's synchronise.  One JSON line per
schedule and arm with the median, min and max of both, and policies_same / sample_25 and policies_100 / sample_100 of the
kernel medians, appended to --out.
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
from monsoon_amd.engine import BatchEngine, Explore, Policies, sample_entry_bytes  # noqa: E402
from monsoon_amd.fitness import MATCH_DTYPE, hash32_array  # noqa: E402

ROWS = 64


def summary(v):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], 3), min=round(v[0], 3), max=round(v[-1], 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--games", type=int, default=45056)
    ap.add_argument("--max-turns", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rollout_policies_bench.jsonl"))
    args = ap.parse_args()
    n, T = args.games, args.max_turns
    d = deck_indices("N12M")
    pairs = np.stack([d, d])[None]
    w = np.random.RandomState(42).uniform(0, 1, (ROWS, 10))
    k = np.arange(n)
    plain = np.zeros(n, dtype=MATCH_DTYPE)
    plain["p1"], plain["p2"], plain["seed"] = k % ROWS, (k + 1) % ROWS, hash32_array(0, k, 0xE)
    mixed = plain.copy()
    mixed["p1"][k % 3 == 0] = EXPERT
    mixed["p2"][k % 3 == 1] = EXPERT
    eng = BatchEngine(n)
    cycle = np.arange(ROWS) % 4
    arms = {
        "sample_25": Explore(0.25, 7, temperature=1.0),
        "policies_same": Policies(np.full(ROWS, 0.25), np.ones(ROWS), 7),
        "policies_mixed": Policies(np.array([0.0, 0.5, 1.0, 0.3])[cycle], np.array([1.0, np.inf, 1.0, 0.25])[cycle], 7),
        "sample_100": Explore(1.0, 7, temperature=1.0),
        "policies_100": Policies(np.ones(ROWS), np.ones(ROWS), 7),
    }
    rows = []
    for name, m in (("plain", plain), ("mixed", mixed)):
        kernel, wall, facts = {a: [] for a in arms}, {a: [] for a in arms}, {}
        for i in range(args.warmup + args.reps):
            for a, rule in arms.items():
                k0 = eng.kernel_time()[0]
                t0 = time.perf_counter()
                log = eng.rollout_logged(w, m, pairs, T, explore=rule)[3]
                t1 = time.perf_counter()
                if i >= args.warmup:
                    kernel[a].append(eng.kernel_time()[0] - k0)
                    wall[a].append((t1 - t0) * 1e3)
                if a not in facts:
                    facts[a] = dict(committed_steps=int(log.steps.sum()), decisions=int((log.n_legal > 0).sum()),
                                    lookahead_steps=int(log.n_legal.astype(np.int64).sum()), weighed=int((log.weight_total != 0).sum()),
                                    left_argmax_by_draw=int(log.explored.sum()),
                                    restepped=int(((log.explored != 0) & (log.action != log.greedy)).sum()))
                    facts[a]["steps"] = log.steps.copy()
        for a, b in (("sample_25", "policies_same"), ("sample_100", "policies_100")):   # the same games
            assert np.array_equal(facts[a].pop("steps"), facts[b].pop("steps")) and facts[a]["restepped"] == facts[b]["restepped"]
        facts["policies_mixed"].pop("steps")
        ratio = round(summary(kernel["policies_same"])["median"] / summary(kernel["sample_25"])["median"], 4)
        ratio_100 = round(summary(kernel["policies_100"])["median"] / summary(kernel["sample_100"])["median"], 4)
        for a in arms:
            ks, ws, f = summary(kernel[a]), summary(wall[a]), facts[a]
            row = dict(schedule=name, arm=a, games=n, max_turns=T, **f, kernel_ms=ks, wall_ms=ws,
                       games_per_s_kernel=round(n / ks["median"] * 1e3), decisions_per_s_kernel=round(f["decisions"] / ks["median"] * 1e3),
                       games_per_s_wall=round(n / ws["median"] * 1e3),
                       kernel_ns_per_lookahead_step=round(ks["median"] * 1e6 / max(f["lookahead_steps"], 1), 2),
                       log_bytes_copied=n * T * sample_entry_bytes(), policies_same_over_sample_25_kernel=ratio,
                       policies_100_over_sample_100_kernel=ratio_100, reps=args.reps)
            rows.append(row)
            print(json.dumps(row), flush=True)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
