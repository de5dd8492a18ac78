#!/usr/bin/env python3
"""What the device replay of a game log costs: game_log.dataset (k_replay_log) next to the generator it complements and
to the rollout that wrote the log.

Workload: --games matches (default 8 192) of N12M against N12M, max_turns 200, 64 weight vectors, logged once by
rollout_logged.  Arms on the bot-free schedule:
  * replay_generator: game_log.replay drained (reset / legal_mask / observe / step per step index; the baseline),
  * dataset_all: game_log.dataset with every column,
  * dataset_no_hash: every column but state_hash (the canonical record and its hash are one lane's serial work per row),
  * dataset_columns: game_log.dataset with action / to_play only (no observation, no legal bytes, no hash),
  * rollout_logged: the rollout that wrote the log (k_play_log), for the ratio replay : play,
  * dataset_after_features: dataset with the candidates of every row (k_replay_after): after_features + before_features,
    K = 64, no observations -- the committed steps of dataset_columns plus the look-ahead steps of rollout_logged,
  * dataset_after_obs: the same with after_obs (138 KB per row), on the first --obs-games games (default games / 16).
And dataset_all on the mixed schedule (a third each of bot-FIRST, bot-SECOND and plain matches), whose bot steps run
expert_action again.
Method: one handle, the arms called in turn, --reps rounds after --warmup; per call the kernel time is the difference of
BatchEngine.kernel_time() (HIP events round the launch) and the wall time is the whole Python call (for dataset: the
allocation of the tensors, the reset, the copy of the log to the device, the launch and the copy of the outcome back).
One JSON line per schedule and arm with the median, min and max of both, appended to --out; the dataset arms add rows/s
and the bandwidth of their row writes by kernel time (the MI355X's HBM peak is 8 TB/s).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the library loads: monsoon_amd/vec_env.py VecEnv.__init__)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from monsoon_amd import EXPERT, game_log  # noqa: E402
from monsoon_amd.cards import deck_indices  # noqa: E402
from monsoon_amd.engine import BatchEngine  # noqa: E402
from monsoon_amd.fitness import MATCH_DTYPE, hash32_array  # noqa: E402


def summary(v):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], 3), min=round(v[0], 3), max=round(v[-1], 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--games", type=int, default=8192)
    ap.add_argument("--max-turns", type=int, default=200)
    ap.add_argument("--obs-games", type=int, default=0, help="games of the dataset_after_obs arm (default: games / 16)")
    ap.add_argument("--max-after", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "replay_dataset_bench.jsonl"))
    args = ap.parse_args()
    n, T, K = args.games, args.max_turns, args.max_after
    n_obs = args.obs_games or max(n // 16, 1)
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
    all_bytes = sum(game_log.ROW_BYTES.values())
    col_bytes = game_log.ROW_BYTES["action"] + game_log.ROW_BYTES["to_play"]
    feat_bytes = col_bytes + 4 + 2 * K + 80 * K + 80   # n_legal, after_action + after_status, after_features, before_features (all K entries)
    rows_out = []
    for name, m in (("plain", plain), ("mixed", mixed)):
        log = eng.rollout_logged(w, m, pairs, T)[3]
        entries = int(log.steps.sum())

        def drain():
            for _ in game_log.replay(eng, m, pairs, log):
                pass
            return entries

        def dataset(columns):
            out = game_log.dataset(eng, m, pairs, log, columns=columns)
            assert not out["status"].any() and len(out["action"]) == entries
            return entries

        def candidates(columns, games):   # the first `games` games, with the look-ahead of every row
            sub = game_log.RolloutLog(log.action[:games], None, None, log.steps[:games])
            out = game_log.dataset(eng, m[:games], pairs, sub, columns=columns, max_after=K)
            assert not out["status"].any()
            return len(out["action"])

        arms = {"dataset_all": (lambda: dataset(tuple(game_log.COLUMNS)), all_bytes)}
        if name == "plain":
            no_hash = tuple(c for c in game_log.COLUMNS if c != "state_hash")
            arms = {"replay_generator": (drain, 0), **arms, "dataset_no_hash": (lambda: dataset(no_hash), all_bytes - 8),
                    "dataset_columns": (lambda: dataset(("to_play",)), col_bytes),
                    "rollout_logged": (lambda: int(eng.rollout_logged(w, m, pairs, T)[2].sum()), 0),
                    "dataset_after_features": (lambda: candidates(("to_play", "after_features", "before_features"), n), feat_bytes),
                    "dataset_after_obs": (lambda: candidates(("to_play", "after_features", "before_features", "after_obs"), n_obs),
                                          feat_bytes + 2160 * K)}
        kernel, wall = {a: [] for a in arms}, {a: [] for a in arms}
        rows_of = {a: entries for a in arms}
        rows_of["dataset_after_obs"] = int(log.steps[:n_obs].sum())
        for i in range(args.warmup + args.reps):
            for a, (fn, _) in arms.items():
                k0 = eng.kernel_time()[0]
                t0 = time.perf_counter()
                assert fn() == rows_of[a]
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if i >= args.warmup:
                    kernel[a].append(eng.kernel_time()[0] - k0)
                    wall[a].append((t1 - t0) * 1e3)
        for a, (_, row_bytes) in arms.items():
            rows = rows_of[a]
            row = dict(schedule=name, arm=a, games=n_obs if a == "dataset_after_obs" else n, max_turns=T, rows=rows,
                       kernel_ms=summary(kernel[a]), wall_ms=summary(wall[a]), reps=args.reps)
            if a.startswith("dataset_after"):
                row.update(max_after=K)
            if row_bytes and row["kernel_ms"]["median"] > 0:
                sec = row["kernel_ms"]["median"] / 1e3
                row.update(row_bytes=row_bytes, rows_per_s=round(rows / sec), write_gb_per_s=round(rows * row_bytes / sec / 1e9, 1),
                           rows_per_s_wall=round(rows / (row["wall_ms"]["median"] / 1e3)))
            rows_out.append(row)
            print(json.dumps(row), flush=True)
    eng.close()
    with open(args.out, "a") as f:
        for row in rows_out:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
