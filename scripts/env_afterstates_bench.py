#!/usr/bin/env python3
"""Cost of VecEnv.afterstates (monsoon_env_afterstates_dev, k_env_after) next to a one-decision k_play launch.

Workload: --slots slots (default 65 536), opponent none, N12M decks or a per-episode pool (every card of the standard
record but up01/up02/up03), K = --max-after (default 64).

Method (one JSON line per configuration):
  * first state: the env sits in the first state of episode 0; a second handle is reset to the same seeds and decks, given
    one weight vector, and asked for monsoon_play_rounds_dev(1) -- the same legal mask, clones, steps and features plus
    arg-max, commit and refill.  The two launches alternate, --reps times each after --warmup; the second handle is reset
    before each of its launches, outside the timed region, so both always work on the same states.  Each launch is timed
    with a pair of events on its own stream; median and min / max are reported.
  * mid-game: the env is advanced --advance steps by a random policy, then afterstates with obs off and on are timed the
    same way, and a plain device copy of as many bytes as the obs phase wrote.
  * the event pair brackets the Python call, so a launch's ctypes and enqueue cost (some 10 us) is inside every figure, on
    both sides of the yardstick alike; per-kernel times without it come from a separate `rocprofv3 --kernel-trace --stats`
    run of this script.
  * bytes written come from the outputs themselves (entries with status 0 get features and an observation).
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from monsoon_amd.cards import CARD_INDEX, deck_indices, supported_pool  # noqa: E402
from monsoon_amd.engine import BatchEngine  # noqa: E402
from monsoon_amd.vec_env import VecEnv  # noqa: E402


def timed(torch, stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        fn()
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(ms):
    ms = sorted(ms)
    return dict(median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4))


def written(after, obs):
    k = after["action"].shape[1]
    import torch
    shown = torch.arange(k, device="cuda")[None, :] < after["n_legal"][:, None]
    entries = int(shown.sum())
    ok = int((shown & (after["status"] == 0)).sum())
    n = after["n_legal"].shape[0]
    small = n * 4 + n * k + entries * 3 + n * 80 + ok * 80   # n_legal, the action row, status / reward / winner, features
    return entries, ok, small, ok * 2160 if obs else 0


def sample(torch, legal, gen):
    u = torch.rand(legal.shape, device=legal.device, generator=gen)
    u.masked_fill_(~legal, -1.0)
    return u.argmax(dim=1).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--slots", type=int, default=65536)
    ap.add_argument("--max-after", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--advance", type=int, default=12)
    ap.add_argument("--label", default="", help="free text copied into every line (e.g. the obs-write form of the build)")
    args = ap.parse_args()
    import torch
    n, k = args.slots, args.max_after
    seed0 = np.arange(n, dtype=np.uint32) + 1000
    deck = np.stack([deck_indices("N12M"), deck_indices("N12M")])
    pool = np.array(sorted(CARD_INDEX[c] for c in supported_pool()), dtype=np.uint8)
    w = np.random.RandomState(42).uniform(0, 1, (1, 10))
    for name, p in (("N12M", None), ("pool", pool)):
        env = VecEnv(n)
        views = env.reset(seed0, None if p is not None else deck, pool=p)
        eng = BatchEngine(n)
        decks = np.broadcast_to(deck, (n, 2, 12)).copy() if p is None else eng.draw_decks(seed0 ^ np.uint32(0x9E3779B9), p)
        eng_stream = torch.cuda.ExternalStream(eng.stream_ptr(), device=torch.device("cuda", 0))
        zeros = np.zeros(n, dtype=np.int32)

        def fresh():
            eng.reset(seed0, decks)
            eng.upload_weights(w)
            eng.assign_players(zeros, zeros)
            eng.sync()

        t_after, t_play = [], []
        for i in range(args.warmup + args.reps):
            a = timed(torch, env.stream, lambda: env.afterstates(k, obs=False))
            fresh()
            b = timed(torch, eng_stream, lambda: eng.play_rounds(1))
            if i >= args.warmup:
                t_after.append(a)
                t_play.append(b)
        first = written(env.afterstates(k, obs=False), False)
        row = dict(config=name, slots=n, max_after=k, label=args.label, first_state=dict(
            afterstates=first[0], afterstates_no_obs=summary(t_after), k_play_one_decision=summary(t_play),
            afterstates_per_s=round(first[0] / (sorted(t_after)[len(t_after) // 2] * 1e-3))))
        eng.close()
        gen = torch.Generator(device="cuda")
        gen.manual_seed(7)
        for _ in range(args.advance):
            views = env.step(sample(torch, views["legal"], gen))
        torch.cuda.synchronize()
        t_off, t_on = [], []
        for i in range(args.warmup + args.reps):
            a = timed(torch, env.stream, lambda: env.afterstates(k, obs=False))
            b = timed(torch, env.stream, lambda: env.afterstates(k, obs=True))
            if i >= args.warmup:
                t_off.append(a)
                t_on.append(b)
        entries, ok, small, obs_bytes = written(env.afterstates(k, obs=True), True)
        src = torch.zeros(max(obs_bytes, 4) // 4, dtype=torch.int32, device="cuda")
        dst = torch.empty_like(src)
        t_copy = [timed(torch, env.stream, lambda: dst.copy_(src)) for _ in range(args.warmup + args.reps)][args.warmup:]
        off, on, cp = (sorted(x)[len(x) // 2] for x in (t_off, t_on, t_copy))
        copy_gbs = obs_bytes / (cp * 1e-3) / 1e9
        row["mid_game"] = dict(
            advance=args.advance, afterstates=entries, with_features_and_obs=ok, no_obs=summary(t_off), obs=summary(t_on),
            afterstates_per_s_no_obs=round(entries / (off * 1e-3)), afterstates_per_s_obs=round(entries / (on * 1e-3)),
            bytes_small_outputs=small, bytes_obs=obs_bytes, obs_extra_ms=round(on - off, 4), device_copy=summary(t_copy),
            device_copy_gb_per_s_written=round(copy_gbs, 1), obs_bytes_over_copy_bandwidth_ms=round(cp, 4),
            obs_write_gb_per_s=round(obs_bytes / (max(on - off, 1e-6) * 1e-3) / 1e9, 1),
            obs_write_share_of_copy_bandwidth=round(cp / max(on - off, 1e-6), 3))
        print(json.dumps(row), flush=True)
        env.close()


if __name__ == "__main__":
    main()
