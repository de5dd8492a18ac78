#!/usr/bin/env python3
"""Cost of VecEnv.determinize next to VecEnv.restore for the same pairs (monsoon_env_load_determinized_dev: k_env_load_det,
k_env_determinize, k_env_view; monsoon_env_load_dev: k_env_load, k_env_view).

Workload: --slots forks (default 65 536) of --entries entries (default 1 024) of the standard record, opponent none,
N12M decks, the roots advanced --advance steps (default 12) by a random policy; fork j is entry j // (slots / entries)
loaded into slot j.

Method (one JSON line per measurement; as scripts/env_snapshot_bench.py):
  * every figure is the median (min - max) of --reps event-bracketed repetitions after --warmup warm-ups; the event pair
    brackets the Python call on the env's stream, so the ctypes and enqueue cost of a call (some 10 us) is inside it.
  * the three calls alternate inside a repetition (restore, determinize stream, determinize hand, restore again ...), so a
    drift of the machine shows in all of them; restore is measured a second time at the end.
  * ratio = restore's median / the call's median, on this run.
Before the timing the script checks that the determinized slots differ from the restored ones where they should: the
stream in both modes, the record in "hand" only.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from monsoon_amd.cards import deck_indices  # noqa: E402
from monsoon_amd.vec_env import VecEnv  # noqa: E402


def timed(torch, stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        fn()
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--slots", type=int, default=65536)
    ap.add_argument("--entries", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--advance", type=int, default=12)
    ap.add_argument("--label", default="", help="free text copied into every line")
    args = ap.parse_args()
    import torch
    n, roots = args.slots, args.entries
    assert n % roots == 0
    deck = np.stack([deck_indices("N12M"), deck_indices("N12M")])
    env = VecEnv(n)
    views = env.reset(np.arange(n, dtype=np.uint32) + 1000, deck)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    for _ in range(args.advance):
        u = torch.rand(views["legal"].shape, device="cuda", generator=gen)
        u.masked_fill_(~views["legal"], -1.0)
        views = env.step(u.argmax(dim=1).to(torch.uint8))
    snap = env.snapshot(torch.arange(roots, device="cuda", dtype=torch.int32))
    src = (torch.arange(n, device="cuda") // (n // roots)).to(torch.int32)
    dst = torch.arange(n, device="cuda", dtype=torch.int32)
    seeds = torch.from_numpy((np.arange(n, dtype=np.uint32) * np.uint32(2654435761)).view(np.int32).copy()).cuda()
    loaded = torch.zeros(n, dtype=torch.uint8, device="cuda")
    calls = [("restore", lambda: env.restore(snap, src, dst, loaded)),
             ("determinize_stream", lambda: env.determinize(snap, seeds, src, dst, what="stream", loaded=loaded)),
             ("determinize_hand", lambda: env.determinize(snap, seeds, src, dst, what="hand", loaded=loaded))]
    # what the calls leave, before anything is timed
    size = env.entry_bytes
    mt_at = size - 3 * 624 * 4
    left = {}
    for name, fn in calls:
        fn()
        torch.cuda.synchronize()
        assert bool(loaded.all()), name
        left[name] = env.snapshot().data
    running = left["restore"][:, 24] == 0xFE   # GameMeta.result == -2
    rec = lambda t: t[:, 80:mt_at]   # noqa: E731
    assert bool((rec(left["determinize_stream"]) == rec(left["restore"])).all())
    assert bool(((left["determinize_stream"][:, mt_at:] != left["restore"][:, mt_at:]).any(dim=1) == running).all())
    assert bool((left["determinize_hand"][:, mt_at:] == left["determinize_stream"][:, mt_at:]).all())
    redealt = int((rec(left["determinize_hand"]) != rec(left["restore"])).any(dim=1).sum())
    del left
    times = {name: [] for name, _ in calls}
    for i in range(args.warmup + args.reps):
        for name, fn in calls:
            ms = timed(torch, env.stream, fn)
            if i >= args.warmup:
                times[name].append(ms)
    times["restore_again"] = [timed(torch, env.stream, calls[0][1]) for _ in range(args.warmup + args.reps)][args.warmup:]
    base = sorted(times["restore"])[len(times["restore"]) // 2]
    for name, ms in times.items():
        ms = sorted(ms)
        med = ms[len(ms) // 2]
        print(json.dumps(dict(what=name, forks=n, entries=roots, entry_bytes=size, running=int(running.sum()), redealt=redealt,
                              label=args.label, advance=args.advance, median_ms=round(med, 4), min_ms=round(ms[0], 4),
                              max_ms=round(ms[-1], 4), us_per_fork=round(med * 1e3 / n, 4), ratio_to_restore=round(base / med, 3))), flush=True)
    env.close()


if __name__ == "__main__":
    main()
