#!/usr/bin/env python3
"""Cost of VecEnv.snapshot / VecEnv.restore (monsoon_env_save_dev / monsoon_env_load_dev: k_env_save, k_env_load,
k_env_view) next to a plain device copy of as many bytes.

Workload: --slots slots (default 65 536) of the standard record, opponent none, N12M decks, advanced --advance steps
(default 12) by a random policy.

Method (one JSON line per measurement; as scripts/env_afterstates_bench.py):
  * every figure is the median (min - max) of --reps event-bracketed repetitions after --warmup warm-ups; the event pair
    brackets the Python call on the env's stream, so the ctypes and enqueue cost of a call (some 10 us) is inside it.
  * snapshot: all slots into an existing snapshot (out=).  restore 1:1: that snapshot back into its slots.  restore
    fork 16: the first slots / 16 entries, each into 16 consecutive slots, all slots written.
  * copy part and views part: the same restores on a second env whose obs / legal / obs_raises / to_play views are NULL
    (it was given the first env's entries, so it holds the same states): there k_env_view loads the record and writes
    the per-call bytes only.  views part = full restore - restore without those views.
  * the yardstick is torch's device copy of slots * entry_bytes bytes in the same run; GB/s counts those bytes once (the
    copy reads and writes each of them, as the kernels do: the fork reads a sixteenth of them).  ratio = copy time / time.
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


class BareEnv(VecEnv):
    """A VecEnv whose state views are NULL: only the per-call bytes are written."""

    def _alloc(self, n):
        views = super()._alloc(n)
        for name in ("obs", "legal", "obs_raises", "to_play"):
            views[name] = views[name][:0]   # an empty tensor's data_ptr() is 0
        return views


def timed(torch, stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        fn()
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(torch, stream, fn, warmup, reps):
    ms = sorted([timed(torch, stream, fn) for _ in range(warmup + reps)][warmup:])
    return dict(median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--slots", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--advance", type=int, default=12)
    ap.add_argument("--fork", type=int, default=16)
    ap.add_argument("--label", default="", help="free text copied into every line")
    args = ap.parse_args()
    import torch
    n = args.slots
    seed0 = np.arange(n, dtype=np.uint32) + 1000
    deck = np.stack([deck_indices("N12M"), deck_indices("N12M")])
    env, bare = VecEnv(n), BareEnv(n)
    views = env.reset(seed0, deck)
    bare.reset(seed0, deck)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    for _ in range(args.advance):
        u = torch.rand(views["legal"].shape, device="cuda", generator=gen)
        u.masked_fill_(~views["legal"], -1.0)
        views = env.step(u.argmax(dim=1).to(torch.uint8))
    snap = env.snapshot()
    torch.cuda.synchronize()
    loaded = torch.zeros(n, dtype=torch.uint8, device="cuda")
    bare.restore(snap, loaded=loaded)
    torch.cuda.synchronize()
    assert bool(loaded.all()) and np.array_equal(bare.state_hash(), env.state_hash())
    size = env.entry_bytes
    nbytes = n * size
    roots = n // args.fork
    src = (torch.arange(n, device="cuda") // args.fork).to(torch.int32)
    dst = torch.arange(n, device="cuda", dtype=torch.int32)
    roots_snap = env.snapshot(torch.arange(roots, device="cuda", dtype=torch.int32))
    a, b = torch.zeros(nbytes // 4, dtype=torch.int32, device="cuda"), torch.empty(nbytes // 4, dtype=torch.int32, device="cuda")
    w, r = args.warmup, args.reps
    rows = [
        ("torch_copy", measure(torch, env.stream, lambda: b.copy_(a), w, r)),
        ("snapshot", measure(torch, env.stream, lambda: env.snapshot(out=snap), w, r)),
        ("restore_1to1", measure(torch, env.stream, lambda: env.restore(snap), w, r)),
        ("restore_1to1_no_state_views", measure(torch, bare.stream, lambda: bare.restore(snap), w, r)),
        (f"restore_fork{args.fork}", measure(torch, env.stream, lambda: env.restore(roots_snap, src, dst), w, r)),
        (f"restore_fork{args.fork}_no_state_views", measure(torch, bare.stream, lambda: bare.restore(roots_snap, src, dst), w, r)),
        ("torch_copy_again", measure(torch, env.stream, lambda: b.copy_(a), w, r)),
    ]
    copy_ms = rows[0][1]["median_ms"]
    for name, t in rows:
        print(json.dumps(dict(what=name, slots=n, entry_bytes=size, bytes=nbytes, label=args.label, advance=args.advance, **t,
                              gb_per_s=round(nbytes / (t["median_ms"] * 1e-3) / 1e9, 1),
                              ratio_to_torch_copy=round(copy_ms / t["median_ms"], 3))), flush=True)
    env.close()
    bare.close()


if __name__ == "__main__":
    main()
