#!/usr/bin/env python3
"""How empty the GPU runs at the end of one k_play launch of several decisions per game (the launch's drain), from the
per-visit wall-clock stamps of the profiling build libmonsoon_hip_prof.so (scripts/phase_profile.py has the phases).

    make -C monsoon_amd/csrc prof && python scripts/launch_tail.py [--games 65536] [--rounds 8] [--repeat 5]

A visit is one game's `rounds` decisions by one wavefront.  Per measured launch: its span, the average number of
wavefronts inside a visit (sum of visit times / span) against the persistent grid, and the drain: from the start of the
last visit (the moment the last game is popped) to the end of the launch.  1 - resident average / grid bounds what
filling the drain with the next launch's games can gain.  --grid is the product's (20 wavefronts x 256 CUs); the
profiling build keeps 928 bytes more of LDS per wavefront and may hold fewer, so read the share against the grid as an
upper bound and the drain as the direct figure.  MONSOON_SPLIT=0 is set: one launch, one stream.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ["MONSOON_SPLIT"] = "0"
os.environ.setdefault("MONSOON_PROF_WINDOW_MS", "1000")   # the stamps of one long launch: reset_stats cleared the older ones
import monsoon_amd._lib as L  # noqa: E402

L.LIB_PATH = os.path.join(REPO, "monsoon_amd", os.environ.get("MSB_PROF_LIB", "libmonsoon_hip_prof.so"))
from monsoon_amd.cards import deck_indices  # noqa: E402
from monsoon_amd.engine import BatchEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--grid", type=int, default=int(os.environ.get("MONSOON_GRID", 5120)),
                    help="persistent grid of the launch: 20 wavefronts x 256 CUs unless MONSOON_GRID says otherwise")
    args = ap.parse_args()
    n = args.games
    eng = BatchEngine(n)
    deck = deck_indices("N12M")
    eng.reset(np.arange(n, dtype=np.uint32), np.stack([deck, deck]))
    eng.upload_weights(np.random.RandomState(2024).uniform(0, 1, 10).reshape(1, 10))
    eng.assign_players(np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32))
    for _ in range(args.warmup):
        eng.play_rounds(args.rounds)
    eng.sync()
    print(f"games {n}, {args.rounds} decisions per launch, grid {args.grid}")
    fr, dr = [], []
    for i in range(args.repeat):
        eng.reset_stats()   # clears the stamps: what is read below is this launch's
        eng.play_rounds(args.rounds)
        eng.sync()
        c = np.zeros(192, dtype=np.uint64)
        eng._ck(eng.lib.monsoon_debug_counters(eng.h, c.ctypes.data_as(ctypes.c_void_p)), "counters")
        kms, launches = eng.kernel_time()
        if not c[96]:
            print("no stamps: not a profiling build")
            return 1
        span, total, _, longest, nv, last_start = (float(c[j]) / 100 for j in range(96, 102))   # 100 MHz -> us
        nv = int(c[100])
        drain = span - last_start
        fr.append(total / span / args.grid)
        dr.append(drain / span)
        print(f"launch {i}: k_play {kms / max(launches, 1):.3f} ms, span {span:.0f} us, {nv} visits, mean visit {total / nv:.0f} us, "
              f"longest {longest:.0f} us")
        print(f"  resident-wave average {total / span:.0f} of {args.grid} ({100 * total / span / args.grid:.1f} %); last game popped at "
              f"{last_start:.0f} us; drain {drain:.0f} us ({100 * drain / span:.1f} % of the launch)")
    print(f"resident average {100 * min(fr):.1f} .. {100 * max(fr):.1f} % of the grid, idle share {100 * (1 - max(fr)):.1f} .. "
          f"{100 * (1 - min(fr)):.1f} %; drain {100 * min(dr):.1f} .. {100 * max(dr):.1f} % of the launch")
    return 0


if __name__ == "__main__":
    sys.exit(main())
