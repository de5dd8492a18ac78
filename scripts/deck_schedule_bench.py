#!/usr/bin/env python3
"""Cost of a deck schedule's per-game decks: the sequential host loop, the per-game host specification and the device draw
(monsoon_draw_schedule, k_draw_schedule).

Workload: one explore and one balance generation of --games games (default 524 288, a C5-sized generation) of a schedule
over the IRONCLAD and SWARM archetypes (exploit 30, explore 30 generations, the defaults; generation 45 is mid-explore,
generation 70 balance), game seeds from ring_schedule.

Method (one JSON line per generation):
  * host_sequential_us_per_game: FitnessEvaluator._decks_for's loop of the sequential mode (get_deck_configuration +
    deck_indices per game), timed on --host-games games (default 16 384).
  * host_per_game_us_per_game: the same loop over DeckEvolutionConfig.game_decks, the specification of the per-game mode
    (it also seeds a random.Random per game), likewise.
  * device_call_ms: BatchEngine.draw_schedule end to end, host buffers in and out, median (min - max) of --reps calls after
    --warmup warm-ups, host clock (the call returns after its stream has finished).
  * kernel_ms: k_draw_schedule alone inside those calls, by HIP events (monsoon_draw_schedule_time), median likewise.
  * the first --check games of the device draw are compared with game_decks."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from monsoon_amd.cards import DECKS, deck_indices  # noqa: E402
from monsoon_amd.decks import DeckEvolutionConfig  # noqa: E402
from monsoon_amd.engine import BatchEngine  # noqa: E402
from monsoon_amd.fitness import ring_schedule  # noqa: E402


def host_loop(draw, n):
    pairs = np.zeros((n, 2, 12), dtype=np.uint8)
    t0 = time.perf_counter()
    for k in range(n):
        d1, d2 = draw(k)
        pairs[k, 0], pairs[k, 1] = deck_indices(d1), deck_indices(d2)
    return (time.perf_counter() - t0) / n * 1e6, pairs


def spread(v):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], 4), min=round(v[0], 4), max=round(v[-1], 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--games", type=int, default=524288)
    ap.add_argument("--host-games", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", type=int, default=2000)
    ap.add_argument("--label", default="", help="free text copied into every line")
    args = ap.parse_args()
    eng = BatchEngine(64)
    per_individual = 128
    seeds = ring_schedule((args.games + per_individual - 1) // per_individual, per_individual, 0)["seed"][:args.games].copy()
    for phase, generation in (("explore", 45), ("balance", 70)):
        seq = DeckEvolutionConfig(DECKS["IRONCLAD"], DECKS["SWARM"], seed=5)
        dc = DeckEvolutionConfig(DECKS["IRONCLAD"], DECKS["SWARM"], seed=5, per_game=True)
        params = dc.schedule_params(generation)
        nh = min(args.host_games, args.games)
        seq_us, _ = host_loop(lambda k: seq.get_deck_configuration(generation), nh)
        spec_us, want = host_loop(lambda k: dc.game_decks(generation, seeds[k]), nh)
        call_ms, kernel_ms = [], []
        for _ in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            got = eng.draw_schedule(params, seeds)
            call_ms.append((time.perf_counter() - t0) * 1e3)
            kernel_ms.append(eng.draw_schedule_time())
        nc = min(args.check, nh)
        assert np.array_equal(got[:nc], want[:nc]), "the device draw differs from game_decks"
        call, kern = spread(call_ms[args.warmup:]), spread(kernel_ms[args.warmup:])
        print(json.dumps(dict(what="deck_schedule_draw", phase=phase, generation=generation, games=args.games, host_games=nh,
                              n_preserve=params["n_preserve"], label=args.label,
                              host_sequential_us_per_game=round(seq_us, 2), host_per_game_us_per_game=round(spec_us, 2),
                              host_sequential_s_for_games=round(seq_us * args.games * 1e-6, 2),
                              device_call_ms=call, kernel_ms=kern, first_call_ms=round(call_ms[0], 3),
                              kernel_us_per_game=round(kern["median"] * 1e3 / args.games, 4),
                              host_sequential_over_device_call=round(seq_us * args.games * 1e-3 / call["median"], 1))), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
