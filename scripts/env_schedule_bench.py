#!/usr/bin/env python3
"""Throughput of VecEnv.step by the source of the episode decks: fixed decks, the C5 pool, a deck schedule.

Workload: --slots slots (default 65 536) against the scripted bot, episodes truncated at --max-steps committed steps so
that a steady share of the slots starts an episode in every step, a random policy sampled on the device from the legal
mask.  Four envs, each a handle of its own, on the same seeds:
    fixed     the IRONCLAD / SWARM archetypes for every episode
    pool      every episode draws from the cards of the standard record (monsoon_draw_decks' code in k_env_reseed)
    explore   every episode draws from a deck schedule, explore phase, 6 archetype cards kept (k_env_reseed_schedule)
    balance   the same schedule in its balance phase at ratio 0.7
The schedule is made by hand from the two factions' pools without ua20 / b005, so that all four run on the standard
record; pool and schedule both draw only for the slots whose episode ended, which makes pool the yardstick.

Method: --warmup steps per env, then --rounds rounds; a round times one window of --window-steps steps of every env in
turn (alternating, so that drift hits all alike), ended by a synchronise.  Per mode the median window is reported, with
all windows, and the median HIP-event time of the reseed kernel (monsoon_env_reseed_time) over steps sampled in a
separate pass after the windows, with the share of slots that started an episode in the sampled steps.  One JSON line per
mode.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from monsoon_amd.cards import CARD_INDEX, DECKS, UNSUPPORTED, deck_indices, supported_pool  # noqa: E402
from monsoon_amd.decks import IRONCLAD, SWARM, TAG_ENV, available_cards  # noqa: E402
from monsoon_amd.vec_env import VecEnv  # noqa: E402

MODES = ("fixed", "pool", "explore", "balance")


def schedule(phase):
    pools = [[CARD_INDEX[c] for c in available_cards(f) if c not in UNSUPPORTED] for f in (IRONCLAD, SWARM)]
    pool = np.zeros((2, 128), dtype=np.uint8)
    for side, p in enumerate(pools):
        pool[side, :len(p)] = p
    return {"seed": 2024, "generation": 45, "tag": TAG_ENV, "phase": phase, "n_preserve": 6, "balance_archetype_ratio": 0.7,
            "archetype": np.stack([deck_indices(DECKS["IRONCLAD"]), deck_indices(DECKS["SWARM"])]),
            "pool_n": np.array([len(p) for p in pools], dtype=np.int32), "pool": pool}


def sample(torch, legal, gen):
    u = torch.rand(legal.shape, device=legal.device, generator=gen)
    u.masked_fill_(~legal, -1.0)
    return u.argmax(dim=1).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--slots", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-steps", type=int, default=200)
    ap.add_argument("--max-steps", type=int, default=40)
    ap.add_argument("--timed-steps", type=int, default=40)
    ap.add_argument("--only", default="", help="comma list of modes")
    args = ap.parse_args()
    import torch
    n = args.slots
    seed0 = np.arange(n, dtype=np.uint32) + 1000
    factions = np.tile(np.array([IRONCLAD, SWARM], dtype=np.uint8), (n, 1))
    pair = np.stack([deck_indices("IRONCLAD"), deck_indices("SWARM")])
    pool = np.array(sorted(CARD_INDEX[c] for c in supported_pool()), dtype=np.uint8)
    how = {"fixed": dict(decks=pair), "pool": dict(pool=pool), "explore": dict(deck_schedule=schedule(1)), "balance": dict(deck_schedule=schedule(2))}
    modes = [m for m in MODES if not args.only or m in args.only.split(",")]
    envs, views, gens = {}, {}, {}
    for m in modes:
        envs[m] = VecEnv(n)
        views[m] = envs[m].reset(seed0, factions=factions, opponent="expert", max_steps=args.max_steps, **how[m])
        gens[m] = torch.Generator(device="cuda")
        gens[m].manual_seed(7)

    def run(m, steps):
        for _ in range(steps):
            views[m] = envs[m].step(sample(torch, views[m]["legal"], gens[m]))

    def agent_steps(m):
        return int(envs[m].engine.debug_counters()[6])

    for m in modes:
        run(m, args.warmup)
    torch.cuda.synchronize()
    rates = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes:
            a0 = agent_steps(m)
            t0 = time.perf_counter()
            run(m, args.window_steps)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            rates[m].append((agent_steps(m) - a0) / dt)
    for m in modes:
        eng = envs[m].engine
        eng.env_reseed_time(True)
        ms, started = [], 0
        for _ in range(args.timed_steps):
            run(m, 1)
            ms.append(eng.env_reseed_time(True))
            started += int(views[m]["done"].sum().item())
        eng.env_reseed_time(False)
        r = sorted(rates[m])
        row = dict(mode=m, slots=n, max_steps=args.max_steps, agent_steps_per_s=round(r[len(r) // 2]), windows_agent_steps_per_s=[round(x) for x in rates[m]],
                   window_steps=args.window_steps, reseed_kernel_ms_per_step=round(float(np.median(ms)), 4),
                   reseed_kernel_ms_min_max=[round(min(ms), 4), round(max(ms), 4)],
                   episodes_started_per_step=round(started / args.timed_steps, 1), schedule_overruns=int(eng.debug_counters()[17]))
        print(json.dumps(row), flush=True)
    for m in modes:
        envs[m].close()


if __name__ == "__main__":
    main()
