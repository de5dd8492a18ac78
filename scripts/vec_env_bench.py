#!/usr/bin/env python3
"""Throughput of the device-resident vector env (monsoon_amd/vec_env.py) against the host-API loop on the same seeds.

Workload: --slots games (default 65 536), N12M decks or a per-episode pool (every card of the standard record but
up01/up02/up03), opponent none, the scripted bot or the heuristic agent (8 weight vectors, slot i playing row i % 8), a
random policy sampled on the device from the legal mask with torch ops.  Agent env-steps/s and opponent steps/s are
reported separately (the env's own counters, monsoon_debug_counters words 6 / 7); for the heuristic opponent, whose steps
are its decisions, also its look-ahead transitions/s (word 16).  The host loop is not run for the heuristic opponent.  The host loop is what the C ABI offered before the env: monsoon_legal_mask + monsoon_step +
monsoon_observe_dev every step (the policy samples on the device from the uploaded mask), the bot's turn as
monsoon_status + monsoon_expert_action + monsoon_step rounds, and the whole batch re-reset once every game is done.

Method: --warmup steps, then --windows timed windows of at least --window-s seconds, each ended by a synchronise;
the median window is reported.  Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this
script (e.g. with --windows 1 --window-s 0.5).  One JSON line per configuration and path.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from monsoon_amd.cards import CARD_INDEX, deck_indices, supported_pool  # noqa: E402
from monsoon_amd.engine import BatchEngine  # noqa: E402
from monsoon_amd.vec_env import VecEnv  # noqa: E402


OPPONENTS = ("none", "expert", "heuristic")


def counters(eng):
    c = np.zeros(192, dtype=np.uint64)
    eng._ck(eng.lib.monsoon_debug_counters(eng.h, c.ctypes.data_as(ctypes.c_void_p)), "monsoon_debug_counters")
    return int(c[6]), int(c[7]), int(c[16])


def sample(torch, legal, gen):
    u = torch.rand(legal.shape, device=legal.device, generator=gen)
    u.masked_fill_(~legal, -1.0)
    return u.argmax(dim=1).to(torch.uint8)


def windows(step_fn, count_fn, sync, args, chunk):
    """Median over timed windows of (agent steps/s, bot steps/s, steps per window, window seconds, look-ahead
    transitions/s)."""
    for _ in range(args.warmup):
        step_fn()
    sync()
    res = []
    for _ in range(args.windows):
        a0, b0, l0 = count_fn()
        t0 = time.perf_counter()
        calls = 0
        while True:
            step_fn()
            calls += 1
            if calls % chunk == 0:
                sync()
                if time.perf_counter() - t0 >= args.window_s:
                    break
        dt = time.perf_counter() - t0
        a1, b1, l1 = count_fn()
        res.append(((a1 - a0) / dt, (b1 - b0) / dt, calls, dt, (l1 - l0) / dt))
    res.sort(key=lambda r: r[0])
    return res[len(res) // 2], res


def bench_env(torch, args, seed0, decks, pool, opponent):
    env = VecEnv(args.slots)
    kw = {}
    if opponent == 2:
        kw = dict(opponent_weights=np.random.RandomState(42).uniform(0, 1, (8, 10)), opponent_rows=np.arange(args.slots) % 8)
    views = env.reset(seed0, None if pool is not None else decks, opponent=OPPONENTS[opponent], pool=pool,
                      max_steps=args.max_steps, **kw)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    state = {"v": views}

    def step():
        state["v"] = env.step(sample(torch, state["v"]["legal"], gen))

    med, all_ = windows(step, lambda: counters(env.engine), torch.cuda.synchronize, args, 8)
    eps = int(views["episode"].sum().item())
    env.close()
    return med, all_, eps


def bench_host(torch, args, seed0, decks, pool, opponent):
    n = args.slots
    eng = BatchEngine(n)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    obs = torch.empty((n, 27, 5, 4), dtype=torch.int32, device="cuda")
    raises = torch.empty((n,), dtype=torch.uint8, device="cuda")
    st = {"episode": 0, "agent": 0, "bot": 0, "live": None}

    def reset():
        k = st["episode"]
        seeds = (seed0.astype(np.int64) + k * n).astype(np.uint32)
        d = decks if pool is None else eng.draw_decks(seeds ^ np.uint32(0x9E3779B9), pool)
        eng.reset(seeds, d)
        st["episode"] += 1
        st["live"] = np.ones(n, dtype=bool)
        if opponent:
            bot_turn()

    def bot_turn():
        for _ in range(64):
            tp = eng.status()[:, 0]
            mine = st["live"] & (tp == 1)
            if not mine.any():
                return
            act, _ = eng.expert_action()
            act = np.where(mine, act, 255).astype(np.uint8)
            _, done, fault = eng.step(act)
            st["bot"] += int(mine.sum())
            st["live"] &= ~((done | fault).astype(bool))

    def step():
        if st["live"] is None or not st["live"].any():
            reset()
        masks = eng.legal_mask()
        bits = np.unpackbits(masks.view(np.uint8), axis=1, bitorder="little")[:, :156]
        a = sample(torch, torch.from_numpy(bits).cuda().bool(), gen).cpu().numpy()
        a = np.where(st["live"], a, 255).astype(np.uint8)
        _, done, fault = eng.step(a)
        st["agent"] += int(st["live"].sum())
        st["live"] &= ~((done | fault).astype(bool))
        if opponent:
            bot_turn()
        eng._ck(eng.lib.monsoon_observe_dev(eng.h, ctypes.c_void_p(obs.data_ptr()), ctypes.c_void_p(raises.data_ptr())), "observe_dev")

    med, all_ = windows(step, lambda: (st["agent"], st["bot"], 0), eng.sync, args, 1)
    eng.close()
    return med, all_, st["episode"]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--slots", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=1.0)
    ap.add_argument("--max-steps", type=int, default=0)
    ap.add_argument("--only", default="", help="comma list of config names to run (e.g. N12M/none,pool/expert)")
    ap.add_argument("--no-host", action="store_true", help="skip the host-API loop")
    args = ap.parse_args()
    import torch
    n = args.slots
    seed0 = np.arange(n, dtype=np.uint32) + 1000
    deck = np.stack([deck_indices("N12M"), deck_indices("N12M")])
    decks = np.broadcast_to(deck, (n, 2, 12)).copy()
    pool = np.array(sorted(CARD_INDEX[c] for c in supported_pool()), dtype=np.uint8)
    for dname, p in (("N12M", None), ("pool", pool)):
        for opponent in (0, 1, 2):
            name = f"{dname}/{OPPONENTS[opponent]}"
            if args.only and name not in args.only.split(","):
                continue
            paths = [("env", bench_env)] + ([] if args.no_host or opponent == 2 else [("host_loop", bench_host)])
            for path, fn in paths:
                med, all_, eps = fn(torch, args, seed0, decks, p, opponent)
                row = dict(config=name, path=path, slots=n, agent_steps_per_s=round(med[0]), bot_steps_per_s=round(med[1]),
                           calls_per_window=med[2], window_s=round(med[3], 3),
                           windows_agent_steps_per_s=[round(r[0]) for r in all_], episodes=eps)
                if opponent == 2:
                    row.update(opponent_decisions_per_s=round(med[1]), lookahead_transitions_per_s=round(med[4]))
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
