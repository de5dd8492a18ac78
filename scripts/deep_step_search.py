#!/usr/bin/env python3
"""Search for steps that drive the rules core's work stack deep (CPU, test infrastructure).

Plays heuristic (W0) and random-policy games on the counting host builds of the product's rules core with the device's
21-word resident stack (oracle/Makefile libproduct_host_count{,_ext}.so) and records, for every committed step and every
look-ahead, the step's own recursion depth (H_DEPTH), work-stack words and pending evictions (Wk::seg).  Sources:
  * C5 games 0..N-1 (tests/c5_games.py) plus any named with --c5 (2683, 2427 and 29409 by default);
  * --guard-scan N: the C5 games below N that end with code 18, found with the multi-threaded oracle rollout;
  * --chain N: games on decks drawn from the cards DESIGN.md §2 names for F_EACH / F_AFTER (every second one with b005 or
    ua20 added, which puts it on the extended record): heuristic, random policy, and heuristic against the scripted bot.
  * --scenarios: every recorded call of the reference's own unit tests (tests/golden/scenarios.json.gz, the 16-unit u401
    chain reaction of its BaseTestCase among them) on the counting builds: measured only (its triggers pop one after the
    other, so the chain is long but not deep: 3 nested calls, 23 words at the most).
The first half of the C5 games is also played with a random policy and against the bot (the bot plays SECOND and draws
from the game's stream before each of its steps: a replay calls expert_action wherever bot_side is to play).
It prints the distribution and writes the chosen POSITIONS -- (tier, seed, decks, factions, bot side, action prefix, action) -- as
JSON; oracle/pyref/gen_deep_steps.py replays them on the Python reference and writes tests/golden/deep_steps.json.gz.

Classes (tests/test_deep_steps_cpu.py asserts them on the fixture):
  A  two or more evictions pending on a step that completes;        B  steps the recursion guard ends (code 18);
  C  the deepest chain that completes;                              D  decisions in which several candidates evict.

    make -C oracle && python scripts/deep_step_search.py --games 3000 --guard-scan 524288 --chain 4000 --out positions.json
"""
import argparse
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)
import oracle_lib  # noqa: E402
from c5_games import c5_games  # noqa: E402
from monsoon_amd.cards import CARD_IDS  # noqa: E402

W0 = np.random.RandomState(2024).uniform(0, 1, 10)
CHAIN = "u401 b004 u405 s003 ue12 ue21 b203 u101 ud02 s013 s203 s302 u018 ue01 u017 u076 u302 b305".split()
EXT_CARDS = {CARD_IDS.index("ua20"), CARD_IDS.index("b005")}


def is_ext(d0, d1):
    return bool(EXT_CARDS & (set(int(c) for c in d0) | set(int(c) for c in d1)))


def chain_game(k):
    """Game k of the chain family: seed 70000 + k, both decks 12 of the 18 chaining cards (odd k: one of them replaced by
    b005 or ua20), drawn by RandomState(k ^ 0x51ED270B)."""
    rs = np.random.RandomState(k ^ 0x51ED270B)
    decks = []
    for _ in range(2):
        d = [CARD_IDS.index(c) for c in rs.choice(CHAIN, 12, replace=False)]
        if k & 1:
            d[int(rs.randint(12))] = CARD_IDS.index(("b005", "ua20")[int(rs.randint(2))])
        decks.append(d)
    return 70000 + k, decks[0], decks[1]


def play(spec):
    """One game on the counting build.  Returns every step of interest and the game's summary."""
    label, seed, d0, d1, policy, max_turns = spec
    ext = is_ext(d0, d1)
    o = oracle_lib.Oracle(1, extended=ext, core="product_count")
    if o.reset(0, seed, d0, d1) != 0:
        return None
    pol = np.random.RandomState(seed + 1000)
    actions, events = [], []
    deepest = (0, 0, 0)
    bot_side = 1 if policy == "b" else -1   # "b": the reference's scripted bot plays SECOND (rollouts against the expert)
    for t in range(max_turns):
        if o.have_winner(0):
            break
        if o.to_play(0) == bot_side:
            # the bot draws from the game's stream before it steps: only the committed step itself is this position's step
            a, f = o.expert_action(0)
            if f:
                break
            (f, _, _), (depth, words, seg, at_guard) = o.step_counts(0, a)
            if seg >= 2 or f in (18, 29):
                events.append(dict(step=t, action=a, committed=True, fault=f, depth=depth, words=words, seg=seg, at_guard=at_guard, evicting=0))
            deepest = max(deepest, (words, depth, seg))
            actions.append(a)
            if f:
                break
            continue
        cnt = o.lookahead_counts(0)
        legal = np.nonzero(cnt[:, 0] != 255)[0]
        a = int(legal[pol.randint(len(legal))]) if policy == "r" else int(o.decide(0, W0)[0])
        evicting = int((cnt[legal, 3] >= 1).sum())
        for c in legal:
            f, depth, words, seg, at_guard = (int(v) for v in cnt[c])
            deepest = max(deepest, (words, depth, seg))
            if seg >= 2 or f in (18, 29) or depth >= 12 or (evicting >= 3 and seg >= 1):
                events.append(dict(step=t, action=int(c), committed=bool(c == a), fault=f, depth=depth, words=words, seg=seg,
                                   at_guard=at_guard, evicting=evicting))
        f = o.step(0, a)[0]
        actions.append(a)
        if f:
            break
    return dict(label=label, tier=int(ext), seed=int(seed), decks=[[int(c) for c in d0], [int(c) for c in d1]], policy=policy,
                bot_side=bot_side, actions=actions, events=events, words=deepest[0], depth=max([e["depth"] for e in events], default=0), deepest=deepest)


def scenario_depths():
    """(depth, words, evictions pending, fault, test, call number, op) of every recorded scenario call, deepest first."""
    import scenario_lib as S
    ext_cards = sorted(EXT_CARDS)
    orcs = {e: oracle_lib.Oracle(1, extended=e, core="product_count") for e in (False, True)}
    rows = []
    for case in S.load():
        for k, rec in enumerate(case["records"]):
            orc = orcs[S.needs_extended(rec, ext_cards)]
            c = orc.L.orc_frame_counts()
            st = rec["before"]
            if orc.scn_build(0, st["seed"], st["stream_pos"], S.encode_state(st)) != 0:
                continue
            c[12] = c[13] = c[14] = c[15] = 0
            f, _ = orc.scn_op(0, S.encode_op(rec))
            rows.append((int(c[13]), int(c[15]), int(c[14]), f, case["test"], k, rec["op"]))
    return sorted(rows, reverse=True)


def position(g, e, cls):
    return dict(cls=cls, source=g["label"], policy=g["policy"], tier=g["tier"], seed=g["seed"], decks=g["decks"], factions=[0, 0],
                bot_side=g["bot_side"], prefix=g["actions"][:e["step"]], action=e["action"], committed=e["committed"],
                count=dict(fault=e["fault"], depth=e["depth"], words=e["words"], seg=e["seg"], at_guard=e["at_guard"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=3000)
    ap.add_argument("--c5", type=int, nargs="*", default=[2683, 2427, 29409])
    ap.add_argument("--guard-scan", type=int, default=0)
    ap.add_argument("--chain", type=int, default=0)
    ap.add_argument("--scenarios", action="store_true")
    ap.add_argument("--max-turns", type=int, default=200)
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--out", default="deep_positions.json")
    args = ap.parse_args()

    if args.scenarios:
        rows = scenario_depths()
        print(f"scenarios: {len(rows)} recorded calls, deepest (depth, words, seg, fault, test, call, op): {rows[:4]}")
    c5 = sorted(set(range(args.games)) | set(args.c5))
    if args.guard_scan:
        from oracle_rollout import oracle_rollout_fn_mt
        m, pairs = c5_games(range(args.guard_scan))
        _, _, _, faults = oracle_rollout_fn_mt(W0[None, :], m, pairs, args.max_turns, threads=args.jobs, want_faults=True)
        guard = np.nonzero(faults == 18)[0].tolist()
        print(f"guard scan: C5 games 0..{args.guard_scan - 1}: code 18 in {guard}; other codes left "
              f"{dict(zip(*np.unique(faults[faults >= 16], return_counts=True)))}")
        c5 = sorted(set(c5) | set(guard))
    m, pairs = c5_games(c5)
    specs = [(f"c5:{k}", int(m["seed"][j]), pairs[j, 0], pairs[j, 1], "h", args.max_turns) for j, k in enumerate(c5)]
    specs += [(f"c5r:{k}", int(m["seed"][j]), pairs[j, 0], pairs[j, 1], "r", args.max_turns) for j, k in enumerate(c5) if k < args.games // 2]
    specs += [(f"c5b:{k}", int(m["seed"][j]), pairs[j, 0], pairs[j, 1], "b", args.max_turns) for j, k in enumerate(c5) if k < args.games // 2]
    for k in range(args.chain):
        s, d0, d1 = chain_game(k)
        specs.append((f"chain:{k}", s, d0, d1, "hhrb"[k // 2 % 4], args.max_turns))
    with ProcessPoolExecutor(args.jobs) as ex:
        games = [g for g in ex.map(play, specs, chunksize=8) if g is not None]

    n_steps = sum(len(g["actions"]) for g in games)
    print(f"search: {len(games)} games ({len(c5)} C5 heuristic; {args.chain} on chain decks; by policy "
          f"{ {p: sum(g['policy'] == p for g in games) for p in 'hrb'} }), {n_steps} committed steps")
    for fam in ("c5:", "c5r:", "c5b:", "chain:"):
        for tier in (0, 1):
            w = np.array([g["words"] for g in games if g["label"].startswith(fam) and g["tier"] == tier])
            if len(w):
                top = sorted(w)[-3:][::-1]
                print(f"  {fam:7s} tier {tier}: {len(w):5d} games, deepest words per game: median {int(np.median(w))} p90 "
                      f"{int(np.percentile(w, 90))} p99 {int(np.percentile(w, 99))} max {top}")
    ev = [(g, e) for g in games for e in g["events"]]
    print("  steps with seg >= 2:", sum(e["seg"] >= 2 for _, e in ev), " seg >= 3:", sum(e["seg"] >= 3 for _, e in ev),
          " code 18:", sum(e["fault"] == 18 for _, e in ev), " code 29:", sum(e["fault"] == 29 for _, e in ev))
    finite = [(g, e) for g, e in ev if e["fault"] == 0]
    if finite:
        gd, ed = max(finite, key=lambda x: (x[1]["depth"], x[1]["words"]))
        print(f"  deepest finite chain: depth {ed['depth']} words {ed['words']} seg {ed['seg']} ({gd['label']} step {ed['step']} action {ed['action']})")
    guard = [(g, e) for g, e in ev if e["fault"] == 18]
    if guard:
        print("  words where the guard tripped:", sorted(e["at_guard"] for _, e in guard)[-5:], "depth histogram of finite steps >= 12:",
              dict(zip(*np.unique([e["depth"] for _, e in finite if e["depth"] >= 12], return_counts=True))))

    # ---- choose the positions: short prefixes first, one per (game, step) ----
    out, seen = [], set()

    def take(cands, cls, n, key):
        got = 0
        for g, e in sorted(cands, key=key):
            if got >= n:
                break
            if (g["label"], e["step"], e["action"]) in seen:
                continue
            if sum(1 for p in out if p["source"] == g["label"]) >= 3:   # spread over games
                continue
            seen.add((g["label"], e["step"], e["action"]))
            out.append(position(g, e, cls))
            got += 1
        return got

    if finite:
        take([(gd, ed)], "C", 1, key=lambda x: 0)
    for tier in (0, 1):
        a = [(g, e) for g, e in finite if e["seg"] >= 2 and g["tier"] == tier and g["bot_side"] < 0]
        take(a, "A", 4, key=lambda x: (-x[1]["seg"], -x[1]["words"]))                                    # the deepest of the tier,
        take([x for x in a if 4 <= x[1]["seg"] <= 6], "A", 3, key=lambda x: (x[1]["step"], -x[1]["words"]))   # the middle,
        take(a, "A", 3, key=lambda x: (x[1]["step"], -x[1]["words"]))                                      # the ones reached soonest
        take([(g, e) for g, e in finite if e["seg"] >= 2 and g["tier"] == tier and g["bot_side"] >= 0], "A", 3,
             key=lambda x: (-min(x[1]["seg"], 4), x[1]["step"]))                                           # and games against the bot
    for tier in (0, 1):
        take([(g, e) for g, e in guard if g["tier"] == tier], "B", 4, key=lambda x: (x[0]["bot_side"] < 0, x[1]["step"]))
    for tier in (0, 1):   # one position per decision: its deepest candidate
        best = {}
        for g, e in finite:
            if e["evicting"] >= 3 and e["seg"] >= 1 and g["tier"] == tier:
                k = (g["label"], e["step"])
                if k not in best or e["words"] > best[k][1]["words"]:
                    best[k] = (g, e)
        take(best.values(), "D", 3, key=lambda x: (-x[1]["evicting"], x[1]["step"]))
    out = out[:64]
    print("positions:", {c: sum(p["cls"] == c for p in out) for c in "ABCD"}, "longest prefix", max([len(p["prefix"]) for p in out], default=0))
    with open(args.out, "w") as f:
        json.dump(dict(search=dict(games=len(games), committed_steps=n_steps, c5=len(c5), chain=args.chain, guard_scan=args.guard_scan),
                       positions=out), f)


if __name__ == "__main__":
    main()
