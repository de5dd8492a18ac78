#!/usr/bin/env python3
"""How often the per-pass glue of the hot kernel's decision loop runs: the bench's own games replayed on the CPU.

    python scripts/pass_stats.py [--games 200] [--decisions 120] > profiles/pass_stats.md

N12M on both sides, W0 on both sides, seeds 0 .. games-1 (bench.py's C2), every decision taken by the recursive oracle.
Prints the histogram of legal actions per decision, the passes per decision and the fill of the passes for every lane
count U of variants.def, how full the last pass of a decision is, how many candidates share their score bit for bit with
another candidate of the same decision, and the kinds of the candidates.  CPU only, no GPU involved."""
import argparse
import os
import sys
import time
from collections import Counter

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import oracle_lib  # noqa: E402
from monsoon_amd.cards import deck_indices  # noqa: E402

W0 = np.random.RandomState(2024).uniform(0, 1, 10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=200)
    ap.add_argument("--decisions", type=int, default=120)
    a = ap.parse_args()
    deck = deck_indices("N12M")
    orc = oracle_lib.Oracle(1)
    hist, kinds = Counter(), Counter()
    cands = tied = decisions = tie_dec = 0
    t0 = time.time()
    for seed in range(a.games):
        orc.reset(0, seed, deck, deck)
        for _ in range(a.decisions):
            if orc.have_winner(0):
                break
            act, sc, _ = orc.decide(0, W0)
            legal = np.nonzero(~np.isnan(sc))[0]
            hist[len(legal)] += 1
            decisions += 1
            cands += len(legal)
            _, inv, cnt = np.unique(sc[legal].view(np.uint64), return_inverse=True, return_counts=True)
            tied += int((cnt[inv] > 1).sum())
            tie_dec += int((sc[legal] == sc[act]).sum() > 1)
            for x in legal:
                kinds["PLACE" if x < 64 else "USE" if x < 148 else "REPLACE" if x < 152 else "other (152..155)"] += 1
            if orc.step(0, act)[0]:
                break
    dt = time.time() - t0
    n = np.array(sorted(hist.elements()))
    print("# Passes of the decision loop in the bench's games (scripts/pass_stats.py)\n")
    print(f"{a.games} N12M self-play games, W0 both sides, seeds 0..{a.games - 1}, up to {a.decisions} decisions each, replayed by the "
          f"recursive oracle on the CPU: {decisions} decisions, {cands} candidates, {dt:.1f} s.\n")
    print(f"- legal actions per decision: mean {n.mean():.1f}, min {n.min()}, max {n.max()}; values seen: "
          + ", ".join(f"{lo}..{hi}" if lo != hi else str(lo) for lo, hi in _runs(sorted(hist))))
    print(f"- decisions with a single legal action: {100 * hist[1] / decisions:.1f} %")
    print(f"- candidates whose score equals another candidate's of the same decision bit for bit: {100 * tied / cands:.1f} %; "
          f"decisions whose maximal score is shared: {100 * tie_dec / decisions:.1f} %")
    print("- candidates by kind: " + ", ".join(f"{k} {100 * v / cands:.1f} %" for k, v in kinds.most_common()) + "\n")
    print("| U | passes per decision | ideal n/U | column fill | last pass holds 1 | last pass holds <= 2 |")
    print("|---|---|---|---|---|---|")
    for u in (4, 8, 16, 32, 64):
        passes = (n + u - 1) // u
        last = n - (passes - 1) * u
        print(f"| {u} | {passes.mean():.3f} | {(n / u).mean():.2f} | {n.sum() / (passes.sum() * u):.2f} | "
              f"{100 * (last == 1).mean():.0f} % | {100 * (last <= 2).mean():.0f} % |")
    print("\n| legal actions | decisions |\n|---|---|")
    for k in sorted(hist):
        print(f"| {k} | {hist[k]} |")


def _runs(v):
    out, lo = [], v[0]
    for x, y in zip(v, v[1:] + [None]):
        if y != x + 1:
            out.append((lo, x))
            lo = y
    return out


if __name__ == "__main__":
    main()
