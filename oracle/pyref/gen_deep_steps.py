#!/usr/bin/env python3
"""Record the Python reference on the deep-step positions found by scripts/deep_step_search.py.

TEST INFRASTRUCTURE (build container only; needs the reference tree, see refenv.py).  Writes data only:
tests/golden/deep_steps.json.gz.  Every position -- (tier, seed, decks, factions, bot side, action prefix, action) -- is replayed on
the imported reference through harness.py: the prefix step by step (it must not raise), then the deep action.  Recorded
per position: the position itself and the search's figures for the step (recursion depth, work-stack words, pending
evictions on the counting host build), the reference's canonical record after the step (harness.canon, hex), reward and
done, whether the step raised and the exception's class name, the legal mask after the step, and -- where it raised
RecursionError -- the reference's real nesting at that point: the frames of Unit.move and of the wrapped
activate_ability (card.py:48-62) on the traceback, the two calls the engine's depth counter counts.

Usage: PYTHONHASHSEED=0 python oracle/pyref/gen_deep_steps.py positions.json
"""
import contextlib
import gzip
import io
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import harness as H  # noqa: E402

OUT = os.path.join(H.REPO, "tests", "golden", "deep_steps.json.gz")


def nesting(tb):
    n = dict(move=0, ability=0, frames=0)
    while tb is not None:
        name = tb.tb_frame.f_code.co_name
        n["frames"] += 1
        n["move"] += name == "move"
        n["ability"] += name == "wrapped"
        tb = tb.tb_next
    return n


def record(p):
    g = H.make_game(p["seed"], [H.CARD_IDS[c] for c in p["decks"][0]], [H.CARD_IDS[c] for c in p["decks"][1]], *p["factions"])
    with contextlib.redirect_stdout(io.StringIO()):
        bot = p["bot_side"]   # -1, or the side the reference's scripted bot plays: it draws from the game's stream first

        def bot_draws(a):
            if bot >= 0 and (0 if g.player == 1 else 1) == bot:
                assert int(g.expert_action()) == a, (p["source"], a)
        for a in p["prefix"]:
            assert a in g.legal_actions(), (p["source"], a)
            bot_draws(a)
            g.step(a)
        before = H.fnv1a64(H.canon(g))
        bot_draws(p["action"])
        assert p["action"] in g.legal_actions(), (p["source"], p["action"])
        out = dict(p, hash_before=before, raised=None, nesting=None, canon=None, reward=None, done=None, legal=None)
        try:
            _, reward, done = g.step(p["action"])
        except Exception as e:  # noqa: BLE001  the agent layer swallows these (evo/heuristic_agent.py:48-51)
            out["raised"] = type(e).__name__
            if isinstance(e, RecursionError):
                out["nesting"] = nesting(e.__traceback__)
            return out
    out.update(canon=H.canon(g).hex(), reward=int(reward), done=int(bool(done)), legal=H.legal_mask(g.legal_actions()))
    return out


def main():
    with open(sys.argv[1]) as f:
        src = json.load(f)
    rows = [record(p) for p in src["positions"]]
    for r in rows:
        print(r["cls"], r["source"], "tier", r["tier"], "prefix", len(r["prefix"]), "action", r["action"], r["count"],
              "raised", r["raised"], r["nesting"] or "")
    data = json.dumps(dict(search=src["search"], positions=rows), separators=(",", ":")).encode()
    with open(OUT, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as z:
        z.write(data)
    print(OUT, len(rows), "positions", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
