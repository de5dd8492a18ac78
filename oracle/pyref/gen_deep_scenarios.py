#!/usr/bin/env python3
"""The deep-step positions as scenario records: boards for monsoon_debug_build / monsoon_debug_op.

TEST INFRASTRUCTURE (build container only; needs the reference tree, see refenv.py).  Writes data only:
tests/golden/deep_scenarios.json.gz, in the format of scenarios.json.gz (gen_scenarios.py, whose recorder this uses).
Every position of tests/golden/deep_steps.json.gz is reached on the reference (seed, decks, action prefix), the engine
classes are instrumented as for the reference's unit tests, and the deep action is stepped: each call Stormbound.step
makes into the engine (Player.play, Board.to_next_turn ...) becomes one record -- complete state before, the call,
canonical state after, the order in which abilities ran, whether it raised.  A replayer (tests/scenario_lib.py) builds
the board and makes the one call: the work stack goes as deep as it did in the game, without the game.

CONSTRUCTED boards follow: play found no chain between depth 30 and the guard's 40 that completes, so five of the boards
above are changed by hand as the reference's unit tests change theirs -- one token unit spawned on a free tile, the
shared stream re-seeded -- until the endless ue21 / u320 chain of the guard positions ends by itself after 30 to 40
nested calls (the variants were searched on the counting host build; the reference decides what they do).  Their
`count` is what the counting build measures on the recorded call.

Usage: PYTHONHASHSEED=0 python oracle/pyref/gen_deep_scenarios.py
"""
import contextlib
import gzip
import io
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import harness as H  # noqa: E402
import gen_scenarios as G  # noqa: E402

# (position the board comes from, tile of the spawned token, its owner, its strength, its unit type, the seed)
CONSTRUCTED = [("B:c5:355025:30:155", 6, 1, 1, 84), ("B:c5:280013:89:42", 14, 1, 1, 86), ("B:c5:474669:49:41", 4, 1, 30, 31),
               ("C:c5:45162:188:37", 10, 0, 30, 208), ("C:c5:45162:188:37", 13, 1, 1, 327)]
TOKEN_TYPE = 11   # UnitType.DRAGON: a token of one type, no ability

SRC = os.path.join(H.REPO, "tests", "golden", "deep_steps.json.gz")
OUT = os.path.join(H.REPO, "tests", "golden", "deep_scenarios.json.gz")


def at_position(p):
    """The reference's game at position p, the bot's draw for the deep action made."""
    g = H.make_game(p["seed"], [H.CARD_IDS[c] for c in p["decks"][0]], [H.CARD_IDS[c] for c in p["decks"][1]], *p["factions"])
    bot = p["bot_side"]
    for a in p["prefix"] + [None]:
        if bot >= 0 and (0 if g.player == 1 else 1) == bot:
            assert int(g.expert_action()) == (p["action"] if a is None else a)
        if a is not None:
            g.step(a)
    return g


def record(tr, g, seed, action):
    tr.board, tr.seed, tr.records, tr.skipped, tr.depth = g.board, seed, [], [], 0
    raised = None
    try:
        g.step(action)
    except Exception as e:  # noqa: BLE001
        raised = type(e).__name__
    tr.board = None
    tr.depth = 0
    return raised


def measured(tier, rec):
    """(fault, depth, words, evictions pending) of the recorded call on the counting host build."""
    sys.path.insert(0, os.path.join(H.REPO, "tests"))
    import oracle_lib
    import scenario_lib as S
    orc = oracle_lib.Oracle(1, extended=tier, core="product_count")
    c = orc.L.orc_frame_counts()
    st = rec["before"]
    assert orc.scn_build(0, st["seed"], st["stream_pos"], S.encode_state(st)) == 0
    c[12] = c[13] = c[14] = c[15] = 0
    f, _ = orc.scn_op(0, S.encode_op(rec))
    return dict(fault=f, depth=int(c[13]), words=int(c[15]), seg=int(c[14]), at_guard=int(c[12]))


def main():
    from enums import UnitType
    from point import Point
    with gzip.open(SRC, "rt") as f:
        positions = json.load(f)["positions"]
    tr = G.Tracer()
    G.install(tr)
    out, by_name, recorded = [], {}, {}
    for p in positions:
        with contextlib.redirect_stdout(io.StringIO()):
            g = at_position(p)
            raised = record(tr, g, p["seed"], p["action"])
        name = f"{p['cls']}:{p['source']}:{len(p['prefix'])}:{p['action']}"
        by_name[name] = p
        recorded[name] = tr.records[0]
        assert raised == p["raised"], (name, raised)
        print(name, "tier", p["tier"], p["count"], "records", [(r["op"], r["raised"], len(r["activations"])) for r in tr.records], "skipped", tr.skipped)
        out.append({"test": name, "cls": p["cls"], "tier": p["tier"], "count": p["count"], "seed": p["seed"], "constructed": False,
                    "records": tr.records, "skipped": tr.skipped})
    for base, tile, owner, strength, seed in CONSTRUCTED:
        p = by_name[base]
        with contextlib.redirect_stdout(io.StringIO()):
            g = at_position(p)
            b = g.board
            player = b.local if int(b.local.order) == owner else b.remote
            # `tile` is in the orientation of the recorded call; Stormbound.step may turn the board before it makes the call
            want = [k for k, t in enumerate(recorded[base]["before"]["tiles"]) if t is not None]
            have = [y * 4 + x for y in range(5) for x in range(4) if b.board[y][x] is not None]
            if have != want:
                assert sorted(19 - k for k in have) == want, base
                tile = 19 - tile
            assert b.board[tile // 4][tile % 4] is None
            b.spawn_token_unit(player, Point(tile % 4, tile // 4), strength, [UnitType(TOKEN_TYPE)])
            b.random.seed(seed)   # the ONE RandomState object shared by game, board, players and cards
            raised = record(tr, g, seed, p["action"])
        name = f"constructed:{base}:token@{tile}:{owner}:{strength}:seed{seed}"
        assert len(tr.records) == 1 and not tr.skipped, (name, tr.skipped)
        count = measured(p["tier"], tr.records[0])
        print(name, "raised", raised, count, "activations", len(tr.records[0]["activations"]))
        out.append({"test": name, "cls": "constructed", "tier": p["tier"], "count": count, "seed": seed, "constructed": True,
                    "raised": raised, "records": tr.records, "skipped": tr.skipped})
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print("wrote", OUT, len(out), "boards", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
