"""The contract of monsoon_replay_logged_dev (include/monsoon.h) as a few lines of Python over the CPU oracle.  Test
infrastructure only.

    reset(seed, decks)
    for k, a in enumerate(log[:steps]):
        if a fault so far, a winner, or the observation raised after the step before:   stop ENDED_EARLY
        if a >= 156 or (a != 155 and a is not legal):                                   stop ILLEGAL
        if the entry is kept:  a row of (observe, legal_mask, to_play, a, bot, game, k, canon_hash) BEFORE the step
        if to_play is the bot:  b = expert_action()    (raises -> stop BOT_RAISED;  b != a -> stop BOT_DIFFERS)
        step(a)                                        (faults, or the observation raises -> the game is over)
"""
import numpy as np

import oracle_lib
from monsoon_amd.game_log import row_bases

EXPERT = -1
FAULT_INT_CARD = 2
OK, ILLEGAL, BOT_DIFFERS, BOT_RAISED, ENDED_EARLY = range(5)
COLS = ("obs", "legal", "obs_raises", "to_play", "action", "bot", "game", "step", "state_hash")


def legal_bytes(mask):
    """uint8[156] of a uint64[3] legal mask."""
    return np.unpackbits(np.ascontiguousarray(mask, dtype="<u8").view(np.uint8), bitorder="little")[:156]


def fixture_log(g):
    """(action uint8[n][T], steps int32[n]) of a golden trace: game i's entries are action[offsets[i]:offsets[i+1]]; a
    trailing 255 (a bot that raised) is not an entry."""
    off = g["offsets"]
    n = len(off) - 1
    steps = np.array([int(((g["action"][off[i]:off[i + 1]]) != 255).sum()) for i in range(n)], dtype=np.int32)
    action = np.full((n, max(int(np.diff(off).max()), 1)), 255, dtype=np.uint8)
    for i in range(n):
        action[i, :off[i + 1] - off[i]] = g["action"][off[i]:off[i + 1]]
    return action, steps


def other_legal_entry(g, action, game, first):
    """(k, a): the first entry k >= first of `game` in golden trace g where an action a other than the logged one is legal
    (the lowest such a), from the fixture's own masks."""
    off = g["offsets"]
    for k in range(first, int(off[game + 1] - off[game])):
        legal = np.nonzero(legal_bytes(g["legal"][off[game] + k]))[0]
        others = [int(a) for a in legal if a != action[game, k]]
        if others:
            return k, others[0]
    raise ValueError("no such entry")


def replay(matches, deck_pairs, action, steps, keep=None, tier=0):
    """The rows and host outputs of the call, as numpy arrays: COLS with S rows each (state_hash uint64), reached bool[S]
    (False = a row behind a stop: action 255, the other columns unspecified), status, replayed, fault [n] and final
    uint64[n], the canonical hash every game is left in."""
    deck_pairs = np.asarray(deck_pairs, dtype=np.uint8).reshape(-1, 2, 12)
    n = len(matches)
    base, total = row_bases(steps, keep)
    out = dict(obs=np.zeros((total, 27, 5, 4), np.int32), legal=np.zeros((total, 156), np.uint8), obs_raises=np.zeros(total, np.uint8),
               to_play=np.zeros(total, np.uint8), action=np.full(total, 255, np.uint8), bot=np.zeros(total, np.uint8),
               game=np.zeros(total, np.int32), step=np.zeros(total, np.int32), state_hash=np.zeros(total, np.uint64),
               reached=np.zeros(total, bool), status=np.zeros(n, np.uint8), replayed=np.zeros(n, np.int32), fault=np.zeros(n, np.uint8),
               final=np.zeros(n, np.uint64))
    orc = oracle_lib.Oracle(1, extended=tier)
    for g, m in enumerate(matches):
        d = deck_pairs[int(m["deck"])]
        rows = (int(m["p1"]), int(m["p2"]))
        fault = orc.reset(0, int(m["seed"]), d[0], d[1])
        status, done, r = OK, 0, int(base[g])
        for k in range(int(steps[g])):
            if fault or orc.have_winner(0):
                status = ENDED_EARLY
                break
            a = int(action[g, k])
            mask = orc.legal_mask(0)
            if a >= 156 or (a != 155 and not (int(mask[a >> 6]) >> (a & 63)) & 1):
                status = ILLEGAL
                break
            side = orc.to_play(0)
            bot = rows[side] == EXPERT
            if keep is None or keep[g][k]:
                obs = orc.observe(0)
                if obs is not None:
                    out["obs"][r] = obs
                out["obs_raises"][r] = obs is None
                out["legal"][r], out["to_play"][r], out["action"][r], out["bot"][r] = legal_bytes(mask), side, a, bot
                out["game"][r], out["step"][r], out["state_hash"][r], out["reached"][r] = g, k, orc.canon_hash(0), True
                r += 1
            if bot:
                b, f = orc.expert_action(0)
                if f:
                    status, fault = BOT_RAISED, f
                    break
                if b != a:
                    status = BOT_DIFFERS
                    break
            fault = orc.step(0, a)[0]
            done += 1
            if not fault and orc.observe(0) is None:
                fault = FAULT_INT_CARD
        out["status"][g], out["replayed"][g], out["fault"][g], out["final"][g] = status, done, fault, orc.canon_hash(0)
    return out


def fnv1a64_rows(rows):
    """oracle_lib.fnv1a64 of the bytes of every row of a 2-D uint8 array, vectorised over the rows."""
    h = np.full(len(rows), 0xCBF29CE484222325, dtype=np.uint64)
    prime = np.uint64(0x100000001B3)
    for j in range(rows.shape[1]):
        h = (h ^ rows[:, j]) * prime
    return h


def check_fixture(g, rows, base, steps, bot_fixture=False):
    """The rows of a replay of golden trace g (every entry kept) against the reference's own values: entry t's legal mask
    (where the fixture has masks), and the observation and state of entry t+1 = the reference's after step t.  A row is
    skipped only where the fixture itself marks it: hash == 0, or the last step of a game whose fault flag is set.
    Returns (rows checked, rows)."""
    off = g["offsets"]
    checked = total = 0
    obs_hash = fnv1a64_rows(np.ascontiguousarray(rows["obs"]).reshape(len(rows["obs"]), -1).view(np.uint8)) if "obs" in g.files else None
    for i in range(len(off) - 1):
        for t in range(int(steps[i])):
            r, j = int(base[i]) + t, int(off[i]) + t
            total += 1
            assert rows["action"][r] == g["action"][j] and rows["game"][r] == i and rows["step"][r] == t, (i, t)
            if "legal" in g.files:
                assert np.array_equal(rows["legal"][r], legal_bytes(g["legal"][j])), (i, t)
            if bot_fixture:
                assert rows["bot"][r] == 1, (i, t)
            if "bot" in g.files:
                assert rows["bot"][r] == g["bot"][j], (i, t)
            if t == 0:   # (the state before the first step: the fixture's init_hash where it has one)
                if "init_hash" in g.files:
                    assert rows["state_hash"][r] == g["init_hash"][i], i
                    checked += 1
                continue
            marked = g["hash"][j - 1] == 0 or (g["fault"][i] and t - 1 == off[i + 1] - off[i] - 1)
            if marked:
                continue
            assert rows["state_hash"][r] == g["hash"][j - 1], (i, t)
            if obs_hash is not None:
                assert not rows["obs_raises"][r] and obs_hash[r] == g["obs"][j - 1], (i, t)
            checked += 1
    return checked, total


def same_rows(dev, model, cols=COLS):
    """A device result (game_log.dataset's dict, or host copies of its columns) equals the model's: the action of every row,
    every other column on the rows the replay reached, and the three host arrays.  Returns the first difference or None."""
    for c in ("status", "replayed", "fault"):
        if not np.array_equal(dev[c], model[c]):
            return c
    for c in cols:
        a = dev[c].cpu().numpy() if hasattr(dev[c], "cpu") else np.asarray(dev[c])
        if c == "state_hash":
            a = a.view(np.uint64)
        if a.shape != model[c].shape:
            return c + " shape"
        on = slice(None) if c == "action" else model["reached"]
        if not np.array_equal(a[on], model[c][on]):
            return c
    return None
