"""The contract of monsoon_replay_logged_after_dev (include/monsoon.h) over the CPU oracle: monsoon_replay_logged_dev's
order (tests/replay_model.py) with, in its step 3, the afterstates of the state the row shows in monsoon_env_after's
meaning (tests/env_afterstates_model.py).  Test infrastructure only.

The oracle has no clone: AfterstatesModel.rebuild replays the game's committed actions on a scratch game before every
candidate, the bot's expert_action included, so a row costs (1 + candidates) replays of the entries before it.  Quadratic
in a game's length: for whole games of a few matches.
"""
import numpy as np

import oracle_lib
import replay_model as RM
from env_afterstates_model import AfterstatesModel, History, compare_slot
from monsoon_amd.game_log import row_bases

AFTER_COLS = ("n_legal", "chosen", "after_action", "after_status", "after_reward", "after_winner", "after_features",
              "before_features", "after_obs")


class _Game:
    """What AfterstatesModel reads of a VecEnvModel, for one replayed match: slot 0, episode 0, the match's seed and decks;
    the side that is not the scripted bot is the 'agent', so the replay of a bot step runs its expert_action."""

    def __init__(self, orc, match, decks):
        p1, p2 = int(match["p1"]), int(match["p2"])
        assert not (p1 == RM.EXPERT and p2 == RM.EXPERT), "a match with the bot on both sides has no agent side"
        self.orc, self.decks, self._seed = orc, np.asarray(decks)[None], int(match["seed"])
        self.result, self.episode, self.factions = np.array([-2]), np.array([0]), np.zeros((1, 2), dtype=np.int64)
        self.opponent = 1 if RM.EXPERT in (p1, p2) else 0
        self.agent_side = 1 if p1 == RM.EXPERT else 0

    def seed(self, j):
        return self._seed


def rows(matches, deck_pairs, action, steps, max_after, games, keep=None, tier=0):
    """A generator over the kept, reached entries of `games` (match indices): (r, g, k, row, orc) with row = dict(n_legal,
    chosen, before (features or None), entries, action, bot, to_play) and orc the oracle, game 0 of which is in the row's
    state (read it, do not step it).  The rows of a game end where its replay stops."""
    deck_pairs = np.asarray(deck_pairs, dtype=np.uint8).reshape(-1, 2, 12)
    base, _ = row_bases(steps, keep)
    orc = oracle_lib.Oracle(1, extended=tier)
    for g in games:
        m = matches[g]
        d = deck_pairs[int(m["deck"])]
        sides = (int(m["p1"]), int(m["p2"]))
        hist = History()
        after = AfterstatesModel(_Game(orc, m, d), hist, extended=tier)
        fault = orc.reset(0, int(m["seed"]), d[0], d[1])
        r = int(base[g])
        for k in range(int(steps[g])):
            if fault or orc.have_winner(0):
                break
            a = int(action[g, k])
            legal = orc.legal_actions(0)
            if a >= 156 or (a != 155 and a not in legal):
                break
            side = orc.to_play(0)
            bot = sides[side] == RM.EXPERT
            if keep is None or keep[g][k]:
                row = after.slot(0, max_after)   # (every rebuild leaves the scratch game in orc's state, or asserts)
                assert row["n_legal"] == len(legal)
                row.update(chosen=legal.index(a) if a in legal else -1, action=a, bot=bot, to_play=side)
                yield r, g, k, row, orc
                r += 1
            if bot:
                b, f = orc.expert_action(0)
                if f or b != a:
                    break
            fault = orc.step(0, a)[0]
            hist(0, 0, a, None)
            if not fault and orc.observe(0) is None:
                fault = RM.FAULT_INT_CARD


def replay_after(matches, deck_pairs, action, steps, max_after, games, keep=None, tier=0):
    """{r: row} of rows()."""
    return {r: row for r, _, _, row, _ in rows(matches, deck_pairs, action, steps, max_after, games, keep, tier)}


def host(d, cols=AFTER_COLS):
    """The candidate columns of a dataset dict as numpy arrays under monsoon_env_after's names (compare_slot's)."""
    names = {"n_legal": "n_legal", "chosen": "chosen", "after_action": "action", "after_status": "status", "after_reward": "reward",
             "after_winner": "winner", "after_features": "features", "before_features": "before_features", "after_obs": "obs"}
    return {names[c]: (d[c].cpu().numpy() if hasattr(d[c], "cpu") else np.asarray(d[c])) for c in cols if c in d}


def compare_row(want, got, r, max_after, ctx):
    """Every specified entry of row r of the device's candidate columns (host()) against the model's row: exact, floats by
    bit pattern.  Returns the entries compared."""
    n = compare_slot(want, got, r, max_after, ctx, obs="obs" in got)
    if "chosen" in got:
        assert int(got["chosen"][r]) == want["chosen"], (ctx, "chosen", int(got["chosen"][r]), want["chosen"])
    if want["before"] is None and "before_features" in got:
        assert not got["before_features"][r].view(np.uint64).any(), (ctx, "before_features where the observation raises")
    return n


def same_candidates(a, b, rows_a=slice(None), rows_b=slice(None)):
    """Two sets of candidate columns (host()) equal on what the contract specifies, rows_a of a against rows_b of b: n_legal,
    chosen, action and before_features whole, status / reward / winner on the entries that exist, features / obs on those
    with status 0.  Returns the first column that differs, or None."""
    k = a["action"].shape[1]
    if b["action"].shape[1] != k:
        return "K"
    nl = a["n_legal"][rows_a]
    exists = np.arange(k)[None, :] < nl[:, None]
    for c in ("n_legal", "chosen", "action", "before_features"):
        if c in a and not np.array_equal(a[c][rows_a].view(np.uint8), b[c][rows_b].view(np.uint8)):
            return c
    for c in ("status", "reward", "winner"):
        if c in a and not np.array_equal(a[c][rows_a][exists], b[c][rows_b][exists]):
            return c
    ok = exists & (a["status"][rows_a] == 0)
    for c in ("features", "obs"):
        if c in a and not np.array_equal(a[c][rows_a][ok].view(np.uint8), b[c][rows_b][ok].view(np.uint8)):
            return c
    return None


def stream_words(orc, match, decks, action, steps):
    """The words of its stream a replayed game has consumed after its last entry (the bot's draws included): the position
    of the record's next word -- the last four bytes of the canonical record -- in RandomState(seed)'s output."""
    import ctypes
    seed, sides = int(match["seed"]), (int(match["p1"]), int(match["p2"]))
    orc.reset(0, seed, decks[0], decks[1])
    for k in range(int(steps)):
        if sides[orc.to_play(0)] == RM.EXPERT:
            orc.expert_action(0)
        if orc.step(0, int(action[k]))[0]:
            break
    words = np.zeros(4096, dtype=np.uint32)
    orc.L.orc_rng_u32(ctypes.c_uint32(seed), len(words), words.ctypes.data_as(ctypes.c_void_p))
    at = np.nonzero(words == int.from_bytes(orc.canon(0)[-4:], "little"))[0]
    assert len(at), "the game's next word is not among the first 4 096 of its stream"
    return int(at[0])


def decision(w, before, status, features, score):
    """The heuristic decision rebuilt from a row's candidates: (index of the first maximum, its score, the scores).  An
    entry whose look-ahead raised (status != 0) scores 0.0, and so does every entry where the row's observation raises
    (before is None): evo/heuristic_agent.py's except Exception -> 0.0."""
    s = [score(w, before, features[k]) if (before is not None and status[k] == 0) else 0.0 for k in range(len(status))]
    best = 0
    for k in range(1, len(s)):
        if s[k] > s[best]:
            best = k
    return best, s[best], s
