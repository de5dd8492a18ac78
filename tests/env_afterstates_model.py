"""Python model of the afterstates contract (include/monsoon.h, monsoon_env_afterstates_dev) over the CPU oracle (test
helper, next to vec_env_model.py).

The oracle has no clone.  A slot's current state is rebuilt on a scratch oracle game by replaying the slot's episode from
its seed and decks: `History` records the committed actions of every slot's current episode through
VecEnvModel.on_commit, and the replay calls expert_action before every step of the scripted bot, so the stream advances as
it did.  One legal action is then stepped and the successor read (observe, features, have_winner, bases, fault); the next
action starts from a fresh replay.  O(steps^2) per slot: for small samples of slots.
"""
import numpy as np

import oracle_lib
from vec_env_model import FAULT_INT_CARD, bases


class History:
    """on_commit for a VecEnvModel: the committed actions (agent's and bot's) of every model slot's current episode."""

    def __init__(self):
        self.acts = {}   # j -> (episode, [action, ...])

    def __call__(self, j, episode, action, canon_hash):
        ep, lst = self.acts.get(j, (None, None))
        if ep != episode:
            lst = []
            self.acts[j] = (episode, lst)
        lst.append(int(action))

    def of(self, j, episode):
        ep, lst = self.acts.get(j, (None, None))
        return lst if ep == episode else []


def winner_code(orc, i):
    """-2 without a winner; else 0 / 1 / -1 by the rollout contract."""
    if not orc.have_winner(i):
        return -2
    b0, b1 = bases(orc.canon(i))
    return 0 if (b1 < 0 <= b0) else 1 if (b0 < 0 <= b1) else -1


class AfterstatesModel:
    """The afterstates of the slots of a VecEnvModel built with on_commit=history."""

    def __init__(self, model, history, extended=False):
        self.model, self.history = model, history
        self.orc = oracle_lib.Oracle(1, extended=extended)

    def rebuild(self, j):
        """Slot j's current state on the scratch game (copy.deepcopy of the game, stream included)."""
        m, orc = self.model, self.orc
        k = int(m.episode[j])
        f0, f1 = (int(m.factions[j, 0]), int(m.factions[j, 1])) if k == 0 else (0, 0)
        orc.reset(0, m.seed(j), m.decks[j, 0], m.decks[j, 1], f0, f1)
        for a in self.history.of(j, k):
            # the scripted bot's step: its expert_action drew from the stream (the heuristic opponent, 2, decides on copies)
            if m.opponent == 1 and orc.to_play(0) != m.agent_side:
                ea, _ = orc.expert_action(0)
                assert ea == a, (j, ea, a)
            orc.step(0, a)
        assert orc.canon_hash(0) == m.orc.canon_hash(j), f"slot {j}: the replay left the model's state"

    def slot(self, j, max_after):
        """dict for model slot j: n_legal, before (features or None), entries = [dict(action, status, reward, winner,
        features, obs)] for k < min(n_legal, max_after); features / obs are None where status != 0."""
        m, orc = self.model, self.orc
        if m.result[j] != -2:   # the episode ended before the agent could act: the next step reports it
            return dict(n_legal=0, before=None, entries=[])
        self.rebuild(j)
        legal = orc.legal_actions(0)
        before = orc.features(0)   # None where the observation raises
        entries = []
        for a in legal[:max_after]:
            self.rebuild(j)
            fs, r, _ = orc.step(0, a)
            if fs:   # the step raised: no reward, no winner
                entries.append(dict(action=a, status=fs, reward=0, winner=-2, features=None, obs=None))
                continue
            obs = orc.observe(0)
            e = dict(action=a, status=0 if obs is not None else FAULT_INT_CARD, reward=r, winner=winner_code(orc, 0), features=None,
                     obs=None)
            if obs is not None:
                e["features"], e["obs"] = orc.features(0), obs
            entries.append(e)
        return dict(n_legal=len(legal), before=before, entries=entries)


def compare_slot(want, got, i, max_after, ctx, obs=True):
    """Every output of slot i of VecEnv.afterstates (host copies, got[name][i]) against AfterstatesModel.slot: exact, floats by
    bit pattern.  Returns the number of entries compared."""
    assert int(got["n_legal"][i]) == want["n_legal"], (ctx, "n_legal", int(got["n_legal"][i]), want["n_legal"])
    shown = min(want["n_legal"], max_after)
    assert (got["action"][i, shown:] == 255).all(), (ctx, "action beyond the legal set")
    if want["before"] is not None:
        assert got["before_features"][i].tobytes() == want["before"].tobytes(), (ctx, "before_features")
    for k, e in enumerate(want["entries"]):
        c = (ctx, k, e["action"])
        assert int(got["action"][i, k]) == e["action"], c
        assert int(got["status"][i, k]) == e["status"], (c, "status", int(got["status"][i, k]), e["status"])
        assert int(got["reward"][i, k]) == e["reward"], (c, "reward")
        assert int(got["winner"][i, k]) == e["winner"], (c, "winner", int(got["winner"][i, k]), e["winner"])
        if e["status"] == 0:
            assert got["features"][i, k].tobytes() == e["features"].tobytes(), (c, "features", got["features"][i, k], e["features"])
            if obs:
                assert np.array_equal(got["obs"][i, k], e["obs"]), (c, "obs")
    return len(want["entries"])
