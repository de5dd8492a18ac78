"""Python model of saving and restoring vector-env slots (include/monsoon.h, monsoon_env_save_dev / monsoon_env_load_dev)
over the models of the env contract (tests/vec_env_model.py, tests/vec_env_heuristic_model.py), used unchanged (test
helper).

No state is ever copied here.  The env is deterministic, so a slot that received entry E -- saved from slot s after the
action prefix A -- and then plays the actions B is a fresh model of slot s that plays A, then B, from reset.  The
bookkeeping is a LINEAGE per tracked slot: the events that lead to its state,

    ("root", spec, slot)    episode 0 of `slot` of the env that `spec` describes
    ("act", a)              one step with action a
    ("move", spec, slot)    the state was loaded into `slot` of the env `spec`: from here on that slot's configuration
                            applies -- its seed0 and the env's stride, opponent kind, agent_side, max_steps, pool and (with
                            the heuristic opponent) weight table and row -- while the episode in flight, the episode
                            count and, without a pool, the decks are the carried ones

and a snapshot is a list of lineages.  A restore replays the entry's lineage on a fresh one-slot model and appends the
move.  A spec is the keyword dictionary of VecEnvModel (seed0, decks, factions, opponent, agent_side, seed_stride,
max_steps, pool, extended), plus opponent_weights / opponent_rows for the heuristic opponent.
"""
import numpy as np

from vec_env_heuristic_model import HeuristicVecEnvModel
from vec_env_model import VecEnvModel


def _fresh(spec, slot):
    kw = dict(spec)
    w, rows = kw.pop("opponent_weights", None), kw.pop("opponent_rows", None)
    if w is not None:
        kw.pop("opponent", None)
        return HeuristicVecEnvModel(kw.pop("seed0"), w, rows, slots=[slot], **kw)
    return VecEnvModel(slots=[slot], **kw)


def _move(model, spec, slot):
    """The one-slot model now lives in `slot` of the env `spec`."""
    seed0 = np.asarray(spec["seed0"], dtype=np.uint32)
    model.seed0[0] = int(seed0[slot])
    model.stride = int(spec.get("seed_stride", 0)) or len(seed0)
    model.agent_side, model.max_steps = int(spec.get("agent_side", 0)), int(spec.get("max_steps", 0))
    heuristic = spec.get("opponent_weights") is not None
    assert heuristic == isinstance(model, HeuristicVecEnvModel), "an entry moves between envs of one opponent kind here"
    if heuristic:
        model.set_opponents(spec["opponent_weights"], spec.get("opponent_rows"), np.array([slot]))
    else:
        model.opponent = int(spec.get("opponent", 0))
    pool = spec.get("pool")
    if pool is None:   # the carried deck bytes are the slot's decks from now on
        model.pool = None
        model.reset_decks = model.decks.copy()
    else:
        model.pool = np.asarray(pool, dtype=np.uint8)


def replay(lineage):
    model = None
    for ev in lineage:
        if ev[0] == "root":
            model = _fresh(ev[1], ev[2])
        elif ev[0] == "act":
            model.step([ev[1]])
        else:
            _move(model, ev[1], ev[2])
    return model


class EnvSnapshotModel:
    """The slots `slots` (None = all) of the env that `spec` describes, each a one-slot model with its lineage."""

    PER_CALL = (("reward", 0), ("done", False), ("winner", -2), ("truncated", False), ("fault", 0), ("illegal", False), ("final_hash", 0))

    def __init__(self, spec, slots=None):
        self.spec = spec
        self.n = len(np.asarray(spec["seed0"]))
        self.slots = list(range(self.n)) if slots is None else [int(s) for s in slots]
        self.lineage = {s: (("root", spec, s),) for s in self.slots}
        self.model = {s: replay(self.lineage[s]) for s in self.slots}
        self.fresh = set()   # slots loaded since their last step: their per-call views read as after a step that ended nothing

    def step(self, actions):
        """actions: one per tracked slot, in the order of self.slots."""
        for s, a in zip(self.slots, actions):
            self.model[s].step([int(a)])
            self.lineage[s] += (("act", int(a)),)
        self.fresh.clear()
        return self.views()

    def snapshot(self, slots=None):
        """The entries of `slots` (tracked ones; None = all tracked, in order).  An untracked or out-of-range slot gives
        None: an entry this model cannot load."""
        return [self.lineage.get(int(s)) for s in (self.slots if slots is None else slots)]

    def restore(self, snap, src=None, dst=None, spec=None):
        """-> loaded [m] as the device reports it.  Pairs whose dst is not tracked are judged (loaded or not) but not modelled."""
        m = len(src) if src is not None else len(dst) if dst is not None else len(snap)
        src = range(m) if src is None else [int(x) for x in src]
        dst = range(m) if dst is None else [int(x) for x in dst]
        loaded = np.zeros(m, dtype=np.uint8)
        for j, (s, d) in enumerate(zip(src, dst)):
            if not (0 <= s < len(snap) and 0 <= d < self.n and snap[s] is not None):
                continue
            loaded[j] = 1
            if d in self.model:
                self.lineage[d] = snap[s] + (("move", self.spec, d),)
                self.model[d] = replay(self.lineage[d])
                self.fresh.add(d)
        return loaded

    def views(self):
        out = {}
        for k in self.model[self.slots[0]].views:
            out[k] = np.concatenate([self.model[s].views[k] for s in self.slots])
        for i, s in enumerate(self.slots):
            if s in self.fresh:
                for k, v in self.PER_CALL:
                    out[k][i] = v
        return out

    def hashes(self):
        return np.array([self.model[s].hashes()[0] for s in self.slots], dtype=np.uint64)

    def episodes(self):
        return np.array([int(self.model[s].episode[0]) for s in self.slots])
