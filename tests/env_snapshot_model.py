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

The bytes of an entry (monsoon_amd/csrc/env_snap.h) are modelled too, for all three record builds: entry_layout gives the
sizes from the build's record size, build_entry puts an entry together from what the handle exports by another path
(monsoon_state_save: the meta row, the record and the stream of one slot).
"""
import numpy as np

from vec_env_heuristic_model import HeuristicVecEnvModel
from vec_env_model import VecEnvModel


SNAP_MAGIC = 0x50414E53                     # "SNAP"
HEAD_BYTES, META_BYTES, DECK_BYTES = 16, 32, 24
BODY_AT = 80                                # header, meta row, 24 deck bytes and 8 bytes of zero
MT_BYTES, OUT_BYTES = 624 * 4, 2 * 624 * 4  # the raw stream state, the two tempered blocks
PASS_GRANULES = 64 * 10                     # the copy kernels move 64 lanes x SNAP_PASS granules per pass
BLOB_HEAD = 8                               # monsoon_state_save: {u32 magic, u32 record bytes}, meta row, record, stream


def record_bytes(extended):
    """The record size of a build, from the size of its state blob (a host function of the library: no GPU needed)."""
    from monsoon_amd import _lib
    return int(_lib.load(int(extended)).monsoon_state_blob_bytes()) - BLOB_HEAD - META_BYTES - MT_BYTES - OUT_BYTES


def entry_layout(extended):
    """Sizes of one saved slot of record build 0 / 1 / 2: entry bytes, body granules (record + rng_mt + rng_out), the byte
    offsets of the two seams inside the entry, the passes of the copy loop and the granules of its last pass."""
    rec = record_bytes(extended)
    assert rec % 16 == 0
    body = (rec + MT_BYTES + OUT_BYTES) // 16
    passes = -(-body // PASS_GRANULES)
    return dict(record_bytes=rec, entry_bytes=BODY_AT + 16 * body, body_granules=body, mt_at=BODY_AT + rec,
                out_at=BODY_AT + rec + MT_BYTES, passes=passes, tail_granules=body - (passes - 1) * PASS_GRANULES)


def build_entry(extended, version, episode, decks, blob):
    """The entry monsoon_env_save_dev writes for a slot whose monsoon_state_save blob is `blob`, whose episode count is
    `episode` and whose current decks are `decks` ([2][12] uint8): header {magic, monsoon_version(), record words, episode},
    the meta row, the decks and 8 zero bytes, then record, rng_mt and rng_out as they sit in the blob."""
    lay = entry_layout(extended)
    blob = np.frombuffer(bytes(blob), dtype=np.uint8)
    assert len(blob) == BLOB_HEAD + META_BYTES + lay["record_bytes"] + MT_BYTES + OUT_BYTES
    assert int(blob[4:8].view("<u4")[0]) == lay["record_bytes"]
    head = np.array([SNAP_MAGIC, int(version) & 0xFFFFFFFF, lay["record_bytes"] // 4, int(episode) & 0xFFFFFFFF], dtype="<u4")
    out = np.concatenate([head.view(np.uint8), blob[BLOB_HEAD:BLOB_HEAD + META_BYTES], np.asarray(decks, dtype=np.uint8).reshape(24),
                          np.zeros(8, dtype=np.uint8), blob[BLOB_HEAD + META_BYTES:]])
    assert len(out) == lay["entry_bytes"]
    return out


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
