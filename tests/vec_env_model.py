"""Python model of the vector env contract (include/monsoon.h, monsoon_env_*) over the CPU oracle (test helper).

Every slot of the device env is independent, so the model replays any subset of slots: `slots` names them, and the
seed schedule (episode k of slot i starts from seed0[i] + k * stride, stride 0 = n of the WHOLE env) and the reset decks
are taken from the full arrays.  The views it returns have the device env's dtypes (legal as bool) for those slots.
"""
import numpy as np

import oracle_lib
from monsoon_amd.cards import C5_STREAM_XOR, draw_random_decks_numpy

FAULT_INT_CARD = 2
FAULT_BOT_BOUND = 27   # msb_base.h: the scripted bot still to play after BOT_BOUND actions in one call
BOT_BOUND = 64
SKIP, PASS = 255, 155


def bases(canon):
    """(FIRST's base, SECOND's base) from a canonical record (monsoon_amd/csrc/canon.h)."""
    b = bytes(canon)
    o1 = 24 + 3 * b[21] + 11 * b[22]
    return int.from_bytes(b[12:14], "little", signed=True), int.from_bytes(b[o1:o1 + 2], "little", signed=True)


def is_noop_use(a):
    """A USE whose index falls off the reference's tile loop (rules.h step, idx == 20): nothing happens, not even the
    mana cost -- the reference's scripted bot can pick such actions for ever without ending its turn."""
    return 64 <= a < 148 and (a - 64) % 21 == 20


def legal_bools(mask3):
    m = [int(x) for x in mask3]
    return np.array([(m[a >> 6] >> (a & 63)) & 1 for a in range(156)], dtype=bool)


class VecEnvModel:
    def __init__(self, seed0, decks=None, factions=None, opponent=0, agent_side=0, seed_stride=0, max_steps=0, pool=None,
                 extended=False, slots=None, on_commit=None):
        seed0 = np.asarray(seed0, dtype=np.uint32)
        n_all = len(seed0)
        self.slots = np.arange(n_all) if slots is None else np.asarray(slots, dtype=np.int64)
        m = len(self.slots)
        self.m = m
        self.stride = int(seed_stride) or n_all
        self.seed0 = seed0[self.slots].astype(np.int64)
        self.pool = None if pool is None else np.asarray(pool, dtype=np.uint8)
        if self.pool is None:
            d = np.asarray(decks, dtype=np.uint8)
            d = np.broadcast_to(d, (n_all, 2, 12)) if d.shape == (2, 12) else d.reshape(n_all, 2, 12)
            self.reset_decks = d[self.slots].copy()
        f = np.zeros((n_all, 2), dtype=np.uint8) if factions is None else np.asarray(factions, dtype=np.uint8).reshape(n_all, 2)
        self.factions = f[self.slots].copy()
        self.opponent, self.agent_side, self.max_steps = int(opponent), int(agent_side), int(max_steps)
        self.on_commit = on_commit   # on_commit(j, episode, action, canon hash) after every committed step (agent or bot)
        self.orc = oracle_lib.Oracle(m, extended=extended)
        self.episode = np.zeros(m, dtype=np.int64)
        self.decks = np.zeros((m, 2, 12), dtype=np.uint8)   # the decks of each slot's current episode
        self.steps = np.zeros(m, dtype=np.int64)
        self.result = np.full(m, -2, dtype=np.int64)       # -2 = live; else the ended episode's winner code
        self.end_fault = np.zeros(m, dtype=np.int64)
        self.end_trunc = np.zeros(m, dtype=bool)
        self.bot_bound_hits = 0
        self.bot_bound_turns = []   # the bot's actions in every turn the guard ended
        for j in range(m):
            self._start(j)
        self.views = self._blank()
        for j in range(m):
            self._write_state(j)

    # ---- the contract -------------------------------------------------------------------------------
    def seed(self, j, k=None):
        k = self.episode[j] if k is None else k
        return int(self.seed0[j] + k * self.stride) & 0xFFFFFFFF

    def _end(self, j, result, fault=0, truncated=False):
        self.result[j], self.end_fault[j], self.end_trunc[j] = result, fault, truncated

    def _start(self, j):
        k, s = int(self.episode[j]), self.seed(j)
        self.decks[j] = draw_random_decks_numpy([s ^ C5_STREAM_XOR], self.pool)[0] if self.pool is not None else self.reset_decks[j]
        f0, f1 = (int(self.factions[j, 0]), int(self.factions[j, 1])) if k == 0 else (0, 0)
        f = self.orc.reset(j, s, self.decks[j, 0], self.decks[j, 1], f0, f1)
        self.steps[j] = 0
        self._end(j, -2)
        if not f and self.orc.observe(j) is None:
            f = FAULT_INT_CARD   # the reference's reset() returns get_observation()
        if f:
            self._end(j, -1, f)
        elif self.opponent and self.orc.to_play(j) != self.agent_side:
            self._bot_turn(j)

    def _after_step(self, j, action, f):
        """A committed step of either side: True when it ended the episode."""
        self.steps[j] += 1
        if self.on_commit is not None:
            self.on_commit(j, int(self.episode[j]), action, self.orc.canon_hash(j))
        if not f and self.orc.observe(j) is None:
            f = FAULT_INT_CARD
        if f:
            self._end(j, -1, f)
        elif self.orc.have_winner(j):
            b0, b1 = bases(self.orc.canon(j))
            self._end(j, 0 if (b1 < 0 <= b0) else 1 if (b0 < 0 <= b1) else -1)
        elif self.max_steps and self.steps[j] >= self.max_steps:
            self._end(j, -1, 0, True)
        return self.result[j] != -2

    def _bot_turn(self, j):
        turn = []
        for _ in range(BOT_BOUND):
            if self.orc.to_play(j) == self.agent_side:
                return
            a, f = self.orc.expert_action(j)
            turn.append(a)
            if f:
                self._end(j, -1, f)
                return
            fs, _, _ = self.orc.step(j, a)
            if self._after_step(j, a, fs):
                return
        if self.orc.to_play(j) != self.agent_side:
            self.bot_bound_hits += 1
            self.bot_bound_turns.append(turn)
            self._end(j, -1, FAULT_BOT_BOUND)

    def agent_step(self, j, a):
        """One slot's part of a step: (reward, illegal).  The slot's episode may end (self.result[j] != -2)."""
        if self.result[j] != -2 or a == SKIP:
            return 0, 0
        if a >= 156 or (a != PASS and not legal_bools(self.orc.legal_mask(j))[a]):
            return 0, 1
        fs, r, _ = self.orc.step(j, a)
        if not self._after_step(j, a, fs) and self.opponent:
            self._bot_turn(j)
        return r, 0

    def step(self, actions):
        """actions[m] for the model's slots -> the views (numpy, same names and dtypes as VecEnv's)."""
        v = self.views
        for j in range(self.m):
            r, ill = self.agent_step(j, int(actions[j]))
            ended = self.result[j] != -2
            v["reward"][j], v["illegal"][j], v["done"][j] = r, ill, ended
            v["winner"][j] = self.result[j] if ended else -2
            v["truncated"][j] = ended and self.end_trunc[j]
            v["fault"][j] = self.end_fault[j] if ended else 0
            v["final_hash"][j] = np.uint64(self.orc.canon_hash(j)).view(np.int64) if ended else 0
            if ended:
                self.episode[j] += 1
                self._start(j)
            v["episode"][j] = self.episode[j]
            self._write_state(j)
        return v

    def hashes(self):
        return np.array([self.orc.canon_hash(j) for j in range(self.m)], dtype=np.uint64)

    # ---- views --------------------------------------------------------------------------------------
    def _blank(self):
        m = self.m
        return dict(obs=np.zeros((m, 27, 5, 4), np.int32), legal=np.zeros((m, 156), bool), obs_raises=np.zeros(m, bool),
                    to_play=np.zeros(m, np.uint8), reward=np.zeros(m, np.int8), done=np.zeros(m, bool), winner=np.full(m, -2, np.int8),
                    truncated=np.zeros(m, bool), fault=np.zeros(m, np.uint8), illegal=np.zeros(m, bool), episode=np.zeros(m, np.int32),
                    final_hash=np.zeros(m, np.int64))

    def _write_state(self, j):
        v = self.views
        v["to_play"][j] = self.orc.to_play(j)
        v["legal"][j] = legal_bools(self.orc.legal_mask(j))
        o = self.orc.observe(j)
        v["obs_raises"][j] = o is None
        v["obs"][j] = 0 if o is None else o
