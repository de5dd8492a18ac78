"""Python model of the vector env with the heuristic opponent (include/monsoon.h, opponent 2) over the CPU oracle (test
helper).  The opponent's turn is the reference's HeuristicAgent loop: Oracle.decide with the slot's weight row, then step,
under the env's end rules, for at most OPP_BOUND decisions per call."""
import numpy as np

from vec_env_model import VecEnvModel

FAULT_OPP_BOUND = 28   # msb_base.h: the heuristic opponent still to play after OPP_BOUND decisions in one call
OPP_BOUND = 64


class HeuristicVecEnvModel(VecEnvModel):
    """opponent_weights: [k][10]; opponent_rows: [n] over the WHOLE env (None = row 0), taken for the model's slots."""

    def __init__(self, seed0, opponent_weights, opponent_rows=None, slots=None, on_decide=None, **kw):
        n_all = len(np.asarray(seed0))
        sl = np.arange(n_all) if slots is None else np.asarray(slots, dtype=np.int64)
        self.set_opponents(opponent_weights, opponent_rows, sl)
        self.opp_bound_turns = []   # the opponent's decisions in every turn the guard ended
        self.on_decide = on_decide  # on_decide(j, action, legal mask words) after every decision of the opponent
        super().__init__(seed0, opponent=2, slots=slots, **kw)

    def set_opponents(self, weights, rows=None, slots=None):
        """A league update: applies from the next decision (as monsoon_env_set_opponents between steps)."""
        w = np.asarray(weights, dtype=np.float64)
        self.weights = w[None] if w.ndim == 1 else w
        sl = self.slots if slots is None else slots
        self.rows = np.zeros(len(sl), dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)[sl]

    def _bot_turn(self, j):
        turn = []
        w = self.weights[self.rows[j]]
        for _ in range(OPP_BOUND):
            if self.orc.to_play(j) == self.agent_side:
                return
            a, _, mask = self.orc.decide(j, w)
            if self.on_decide is not None:
                self.on_decide(j, int(a), mask)
            turn.append(int(a))
            fs, _, _ = self.orc.step(j, a)
            if self._after_step(j, a, fs):
                return
        if self.orc.to_play(j) != self.agent_side:
            self.bot_bound_hits += 1
            self.opp_bound_turns.append(turn)
            self._end(j, -1, FAULT_OPP_BOUND)
