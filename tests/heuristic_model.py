"""An independent model of the heuristic agent's leaf math (test helper): the reference's StateFeatures
(evo/features.py) computed from the (27, 5, 4) int32 observation alone, and HeuristicAgent.score_action's score
(evo/heuristic_agent.py with WeightVector.dot_product).  Written from the reference's documented behaviour in float64
with the reference's order of operations; it shares no code with the library or the CPU oracle, so the tests that
compare the two with it see a wrong feature, a wrong score or a miscompile of the shared leaf headers.

- features(): integer sums are exact; ratios are true divisions of the converted values; threat and protection are
  accumulated tile by tile in row-major order (protection: the unit term before the structure term of a tile); clips
  where the reference clips.  Vectorised across games: adding a masked 0.0 to an accumulator that is never -0.0 is exact.
- score(): enemy - agent - penalty, where agent / enemy are the sequential chain acc = fma(w[i], +-d[i], acc) from 0.0
  (np.dot of ten float64 on the reference's BLAS, pinned by tests/golden/score_kat.npz); each fma is evaluated exactly
  and rounded once -- no BLAS, no libm fma.
- decide(): the first maximum over the ascending legal list (np.argmax).
"""
import math
from fractions import Fraction

import numpy as np

HAND_SENTINEL = 32767


def _masked(v, keep):
    return np.where(keep, v, 0)


def features(obs):
    """obs: int32 (..., 27, 5, 4) observations -> float64 (..., 10) StateFeatures.get_feature_vector()."""
    obs = np.asarray(obs)
    lead = obs.shape[:-3]
    o = obs.reshape(-1, 27, 20).astype(np.int64)
    n = o.shape[0]
    f = np.zeros((n, 10), dtype=np.float64)

    # _extract_*: a value of exactly -1 is "missing": mana 0.0, base 20.0 (also a base really at -1 after a win)
    mana = np.where(o[:, 13, 0] != -1, o[:, 13, 0].astype(np.float64), 0.0)
    health = np.where(o[:, 14, 0] != -1, o[:, 14, 0].astype(np.float64), 20.0)
    opp_health = np.where(o[:, 23, 0] != -1, o[:, 23, 0].astype(np.float64), 20.0)

    # _calculate_mana_efficiency: min(10, max(3, mana + 2)); clip(1 - mana / est, 0, 1)
    est = np.minimum(10.0, np.maximum(3.0, mana + 2.0))
    f[:, 0] = np.clip(1.0 - mana / est, 0.0, 1.0)
    f[:, 1] = health - opp_health

    # strengths of the unit / structure planes; -1 is skipped (a real strength of -1 too)
    lu_s, ls_s, ru_s, rs_s = o[:, 1], o[:, 5], o[:, 17], o[:, 21]
    player = _masked(lu_s, lu_s != -1).sum(axis=1) + _masked(ls_s, ls_s != -1).sum(axis=1)
    opponent = _masked(ru_s, ru_s != -1).sum(axis=1) + _masked(rs_s, rs_s != -1).sum(axis=1)
    total = player + opponent
    diff = player - opponent
    f[:, 2] = np.divide(diff.astype(np.float64), total.astype(np.float64), out=np.zeros(n), where=total != 0)

    # _calculate_front_line_advantage: rows from the id planes
    rows = np.arange(20) // 4
    lu_id, ru_id = o[:, 0] != -1, o[:, 16] != -1
    any_l, any_r = lu_id.any(axis=1), ru_id.any(axis=1)
    player_adv = np.where(any_l, np.where(lu_id, rows, 99).min(axis=1), 4)
    opp_adv = np.where(any_r, np.where(ru_id, rows, -1).max(axis=1), 0)
    f[:, 3] = np.where(any_l | any_r, (opp_adv - player_adv).astype(np.float64) / 4.0, 0.0)

    f[:, 4] = diff.astype(np.float64)
    f[:, 5] = (lu_id.sum(axis=1) - ru_id.sum(axis=1)).astype(np.float64)
    f[:, 6] = ((o[:, 4] != -1).sum(axis=1) - (o[:, 20] != -1).sum(axis=1)).astype(np.float64)

    # _calculate_base_threat / _calculate_protection: row-major accumulation, weights (row + 1) / 5 and (5 - row) / 5
    threat = np.zeros(n)
    protection = np.zeros(n)
    for t in range(20):
        row = t // 4
        s = ru_s[:, t]
        threat = threat + np.where(s != -1, s.astype(np.float64) * ((row + 1) / 5.0), 0.0)
        w = (5 - row) / 5.0
        s = lu_s[:, t]
        protection = protection + np.where(s != -1, s.astype(np.float64) * w, 0.0)
        s = ls_s[:, t]
        protection = protection + np.where(s != -1, s.astype(np.float64) * w, 0.0)
    f[:, 7] = threat
    f[:, 8] = protection

    # _calculate_hand_quality: the first four rows of plane 6 = (card id, cost, strength, movement)
    playable = np.zeros(n, dtype=np.int64)
    valid = np.zeros(n, dtype=np.int64)
    total_value = np.zeros(n)
    for i in range(4):
        cid, cost, strength = o[:, 6, 4 * i], o[:, 6, 4 * i + 1], o[:, 6, 4 * i + 2]
        ok = (cid != -1) & (cid != HAND_SENTINEL)
        strength = np.where(strength != -1, strength, 0)   # a spell's strength -1 counts as 0
        valid += ok
        has = ok & (cost > 0)
        value = np.divide(strength.astype(np.float64), cost.astype(np.float64), out=np.zeros(n), where=has)
        total_value = total_value + np.where(has, value, 0.0)
        playable += has & (cost.astype(np.float64) <= mana)
    vf = np.maximum(valid, 1).astype(np.float64)
    playability = playable.astype(np.float64) / vf
    avg = total_value / vf
    nv = np.clip(avg / 3.0, 0.0, 1.0)
    f[:, 9] = np.where(valid == 0, 0.0, (playability + nv) / 2.0)
    return f.reshape(lead + (10,))


def _zero_sum_sign(a, b, c):
    """IEEE round-to-nearest sign of an exactly zero a*b + c: -0.0 only when both the product and c are -0."""
    prod_neg = (math.copysign(1.0, a) * math.copysign(1.0, b)) < 0
    return -0.0 if (prod_neg and math.copysign(1.0, c) < 0) else 0.0


def fma_fraction(a, b, c):
    """a * b + c evaluated exactly as a Fraction and rounded once (the definition)."""
    p = Fraction(a) * Fraction(b)
    s = p + Fraction(c)
    if s == 0:
        return _zero_sum_sign(a, b, c) if (p == 0 and c == 0) else 0.0
    return float(s)   # numerator / denominator: Python's integer true division is correctly rounded


def fma(a, b, c):
    """The same as fma_fraction with the power-of-two denominators of float64 kept unreduced (no gcd): faster."""
    na, da = a.as_integer_ratio()
    nb, db = b.as_integer_ratio()
    nc, dc = c.as_integer_ratio()
    dp = da * db
    d = dp if dp >= dc else dc   # both are powers of two: the larger is the common denominator
    num = na * nb * (d // dp) + nc * (d // dc)
    if num == 0:
        return _zero_sum_sign(a, b, c) if (na == 0 or nb == 0) and nc == 0 else 0.0
    return num / d


def score(w, before, after, fma=fma):
    """HeuristicAgent.score_action from the two feature vectors: enemy - agent - resource penalty."""
    w = [float(x) for x in w]
    d = (np.asarray(after, dtype=np.float64) - np.asarray(before, dtype=np.float64)).tolist()
    agent = 0.0
    enemy = 0.0
    for i in range(10):
        agent = fma(w[i], d[i], agent)
        enemy = fma(w[i], -d[i], enemy)
    eff = d[0]
    penalty = abs(eff) * 0.2 if eff < -0.3 else 0.0
    return enemy - agent - penalty


def first_max(scores):
    """np.argmax over a list of floats without NaN: the index of the first maximum."""
    best = 0
    for i in range(1, len(scores)):
        if scores[i] > scores[best]:
            best = i
    return best


class ScoreCache:
    """score() memoised on the bit patterns of (weights, after - before), all it depends on: many candidates of a
    decision share a feature delta."""

    def __init__(self):
        self.memo = {}

    def __call__(self, w, before, after):
        w = np.asarray(w, dtype=np.float64)
        before = np.asarray(before, dtype=np.float64)
        after = np.asarray(after, dtype=np.float64)
        key = (w.tobytes(), (after - before).tobytes())
        r = self.memo.get(key)
        if r is None:
            r = self.memo[key] = score(w, before, after)
        return r
