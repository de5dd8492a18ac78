"""The independent model of tests/heuristic_model.py against the reference's own rows, and against the CPU oracle at
scale (CPU only).  The oracle compiles the library's leaf headers (observe.inc), so the second half pins that shared
code to something that shares none of it."""
import os
import struct

import numpy as np
import pytest

import heuristic_model as HM
import oracle_lib
from monsoon_amd.cards import CARD_INDEX, FAULT_CARDS, UNSUPPORTED, observable_pool

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")

# fixture -> (record build, the reference's scripted bot plays both sides)
FEATURE_FIXTURES = {"trace_random_N12M.npz": (False, False), "trace_live_pool.npz": (False, False),
                    "trace_live_pool_ext.npz": (True, False), "trace_live_b005.npz": (True, False),
                    "trace_live_expert.npz": (False, True)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def replay_observations(g, ext, expert):
    """The fixture's games on the oracle with test_reference_live._replay's rules (a recorded expert action 255 ends
    the game; a capacity fault 16 / 22 / 23 of the extended record ends it early).  The oracle's observation after every
    step is first required to hash to the fixture's; returns (observations, fixture feature rows) of the steps reached."""
    orc = oracle_lib.Oracle(1, extended=ext, core="oracle")
    obs, rows = [], []
    faulted_before = 0
    for k in range(len(g["seeds"])):
        lo, hi = int(g["offsets"][k]), int(g["offsets"][k + 1])
        assert orc.reset(0, int(g["seeds"][k]), g["deck0"][k], g["deck1"][k]) == 0
        assert orc.canon_hash(0) == int(g["init_hash"][k]), k
        for t in range(lo, hi):
            a = int(g["action"][t])
            if expert:   # the bot's choice consumes the game's stream before the step
                b, fe = orc.expert_action(0)
                if a == 255:
                    break
                assert fe == 0 and a == b, (k, t)
            f, _, _ = orc.step(0, a)
            if g["fault"][k] and t == hi - 1:
                break
            if f != 0:
                assert ext and f in (16, 22, 23), (k, t, f)
                break
            assert orc.obs_hash(0) == int(g["obs"][t]), (k, t)   # the model reads the reference's own observation
            obs.append(orc.observe(0))
            rows.append(g["feat"][t - faulted_before])
        faulted_before += int(g["fault"][k])
    return np.array(obs), np.array(rows)


def test_model_equals_the_reference_feature_rows():
    """StateFeatures of the reference at every step of its recorded games (standard and extended records, random policy
    and the scripted bot): the model on the reference's observation gives the reference's row, bit for bit."""
    total, stored = 0, 0
    for name, (ext, expert) in FEATURE_FIXTURES.items():
        g = np.load(os.path.join(GOLD, name))
        obs, rows = replay_observations(g, ext, expert)
        got = HM.features(obs)
        bad = np.nonzero((_bits(got) != _bits(rows)).any(axis=1))[0]
        assert len(bad) == 0, (name, len(bad), obs[bad[0]].tolist(), rows[bad[0]], got[bad[0]])
        total += len(rows)
        stored += len(g["feat"])
        print(f"{name}: {len(rows)} of {len(g['feat'])} reference feature rows equal bit for bit")
    print(f"reference feature rows: {total} of {stored} compared")
    assert stored == 10985 and total >= 10900


def test_model_score_equals_the_reference_score_rows():
    """HeuristicAgent.score_action's arithmetic on 2 000 recorded (weights, before, after) rows of the reference (456 with
    the resource penalty): the model's sequential exact-fma chain gives the reference's score, bit for bit."""
    k = np.load(os.path.join(GOLD, "score_kat.npz"))
    got = np.array([HM.score(w, b, a) for w, b, a in zip(k["w"], k["before"], k["after"])])
    assert np.array_equal(_bits(got), _bits(k["score"]))
    pen = int(((k["after"][:, 0] - k["before"][:, 0]) < -0.3).sum())
    print(f"score rows: {len(got)} equal bit for bit ({pen} with the resource penalty)")
    assert len(got) == 2000 and pen == 456


def _f64(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def test_fast_fma_equals_the_fraction_definition():
    """heuristic_model.fma (unreduced power-of-two denominators) against the Fraction definition: the score rows' operands,
    subnormal and huge products, exact cancellation and every sign of zero."""
    k = np.load(os.path.join(GOLD, "score_kat.npz"))
    rs = np.random.RandomState(5)
    cases = []
    for w, b, a in zip(k["w"][:300], k["before"][:300], k["after"][:300]):
        d = a - b
        for i in range(10):
            cases.append((float(w[i]), float(d[i]), float(rs.choice([0.0, -0.0, d[(i + 1) % 10], w[i] * d[i]]))))
            cases.append((float(w[i]), float(-d[i]), float(-w[i] * -d[i])))
    zeros = [0.0, -0.0]
    for a in zeros + [1.5, -1.5]:
        for b in zeros + [2.0, -2.0]:
            for c in zeros + [-3.0, 3.0]:
                cases.append((a, b, c))
    for _ in range(3000):
        a = float(rs.uniform(-1, 1)) * 10.0 ** int(rs.randint(-320, 300))
        b = float(rs.uniform(-4, 4)) * 10.0 ** int(rs.randint(-20, 5))
        c = float(rs.choice([0.0, -0.0, _f64(int(rs.randint(1, 1 << 30))), float(rs.uniform(-1, 1)) * 1e-300, a * b]))
        cases.append((a, b, c))
        cases.append((a, b, -a * b))
    for a, b, c in cases:
        x, y = HM.fma(a, b, c), HM.fma_fraction(a, b, c)
        assert struct.pack("<d", x) == struct.pack("<d", y), (a, b, c, x, y)
    assert HM.fma(1e-300, -1e-300, 0.0) == 0.0 and struct.pack("<d", HM.fma(1e-300, -1e-300, 0.0)) == struct.pack("<d", -0.0)
    assert HM.fma(1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53, -1.0) == 2.0 ** -53 - 2.0 ** -105   # one rounding, not two
    print(f"fma cases: {len(cases)}")


def _random_policy_states(ext, n_games, min_states, seed, up_games):
    """Random-policy games on the oracle (pool decks of the record; the first up_games games also deal up01-03), the
    observation and the oracle's features after every step.  Returns (obs, oracle features, raising rows)."""
    pool = [int(c) for c in observable_pool()]
    if not ext:
        pool = [c for c in pool if c not in {CARD_INDEX[x] for x in UNSUPPORTED}]
    up = [CARD_INDEX[c] for c in sorted(FAULT_CARDS)]
    orc = oracle_lib.Oracle(1, extended=ext, core="oracle")
    rs = np.random.RandomState(seed)
    obs, feat = [], []
    raising = 0
    for k in range(n_games):
        if len(obs) >= min_states and k >= up_games:
            break
        d0 = rs.choice(pool, 12, replace=False)
        d1 = rs.choice(pool, 12, replace=False)
        if k < up_games:   # one up card in either deck: rows where the observation raises, and rows before it does
            d0[rs.randint(12)] = up[k % 3]
        if orc.reset(0, int(rs.randint(1 << 31)), d0, d1) != 0:
            continue
        for _ in range(300):
            acts = orc.legal_actions(0)
            if not acts:
                break
            f, _, done = orc.step(0, int(acts[rs.randint(len(acts))]))
            if f != 0:
                break
            o, x = orc.observe(0), orc.features(0)
            assert (o is None) == (x is None)
            if o is None:
                raising += 1
            else:
                obs.append(o)
                feat.append(x)
            if done or orc.have_winner(0):
                break
    return np.array(obs), np.array(feat), raising


@pytest.mark.parametrize("ext", [False, True, 2], ids=["standard", "extended", "large"])
def test_model_equals_the_oracle_on_random_policy_games(ext):
    """The oracle's features (the library's features() compiled for the CPU) against the model on >= 20 000 states of
    random-policy games on pool decks of each record, a few of them dealt up01-03."""
    obs, feat, raising = _random_policy_states(ext, 10000, 20000, 7100 + int(ext), up_games=12)
    got = HM.features(obs)
    bad = np.nonzero((_bits(got) != _bits(feat)).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), obs[bad[0]].tolist(), feat[bad[0]], got[bad[0]])
    print(f"record {ext}: {len(obs)} oracle states equal bit for bit ({raising} more whose observation raises)")
    assert len(obs) >= 20000 and raising > 0
