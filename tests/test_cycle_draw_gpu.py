"""The weighted draw of a decision's REPLACE candidates (actions 148..151), which the hot kernel resolves once per decision
with the whole wavefront (monsoon_amd/csrc/coop_draw.h), against the serial draw of monsoon_step (k_step), on every
standard-record variant of the hot kernel.

States are made by patching blobs of monsoon_state_save and loading them with monsoon_state_load: deck sizes 0..12, ages
0 / 1 / mixed / one card at AGE_MAX - 1 (its weight is the whole sum) / a card at AGE_MAX (reweight faults, also from a
stale byte behind the list), single-use cards in hand next to ordinary ones, the stream cursor at the last two positions
of a block and at the end of the window, and samples u planted on the cdf boundaries a host computation gives (the
boundary itself and the multiples of 2^-53 on either side).  Every state is decided under several weight vectors.

For each state the fused decision (monsoon_decide) must give, bit for bit, the score a Python-level look-ahead computes for
each of 148..151 over a clone stepped by monsoon_step -- the pattern of
test_python_level_lookahead_on_clones_equals_the_fused_decision -- and the successor it commits must have the canonical
hash, record and fault code of the clone stepped with the same action."""
import math

import numpy as np
import pytest

import kernel_variants
from monsoon_amd.cards import deck_indices

pytestmark = pytest.mark.gpu

# record layout of the standard build (monsoon_amd/csrc/state.h) and of the blob (monsoon_hip.hip k_blob)
BLOB_META, BLOB_REC = 8, 40
META_RNG = BLOB_META + 16
H_TOPLAY, OFF_PL, PL_SIZE = 0, 80, 96
P_FLAGS, P_HAND_N, P_DECK_N, P_HAND, P_DECK, P_AGE = 7, 9, 10, 12, 32, 80
DECK_CAP, AGE_MAX, MT_N = 12, 255, 624
CF_SINGLE_USE = 1
REPLACE = (148, 149, 150, 151)

WTAB = [1.0]
for _ in range(AGE_MAX):
    WTAB.append(WTAB[-1] * 1.6 + 100)   # Player.reweight, two rounded operations


def _weights():
    rs = np.random.RandomState(77)
    w0 = np.random.RandomState(2024).uniform(0, 1, 10)
    e9 = np.zeros(10)
    e9[9] = 1.0
    return [w0, -w0, e9, -e9, rs.uniform(-1, 1, 10), rs.uniform(-1, 1, 10)]


class Blob:
    def __init__(self, raw):
        self.b = bytearray(raw)
        self.state_bytes = int.from_bytes(self.b[4:8], "little")
        self.rng_out = BLOB_REC + self.state_bytes + MT_N * 4

    def copy(self):
        return Blob(bytes(self.b))

    def mover(self):
        return self.b[BLOB_REC + H_TOPLAY]

    def pl(self, f):
        return BLOB_REC + OFF_PL + PL_SIZE * self.mover() + f

    def deck_n(self):
        return self.b[self.pl(P_DECK_N)]

    def hand_n(self):
        return self.b[self.pl(P_HAND_N)]

    def set_deck(self, n, ages):
        n0 = self.deck_n()
        for i in range(n0, n):   # further entries: copies of the cards that are there (of the hand where the deck is empty)
            src = self.pl(P_DECK + 4 * (i % n0)) if n0 else self.pl(P_HAND + 4 * (i % self.hand_n()))
            self.b[self.pl(P_DECK + 4 * i):self.pl(P_DECK + 4 * i) + 4] = self.b[src:src + 4]
        self.b[self.pl(P_DECK_N)] = n
        for i, a in enumerate(ages):
            self.b[self.pl(P_AGE + i)] = a

    def set_single_use(self, hand_index):
        self.b[self.pl(P_HAND + 4 * hand_index + 2)] |= CF_SINGLE_USE

    def set_cursor(self, pos, block=None):
        rng = int.from_bytes(self.b[META_RNG:META_RNG + 4], "little")
        blk = (rng >> 16) & 1 if block is None else block
        self.b[META_RNG:META_RNG + 4] = (pos | (blk << 16)).to_bytes(4, "little")

    def plant_u(self, m):
        """The next random_sample gives m / 2^53."""
        rng = int.from_bytes(self.b[META_RNG:META_RNG + 4], "little")
        pos, cur = rng & 0xffff, (rng >> 16) & 1
        for k, word in enumerate((((m >> 26) << 5) | 21, ((m & ((1 << 26) - 1)) << 6) | 42)):
            p = pos + k
            assert p < 2 * MT_N
            at = self.rng_out + 4 * ((cur * MT_N + p) if p < MT_N else ((cur ^ 1) * MT_N + p - MT_N))
            self.b[at:at + 4] = word.to_bytes(4, "little")

    def next_u(self):
        """What the next random_sample gives (rules.h rng_random_sample over the two resident blocks)."""
        rng = int.from_bytes(self.b[META_RNG:META_RNG + 4], "little")
        pos, cur = rng & 0xffff, (rng >> 16) & 1
        words = []
        for p in (pos, pos + 1):
            at = self.rng_out + 4 * ((cur * MT_N + p) if p < MT_N else ((cur ^ 1) * MT_N + p - MT_N))
            words.append(int.from_bytes(self.b[at:at + 4], "little"))
        return ((words[0] >> 5) * 67108864.0 + (words[1] >> 6)) / 9007199254740992.0

    def cdf(self, appended):
        """numpy's choice(deck, p=w / sum(w)) after Player.discard: sum() left to right, cumsum, division by the last."""
        ages = [self.b[self.pl(P_AGE + i)] for i in range(self.deck_n())]
        w = [WTAB[a + 1] for a in ages] + ([1.0] if appended else [])
        s = 0.0
        for x in w:
            s = s + x
        c = np.cumsum(np.array([x / s for x in w]))
        return list(c / c[-1])


def _base_states():
    """Blobs of positions in which the mover may replace a card."""
    from monsoon_amd.engine import BatchEngine
    deck = deck_indices("N12M")
    eng = BatchEngine(8)
    eng.reset(np.arange(8, dtype=np.uint32) + 500, np.stack([deck, deck]))
    w0 = _weights()[0]
    out = []
    for t in range(6):
        masks = eng.legal_mask()
        for i in range(8):
            if (int(masks[i][2]) >> (148 - 128)) & 1:
                bl = Blob(eng.save_state(i))
                if bl.hand_n() == 4 and bl.deck_n() >= 4:
                    out.append(bl)
        eng.decide(w0)
    eng.close()
    assert len(out) >= 8
    return out


def _states():
    base = _base_states()
    rs = np.random.RandomState(5)
    out, k = [], 0

    def nxt():
        nonlocal k
        k += 1
        return base[k % len(base)].copy()

    for n in range(DECK_CAP + 1):   # 12: the returned card finds the deck full
        patterns = {"zeros": [0] * n, "ones": [1] * n, "mixed": list(rs.randint(0, 60, n)),
                    "dominant": [int(a) for a in rs.randint(0, 8, n)], "fault": list(rs.randint(0, 60, n))}
        if n:
            patterns["dominant"][int(rs.randint(0, n))] = AGE_MAX - 1
            patterns["fault"][int(rs.randint(0, n))] = AGE_MAX
        for name, ages in patterns.items():
            s = nxt()
            s.set_deck(n, ages)
            out.append((f"n{n}-{name}", s))
    for n in (5, 6, 9):   # a stale AGE_MAX byte behind the list, inside / outside the last age word reweight tests
        s = nxt()
        s.set_deck(n, [3] * n + [AGE_MAX] * (DECK_CAP - n))
        out.append((f"n{n}-stale", s))
    for n in (0, 1, 2, 5, 8, 11, 12):
        for single in ((1,), (0, 3), (0, 1, 2, 3)):
            s = nxt()
            s.set_deck(n, list(rs.randint(0, 40, n)))
            for h in single:
                s.set_single_use(h)
            out.append((f"n{n}-single{single}", s))
    for pos in (MT_N - 2, MT_N - 1, 2 * MT_N - 2, 2 * MT_N - 1):
        for block in (0, 1):
            s = nxt()
            s.set_deck(7, list(rs.randint(0, 30, 7)))
            s.set_single_use(2)
            s.set_cursor(pos, block)
            out.append((f"cursor{pos}-block{block}", s))
    for n, ages, single in ((3, [0, 0, 0], ()), (8, list(rs.randint(0, 50, 8)), (1,)), (11, [2] * 5 + [AGE_MAX - 1] + [4] * 5, (0,)),
                            (6, [1, 1, 1, 1, 1, 1], (3,))):
        proto = nxt()
        proto.set_deck(n, ages)
        for h in single:
            proto.set_single_use(h)
        for appended in (True, False):
            for j, c in enumerate(proto.cdf(appended)):
                m0 = int(math.floor(math.ldexp(c, 53)))
                for dm in (-1, 0, 1):
                    m = min(max(m0 + dm, 0), (1 << 53) - 1)
                    for pos in ((40,) if dm else (40, MT_N - 1)):
                        s = proto.copy()
                        s.set_cursor(pos)
                        s.plant_u(m)
                        out.append((f"n{n}-cdf{'+' if appended else '-'}{j}{dm:+d}@{pos}", s))
    return out


def _load_all(eng, blobs):
    for i, bl in enumerate(blobs):
        eng.load_state(i, bytes(bl.b))


def _score(w, before, after):
    d = after - before
    agent, enemy = np.dot(w, d), np.dot(w, -d)
    eff = d[0]
    pen = abs(eff) * 0.2 if eff < -0.3 else 0.0
    return enemy - agent - pen


CASES = [(u, w) for u, w in kernel_variants.variants(False)]


@pytest.fixture(scope="module")
def reference():
    """The serial side, once for all variants: per state and REPLACE action the clone's fault, features and hash."""
    from monsoon_amd.engine import BatchEngine
    states = _states()
    blobs = [s for _, s in states]
    K = len(blobs)
    ser = BatchEngine(K)
    _load_all(ser, blobs)
    before = ser.features()
    _, before_raises = ser.observe()
    masks = ser.legal_mask()
    ser.close()
    ref = {}
    for a in REPLACE:
        legal = np.array([(int(masks[i][a >> 6]) >> (a & 63)) & 1 for i in range(K)], dtype=bool)
        c = BatchEngine(K)
        _load_all(c, blobs)
        _, _, fault = c.step(np.where(legal, a, 255).astype(np.uint8))
        after = c.features()
        _, raises = c.observe()
        ref[a] = dict(legal=legal, fault=fault.copy(), after=after, raises=raises.copy())
        # the serial side itself against numpy's definition, computed here: the card that arrived in the hand is the one
        # searchsorted(cdf, u, 'right') picks from the deck as Player.discard left it
        for k, bl in enumerate(blobs):
            if fault[k]:
                continue
            entry = bl.b[bl.pl(P_HAND + 4 * (a - 148)):bl.pl(P_HAND + 4 * (a - 148)) + 4]
            appended = not (entry[2] & CF_SINGLE_USE)
            deck = [bytes(bl.b[bl.pl(P_DECK + 4 * i):bl.pl(P_DECK + 4 * i) + 4]) for i in range(bl.deck_n())] + ([bytes(entry)] if appended else [])
            idx = int(np.searchsorted(np.array(bl.cdf(appended)), bl.next_u(), side="right"))
            got = Blob(c.save_state(k))
            assert got.hand_n() == 4 and bytes(got.b[got.pl(P_HAND + 12):got.pl(P_HAND + 16)]) == deck[idx], (states[k][0], a, idx)
        c.close()
    assert all(ref[a]["legal"].all() for a in REPLACE)   # four cards in hand, the replace not yet used
    return states, before, before_raises, ref


@pytest.mark.parametrize("u,w", CASES, ids=[f"{u}x{w}" for u, w in CASES])
def test_replace_candidates_equal_the_serial_draw(monkeypatch, reference, u, w):
    from monsoon_amd.engine import BatchEngine
    states, before, before_raises, ref = reference
    names = [n for n, _ in states]
    blobs = [s for _, s in states]
    K, W = len(blobs), _weights()
    J = len(W)
    kernel_variants.select(monkeypatch, u, w)
    fused = BatchEngine(K * J)
    assert fused.variant() == (u, w)
    monkeypatch.delenv("MONSOON_LANES")
    monkeypatch.delenv("MONSOON_WPE")
    clone = BatchEngine(K * J)
    many = [blobs[i // J] for i in range(K * J)]
    _load_all(fused, many)
    _load_all(clone, many)
    weights = np.stack([np.stack([W[i % J], W[i % J]]) for i in range(K * J)])
    action, _, scores = fused.decide(weights, want_scores=True)
    # the score of every REPLACE candidate
    bad = []
    for i in range(K * J):
        k, wv = i // J, W[i % J]
        for a in REPLACE:
            r = ref[a]
            if r["fault"][k] or before_raises[k] or r["raises"][k]:
                want = 0.0   # except Exception: return 0.0
            else:
                want = _score(wv, before[k], r["after"][k])
            got = scores[i, a]
            if np.float64(want).view(np.uint64) != np.float64(got).view(np.uint64):
                bad.append((names[k], i % J, a, want, got))
    assert not bad, bad[:10]
    # the committed successor: the clone stepped with the same action
    _, _, cfault = clone.step(action)
    ffault = fused.game_faults()
    hf, hc = fused.state_hash(), clone.state_hash()
    committed = {a: 0 for a in REPLACE}
    for i in range(K * J):
        k = i // J
        # monsoon_game_faults: the fault that stopped the game, else the first limit of the record (code >= 16) one of the
        # decision's look-aheads hit -- a full deck under another REPLACE candidate, say -- which the clone never stepped
        assert ffault[i] == cfault[i] or (not cfault[i] and ffault[i] >= 16), (names[k], i % J, int(action[i]), int(ffault[i]), int(cfault[i]))
        if not cfault[i]:
            assert hf[i] == hc[i], (names[k], i % J, int(action[i]))
            assert fused.export(i) == clone.export(i), (names[k], i % J, int(action[i]))
            if int(action[i]) in committed:
                committed[int(action[i])] += 1
    # the hash comparison must have seen REPLACE successors of every hand position
    assert all(v > 0 for v in committed.values()), committed
    fused.close()
    clone.close()
