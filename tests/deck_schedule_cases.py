"""Cases of the per-game deck schedule shared by tests/test_deck_schedule_cpu.py (the walk of csrc/deck_schedule.h on the
host) and tests/test_deck_schedule_gpu.py (monsoon_draw_schedule), with their expected pairs from Python's own
random.Random.  Test infrastructure only.

A case is (name, params, ref): params = the fields of monsoon_deck_schedule (DeckEvolutionConfig.schedule_params), ref(seed)
= the pair uint8[2][12] the stdlib draws for that game seed.  Schedule cases take ref from DeckEvolutionConfig.game_decks,
the specification; synthetic pools, which no faction has, from params_decks below (the same calls written out)."""
import functools
import random

import numpy as np

from monsoon_amd.cards import CARD_IDS, CARD_INDEX
from monsoon_amd.decks import FACTION_OF, IRONCLAD, NEUTRAL, DeckEvolutionConfig

EDGE_SEEDS = (0, 1, 0xFFFFFFFF)
S32 = (0, 0xFFFFFFFE)
EXPLORE_PRESERVE = (0, 3, 6, 7, 11, 12)   # 12 - n needed from a pool of 58 / 74: 5 or fewer = set path, 6 or more = pool path
BALANCE_RATIOS = (0.0, 0.7, 1.0)
SYNTHETIC = ((12, 12), (21, 5), (22, 5), (85, 12), (86, 12), (128, 12))   # (pool size, cards needed): both sides of setsize 21 / 85


def game_seeds(n, salt=0):
    """n game seeds: 0, 1 and 2**32 - 1 first, seeded random ones behind."""
    rest = np.random.RandomState(1000 + salt).randint(0, 1 << 32, size=max(n - 3, 0), dtype=np.uint64)
    return np.concatenate([np.array(EDGE_SEEDS, dtype=np.uint64), rest])[:n].astype(np.uint32)


def archetype(faction):
    """12 card ids whose first card has the faction (DeckEvolutionConfig takes the pool's faction from it)."""
    own = [c for c in CARD_IDS if FACTION_OF[c] == faction]
    return (own[:4] + [c for c in CARD_IDS if FACTION_OF[c] == NEUTRAL][5:40:3])[:12]


def params_decks(params, game_seed):
    """The draws of get_deck_configuration written out over the fields of monsoon_deck_schedule, by the stdlib."""
    rng = random.Random(int(params["seed"]) | int(params["generation"]) << 32 | int(game_seed) << 64 | int(params["tag"]) << 96)
    arch = [[int(c) for c in a] for a in params["archetype"]]
    pools = [[int(c) for c in params["pool"][s][:params["pool_n"][s]]] for s in (0, 1)]
    if params["phase"] == 1:
        k = params["n_preserve"]
        out = [arch[s] if k == 12 else rng.sample(arch[s], k) + rng.sample(pools[s], 12 - k) for s in (0, 1)]
    else:
        use = [rng.random() < params["balance_archetype_ratio"], rng.random() < params["balance_archetype_ratio"]]
        out = [arch[s] if use[s] else rng.sample(pools[s], 12) for s in (0, 1)]
    return np.array(out, dtype=np.uint8)


def _schedule_case(name, dc, generation, tag):
    params = dc.schedule_params(generation, tag)
    assert params is not None, name

    def ref(seed):
        d1, d2 = dc.game_decks(generation, seed, tag)
        return np.array([[CARD_INDEX[c] for c in d1], [CARD_INDEX[c] for c in d2]], dtype=np.uint8)
    return name, params, ref


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    sides = [(archetype(NEUTRAL), archetype(IRONCLAD)), (archetype(IRONCLAD), archetype(NEUTRAL))]   # pools of 58 and 74 cards
    for i, s32 in enumerate(S32):
        # 24 explore generations with max_random_ratio 1.0 reach every n_preserve wanted (generation 0: ratio 0.0, the archetype)
        dc = DeckEvolutionConfig(*sides[i], exploit_generations=0, explore_generations=24, max_random_ratio=1.0, seed=s32 + (1 << 32),
                                 per_game=True)
        by_preserve = {}
        for g in range(24):
            by_preserve.setdefault(dc.schedule_params(g)["n_preserve"], g)
        for k in EXPLORE_PRESERVE:
            out.append(_schedule_case(f"explore-s{i}-keep{k}", dc, by_preserve[k], 1 + (k & 1)))
        for ratio in BALANCE_RATIOS:
            db = DeckEvolutionConfig(*sides[i], exploit_generations=1, explore_generations=1, balance_archetype_ratio=ratio, seed=s32,
                                     per_game=True)
            out.append(_schedule_case(f"balance-s{i}-ratio{ratio}", db, 2 + 7 * i, 1 + i))
    base = out[0][1]
    for n, needed in SYNTHETIC:
        pool = np.zeros((2, 128), dtype=np.uint8)
        pool[0, :n] = [(5 + 37 * j) % 112 for j in range(n)]
        pool[1, :n] = pool[0, :n][::-1]
        params = dict(base, seed=S32[n & 1], generation=n, tag=2, phase=1, n_preserve=12 - needed, pool=pool, pool_n=np.array([n, n], dtype=np.int32))
        out.append((f"synthetic-{n}-{needed}", params, functools.partial(params_decks, params)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(case, n):
    """(game seeds uint32[n], pairs uint8[n][2][12]) of case number `case`: computed once, shared, read-only."""
    seeds = game_seeds(n, case)
    pairs = np.stack([cases()[case][2](int(s)) for s in seeds])
    seeds.setflags(write=False)
    pairs.setflags(write=False)
    return seeds, pairs
