"""Deck schedule of the GA: generate_random_deck and the three-phase DeckEvolutionConfig.

Mirrors /root/reference/utils.py:26-242 over card ids instead of card objects.  The reference draws from Python's
global `random` module (unseeded); here every draw goes through an injectable `random.Random`, so that a schedule is
reproducible.  With the same generator state the selections are the reference's own (same `sample` / `choices` /
`random` calls over the same lists in the same order), pinned by tests/golden/deck_schedule.json.

DeckEvolutionConfig(per_game=True) replaces the one sequential stream by a stream per game, so that a game's decks no
longer depend on what was drawn before it: see game_decks.  That form is what monsoon_draw_schedule draws on the device
(include/monsoon.h; csrc/deck_schedule.h).
"""
import random as _random

from .cards import CARD_IDS, CARD_META

NEUTRAL, WINTER, SWARM, IRONCLAD, SHADOWFEN = range(5)   # enums.py:44-49
FACTION_OF = {c["id"]: c["faction"] for c in CARD_META}

# stream tags of the per-game mode: which caller a game's decks are drawn for (never 0: the key keeps four words)
TAG_POPULATION, TAG_EXPERT = 1, 2
TAG_ENV = 3   # the vector env's episodes and EvolutionaryGame (VecEnv.reset(deck_schedule=...))


def available_cards(faction):
    """utils.py:63-88: every card class of the faction or NEUTRAL, in dir(cards) order (= sorted ids)."""
    return [c for c in CARD_IDS if FACTION_OF[c] in (faction, NEUTRAL)]


def generate_random_deck(faction, original=None, preserve_ratio=0.0, rng=_random):
    """utils.py:26-119.  `original`: list of card ids; returns 12 card ids (fewer only if the pool is empty)."""
    preserve_ratio = max(0.0, min(1.0, preserve_ratio))
    if original and preserve_ratio > 0.0:
        cards_to_preserve = min(int(12 * preserve_ratio), len(original), 12)
        if preserve_ratio == 1.0:
            preserved = list(original[:12])
            if len(preserved) < 12:
                cards_needed = 12 - len(preserved)
            else:
                return preserved
        else:
            preserved = rng.sample(list(original), cards_to_preserve)
            cards_needed = 12 - cards_to_preserve
    else:
        preserved = []
        cards_needed = 12
    if cards_needed > 0:
        pool = available_cards(faction)
        if not pool:
            return preserved
        if cards_needed > len(pool):
            selected = rng.choices(pool, k=cards_needed)   # not enough cards: duplicates allowed
        else:
            selected = rng.sample(pool, cards_needed)
        return preserved + selected
    return preserved


class DeckEvolutionConfig:
    """utils.py:121-242: exploit (archetypes) -> explore (growing share of random cards) -> balance (steady mix)."""

    def __init__(self, player1_archetype, player2_archetype, exploit_generations=30, explore_generations=30,
                 max_random_ratio=0.5, balance_archetype_ratio=0.7, seed=None, per_game=False):
        """per_game=True (needs a seed): every game draws from a stream of its own (game_decks) instead of the one
        sequential stream that get_deck_configuration advances."""
        if per_game and seed is None:
            raise ValueError("per_game=True needs a seed: a game's stream is keyed by it")
        self.player1_archetype = list(player1_archetype)
        self.player2_archetype = list(player2_archetype)
        self.exploit_generations = exploit_generations
        self.explore_generations = explore_generations
        self.max_random_ratio = max_random_ratio
        self.balance_archetype_ratio = balance_archetype_ratio
        self.player1_faction = FACTION_OF[self.player1_archetype[0]] if self.player1_archetype else NEUTRAL
        self.player2_faction = FACTION_OF[self.player2_archetype[0]] if self.player2_archetype else NEUTRAL
        self.rng = _random.Random(seed) if seed is not None else _random
        self.per_game = bool(per_game)
        self.seed32 = int(seed) & 0xFFFFFFFF if per_game else None

    def get_deck_configuration(self, generation, rng=None):
        """One deck pair from the schedule's sequential stream (rng: another generator to draw from instead)."""
        rng = self.rng if rng is None else rng
        if generation < self.exploit_generations:
            return list(self.player1_archetype), list(self.player2_archetype)
        if generation < self.exploit_generations + self.explore_generations:
            progress = (generation - self.exploit_generations) / self.explore_generations
            ratio = progress * self.max_random_ratio
            d1 = generate_random_deck(self.player1_faction, self.player1_archetype, 1.0 - ratio, rng)
            d2 = generate_random_deck(self.player2_faction, self.player2_archetype, 1.0 - ratio, rng)
            return d1, d2
        use1 = rng.random() < self.balance_archetype_ratio
        use2 = rng.random() < self.balance_archetype_ratio
        d1 = list(self.player1_archetype) if use1 else generate_random_deck(self.player1_faction, rng=rng)
        d2 = list(self.player2_archetype) if use2 else generate_random_deck(self.player2_faction, rng=rng)
        return d1, d2

    def game_decks(self, generation, game_seed, tag=TAG_POPULATION):
        """The specification of the per-game mode: the pair get_deck_configuration(generation) draws from
            random.Random(seed & 0xFFFFFFFF | generation << 32 | game_seed << 64 | tag << 96)
        (generation, game_seed < 2**32; tag 1 = evaluate_population, 2 = evaluate_vs_expert, never 0).  CPython seeds an int
        with init_by_array over its 32-bit words, here always [seed32, generation, game_seed, tag].  The pair depends on
        nothing else: not on the game's place in a schedule, the rank that draws it, or earlier draws."""
        if not self.per_game:
            raise ValueError("game_decks needs DeckEvolutionConfig(per_game=True)")
        generation, game_seed, tag = int(generation), int(game_seed), int(tag)
        if not (0 <= generation < 1 << 32 and 0 <= game_seed < 1 << 32 and 0 < tag < 1 << 32):
            raise ValueError("generation and game_seed must be below 2**32, tag in 1 .. 2**32 - 1")
        return self.get_deck_configuration(generation, _random.Random(self.seed32 | generation << 32 | game_seed << 64 | tag << 96))

    def schedule_params(self, generation, tag=TAG_POPULATION):
        """The fields of monsoon_deck_schedule for one generation's per-game draws, every float decision of the schedule
        already taken (the device sees integers and balance_archetype_ratio): dict(seed, generation, tag, phase (1 explore,
        2 balance), n_preserve, balance_archetype_ratio, archetype uint8[2][12], pool_n int32[2], pool uint8[2][128]), card
        indices with the pools in available_cards order.  None where the device entry does not apply and the host draw
        (game_decks) stays: the exploit phase (no draws), an archetype that is not 12 cards, a pool outside 12..128."""
        import numpy as np
        from .cards import CARD_INDEX
        if not self.per_game:
            raise ValueError("schedule_params needs DeckEvolutionConfig(per_game=True)")
        if self.is_static(generation) or len(self.player1_archetype) != 12 or len(self.player2_archetype) != 12:
            return None
        pools = [available_cards(self.player1_faction), available_cards(self.player2_faction)]
        if not all(12 <= len(p) <= 128 for p in pools):
            return None
        if generation < self.exploit_generations + self.explore_generations:
            # generate_random_deck's own arithmetic on preserve_ratio = 1.0 - ratio
            progress = (generation - self.exploit_generations) / self.explore_generations
            preserve = max(0.0, min(1.0, 1.0 - progress * self.max_random_ratio))
            phase, n_preserve = 1, 12 if preserve == 1.0 else min(int(12 * preserve), 12) if preserve > 0.0 else 0
        else:
            phase, n_preserve = 2, 0
        pool = np.zeros((2, 128), dtype=np.uint8)
        for side, p in enumerate(pools):
            pool[side, :len(p)] = [CARD_INDEX[c] for c in p]
        arch = np.array([[CARD_INDEX[c] for c in a] for a in (self.player1_archetype, self.player2_archetype)], dtype=np.uint8)
        return {"seed": self.seed32, "generation": int(generation), "tag": int(tag), "phase": phase, "n_preserve": n_preserve,
                "balance_archetype_ratio": float(self.balance_archetype_ratio), "archetype": arch,
                "pool_n": np.array([len(p) for p in pools], dtype=np.int32), "pool": pool}

    def env_schedule(self, generation):
        """The fields of monsoon_deck_schedule for the vector env (VecEnv.reset(deck_schedule=...), monsoon_env_set_schedule):
        schedule_params(generation, TAG_ENV), and in the exploit phase -- which the env needs for a curriculum that
        crosses phases -- phase 0 with the archetypes instead of None (the device reads no stream; n_preserve, pool_n and
        pool are ignored there and left zero).  ValueError where schedule_params returns None for another reason: an
        archetype that is not 12 cards, a pool outside 12..128."""
        import numpy as np
        from .cards import CARD_INDEX
        if not self.per_game:
            raise ValueError("env_schedule needs DeckEvolutionConfig(per_game=True)")
        if len(self.player1_archetype) != 12 or len(self.player2_archetype) != 12:
            raise ValueError("the device draws for archetypes of exactly 12 cards")
        if not self.is_static(generation):
            params = self.schedule_params(generation, TAG_ENV)
            if params is None:
                raise ValueError("the device draws from faction pools of 12..128 cards")
            return params
        arch = np.array([[CARD_INDEX[c] for c in a] for a in (self.player1_archetype, self.player2_archetype)], dtype=np.uint8)
        return {"seed": self.seed32, "generation": int(generation), "tag": TAG_ENV, "phase": 0, "n_preserve": 0,
                "balance_archetype_ratio": float(self.balance_archetype_ratio), "archetype": arch,
                "pool_n": np.zeros(2, dtype=np.int32), "pool": np.zeros((2, 128), dtype=np.uint8)}

    def is_static(self, generation):
        """True while every game of the generation gets the same pair (exploit phase)."""
        return generation < self.exploit_generations

    def get_phase_info(self, generation):
        if generation < self.exploit_generations:
            phase, ratio = "Exploit", 0.0
        elif generation < self.exploit_generations + self.explore_generations:
            phase = "Explore"
            ratio = (generation - self.exploit_generations) / self.explore_generations * self.max_random_ratio
        else:
            phase, ratio = "Balance", 1.0 - self.balance_archetype_ratio
        return {"phase": phase, "generation": generation, "random_ratio": ratio,
                "exploit_complete": generation >= self.exploit_generations,
                "explore_complete": generation >= self.exploit_generations + self.explore_generations}
