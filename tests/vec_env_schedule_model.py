"""Python model of the vector env's schedule mode (include/monsoon.h, monsoon_env_set_schedule) over the model of the env
contract (tests/vec_env_model.py), used unchanged (test helper).

Only the source of an episode's decks differs from the other modes: the pair that the schedule in force when the episode
starts draws for the episode's seed.  The specification is the stdlib: deck_schedule_cases.params_decks writes
get_deck_configuration's calls out over random.Random(seed | generation << 32 | episode seed << 64 | tag << 96); phase 0
is both archetypes.  `params` may be replaced between steps, as monsoon_env_set_schedule replaces the handle's.
"""
import numpy as np

from deck_schedule_cases import params_decks
from monsoon_amd.cards import CARD_INDEX, DECKS, UNSUPPORTED, deck_indices
from monsoon_amd.decks import IRONCLAD, SWARM, TAG_ENV, available_cards
from vec_env_model import VecEnvModel

FACTIONS = (IRONCLAD, SWARM)   # of the archetypes below: monsoon_amd/game.py FACTION has the same numbers


def schedule_decks(params, seed):
    """uint8[2][12]: the pair an episode that starts from `seed` plays under the schedule `params`."""
    if params["phase"] == 0:
        return np.array(params["archetype"], dtype=np.uint8).reshape(2, 12)
    return params_decks(params, seed)


def standard_schedule(phase, n_preserve=0, ratio=0.7, generation=0, seed=20240519):
    """A hand-made schedule the standard record build plays: the IRONCLAD and SWARM archetypes, each faction's pool
    (available_cards) without ua20 / b005, tag TAG_ENV."""
    pools = [[CARD_INDEX[c] for c in available_cards(f) if c not in UNSUPPORTED] for f in FACTIONS]
    pool = np.zeros((2, 128), dtype=np.uint8)
    for side, p in enumerate(pools):
        pool[side, :len(p)] = p
    return {"seed": seed & 0xFFFFFFFF, "generation": generation, "tag": TAG_ENV, "phase": phase, "n_preserve": n_preserve,
            "balance_archetype_ratio": float(ratio), "archetype": np.stack([deck_indices(DECKS["IRONCLAD"]), deck_indices(DECKS["SWARM"])]),
            "pool_n": np.array([len(p) for p in pools], dtype=np.int32), "pool": pool}


class ScheduleVecEnvModel(VecEnvModel):
    def __init__(self, seed0, params, **kw):
        self.params = params   # the schedule in force: a test assigns another one between steps
        self.drawn = {}        # j -> (the schedule, the seed) its current episode's decks were drawn with
        super().__init__(seed0, decks=np.zeros((2, 12), dtype=np.uint8), **kw)

    def _start(self, j):
        self.drawn[j] = (self.params, self.seed(j))
        self.reset_decks[j] = schedule_decks(self.params, self.seed(j))
        super()._start(j)
